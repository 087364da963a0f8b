"""Darknet import without a GPU: cfg parsing, weight files, the lowering of imported models against
the hand-written ones, the padded conv entry's argument checks, the max pool rule and the head."""
import collections
import ctypes

import numpy as np
import pytest

import darknet_cases as DC
import darknet_import as D
import dnn_hip
import synth
import yolo_post
import yolov3
import yolov3_tiny

lib = dnn_hip.mylib


def _counts(model):
    return collections.Counter(s["type"] for s in D.parse_cfg(D.cfg_text(model)))


# ------------------------------------------------------------------------------------ cfg parsing
def test_public_cfgs_have_the_public_section_counts():
    c = _counts("yolov3")
    assert (c["convolutional"], c["shortcut"], c["route"], c["upsample"], c["yolo"], c["net"]) == (75, 23, 4, 2, 3, 1)
    assert c["maxpool"] == 0
    c = _counts("yolov3-spp")
    assert (c["convolutional"], c["shortcut"], c["upsample"], c["yolo"], c["maxpool"]) == (76, 23, 2, 3, 3)
    secs = D.parse_cfg(D.cfg_text("yolov3-spp"))[1:]
    at = [i for i, s in enumerate(secs) if s["type"] == "route" and s["layers"] == "-1,-3,-5,-6"]
    assert len(at) == 1  # the SPP pattern: pools 5, 9, 13 of one tensor, concatenated as 13, 9, 5, x
    i = at[0]
    assert [(s["type"], s.get("size"), s.get("layers")) for s in secs[i - 5:i]] == [
        ("maxpool", "5", None), ("route", None, "-2"), ("maxpool", "9", None), ("route", None, "-4"),
        ("maxpool", "13", None)]
    c = _counts("yolov3-tiny")
    assert (c["convolutional"], c["maxpool"], c["yolo"], c["route"], c["upsample"]) == (13, 6, 2, 2, 1)
    # the public shapes at 416: three heads of 255 channels on 13, 26 and 52 cells
    secs = D.parse_cfg(D.cfg_text("yolov3"))
    shapes = D.layer_shapes(secs)
    assert [shapes[i] for i, s in enumerate(secs[1:]) if s["type"] == "yolo"] == [(13, 13, 255), (26, 26, 255),
                                                                                 (52, 52, 255)]
    assert [s["layers"] for s in secs if s["type"] == "route"] == ["-4", "-1, 61", "-4", "-1, 36"]
    assert D.net_shape(secs) == (416, 416, 3) and D.net_shape(secs, [2, 320, 608, 3]) == (320, 608, 3)
    # width_div divides every channel count but the heads'
    narrow = D.conv_shapes(D.parse_cfg(D.cfg_text("yolov3", classes=3, width_div=8)))
    full = D.conv_shapes(secs)
    assert [n for n, _, _, bn in narrow if not bn] == [24] * 3 and [n for n, _, _, bn in full if not bn] == [255] * 3
    assert all(a[0] * 8 == b[0] for a, b in zip(narrow, full) if a[3])
    with pytest.raises(ValueError):
        D.cfg_text("yolov4")


def test_parse_cfg_comments_whitespace_and_unknown_keys():
    text = ("# a comment\n\n  [net]  \n width = 32 \nheight=32\n; another comment\nchannels=3\nsome_future_key = 7\n"
            "\n[convolutional]\n  filters = 24\nsize=1\n stride=1\npad=1\nactivation = linear\nfancy=1\n\n"
            "[yolo]\nmask = 0,1,2\nanchors = 1,2, 3,4, 5,6\nclasses=3\n")
    secs = D.parse_cfg(text)
    assert [s["type"] for s in secs] == ["net", "convolutional", "yolo"]
    assert [s["line"] for s in secs] == [3, 10, 18]
    assert secs[0]["width"] == "32" and secs[0]["some_future_key"] == "7" and secs[1]["activation"] == "linear"
    assert D.conv_params(secs[1]) == (24, 1, 1, 0, False, "linear")
    assert D.layer_shapes(secs) == [(32, 32, 24), (32, 32, 24)]


def _cfg(*sections):
    return "[net]\nwidth=32\nheight=32\nchannels=3\n" + "".join(sections)


CONV = "[convolutional]\nbatch_normalize=1\nfilters=8\nsize=3\nstride=1\npad=1\nactivation=leaky\n"


def test_cfg_errors_name_what_is_wrong():
    with pytest.raises(D.DarknetError, match=r"line 6.*\[reorg\]"):
        D.parse_cfg(_cfg("\n[reorg]\nstride=2\n"))
    with pytest.raises(D.DarknetError, match="starts with a .net."):
        D.parse_cfg("[convolutional]\nfilters=1\n")
    with pytest.raises(D.DarknetError, match="activation 'mish'"):
        D.layer_shapes(D.parse_cfg(_cfg(CONV.replace("leaky", "mish"))))
    with pytest.raises(D.DarknetError, match="from -3"):
        D.layer_shapes(D.parse_cfg(_cfg(CONV, CONV, "[shortcut]\nfrom=-3\nactivation=linear\n")))
    with pytest.raises(D.DarknetError, match="from 2"):  # itself
        D.layer_shapes(D.parse_cfg(_cfg(CONV, CONV, "[shortcut]\nfrom=2\nactivation=linear\n")))
    with pytest.raises(D.DarknetError, match="activation 'leaky'"):
        D.layer_shapes(D.parse_cfg(_cfg(CONV, CONV, "[shortcut]\nfrom=-2\nactivation=leaky\n")))
    with pytest.raises(D.DarknetError, match="layers 7"):
        D.layer_shapes(D.parse_cfg(_cfg(CONV, "[route]\nlayers=-1, 7\n")))
    with pytest.raises(D.DarknetError, match="3 layers"):
        D.layer_shapes(D.parse_cfg(_cfg(CONV, CONV, CONV, "[route]\nlayers=-1,-2,-3\n")))
    with pytest.raises(D.DarknetError, match="not a list of integers"):
        D.layer_shapes(D.parse_cfg(_cfg(CONV, "[route]\nlayers=-1, x\n")))
    with pytest.raises(D.DarknetError, match="grouped"):
        D.layer_shapes(D.parse_cfg(_cfg(CONV + "groups=2\n")))
    # a four-layer route that is not an SPP block
    text = _cfg(CONV, CONV, CONV, CONV, "[route]\nlayers=-1,-2,-3,-4\n",
                "[convolutional]\nfilters=24\nsize=1\nactivation=linear\n", "[yolo]\nmask=0,1,2\nanchors=1,2,3,4,5,6\nclasses=3\n")
    secs = D.parse_cfg(text)
    with pytest.raises(D.DarknetError, match="SPP block"):
        D.build_graph(dnn_hip.DnnGraphBuilder, secs, DC.darknet_layers(secs), [1, 32, 32, 3])


def test_heads_chained_on_the_main_line_and_the_limit_of_four():
    head = "[convolutional]\nfilters=24\nsize=1\nactivation=linear\n[yolo]\nmask=0,1,2\nanchors=1,2,3,4,5,6\nclasses=3\n"
    secs = D.parse_cfg(_cfg(head * 2))
    m = D.DarknetModel(_cfg(head * 2), DC.darknet_layers(secs), in_shape=[2, 32, 32, 3])
    kinds = [type(e).__name__ for e in dnn_hip.lower_graph(m.g)]
    assert kinds == ["PaddedConvEntry", "TapEntry", "PaddedConvEntry"] and len(m.head.scales) == 2
    secs = D.parse_cfg(_cfg(head * 5))
    with pytest.raises(D.DarknetError, match="5 .yolo. sections: at most 4"):
        D.build_graph(dnn_hip.DnnGraphBuilder, secs, DC.darknet_layers(secs), [1, 32, 32, 3])
    with pytest.raises(D.DarknetError, match="must end the cfg"):
        secs = D.parse_cfg(_cfg(head, CONV.replace("filters=8", "filters=8\n")))
        D.build_graph(dnn_hip.DnnGraphBuilder, secs, DC.darknet_layers(secs), [1, 32, 32, 3])


# -------------------------------------------------------------------------------- weight files
def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert sorted(x) == sorted(y)
        for k in x:
            assert x[k].dtype == np.float32 and x[k].shape == y[k].shape
            assert np.array_equal(x[k].view(np.int32), np.ascontiguousarray(y[k]).view(np.int32)), k


@pytest.mark.parametrize("model", ["yolov3-tiny", "yolov3"])
@pytest.mark.parametrize("minor", [1, 2])
def test_weights_round_trip_bit_equal(tmp_path, model, minor):
    secs = D.parse_cfg(DC.narrow_cfg(model))
    layers = DC.darknet_layers(secs)
    path = str(tmp_path / "w.weights")
    D.save_weights(path, layers, minor=minor, revision=5, seen=123456)
    floats = sum(a.size for l in layers for a in l.values())
    with open(path, "rb") as f:
        data = f.read()
    assert len(data) == 12 + (8 if minor == 2 else 4) + 4 * floats  # seen is 8 bytes from version 0.2 on
    back = D.load_weights(path, secs)
    assert (back.major, back.minor, back.revision, back.seen) == (0, minor, 5, 123456)
    _same(back, layers)
    assert [("scales" in l) for l in back] == [bn for _, _, _, bn in D.conv_shapes(secs)]


def test_weight_files_short_long_and_empty(tmp_path):
    secs = D.parse_cfg(DC.narrow_cfg("yolov3-tiny"))
    layers = DC.darknet_layers(secs)
    good = str(tmp_path / "good.weights")
    D.save_weights(good, layers)
    with open(good, "rb") as f:
        data = f.read()
    cases = {"short": data[:-4], "long": data + b"\0\0\0\0", "empty": b"", "header": data[:14]}
    for name, blob in cases.items():
        p = str(tmp_path / f"{name}.weights")
        with open(p, "wb") as f:
            f.write(blob)
        with pytest.raises(D.DarknetError):
            D.load_weights(p, secs)
    with pytest.raises(D.DarknetError, match="ends inside the weights of convolutional layer 12"):
        D.load_weights(str(tmp_path / "short.weights"), secs)
    with pytest.raises(D.DarknetError, match="4 bytes left"):
        D.load_weights(str(tmp_path / "long.weights"), secs)
    # partial: the whole layers the file holds; trailing bytes ignored
    part = D.load_weights(str(tmp_path / "short.weights"), secs, partial=True)
    _same(part, layers[:12])
    _same(D.load_weights(str(tmp_path / "long.weights"), secs, partial=True), layers)
    # weights that do not fit the cfg
    with pytest.raises(D.DarknetError):
        D.check_layers(secs, layers[:-1])
    bad = list(layers)
    bad[3] = dict(bad[3], weights=bad[3]["weights"][:, :1])
    with pytest.raises(D.DarknetError, match="layer 3"):
        D.check_layers(secs, bad)


def test_hwio_transpose_on_an_index_encoding_kernel():
    n, c, kh, kw = 5, 3, 3, 3
    idx = np.indices((n, c, kh, kw))
    w = (idx[0] * 1000 + idx[1] * 100 + idx[2] * 10 + idx[3]).astype(np.float32)  # entry = its (n, c, kh, kw)
    k = D.kernel_hwio({"weights": w})
    assert k.shape == (kh, kw, c, n) and k.flags["C_CONTIGUOUS"]
    for a in range(kh):
        for b in range(kw):
            for i in range(c):
                for o in range(n):
                    assert k[a, b, i, o] == o * 1000 + i * 100 + a * 10 + b


def test_batchnorm_fold_is_darknets_inference_form():
    layer = {"biases": np.float32([0.5, -1.0, 2.0]), "scales": np.float32([2.0, -3.0, 0.0]),
             "rolling_mean": np.float32([1.0, 0.25, -4.0]), "rolling_variance": np.float32([4.0, 0.25, 1.0]),
             "weights": np.zeros((3, 1, 1, 1), np.float32)}
    scale, shift = D.fold_batchnorm(layer)
    assert scale.dtype == shift.dtype == np.float32
    alpha = np.float64([2.0 / (2.0 + 1e-6), -3.0 / (0.5 + 1e-6), 0.0])  # sqrt(var) + eps, not sqrt(var + eps)
    assert np.array_equal(scale, alpha.astype(np.float32))
    assert np.array_equal(shift, (np.float64([0.5, -1.0, 2.0]) - np.float64([1.0, 0.25, -4.0]) * alpha).astype(np.float32))
    scale, shift = D.fold_batchnorm({"biases": layer["biases"], "weights": layer["weights"]})
    assert np.array_equal(scale, np.ones(3, np.float32)) and np.array_equal(shift, layer["biases"])


# ------------------------------------------------------------------------------------ lowering
def _imported(model, B, size, latency=False):
    secs = D.parse_cfg(DC.narrow_cfg(model, size))
    g, outs, yolos = D.build_graph(dnn_hip.DnnGraphBuilder, secs, DC.darknet_layers(secs), [B, size, size, 3])
    entries = dnn_hip.lower_graph(g)
    assert entries is not None
    return entries, dnn_hip.Plan.lowering(B, (size, size, 3), entries, latency=latency)


@pytest.mark.parametrize("latency", [False, True], ids=["batch", "latency"])
def test_imported_tiny_lowers_like_the_hand_written_model(latency):
    B, size = 2, 96
    entries, text = _imported("yolov3-tiny", B, size, latency)
    ws = synth.yolov3_tiny_weights(width_div=DC.NARROW["yolov3-tiny"][0], n_out=24)
    g, _, _ = yolov3_tiny.build_graph(dnn_hip.DnnGraphBuilder, yolov3_tiny.validate(ws, 24), in_shape=(B, size, size, 3))
    hand = dnn_hip.Plan.lowering(B, (size, size, 3), dnn_hip.lower_graph(g), latency=latency)
    assert DC.conv_lines(text) == hand.splitlines()
    convs = [l for l in text.splitlines() if l.startswith("conv ")]
    assert len(convs) == 13 and all(l.endswith(" affine") for l in convs)
    assert sum(isinstance(e, dnn_hip.PaddedConvEntry) for e in entries) == 13
    assert all(e.leaky in (0, 2) and e.affine is not None for e in entries if isinstance(e, dnn_hip.PaddedConvEntry))


@pytest.mark.parametrize("model", ["yolov3", "yolov3-spp"])
def test_imported_yolov3_lowers_like_the_hand_written_model_but_for_five_pads(model):
    import yolov3_spp
    B, size = 1, 96
    _, text = _imported(model, B, size)
    mod, make = (yolov3, synth.yolov3_weights) if model == "yolov3" else (yolov3_spp, synth.yolov3_spp_weights)
    g, _, _ = mod.build_graph(dnn_hip.DnnGraphBuilder, mod.validate(make(width_div=8, n_out=24), 24),
                              in_shape=(B, size, size, 3))
    hand = dnn_hip.Plan.lowering(B, (size, size, 3), dnn_hip.lower_graph(g))
    assert DC.conv_lines(text) == hand.splitlines()  # kinds, shapes and execution modes
    s2 = [l for l in text.splitlines() if l.startswith("conv ") and " s2 " in l]
    assert len(s2) == 5 and all(l.endswith(" pad=1,1 affine") for l in s2)  # Darknet's pads where SAME's are 0
    assert sum(l.startswith("spp ") for l in text.splitlines()) == (1 if model == "yolov3-spp" else 0)


def _padded(p, kh, kw, od, s, ph, pw, scale=None, shift=None, leaky=0):
    return lib.dnn_plan_add_conv_padded(p, kh, kw, od, s, s, ph, pw, None, scale, shift, leaky)


def _new_plan(*shape, fp16=False):
    p = ctypes.c_void_p()
    assert lib.dnn_plan_create(*shape, ctypes.byref(p)) == 0
    if fp16:
        assert lib.dnn_plan_set_precision(p, 1) == 0
    return p


def _describe(p):
    buf = ctypes.create_string_buffer(8192)
    assert lib.dnn_plan_describe(p, buf, 8192) == 0
    return buf.value.decode()


@pytest.mark.parametrize("size", [8, 7])
def test_describe_shows_darknet_pads_and_the_halved_output(size):
    p = _new_plan(2, size, size, 32)
    try:
        assert _padded(p, 3, 3, 64, 2, 1, 1) == 0
        line = _describe(p).strip()
        assert line.startswith(f"conv {size}x{size}x32 -> 4x4x64 k3x3 s2 ") and line.endswith(" pad=1,1")
        one = np.ones(64, np.float32)
        assert _padded(p, 1, 1, 64, 1, 0, 0, dnn_hip._vp(one), dnn_hip._vp(one), 2) == 0
        assert _describe(p).splitlines()[1].endswith(" pad=0,0 affine")
        # dnn_plan_add_conv's lines are what they were
        assert lib.dnn_plan_add_conv(p, 3, 3, 64, 1, 1, 1, None, None, None, None, None, 0.0, 0) == 0
        assert " pad=" not in _describe(p).splitlines()[2]
    finally:
        lib.dnn_plan_destroy(p)


def test_padded_entry_refuses_bad_arguments_and_leaves_the_plan_unchanged():
    one = np.ones(8, np.float32)
    v = dnn_hip._vp(one)
    p = _new_plan(1, 8, 8, 32)
    try:
        assert _padded(p, 3, 3, 8, 1, 1, 1, v, v, 2) == 0
        before = _describe(p)
        for args, msg in (((3, 3, 8, 1, 3, 1), "pads 3,1"), ((3, 3, 8, 1, 1, 3), "pads 1,3"), ((3, 3, 8, 1, -1, 0), "pads"),
                          ((3, 3, 8, 0, 1, 1), "bad args"), ((3, 3, 0, 1, 1, 1), "bad args")):
            assert _padded(p, *args) != 0 and msg in dnn_hip.last_error(), args
            assert _describe(p) == before
        assert _padded(p, 11, 11, 8, 1, 0, 0) != 0 and "empty output" in dnn_hip.last_error()  # 8 + 0 < 11
        assert _padded(p, 3, 3, 8, 1, 1, 1, v, None, 0) != 0 and "both set or both NULL" in dnn_hip.last_error()
        assert _padded(p, 3, 3, 8, 1, 1, 1, None, v, 0) != 0 and "both set or both NULL" in dnn_hip.last_error()
        assert _padded(p, 3, 3, 8, 1, 1, 1, v, v, 3) != 0 and "leaky" in dnn_hip.last_error()
        assert _describe(p) == before
        out = [ctypes.c_int() for _ in range(4)]
        assert lib.dnn_plan_output_shape(p, *map(ctypes.byref, out)) == 0 and [o.value for o in out] == [1, 8, 8, 8]
    finally:
        lib.dnn_plan_destroy(p)
    p = _new_plan(1, 8, 8, 32, fp16=True)
    try:
        assert _padded(p, 3, 3, 8, 1, 1, 1) != 0 and "fp32 plans only" in dnn_hip.last_error()
        assert _describe(p) == ""
    finally:
        lib.dnn_plan_destroy(p)


# ----------------------------------------------------------------------------------- graph API
def test_graph_nodes_validate_and_lower():
    g = dnn_hip.DnnGraphBuilder()
    x = g.create_input([1, 8, 8, 4])
    k = np.ones((3, 3, 4, 6), np.float32)
    for pads in ((3, 1), (1, 3), (-1, 0), (1,), (0.5, 1)):
        with pytest.raises(ValueError):
            g.create_conv2d_padded(x, k, [1, 1, 1, 1], pads)
    with pytest.raises(ValueError):
        g.create_conv2d_padded(x, np.ones((3, 3, 5, 6), np.float32), [1, 1, 1, 1], (1, 1))
    t = g.create_conv2d_padded(x, k, [1, 2, 2, 1], (1, 1))
    assert t.result.shape == (1, 4, 4, 6) and t.pads == (1, 1)
    with pytest.raises(ValueError):
        g.create_scale_shift(t, np.ones(5), np.ones(6))
    # the padding string of create_conv2d is what it was
    with pytest.raises(ValueError):
        g.create_conv2d(x, k, [1, 1, 1, 1], (1, 1))
    # a ScaleShift that does not follow a conv is refused with a clear error
    g2 = dnn_hip.DnnGraphBuilder()
    x2 = g2.create_input([1, 8, 8, 4])
    p = g2.create_max_pool2d(x2, [1, 2, 2, 1], [1, 2, 2, 1], "SAME")
    g2.set_out_node(g2.create_scale_shift(p, np.ones(4), np.ones(4)))
    with pytest.raises(dnn_hip.DnnHipError, match="ScaleShift exists in a plan only as the epilogue of the conv"):
        dnn_hip.lower_graph(g2)
    # ... and one after a SAME conv whose pads differ front and back
    g3 = dnn_hip.DnnGraphBuilder()
    x3 = g3.create_input([1, 8, 8, 4])
    c3 = g3.create_conv2d(x3, k, [1, 2, 2, 1], "SAME")
    g3.set_out_node(g3.create_scale_shift(c3, np.ones(6), np.ones(6)))
    with pytest.raises(dnn_hip.DnnHipError, match="ScaleShift"):
        dnn_hip.lower_graph(g3)
    # conv -> ScaleShift -> leaky is ONE entry, for the padded conv and for a symmetric SAME conv
    for make in (lambda gg, xx: gg.create_conv2d_padded(xx, k, [1, 1, 1, 1], (1, 1)),
                 lambda gg, xx: gg.create_conv2d(xx, k, [1, 1, 1, 1], "SAME")):
        for f32 in (True, False):
            gg = dnn_hip.DnnGraphBuilder()
            xx = gg.create_input([1, 8, 8, 4])
            t = gg.create_scale_shift(make(gg, xx), np.ones(6), np.ones(6))
            gg.set_out_node(gg.create_leaky_relu_f32(t) if f32 else gg.create_leaky_relu(t))
            es = dnn_hip.lower_graph(gg)
            assert len(es) == 1 and isinstance(es[0], dnn_hip.PaddedConvEntry)
            assert es[0].pads == (1, 1) and es[0].leaky == (2 if f32 else None) and len(es[0].nodes) == 3


# -------------------------------------------------------------------------------- max pool rule
@pytest.mark.parametrize("n", [12, 13])
@pytest.mark.parametrize("size,stride", [(2, 2), (2, 1), (5, 1), (9, 1), (13, 1)])
def test_maxpool_rule_accepts_what_the_same_pool_computes(size, stride, n):
    sec = {"type": "maxpool", "line": 1, "size": str(size), "stride": str(stride)}
    assert D.maxpool_params(sec, n, n) == (size, stride)
    # and the SAME pool there is Darknet's pool, value for value
    import darknet_oracle as DO
    import ref_numpy as R
    x = np.random.default_rng(size * 100 + n).standard_normal((1, n, n, 2)).astype(np.float32)
    assert np.array_equal(DO.maxpool_layer(x, sec), R.max_pool2d(x, [1, size, size, 1], [1, stride, stride, 1], "SAME"))


def test_maxpool_rule_refuses_3_2_on_an_even_map():
    sec = {"type": "maxpool", "line": 9, "size": "3", "stride": "2"}
    with pytest.raises(D.DarknetError, match="3/2 max pool on a map of 12 is not supported"):
        D.maxpool_params(sec, 12, 12)
    with pytest.raises(D.DarknetError, match="padding = 0"):
        D.maxpool_params(dict(sec, size="2", padding="0"), 12, 12)


# ----------------------------------------------------------------------------------------- head
def test_head_from_the_cfg_is_the_library_yolov3_head():
    secs = D.parse_cfg(D.cfg_text("yolov3"))
    shapes = D.layer_shapes(secs)
    yolos = [dict(s, grid=shapes[i][:2]) for i, s in enumerate(secs[1:]) if s["type"] == "yolo"]
    got = D.multi_head(yolos, 416, 416)
    want = yolo_post.MultiHead.yolov3(416, 416, nms="per_class", labels="multi", score_thr=0.5, iou_thr=0.45)
    assert got.scales == want.scales  # grids, anchors / stride, cell, classes, thresholds, field for field
    for f in ("class_mode", "nms", "labels", "n_classes", "score_thr", "iou_thr", "boxes", "scale_boxes", "max_det",
              "n_out", "pred_shapes", "pred_floats"):
        assert getattr(got, f) == getattr(want, f), f
    assert bytes(got.c) == bytes(want.c)
    tiny = D.parse_cfg(D.cfg_text("yolov3-tiny"))
    ts = D.layer_shapes(tiny)
    ty = [dict(s, grid=ts[i][:2]) for i, s in enumerate(tiny[1:]) if s["type"] == "yolo"]
    assert D.multi_head(ty, 416, 416).scales == yolo_post.MultiHead.yolov3_tiny(
        416, 416, nms="per_class", labels="multi", score_thr=0.5, iou_thr=0.45).scales
    # 608 x 608: 22,743 boxes, above the decode's limit
    big = D.layer_shapes(secs, [1, 608, 608, 3])
    by = [dict(s, grid=big[i][:2]) for i, s in enumerate(secs[1:]) if s["type"] == "yolo"]
    with pytest.raises(ValueError, match="22743 boxes"):
        D.multi_head(by, 608, 608)


def test_model_above_the_box_limit_is_built_without_a_head():
    """608 x 608 YOLOv3 has 22,743 boxes, more than the decode takes: the model is built with
    head=None and detect / postprocessing raise the decode's error (no device is touched)."""
    cfg = D.cfg_text("yolov3", classes=3, width=608, height=608, width_div=8)
    secs = D.parse_cfg(cfg)
    m = D.DarknetModel(cfg, DC.darknet_layers(secs))
    assert m.in_shape == (1, 608, 608, 3) and m.head is None
    assert [tuple(o.result.shape) for o in m.outs] == [(1, 19, 19, 24), (1, 38, 38, 24), (1, 76, 76, 24)]
    with pytest.raises(ValueError, match="22743 boxes"):
        m.detect(np.zeros((1, 608, 608, 3), np.float32))
    with pytest.raises(ValueError, match="22743 boxes"):
        m.postprocessing([np.zeros(o.result.shape, np.float32) for o in m.outs])
    # at 416 the same cfg gets Darknet's detector defaults, all overridable
    m = D.DarknetModel(cfg, DC.darknet_layers(secs), in_shape=[2, 416, 416, 3])
    assert (m.head.score_thr, m.head.iou_thr, m.head.nms, m.head.labels, m.head.class_mode) == \
        (0.5, 0.45, "per_class", "multi", "logistic")
    m = D.DarknetModel(cfg, DC.darknet_layers(secs), in_shape=[2, 416, 416, 3], score_thr=0.25, nms="any",
                       labels="argmax")
    assert (m.head.score_thr, m.head.nms, m.head.labels) == (0.25, "any", "argmax")
    with pytest.raises(ValueError, match="does not fit the outputs"):
        D.DarknetModel(cfg, DC.darknet_layers(secs), in_shape=[2, 416, 416, 3], head=yolo_post.MultiHead.yolov3(416, 416))
