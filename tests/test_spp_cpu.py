"""The SPP entry, node and lowering, and the YOLOv3-SPP and YOLOv3-tiny models, without a GPU:
exported symbols, shapes, describe lines, every refusal with the plan compared before and after,
the 2 GiB refusal of the host form, lower_graph with an Spp node, Plan.memory, the two models'
lowerings and validators, and the two-scale head's boxes and anchors.  (A finalized plan's refusal
needs a device: tests/test_gpu_spp.py.)"""
import ctypes

import numpy as np
import pytest

import dnn_hip
import multi_out_cases as MC
import residual_cases as RS
import route_cases as RC
import spp_cases as SC
import synth
import yolo_post
import yolo_weights
import yolov3
import yolov3_spp
import yolov3_tiny

lib = dnn_hip.mylib


def _sizes(*ks):
    return (ctypes.c_int * len(ks))(*ks)


def _plan(batch, h, w, c, fp16=False, latency=False):
    p = ctypes.c_void_p()
    assert lib.dnn_plan_create(batch, h, w, c, ctypes.byref(p)) == 0
    if fp16:
        assert lib.dnn_plan_set_precision(p, 1) == 0
    if latency:
        assert lib.dnn_plan_set_latency_mode(p, 1) == 0
    return p


def _state(p):
    b, h, w, c = (ctypes.c_int() for _ in range(4))
    assert lib.dnn_plan_output_shape(p, ctypes.byref(b), ctypes.byref(h), ctypes.byref(w), ctypes.byref(c)) == 0
    buf = ctypes.create_string_buffer(16384)
    assert lib.dnn_plan_describe(p, buf, 16384) == 0
    wb, sb = ctypes.c_size_t(), ctypes.c_size_t()
    assert lib.dnn_plan_memory(p, ctypes.byref(wb), ctypes.byref(sb)) == 0
    return (h.value, w.value, c.value), buf.value.decode().splitlines(), wb.value, sb.value, lib.dnn_plan_num_kernels(p)


def _conv(p, k, od):
    assert lib.dnn_plan_add_conv(p, k, k, od, 1, 1, 1, None, None, None, None, None, 0.0, 0) == 0, dnn_hip.last_error()


def test_both_libraries_export_the_spp_symbols_and_python_mirrors_the_header():
    for name in ("libdnn_hip.so", "libdnn_hip_avx.so"):
        other = dnn_hip.load_library(name)
        for sym in ("dnn_plan_add_spp", "dnn_spp_host"):
            assert hasattr(other, sym), f"{name} does not export {sym}"
    import os
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include",
                               "dnn_hip_plan.h")).read()
    assert f"#define DNN_SPP_MAX_SIZES {dnn_hip.MAX_SPP_SIZES}\n" in header
    assert f"#define DNN_SPP_MAX_K {dnn_hip.MAX_SPP_K}\n" in header
    assert (dnn_hip.MAX_SPP_SIZES, dnn_hip.MAX_SPP_K) == (3, 13)


@pytest.mark.parametrize("latency", [False, True], ids=["batch", "latency"])
def test_add_spp_shape_describe_kernel_and_memory(latency):
    B = 2
    p = _plan(B, 13, 13, 3, latency=latency)
    q = _plan(B, 13, 13, 3, latency=latency)
    try:
        _conv(p, 3, 32)
        _conv(q, 3, 32)
        assert lib.dnn_plan_add_spp(p, 3, _sizes(13, 9, 5), 0) == 0, dnn_hip.last_error()
        shape, lines, _, _, _ = _state(p)
        assert shape == (13, 13, 128)
        assert lines[-1] == "spp 13x13x32 -> 13x13x128 sizes=13,9,5 x=last"
        _conv(p, 1, 16)
        _conv(q, 1, 16)
        shape, lines, wb, sb, nk = _state(p)
        assert shape == (13, 13, 16) and lines[-1].startswith("conv 13x13x128 -> 13x13x16 ")
        # the peepholes stop at the entry: the conv before it is what it is in the plain chain
        _, qlines, _, qsb, qnk = _state(q)
        assert lines[0] == qlines[0] and nk == qnk + 1
        # one kernel, 0 flops, (n_sizes + 2) tensors of bytes
        name = ctypes.create_string_buffer(64)
        fl, by = ctypes.c_double(), ctypes.c_double()
        infos = []
        for i in range(nk):
            assert lib.dnn_plan_kernel_info(p, i, name, 64, ctypes.byref(fl), ctypes.byref(by)) == 0
            infos.append((name.value.decode(), fl.value, by.value))
        spp = [k for k in infos if k[0].startswith("spp")]
        assert spp == [("spp0", 0.0, 5.0 * B * 13 * 13 * 32 * 4)]
        # memory: the activation buffers grow to the SPP output, the largest tensor of the plan
        assert sb > qsb and sb >= 2 * B * 13 * 13 * 128 * 4
        # x first, a single size, a repeated size
        assert lib.dnn_plan_add_spp(p, 1, _sizes(3), 1) == 0
        assert _state(p)[1][-1] == "spp 13x13x16 -> 13x13x32 sizes=3 x=first"
        assert lib.dnn_plan_add_spp(p, 2, _sizes(5, 5), 0) == 0
        assert _state(p)[1][-1] == "spp 13x13x32 -> 13x13x96 sizes=5,5 x=last"
        assert [k for k in _kernel_names(p) if k.startswith("spp")] == ["spp0", "spp1", "spp2"]
    finally:
        lib.dnn_plan_destroy(p)
        lib.dnn_plan_destroy(q)


def _kernel_names(p):
    name = ctypes.create_string_buffer(64)
    out = []
    for i in range(lib.dnn_plan_num_kernels(p)):
        assert lib.dnn_plan_kernel_info(p, i, name, 64, None, None) == 0
        out.append(name.value.decode())
    return out


def test_spp_as_the_first_entry_reads_the_plans_input():
    p = _plan(1, 19, 19, 12)
    try:
        assert lib.dnn_plan_add_spp(p, 3, _sizes(5, 9, 13), 1) == 0
        shape, lines, _, _, nk = _state(p)
        assert shape == (19, 19, 48) and lines == ["spp 19x19x12 -> 19x19x48 sizes=5,9,13 x=first"] and nk == 1
    finally:
        lib.dnn_plan_destroy(p)


def test_every_refusal_leaves_the_plan_unchanged():
    p = _plan(2, 13, 13, 8)
    try:
        _conv(p, 3, 16)
        before = _state(p)

        def refused(rc, word=None):
            assert rc != 0 and dnn_hip.last_error() != ""
            if word:
                assert word in dnn_hip.last_error(), dnn_hip.last_error()
            assert _state(p) == before

        refused(lib.dnn_plan_add_spp(p, 0, _sizes(5), 0), "n_sizes")
        refused(lib.dnn_plan_add_spp(p, 4, _sizes(5, 7, 9, 11), 0), "n_sizes")
        refused(lib.dnn_plan_add_spp(p, -1, _sizes(5), 0), "n_sizes")
        refused(lib.dnn_plan_add_spp(p, 3, None, 0), "NULL")
        for bad in (4, 12, 1, 15, 0, -5, 2):  # even, below 3, above 13
            refused(lib.dnn_plan_add_spp(p, 1, _sizes(bad), 0), str(bad))
            refused(lib.dnn_plan_add_spp(p, 3, _sizes(13, 9, bad), 0), str(bad))
        assert lib.dnn_plan_add_spp(None, 1, _sizes(5), 0) != 0
        # and a good call still works afterwards
        assert lib.dnn_plan_add_spp(p, 3, _sizes(13, 9, 5), 0) == 0
        assert _state(p)[0] == (13, 13, 64)
    finally:
        lib.dnn_plan_destroy(p)


def test_fp16_plans_refuse_the_entry_and_say_so():
    p = _plan(2, 13, 13, 8, fp16=True)
    try:
        _conv(p, 3, 16)
        before = _state(p)
        assert lib.dnn_plan_add_spp(p, 3, _sizes(13, 9, 5), 0) != 0
        assert "fp16" in dnn_hip.last_error()
        assert _state(p) == before
    finally:
        lib.dnn_plan_destroy(p)


def test_spp_host_refuses_from_its_arguments_alone():
    tiny = np.zeros(16, np.float32)
    v = dnn_hip._vp
    # [1, 8192, 8192, 2] is 512 MiB: with three sizes the output is 2 GiB
    assert lib.dnn_spp_host(v(tiny), v(tiny), 1, 8192, 8192, 2, 3, _sizes(13, 9, 5), 0) != 0
    assert "2 GiB" in dnn_hip.last_error()
    assert lib.dnn_spp_host(v(tiny), v(tiny), 2, 16384, 16384, 4, 1, _sizes(3), 0) != 0
    assert "2 GiB" in dnn_hip.last_error()
    for n_sizes, sizes in ((0, _sizes(5)), (4, _sizes(3, 5, 7, 9)), (1, _sizes(4)), (1, _sizes(15)), (2, _sizes(5, 1))):
        assert lib.dnn_spp_host(v(tiny), v(tiny), 1, 2, 2, 4, n_sizes, sizes, 0) != 0 and dnn_hip.last_error() != ""
    assert lib.dnn_spp_host(v(tiny), v(tiny), 1, 2, 2, 4, 1, None, 0) != 0
    assert lib.dnn_spp_host(None, v(tiny), 1, 2, 2, 4, 1, _sizes(5), 0) != 0
    assert lib.dnn_spp_host(v(tiny), v(tiny), 1, 0, 2, 4, 1, _sizes(5), 0) != 0


def test_spp_node_shapes_names_and_value_errors():
    g = dnn_hip.DnnGraphBuilder()
    x = g.create_input([2, 13, 13, 8])
    s = g.create_spp(x, (13, 9, 5))
    assert s.name == "spp_0" and s.result.shape == (2, 13, 13, 32) and s.ksizes == (13, 9, 5) and not s.x_first
    t = g.create_spp(s, [5], x_first=True)
    assert t.name == "spp_1" and t.result.shape == (2, 13, 13, 64) and t.x_first
    assert g.successors(x) == [s] and g.predecessors(t) == [s]
    for bad in ((), (5, 7, 9, 11), (4,), (15,), (1,), (5, 6), (5.5,), 5, None, (True,)):
        with pytest.raises(ValueError):
            g.create_spp(x, bad)
    flat = dnn_hip.Input("flat", (4, 4))
    flat.result = np.zeros((4, 4), np.float32)
    with pytest.raises(ValueError):
        dnn_hip.Spp("bad", flat, (5,))
    assert g.successors(x) == [s]  # a refused node adds no edge


def test_concat_still_takes_exactly_two_inputs():
    g = dnn_hip.DnnGraphBuilder()
    x = g.create_input([1, 4, 4, 8])
    with pytest.raises(ValueError):
        g.create_concat([x, x, x])


def test_lowering_covers_the_spp_node_once():
    ws = RC.exact_weights(SC.CHAIN_LAYERS, seed=5)
    g = SC.chain_graph(2, ws)
    entries = dnn_hip.lower_graph(g)
    assert SC.entry_kinds(entries) == "CYC"
    e = entries[1]
    assert isinstance(e, dnn_hip.SppEntry) and e.ksizes == (13, 9, 5) and not e.x_first
    spp_nodes = [n for n in RC.topo_nodes(g) if isinstance(n, dnn_hip.Spp)]
    assert len(spp_nodes) == 1 and e.nodes == spp_nodes
    covered = [n for en in entries for n in en.nodes]
    assert len(covered) == len(set(map(id, covered))) == len(RC.topo_nodes(g)) - 1  # every node but the Input, once
    for name, (layers, build, kinds) in SC.PLAN_CASES.items():
        es = dnn_hip.lower_graph(build(2, RC.exact_weights(layers, seed=5)))
        assert es is not None and SC.entry_kinds(es) == kinds, name
    with pytest.raises(ValueError):
        dnn_hip.SppEntry((4,))


def test_plan_memory_from_entries_with_an_spp():
    B = 2
    ws = RC.exact_weights(SC.CHAIN_LAYERS, seed=5)
    entries = dnn_hip.lower_graph(SC.chain_graph(B, ws))
    wb, sb = dnn_hip.Plan.memory(B, SC.IN_SHAPE, entries)
    p = _plan(B, *SC.IN_SHAPE)
    try:
        _conv(p, 3, 32)
        assert lib.dnn_plan_add_spp(p, 3, _sizes(13, 9, 5), 0) == 0
        _conv(p, 1, 8)
        _, _, wb2, sb2, _ = _state(p)
    finally:
        lib.dnn_plan_destroy(p)
    assert (wb, sb) == (wb2, sb2)
    assert sb >= 2 * B * 8 * 8 * 128 * 4  # two activation buffers of the SPP output
    # an SPP whose output is tapped lives in a region of its own size
    tapped = dnn_hip.lower_graph(SC.tap_graph(B, RC.exact_weights(SC.TAP_LAYERS, seed=5)))
    plain = [e for e in tapped if not isinstance(e, dnn_hip.TapEntry)]
    assert dnn_hip.Plan.memory(B, SC.IN_SHAPE, tapped)[1] - dnn_hip.Plan.memory(B, SC.IN_SHAPE, plain)[1] \
        == B * 8 * 8 * 96 * 4


# ------------------------------------------------------------------------------ YOLOv3-SPP
def test_yolov3_spp_lowers_to_one_plan():
    ws = synth.yolov3_spp_weights(width_div=8, n_out=24)
    assert len(ws) == yolov3_spp.N_LAYERS == 76
    w = yolov3_spp.validate(ws, 24)
    g, nodes, outs = yolov3_spp.build_graph(dnn_hip.DnnGraphBuilder, w, in_shape=(1, 96, 96, 3))
    assert [o.result.shape for o in outs] == [(1, 3, 3, 24), (1, 6, 6, 24), (1, 12, 12, 24)]
    entries = dnn_hip.lower_graph(g)
    assert entries is not None
    kinds = SC.entry_kinds(entries)
    assert kinds.count("C") == 76 and kinds.count("Y") == 1 and kinds.count("T") == 2
    assert kinds.count("J") == 2 and kinds.count("U") == 2 and kinds.count("A") == 23
    assert SC.max_live_slots(entries) <= 3
    spp = [e for e in entries if isinstance(e, dnn_hip.SppEntry)][0]
    assert spp.ksizes == (13, 9, 5) and not spp.x_first
    # the entries around the SPP block: the neck's third conv in front, the 1x1 on 4 x the width behind
    i = entries.index(spp)
    assert entries[i - 1].conv.kernel.shape == (1, 1, 128, 64) and entries[i + 1].conv.kernel.shape == (1, 1, 256, 64)
    # YOLOv3 itself lowers as before: the same graph without the block and its conv
    g3, _, _ = yolov3.build_graph(dnn_hip.DnnGraphBuilder, yolov3.validate(synth.yolov3_weights(width_div=8, n_out=24)),
                                  in_shape=(1, 96, 96, 3))
    k3 = SC.entry_kinds(dnn_hip.lower_graph(g3))
    assert "Y" not in k3 and kinds.replace("YC", "", 1) == k3
    # the trunk's weights are YOLOv3's
    w3 = synth.yolov3_weights(width_div=8, n_out=24)
    assert all(np.array_equal(a["kernel"], b["kernel"]) for a, b in zip(ws[:52], w3[:52]))
    wb, sb = dnn_hip.Plan.memory(1, (96, 96, 3), entries)
    assert wb > 0 and sb > 0


def test_yolov3_spp_validate_refuses_wrong_structures():
    ws = synth.yolov3_spp_weights(width_div=8, n_out=24)
    E = yolo_weights.WeightFileError
    with pytest.raises(E):
        yolov3_spp.validate(ws[:-1])
    with pytest.raises(E):
        yolov3_spp.validate(synth.yolov3_weights(width_div=8, n_out=24))  # YOLOv3's 75 layers
    with pytest.raises(E, match="needs 27"):
        yolov3_spp.validate(ws, 27)
    bad = list(ws)  # the conv after the SPP block must read 4 x the width
    bad[55] = synth.layer_weights(55, 64, 64, k=1)
    with pytest.raises(E, match="layer 55"):
        yolov3_spp.validate(bad)
    bad = list(ws)  # a 3x3 where the neck has a 1x1
    bad[54] = synth.layer_weights(54, 128, 64, k=3)
    with pytest.raises(E, match="layer 54"):
        yolov3_spp.validate(bad)
    bad = list(ws)
    bad[60] = {k: v for k, v in ws[60].items() if k != "biases"}
    with pytest.raises(E, match="layer 60"):
        yolov3_spp.validate(bad)
    with pytest.raises(ValueError):
        yolov3_spp.YOLO_V3_SPP([1, 100, 96, 3], ws, False)
    # yolov3's public constants are what they were
    assert (yolov3.N_LAYERS, yolov3.N_SCALE, yolov3.N_TRUNK, yolov3.STRIDES) == (75, 7, 52, (32, 16, 8))


# ------------------------------------------------------------------------------ YOLOv3-tiny
TINY_KINDS = "C P C P C P C P C S P C P C C S C C T R X C U J X C C".replace(" ", "")


def test_yolov3_tiny_lowers_to_the_quoted_entries_and_validates():
    ws = synth.yolov3_tiny_weights(width_div=4, n_out=24)
    assert len(ws) == yolov3_tiny.N_LAYERS == 13
    w = yolov3_tiny.validate(ws, 24)
    g, nodes, outs = yolov3_tiny.build_graph(dnn_hip.DnnGraphBuilder, w, in_shape=(2, 96, 96, 3))
    assert [o.result.shape for o in outs] == [(2, 3, 3, 24), (2, 6, 6, 24)]
    assert g.extra_out_nodes == [outs[0]] and g.is_out_node(outs[1])
    entries = dnn_hip.lower_graph(g)
    assert entries is not None and SC.entry_kinds(entries) == TINY_KINDS
    assert MC.max_live_slots(entries) == 2
    assert MC.numbers(entries) == [("S", 0), ("S", 1), ("T", 0), ("R", 1), ("X", 1), ("J", 0), ("X", 0)]
    pools = [e.pool for e in entries if isinstance(e, dnn_hip.PoolEntry)]
    assert [tuple(p.strides[1:3]) for p in pools] == [(2, 2)] * 5 + [(1, 1)]
    # the stride-1 pool pads bottom / right only, as Darknet does there
    assert (pools[5].pad_top, pools[5].pad_bottom, pools[5].pad_left, pools[5].pad_right) == (0, 1, 0, 1)
    assert pools[5].result.shape == (2, 3, 3, 128)
    # full width at 416: the public shapes
    full = synth.YOLOV3_TINY_CONVS
    assert [c for c, _ in full] == [16, 32, 64, 128, 256, 512, 1024, 256, 512, None, 128, 256, None]
    assert ws[11]["kernel"].shape == (3, 3, 32 + 64, 64)  # the conv after the concat: 128 + 256 at full width
    E = yolo_weights.WeightFileError
    with pytest.raises(E):
        yolov3_tiny.validate(ws[:-1])
    with pytest.raises(E, match="needs 27"):
        yolov3_tiny.validate(ws, 27)
    bad = list(ws)  # the conv after the concat must read the reduce conv's and conv 4's channels
    bad[11] = synth.layer_weights(11, 32, 64, k=3)
    with pytest.raises(E, match="layer 11"):
        yolov3_tiny.validate(bad)
    bad = list(ws)  # head 0 reads y, not the 1024 conv
    bad[8] = synth.layer_weights(8, 256, 128, k=3)
    with pytest.raises(E, match="layer 8"):
        yolov3_tiny.validate(bad)
    bad = list(ws)
    bad[7] = synth.layer_weights(7, 256, 64, k=3)
    with pytest.raises(E, match="layer 7"):
        yolov3_tiny.validate(bad)
    with pytest.raises(ValueError):
        yolov3_tiny.YOLO_V3_TINY([1, 96, 100, 3], ws, False)


def test_multihead_yolov3_tiny_boxes_grids_and_exact_anchors():
    head = yolo_post.MultiHead.yolov3_tiny(416, 416)
    assert head.boxes == 2535 and head.scale_boxes == [507, 2028]
    assert [(s.grid_h, s.grid_w) for s in head.scales] == [(13, 13), (26, 26)]
    assert head.class_mode == "logistic" and head.n_classes == 80 and head.n_out == [255, 255]
    px = ((81, 82, 135, 169, 344, 319), (10, 14, 23, 27, 37, 58))
    for s, want in zip(head.scales, px):
        assert s.n_anchors == 3 and s.cell in (32.0, 16.0)
        a = np.asarray(s.anchors, np.float32)
        assert np.array_equal(a.astype(np.float64), np.asarray(s.anchors))  # the anchors are fp32 numbers
        assert np.array_equal(a * np.float32(s.cell), np.asarray(want, np.float32))  # anchor x cell is exact
    assert [s.cell for s in head.scales] == [32.0, 16.0]
    with pytest.raises(ValueError):
        yolo_post.MultiHead.yolov3_tiny(400, 416)
    named = yolo_post.MultiHead.yolov3_tiny(96, 64, classes=("a", "b", "c"))
    assert named.names == ("a", "b", "c") and named.n_out == [24, 24] and named.pred_shapes == [(3, 2, 24), (6, 4, 24)]
    # YOLOv3's own head is what it was
    assert yolo_post.MultiHead.yolov3(416, 416).boxes == 10647
