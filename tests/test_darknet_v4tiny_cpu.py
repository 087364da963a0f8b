"""CPU: the Darknet import of YOLOv4-tiny without a device: the public cfg, the channel-group
[route] and its errors, the [yolo] keys (scale_x_y, new_coords, nms_kind), weight files, and the
lowering of the CSP topology (slot release in nested forks; arrival plus a new long skip) within the
plan's slots, with the hand-written YOLOv2 graph lowered exactly as before."""
import collections

import numpy as np
import pytest

import darknet_import as D
import darknet_v4_oracle as V4O
import dnn_hip
import synth
import v4tiny_cases as VK


def _sections(**kw):
    return D.parse_cfg(D.cfg_text("yolov4-tiny", **kw))


# ------------------------------------------------------------------------------ the public cfg
def test_stock_cfg_section_counts_and_shapes():
    secs = _sections()
    kinds = collections.Counter(s["type"] for s in secs[1:])
    assert kinds == {"convolutional": 21, "route": 11, "maxpool": 3, "upsample": 1, "yolo": 2} and len(secs) - 1 == 38
    shapes = D.layer_shapes(secs, [1, 416, 416, 3])
    yolo_at = [k for k, s in enumerate(secs[1:]) if s["type"] == "yolo"]
    assert yolo_at == [30, 37] and [shapes[k] for k in yolo_at] == [(13, 13, 255), (26, 26, 255)]
    assert [secs[1 + k]["mask"] for k in yolo_at] == ["3,4,5", "1,2,3"]
    for k in yolo_at:
        y = secs[1 + k]
        assert [float(v) for v in y["anchors"].split(",")] == [10, 14, 23, 27, 37, 58, 81, 82, 135, 169, 344, 319]
        assert float(y["scale_x_y"]) == 1.05 and y["nms_kind"] == "greedynms" and y["classes"] == "80"
    # the CSP blocks: a group route takes the second half of A; layer 23 is the third block's D and the lateral
    groups = [(k, s) for k, s in enumerate(secs[1:]) if s["type"] == "route" and "groups" in s]
    assert [k for k, _ in groups] == [3, 11, 19] and all((s["groups"], s["group_id"]) == ("2", "1") for _, s in groups)
    assert [shapes[k] for k in (2, 3, 4, 5, 6, 7, 8, 9)] == [(104, 104, 64), (104, 104, 32), (104, 104, 32), (104, 104, 32),
                                                           (104, 104, 64), (104, 104, 64), (104, 104, 128), (52, 52, 128)]
    assert shapes[23] == (26, 26, 256) and secs[1 + 34]["layers"].replace(" ", "") == "-1,23" and shapes[34] == (26, 26, 384)
    assert shapes[26] == (13, 13, 512) and secs[1 + 31]["layers"] == "-4"
    assert "yolov4-tiny" in D.MODELS
    with pytest.raises(ValueError):
        D.cfg_text("yolov4")


def test_width_div_divides_every_width_but_the_heads():
    wide, narrow = _sections(classes=3), _sections(classes=3, width_div=4)
    for (n, c, size, bn), (n4, c4, size4, bn4) in zip(D.conv_shapes(wide), D.conv_shapes(narrow)):
        assert (size, bn) == (size4, bn4)
        assert n4 == (n // 4 if bn else 24) and (bn or n == 24)  # the two linear heads keep 3 x (5 + 3)
        assert c4 == (c // 4 if c != 3 else 3)
    assert [s for s in D.layer_shapes(D.parse_cfg(VK.narrow_cfg()), [2, 64, 96, 3]) if s[2] == 24][::2] == [(2, 3, 24), (4, 6, 24)]


# ------------------------------------------------------------------------------ group routes
def _cfg_with(route_lines, filters=6):
    return "\n".join(["[net]", "width=8", "height=8", "channels=3", "", "[convolutional]", f"filters={filters}", "size=3", "pad=1",
                      "activation=leaky", "", "[convolutional]", "filters=4", "size=1", "activation=leaky", "",
                      "[route]"] + route_lines + ["", "[convolutional]", "filters=18", "size=1", "activation=linear", "",
                                                  "[yolo]", "mask=0,1", "anchors=1,2, 3,4", "classes=4"])


def test_group_route_shapes_follow():
    secs = D.parse_cfg(_cfg_with(["layers=-2", "groups=3", "group_id=2"]))
    assert D.layer_shapes(secs)[:3] == [(8, 8, 6), (8, 8, 4), (8, 8, 2)]
    assert D.conv_shapes(secs) == [(6, 3, 3, False), (4, 6, 1, False), (18, 2, 1, False)]
    secs = D.parse_cfg(_cfg_with(["layers=-1", "groups=1", "group_id=0"]))  # groups = 1: the tensor again
    assert D.layer_shapes(secs)[2] == (8, 8, 4)
    layers = [{"biases": np.zeros(n, np.float32), "weights": np.zeros((n, c, k, k), np.float32)}
              for n, c, k, _ in D.conv_shapes(secs)]
    g, _, _ = D.build_graph(dnn_hip.DnnGraphBuilder, secs, layers, [1, 8, 8, 3])
    assert not any(isinstance(e, dnn_hip.SliceEntry) for e in dnn_hip.lower_graph(g))


@pytest.mark.parametrize("lines,words", [
    (["layers=-2", "groups=4", "group_id=1"], ["line 17", "groups = 4", "does not divide", "6 channels"]),
    (["layers=-2", "groups=2", "group_id=2"], ["line 17", "group_id = 2", "0..1"]),
    (["layers=-2", "groups=2", "group_id=-1"], ["line 17", "group_id = -1"]),
    (["layers=-1,-2", "groups=2", "group_id=1"], ["line 17", "groups = 2", "2 layers"]),
    (["layers=-2", "groups=0"], ["line 17", "groups = 0"]),
])
def test_group_route_errors_name_the_line(lines, words):
    secs = D.parse_cfg(_cfg_with(lines))
    assert secs[3]["type"] == "route" and secs[3]["line"] == 17
    for fn in (D.layer_shapes, D.conv_shapes):
        with pytest.raises(D.DarknetError) as e:
            fn(secs)
        for w in words:
            assert w in str(e.value), (w, str(e.value))


def test_group_route_in_the_graph_and_the_oracle():
    secs = D.parse_cfg(_cfg_with(["layers=-1", "groups=2", "group_id=1"]))
    layers = VK.random_layers(secs)
    g, outs, _ = D.build_graph(dnn_hip.DnnGraphBuilder, secs, layers, [1, 8, 8, 3])
    entries = dnn_hip.lower_graph(g)
    sl = [e for e in entries if isinstance(e, dnn_hip.SliceEntry)]
    assert len(sl) == 1 and (sl[0].first, sl[0].channels) == (2, 2)
    # the oracle's route: the second half of the layer's channels
    t = np.arange(2 * 3 * 3 * 6, dtype=np.float32).reshape(2, 3, 3, 6)
    np.testing.assert_array_equal(V4O.route_layer(secs[3], [t]), t[..., 3:])
    np.testing.assert_array_equal(V4O.route_layer({"groups": "3", "group_id": "1"}, [t]), t[..., 2:4])
    np.testing.assert_array_equal(V4O.route_layer({"groups": "2", "group_id": "1"}, [t, t + 1]),
                                  np.concatenate([t[..., 3:], t[..., 3:] + 1], axis=3))


# ------------------------------------------------------------------------------ [yolo] keys
@pytest.mark.parametrize("line,words", [("new_coords=1", ["new_coords", "[yolo] at line"]),
                                        ("nms_kind=diounms", ["nms_kind", "diounms"])])
def test_refused_yolo_keys(line, words):
    cfg = VK.narrow_cfg().replace("nms_kind=greedynms\n", "") if line.startswith("nms_kind") else VK.narrow_cfg()
    cfg = cfg.replace("scale_x_y=1.05\n", "scale_x_y=1.05\n" + line + "\n")
    assert line in cfg
    secs = D.parse_cfg(cfg)
    with pytest.raises(D.DarknetError) as e:
        D.layer_shapes(secs)
    for w in words:
        assert w in str(e.value)
    with pytest.raises(D.DarknetError):
        D.DarknetModel(cfg, [])  # (raised before any weight is looked at)


def test_accepted_yolo_keys_and_the_head():
    for kind in ("nms_kind=default", "nms_kind=greedynms", "new_coords=0"):
        cfg = VK.narrow_cfg().replace("nms_kind=greedynms\n", "").replace("scale_x_y=1.05\n", "scale_x_y=1.05\n" + kind + "\n")
        D.layer_shapes(D.parse_cfg(cfg))
    secs = D.parse_cfg(VK.narrow_cfg())
    g, outs, yolos = D.build_graph(dnn_hip.DnnGraphBuilder, secs, VK.random_layers(secs), [VK.BATCH, VK.HEIGHT, VK.WIDTH, 3])
    head = D.multi_head(yolos, VK.HEIGHT, VK.WIDTH)
    assert head.scale_x_y == (1.05, 1.05) and head.xy is not None and "scale_x_y 1.05,1.05" in repr(head)
    assert [(s.grid_h, s.grid_w, s.cell) for s in head.scales] == [(2, 3, 32.0), (4, 6, 16.0)]
    assert head.scales[0].anchors == tuple(a / 32 for a in (81, 82, 135, 169, 344, 319))
    assert head.scales[1].anchors == tuple(a / 16 for a in (23, 27, 37, 58, 81, 82))  # mask 1,2,3
    wide = D.multi_head(yolos, VK.HEIGHT, VK.WIDTH, wide=True)
    assert type(wide).__name__ == "WideHead" and wide.scale_x_y == (1.05, 1.05)
    # every scale at 1: the head is built exactly as before
    plain = D.multi_head([dict(y, scale_x_y="1") for y in yolos], VK.HEIGHT, VK.WIDTH)
    assert plain.scale_x_y is None and plain.xy is None and "scale_x_y" not in repr(plain)
    mixed = D.multi_head([dict(yolos[0], scale_x_y="1.0"), yolos[1]], VK.HEIGHT, VK.WIDTH)
    assert mixed.scale_x_y == (1.0, 1.05)
    with pytest.raises(D.DarknetError, match="scale_x_y"):
        D.multi_head([dict(yolos[0], scale_x_y="0"), yolos[1]], VK.HEIGHT, VK.WIDTH)


def test_weight_file_round_trip_and_leftover_bytes(tmp_path):
    """The group route halves B's input channels: read against a cfg without the groups, the file does
    not match (as it did not while the importer ignored the key)."""
    secs = D.parse_cfg(VK.narrow_cfg())
    layers = VK.random_layers(secs)
    assert [l["weights"].shape[1] for l in layers[2:5]] == [16, 8, 8]  # A reads 16, B the second half of A's 16, C B's 8
    path = str(tmp_path / "v4tiny.weights")
    D.save_weights(path, layers)
    back = D.load_weights(path, secs)
    assert len(back) == 21
    for a, b in zip(back, layers):
        assert sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k]) for k in a)
    no_groups = D.parse_cfg(VK.narrow_cfg().replace("groups=2\n", "").replace("group_id=1\n", ""))
    with pytest.raises(D.DarknetError):
        D.load_weights(path, no_groups)


# ------------------------------------------------------------------------------ lowering
def _narrow_entries():
    secs = D.parse_cfg(VK.narrow_cfg())
    g, outs, _ = D.build_graph(dnn_hip.DnnGraphBuilder, secs, VK.random_layers(secs), [VK.BATCH, VK.HEIGHT, VK.WIDTH, 3])
    return g, dnn_hip.lower_graph(g)


def test_narrow_yolov4_tiny_lowers_within_the_slots():
    g, entries = _narrow_entries()
    assert entries is not None
    kinds = collections.Counter(type(e).__name__ for e in entries)
    assert kinds["SliceEntry"] == 3 and kinds["PaddedConvEntry"] == 21 and kinds["PoolEntry"] == 3
    assert kinds["UpsampleEntry"] == 1 and kinds["TapEntry"] == 1 and kinds["RouteEntry"] == 7
    assert [(e.first, e.channels) for e in entries if isinstance(e, dnn_hip.SliceEntry)] == [(8, 8), (16, 16), (32, 32)]
    most, live = VK.replay_slots(entries)
    assert most <= dnn_hip.MAX_SLOTS and most == 2
    assert live == set()  # every stash is released: nothing is kept to the end of the plan
    assert kinds["StashEntry"] == kinds["ReleaseEntry"] == 8
    # a CSP block: Stash(A), slice, B, Stash(B), C, Route [C, B], Release(B), D, Route [A, D], Release(A)
    names = [type(e).__name__ for e in entries]
    at = names.index("SliceEntry")
    assert [VK.entry_line(e).split(" k")[0] for e in entries[at - 1:at + 9]] == [
        "StashEntry slot=0", "SliceEntry first=8 channels=8", "PaddedConvEntry", "StashEntry slot=1", "PaddedConvEntry",
        "RouteEntry block=1 slot=1 slot_first=False", "ReleaseEntry slot=1", "PaddedConvEntry",
        "RouteEntry block=1 slot=0 slot_first=True", "ReleaseEntry slot=0"]
    # layer 23: arrival at [A, D] plus the new long skip into route -1,23: Stash(D), Route, Release
    third = [k for k, n in enumerate(names) if n == "SliceEntry"][2]
    tail = [VK.entry_line(e).split(" k")[0] for e in entries[third + 6:third + 10]]
    assert tail == ["PaddedConvEntry", "StashEntry slot=1", "RouteEntry block=1 slot=0 slot_first=True", "ReleaseEntry slot=0"]
    up = names.index("UpsampleEntry")
    assert [VK.entry_line(e) for e in entries[up + 1:up + 3]] == ["RouteEntry block=1 slot=1 slot_first=False",
                                                                 "ReleaseEntry slot=1"]
    # the plan's own walk agrees (dnn_plan_add_stash hands out the numbers the lowering expects)
    text = dnn_hip.Plan.lowering(VK.BATCH, (VK.HEIGHT, VK.WIDTH, 3), entries)
    assert sum(l.startswith("slice ") for l in text.splitlines()) == 3 and len(text.splitlines()) == len(entries)
    wb, sb = dnn_hip.Plan.memory(VK.BATCH, (VK.HEIGHT, VK.WIDTH, 3), entries)
    assert wb > 0 and sb > 0


def test_stock_width_yolov4_tiny_lowers_too():
    secs = _sections()
    layers = [{"biases": np.zeros(n, np.float32), "weights": np.zeros((n, c, k, k), np.float32),
               **({"scales": np.ones(n, np.float32), "rolling_mean": np.zeros(n, np.float32),
                   "rolling_variance": np.ones(n, np.float32)} if bn else {})} for n, c, k, bn in D.conv_shapes(secs)]
    g, outs, yolos = D.build_graph(dnn_hip.DnnGraphBuilder, secs, layers, [1, 416, 416, 3])
    entries = dnn_hip.lower_graph(g)
    assert entries is not None and VK.replay_slots(entries) == (2, set())
    assert [o.result.shape for o in outs] == [(1, 13, 13, 255), (1, 26, 26, 255)]
    assert D.multi_head(yolos, 416, 416).boxes == (13 * 13 + 26 * 26) * 3


# the entries yolov2.YOLO_V2([1, 64, 64, 3], synth.yolov2_weights(width_div=4)) lowered to before this
# lowering learnt to release a nested fork's slots (its fork is lowered with no slot live: unchanged)
def _v2_conv(k, cin, cout, bn=True):
    return f"ConvEntry k{k}x{k}x{cin}x{cout} s1,1 SAME bias=True bn={bn} leaky={bn}"


_POOL = "PoolEntry k2,2 s2,2 SAME"
YOLO_V2_ENTRIES = [
    _v2_conv(3, 3, 8), _POOL, _v2_conv(3, 8, 16), _POOL,
    _v2_conv(3, 16, 32), _v2_conv(1, 32, 16), _v2_conv(3, 16, 32), _POOL,
    _v2_conv(3, 32, 64), _v2_conv(1, 64, 32), _v2_conv(3, 32, 64), _POOL,
    _v2_conv(3, 64, 128), _v2_conv(1, 128, 64), _v2_conv(3, 64, 128), _v2_conv(1, 128, 64), _v2_conv(3, 64, 128),
    "StashEntry slot=0", _POOL,
    _v2_conv(3, 128, 256), _v2_conv(1, 256, 128), _v2_conv(3, 128, 256), _v2_conv(1, 256, 128), _v2_conv(3, 128, 256),
    _v2_conv(3, 256, 256), _v2_conv(3, 256, 256),
    "StashEntry slot=1", "RestoreEntry slot=0", _v2_conv(1, 128, 16),
    "RouteEntry block=2 slot=1 slot_first=False",
    _v2_conv(3, 320, 256), _v2_conv(1, 256, 425, bn=False),
]


def test_yolov2_lowers_exactly_as_before():
    import yolov2
    m = yolov2.YOLO_V2([1, 64, 64, 3], synth.yolov2_weights(width_div=4), False)
    entries = dnn_hip.lower_graph(m.g)
    assert [VK.entry_line(e) for e in entries] == YOLO_V2_ENTRIES
    assert VK.replay_slots(entries) == (2, {0, 1})  # a fork with no slot live keeps its slots to the end


def test_nested_fork_releases_and_outer_fork_does_not():
    """The same Concat fork lowered alone and inside a long skip."""
    def fork(g, x):
        k = np.zeros((3, 3, 8, 8), np.float32)
        a = g.create_conv2d(x, k, [1, 1, 1, 1], "SAME")
        return g.create_concat([a, x])
    g = dnn_hip.DnnGraphBuilder()
    x = g.create_input([1, 8, 8, 8])
    g.set_out_node(fork(g, x))
    alone = [VK.entry_line(e).split(" k")[0] for e in dnn_hip.lower_graph(g)]
    assert alone == ["StashEntry slot=0", "ConvEntry", "RouteEntry block=1 slot=0 slot_first=False"]
    g = dnn_hip.DnnGraphBuilder()
    x = g.create_input([1, 8, 8, 8])
    a = g.create_conv2d(x, np.zeros((3, 3, 8, 8), np.float32), [1, 1, 1, 1], "SAME")
    s = g.create_channel_slice(a, 0, 8)
    f = fork(g, s)
    d = g.create_conv2d(f, np.zeros((1, 1, 16, 8), np.float32), [1, 1, 1, 1], "SAME")
    g.set_out_node(g.create_concat([a, d]))
    nested = [VK.entry_line(e).split(" k")[0] for e in dnn_hip.lower_graph(g)]
    assert nested == ["ConvEntry", "StashEntry slot=0", "SliceEntry first=0 channels=8", "StashEntry slot=1", "ConvEntry",
                      "RouteEntry block=1 slot=1 slot_first=False", "ReleaseEntry slot=1", "ConvEntry",
                      "RouteEntry block=1 slot=0 slot_first=True", "ReleaseEntry slot=0"]
