"""Host-only checks of the fork/join feature: the numpy definition of the route op, the
lowering of fork/join graphs to stash / restore / route entries, the new plan calls of the C API
(shapes, memory, describe, errors) and the narrow YOLOv2 model's graph."""
import ctypes

import numpy as np
import pytest

import dnn_hip
import synth
import yolo_graph

import route_cases as RC

lib = dnn_hip.mylib


# ------------------------------------------------------------------------------ definition
@pytest.mark.parametrize("block,cb,b_first", [(2, 3, False), (2, 3, True), (1, 2, False), (3, 0, False)])
def test_route_helper_matches_the_literal_loops(block, cb, b_first):
    n, h, w, ca = 2, 6, 6, 2
    a = np.arange(n * h * w * ca, dtype=np.float32).reshape(n, h, w, ca)
    b = None
    if cb:
        b = 1000 + np.arange(n * (h // block) * (w // block) * cb, dtype=np.float32).reshape(n, h // block, w // block, cb)
    want = RC.route_loops(a, b, block, b_first)
    got = RC.route(a, b, block, b_first)
    assert got.shape == want.shape and np.array_equal(got, want)
    # TensorFlow's order: channel (dy*block + dx)*Ca + c of output pixel (0, 0)
    if block == 2 and not b_first:
        assert got[0, 0, 0, :8].tolist() == [a[0, 0, 0, 0], a[0, 0, 0, 1], a[0, 0, 1, 0], a[0, 0, 1, 1],
                                             a[0, 1, 0, 0], a[0, 1, 0, 1], a[0, 1, 1, 0], a[0, 1, 1, 1]]


# ------------------------------------------------------------------------------ nodes
def test_node_shapes_and_value_errors():
    g = dnn_hip.DnnGraphBuilder()
    x = g.create_input([2, 6, 8, 4])
    s = g.create_space_to_depth(x, 2)
    assert s.result.shape == (2, 3, 4, 16) and s.name == "space_to_depth_0"
    for bad in (0, 9, 4, 1.5):  # 4 does not divide 6
        with pytest.raises(ValueError):
            g.create_space_to_depth(x, bad)
    p = g.create_max_pool2d(x, [1, 2, 2, 1], [1, 2, 2, 1], "SAME")
    c = g.create_concat([s, p])
    assert c.result.shape == (2, 3, 4, 20) and c.name == "concat_0"
    with pytest.raises(ValueError):
        g.create_concat([s, x])  # spatial mismatch
    with pytest.raises(ValueError):
        g.create_concat([s])
    with pytest.raises(ValueError):
        g.create_concat([s, p, p])
    assert sorted(g.predecessors(c), key=lambda n: n.name) == sorted([s, p], key=lambda n: n.name)


# ------------------------------------------------------------------------------ lowering
def test_fork_join_lowering_entries():
    ws = RC.fork_join_weights("random")
    g = RC.fork_join_graph(1, ws, tail=1)
    entries = dnn_hip.lower_graph(g)
    assert RC.entry_kinds(entries) == "CSPCSRCJC"
    x_slot, trunk_slot = entries[1].slot, entries[4].slot
    assert (x_slot, trunk_slot) == (0, 1)
    assert entries[5].slot == x_slot
    r = entries[7]
    assert (r.block, r.slot, r.slot_first) == (2, trunk_slot, False)  # the SpaceToDepth fused into the join
    assert [type(n).__name__ for n in r.nodes] == ["SpaceToDepth", "Concat"]
    convs = [e for e in entries if isinstance(e, dnn_hip.ConvEntry)]
    assert all(e.bias is not None and e.bn is not None and e.leaky for e in convs)
    # every node but the input is covered exactly once
    covered = [n for e in entries for n in e.nodes]
    assert len(covered) == len(set(map(id, covered))) == len(RC.topo_nodes(g)) - 1


def test_chain_with_space_to_depth_lowering():
    ws = RC.exact_weights(((3, 32, 16), (1, 64, 8)))
    g = dnn_hip.DnnGraphBuilder()
    x = g.create_input([1, 8, 8, 32])
    x = RC._conv(g, x, ws[0])
    x = g.create_space_to_depth(x, 2)
    x = RC._conv(g, x, ws[1])
    g.set_out_node(x)
    entries = dnn_hip.lower_graph(g)
    assert RC.entry_kinds(entries) == "CJC"
    assert (entries[1].block, entries[1].slot) == (2, -1)


def test_empty_branch_and_two_joins_lower():
    g = RC.empty_branch_graph(1, RC.exact_weights(RC.EMPTY_BRANCH_LAYERS))
    entries = dnn_hip.lower_graph(g)
    assert RC.entry_kinds(entries) == "CSCJC"
    r = entries[3]
    assert (r.block, r.slot, r.slot_first) == (1, 0, True)  # Concat([x, f(x)]): the slot (x) first
    g = RC.two_joins_graph(1, RC.exact_weights(RC.TWO_JOINS_LAYERS))
    entries = dnn_hip.lower_graph(g)
    assert RC.entry_kinds(entries) == "C" "SCSRCJ" "C" "SPCSRCJ" "C"
    routes = [e for e in entries if isinstance(e, dnn_hip.RouteEntry)]
    assert [(r.block, r.slot, r.slot_first) for r in routes] == [(1, 1, True), (2, 3, True)]


def test_nested_fork_does_not_raise():
    ws = RC.exact_weights(((3, 32, 32), (3, 32, 32), (3, 32, 32), (1, 32, 32), (3, 32, 32), (1, 96, 8)))
    g = dnn_hip.DnnGraphBuilder()
    x = g.create_input([1, 8, 8, 32])
    x = RC._conv(g, x, ws[0])
    a = RC._conv(g, x, ws[1])
    inner = g.create_concat([RC._conv(g, a, ws[2]), RC._conv(g, a, ws[3])])  # a fork inside a branch
    y = g.create_concat([inner, RC._conv(g, x, ws[4])])
    y = RC._conv(g, y, ws[5])
    g.set_out_node(y)
    entries = dnn_hip.lower_graph(g)
    assert entries is None or all(hasattr(e, "nodes") for e in entries)


def test_graphs_without_new_nodes_lower_as_before():
    g, _ = yolo_graph.build_graph(dnn_hip.DnnGraphBuilder, synth.yolo_zero_weights())
    entries = dnn_hip.lower_graph(g)
    assert RC.entry_kinds(entries) == "CPCPCPCPCPCPCCC"
    g = dnn_hip.DnnGraphBuilder()
    g.set_out_node(g.create_leaky_relu(g.create_input([1, 4, 4, 8])))
    assert dnn_hip.lower_graph(g) is None  # a standalone element-wise op, as before


def test_exact_fork_join_oracles_agree():
    """On the integer inputs and {-1, 0, 1} weights of the exact GPU test, the float32 and float64
    oracles agree bit for bit and every value is an integer below 2^11."""
    ws = RC.fork_join_weights("exact")
    g = RC.fork_join_graph(4, ws)
    x = RC.exact_input(np.random.default_rng(1), (4,) + RC.FORK_JOIN_IN)
    v64 = RC.oracle_graph(g, x, acc=np.float64, keep=True)
    v32 = RC.oracle_graph(g, x, acc=np.float32, keep=True)
    for n, a in v64.items():
        assert a.dtype == np.float32 and a.tobytes() == v32[n].tobytes(), n.name
        assert np.array_equal(a, np.round(a)) and np.abs(a).max() < 2048, n.name
    assert np.abs(v64[g.out_node]).max() > 8  # not a trivial output


# ------------------------------------------------------------------------------ C API
def _plan(batch, h, w, c, fp16=False):
    p = ctypes.c_void_p()
    assert lib.dnn_plan_create(batch, h, w, c, ctypes.byref(p)) == 0
    if fp16:
        assert lib.dnn_plan_set_precision(p, 1) == 0
    return p


def _shape(p):
    b, h, w, c = (ctypes.c_int() for _ in range(4))
    assert lib.dnn_plan_output_shape(p, ctypes.byref(b), ctypes.byref(h), ctypes.byref(w), ctypes.byref(c)) == 0
    return h.value, w.value, c.value


def _memory(p):
    wb, sb = ctypes.c_size_t(), ctypes.c_size_t()
    assert lib.dnn_plan_memory(p, ctypes.byref(wb), ctypes.byref(sb)) == 0
    return wb.value, sb.value


def _conv(p, k, od):
    assert lib.dnn_plan_add_conv(p, k, k, od, 1, 1, 1, None, None, None, None, None, 0.0, 0) == 0, dnn_hip.last_error()


def _fails(rc):
    assert rc != 0
    assert dnn_hip.last_error() != ""


def test_plan_api_shapes_memory_describe():
    B = 4
    slot = ctypes.c_int(-1)
    # the same layers as a chain, for the workspace comparison
    q = _plan(B, 16, 16, 32)
    _conv(q, 3, 64)
    assert lib.dnn_plan_add_max_pool(q, 2, 2, 2, 2, 1) == 0
    _conv(q, 3, 128)
    _, chain_ws = _memory(q)
    lib.dnn_plan_destroy(q)

    p = _plan(B, 16, 16, 32)
    try:
        _conv(p, 3, 64)
        assert lib.dnn_plan_add_stash(p, ctypes.byref(slot)) == 0 and slot.value == 0
        assert _shape(p) == (16, 16, 64)  # a stash keeps the tensor
        assert lib.dnn_plan_add_max_pool(p, 2, 2, 2, 2, 1) == 0
        _conv(p, 3, 128)
        assert lib.dnn_plan_add_stash(p, ctypes.byref(slot)) == 0 and slot.value == 1
        assert _shape(p) == (8, 8, 128)
        _, ws_stashed = _memory(p)
        slot_bytes = 4 * B * (16 * 16 * 64 + 8 * 8 * 128)
        assert ws_stashed >= chain_ws + slot_bytes
        assert lib.dnn_plan_add_restore(p, 0) == 0
        assert _shape(p) == (16, 16, 64)
        _conv(p, 1, 32)
        assert lib.dnn_plan_add_route(p, 2, 1, 0) == 0, dnn_hip.last_error()
        assert _shape(p) == (8, 8, 4 * 32 + 128)
        _conv(p, 3, 64)
        assert lib.dnn_plan_add_route(p, 2, -1, 0) == 0  # a pure space_to_depth
        assert _shape(p) == (4, 4, 256)
        buf = ctypes.create_string_buffer(8192)
        assert lib.dnn_plan_describe(p, buf, 8192) == 0
        lines = buf.value.decode().splitlines()
        assert [l.split()[0] for l in lines] == ["conv", "stash", "pool", "conv", "stash", "restore", "conv", "route",
                                                 "conv", "route"]
        assert lines[1] == "stash 16x16x64 slot=0" and lines[4] == "stash 8x8x128 slot=1"
        assert lines[5] == "restore 16x16x64 slot=0"
        assert lines[7] == "route 16x16x32 -> 8x8x256 block=2 slot=1 (8x8x128) last"
        assert lines[9] == "route 8x8x64 -> 4x4x256 block=2"
        # the 3x3 conv after the route stays on the fp32 GEMM: no split planes come out of a route
        assert "mode=implicit" in lines[8]
        names = []
        for i in range(lib.dnn_plan_num_kernels(p)):
            nm = ctypes.create_string_buffer(64)
            fl, by = ctypes.c_double(), ctypes.c_double()
            assert lib.dnn_plan_kernel_info(p, i, nm, 64, ctypes.byref(fl), ctypes.byref(by)) == 0
            names.append(nm.value.decode())
            if names[-1] == "route0":
                assert fl.value == 0 and by.value == 2 * 4.0 * B * 8 * 8 * 256
        assert [n for n in names if n.startswith("route")] == ["route0", "route1"]
        assert not any("stash" in n or "restore" in n for n in names)
    finally:
        lib.dnn_plan_destroy(p)


def test_stash_of_the_input_needs_no_region():
    p = _plan(2, 8, 8, 16)
    slot = ctypes.c_int(-1)
    try:
        assert lib.dnn_plan_add_stash(p, ctypes.byref(slot)) == 0 and slot.value == 0
        assert lib.dnn_plan_add_route(p, 1, 0, 1) == 0
        assert _shape(p) == (8, 8, 32)
        _, ws = _memory(p)
        assert ws <= 4 * 2 * (2 * 8 * 8 * 32) + 1024  # two activation buffers (+ the zero page), no copy of the input
    finally:
        lib.dnn_plan_destroy(p)


def test_plan_api_errors():
    slot = ctypes.c_int(-1)
    p = _plan(1, 6, 6, 8)
    try:
        _fails(lib.dnn_plan_add_route(p, 4, -1, 0))   # 6 % 4 != 0
        _fails(lib.dnn_plan_add_route(p, 0, -1, 0))
        _fails(lib.dnn_plan_add_route(p, 9, -1, 0))
        _fails(lib.dnn_plan_add_route(p, 2, 0, 0))    # no slot 0 yet
        _fails(lib.dnn_plan_add_restore(p, 0))
        _fails(lib.dnn_plan_add_restore(p, -1))
        assert lib.dnn_plan_add_stash(p, ctypes.byref(slot)) == 0  # 6x6
        _fails(lib.dnn_plan_add_route(p, 2, 0, 0))    # slot 0 is 6x6, the folded input 3x3
        _fails(lib.dnn_plan_add_route(p, 1, 1, 0))    # unknown slot
        for want in (1, 2, 3):
            assert lib.dnn_plan_add_stash(p, ctypes.byref(slot)) == 0 and slot.value == want
        _fails(lib.dnn_plan_add_stash(p, ctypes.byref(slot)))  # a fifth slot
        assert _shape(p) == (6, 6, 8)  # the failed calls changed nothing
    finally:
        lib.dnn_plan_destroy(p)
    p = _plan(1, 8, 8, 8, fp16=True)
    try:
        _fails(lib.dnn_plan_add_stash(p, ctypes.byref(slot)))
        assert "fp16" in dnn_hip.last_error()
        _fails(lib.dnn_plan_add_restore(p, 0))
        assert "fp16" in dnn_hip.last_error()
        _fails(lib.dnn_plan_add_route(p, 2, -1, 0))
        assert "fp16" in dnn_hip.last_error()
    finally:
        lib.dnn_plan_destroy(p)


def test_route_host_refuses_a_2_gib_tensor():
    """Refused from the sizes alone, before any allocation or copy (the arrays are never read)."""
    tiny = np.zeros(16, np.float32)
    for n, h, w, ca, block, cb in ((1, 16384, 16384, 2, 2, 0),       # a and out: 2 GiB each
                                   (1, 8192, 8192, 4, 1, 4),         # a and b 1 GiB each, out 2 GiB
                                   (2, 8192, 8192, 4, 2, 0)):
        b = dnn_hip._vp(tiny) if cb else None
        rc = lib.dnn_route_host(dnn_hip._vp(tiny), b, dnn_hip._vp(tiny), n, h, w, ca, block, cb, 0)
        assert rc != 0 and "2 GiB" in dnn_hip.last_error(), (n, h, w, ca, block, cb)


@pytest.mark.gpu
def test_finalize_refuses_a_trailing_stash_or_restore():
    slot = ctypes.c_int(-1)
    for trailing in ("stash", "restore"):
        p = _plan(1, 8, 8, 32)
        try:
            _conv(p, 3, 32)
            assert lib.dnn_plan_add_stash(p, ctypes.byref(slot)) == 0
            if trailing == "restore":
                _conv(p, 3, 32)
                assert lib.dnn_plan_add_restore(p, 0) == 0
            _fails(lib.dnn_plan_finalize(p, 0, None, None))
            assert trailing in dnn_hip.last_error()
        finally:
            lib.dnn_plan_destroy(p)


def test_plan_memory_from_entries():
    """Plan.memory emits the new entries too."""
    ws = RC.fork_join_weights("exact")
    entries = dnn_hip.lower_graph(RC.fork_join_graph(4, ws))
    wb, sb = dnn_hip.Plan.memory(4, RC.FORK_JOIN_IN, entries)
    assert wb > 0 and sb >= 4 * 4 * (16 * 16 * 64 + 8 * 8 * 128)
    wl, sl = dnn_hip.Plan.memory(4, RC.FORK_JOIN_IN, entries, latency=True)
    assert sl >= 4 * 4 * (16 * 16 * 64 + 8 * 8 * 128)


# ------------------------------------------------------------------------------ model
def test_narrow_yolov2_builds_and_lowers():
    import yolov2
    ws = synth.yolov2_weights(width_div=4)
    assert len(ws) == 23 and ws[-1]["kernel"].shape == (1, 1, 256, 425) and "gamma" not in ws[-1]
    assert ws[20]["kernel"].shape == (1, 1, 128, 16) and ws[21]["kernel"].shape == (3, 3, 64 + 256, 256)
    m = yolov2.YOLO_V2([1, 64, 64, 3], ws, False)
    assert (m.head.grid_h, m.head.grid_w, m.head.n_out, m.head.n_classes) == (2, 2, 425, 80)
    assert m.g.out_node.result.shape == (1, 2, 2, 425)
    entries = dnn_hip.lower_graph(m.g)
    assert entries is not None
    # 13 trunk convs and 4 pools, the stash of the 512-channel activation, the fifth pool and the
    # trunk's other 7 convs, stash / restore, the passthrough conv, the fused route, the 2 head convs
    assert RC.entry_kinds(entries) == "CPCPCCCPCCCPCCCCC" "S" "PCCCCCCC" "SR" "C" "J" "CC"
    r = [e for e in entries if isinstance(e, dnn_hip.RouteEntry)][0]
    assert (r.block, r.slot, r.slot_first) == (2, 1, False)
    with pytest.raises(ValueError):
        yolov2.YOLO_V2([1, 72, 64, 3], ws, False)  # not a multiple of 32
    with pytest.raises(ValueError):
        yolov2.YOLO_V2([1, 64, 64, 3], ws[:-1], False)
