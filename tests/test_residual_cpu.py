"""Host-only checks of the residual / top-down feature: the numpy statements of add and upsample,
the Add and Upsample nodes, the lowering to stash / shortcut / release / upsample entries (with
slot numbers), the new plan calls of the C API (errors, slot and region reuse, memory, describe)
and the narrow Darknet-53 model's graph."""
import ctypes

import numpy as np
import pytest

import dnn_hip
import synth
import yolo_graph
import yolo_weights

import residual_cases as RS
import route_cases as RC

lib = dnn_hip.mylib


# ------------------------------------------------------------------------------ definitions
def test_numpy_statements():
    a = np.arange(2 * 2 * 3 * 2, dtype=np.float32).reshape(2, 2, 3, 2)
    for f in (1, 2, 3):
        assert np.array_equal(RS.upsample(a, f), RS.upsample_loops(a, f))
    t = np.array([-10.0, -1.0, -0.0, 0.0, 3.0, -3e38], np.float32)
    z = np.zeros_like(t)
    assert RS.add(t, z, 0).tobytes() == (t + z).tobytes() and np.array_equal(RS.add(t, z, 0), t)
    assert RS.add(t, z, 1).tolist() == [np.float32(0.1 * -10.0), np.float32(0.1 * -1.0), -0.0, 0.0, 3.0,
                                        np.float32(0.1 * float(np.float32(-3e38)))]
    assert RS.add(t, z, 2)[:2].tolist() == [np.float32(-10.0) * np.float32(0.1), np.float32(-1.0) * np.float32(0.1)]
    assert RS.add(np.float32(3e38), np.float32(3e38)) == np.inf


# ------------------------------------------------------------------------------ nodes
def test_node_shapes_names_and_value_errors():
    g = dnn_hip.DnnGraphBuilder()
    x = g.create_input([2, 6, 8, 4])
    p = g.create_max_pool2d(x, [1, 2, 2, 1], [1, 1, 1, 1], "SAME")
    a = g.create_add([x, p])
    assert a.result.shape == (2, 6, 8, 4) and a.result.dtype == np.float32 and a.name == "add_0"
    assert g.create_add([a, x]).name == "add_1"
    assert sorted(g.predecessors(a), key=lambda n: n.name) == sorted([x, p], key=lambda n: n.name)
    half = g.create_max_pool2d(x, [1, 2, 2, 1], [1, 2, 2, 1], "SAME")
    for bad in ([x], [x, p, p], [x, half]):
        with pytest.raises(ValueError):
            g.create_add(bad)
    u = g.create_upsample(half, 2)
    assert u.result.shape == (2, 6, 8, 4) and u.name == "upsample_0" and u.factor == 2
    assert g.create_upsample(x, 8).result.shape == (2, 48, 64, 4)
    assert g.create_upsample(x, 1).name == "upsample_2"
    for bad in (0, 9, 1.5, -1):
        with pytest.raises(ValueError):
            g.create_upsample(x, bad)
    assert g.predecessors(u) == [half]


# ------------------------------------------------------------------------------ lowering
def _slots(entries):
    """(letter, slot) of every entry that names a slot."""
    k = RS.entry_kinds(entries)
    return [(c, e.slot) for c, e in zip(k, entries) if c in "SRAXJ"]


def test_one_residual_block_lowers():
    g = RS.blocks_graph(1, RC.exact_weights(RS.blocks_layers(1)), 1)
    entries = dnn_hip.lower_graph(g)
    assert RS.entry_kinds(entries) == "C" "SCCAX" "C"
    assert _slots(entries) == [("S", 0), ("A", 0), ("X", 0)]
    assert not entries[4].leaky and [type(n).__name__ for n in entries[4].nodes] == ["Add"]
    covered = [n for e in entries for n in e.nodes]
    assert len(covered) == len(set(map(id, covered))) == len(RC.topo_nodes(g)) - 1


def test_projection_block_lowers():
    g = RS.projection_graph(1, RC.exact_weights(RS.PROJECTION_LAYERS))
    entries = dnn_hip.lower_graph(g)
    assert RS.entry_kinds(entries) == "C" "SCCSRCAXX" "C"
    assert _slots(entries) == [("S", 0), ("S", 1), ("R", 0), ("A", 1), ("X", 0), ("X", 1)]


def test_add_followed_by_leaky_folds():
    g = RS.blocks_graph(1, RC.exact_weights(RS.blocks_layers(2)), 2, act_after_add=True)
    entries = dnn_hip.lower_graph(g)
    assert RS.entry_kinds(entries) == "C" "SCCAX" "SCCAX" "C"
    adds = [e for e in entries if isinstance(e, dnn_hip.ShortcutEntry)]
    assert all(e.leaky and [type(n).__name__ for n in e.nodes] == ["Add", "LeakyReLU"] for e in adds)
    covered = [n for e in entries for n in e.nodes]
    assert len(covered) == len(set(map(id, covered))) == len(RC.topo_nodes(g)) - 1


def test_top_down_merge_lowers_through_the_fork_code():
    g = RS.top_down_graph(1, RC.exact_weights(RS.TOP_DOWN_LAYERS))
    entries = dnn_hip.lower_graph(g)
    # the empty branch (x) waits in the slot; pool, two convs and the upsample are the route's a
    assert RS.entry_kinds(entries) == "C" "SPCCUJ" "C"
    assert entries[5].factor == 2
    r = entries[6]
    assert (r.block, r.slot, r.slot_first) == (1, 0, False)
    assert not any(isinstance(e, dnn_hip.ReleaseEntry) for e in entries)


def test_six_blocks_reuse_one_slot():
    g = RS.blocks_graph(1, RC.exact_weights(RS.blocks_layers(6)), 6)
    entries = dnn_hip.lower_graph(g)
    assert RS.entry_kinds(entries) == "C" + "SCCAX" * 6 + "C"
    assert _slots(entries) == [("S", 0), ("A", 0), ("X", 0)] * 6
    # live slots never exceed three, and every slot opened is released
    live, most = set(), 0
    for c, s in _slots(entries):
        if c == "S":
            assert s not in live
            live.add(s)
        elif c == "X":
            live.remove(s)
        most = max(most, len(live))
    assert not live and most <= 3
    wb, sb = dnn_hip.Plan.memory(1, RS.IN_SHAPE, entries)
    g2 = RS.blocks_graph(1, RC.exact_weights(RS.blocks_layers(2)), 2)
    wb2, sb2 = dnn_hip.Plan.memory(1, RS.IN_SHAPE, dnn_hip.lower_graph(g2))
    assert sb == sb2 and wb > wb2  # the blocks alternate between two regions


def test_add_block_after_a_concat_fork_takes_the_next_slots():
    ws = RC.exact_weights(RC.EMPTY_BRANCH_LAYERS[:2] + ((1, 96, 32),) + RS.BLOCK + ((1, 32, 8),))
    g = dnn_hip.DnnGraphBuilder()
    x = RC._conv(g, g.create_input([1, 8, 8, 32]), ws[0])
    x = RC._conv(g, g.create_concat([x, RC._conv(g, x, ws[1])]), ws[2])
    x = g.create_add([x, RC._conv(g, RC._conv(g, x, ws[3]), ws[4])])
    g.set_out_node(RC._conv(g, x, ws[5]))
    entries = dnn_hip.lower_graph(g)
    assert RS.entry_kinds(entries) == "C" "SCJ" "C" "SCCAX" "C"
    assert _slots(entries) == [("S", 0), ("J", 0), ("S", 1), ("A", 1), ("X", 1)]


def test_nested_and_malformed_forks_do_not_lower():
    ws = RC.exact_weights(((3, 32, 32), (3, 32, 32), (3, 32, 32), (1, 32, 32)))
    g = dnn_hip.DnnGraphBuilder()
    x = RC._conv(g, g.create_input([1, 8, 8, 32]), ws[0])
    a = RC._conv(g, x, ws[1])
    inner = g.create_add([RC._conv(g, a, ws[2]), a])  # a fork inside a branch
    g.set_out_node(RC._conv(g, g.create_add([inner, x]), ws[3]))
    assert dnn_hip.lower_graph(g) is None
    g = dnn_hip.DnnGraphBuilder()
    x = RC._conv(g, g.create_input([1, 8, 8, 32]), ws[0])
    g.set_out_node(g.create_add([x, x]))
    assert dnn_hip.lower_graph(g) is None


def test_existing_graphs_lower_to_the_same_entries():
    g, _ = yolo_graph.build_graph(dnn_hip.DnnGraphBuilder, synth.yolo_zero_weights())
    assert RS.entry_kinds(dnn_hip.lower_graph(g)) == "CPCPCPCPCPCPCCC"
    import yolov2
    m, _ = yolov2.build_graph(dnn_hip.DnnGraphBuilder, synth.yolov2_weights(width_div=8), in_shape=(1, 64, 64, 3))
    assert RS.entry_kinds(dnn_hip.lower_graph(m)) == "CPCPCCCPCCCPCCCCC" "S" "PCCCCCCC" "SR" "C" "J" "CC"
    assert RS.entry_kinds(dnn_hip.lower_graph(RC.fork_join_graph(1, RC.fork_join_weights("exact")))) == "CSPCSRCJCC"
    assert RS.entry_kinds(dnn_hip.lower_graph(
        RC.empty_branch_graph(1, RC.exact_weights(RC.EMPTY_BRANCH_LAYERS)))) == "CSCJC"
    e = dnn_hip.lower_graph(RC.two_joins_graph(1, RC.exact_weights(RC.TWO_JOINS_LAYERS)))
    assert RS.entry_kinds(e) == "C" "SCSRCJ" "C" "SPCSRCJ" "C"
    assert [(r.block, r.slot, r.slot_first) for r in e if isinstance(r, dnn_hip.RouteEntry)] == [(1, 1, True),
                                                                                                (2, 3, True)]


# ------------------------------------------------------------------------------ C API
def _plan(batch, h, w, c, fp16=False, latency=False):
    p = ctypes.c_void_p()
    assert lib.dnn_plan_create(batch, h, w, c, ctypes.byref(p)) == 0
    if fp16:
        assert lib.dnn_plan_set_precision(p, 1) == 0
    if latency:
        assert lib.dnn_plan_set_latency_mode(p, 1) == 0
    return p


def _shape(p):
    b, h, w, c = (ctypes.c_int() for _ in range(4))
    assert lib.dnn_plan_output_shape(p, ctypes.byref(b), ctypes.byref(h), ctypes.byref(w), ctypes.byref(c)) == 0
    return h.value, w.value, c.value


def _ws(p):
    wb, sb = ctypes.c_size_t(), ctypes.c_size_t()
    assert lib.dnn_plan_memory(p, ctypes.byref(wb), ctypes.byref(sb)) == 0
    return sb.value


def _describe(p):
    buf = ctypes.create_string_buffer(16384)
    assert lib.dnn_plan_describe(p, buf, 16384) == 0
    return buf.value.decode().splitlines()


def _conv(p, k, od):
    assert lib.dnn_plan_add_conv(p, k, k, od, 1, 1, 1, None, None, None, None, None, 0.0, 0) == 0, dnn_hip.last_error()


def _stash(p):
    slot = ctypes.c_int(-1)
    assert lib.dnn_plan_add_stash(p, ctypes.byref(slot)) == 0, dnn_hip.last_error()
    return slot.value


def _ok(rc):
    assert rc == 0, dnn_hip.last_error()


def _fails(p, rc, before):
    """The call failed with a message and left the plan's shape and entries as they were."""
    assert rc != 0 and dnn_hip.last_error() != ""
    assert (_shape(p), _describe(p)) == before


def _state(p):
    return _shape(p), _describe(p)


def test_entry_errors_leave_the_plan_unchanged():
    p = _plan(1, 6, 6, 8)
    try:
        st = _state(p)
        _fails(p, lib.dnn_plan_add_shortcut(p, 0, 0), st)    # no slot yet
        _fails(p, lib.dnn_plan_add_release(p, 0), st)
        _fails(p, lib.dnn_plan_add_release(p, -1), st)
        for bad in (0, 9, -2):
            _fails(p, lib.dnn_plan_add_upsample(p, bad), st)
        assert _stash(p) == 0                                # 6x6x8
        st = _state(p)
        for bad in (-1, 3):
            _fails(p, lib.dnn_plan_add_shortcut(p, 0, bad), st)  # leaky outside 0..2
        _fails(p, lib.dnn_plan_add_shortcut(p, 1, 0), st)    # unknown slot
        _fails(p, lib.dnn_plan_add_shortcut(p, -1, 0), st)
        _fails(p, lib.dnn_plan_add_release(p, 1), st)
        _conv(p, 3, 16)
        st = _state(p)
        _fails(p, lib.dnn_plan_add_shortcut(p, 0, 0), st)    # 6x6x8 against 6x6x16
        _ok(lib.dnn_plan_add_upsample(p, 2))
        assert _shape(p) == (12, 12, 16)
        _conv(p, 1, 8)
        st = _state(p)
        _fails(p, lib.dnn_plan_add_shortcut(p, 0, 0), st)    # 6x6x8 against 12x12x8
        _ok(lib.dnn_plan_add_release(p, 0))
        st = _state(p)
        _fails(p, lib.dnn_plan_add_release(p, 0), st)        # a second release
        _fails(p, lib.dnn_plan_add_restore(p, 0), st)        # released
        _fails(p, lib.dnn_plan_add_route(p, 1, 0, 0), st)
        _fails(p, lib.dnn_plan_add_shortcut(p, 0, 0), st)
        assert st[1][-1] == "release 6x6x8 slot=0"
    finally:
        lib.dnn_plan_destroy(p)


def test_fp16_plans_refuse_the_three_entries():
    p = _plan(1, 8, 8, 8, fp16=True)
    try:
        for rc in (lib.dnn_plan_add_shortcut(p, 0, 0), lib.dnn_plan_add_upsample(p, 2), lib.dnn_plan_add_release(p, 0)):
            assert rc != 0 and "fp16" in dnn_hip.last_error()
        assert _shape(p) == (8, 8, 8) and _describe(p) == []
    finally:
        lib.dnn_plan_destroy(p)


def test_slot_numbers_are_reused_after_a_release():
    slot = ctypes.c_int(-1)
    p = _plan(1, 6, 6, 8)
    try:
        assert [_stash(p) for _ in range(4)] == [0, 1, 2, 3]
        assert lib.dnn_plan_add_stash(p, ctypes.byref(slot)) != 0  # a fifth live slot
        _ok(lib.dnn_plan_add_release(p, 1))
        assert _stash(p) == 1
        assert lib.dnn_plan_add_stash(p, ctypes.byref(slot)) != 0
        _ok(lib.dnn_plan_add_release(p, 3))
        _ok(lib.dnn_plan_add_release(p, 0))
        assert _stash(p) == 0 and _stash(p) == 3                   # the lowest free number first
    finally:
        lib.dnn_plan_destroy(p)


def _block_chain(nblocks, latency=False):
    """conv; nblocks x (stash, 1x1, 3x3, shortcut, release); conv — at 8x8x32, batch 2."""
    p = _plan(2, 8, 8, 32, latency=latency)
    _conv(p, 3, 32)
    for _ in range(nblocks):
        s = _stash(p)
        _conv(p, 1, 16)
        _conv(p, 3, 32)
        _ok(lib.dnn_plan_add_shortcut(p, s, 0))
        _ok(lib.dnn_plan_add_release(p, s))
    _conv(p, 1, 8)
    return p


@pytest.mark.parametrize("latency", [False, True], ids=["batch", "latency"])
def test_block_chain_memory_and_describe(latency):
    region = 4 * 2 * 8 * 8 * 32  # one stashed tensor of the planned batch, in bytes
    ws = {}
    for nb in (0, 1, 2, 6):
        p = _block_chain(nb, latency)
        try:
            ws[nb] = _ws(p)
            if nb == 2:
                d = _describe(p)
                assert [l.split()[0] for l in d] == ["conv"] + ["stash", "conv", "conv", "shortcut", "release"] * 2 + ["conv"]
                assert d[4] == "shortcut 8x8x32 slot=0 act=none" and d[5] == "release 8x8x32 slot=0"
                assert d[6] == "stash 8x8x32 slot=0"
                names = _kernel_names(p)
                assert [n for n in names if n[0].startswith("shortcut")] == [
                    ("shortcut0", 2.0 * 8 * 8 * 32, 3 * 4.0 * 2 * 8 * 8 * 32),
                    ("shortcut1", 2.0 * 8 * 8 * 32, 3 * 4.0 * 2 * 8 * 8 * 32)]
                assert not any("release" in n[0] or "stash" in n[0] for n in names)
        finally:
            lib.dnn_plan_destroy(p)
    # block 1 stashes conv0's output in region 0; block 2's stash is the first shortcut's output,
    # which read region 0 and was added before the release: region 1; block 3 takes region 0 again
    assert ws[1] == ws[0] + region
    assert ws[2] == ws[0] + 2 * region
    assert ws[6] == ws[2]


def _kernel_names(p):
    out = []
    for i in range(lib.dnn_plan_num_kernels(p)):
        nm = ctypes.create_string_buffer(64)
        fl, by = ctypes.c_double(), ctypes.c_double()
        assert lib.dnn_plan_kernel_info(p, i, nm, 64, ctypes.byref(fl), ctypes.byref(by)) == 0
        out.append((nm.value.decode(), fl.value, by.value))
    return out


def test_a_region_is_given_only_to_a_later_producer():
    """stash(s), conv, conv, release(s), stash: the second conv was added before the release, so it
    may not take s's region although nothing reads it any more; with one more conv after the
    release it may."""
    region = 4 * 2 * 8 * 8 * 32
    sizes = []
    for extra in (False, True):
        p = _plan(2, 8, 8, 32)
        try:
            _conv(p, 3, 32)
            base = _ws(p)
            s = _stash(p)
            _conv(p, 3, 32)
            _conv(p, 3, 32)
            _ok(lib.dnn_plan_add_release(p, s))
            if extra:
                _conv(p, 3, 32)
            assert _stash(p) == 0  # its producer is the last conv, not the release entry
            _conv(p, 3, 32)
            _ok(lib.dnn_plan_add_shortcut(p, 0, 1))
            assert _describe(p)[-1] == "shortcut 8x8x32 slot=0 act=leaky"
            sizes.append(_ws(p) - base)
        finally:
            lib.dnn_plan_destroy(p)
    assert sizes[0] - sizes[1] == region and sizes[1] >= region


def test_a_region_grows_to_the_largest_tensor_it_holds():
    B = 2
    p = _plan(B, 8, 8, 32)
    try:
        _conv(p, 3, 32)
        base = _ws(p)
        s = _stash(p)                      # 8x8x32 in region 0
        _conv(p, 3, 32)
        _ok(lib.dnn_plan_add_release(p, s))
        _conv(p, 3, 64)                    # added after the release: may write region 0
        assert _stash(p) == 0              # 8x8x64: region 0 grows
        _conv(p, 3, 64)
        _ok(lib.dnn_plan_add_shortcut(p, 0, 2))
        grown = _ws(p)
        assert _describe(p)[-1] == "shortcut 8x8x64 slot=0 act=leaky_f32"
    finally:
        lib.dnn_plan_destroy(p)
    q = _plan(B, 8, 8, 32)
    try:                                   # the same convs with the one large stash only
        _conv(q, 3, 32)
        _conv(q, 3, 32)
        _conv(q, 3, 64)
        _stash(q)
        _conv(q, 3, 64)
        _ok(lib.dnn_plan_add_shortcut(q, 0, 2))
        assert grown == _ws(q) and grown >= base + 4 * B * 8 * 8 * 64
    finally:
        lib.dnn_plan_destroy(q)


def test_upsample_shapes_describe_and_kernel_info():
    B = 2
    p = _plan(B, 4, 6, 16)
    try:
        _conv(p, 3, 32)
        s = _stash(p)
        _ok(lib.dnn_plan_add_upsample(p, 3))
        assert _shape(p) == (12, 18, 32)
        _conv(p, 3, 32)
        d = _describe(p)
        assert d[2] == "upsample 4x6x32 -> 12x18x32 factor=3"
        assert "mode=implicit" in d[3]     # no split planes come out of an upsample
        names = _kernel_names(p)
        assert [n for n in names if n[0].startswith("upsample")] == [
            ("upsample0", 0.0, 4.0 * B * 4 * 6 * 32 * (1 + 9))]
        _ok(lib.dnn_plan_add_release(p, s))
    finally:
        lib.dnn_plan_destroy(p)


def test_host_forms_refuse_a_2_gib_tensor_and_bad_arguments():
    """Refused from the sizes alone, before any allocation or copy (the arrays are never read)."""
    tiny = np.zeros(16, np.float32)
    v = dnn_hip._vp
    assert lib.dnn_shortcut_host(v(tiny), v(tiny), v(tiny), 1, 16384, 16384, 2, 0) != 0
    assert "2 GiB" in dnn_hip.last_error()
    assert lib.dnn_upsample_host(v(tiny), v(tiny), 1, 8192, 8192, 2, 2) != 0
    assert "2 GiB" in dnn_hip.last_error()
    assert lib.dnn_upsample_host(v(tiny), v(tiny), 2, 16384, 16384, 4, 1) != 0
    assert "2 GiB" in dnn_hip.last_error()
    for bad in (0, 9):
        assert lib.dnn_upsample_host(v(tiny), v(tiny), 1, 2, 2, 4, bad) != 0 and dnn_hip.last_error() != ""
    for bad in (-1, 3):
        assert lib.dnn_shortcut_host(v(tiny), v(tiny), v(tiny), 1, 2, 2, 4, bad) != 0
    assert lib.dnn_shortcut_host(v(tiny), None, v(tiny), 1, 2, 2, 4, 0) != 0
    assert lib.dnn_shortcut_host(v(tiny), v(tiny), v(tiny), 1, 0, 2, 4, 0) != 0


def test_plan_memory_from_entries_emits_the_new_entries():
    ws = RC.exact_weights(RS.blocks_layers(2))
    entries = dnn_hip.lower_graph(RS.blocks_graph(4, ws, 2))
    wb, sb = dnn_hip.Plan.memory(4, RS.IN_SHAPE, entries)
    assert wb > 0 and sb >= 4 * 4 * 2 * 8 * 8 * 32
    with pytest.raises(dnn_hip.DnnHipError, match="fp16"):
        dnn_hip.Plan.memory(4, RS.IN_SHAPE, entries, precision="fp16")


# ------------------------------------------------------------------------------ model
def test_narrow_darknet53_builds_validates_and_lowers():
    import darknet53
    ws = synth.darknet53_weights(width_div=8)
    assert len(ws) == darknet53.N_LAYERS == 59 and darknet53.N_TRUNK == 52 and darknet53.N_SHORTCUTS == 23
    assert ws[0]["kernel"].shape == (3, 3, 3, 4) and ws[-1]["kernel"].shape == (1, 1, 128, 425)
    assert "gamma" not in ws[-1] and max(w["kernel"].shape[3] for w in ws[:-1]) == 128
    spec = darknet53.structure()
    assert sum(1 for k, s, _ in spec if (k, s) == (3, 2)) == 5
    assert [r for _, _, r in spec].count("expand") == 23
    m = darknet53.DARKNET53([2, 64, 64, 3], ws, False)
    assert m.g.out_node.result.shape == (2, 2, 2, 425)
    assert (m.head.grid_h, m.head.grid_w, m.head.n_out) == (2, 2, 425)
    assert sum(isinstance(n, dnn_hip.Add) for n in m.nodes) == 23
    entries = dnn_hip.lower_graph(m.g)
    assert entries is not None
    kinds = RS.entry_kinds(entries)
    assert kinds == "C" + "".join("C" + "SCCAX" * b for b in darknet53.STAGE_BLOCKS) + "C" * 7
    assert kinds.count("C") == 59 and kinds.count("A") == 23
    assert all(e.slot == 0 for e in entries if hasattr(e, "slot"))
    assert entries[-1].bn is None and not entries[-1].leaky and entries[-2].leaky
    with pytest.raises(ValueError):
        darknet53.DARKNET53([1, 72, 64, 3], ws, False)  # not a multiple of 32
    with pytest.raises(yolo_weights.WeightFileError):
        darknet53.validate(ws[:-1])
    bad = list(ws)
    bad[3] = synth.layer_weights(3, 4, 16, k=3)          # a block's second conv that changes the width
    with pytest.raises(yolo_weights.WeightFileError):
        darknet53.validate(bad)
    bad = list(ws)
    bad[2] = synth.layer_weights(2, 8, 4, k=3)           # a 3x3 where the block's 1x1 belongs
    with pytest.raises(yolo_weights.WeightFileError):
        darknet53.validate(bad)
    with pytest.raises(yolo_weights.WeightFileError):
        darknet53.validate(ws, n_out=255)
    with pytest.raises(ValueError):
        synth.darknet53_weights(width_div=3)
