"""Host-only checks of plans and graphs with several outputs: the tap entries of the plan ABI
(misuse, shapes, memory), the two lowering patterns that YOLOv3's neck needs (output branch, long
skip into a Concat), the graphs that must lower as before, DnnInferenceEngine.run_all's order, and
yolov3.py's structure and validation.  No GPU: plans are laid out, never finalized."""
import ctypes
import json
import os

import numpy as np
import pytest

import darknet53
import dnn_hip
import multi_out_cases as MC
import residual_cases as RS
import route_cases as RC
import synth
import yolo_graph
import yolo_weights
import yolov2
import yolov3

HERE = os.path.dirname(os.path.abspath(__file__))
lib = dnn_hip.mylib

PLAN_SYMBOLS = ("dnn_plan_add_tap", "dnn_plan_num_taps", "dnn_plan_tap_shape", "dnn_plan_tap_buffer",
                "dnn_plan_tap_read_host")
POST_SYMBOLS = ("dnn_yolo_multi_boxes", "dnn_yolo_multi_workspace", "dnn_yolo_postprocess_multi",
                "dnn_yolo_postprocess_multi_host")


@pytest.mark.parametrize("name", ["libdnn_hip.so", "libdnn_hip_avx.so"])
def test_both_libraries_export_the_new_symbols(name):
    so = ctypes.CDLL(os.path.join(os.path.dirname(HERE), "dnn-inference-engine_amd", name))
    for sym in PLAN_SYMBOLS + POST_SYMBOLS:
        assert hasattr(so, sym), f"{name} lacks {sym}"


# ------------------------------------------------------------------------------ the tap ABI
class RawPlan(object):
    def __init__(self, batch=2, shape=(8, 8, 32), fp16=False):
        self.h = ctypes.c_void_p()
        assert lib.dnn_plan_create(batch, *shape, ctypes.byref(self.h)) == 0
        if fp16:
            assert lib.dnn_plan_set_precision(self.h, 1) == 0

    def conv(self, k, od):
        assert lib.dnn_plan_add_conv(self.h, k, k, od, 1, 1, 1, None, None, None, None, None, 0.0, 0) == 0, \
            dnn_hip.last_error()

    def tap(self):
        index = ctypes.c_int(-7)
        return lib.dnn_plan_add_tap(self.h, ctypes.byref(index)), index.value

    def state(self):
        buf = ctypes.create_string_buffer(8192)
        assert lib.dnn_plan_describe(self.h, buf, 8192) == 0
        wb, sb = ctypes.c_size_t(), ctypes.c_size_t()
        assert lib.dnn_plan_memory(self.h, ctypes.byref(wb), ctypes.byref(sb)) == 0
        return buf.value.decode(), wb.value, sb.value, lib.dnn_plan_num_taps(self.h)

    def close(self):
        lib.dnn_plan_destroy(self.h)


def test_tap_misuse_fails_and_leaves_the_plan_unchanged():
    p = RawPlan(fp16=True)  # an fp16 plan: refused, the message names fp16 as the stash's does
    p.conv(3, 32)
    before = p.state()
    rc, index = p.tap()
    assert rc != 0 and "fp16" in dnn_hip.last_error() and index == -7 and p.state() == before
    p.close()

    p = RawPlan()  # a tap as the first entry: the current tensor is the plan's input
    before = p.state()
    rc, _ = p.tap()
    assert rc != 0 and "input" in dnn_hip.last_error() and p.state() == before
    slot = ctypes.c_int()
    assert lib.dnn_plan_add_stash(p.h, ctypes.byref(slot)) == 0  # ... also when a slot names the input
    before = p.state()
    assert p.tap()[0] != 0 and p.state() == before
    p.close()

    p = RawPlan()  # a fifth tap
    for k in range(4):
        p.conv(1, 8 * (k + 1))
        assert p.tap() == (0, k)
    h, w, c = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    for k in range(4):
        assert lib.dnn_plan_tap_shape(p.h, k, ctypes.byref(h), ctypes.byref(w), ctypes.byref(c)) == 0
        assert (h.value, w.value, c.value) == (8, 8, 8 * (k + 1))
    assert lib.dnn_plan_tap_shape(p.h, 4, ctypes.byref(h), ctypes.byref(w), ctypes.byref(c)) != 0
    assert lib.dnn_plan_num_taps(p.h) == 4
    p.conv(1, 8)
    before = p.state()
    rc, _ = p.tap()
    assert rc != 0 and "4 taps" in dnn_hip.last_error() and p.state() == before
    assert [l for l in before[0].splitlines() if l.startswith("tap")] == [f"tap 8x8x{8 * (k + 1)} index={k}"
                                                                          for k in range(4)]
    # not finalized: no buffer yet
    ptr, nb = ctypes.c_void_p(), ctypes.c_size_t()
    assert lib.dnn_plan_tap_buffer(p.h, 0, ctypes.byref(ptr), ctypes.byref(nb)) != 0
    p.close()


def test_tap_twice_on_one_tensor_and_on_a_stashed_tensor():
    p = RawPlan()
    p.conv(3, 16)
    slot = ctypes.c_int()
    assert lib.dnn_plan_add_stash(p.h, ctypes.byref(slot)) == 0
    one = p.state()[2]
    assert p.tap() == (0, 0) and p.tap() == (0, 1)  # both name the stash's region: no new memory
    assert p.state()[2] == one
    p.close()


def _memory(entries, B=2):
    return dnn_hip.Plan.memory(B, MC.IN_SHAPE, entries)


def test_tap_memory_is_the_tap_tensor():
    ce = RS.conv_entries(RC.exact_weights(MC.TAP_CHAIN_LAYERS, seed=1))
    with_tap = _memory([ce[0], dnn_hip.TapEntry(0), ce[1]])
    without = _memory([ce[0], ce[1]])
    assert with_tap[0] == without[0]
    assert with_tap[1] - without[1] == 2 * 8 * 8 * 32 * 4


def test_tap_region_is_never_handed_to_a_later_producer():
    """Four Add blocks alternate between two regions; with the first conv's output tapped, that
    region stays the tap's and the blocks need two more: one more region of the same size."""
    ws = RC.exact_weights(MC.churn_layers(), seed=5)
    tapped = dnn_hip.lower_graph(MC.churn_graph(2, ws))
    plain = dnn_hip.lower_graph(MC.churn_graph(2, ws, tap=False))
    assert MC.entry_kinds(tapped) == "CT" + "SCCAX" * 4 + "C" and MC.entry_kinds(plain) == "C" + "SCCAX" * 4 + "C"
    assert _memory(tapped)[1] - _memory(plain)[1] == 2 * 8 * 8 * 32 * 4
    two = dnn_hip.lower_graph(MC.churn_graph(2, RC.exact_weights(MC.churn_layers(2), seed=5), nblocks=2, tap=False))
    assert _memory(plain)[1] == _memory(two)[1]  # (without a tap more blocks need no more regions)


def test_a_plan_cannot_end_in_a_tap_entry_list():
    ce = RS.conv_entries(RC.exact_weights(MC.TAP_CHAIN_LAYERS, seed=1))
    g = MC.tap_chain_graph(2, RC.exact_weights(MC.TAP_CHAIN_LAYERS, seed=1))
    g.add_out_node(g.out_node)  # the primary output declared as an extra one too
    assert dnn_hip.lower_graph(g) is None
    assert dnn_hip.TapEntry(0).nodes == [] and ce[0].nodes


# ------------------------------------------------------------------------------ lowering
def test_small_graphs_lower_to_the_expected_entries():
    g = MC.tap_chain_graph(2, RC.exact_weights(MC.TAP_CHAIN_LAYERS, seed=1))
    assert MC.entry_kinds(dnn_hip.lower_graph(g)) == "CTC"
    g = MC.branch_graph(2, RC.exact_weights(MC.BRANCH_LAYERS, seed=1))
    es = dnn_hip.lower_graph(g)
    assert MC.entry_kinds(es) == "CSCTRXC"
    assert MC.numbers(es) == [("S", 0), ("T", 0), ("R", 0), ("X", 0)] and es[3].node is g.extra_out_nodes[0]


def test_mini_neck_lowering():
    g = MC.neck_graph(2, RC.exact_weights(MC.NECK_LAYERS, seed=1))
    es = dnn_hip.lower_graph(g)
    assert MC.entry_kinds(es) == MC.NECK_KINDS
    assert MC.numbers(es) == MC.NECK_NUMBERS
    assert MC.max_live_slots(es) == 2
    route = [e for e in es if isinstance(e, dnn_hip.RouteEntry)][0]
    assert route.block == 1 and not route.slot_first  # the upsampled tensor comes first, x second
    assert _memory(es)[1] > 0
    # without the declaration the head branch is a dead end: not a plan
    g.extra_out_nodes.clear()
    assert dnn_hip.lower_graph(g) is None


def test_long_skip_with_the_skipped_tensor_first():
    ws = RC.exact_weights(MC.NESTED_SKIPS_LAYERS, seed=1)
    g = dnn_hip.DnnGraphBuilder()
    x = MC._conv(g, g.create_input([2] + list(MC.IN_SHAPE)), ws[0])
    t = MC._conv(g, x, ws[0])
    t = g.create_add([t, MC._conv(g, MC._conv(g, t, ws[1]), ws[2])])
    g.set_out_node(MC._conv(g, g.create_concat([x, t]), ws[3]))
    es = dnn_hip.lower_graph(g)
    assert MC.entry_kinds(es) == "CSCSCCAXJXC"
    assert MC.numbers(es) == [("S", 0), ("S", 1), ("A", 1), ("X", 1), ("J", 0), ("X", 0)]
    assert [e for e in es if isinstance(e, dnn_hip.RouteEntry)][0].slot_first


def test_yolov3_graph_lowers_to_one_plan():
    w = yolov3.validate(synth.yolov3_weights(width_div=8, n_out=24), 24)
    g, nodes, outs = yolov3.build_graph(dnn_hip.DnnGraphBuilder, w, in_shape=(2, 64, 64, 3))
    assert g.extra_out_nodes == outs[:2] and g.out_node is outs[2]
    assert [tuple(o.result.shape) for o in outs] == [(2, 2, 2, 24), (2, 4, 4, 24), (2, 8, 8, 24)]
    es = dnn_hip.lower_graph(g)
    kinds = MC.entry_kinds(es)
    assert {k: kinds.count(k) for k in "CAUJT"} == {"C": 75, "A": 23, "U": 2, "J": 2, "T": 2}
    assert kinds.count("S") == kinds.count("X") and MC.max_live_slots(es) == 3
    assert [e.node for e in es if isinstance(e, dnn_hip.TapEntry)] == outs[:2]
    assert all(not e.slot_first for e in es if isinstance(e, dnn_hip.RouteEntry))
    # darknet53's trunk lowers inside it as it does alone, up to the two long-skip stashes
    wd = darknet53.validate(synth.darknet53_weights(width_div=8, n_out=24))
    alone = MC.entry_kinds(dnn_hip.lower_graph(darknet53.build_graph(dnn_hip.DnnGraphBuilder, wd, (2, 64, 64, 3))[0]))
    trunk = kinds[:kinds.index("T")]
    assert trunk.replace("XSCS", "XCS", 2).startswith(alone[:-7])
    wb, sb = dnn_hip.Plan.memory(2, (64, 64, 3), es)
    assert wb > 0 and sb > 0


def test_existing_models_lower_as_on_the_parent_commit():
    """Kind strings and slot numbers recorded from the parent commit's lower_graph
    (tests/golden/lowering_parent.json)."""
    with open(os.path.join(HERE, "golden", "lowering_parent.json")) as f:
        want = json.load(f)
    graphs = {
        "yolov2tiny": yolo_graph.build_graph(dnn_hip.DnnGraphBuilder, synth.yolo_weights())[0],
        "yolov2": yolov2.build_graph(dnn_hip.DnnGraphBuilder, yolov2.validate(synth.yolov2_weights(width_div=8, n_out=40)),
                                     in_shape=(1, 64, 64, 3))[0],
        "darknet53": darknet53.build_graph(dnn_hip.DnnGraphBuilder,
                                           darknet53.validate(synth.darknet53_weights(width_div=8, n_out=24)),
                                           in_shape=(1, 64, 64, 3))[0],
    }
    assert sorted(graphs) == sorted(want)
    for name, g in graphs.items():
        es = dnn_hip.lower_graph(g)
        assert MC.entry_kinds(es) == want[name]["kinds"], name
        assert [s for _, s in MC.numbers(es)] == want[name]["slots"], name
    for build, layers in ((RS.top_down_graph, RS.TOP_DOWN_LAYERS), (RC.two_joins_graph, RC.TWO_JOINS_LAYERS),
                          (RC.empty_branch_graph, RC.EMPTY_BRANCH_LAYERS)):
        assert "T" not in MC.entry_kinds(dnn_hip.lower_graph(build(2, RC.exact_weights(layers))))
    assert MC.entry_kinds(dnn_hip.lower_graph(RC.two_joins_graph(2, RC.exact_weights(RC.TWO_JOINS_LAYERS)))) \
        == "CSCSRCJCSPCSRCJC"


def test_unsupported_patterns_return_none():
    assert dnn_hip.lower_graph(MC.long_skip_add_graph(2, RC.exact_weights(MC.LONG_SKIP_ADD_LAYERS))) is None
    ws = RC.exact_weights(MC.NESTED_SKIPS_LAYERS)
    es = dnn_hip.lower_graph(MC.nested_skips_graph(1, ws, 3))
    assert es is not None and MC.max_live_slots(es) == 4
    assert dnn_hip.Plan.memory(1, MC.IN_SHAPE, es)[1] > 0
    assert dnn_hip.lower_graph(MC.nested_skips_graph(1, ws, 4)) is None  # a fifth live slot


# ------------------------------------------------------------------------------ run_all
class _FakePlan(object):
    def __init__(self, entries, outs):
        self.tap_entries = [e for e in entries if isinstance(e, dnn_hip.TapEntry)]
        self.outs = outs

    def run_host_all(self, x):
        return list(self.outs)


def test_run_all_order_is_extras_then_primary():
    """The branch graph with its two extra outputs declared against the order in which the plan
    computes them: run_all gives declaration order, then the primary output, on the plan path
    (the plan mocked: no GPU) and on the node-by-node path (the nodes' run() mocked)."""
    ws = RC.exact_weights(MC.BRANCH_LAYERS, seed=1)
    g = dnn_hip.DnnGraphBuilder()
    x = MC._conv(g, g.create_input([2] + list(MC.IN_SHAPE)), ws[0])
    a = MC._conv(g, x, ws[1])
    g.set_out_node(MC._conv(g, x, ws[2]))
    g.add_out_node(a)
    g.add_out_node(x)
    es = dnn_hip.lower_graph(g)
    assert MC.entry_kinds(es) == "CTSCTRXC"
    assert [e.node for e in es if isinstance(e, dnn_hip.TapEntry)] == [x, a]  # plan order: x first
    eng = dnn_hip.DnnInferenceEngine(g, False, device=0)
    eng._plan = _FakePlan(es, ["tap0 is x", "tap1 is a", "primary"])
    assert eng.run_all(np.zeros([2] + list(MC.IN_SHAPE), np.float32)) == ["tap1 is a", "tap0 is x", "primary"]
    assert (a.result, x.result, g.out_node.result) == ("tap1 is a", "tap0 is x", "primary")
    # node by node (debug): every node's run() replaced by a marker
    eng = dnn_hip.DnnInferenceEngine(g, True, device=0)
    eng.save_dir = os.devnull
    for n in RC.topo_nodes(MC._View(g, a)) + RC.topo_nodes(g):
        n.run = (lambda n=n: setattr(n, "result", np.full(1, id(n) % 1000, np.float32)))
    import unittest.mock
    with unittest.mock.patch("os.makedirs"), unittest.mock.patch("numpy.save"):
        got = eng.run_all(np.zeros([2] + list(MC.IN_SHAPE), np.float32))
    assert [float(v[0]) for v in got] == [id(a) % 1000, id(x) % 1000, id(g.out_node) % 1000]


# ------------------------------------------------------------------------------ yolov3.validate
def test_yolov3_validate_refuses_wrong_structures():
    ws = synth.yolov3_weights(width_div=8, n_out=24)
    assert len(ws) == yolov3.N_LAYERS == 75 and len(yolov3.structure()) == 75
    assert len(yolov3.validate(ws, 24)) == 75
    assert synth.weights_digest(ws[:52]) == synth.weights_digest(synth.darknet53_weights(width_div=8)[:52])
    E = yolo_weights.WeightFileError
    with pytest.raises(E):
        yolov3.validate(ws[:-1])
    with pytest.raises(E):
        yolov3.validate(ws + ws[-1:])
    with pytest.raises(E):
        yolov3.validate(ws, 27)

    def changed(i, **kw):
        out = list(ws)
        out[i] = dict(ws[i], **kw)
        return out

    k = ws[52]["kernel"]  # the first neck conv: 1x1
    with pytest.raises(E):
        yolov3.validate(changed(52, kernel=np.zeros((3, 3) + k.shape[2:], np.float32)))
    k = ws[57]["kernel"]  # the stride-32 branch's 3x3 conv
    with pytest.raises(E):
        yolov3.validate(changed(57, kernel=np.zeros((1, 1) + k.shape[2:], np.float32)))
    k = ws[60]["kernel"]  # the first conv after the first concat: reduce + stage 4 channels
    with pytest.raises(E):
        yolov3.validate(changed(60, kernel=np.zeros(k.shape[:2] + (k.shape[2] - 1, k.shape[3]), np.float32)))
    k = ws[59]["kernel"]  # the reduce conv reads the fifth neck conv, not the head
    with pytest.raises(E):
        yolov3.validate(changed(59, kernel=np.zeros(k.shape[:2] + (24, k.shape[3]), np.float32)))
    k = ws[66]["kernel"]  # the stride-16 head must have the stride-32 head's outputs
    bad = changed(66, kernel=np.zeros(k.shape[:3] + (21,), np.float32), biases=np.zeros(21, np.float32))
    with pytest.raises(E):
        yolov3.validate(bad, 24)
    with pytest.raises(E):
        yolov3.validate(changed(3, kernel=ws[3]["kernel"][..., :-1]))  # the trunk: darknet53's checks
    with pytest.raises(ValueError):
        yolov3.YOLO_V3([1, 416, 400, 3], ws, False)
