"""Plans with taps on the GPU: the graphs of tests/multi_out_cases.py in exact integer arithmetic
on poisoned, guarded caller buffers (taps and primary output bit-equal to the float64 oracle, in
batch and in latency mode), a tap beside the stash / release churn of residual blocks, n < batch,
graph replay, and the narrow YOLOv3 model against the oracle."""
import numpy as np
import pytest

import dnn_hip
import multi_out_cases as MC
import plan_fuzz_checks as K
import ref_numpy as R
import residual_cases as RS
import route_cases as RC
import synth

pytestmark = pytest.mark.gpu

NET_TOL = 1e-4  # normwise, end to end (the suite's existing bar, tests/test_gpu_residual.py)

CASES = {
    # name: (layers, graph builder, entry kinds)
    "tap_chain": (MC.TAP_CHAIN_LAYERS, MC.tap_chain_graph, "CTC"),       # (a)
    "branch": (MC.BRANCH_LAYERS, MC.branch_graph, "CSCTRXC"),            # (b)
    "neck": (MC.NECK_LAYERS, MC.neck_graph, MC.NECK_KINDS),              # (c)
}


def _case(name, B, seed=6):
    layers, build, kinds = CASES[name]
    g = build(B, RC.exact_weights(layers, seed=5))
    x = RC.exact_input(np.random.default_rng(seed), (B,) + MC.IN_SHAPE)
    want = MC.oracle_outputs(g, x)
    for w in want:
        assert np.array_equal(w, np.round(w)) and 4 < np.abs(w).max() < 1 << 20
    entries = dnn_hip.lower_graph(g)
    assert MC.entry_kinds(entries) == kinds
    return g, x, want, entries


def _check_taps(gp, g, n, want, what, **kw):
    """Every tap of the guarded plan against the oracle's value of the node it taps."""
    extras = list(g.extra_out_nodes)
    assert len(gp.plan.tap_entries) == len(extras) == len(gp.plan.tap_shapes)
    for k, e in enumerate(gp.plan.tap_entries):
        ref = want[[id(n_) for n_ in extras].index(id(e.node))]
        assert gp.plan.tap_shapes[k] == ref.shape[1:]
        K.check_bits(MC.read_tap(gp, k, n, **kw), ref[:n], f"{what}: tap {k}")


@pytest.mark.parametrize("latency", [False, True], ids=["batch", "latency"])
@pytest.mark.parametrize("name", list(CASES))
def test_exact_plan_with_taps(name, latency):
    B = 2
    g, x, want, entries = _case(name, B)
    gp = RS.GuardedPlan(B, MC.IN_SHAPE, entries, latency=latency)
    try:
        assert sum(l.startswith("tap ") for l in gp.plan.describe().splitlines()) == len(g.extra_out_nodes)
        y = gp.run(x, name)
        K.check_bits(y, want[-1], f"{name}: primary output vs the float64 oracle")
        _check_taps(gp, g, B, want, name)
    finally:
        gp.close()
    if latency:
        return
    # the engine: run_all on the plan path and node by node
    eng = dnn_hip.DnnInferenceEngine(g, False, device=0)
    outs = eng.run_all(x)
    assert eng._plan is not None and len(outs) == len(want)
    for o, w in zip(outs, want):
        K.check_bits(o, w, f"{name}: run_all on the plan")
    K.check_bits(eng.run(x), want[-1], f"{name}: run")
    dbg = dnn_hip.DnnInferenceEngine(g, False, device=0)
    g.in_node.set_input(x)
    primary = dbg._run_nodes()
    for o, w in zip([n.result for n in g.extra_out_nodes] + [primary], want):
        K.check_bits(o, w, f"{name}: node by node")


def test_tap_survives_the_churn_of_later_blocks():
    """(d) conv, tap, four Add blocks (stash, two convs, shortcut, release each), conv: the blocks
    alternate between two regions that are not the tap's, and the tap read after the run is the
    first conv's output."""
    B = 2
    ws = RC.exact_weights(MC.churn_layers(), seed=5)
    g = MC.churn_graph(B, ws)
    x = RC.exact_input(np.random.default_rng(6), (B,) + MC.IN_SHAPE)
    want = MC.oracle_outputs(g, x)
    entries = dnn_hip.lower_graph(g)
    assert MC.entry_kinds(entries) == "CT" + "SCCAX" * 4 + "C"
    for latency in (False, True):
        gp = RS.GuardedPlan(B, MC.IN_SHAPE, entries, latency=latency)
        try:
            K.check_bits(gp.run(x, "churn"), want[-1], "churn: primary output")
            _check_taps(gp, g, B, want, "churn")
            K.check_bits(gp.run(x[:1], "churn n=1"), want[-1][:1], "churn: n=1")
            _check_taps(gp, g, 1, want, "churn n=1")
        finally:
            gp.close()


@pytest.mark.parametrize("name", ["branch", "neck"])
def test_n_below_batch_writes_only_n_images_of_a_tap(name):
    """(e) a batch-3 plan that only ever runs 2 images: the third image's part of every tap region
    keeps the workspace's poison."""
    B, n = 3, 2
    g, x, want, entries = _case(name, B)
    gp = RS.GuardedPlan(B, MC.IN_SHAPE, entries)
    try:
        y = gp.run(x[:n], f"{name} n=2 of 3")
        K.check_bits(y, want[-1][:n], f"{name}: n=2 of 3, primary output")
        _check_taps(gp, g, n, want, f"{name} n=2 of 3", fresh_tail=True)
    finally:
        gp.close()


def test_graph_replay_fills_the_same_tap_buffers():
    """(f) dnn_plan_run_graph replayed on two inputs gives the taps and the output dnn_plan_run
    gives, and the tap addresses do not move."""
    B = 2
    g, x, want, entries = _case("neck", B)
    x2 = RC.exact_input(np.random.default_rng(7), (B,) + MC.IN_SHAPE)
    want2 = MC.oracle_outputs(g, x2)
    assert not np.array_equal(want[0], want2[0])
    gp = RS.GuardedPlan(B, MC.IN_SHAPE, entries)
    try:
        addr = [gp.plan.tap_buffer(k) for k in range(len(gp.plan.tap_shapes))]
        for xi, wi, what in ((x, want, "eager 1"), (x2, want2, "eager 2")):
            K.check_bits(gp.run(xi, what), wi[-1], f"{what}: primary output")
            _check_taps(gp, g, B, wi, what)
        for xi, wi, what in ((x, want, "graph 1"), (x2, want2, "graph replay"), (x, want, "graph replay 2")):
            K.check_bits(gp.run(xi, what, how="graph"), wi[-1], f"{what}: primary output")
            _check_taps(gp, g, B, wi, what)
            assert [gp.plan.tap_buffer(k) for k in range(len(addr))] == addr
    finally:
        gp.close()


def test_hand_built_plan_with_two_taps_of_one_tensor_and_run_host_all():
    ws = RC.exact_weights(MC.TAP_CHAIN_LAYERS, seed=5)
    ce = RS.conv_entries(ws)
    x = RC.exact_input(np.random.default_rng(3), (2,) + MC.IN_SHAPE)
    t = RS.conv_ref(x, ws[0])
    plan = dnn_hip.Plan(2, MC.IN_SHAPE, [ce[0], dnn_hip.StashEntry(0), dnn_hip.TapEntry(0), dnn_hip.TapEntry(1),
                                        dnn_hip.ReleaseEntry(0), ce[1]], device=0)
    try:
        assert plan.tap_shapes == [(8, 8, 32)] * 2 and plan.tap_buffer(0) == plan.tap_buffer(1)
        t0, t1, y = plan.run_host_all(x)
        K.check_bits(t0, t, "tap 0")
        K.check_bits(t1, t, "tap 1")
        K.check_bits(y, RS.conv_ref(t, ws[1]), "output")
        assert [a.shape[0] for a in plan.run_host_all(x[:1])] == [1, 1, 1]
        # a finalized plan takes no more taps, and stays as it is
        import ctypes
        before = plan.describe()
        index = ctypes.c_int(-7)
        assert dnn_hip.mylib.dnn_plan_add_tap(plan.h, ctypes.byref(index)) != 0 and index.value == -7
        assert "finalized" in dnn_hip.last_error()
        assert plan.describe() == before and dnn_hip.mylib.dnn_plan_num_taps(plan.h) == 2
        K.check_bits(plan.run_host_all(x)[2], y, "output after the refused tap")
    finally:
        plan.close()
    with pytest.raises(dnn_hip.DnnHipError, match="ends in a tap"):
        dnn_hip.Plan(2, MC.IN_SHAPE, [ce[0], dnn_hip.TapEntry(0)], device=0)


# ------------------------------------------------------------------------------ narrow YOLOv3
def test_narrow_yolov3_against_the_oracle():
    """Narrow YOLOv3 (width_div 8, 3 x (5 + 3) outputs) on 64 x 64 frames at batch 2: grids 2, 4
    and 8.  Each output within NET_TOL normwise of the float64 oracle; each image's rows
    bit-identical to a batch-1 plan's."""
    import yolov3
    ws = synth.yolov3_weights(width_div=8, n_out=3 * (5 + 3))
    m = yolov3.YOLO_V3([2, 64, 64, 3], ws, False)
    x = synth.frames([0, 1], shape=(64, 64, 3))
    outs = [o.copy() for o in m.inference(x)]
    assert m.sess._plan is not None
    assert [o.shape for o in outs] == [(2, 2, 2, 24), (2, 4, 4, 24), (2, 8, 8, 24)]
    lines = m.sess.plan().describe().splitlines()
    assert sum(l.startswith("conv ") for l in lines) == 75 and sum(l.startswith("tap ") for l in lines) == 2
    assert sum(l.startswith("route ") for l in lines) == 2 and sum(l.startswith("upsample ") for l in lines) == 2
    want = MC.oracle_outputs(m.g, x)
    for o, w_, stride in zip(outs, want, (32, 16, 8)):
        K.check_finite(o, f"narrow YOLOv3 stride {stride}")
        assert 0.01 < float(np.abs(w_).mean()) < 100
        err = R.normwise_err(o, w_)
        print(f"narrow YOLOv3 stride {stride}: plan vs float64 oracle, normwise error {err:.3e}")
        assert err < NET_TOL, f"narrow YOLOv3 stride {stride}: normwise error {err:.3e} >= {NET_TOL:.0e}"
    m1 = yolov3.YOLO_V3([1, 64, 64, 3], ws, False)
    for i in range(2):
        for o, o1, stride in zip(outs, m1.inference(x[i:i + 1]), (32, 16, 8)):
            K.check_bits(o1, o[i:i + 1], f"narrow YOLOv3 stride {stride}: image {i} of batch 2 vs a batch-1 plan")
