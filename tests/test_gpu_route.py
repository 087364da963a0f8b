"""The route kernel and fork/join plans on the GPU: the kernel alone (bit-exact data movement),
a fork/join plan in exact integer arithmetic (bit-exact against the float64 oracle in every
mode), the same plan with random weights (the suite's tolerances), the Python engine path, the
narrow YOLOv2 model, and the unchanged YOLOv2-tiny plan."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

import dnn_hip
import plan_fuzz_checks as K
import ref_numpy as R
import route_cases as RC
import synth
import yolo_graph

pytestmark = pytest.mark.gpu

DEV = "cuda"
NET_TOL = 1e-4  # normwise, end to end (the suite's existing bar)


# ------------------------------------------------------------------------------ 1. the kernel
ROUTE_CASES = [
    (2, 4, 6, 4, 2, 8, 0),        # the 16-byte path
    (2, 4, 6, 3, 2, 5, 1),        # the scalar path
    (1, 8, 8, 8, 4, 0, 0),        # a pure space_to_depth, block 4
    (3, 5, 7, 12, 1, 20, 0),      # a pure concat on odd sizes
    (1, 26, 26, 64, 2, 1024, 0),  # the YOLOv2 join
    (5, 26, 26, 64, 2, 1024, 1),  # many workgroups with a tail
]


def _arange_inputs(n, h, w, ca, block, cb):
    a = np.arange(n * h * w * ca, dtype=np.float32).reshape(n, h, w, ca)
    b = None
    if cb:
        nb = n * (h // block) * (w // block) * cb
        b = (a.size + np.arange(nb, dtype=np.float32)).reshape(n, h // block, w // block, cb)
        assert a.size + nb < 1 << 24  # every value distinct and exact in fp32
    return a, b


@pytest.mark.parametrize("case", ROUTE_CASES, ids=lambda c: "x".join(map(str, c)))
def test_route_kernel_bit_exact(case):
    n, h, w, ca, block, cb, b_first = case
    a, b = _arange_inputs(n, h, w, ca, block, cb)
    want = RC.route(a, b, block, bool(b_first))
    out = np.full(want.shape, np.nan, np.float32)
    rc = dnn_hip.mylib.dnn_route_host(dnn_hip._vp(a), dnn_hip._vp(b), dnn_hip._vp(out), n, h, w, ca, block, cb, b_first)
    assert rc == 0, dnn_hip.last_error()
    K.check_bits(out, want, f"route {case}")


def test_route_host_refuses_bad_arguments():
    a = np.zeros((1, 6, 6, 4), np.float32)
    out = np.zeros((1, 3, 3, 16), np.float32)
    for block in (0, 9, 4):
        assert dnn_hip.mylib.dnn_route_host(dnn_hip._vp(a), None, dnn_hip._vp(out), 1, 6, 6, 4, block, 0, 0) != 0
        assert dnn_hip.last_error() != ""
    assert dnn_hip.mylib.dnn_route_host(dnn_hip._vp(a), None, dnn_hip._vp(out), 1, 6, 6, 4, 2, 8, 0) != 0  # cb without b


class GuardedEntries(object):
    """A plan from entries on caller-owned, poisoned, guarded buffers (as test_gpu_plan_fuzz.py)."""

    def __init__(self, B, shape, entries, **kw):
        wb, sb = dnn_hip.Plan.memory(B, shape, entries, **kw)
        self.wbuf = torch.full((wb + 2 * K.GUARD_BYTES,), K.POISON, dtype=torch.uint8, device=DEV)
        self.sbuf = torch.full((sb + 2 * K.GUARD_BYTES,), K.POISON, dtype=torch.uint8, device=DEV)
        torch.cuda.synchronize()
        self.plan = dnn_hip.Plan(B, shape, entries, device=0, weights_ptr=self.wbuf.data_ptr() + K.GUARD_BYTES,
                                 workspace_ptr=self.sbuf.data_ptr() + K.GUARD_BYTES, **kw)
        self.B, self.shape = B, tuple(shape)
        self.in_floats = int(np.prod(shape))
        self.row = int(np.prod(self.plan.out_shape))
        self.xin = torch.empty(2 * K.GUARD_FLOATS + B * self.in_floats, dtype=torch.float32, device=DEV)
        self.out = torch.empty(2 * K.GUARD_FLOATS + B * self.row, dtype=torch.int32, device=DEV)
        self.stream = torch.cuda.Stream()

    def run(self, x, what, how="run"):
        n = x.shape[0]
        assert n <= self.B and tuple(x.shape[1:]) == self.shape
        self.xin.fill_(float("nan"))
        self.xin[K.GUARD_FLOATS:K.GUARD_FLOATS + n * self.in_floats] = torch.from_numpy(x.reshape(-1)).to(DEV)
        self.out.fill_(K.CANARY)
        torch.cuda.synchronize()
        pin, pout = self.xin.data_ptr() + 4 * K.GUARD_FLOATS, self.out.data_ptr() + 4 * K.GUARD_FLOATS
        if how == "graph":
            self.plan.run_graph(n, pin, pout, self.stream.cuda_stream)
        else:
            self.plan.run_device(n, pin, pout)
        torch.cuda.synchronize()
        flat = self.out.cpu().numpy()
        K.check_canary(flat, n, self.row, self.B, f"{what}: output")
        for name, buf in (("workspace", self.sbuf), ("weight arena", self.wbuf)):
            ends = torch.cat([buf[:K.GUARD_BYTES], buf[-K.GUARD_BYTES:]]).cpu().numpy()
            K.check_guard(ends, f"{what}: {name}")
        y = flat[K.GUARD_FLOATS:K.GUARD_FLOATS + n * self.row].view(np.float32)
        y = y.reshape((n,) + self.plan.out_shape).copy()
        K.check_finite(y, what)
        return y

    def close(self):
        self.plan.close()


def test_route_through_a_guarded_plan():
    """The kernel as a plan entry on poisoned buffers: a pure space_to_depth, and a concat whose
    b is the stashed input (the caller's tensor); n < batch leaves the other output rows alone."""
    B, n = 3, 2
    a, _ = _arange_inputs(n, 8, 8, 8, 4, 0)
    gp = GuardedEntries(B, (8, 8, 8), [dnn_hip.RouteEntry(4)])
    try:
        assert [k["name"] for k in gp.plan.kernels()] == ["route0"]
        K.check_bits(gp.run(a, "s2d plan"), RC.route(a, None, 4), "s2d plan")
    finally:
        gp.close()
    a, _ = _arange_inputs(n, 5, 7, 12, 1, 0)
    gp = GuardedEntries(B, (5, 7, 12), [dnn_hip.StashEntry(0), dnn_hip.RouteEntry(1, 0, True)])
    try:
        K.check_bits(gp.run(a, "concat plan"), RC.route(a, a, 1, True), "concat plan")
    finally:
        gp.close()


# ------------------------------------------------------------------------------ 2. exact fork/join
@pytest.fixture(scope="module")
def exact_case():
    ws = RC.fork_join_weights("exact")
    g = RC.fork_join_graph(4, ws)
    x = RC.exact_input(np.random.default_rng(1), (4,) + RC.FORK_JOIN_IN)
    want = RC.oracle_graph(g, x, acc=np.float64)
    assert np.abs(want).max() < 2048 and np.array_equal(want, np.round(want))
    want.setflags(write=False)
    return ws, x, want


@pytest.mark.parametrize("latency", [False, True], ids=["batch", "latency"])
def test_fork_join_plan_exact(exact_case, latency):
    ws, x, want = exact_case
    plans = {}
    try:
        for B in (1, 4):
            entries = dnn_hip.lower_graph(RC.fork_join_graph(B, ws))
            assert RC.entry_kinds(entries) == "CSPCSRCJCC"
            plans[B] = GuardedEntries(B, RC.FORK_JOIN_IN, entries, latency=latency)
        d = plans[4].plan.describe()
        assert "route 16x16x32 -> 8x8x256 block=2 slot=1 (8x8x128) last" in d, d
        # the 3x3 conv after the route reads plain fp32: the implicit fp32-MFMA GEMM
        assert "conv 8x8x256 -> 8x8x64 k3x3 s1 mode=implicit" in d, d
        y4 = plans[4].run(x, "B=4")
        K.check_bits(y4, want, f"B=4 latency={latency} vs the float64 oracle")
        for i in range(4):
            y1 = plans[1].run(x[i:i + 1], f"B=1 row {i}")
            K.check_bits(y1, want[i:i + 1], f"B=1 row {i} latency={latency} vs the float64 oracle")
            K.check_bits(y1[0], y4[i], f"B=1 run of row {i} vs the B=4 run")
        K.check_bits(plans[4].run(x, "B=4 again"), y4, "second run")
        K.check_bits(plans[4].run(x[:3], "n=3 of 4"), y4[:3], "n < batch")
        K.check_bits(plans[4].run(x, "graph", how="graph"), y4, "run_graph")
        K.check_bits(plans[4].run(x, "graph replay", how="graph"), y4, "run_graph replay")
        K.check_bits(plans[1].run(x[2:3], "B=1 graph", how="graph"), y4[2:3], "B=1 run_graph")
    finally:
        for gp in plans.values():
            gp.close()


def test_fork_join_per_kernel_timing(exact_case):
    """Timing events work around the route kernel like any other; stash / restore add no kernel."""
    ws, x, want = exact_case
    entries = dnn_hip.lower_graph(RC.fork_join_graph(4, ws))
    plan = dnn_hip.Plan(4, RC.FORK_JOIN_IN, entries, device=0)
    try:
        names = [k["name"] for k in plan.kernels()]
        assert "route0" in names and not any("stash" in n or "restore" in n for n in names)
        plan.timing_begin(2)
        for _ in range(2):
            K.check_bits(plan.run_host(x), want, "timed run")
        ms, cnt = plan.timing_end()
        assert cnt == [2] * len(names) and all(m > 0 for m in ms)
        plan.timing_begin(1, only="route0")
        plan.run_host(x)
        ms, cnt = plan.timing_end()
        assert [c for c in cnt] == [1 if n == "route0" else 0 for n in names]
    finally:
        plan.close()


# ------------------------------------------------------------------------------ 3. random weights
def test_fork_join_plan_random_weights():
    ws = RC.fork_join_weights("random")
    B = 4
    g = RC.fork_join_graph(B, ws)
    x = np.random.default_rng(2).standard_normal((B,) + RC.FORK_JOIN_IN).astype(np.float32)
    val = RC.oracle_graph(g, x, keep=True)
    want = val[g.out_node]
    join = [n for n in val if isinstance(n, dnn_hip.Concat)][0]
    for latency in (False, True):
        gp = GuardedEntries(B, RC.FORK_JOIN_IN, dnn_hip.lower_graph(g), latency=latency)
        try:
            y = gp.run(x, f"random latency={latency}")
        finally:
            gp.close()
        err = R.normwise_err(y, want)
        print(f"fork/join random weights latency={latency}: normwise error {err:.3e}")
        assert err < NET_TOL, f"latency={latency}: normwise error {err:.3e} >= {NET_TOL:.0e}"
        # the layer after the route, fed the oracle's route output
        g1 = dnn_hip.DnnGraphBuilder()
        t = RC._conv(g1, g1.create_input([B, 8, 8, 256]), ws[3])
        g1.set_out_node(t)
        gp = GuardedEntries(B, (8, 8, 256), dnn_hip.lower_graph(g1), latency=latency)
        try:
            y1 = gp.run(val[join], "layer after the route")
        finally:
            gp.close()
        e1 = K.check_layer_err(y1, RC.oracle_graph(g1, val[join]), K.LAYER_TOL, f"layer after the route latency={latency}")
        print(f"layer after the route latency={latency}: normwise error {e1:.3e}")


# ------------------------------------------------------------------------------ 4. Python path
def test_engine_runs_the_plan_and_equals_the_node_path(exact_case, tmp_path, monkeypatch):
    ws, x, want = exact_case
    monkeypatch.chdir(tmp_path)  # debug=True saves ./intermediate/layer_k.npy
    eng = dnn_hip.DnnInferenceEngine(RC.fork_join_graph(4, ws), False, device=0)
    y = eng.run(x)
    assert eng._plan is not None
    assert "route " in eng.plan().describe()
    names = [k["name"] for k in eng.plan().kernels()]
    assert "route0" in names and not any("stash" in n for n in names)
    K.check_bits(y, want, "engine (plan)")
    dbg = dnn_hip.DnnInferenceEngine(RC.fork_join_graph(4, ws), True, device=0)
    yd = dbg.run(x)
    assert dbg._plan is None and os.path.exists(tmp_path / "intermediate" / "layer_1.npy")
    K.check_bits(yd, y, "engine: node by node vs plan")


@pytest.mark.parametrize("which", ["empty_branch", "two_joins"])
def test_engine_other_topologies(which):
    layers, build = {"empty_branch": (RC.EMPTY_BRANCH_LAYERS, RC.empty_branch_graph),
                     "two_joins": (RC.TWO_JOINS_LAYERS, RC.two_joins_graph)}[which]
    ws = RC.exact_weights(layers, seed=3)
    B = 2
    g = build(B, ws)
    x = RC.exact_input(np.random.default_rng(4), (B, 8, 8, 32))
    want = RC.oracle_graph(g, x)
    assert np.array_equal(want, np.round(want)) and np.abs(want).max() < 1 << 20
    eng = dnn_hip.DnnInferenceEngine(g, False, device=0)
    y = eng.run(x)
    assert eng._plan is not None and "route" in eng.plan().describe()
    K.check_bits(y, want, which)


# ------------------------------------------------------------------------------ 5. narrow YOLOv2
def test_narrow_yolov2_against_the_oracle():
    import yolov2
    ws = synth.yolov2_weights(width_div=4)
    m = yolov2.YOLO_V2([2, 64, 64, 3], ws, False)
    x = synth.frames([0, 1], shape=(64, 64, 3))
    y = m.inference(x)
    assert m.sess._plan is not None and y.shape == (2, 2, 2, 425)
    want = RC.oracle_graph(m.g, x)
    K.check_finite(y, "narrow YOLOv2")
    err = R.normwise_err(y, want)
    print(f"narrow YOLOv2: normwise error {err:.3e}")
    assert err < NET_TOL, f"narrow YOLOv2: normwise error {err:.3e} >= {NET_TOL:.0e}"
    for i in range(2):
        boxes = m.postprocessing(y[i:i + 1])
        assert isinstance(boxes, list)


# ------------------------------------------------------------------------------ 6. nothing else moved
def test_yolov2_tiny_plan_is_the_parents():
    """describe() and kernels() of the default batch-64 YOLOv2-tiny plan equal the strings
    captured from the library as it was before the fork/join entries existed."""
    with open(os.path.join(GOLDEN, "route_parent_plan.json")) as f:
        gold = json.load(f)
    g, _ = yolo_graph.build_graph(dnn_hip.DnnGraphBuilder, synth.yolo_zero_weights(), in_shape=(64, 416, 416, 3))
    entries = dnn_hip.lower_graph(g)
    assert (gold["weight_bytes"], gold["workspace_bytes"]) == dnn_hip.Plan.memory(64, (416, 416, 3), entries)
    plan = dnn_hip.Plan(64, (416, 416, 3), entries, device=0)
    try:
        assert plan.describe() == gold["describe"]
        assert plan.kernels() == gold["kernels"]
    finally:
        plan.close()
