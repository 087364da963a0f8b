"""The shortcut and upsample kernels and residual / top-down plans on the GPU: the kernels alone
(bit-exact against numpy), plans in exact integer arithmetic on poisoned, guarded buffers (bit-exact
against the float64 oracle and the node-by-node path), n < batch, graph replay, latency plans and
per-kernel timing, and the narrow Darknet-53 model."""
import numpy as np
import pytest

import dnn_hip
import plan_fuzz_checks as K
import ref_numpy as R
import residual_cases as RS
import route_cases as RC
import synth

pytestmark = pytest.mark.gpu

NET_TOL = 1e-4  # normwise, end to end (the suite's existing bar)
lib = dnn_hip.mylib


# ------------------------------------------------------------------------------ 1. the kernels
SPECIAL = np.array([0.0, -0.0, 1e-40, -1e-40, 1.1754944e-38, -1.1754944e-38, 3e38, -3e38, 1e30, -1e30, 1.0, -1.0,
                    0.1, -0.1, 16777216.0, -7.5], np.float32)

SHORTCUT_SHAPES = [
    (1, 3, 5, 7),          # 105 = 4 * 26 + 1
    (2, 4, 4, 8),          # a multiple of 4
    (1, 3, 3, 1),          # 4k + 1
    (1, 1, 2, 5),          # 4k + 2
    (1, 1, 1, 3),          # the scalar loop alone
    (1, 1, 1, 11),         # 4k + 3
    (1, 1, 3, 3500003),    # more than one pass of the launch grid: the unrolled loop, its remainder, a tail
]


def _shortcut_inputs(shape, seed):
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    a = rng.standard_normal(n).astype(np.float32)
    b = rng.standard_normal(n).astype(np.float32)
    # every pair of special values (negative, zero, denormal, large), wherever it fits
    pa, pb = np.meshgrid(SPECIAL, SPECIAL)
    m = min(n, pa.size)
    at = rng.choice(n, size=m, replace=False)
    a[at], b[at] = pa.reshape(-1)[:m], pb.reshape(-1)[:m]
    return a.reshape(shape), b.reshape(shape)


@pytest.mark.parametrize("leaky", [0, 1, 2])
@pytest.mark.parametrize("shape", SHORTCUT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_shortcut_kernel_bit_exact(shape, leaky):
    a, b = _shortcut_inputs(shape, seed=len(shape) + shape[3])
    want = RS.add(a, b, leaky)
    out = np.full(shape, np.nan, np.float32)
    rc = lib.dnn_shortcut_host(dnn_hip._vp(a), dnn_hip._vp(b), dnn_hip._vp(out), *shape, leaky)
    assert rc == 0, dnn_hip.last_error()
    K.check_bits(out, want, f"shortcut {shape} leaky={leaky}")


UPSAMPLE_CASES = [
    (2, 3, 5, 3, 2),     # the scalar path, odd width, batch 2
    (2, 3, 5, 4, 3),     # the 16-byte path, factor 3
    (1, 2, 7, 7, 8),     # factor 8, 7 channels
    (2, 5, 3, 64, 1),    # factor 1: a copy
    (2, 13, 13, 64, 2),  # several workgroups with a partial last chunk
    (1, 9, 11, 4, 2),    # one vector column: many pixel lanes
]


@pytest.mark.parametrize("case", UPSAMPLE_CASES, ids=lambda c: "x".join(map(str, c)))
def test_upsample_kernel_bit_exact(case):
    n, h, w, c, f = case
    a = np.arange(n * h * w * c, dtype=np.float32).reshape(n, h, w, c) - 1000.0
    want = RS.upsample(a, f)
    out = np.full(want.shape, np.nan, np.float32)
    rc = lib.dnn_upsample_host(dnn_hip._vp(a), dnn_hip._vp(out), n, h, w, c, f)
    assert rc == 0, dnn_hip.last_error()
    K.check_bits(out, want, f"upsample {case}")


def test_nodes_run_through_the_host_forms():
    g = dnn_hip.DnnGraphBuilder()
    x = g.create_input([2, 3, 5, 6])
    u = g.create_upsample(x, 2)
    u2 = g.create_upsample(x, 2)
    s = g.create_add([u, u2])
    xv = RC.exact_input(np.random.default_rng(0), (2, 3, 5, 6))
    x.set_input(xv)
    for node in (u, u2, s):
        node.run()
    K.check_bits(u.result, RS.upsample(xv, 2), "Upsample.run")
    K.check_bits(s.result, 2 * RS.upsample(xv, 2), "Add.run")


# ------------------------------------------------------------------------------ 2. exact plans
def _input_block_graph(B, ws):
    """Add([input, conv(input)]) then a conv: the shortcut's b is the plan's input."""
    g = dnn_hip.DnnGraphBuilder()
    x = g.create_input([B] + list(RS.IN_SHAPE))
    y = g.create_add([x, RC._conv(g, x, ws[0])])
    g.set_out_node(RC._conv(g, y, ws[1]))
    return g


def _act_last_graph(B, ws):
    """conv -> x; LeakyReLU(Add([x, f(x)])) as the output: the plan ends in shortcut, release."""
    g = dnn_hip.DnnGraphBuilder()
    x = RC._conv(g, g.create_input([B] + list(RS.IN_SHAPE)), ws[0])
    f = RC._conv(g, RC._conv(g, x, ws[1]), ws[2])
    g.set_out_node(g.create_leaky_relu(g.create_add([x, f])))
    return g


EXACT_CASES = {
    # name: (layers, graph builder, entry kinds, a describe line)
    "one_block": (RS.blocks_layers(1), lambda B, ws: RS.blocks_graph(B, ws, 1), "CSCCAXC",
                  "shortcut 8x8x32 slot=0 act=none"),
    "two_blocks": (RS.blocks_layers(2), lambda B, ws: RS.blocks_graph(B, ws, 2), "CSCCAXSCCAXC",
                   "release 8x8x32 slot=0"),
    "projection": (RS.PROJECTION_LAYERS, RS.projection_graph, "CSCCSRCAXXC", "shortcut 8x8x64 slot=1 act=none"),
    "top_down": (RS.TOP_DOWN_LAYERS, RS.top_down_graph, "CSPCCUJC", "upsample 4x4x16 -> 8x8x16 factor=2"),
    "input_as_b": (((3, 32, 32), (1, 32, 8)), _input_block_graph, "SCAXC", "stash 8x8x32 slot=0"),
    "act_last": (RS.blocks_layers(1)[:3], _act_last_graph, "CSCCAX", "shortcut 8x8x32 slot=0 act=leaky"),
}


@pytest.mark.parametrize("name", list(EXACT_CASES))
def test_exact_plan(name):
    layers, build, kinds, line = EXACT_CASES[name]
    ws = RC.exact_weights(layers, seed=5)
    B = 2
    g = build(B, ws)
    x = RC.exact_input(np.random.default_rng(6), (B,) + RS.IN_SHAPE)
    want = RS.oracle_graph(g, x, acc=np.float64)
    if name != "act_last":  # (its leaky output is exact too, but not integral)
        assert np.array_equal(want, np.round(want))
    assert np.abs(want).max() < 1 << 20 and np.abs(want).max() > 4
    entries = dnn_hip.lower_graph(g)
    assert RS.entry_kinds(entries) == kinds
    gp = RS.GuardedPlan(B, RS.IN_SHAPE, entries)
    try:
        assert line in gp.plan.describe().splitlines(), gp.plan.describe()
        y = gp.run(x, name)
        K.check_bits(y, want, f"{name}: plan vs the float64 oracle")
        K.check_bits(gp.run(x[:1], f"{name} n=1"), y[:1], f"{name}: n=1 of a batch-2 plan vs row 0 of n=2")
        K.check_bits(gp.run(x, f"{name} graph", how="graph"), y, f"{name}: run_graph vs eager")
        K.check_bits(gp.run(x, f"{name} graph replay", how="graph"), y, f"{name}: run_graph replay")
    finally:
        gp.close()
    # the node-by-node path on the same graph (host forms of the two new kernels)
    eng = dnn_hip.DnnInferenceEngine(g, False, device=0)
    g.in_node.set_input(x)
    K.check_bits(eng._run_nodes(), y, f"{name}: node by node vs plan")
    # and the engine takes the plan
    ye = eng.run(x)
    assert eng._plan is not None
    K.check_bits(ye, y, f"{name}: engine")


def test_hand_built_entries_with_region_reuse():
    """Entries assembled by hand: stash(s0), conv, conv, release(s0), conv, stash (takes s0's region
    again, which grows from 32 to 64 channels), conv, shortcut with the f32 leaky."""
    ws = RC.exact_weights(((3, 32, 32), (3, 32, 32), (3, 32, 32), (3, 32, 64), (1, 64, 64)), seed=8)
    ce = RS.conv_entries(ws)
    E = dnn_hip
    entries = [ce[0], E.StashEntry(0), ce[1], ce[2], E.ReleaseEntry(0), ce[3], E.StashEntry(0), ce[4],
               E.ShortcutEntry(0, leaky=True)]
    B = 3
    x = RC.exact_input(np.random.default_rng(9), (B,) + RS.IN_SHAPE)
    t = x
    for w in ws[:4]:
        t = RS.conv_ref(t, w)
    want = RS.add(RS.conv_ref(t, ws[4]), t, 2)
    gp = RS.GuardedPlan(B, RS.IN_SHAPE, entries, leaky_variant=2)
    try:
        assert gp.plan.describe().splitlines()[-1] == "shortcut 8x8x64 slot=0 act=leaky_f32"
        y = gp.run(x, "hand-built")
        K.check_bits(y, want, "hand-built plan vs numpy")
        K.check_bits(gp.run(x[:2], "hand-built n=2"), y[:2], "n < batch")
    finally:
        gp.close()


def test_upsample_and_shortcut_alone_in_guarded_plans():
    """Each kernel as a plan's only layer (it writes the caller's output): odd shapes, n < batch."""
    B, n = 3, 2
    a = np.arange(n * 3 * 5 * 7, dtype=np.float32).reshape(n, 3, 5, 7)
    gp = RS.GuardedPlan(B, (3, 5, 7), [dnn_hip.UpsampleEntry(3)])
    try:
        assert [k["name"] for k in gp.plan.kernels()] == ["upsample0"]
        K.check_bits(gp.run(a, "upsample plan"), RS.upsample(a, 3), "upsample plan")
    finally:
        gp.close()
    gp = RS.GuardedPlan(B, (3, 5, 7), [dnn_hip.StashEntry(0), dnn_hip.UpsampleEntry(1), dnn_hip.ShortcutEntry(0),
                                      dnn_hip.ReleaseEntry(0)])
    try:
        assert [k["name"] for k in gp.plan.kernels()] == ["upsample0", "shortcut0"]
        K.check_bits(gp.run(a, "x + x plan"), a + a, "x + x plan")
    finally:
        gp.close()


# ------------------------------------------------------------------------------ 3. tolerance, timing
def _random_weights(layers):
    return [RC.random_layer(i, *l) for i, l in enumerate(layers)]


@pytest.mark.parametrize("which", ["blocks", "top_down"])
def test_random_weights_batch_and_latency(which):
    layers, build = {"blocks": (RS.blocks_layers(2), lambda B, ws: RS.blocks_graph(B, ws, 2, act_after_add=True)),
                     "top_down": (RS.TOP_DOWN_LAYERS, RS.top_down_graph)}[which]
    ws = _random_weights(layers)
    B = 2
    g = build(B, ws)
    x = np.random.default_rng(2).standard_normal((B,) + RS.IN_SHAPE).astype(np.float32)
    want = RS.oracle_graph(g, x)
    for latency in (False, True):
        gp = RS.GuardedPlan(B, RS.IN_SHAPE, dnn_hip.lower_graph(g), latency=latency)
        try:
            y = gp.run(x, f"{which} latency={latency}")
            y1 = gp.run(x[:1], f"{which} latency={latency} n=1")
        finally:
            gp.close()
        err = R.normwise_err(y, want)
        print(f"{which} random weights latency={latency}: normwise error {err:.3e}")
        assert err < NET_TOL, f"{which} latency={latency}: normwise error {err:.3e} >= {NET_TOL:.0e}"
        assert R.normwise_err(y1, want[:1]) < NET_TOL


def test_per_kernel_timing_and_marks():
    ws = RC.exact_weights(RS.blocks_layers(2), seed=5)
    g = RS.blocks_graph(2, ws, 2)
    x = RC.exact_input(np.random.default_rng(6), (2,) + RS.IN_SHAPE)
    want = RS.oracle_graph(g, x)
    plan = dnn_hip.Plan(2, RS.IN_SHAPE, dnn_hip.lower_graph(g), device=0)
    try:
        names = [k["name"] for k in plan.kernels()]
        assert [n for n in names if n.startswith("shortcut")] == ["shortcut0", "shortcut1"]
        assert not any("stash" in n or "release" in n for n in names)
        plan.timing_begin(2)
        for _ in range(2):
            K.check_bits(plan.run_host(x), want, "timed run")
        ms, cnt = plan.timing_end()
        assert cnt == [2] * len(names) and all(m > 0 for m in ms)
        plan.timing_begin(1, only="shortcut1")
        plan.run_host(x)
        ms, cnt = plan.timing_end()
        assert cnt == [1 if n == "shortcut1" else 0 for n in names]
        plan.set_mark("shortcut0")
        K.check_bits(plan.run_host(x), want, "marked run")
        plan.set_mark(None)
    finally:
        plan.close()


# ------------------------------------------------------------------------------ 4. narrow Darknet-53
def test_narrow_darknet53_against_the_oracle():
    """Narrow Darknet-53 (width_div 8: the widest layer has 128 channels) on 64 x 64 frames at batch 2.
    Measured on MI355X: 7.1e-7 normwise for the plan against the float64 oracle."""
    import darknet53
    ws = synth.darknet53_weights(width_div=8)
    m = darknet53.DARKNET53([2, 64, 64, 3], ws, False)
    x = synth.frames([0, 1], shape=(64, 64, 3))
    y = m.inference(x).copy()  # (the node-by-node run below writes the output node's array in place)
    assert m.sess._plan is not None and y.shape == (2, 2, 2, 425)
    names = [k["name"] for k in m.sess.plan().kernels()]
    assert [n for n in names if n.startswith("shortcut")] == [f"shortcut{i}" for i in range(23)]
    assert sum(l.startswith("conv ") for l in m.sess.plan().describe().splitlines()) == 59
    val = RS.oracle_graph(m.g, x, keep=True)
    want = val[m.g.out_node]
    K.check_finite(y, "narrow Darknet-53")
    # the synthetic weights keep the activations O(1) through the 23 sums
    last_sum = [n for n in m.nodes if isinstance(n, dnn_hip.Add)][-1]
    assert 0.05 < float(np.abs(val[last_sum]).mean()) < 50
    err = R.normwise_err(y, want)
    print(f"narrow Darknet-53: plan vs float64 oracle, normwise error {err:.3e}")
    assert err < NET_TOL, f"narrow Darknet-53: normwise error {err:.3e} >= {NET_TOL:.0e}"
    m.g.in_node.set_input(x)
    yn = m.sess._run_nodes()
    en = R.normwise_err(yn, want)
    print(f"narrow Darknet-53: node by node vs float64 oracle {en:.3e}, vs plan {R.normwise_err(yn, y):.3e}")
    assert en < NET_TOL and R.normwise_err(yn, y) < NET_TOL
    assert isinstance(m.postprocessing(y[0:1]), list)
