"""The step list is what runs.  dnn_plan_run walks one list of steps, one per kernel launch, and
kernels() / timing_begin / timing_begin_only index the same list.  For small plans that between
them lower to every kind of step:

1. timing over two runs counts every kernel twice, each with a time above zero;
2. timing only the second kernel of a multi-kernel layer, a conversion step or the pool that
   combines x3 partials counts 1 there and 0 everywhere else;
3. an untimed run, a timed run and a HIP-graph replay give the same bits, and fp32 plans the
   float64 oracle's bits (small-integer tensors, as tests/test_gpu_geometry.py's exact cases; fp16
   plans are held to their own untimed run only).

Each plan's kernel names are asserted before it runs, so a plan that lowered to something simpler
fails instead of passing."""
import numpy as np
import pytest
import torch  # noqa: F401  (one HIP runtime in the process before the library opens the device)

import dnn_hip
import geometry_cases as G
import multi_out_cases as MC
import plan_fuzz_checks as K
import residual_cases as RS
import route_cases as RC
import spp_cases as SC

pytestmark = pytest.mark.gpu

P22, P32 = G.sq(2, 2), G.sq(3, 2)
X3_CONV = dict(conv=G.sq(3), cin=64, oc=512, pre_pool=P22)  # 16x16x64 -> pool -> 8x8x64 -> 3x3 x3 conv, two K slices
F16_CHAIN = [G.block(G.sq(3), 32, 64, pool=P22), G.block(G.sq(1), 64, 125, "bias")]

# name: (kind, environment, B, shape, blocks, kernel names, the kernels timed alone)
CHAINS = {
    "explicit_gemm": ("fp32", {"DNN_HIP_FUSE": "0"}, 2, (8, 8, 3), [G.block(G.sq(3), 3, 16)],
                      ["conv0.im2col", "conv0.gemm"], ["conv0.gemm"]),
    "splitk_reduce": ("fp32", {"DNN_HIP_SPLITK_FUSED": "0"}, 2, (6, 6, 256), [G.block(G.sq(3), 256, 512)],
                      ["conv0.gemm", "conv0.reduce"], ["conv0.reduce"]),
    "x3_combine": ("fp32", {}, 2, (16, 16, 64), [G.block(**X3_CONV), G.block(G.sq(1), 512, 32, "bias")],
                   ["pool0", "conv0.gemm", "conv0.combine", "conv1.gemm"], ["conv0.combine"]),
    "x3_combine_pool": ("fp32", {}, 2, (16, 16, 64), [G.block(pool=P32, **X3_CONV)],
                        ["pool0", "conv0.gemm", "pool1"], ["pool1"]),
    "fp16_direct_out": ("fp16", {}, 2, (8, 8, 32), F16_CHAIN, ["input.cvt", "conv0.gemm", "conv1.gemm"], ["input.cvt"]),
    "fp16_cvt_out": ("fp16", {"DNN_HIP_F16_DIRECT_OUT": "0"}, 2, (8, 8, 32), F16_CHAIN,
                     ["input.cvt", "conv0.gemm", "conv1.gemm", "output.cvt"], ["input.cvt", "output.cvt"]),
}
# name: (graph builder, layers, oracle, kernel names, the kernels timed alone)
GRAPHS = {
    "neck": (MC.neck_graph, MC.NECK_LAYERS, MC.oracle_outputs,
             ["conv0.gemm", "conv1.gemm", "conv2.gemm", "shortcut0", "conv3.gemm", "conv4.gemm", "conv5.gemm",
              "conv6.gemm", "upsample0", "route0", "conv7.im2col", "conv7.gemm"], ["conv7.gemm"]),
    "spp_tap": (SC.tap_graph, SC.TAP_LAYERS, SC.oracle_outputs, ["conv0.gemm", "spp0", "conv1.gemm"], []),
}
KW = {"fp32": {}, "fp16": {"precision": "fp16"}}


def step_kinds(names, describe):
    """The kinds of step a plan's kernel names (and, for the pool that combines, its describe()
    text) show."""
    kinds = set()
    lines = [ln for ln in describe.splitlines() if ln.split()[0] in ("conv", "pool")]
    for nm in names:
        base, _, suffix = nm.partition(".")
        kinds.add({"input.cvt": "cvt_in", "output.cvt": "cvt_out"}.get(nm) or
                  {"im2col": "im2col", "reduce": "reduce", "combine": "x3_combine", "gemm": "conv", "direct": "conv",
                   "patch": "conv"}.get(suffix) or base.rstrip("0123456789"))
    for a, b in zip(lines, lines[1:]):  # a split x3 conv straight before a pool: that pool's step combines
        if a.startswith("conv") and "x3-combine" in a and b.startswith("pool"):
            kinds.add("x3_combine_pool")
    return kinds


ALL_KINDS = {"cvt_in", "im2col", "conv", "reduce", "x3_combine", "pool", "x3_combine_pool", "route", "shortcut",
             "upsample", "spp", "cvt_out"}


def _check_steps(gp, x, names, alone, want, taps=()):
    """The three checks of the module docstring on one guarded plan; `want`: the oracle's primary
    output or None; taps: [(tap index, oracle tensor)]."""
    plan = gp.plan
    got = [k["name"] for k in plan.kernels()]
    assert got == names, (got, plan.describe())
    n = x.shape[0]
    y0 = gp.run(x, "untimed run")
    if want is not None:
        K.check_bits(y0, want, "untimed run against the float64 oracle")
    plan.timing_begin(2)
    y1 = gp.run(x, "timed run 1")
    y2 = gp.run(x, "timed run 2")
    ms, cnt = plan.timing_end()
    print(plan.describe(), [(k, round(t, 4)) for k, t in zip(names, ms)])
    assert cnt == [2] * len(names), (cnt, names)
    assert all(t > 0 for t in ms), (ms, names)
    K.check_bits(y1, y0, "timed run 1 against the untimed run")
    K.check_bits(y2, y0, "timed run 2 against the untimed run")
    for only in alone:
        plan.timing_begin(1, only=only)
        y = gp.run(x, f"run timing only {only}")
        ms, cnt = plan.timing_end()
        assert cnt == [1 if k == only else 0 for k in names], (only, cnt, names)
        assert ms[names.index(only)] > 0
        K.check_bits(y, y0, f"run timing only {only} against the untimed run")
    for rep in (1, 2):
        K.check_bits(gp.run(x, f"graph replay {rep}", how="graph"), y0, f"run_graph {rep} against the untimed run")
    for k, t in taps:
        K.check_bits(MC.read_tap(gp, k, n), t, f"tap {k} against the float64 oracle")


@pytest.mark.parametrize("name", sorted(CHAINS))
def test_chain_steps(monkeypatch, name):
    kind, env, B, shape, blocks, names, alone = CHAINS[name]
    for flag in ("DNN_HIP_FUSE", "DNN_HIP_PATCH", "DNN_HIP_SPLITK_FUSED", "DNN_HIP_F16_DIRECT_OUT", "DNN_HIP_X3"):
        monkeypatch.delenv(flag, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    X, _, ws = G.exact_tensors(7, B, shape, blocks)
    gp = RS.GuardedPlan(B, shape, dnn_hip.lower_graph(G.graph(B, shape, blocks, ws)), **KW[kind])
    try:
        _check_steps(gp, X, names, alone, G.oracle_chain(X, blocks, ws)[-1] if kind == "fp32" else None)
    finally:
        gp.close()


@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_graph_steps(name):
    build, layers, oracle, names, alone = GRAPHS[name]
    B = 2
    g = build(B, RC.exact_weights(layers))
    x = RC.exact_input(np.random.default_rng(11), (B,) + MC.IN_SHAPE)
    outs = oracle(g, x)
    gp = RS.GuardedPlan(B, MC.IN_SHAPE, dnn_hip.lower_graph(g))
    try:
        assert len(gp.plan.tap_shapes) == len(outs) - 1 >= 1
        _check_steps(gp, x, names, alone, outs[-1], taps=list(enumerate(outs[:-1])))
    finally:
        gp.close()


def test_the_plans_cover_every_step_kind():
    """From the expected kernel names alone (they are asserted against kernels() before each plan
    runs), so this holds whichever tests of the module were selected."""
    def text(kind, env, B, shape, entries, monkey):
        for k, v in env.items():
            monkey.setenv(k, v)
        try:
            return dnn_hip.Plan.lowering(B, shape, entries, precision="fp16" if kind == "fp16" else "fp32")
        finally:
            for k in env:
                monkey.delenv(k)

    kinds = set()
    with pytest.MonkeyPatch.context() as monkey:
        for kind, env, B, shape, blocks, names, _ in CHAINS.values():
            es = dnn_hip.lower_graph(G.graph(B, shape, blocks, G.zero_tensors(blocks)))
            kinds |= step_kinds(names, text(kind, env, B, shape, es, monkey))
        for build, layers, _, names, _ in GRAPHS.values():
            es = dnn_hip.lower_graph(build(2, RC.exact_weights(layers)))
            kinds |= step_kinds(names, text("fp32", {}, 2, MC.IN_SHAPE, es, monkey))
    assert kinds == ALL_KINDS, sorted(ALL_KINDS - kinds)
