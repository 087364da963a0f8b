"""Conv and pool geometry through plans on the GPU: strides (equal and not), VALID padding, front
pads of 0 / 1 / 2, non-square and wide kernels, general pool windows, on the kernels that are
generic in geometry (the fp32 implicit GEMM on the LDS-DMA ring and its persistent form, the fp16
implicit GEMM, the explicit im2col + GEMM, the pool kernels, the x3 combine at a general window).

Every plan runs on poisoned, guarded, caller-owned buffers (residual_cases.GuardedPlan).  The
named cases of tests/geometry_cases.py run twice: on small-integer tensors, where every path must
give the float64 oracle's bits, and on random tensors against the suite's per-layer bars.  The
seeded cases run the checks of test_gpu_plan_fuzz.py.  tests/test_geometry_cases.py shows without
a GPU which kernel each case reaches and that the oracle agrees with torch's float64 conv and
pool at every one of these geometries."""
import numpy as np
import pytest
import torch  # noqa: F401  (one HIP runtime in the process before the library opens the device)

import dnn_hip
import geometry_cases as G
import plan_fuzz_checks as K
import residual_cases as RS
import synth

pytestmark = pytest.mark.gpu

KW = {"fp32": {}, "latency": {"latency": True}, "fp16": {"precision": "fp16"}}


def _tol(kind):
    return K.FP16_LAYER_TOL if kind == "fp16" else K.LAYER_TOL


class _Plans(object):
    """Guarded plans of one test, closed together; describe() of the first one for messages."""

    def __init__(self, label):
        self.label, self.plans = label, []

    def guarded(self, kind, B, shape, blocks, ws):
        entries = dnn_hip.lower_graph(G.graph(B, shape, blocks, ws))
        assert entries is not None
        self.plans.append(RS.GuardedPlan(B, shape, entries, **KW[kind]))
        return self.plans[-1]

    def owned(self, kind, B, shape, blocks, ws):
        """The same plan on its own allocation (fresh zero pages instead of poison)."""
        self.plans.append(dnn_hip.Plan.from_graph(G.graph(B, shape, blocks, ws), device=0, **KW[kind]))
        return self.plans[-1]

    def __enter__(self):
        return self

    def __exit__(self, et, ev, tb):
        info = self.label + ("\n" + getattr(self.plans[0], "plan", self.plans[0]).describe() if self.plans else "")
        for p in self.plans:
            p.close()
        if et is AssertionError:
            raise AssertionError(f"{ev}\n{info}") from None
        return False


def _chain_checks(label, kind, B, shape, blocks, X, X2, ws):
    """test_plan_chain_fuzz's steps 1-4: three runs through one poisoned plan (n = B, n < B with
    other data, n = B) against plans on zeroed buffers, every block against the oracle by teacher
    forcing through the prefix plans, row 0 against the one-frame plan where it runs the same
    kernels."""
    tol = _tol(kind)
    with _Plans(f"{label}: kind={kind} B={B} frame={shape} blocks={blocks}") as P:
        full = P.guarded(kind, B, shape, blocks, ws)
        k = max(1, B // 2)
        y1 = full.run(X, "run 1 (n = B)")
        y2 = full.run(X2[:k], "run 2 (n < B)") if B > 1 else None
        y3 = full.run(X, "run 3 (n = B)")
        K.check_bits(y3, y1, "run 3 against run 1")
        K.check_bits(y1, P.owned(kind, B, shape, blocks, ws).run_host(X), "poisoned run 1 against the zeroed-buffer plan")
        if y2 is not None:
            K.check_bits(y2, P.owned(kind, B, shape, blocks, ws).run_host(X2[:k]),
                         "poisoned run 2 (n < B) against a fresh zeroed-buffer plan")
        outs = []
        a_prev = X
        for j in range(1, len(blocks) + 1):
            b = blocks[j - 1]
            a_j = y1 if j == len(blocks) else P.guarded(kind, B, shape, blocks[:j], ws[:j]).run(X, f"prefix {j}")
            want = G.oracle_block(a_prev, b, ws[j - 1], skip=None if b["add"] is None else outs[b["add"]])
            err = K.check_layer_err(a_j, want, tol, f"block {j} of {len(blocks)} (teacher forced)")
            print(f"{label} {kind} block {j}: normwise error {err:.3e}")
            outs.append(a_j)
            a_prev = a_j
        if kind != "latency" and B > 1:
            one = P.guarded(kind, 1, shape, blocks, ws)
            same = ([G.layer_config(ln) for ln in one.plan.describe().splitlines()] ==
                    [G.layer_config(ln) for ln in full.plan.describe().splitlines()])
            if same:
                K.check_bits(y1[:1], one.run(X[:1], "one-frame plan"), "row 0 against the one-frame plan")


# ------------------------------------------------------------------------------ named, exact
@pytest.mark.parametrize("name", G.NAMES)
def test_named_exact(monkeypatch, name):
    """Small-integer tensors (no BatchNorm, no leaky): every partial sum is an integer below 2^24,
    so the plan in either fp32 kind, a one-frame run of the batch plan, a rerun after other data,
    the HIP-graph replay, the node-by-node path and the same plan with buffer addressing, fusion
    or the x3 convs switched off all give the float64 oracle's bits."""
    c = G.named(name)
    B, shape, blocks = c["B"], c["shape"], c["blocks"]
    X, X2, ws = G.exact_tensors(G.NAMES.index(name), B, shape, blocks)
    want = G.oracle_chain(X, blocks, ws)[-1]
    want2 = G.oracle_chain(X2, blocks, ws)[-1]
    for flag in ("DNN_HIP_GEMM_BUF", "DNN_HIP_FUSE", "DNN_HIP_X3"):
        monkeypatch.delenv(flag, raising=False)
    for kind in ("fp32", "latency"):
        with _Plans(f"{name}: kind={kind} B={B} frame={shape} blocks={blocks}") as P:
            gp = P.guarded(kind, B, shape, blocks, ws)
            lines = gp.plan.describe().splitlines()
            y1 = gp.run(X, "run 1")
            K.check_bits(y1, want, f"{kind} plan against the float64 oracle")
            K.check_bits(gp.run(X[:1], "n = 1 of the batch plan"), want[:1], "n = 1 of the batch plan against row 0")
            k = max(1, B // 2)
            K.check_bits(gp.run(X2[:k], "run 2 (other data)"), want2[:k], "run 2 (n < B, other data) against the oracle")
            K.check_bits(gp.run(X, "run 3"), y1, "run 3 against run 1")
            K.check_bits(gp.run(X, "graph replay", how="graph"), y1, "run_graph against the eager run")
            K.check_bits(gp.run(X, "graph replay 2", how="graph"), y1, "second run_graph against the eager run")
            if kind == "fp32":
                eng = dnn_hip.DnnInferenceEngine(G.graph(B, shape, blocks, ws), False, device=0)
                eng.g.in_node.set_input(X)
                K.check_bits(np.array(eng._run_nodes()), y1, "node by node against the plan")
            flags = ["DNN_HIP_FUSE"]
            if any("mode=implicit" in ln or "mode=patch" in ln.split() for ln in lines):
                flags.append("DNN_HIP_GEMM_BUF")
            if any(f"mode={m}" in ln for ln in lines for m in G.X3_MODES + ("x3_1x1",)):
                flags.append("DNN_HIP_X3")
            for flag in flags:
                monkeypatch.setenv(flag, "0")
                try:
                    alt = P.guarded(kind, B, shape, blocks, ws)
                    # (the other two change the choice of kernel where a fused kernel was chosen)
                    if flag == "DNN_HIP_X3" or (flag == "DNN_HIP_FUSE" and any("mode=implicit" in ln for ln in lines)):
                        assert alt.plan.describe().splitlines() != lines, (flag, lines)
                    K.check_bits(alt.run(X, f"{flag}=0"), y1, f"the plan built and run with {flag}=0 against the plan")
                finally:
                    monkeypatch.delenv(flag)


# ------------------------------------------------------------------------------ named, random
NAMED_KINDS = [(c["name"], kind) for c in G.NAMED for kind in G.named_kinds(c)]


@pytest.mark.parametrize("name,kind", NAMED_KINDS)
def test_named_random(name, kind):
    """Random tensors: every block within the suite's per-layer bar of the oracle (teacher forced),
    poisoned and zeroed buffers bit-equal."""
    c = G.named(name)
    X, X2, ws = G.case_tensors(G.NAMES.index(name), c["B"], c["shape"], c["blocks"])
    _chain_checks(name, kind, c["B"], c["shape"], c["blocks"], X, X2, ws)


# ------------------------------------------------------------------------------ seeded
@pytest.mark.parametrize("seed", range(G.NSEEDS))
def test_geometry_fuzz(seed):
    """The checks of test_plan_chain_fuzz over geometry_case(seed).  (Seed 19, block 2: a 7x7 conv
    9x7x125 -> 128, `mode=gemm cfg=7 K=6125`, measured 2.690e-06 against the 2e-6 bar as one fp32
    chain over all of K; the plan now sums such layers in three K parts)"""
    kind, B, shape, blocks = G.geometry_case(seed)
    X, X2, ws = G.case_tensors(1000 + seed, B, shape, blocks)
    _chain_checks(f"seed {seed}", kind, B, shape, blocks, X, X2, ws)


# ------------------------------------------------------------------------------ Darknet-53's strided layers
def test_narrow_darknet53_down_layers():
    """The five stage-opening convs (3x3 stride 2 SAME on even frames: pads top / left 0) of the
    narrow Darknet-53 of test_gpu_residual.py, each as a one-block plan (conv + bias + bn + leaky)
    on the oracle's own input to that layer, held to the per-layer bar: the end-to-end test's 1e-4
    over 59 layers cannot see them.  Measured on MI355X: see DESIGN.md §8."""
    import darknet53
    ws = darknet53.validate(synth.darknet53_weights(width_div=8))
    B = 2
    g, nodes = darknet53.build_graph(dnn_hip.DnnGraphBuilder, ws, in_shape=(B, 64, 64, 3))
    x = synth.frames([0, 1], shape=(64, 64, 3))
    val = RS.oracle_graph(g, x, keep=True)
    downs = [(w, n) for w, n in zip(ws, [n for n in nodes if isinstance(n, dnn_hip.Conv2D)]) if n.strides[1] == 2]
    assert len(downs) == 5
    for i, (w, conv) in enumerate(downs):
        leaky = nodes[nodes.index(conv) + 3]
        assert isinstance(leaky, dnn_hip.LeakyReLU)
        a = val[conv.in_node]
        shape = a.shape[1:]
        assert shape[0] % 2 == 0 and shape[1] % 2 == 0
        blk = [G.block(G.sq(3, 2), shape[2], w["kernel"].shape[3], "bn")]
        wt = [(w["kernel"], w["biases"], (w["moving_mean"], w["moving_variance"], w["gamma"]), True)]
        with _Plans(f"down {i}: {shape} -> {w['kernel'].shape[3]}") as P:
            gp = P.guarded("fp32", B, shape, blk, wt)
            y = gp.run(a, f"down {i}")
            err = K.check_layer_err(y, val[leaky], K.LAYER_TOL, f"down {i} ({gp.plan.describe().strip()})")
            print(f"narrow Darknet-53 down {i}: {gp.plan.describe().strip()}: normwise error {err:.3e}")


# ------------------------------------------------------------------------------ an fp16 plan the path rejects
def test_fp16_plan_rejects_a_7x7_conv_and_the_next_plan_works():
    shape, bad = (12, 12, 8), [G.block(G.sq(7, 2), 8, 16, "bias")]
    lines, _ = G.lower_host("fp16", 1, shape, bad)
    assert "mode=gemm" in lines[0]
    _, _, ws = G.case_tensors(1, 1, shape, bad)
    with pytest.raises(dnn_hip.DnnHipError, match="fp16 plan cannot run conv"):
        dnn_hip.Plan.from_graph(G.graph(1, shape, bad, ws), device=0, precision="fp16")
    c = G.named("down_even")
    X, _, ws = G.case_tensors(2, c["B"], c["shape"], c["blocks"])
    with _Plans("down_even fp16 after the rejected plan") as P:
        y = P.guarded("fp16", c["B"], c["shape"], c["blocks"], ws).run(X, "fp16 plan")
        K.check_layer_err(y, G.oracle_chain(X, c["blocks"], ws)[-1], K.FP16_LAYER_TOL, "fp16 plan after the rejected one")
