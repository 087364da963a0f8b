"""The SPP kernel and entry on the GPU: dnn_spp_host bit-identical to the oracle composed from
oracle/ref_numpy.py's max pool on tie-heavy inputs with both zeros; plans with an spp entry on
poisoned, guarded caller buffers (in every position the entry can take, in batch and latency mode,
through a captured graph, and with n < batch); the narrow YOLOv3-SPP and YOLOv3-tiny models against
the float64 oracle; and their detect() against the host decode of their own head tensors."""
import ctypes

import numpy as np
import pytest

import dnn_hip
import multi_out_cases as MC
import plan_fuzz_checks as K
import ref_numpy as R
import residual_cases as RS
import route_cases as RC
import spp_cases as SC
import synth
import yolo_post

pytestmark = pytest.mark.gpu

NET_TOL = 1e-4  # normwise, end to end (the suite's existing bar, tests/test_gpu_multi_out.py)


# ------------------------------------------------------------------------------ the kernel
def _spp_host(x, sizes, x_first):
    n, h, w, c = x.shape
    out = np.full((n, h, w, (len(sizes) + 1) * c), np.nan, np.float32)
    ks = (ctypes.c_int * len(sizes))(*sizes)
    rc = dnn_hip.mylib.dnn_spp_host(dnn_hip._vp(x), dnn_hip._vp(out), n, h, w, c, len(sizes), ks, 1 if x_first else 0)
    assert rc == 0, dnn_hip.last_error()
    return out


@pytest.mark.parametrize("shape", SC.KERNEL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_is_bit_identical_to_the_composed_oracle(shape):
    """Every block of every size case, signed zeros included; the last image is all negative."""
    x = SC.tie_input(np.random.default_rng(sum(shape)), shape)
    assert x.shape[0] == shape[0] + 1 and (x[-1] < 0).all()
    if x[:-1].size >= 64:
        assert np.signbit(x[x == 0]).any() and not np.signbit(x[x == 0]).all()
    for sizes, x_first in SC.SIZE_CASES:
        got = _spp_host(x, sizes, x_first)
        K.check_bits(got, SC.spp(x, sizes, x_first), f"spp {shape} sizes {sizes} x_first {x_first}")


def test_kernel_on_the_full_width_map_and_an_empty_batch():
    """13 x 13 x 512 at batch 8 (the shape where SPP occurs: 64-byte slabs, 2048 workgroups)."""
    x = SC.tie_input(np.random.default_rng(3), (7, 13, 13, 512))
    K.check_bits(_spp_host(x, (13, 9, 5), False), SC.spp(x, (13, 9, 5)), "spp 8x13x13x512")
    ks = (ctypes.c_int * 1)(5)
    assert dnn_hip.mylib.dnn_spp_host(dnn_hip._vp(x), dnn_hip._vp(x), 0, 13, 13, 512, 1, ks, 0) == 0


def test_spp_node_runs_through_the_host_form():
    g = dnn_hip.DnnGraphBuilder()
    xin = g.create_input([2, 7, 6, 12])
    node = g.create_spp(xin, (5, 9, 13), x_first=True)
    x = SC.tie_input(np.random.default_rng(1), (1, 7, 6, 12))
    xin.set_input(x)
    node.run()
    K.check_bits(node.result, SC.spp(x, (5, 9, 13), True), "Spp.run")


# ------------------------------------------------------------------------------ plans
def _case(name, B, seed=6):
    layers, build, kinds = SC.PLAN_CASES[name]
    g = build(B, RC.exact_weights(layers, seed=5))
    x = RC.exact_input(np.random.default_rng(seed), (B,) + SC.IN_SHAPE)
    want = SC.oracle_outputs(g, x)
    for w in want:
        assert np.array_equal(w, np.round(w)) and 2 < np.abs(w).max() < 1 << 20
    entries = dnn_hip.lower_graph(g)
    assert SC.entry_kinds(entries) == kinds
    return g, x, want, entries


def _check_taps(gp, g, n, want, what, **kw):
    extras = list(g.extra_out_nodes)
    assert len(gp.plan.tap_entries) == len(extras)
    for k, e in enumerate(gp.plan.tap_entries):
        ref = want[[id(n_) for n_ in extras].index(id(e.node))]
        assert gp.plan.tap_shapes[k] == ref.shape[1:]
        K.check_bits(MC.read_tap(gp, k, n, **kw), ref[:n], f"{what}: tap {k}")


@pytest.mark.parametrize("latency", [False, True], ids=["batch", "latency"])
@pytest.mark.parametrize("name", list(SC.PLAN_CASES))
def test_exact_plan_with_an_spp_entry(name, latency):
    """conv -> spp -> conv, spp first (it reads d_in), spp last (it writes d_out), spp -> tap -> conv
    (it writes a region) and restore -> spp (it reads a region): output and taps bit-equal to the
    float64 oracle, guards intact; and the engine on the plan path and node by node."""
    B = 2
    g, x, want, entries = _case(name, B)
    gp = RS.GuardedPlan(B, SC.IN_SHAPE, entries, latency=latency)
    try:
        lines = gp.plan.describe().splitlines()
        assert sum(l.startswith("spp ") for l in lines) == 1
        assert sum(k["name"].startswith("spp") for k in gp.plan.kernels()) == 1
        K.check_bits(gp.run(x, name), want[-1], f"{name}: primary output vs the float64 oracle")
        _check_taps(gp, g, B, want, name)
    finally:
        gp.close()
    if latency:
        return
    eng = dnn_hip.DnnInferenceEngine(g, False, device=0)
    outs = eng.run_all(x)
    assert eng._plan is not None and len(outs) == len(want)
    for o, w in zip(outs, want):
        K.check_bits(o, w, f"{name}: run_all on the plan")
    g.in_node.set_input(x)
    primary = dnn_hip.DnnInferenceEngine(g, False, device=0)._run_nodes()
    for o, w in zip([n.result for n in g.extra_out_nodes] + [primary], want):
        K.check_bits(o, w, f"{name}: node by node")


def test_debug_engine_runs_the_spp_node_by_node(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    g, x, want, _ = _case("chain", 2)
    eng = dnn_hip.DnnInferenceEngine(g, True, device=0)
    K.check_bits(eng.run(x), want[-1], "debug=True")
    assert eng._plan is None and (tmp_path / "intermediate" / "layer_5.npy").exists()


@pytest.mark.parametrize("name", ["chain", "restore"])
def test_graph_replay_equals_run_device(name):
    B = 2
    g, x, want, entries = _case(name, B)
    x2 = RC.exact_input(np.random.default_rng(7), (B,) + SC.IN_SHAPE)
    want2 = SC.oracle_outputs(g, x2)
    assert not np.array_equal(want[-1], want2[-1])
    gp = RS.GuardedPlan(B, SC.IN_SHAPE, entries)
    try:
        eager = gp.run(x, "eager")
        K.check_bits(eager, want[-1], "eager")
        for xi, wi, what in ((x, want, "graph"), (x2, want2, "graph replay"), (x, want, "graph replay 2")):
            K.check_bits(gp.run(xi, what, how="graph"), wi[-1], f"{name} {what}: primary output")
            _check_taps(gp, g, B, wi, what)
        K.check_bits(gp.run(x, "graph again", how="graph"), eager, "run_graph == run_device")
    finally:
        gp.close()


@pytest.mark.parametrize("name", ["last", "tap"])
def test_n_below_batch_writes_only_n_images(name):
    """n = 1 of a batch-3 plan: with the spp entry last, images 1..2 of the caller's output keep the
    canary (GuardedPlan.run checks every word past the first n rows); with its output tapped,
    images 1..2 of the tap's region keep the workspace's poison."""
    B, n = 3, 1
    g, x, want, entries = _case(name, B)
    gp = RS.GuardedPlan(B, SC.IN_SHAPE, entries)
    try:
        y = gp.run(x[:n], f"{name} n=1 of 3")
        K.check_bits(y, want[-1][:n], f"{name}: n=1 of 3, primary output")
        _check_taps(gp, g, n, want, f"{name} n=1 of 3", fresh_tail=True)
    finally:
        gp.close()


def test_a_finalized_plan_refuses_the_entry_and_stays_as_it_is():
    g, x, want, entries = _case("chain", 2)
    plan = dnn_hip.Plan(2, SC.IN_SHAPE, entries, device=0)
    try:
        before = plan.describe()
        y = plan.run_host(x)
        ks = (ctypes.c_int * 1)(5)
        assert dnn_hip.mylib.dnn_plan_add_spp(plan.h, 1, ks, 0) != 0
        assert "finalized" in dnn_hip.last_error()
        assert plan.describe() == before and plan.out_shape == (8, 8, 8)
        K.check_bits(plan.run_host(x), y, "output after the refused entry")
        K.check_bits(y, want[-1], "chain")
    finally:
        plan.close()
    with pytest.raises(dnn_hip.DnnHipError, match="fp16"):
        dnn_hip.Plan(2, SC.IN_SHAPE, entries, device=0, precision="fp16")


# ------------------------------------------------------------------------------ the models
def _narrow_model(make, ws, grids, n_convs, counts):
    """A narrow model at batch 2 on two 96 x 96 frames: every output within NET_TOL normwise of the
    float64 oracle, every image bit-identical to a batch-1 plan, the describe counts."""
    x = synth.frames([0, 1], shape=(96, 96, 3))
    m = make([2, 96, 96, 3], ws, False)
    outs = [o.copy() for o in m.inference(x)]
    assert m.sess._plan is not None
    assert [o.shape for o in outs] == [(2, g_, g_, 24) for g_ in grids]
    lines = m.sess.plan().describe().splitlines()
    counts = dict(counts, conv=n_convs)
    got = {k: sum(l.startswith(k + " ") for l in lines) for k in counts}
    assert got == counts, got
    want = SC.oracle_outputs(m.g, x)
    name = type(m).__name__
    for o, w_, g_ in zip(outs, want, grids):
        K.check_finite(o, f"{name} grid {g_}")
        assert 0.01 < float(np.abs(w_).mean()) < 100
        err = R.normwise_err(o, w_)
        print(f"narrow {name} grid {g_}: plan vs float64 oracle, normwise error {err:.3e}")
        assert err < NET_TOL, f"narrow {name} grid {g_}: normwise error {err:.3e} >= {NET_TOL:.0e}"
    m1 = make([1, 96, 96, 3], ws, False)
    for i in range(2):
        for o, o1, g_ in zip(outs, m1.inference(x[i:i + 1]), grids):
            K.check_bits(o1, o[i:i + 1], f"narrow {name} grid {g_}: image {i} of batch 2 vs a batch-1 plan")
    return m, x, outs


def _check_detect(m, x, outs):
    """detect() (plan and decode on the device) == the host decode of the model's own head tensors."""
    rows = m.detect(x, raise_errors=False)
    assert len(rows) == 2
    assert rows == yolo_post.detect_batch_multi(outs, m.head, raise_errors=False)
    assert m.detect(x[1:], raise_errors=False) == rows[1:]
    for i in range(2):
        if not isinstance(rows[i], int):
            assert m.postprocessing([o[i:i + 1] for o in outs]) == yolo_post.label_boxes(rows[i], m.head)
    print(f"{type(m).__name__} detect:", [r if isinstance(r, int) else len(r) for r in rows], "detections")
    return rows


def test_narrow_yolov3_spp_against_the_oracle_and_its_decode():
    import yolov3_spp
    ws = synth.yolov3_spp_weights(width_div=8, n_out=24)
    m, x, outs = _narrow_model(yolov3_spp.YOLO_V3_SPP, ws, (3, 6, 12), 76,
                               {"spp": 1, "tap": 2, "route": 2, "upsample": 2, "pool": 0})
    assert [(s.grid_h, s.cell) for s in m.head.scales] == [(3, 32.0), (6, 16.0), (12, 8.0)]
    _check_detect(m, x, outs)
    # with the public anchors the synthetic heads give degenerate boxes (an error code per image,
    # the same from both decodes); 16 x the anchors and a 0.9 threshold give rows to compare
    head = yolo_post.MultiHead(
        [yolo_post.Scale(96 // st, 96 // st, 3, 3, tuple(16.0 * a / st for a in px), float(st), 0.9, 0.3)
         for st, px in yolo_post.YOLOV3_ANCHORS], "logistic")
    big = yolov3_spp.YOLO_V3_SPP([2, 96, 96, 3], ws, False, head=head)
    rows = _check_detect(big, x, outs)
    assert all(not isinstance(r, int) and len(r) > 0 for r in rows), rows


def test_narrow_yolov3_tiny_against_the_oracle_and_its_decode():
    import yolov3_tiny
    ws = synth.yolov3_tiny_weights(width_div=4, n_out=24)
    m, x, outs = _narrow_model(yolov3_tiny.YOLO_V3_TINY, ws, (3, 6), 13,
                               {"spp": 0, "tap": 1, "route": 1, "upsample": 1})
    assert [(s.grid_h, s.cell) for s in m.head.scales] == [(3, 32.0), (6, 16.0)]
    rows = _check_detect(m, x, outs)
    assert all(not isinstance(r, int) and len(r) > 0 for r in rows), rows
