"""GPU: the padded conv entry (dnn_plan_add_conv_padded) in every fp32 execution mode, explicit
padding against the float64 oracle on poisoned, guarded buffers, and imported narrow Darknet models
end to end (tests/darknet_cases.py, tests/darknet_oracle.py)."""
import numpy as np
import pytest

import darknet_cases as DC
import darknet_import as D
import darknet_oracle as DO
import dnn_hip
import plan_fuzz_checks as K
import post_head_cases as HK
import post_multi_oracle as MO
import post_multilabel_oracle as LO
import ref_numpy as R
import residual_cases as RS
import synth
import yolo_post

pytestmark = pytest.mark.gpu

NET_TOL = 1e-4  # normwise, end to end (the suite's existing bar, tests/test_gpu_multi_out.py)


def _run_chain(c, ws, x, padded, leaky, what):
    """The chain on a guarded plan: (output, describe text).  The modes the chain is there for are
    asserted from the text, so a plan that chose another kernel fails here."""
    g = DC.chain_graph(c, ws, padded, leaky)
    entries = dnn_hip.lower_graph(g)
    assert entries is not None
    assert all(isinstance(e, dnn_hip.PaddedConvEntry) == padded for e in entries if not isinstance(e, dnn_hip.PoolEntry))
    kw = {} if padded else {"leaky_variant": leaky or 1}
    gp = RS.GuardedPlan(c["B"], c["shape"], entries, latency=c["latency"], **kw)
    try:
        text = gp.plan.describe()
        DC.check_chain_lines(c, text)
        return gp.run(x, what), text
    finally:
        gp.close()


# ------------------------------------------------------------------ 1. bit-exact where it can be
@pytest.mark.parametrize("name", list(DC.MODE_CHAINS))
def test_unit_scale_affine_equals_bias_add_bit_for_bit(monkeypatch, name):
    """scale = 1, shift = b, pads = SAME's, the same leaky: v * 1 - (-b) == v + b exactly, so the
    padded entry and dnn_plan_add_conv with biases = b run the same kernels to the same bits."""
    c = DC.MODE_CHAINS[name]
    for k, v in c["env"].items():
        monkeypatch.setenv(k, v)
    x, ws = DC.chain_tensors(c, 1, unit_scale=True)
    for leaky in (2, 1, 0):
        got, text = _run_chain(c, ws, x, True, leaky, f"{name} padded leaky {leaky}")
        want, ref_text = _run_chain(c, ws, x, False, leaky, f"{name} bias_add leaky {leaky}")
        assert DC.conv_lines(text) == ref_text.splitlines()  # the same modes, configs and splits
        assert all(l.endswith(" affine") for l in text.splitlines() if l.startswith("conv "))
        K.check_bits(got, want, f"{name} leaky {leaky}: padded entry vs dnn_plan_add_conv")
        assert float(np.abs(want).max()) > 0.1


# ------------------------------------------------------------------ 2. against the oracle
@pytest.mark.parametrize("name", list(DC.MODE_CHAINS))
def test_mixed_scales_against_the_oracle(monkeypatch, name):
    """Positive, negative and exactly-zero scales of mixed magnitude with a nonzero shift, leaky 2
    and none: every chain's output within NET_TOL normwise of the float64 oracle (a pool fused
    before the epilogue must take the window's minimum where the scale is negative)."""
    c = DC.MODE_CHAINS[name]
    for k, v in c["env"].items():
        monkeypatch.setenv(k, v)
    x, ws = DC.chain_tensors(c, 2, unit_scale=False)
    for _, scale, shift in ws:
        assert (scale > 0).any() and (scale < 0).any() and (scale == 0).sum() == 2 and (shift != 0).all()
    for leaky in (2, 0):
        got, _ = _run_chain(c, ws, x, True, leaky, f"{name} leaky {leaky}")
        want = DC.chain_oracle(c, x, ws, leaky)
        err = R.normwise_err(got, want)
        print(f"affine epilogue, {name}, leaky {leaky}: normwise error {err:.3e}")
        assert err < NET_TOL, f"{name} leaky {leaky}: normwise error {err:.3e} >= {NET_TOL:.0e}"
        # the zero-scale channels are the shift (through the leaky), whatever the conv gave
        last = ws[-1]
        if c["ops"][-1][0] == "conv":
            z = DO.affine_leaky(np.zeros(1), np.zeros(1), last[2][1:2], leaky == 2)[0]
            assert (got[..., 1] == z).all()


def test_c16_pingpong_kernel_with_the_affine_epilogue(monkeypatch):
    """conv1's ping-pong kernel runs only on batch grids (>= 4 tiles of 16 x 26 per CU: 11 frames of
    208 x 208): with negative and zero scales it equals the persistent kernel (DNN_HIP_X3_C16PP=0,
    the form the small chains above hold to the oracle) bit for bit, and the first and last frame
    are within NET_TOL of the oracle."""
    c = DC._chain(11, (208, 208, 16), [DC.P1, ("conv", 3, 32), DC.P2, ("conv", 3, 64)],
                  [["mode=patch_x3", "+pool2x2s2"], ["mode=patch_x3"]])
    x, ws = DC.chain_tensors(c, 4, unit_scale=False)
    outs = {}
    for arm in ("1", "0"):
        monkeypatch.setenv("DNN_HIP_X3_C16PP", arm)
        eng = dnn_hip.DnnInferenceEngine(DC.chain_graph(c, ws, True, 2), False, device=0)
        DC.check_chain_lines(c, eng.plan().describe())
        outs[arm] = eng.run(x)
    K.check_bits(outs["1"], outs["0"], "ping-pong vs persistent 16-channel x3 conv")
    ends = dict(c, B=2)
    err = R.normwise_err(outs["1"][[0, 10]], DC.chain_oracle(ends, x[[0, 10]], ws, 2))
    print(f"affine epilogue, 16-channel ping-pong kernel: normwise error {err:.3e}")
    assert err < NET_TOL


# ------------------------------------------------------------------ 3. explicit padding
PAD_CASES = {
    # name: (B, (H, W, C), kernel, stride, (pad_h, pad_w), oc, pool stride or None, mode)
    "s2_8x8_implicit": (3, (8, 8, 32), 3, 2, (1, 1), 64, None, "implicit"),
    "s2_7x7_implicit": (3, (7, 7, 32), 3, 2, (1, 1), 64, None, "implicit"),
    "s2_6x10_implicit": (1, (6, 10, 32), 3, 2, (1, 1), 48, None, "implicit"),
    "s2_8x8_c16": (3, (8, 8, 16), 3, 2, (1, 1), 32, None, "implicit"),
    "s2_8x8_gemm": (3, (8, 8, 5), 3, 2, (1, 1), 24, None, "gemm"),
    "s2_7x7_gemm": (1, (7, 7, 3), 3, 2, (1, 1), 16, None, "gemm"),
    "s2_6x10_gemm": (3, (6, 10, 5), 3, 2, (1, 1), 24, None, "gemm"),
    "s2_16x16_pool": (3, (16, 16, 32), 3, 2, (1, 1), 64, 2, "implicit"),   # the pool fused behind a stride-2 conv
    "s2_12x10_splitk": (1, (12, 10, 256), 3, 2, (1, 1), 768, None, "implicit"),
    "k1_s1_p0": (3, (9, 12, 64), 1, 1, (0, 0), 125, None, "direct_a"),
    "k1_s2_p0": (1, (9, 12, 64), 1, 2, (0, 0), 128, None, "implicit"),
    "k3_s1_p1": (3, (10, 9, 32), 3, 1, (1, 1), 48, None, "implicit"),
    "k5_s1_p2": (3, (9, 11, 32), 5, 1, (2, 2), 64, None, "implicit"),     # top pad 2: flat input addresses
    "k5_s1_p2_gemm": (1, (9, 11, 5), 5, 1, (2, 2), 24, None, "gemm"),
    "k7_s2_p3": (3, (20, 18, 3), 7, 2, (3, 3), 16, None, "gemm"),
    "k7_s2_p3_c32": (1, (12, 13, 32), 7, 2, (3, 3), 32, None, "gemm"),
    "k3_s1_p0": (3, (10, 9, 32), 3, 1, (0, 0), 48, None, "implicit"),
    "k3_s1_p0_gemm": (1, (10, 9, 5), 3, 1, (0, 0), 24, None, "gemm"),
    "k3_s1_p2": (3, (7, 9, 32), 3, 1, (2, 2), 64, None, "implicit"),     # pad beyond k // 2: a frame that grows
    "k3_s1_p0x1": (1, (9, 8, 32), 3, 1, (0, 1), 64, None, "implicit"),   # pad_h != pad_w
    "k3_p2_pool_no_direct": (3, (10, 12, 3), 3, 1, (2, 2), 16, 2, "gemm"),  # conv0's shape, pads the direct kernels decline
    "k3_p1_pool_direct": (1, (10, 12, 3), 3, 1, (1, 1), 16, 2, "direct"),
}


@pytest.mark.parametrize("name", list(PAD_CASES))
def test_explicit_padding_against_the_oracle(name):
    B, shape, k, s, pads, oc, pool, mode = PAD_CASES[name]
    rng = np.random.default_rng(81000 + sorted(PAD_CASES).index(name))
    x = rng.standard_normal((B,) + shape).astype(np.float32)
    kern = (rng.standard_normal((k, k, shape[2], oc)) * np.sqrt(2.0 / (k * k * shape[2]))).astype(np.float32)
    scale = rng.uniform(0.5, 2.0, oc).astype(np.float32)
    scale[::3] *= np.float32(-1)
    scale[1] = 0
    shift = rng.uniform(-1.5, 1.5, oc).astype(np.float32)
    g = DC.padded_graph(B, shape, [kern], [s], [pads], [scale], [shift], [2], [pool])
    entries = dnn_hip.lower_graph(g)
    gp = RS.GuardedPlan(B, shape, entries)
    try:
        oh, ow = (shape[0] + 2 * pads[0] - k) // s + 1, (shape[1] + 2 * pads[1] - k) // s + 1
        line = gp.plan.describe().splitlines()[0]
        assert f" pad={pads[0]},{pads[1]} affine" in line and f"mode={mode} " in line, line
        assert ("+pool2x2s2" in line) == (pool is not None and mode != "gemm"), line
        want = DO.affine_leaky(DO.conv_padded(x, kern, s, *pads), scale, shift, True)
        assert want.shape == (B, oh, ow, oc)
        if pool:
            want = R.max_pool2d(want, [1, 2, 2, 1], [1, pool, pool, 1], "SAME")
        for n in (B, 1):
            got = gp.run(x[:n], f"{name} n={n}")  # (guards, canaries and finiteness checked inside)
            err = R.normwise_err(got, want[:n])
            print(f"explicit padding, {name}, n={n}: normwise error {err:.3e}")
            assert err < NET_TOL, f"{name}: normwise error {err:.3e} >= {NET_TOL:.0e}"
    finally:
        gp.close()
    # under SAME the stride-2 cases on an even map sample one pixel off: the oracle tells them apart
    if s == 2 and pads == (1, 1) and k == 3 and shape[0] % 2 == 0 and pool is None:
        same = DO.affine_leaky(R.conv2d(x, kern, strides=(1, 2, 2, 1), padding="SAME"), scale, shift, True)
        assert same.shape == want.shape and R.normwise_err(same, want) > 0.05


def test_padded_entry_on_a_finalized_plan_is_refused():
    g = DC.padded_graph(1, (8, 8, 32), [np.ones((3, 3, 32, 8), np.float32)], [1], [(1, 1)])
    plan = dnn_hip.Plan.from_graph(g)
    try:
        before = plan.describe()
        rc = dnn_hip.mylib.dnn_plan_add_conv_padded(plan.h, 3, 3, 8, 1, 1, 1, 1, None, None, None, 0)
        assert rc != 0 and "finalized" in dnn_hip.last_error()
        assert plan.describe() == before
    finally:
        plan.close()


def test_shape_only_padded_entries_with_a_copied_arena():
    """kernel == NULL declares the shape only (upload=False): with the uploading plan's arena copied
    in, the outputs are its outputs bit for bit (scale and shift travel in the arena)."""
    import torch
    c = DC.MODE_CHAINS["implicit_pool_out_x3"]
    x, ws = DC.chain_tensors(c, 3, unit_scale=False)
    entries = dnn_hip.lower_graph(DC.chain_graph(c, ws, True, 2))
    wb, sb = dnn_hip.Plan.memory(c["B"], c["shape"], entries)
    bufs = [(torch.zeros(wb, dtype=torch.uint8, device="cuda"), torch.zeros(sb, dtype=torch.uint8, device="cuda"))
            for _ in range(2)]
    plans = [dnn_hip.Plan(c["B"], c["shape"], entries, device=0, weights_ptr=w.data_ptr(), workspace_ptr=s.data_ptr(),
                          upload=(k == 0)) for k, (w, s) in enumerate(bufs)]
    try:
        assert plans[0].describe() == plans[1].describe()
        bufs[1][0].copy_(bufs[0][0])
        xd = torch.from_numpy(x).cuda()
        ys = [torch.empty((c["B"],) + p.out_shape, device="cuda") for p in plans]
        for p, y in zip(plans, ys):
            p.run_device(c["B"], xd.data_ptr(), y.data_ptr())
        torch.cuda.synchronize()
        K.check_bits(ys[1].cpu().numpy(), ys[0].cpu().numpy(), "shape-only plan with the copied arena")
        assert R.normwise_err(ys[0].cpu().numpy(), DC.chain_oracle(c, x, ws, 2)) < NET_TOL
    finally:
        for p in plans:
            p.close()


def test_nodes_run_one_by_one_like_the_plan():
    """The per-node run() of Conv2DPadded, ScaleShift and LeakyReLUF32 (the debug path)."""
    B, shape = 2, (7, 9, 8)
    rng = np.random.default_rng(5)
    x = rng.standard_normal((B,) + shape).astype(np.float32)
    kern = (rng.standard_normal((3, 3, 8, 12)) * 0.2).astype(np.float32)
    scale, shift = rng.uniform(-2, 2, 12).astype(np.float32), rng.uniform(-1, 1, 12).astype(np.float32)
    g = DC.padded_graph(B, shape, [kern], [2], [(1, 1)], [scale], [shift], [2])
    want = DO.affine_leaky(DO.conv_padded(x, kern, 2, 1, 1), scale, shift, True)
    got = dnn_hip.DnnInferenceEngine(g, False, device=0).run(x)
    assert R.normwise_err(got, want) < NET_TOL
    g.in_node.set_input(x)
    nodes = dnn_hip.DnnInferenceEngine(g, False, device=0)._run_nodes()
    assert nodes.shape == want.shape and R.normwise_err(nodes, want) < NET_TOL
    # the element-wise nodes are exact given their input: fp32 multiply, fp32 add, fp32 max
    conv = g.out_node.in_node.in_node.result
    aff = (conv * scale).astype(np.float32) + shift
    K.check_bits(g.out_node.in_node.result, aff, "ScaleShift.run")
    K.check_bits(nodes, R.leaky_relu_avx(aff), "LeakyReLUF32.run")


# ------------------------------------------------------------------ 4. imported narrow models
def _model(tmp_path, model, B, latency=False, **kw):
    size = DC.NARROW[model][1]
    cfg = DC.narrow_cfg(model)
    secs = D.parse_cfg(cfg)
    path = str(tmp_path / f"{model}.weights")
    D.save_weights(path, DC.darknet_layers(secs))
    layers = D.load_weights(path, secs)  # what the model reads back from the file
    m = D.DarknetModel(cfg, path, in_shape=[B, size, size, 3], latency=latency, **kw)
    return m, secs, layers, size


@pytest.mark.parametrize("latency", [False, True], ids=["batch", "latency"])
@pytest.mark.parametrize("model", list(DC.NARROW))
def test_imported_narrow_model_against_the_darknet_oracle(tmp_path, model, latency):
    B = 1 if latency else 2
    m, secs, layers, size = _model(tmp_path, model, B, latency)
    x = synth.frames([2, 3][:B], shape=(size, size, 3))
    outs = [o.copy() for o in m.inference(x)]
    assert m.sess._plan is not None  # the plan ran, not the node-by-node path
    text = m.sess.plan().describe()
    convs = [l for l in text.splitlines() if l.startswith("conv ")]
    assert len(convs) == sum(s["type"] == "convolutional" for s in secs) and all(" affine" in l for l in convs)
    assert all((" latency" in l) == latency for l in convs)
    want = DO.forward(secs, layers, x)
    assert [o.shape for o in outs] == [w.shape for w in want] and len(outs) == len(m.yolos)
    for k, (o, w) in enumerate(zip(outs, want)):
        K.check_finite(o, f"{model} head {k}")
        assert 0.01 < float(np.abs(w).mean()) < 100
        err = R.normwise_err(o, w)
        print(f"imported narrow {model} ({'latency' if latency else 'batch'}) head {k}: normwise error {err:.3e}")
        assert err < NET_TOL, f"{model} head {k}: normwise error {err:.3e} >= {NET_TOL:.0e}"
    if latency:
        return
    # detect: the device decode's rows are the numpy multi-label oracle's on the device outputs
    assert m.head.nms == "per_class" and m.head.labels == "multi"
    assert (m.head.score_thr, m.head.iou_thr) == (0.5, 0.45)
    multi = MO.Multi(tuple(m.head.scales), "logistic")
    gold = [LO.detect_or_code([o[i] for o in outs], multi) for i in range(B)]
    rows = m.detect(x, raise_errors=False)
    assert len(rows) == B
    for i in range(B):
        HK.same_rows(rows[i], gold[i], f"{model} detect image {i}")
    # ... and at a low threshold, where the narrow model has rows to compare
    low, _, _, _ = _model(tmp_path, model, B, score_thr=0.05)
    multi = MO.Multi(tuple(low.head.scales), "logistic")
    rows = low.detect(x, raise_errors=False)
    outs = [o.copy() for o in low.inference(x)]
    gold = [LO.detect_or_code([o[i] for o in outs], multi) for i in range(B)]
    for i in range(B):
        HK.same_rows(rows[i], gold[i], f"{model} detect image {i} at score 0.05")
    print(f"imported narrow {model}: rows at score 0.05: {[r if isinstance(r, int) else len(r) for r in rows]}")


def test_imported_model_with_too_many_boxes_infers_without_a_head():
    """Above the decode's 16,384 boxes the model has head=None: inference works, detect raises the
    decode's error.  (A narrow YOLOv3-tiny at 1088 x 1088: 34^2 x 3 + 68^2 x 3 = 17,340 boxes.)"""
    cfg = D.cfg_text("yolov3-tiny", classes=3, width=1088, height=1088, width_div=16)
    m = D.DarknetModel(cfg, DC.darknet_layers(D.parse_cfg(cfg)))
    assert m.in_shape == (1, 1088, 1088, 3) and m.head is None
    x = synth.frames([0], shape=(1088, 1088, 3))
    outs = m.inference(x)
    assert m.sess._plan is not None and [o.shape for o in outs] == [(1, 34, 34, 24), (1, 68, 68, 24)]
    for o in outs:
        K.check_finite(o, "1088 x 1088 narrow YOLOv3-tiny")
    with pytest.raises(ValueError, match="17340 boxes"):
        m.detect(x)


# ------------------------------------------------------------------ 5. graph replay
def test_graph_replay_of_an_imported_model_equals_the_eager_run(tmp_path):
    import torch
    m, secs, layers, size = _model(tmp_path, "yolov3", 2)
    plan = m.sess.plan()
    xs = [synth.frames([0, 1], shape=(size, size, 3)), synth.frames([2, 3], shape=(size, size, 3))]
    d_in = torch.empty((2, size, size, 3), dtype=torch.float32, device="cuda")
    d_out = torch.empty((2,) + plan.out_shape, dtype=torch.float32, device="cuda")
    stream = torch.cuda.Stream()

    def run(x, how):
        d_in.copy_(torch.from_numpy(x))
        d_out.fill_(float("nan"))
        torch.cuda.synchronize()
        if how == "graph":
            plan.run_graph(2, d_in.data_ptr(), d_out.data_ptr(), stream.cuda_stream)
        else:
            plan.run_device(2, d_in.data_ptr(), d_out.data_ptr())
        torch.cuda.synchronize()
        taps = []
        for k, shape in enumerate(plan.tap_shapes):
            t = np.empty((2,) + shape, np.float32)
            dnn_hip._check(plan.lib.dnn_plan_tap_read_host(plan.h, k, 2, dnn_hip._vp(t)), "tap_read_host")
            taps.append(t)
        return taps + [d_out.cpu().numpy()]

    eager = [run(x, "run") for x in xs]
    assert not np.array_equal(eager[0][-1], eager[1][-1])
    for i in (0, 1, 0):  # capture, replay on other frames, replay again
        for k, (a, b) in enumerate(zip(run(xs[i], "graph"), eager[i])):
            K.check_bits(a, b, f"graph replay, frames {i}, output {k}")
