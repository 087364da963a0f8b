"""GPU: the reorg kernel against Darknet's definition (bit for bit), and narrow YOLOv2 / YOLOv2-tiny
imported from cfg text: the plan against the float64 forward, detect against the numpy multi-label
oracle, graph replay against the eager run, and the passthrough join as one launch."""
import numpy as np
import pytest
import torch

import darknet_cases as DC
import darknet_import as D
import dnn_hip
import plan_fuzz_checks as K
import post_head_cases as HK
import post_multi_oracle as MO
import post_multilabel_oracle as LO
import ref_numpy as R
import reorg_cases as RC
import synth

pytestmark = pytest.mark.gpu

NET_TOL = 1e-4  # normwise, end to end (the suite's existing bar)


@pytest.mark.parametrize("case", RC.KERNEL_CASES, ids=lambda c: "x".join(map(str, c)))
def test_reorg_kernel_bit_exact(case):
    h, w, ca, stride, cb, b_first, n = case
    a, b = RC.arange_inputs(n, h, w, ca, stride, cb)
    want = RC.reorg_loops(a, stride)
    if b is not None:
        want = np.concatenate([b, want] if b_first else [want, b], axis=3)
    out = np.full(want.shape, np.nan, np.float32)  # (dnn_reorg_host fills the device output with NaN too)
    rc = dnn_hip.mylib.dnn_reorg_host(dnn_hip._vp(a), dnn_hip._vp(b), dnn_hip._vp(out), n, h, w, ca, stride, cb, b_first)
    assert rc == 0, dnn_hip.last_error()
    np.testing.assert_array_equal(out.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("latency", [False, True], ids=["batch", "latency"])
@pytest.mark.parametrize("model", list(RC.NARROW))
def test_imported_narrow_yolov2_against_the_float64_forward(tmp_path, model, latency):
    B, size = 1 if latency else 2, RC.NARROW[model][1]
    cfg = RC.narrow_cfg(model)
    secs = RC.parse(cfg)
    path = str(tmp_path / f"{model}.weights")
    D.save_weights(path, DC.darknet_layers(secs))
    m = D.DarknetModel(cfg, path, in_shape=[B, size, size, 3], latency=latency, score_thr=0.05)
    x = synth.frames([2, 3][:B], shape=(size, size, 3))
    out = m.inference(x)[0].copy()
    assert m.sess._plan is not None  # the plan ran, not the node-by-node path
    plan = m.sess.plan()
    if model == "yolov2":  # the reorg and the concat are one step: no route or slice serves the pair
        assert "reorg 6x6x8 -> 3x3x160 stride=2 slot=1 (3x3x128) last" in plan.describe(), plan.describe()
        assert [k["name"] for k in plan.kernels() if not k["name"].startswith(("conv", "pool"))] == ["reorg0"]
    want = RC.forward(secs, D.load_weights(path, secs), x)
    assert out.shape == want.shape == (B, 3, 3, 5 * (5 + RC.CLASSES)) and 0.01 < float(np.abs(want).mean()) < 100
    K.check_finite(out, model)
    err = R.normwise_err(out, want)
    print(f"imported narrow {model} ({'latency' if latency else 'batch'}): normwise error {err:.3e}")
    assert err < NET_TOL, f"{model}: normwise error {err:.3e} >= {NET_TOL:.0e}"
    # detect: the device decode's rows are the numpy multi-label oracle's on the device output
    assert (m.head.class_mode, m.head.nms, m.head.labels) == ("softmax", "per_class", "multi")
    multi = MO.Multi(tuple(m.head.scales), "softmax")
    rows = m.detect(x, raise_errors=False)
    for i in range(B):
        HK.same_rows(rows[i], LO.detect_or_code([out[i]], multi), f"{model} detect image {i}")
    print(f"imported narrow {model}: rows at score 0.05: {[r if isinstance(r, int) else len(r) for r in rows]}")
    # graph capture, then a replay on other frames and one on the first: each equals the eager run
    xs = [x, synth.frames([0, 1][:B], shape=(size, size, 3))]
    d_in = torch.empty((B, size, size, 3), dtype=torch.float32, device="cuda")
    d_out = torch.empty((B,) + plan.out_shape, dtype=torch.float32, device="cuda")
    stream = torch.cuda.Stream()
    for i in (0, 1, 0):
        got = {}
        for how in ("run", "graph"):
            d_in.copy_(torch.from_numpy(xs[i]))
            d_out.fill_(float("nan"))
            torch.cuda.synchronize()
            if how == "graph":
                plan.run_graph(B, d_in.data_ptr(), d_out.data_ptr(), stream.cuda_stream)
            else:
                plan.run_device(B, d_in.data_ptr(), d_out.data_ptr())
            torch.cuda.synchronize()
            got[how] = d_out.cpu().numpy()
        K.check_bits(got["graph"], got["run"], f"{model}: graph replay, frames {i}")
    K.check_bits(got["run"], out, f"{model}: run_device vs inference")
