"""The classifier tail's kernels on the GPU (csrc/classify.hip) through dnn_hip.Plan and classify.TopK,
each against a few lines of float64 numpy."""
import numpy as np
import pytest

import classify
import dnn_hip

pytestmark = pytest.mark.gpu

f8 = np.float64
MAX = dnn_hip.SOFTMAX_MAX_CLASSES
AVG, SOFT = dnn_hip.AvgPoolEntry, dnn_hip.SoftmaxEntry
# The largest |float32 numpy softmax - float64 softmax| over every softmax case below is 2.58e-08 (the
# two-class rows, p = 0.88: measured on these inputs); the device's expf gets four times that.
SOFTMAX_TOL = 4 * 2.58e-08


def run_plan(entries, x, batch=None):
    plan = dnn_hip.Plan(batch or x.shape[0], x.shape[1:], [e() for e in entries])
    try:
        return plan.run_host(x)
    finally:
        plan.close()


def softmax_rows(classes):
    """Three rows of standard-normal logits, the second offset by +90 and the third by -90."""
    x = np.random.default_rng(classes).standard_normal((3, classes)).astype(np.float32)
    x[1] += np.float32(90)
    x[2] -= np.float32(90)
    return x


def softmax_ref(x, dtype=f8):
    e = np.exp(x.astype(dtype) - x.astype(dtype).max(1, keepdims=True))
    return e / e.sum(1, keepdims=True)


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("shape", [(1, 1, 8), (5, 3, 3), (7, 7, 260), (13, 13, 1000), (2, 2, 125)], ids=str)
def test_avgpool_is_within_the_summation_bound_of_the_float64_mean(shape, n):
    """|out - mean| <= (H W + 2) 2^-24 mean|x|: H W - 1 adds in any order, one division, fp32."""
    x = np.random.default_rng(sum(shape)).standard_normal((n,) + shape).astype(np.float32)
    out = run_plan([AVG], x)
    assert out.shape == (n, 1, 1, shape[2])
    err = np.abs(out[:, 0, 0].astype(f8) - x.astype(f8).mean((1, 2)))
    bound = (shape[0] * shape[1] + 2) * 2.0 ** -24 * np.abs(x).astype(f8).mean((1, 2))
    print("avgpool", shape, n, "largest err / bound", (err / bound).max())
    assert (err <= bound).all()


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("classes", [1, 2, 63, 64, 65, 1000, MAX])
def test_softmax_matches_float64_and_sums_to_one(classes, n):
    x = softmax_rows(classes)[3 - n:]
    p = run_plan([SOFT], x.reshape(n, 1, 1, classes)).reshape(n, classes)
    err = np.abs(p.astype(f8) - softmax_ref(x)).max()
    off = np.abs(p.astype(f8).sum(1) - 1).max()
    print("softmax", classes, n, "err", err, "numpy fp32 err", np.abs(softmax_ref(x, np.float32) - softmax_ref(x)).max(),
          "|sum - 1|", off)
    assert err <= SOFTMAX_TOL
    assert off <= classes * 2.0 ** -23


@pytest.mark.parametrize("shape", [(5, 3, 65), (7, 7, 260)], ids=str)
@pytest.mark.parametrize("entries", [[AVG], [AVG, SOFT]], ids=["avgpool", "avgpool+softmax"])
def test_an_image_has_the_same_bits_in_a_batch_of_three_and_alone(entries, shape):
    x = np.random.default_rng(7).standard_normal((3,) + shape).astype(np.float32)
    both, alone = run_plan(entries, x), run_plan(entries, x[2:])
    assert np.array_equal(both[2].view(np.int32), alone[0].view(np.int32))
    assert not np.array_equal(both[2], both[1])


def test_a_row_longer_than_the_lds_limit_is_refused_with_a_message():
    x = np.zeros((1, MAX + 1), np.float32)
    out = np.full_like(x, 7)
    assert dnn_hip.mylib.dnn_softmax_host(dnn_hip._vp(x), dnn_hip._vp(out), 1, MAX + 1) != 0
    assert "DNN_SOFTMAX_MAX_CLASSES" in dnn_hip.last_error() and (out == 7).all()
    with pytest.raises(dnn_hip.DnnHipError, match="DNN_SOFTMAX_MAX_CLASSES"):
        dnn_hip.Plan(1, (1, 1, MAX + 1), [SOFT()])


@pytest.mark.parametrize("k", [1, 5, 16])
@pytest.mark.parametrize("classes", [17, 1000, 4097, MAX])
def test_topk_order_ties_and_a_nan_row(classes, k):
    """Rows 0 and 3: permutations of distinct values 0.05 apart (the order is exact in fp32 and float64
    alike); row 1: all equal, so indices 0..k-1; row 2 holds a NaN: its status, and nobody else's rows."""
    import torch
    rng = np.random.default_rng(classes + k)
    vals = ((np.arange(classes) - classes // 2) * 0.05).astype(np.float32)
    x = np.stack([rng.permutation(vals), np.full(classes, 0.25, np.float32), rng.permutation(vals), rng.permutation(vals)])
    x[2, classes // 3] = np.nan
    tk = classify.TopK(4, classes, k, "cuda:0")
    d = torch.from_numpy(x).cuda()
    tk.run(d.data_ptr(), 4, torch.cuda.current_stream().cuda_stream)
    index, score, status = (t.cpu().numpy() for t in (tk.index, tk.score, tk.status))
    assert status.tolist() == [0, 0, classify.TOPK_NAN, 0]
    for i in (0, 1, 3):
        want = np.argsort(-x[i].astype(f8), kind="stable")[:k]
        assert index[i].tolist() == want.tolist(), i
        assert np.array_equal(score[i].view(np.int32), x[i][want].view(np.int32)), i
    assert index[1].tolist() == list(range(k))
    assert (index[2] == -1).all() and np.isnan(score[2]).all()  # as TopK allocated them
    with pytest.raises(ValueError, match="image 2"):
        classify.TopK.to_rows(index, score, status)
    host = classify.topk_host(x, k)
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(host, (index, score, status)))
