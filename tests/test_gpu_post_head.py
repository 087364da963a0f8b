"""GPU: dnn_yolo_postprocess_head (csrc/postprocess_head.hip) — the postprocessing of any
YOLOv2 head — against the reference's own function on small grids embedded in a 13 x 13
tensor, the generalised oracle (tests/post_head_oracle.py) on seeded batches, the 13 x 13
kernel bit for bit, and its per-image contracts on poisoned, guarded buffers.  The cases and
their oracle results are shared through tests/post_head_cases.py."""
import ctypes

import numpy as np
import pytest

import dnn_hip
import plan_fuzz_checks as C
import post_head_cases as K
import post_head_oracle as O
import post_numpy as PN
import ref_numpy as R
import synth
import yolo_post

pytestmark = pytest.mark.gpu

NET_TOL = 1e-4  # the suite's normwise bar for the 9-layer net (tests/test_gpu_parity.py)


# ------------------------------------------------------------------ 1. reference goldens
def test_embedded_reference_goldens():
    """Small VOC grids through detect_batch(head=...) == the reference's unmodified function on
    their 13 x 13 embedding (tests/golden/make_golden_post_ms.py)."""
    n = 0
    for name, (pred, gold) in K.ms_golden().items():
        head = yolo_post.YoloHead(tuple(gold["grid"]))
        rows = yolo_post.detect_batch(pred, head=head, raise_errors=False)[0]
        if "raises" in gold:
            assert rows == -2, name
            continue
        got = [[b[0], list(b[1]), list(b[2])] for b in yolo_post.label_boxes(rows, head)]
        assert got == gold["boxes"], name
        assert yolo_post.postprocessing(pred[None], head=head) == yolo_post.label_boxes(rows, head)
        n += len(rows)
    assert n > 400


# ------------------------------------------------------------------ 2. oracle parity
@pytest.mark.parametrize("name", sorted(K.PARITY))
def test_head_vs_oracle_seeded_batch(name):
    """Classes, corners and order identical, scores to rtol 1e-6; an image on which the oracle
    raises ZeroDivisionError gives -2."""
    spec, n, _ = K.PARITY[name]
    preds, refs = K.parity(name)
    rows = yolo_post.detect_batch(preds, head=K.device_head(spec), raise_errors=False)
    assert len(rows) == n
    for i, (r, ref) in enumerate(zip(rows, refs)):
        K.same_rows(r, ref, f"{name} image {i}")
    # what keeps this from passing vacuously (also checked without a GPU)
    assert sum(isinstance(r, int) for r in refs) <= n // 4
    if name in K.MULTI_CELL:
        assert sum(len(r) for r in rows if not isinstance(r, int)) >= 100


# ------------------------------------------------------------------ 3. saturation
@pytest.mark.parametrize("name", sorted(K.SATURATED))
def test_head_saturated_every_box_a_candidate(name):
    spec, _, raises = K.SATURATED[name]
    pred, ref, cand = K.saturated(name)
    head = K.device_head(spec)
    rows = yolo_post.detect_batch(pred, head=head, raise_errors=False)[0]
    if raises:
        assert ref == -2 and rows == -2
        return
    assert cand == head.boxes and len(ref) > 100
    K.same_rows(rows, ref, name)


def test_head_saturated_at_the_box_cap():
    """8192 boxes, all candidates, 2402 kept (the recorded oracle rows of post_head_cases.CAP)."""
    pred, ref = K.cap8192()
    head = K.device_head(K.CAP[0])
    assert head.boxes == yolo_post.MAX_BOXES and len(ref) > 2000
    K.same_rows(yolo_post.detect_batch(pred, head=head, raise_errors=False)[0], ref, "cap8192")


@pytest.mark.parametrize("n", K.DENSE)
def test_head_dense_every_candidate_kept(n):
    """The kept list in place over the consumed keys, growing by 64 for every 64 keys: the rows equal
    the oracle's (all n candidates), and two launches are byte-equal."""
    pred, ref = K.dense(n)
    head = K.device_head(K.dense_spec(n))
    assert head.boxes == n and len(ref) == n
    K.same_rows(yolo_post.detect_batch(pred, head=head, raise_errors=False)[0], ref, f"dense {n}")
    out = []
    for _ in range(2):
        dets = np.zeros((1, n), yolo_post.DETECTION_DTYPE)
        counts = np.zeros(1, np.int32)
        assert dnn_hip.mylib.dnn_yolo_postprocess_head_host(ctypes.byref(head.c), pred.ctypes.data, 1, dets.ctypes.data,
                                                            n, counts.ctypes.data) == 0, dnn_hip.last_error()
        out.append((dets.tobytes(), int(counts[0])))
    assert out[0] == out[1] and out[0][1] == n


# ------------------------------------------------------------------ 4. old entry == new entry
def _raw(preds, head=None):
    p = np.ascontiguousarray(preds, np.float32)
    n = len(p)
    dets = np.zeros((n, yolo_post.N_BOXES), yolo_post.DETECTION_DTYPE)
    counts = np.zeros(n, np.int32)
    if head is None:
        rc = dnn_hip.mylib.dnn_yolo_postprocess_host(p.ctypes.data, n, dets.ctypes.data, yolo_post.N_BOXES,
                                                     counts.ctypes.data)
    else:
        rc = dnn_hip.mylib.dnn_yolo_postprocess_head_host(ctypes.byref(head), p.ctypes.data, n, dets.ctypes.data,
                                                          yolo_post.N_BOXES, counts.ctypes.data)
    assert rc == 0, dnn_hip.last_error()
    return dets, counts


def test_voc_13x13_head_equals_the_13x13_kernel_bit_for_bit(post_golden):
    voc = yolo_post.HeadStruct()
    assert dnn_hip.mylib.dnn_yolo_head_voc(13, 13, ctypes.byref(voc)) == 0
    rng = np.random.default_rng(77)
    preds = np.stack([post_golden[k][0] for k in post_golden]
                     + [PN.synthetic_predictions(rng, tw_scale=(1.0 if i % 4 else 6.0)) for i in range(64)])
    d_old, c_old = _raw(preds)
    d_new, c_new = _raw(preds, voc)
    assert np.array_equal(c_old, c_new)
    assert d_old.tobytes() == d_new.tobytes()  # scores included; rows past the count stay zero in both
    assert (c_old > 0).sum() > 60 and (c_old == -2).sum() >= 1
    # and through the Python front: YoloHead(13) == head=None
    assert (yolo_post.detect_batch(preds[:16], head=yolo_post.YoloHead(13), raise_errors=False)
            == yolo_post.detect_batch(preds[:16], raise_errors=False))


# ------------------------------------------------------------------ 5. per-image contracts
def _guarded(torch, dev, nbytes):
    """uint8 device tensor: GUARD_BYTES of poison, nbytes of poison payload, GUARD_BYTES of poison."""
    t = torch.full((2 * C.GUARD_BYTES + nbytes,), C.POISON, dtype=torch.uint8, device=dev)
    return t, t[C.GUARD_BYTES:C.GUARD_BYTES + nbytes]


@pytest.mark.parametrize("grid", [(10, 10), (21, 21)], ids=["lds", "workspace"])
def test_head_per_image_contracts_on_guarded_buffers(grid):
    """max_det below the count: counts is the full number, only max_det rows are written and
    the rows after them keep their poison; a non-finite corner gives -1 and leaves the
    neighbours' results as they are without it; the guards around dets, counts and the
    workspace survive.  21 x 21 x 5 = 2205 boxes is a head whose boxes live in the workspace."""
    import torch
    dev = torch.device("cuda", 0)
    head = yolo_post.YoloHead(grid)
    ohead = O.voc_head(*grid)
    rng = np.random.default_rng(5)
    preds = np.stack([O.synthetic_predictions(rng, ohead) for _ in range(3)])
    refs = [O.detect_or_code(p, ohead) for p in preds]
    assert all(not isinstance(r, int) for r in refs)
    bad = preds.copy()
    bad.reshape(3, head.boxes, 25)[1, head.boxes - 1, 2] = 100.0  # exp(100) = inf: int(inf) raises; not a candidate
    bad.reshape(3, head.boxes, 25)[1, head.boxes - 1, 4] = -20.0
    max_det = min(len(r) for r in refs) - 3
    assert max_det > 0
    n_ws = head.workspace_bytes(3)
    assert (n_ws > 0) == (grid == (21, 21))
    stream = torch.cuda.current_stream(dev).cuda_stream
    for p, want in ((preds, [len(r) for r in refs]), (bad, [len(refs[0]), -1, len(refs[2])])):
        dets_all, dets = _guarded(torch, dev, 3 * max_det * 40)
        counts_all, counts = _guarded(torch, dev, 3 * 4)
        ws_all, ws = _guarded(torch, dev, n_ws)
        x = torch.from_numpy(p).to(dev)
        dnn_hip._check(dnn_hip.mylib.dnn_yolo_postprocess_head(
            ctypes.byref(head.c), x.data_ptr(), 3, dets.data_ptr(), max_det, counts.data_ptr(), ws.data_ptr(), n_ws,
            stream), "dnn_yolo_postprocess_head")
        torch.cuda.synchronize()
        got_counts = counts.cpu().numpy().view(np.int32)
        assert list(got_counts) == want
        d = dets.cpu().numpy().reshape(3, max_det, 40)
        for i in range(3):
            if want[i] < 0:
                assert (d[i] == C.POISON).all(), f"image {i}: rows written beside the error code"
                continue
            rows = yolo_post.DetectionBuffers.to_rows(d[i:i + 1], [max_det], max_det=max_det)[0]
            K.same_rows(rows, refs[i][:max_det], f"image {i}")
        for buf, what in ((dets_all, "dets"), (counts_all, "counts"), (ws_all, "workspace")):
            C.check_guard(buf.cpu().numpy(), what)
    # a count below max_det: the rows after it keep their poison (the canary rows)
    big = len(refs[0]) + 2
    dets_all, dets = _guarded(torch, dev, big * 40)
    counts_all, counts = _guarded(torch, dev, 4)
    ws_all, ws = _guarded(torch, dev, head.workspace_bytes(1))
    x = torch.from_numpy(preds[:1]).to(dev)
    dnn_hip._check(dnn_hip.mylib.dnn_yolo_postprocess_head(
        ctypes.byref(head.c), x.data_ptr(), 1, dets.data_ptr(), big, counts.data_ptr(), ws.data_ptr(),
        head.workspace_bytes(1), stream), "dnn_yolo_postprocess_head")
    torch.cuda.synchronize()
    assert counts.cpu().numpy().view(np.int32)[0] == len(refs[0])
    assert (dets.cpu().numpy().reshape(big, 40)[len(refs[0]):] == C.POISON).all()
    for buf, what in ((dets_all, "dets"), (counts_all, "counts"), (ws_all, "workspace")):
        C.check_guard(buf.cpu().numpy(), what)


def test_head_error_cases_and_empty_input():
    head = yolo_post.YoloHead((2, 3))
    p = np.zeros((2, 2, 3, 125), np.float32)
    p.reshape(2, 30, 25)[1, 17, 3] = 100.0
    with pytest.raises(dnn_hip.DnnHipError):
        yolo_post.detect_batch(p, head=head)
    assert yolo_post.detect_batch(p, head=head, raise_errors=False) == [[], -1]
    assert yolo_post.detect_batch(np.zeros((0, 2, 3, 125), np.float32), head=head) == []


# ------------------------------------------------------------------ 6. other thresholds
@pytest.mark.parametrize("name", ["voc19", "wide6"])
def test_head_other_thresholds_vs_oracle(name):
    spec, n, _ = K.PARITY[name]
    preds, refs = K.parity(name, 0.5, 0.45)
    base = K.parity(name)[1]
    assert [len(r) for r in refs if not isinstance(r, int)] != [len(r) for r in base if not isinstance(r, int)]
    rows = yolo_post.detect_batch(preds, head=K.device_head(spec, 0.5, 0.45), raise_errors=False)
    for i, (r, ref) in enumerate(zip(rows, refs)):
        K.same_rows(r, ref, f"{name} image {i} at score > 0.5, IoU > 0.45")
    assert sum(len(r) for r in rows if not isinstance(r, int)) >= 100


# ------------------------------------------------------------------ 7. determinism
@pytest.mark.parametrize("name", ["voc19", "voc40"])
def test_head_two_launches_are_byte_equal(name):
    spec = K.SATURATED[name][0]
    pred = K.saturated(name)[0]
    head = K.device_head(spec)
    out = []
    for _ in range(2):
        dets = np.zeros((1, head.boxes), yolo_post.DETECTION_DTYPE)
        counts = np.zeros(1, np.int32)
        assert dnn_hip.mylib.dnn_yolo_postprocess_head_host(ctypes.byref(head.c), pred.ctypes.data, 1,
                                                            dets.ctypes.data, head.boxes, counts.ctypes.data) == 0
        out.append((dets.tobytes(), int(counts[0])))
    assert out[0] == out[1] and out[0][1] > 100


# ------------------------------------------------------------------ 8. detection gather
def test_head_device_buffers_pack_and_gather_round_trip():
    """DetectionBuffers(head=...) -> run -> pack -> dist.gather_detections -> unpack at 10 x 10:
    dist.py sizes everything from DetectionBuffers.max_det and needs no head."""
    import torch
    import dist as D
    head = yolo_post.YoloHead(10)
    cases = [(k, v) for k, v in K.ms_golden().items() if v[1]["grid"] == [10, 10]]
    preds = np.stack([v[0] for _, v in cases])
    dev = torch.device("cuda", 0)
    buf = yolo_post.DetectionBuffers(len(preds), dev, head=head)
    assert buf.max_det == 500 and buf.dets.shape == (len(preds), 500, 40) and buf.packed.shape == (len(preds) * 500, 40)
    stream = torch.cuda.current_stream(dev).cuda_stream
    t = torch.from_numpy(preds).to(dev)
    buf.run(t.data_ptr(), len(preds), stream)
    torch.cuda.synchronize()
    rows = yolo_post.DetectionBuffers.to_rows(buf.dets.cpu().numpy(), buf.counts.cpu().numpy(), head=head,
                                              raise_errors=False)
    assert rows == yolo_post.detect_batch(preds, head=head, raise_errors=False)
    packed, total, counts = buf.pack(len(preds), stream)
    d, c = D.gather_detections(packed, total, counts, len(preds))
    assert D.unpack_detections(d, c) == rows
    assert len(d) == sum(len(r) for r in rows if not isinstance(r, int)) > 100
    # a head that needs the workspace owns one of the right size
    big = yolo_post.DetectionBuffers(2, dev, max_det=64, head=yolo_post.YoloHead(40))
    assert big.workspace.numel() == 2 * 8000 * 40 and big.max_det == 64


# ------------------------------------------------------------------ 9. end to end
@pytest.mark.parametrize("in_shape", [[2, 64, 96, 3], [1, 320, 320, 3]], ids=["2x3", "10x10"])
def test_front_end_at_other_input_sizes(in_shape, yolo_weights):
    """YOLO_V2_TINY at 64 x 96 (2 x 3 cells, the smallest non-square grid) and 320 x 320
    (10 x 10): the forward within NET_TOL of the float64 oracle, .postprocessing(out) equal to
    the generalised oracle on that same tensor."""
    import yolov2tiny
    b, h, w, _ = in_shape
    y2t = yolov2tiny.YOLO_V2_TINY(in_shape, yolo_weights, False)
    assert (y2t.head.grid_h, y2t.head.grid_w) == (h // 32, w // 32)
    x = synth.frames(range(b), tuple(in_shape[1:]))
    out = y2t.inference(x)
    assert out.shape == (b,) + y2t.head.pred_shape
    assert R.normwise_err(out, R.yolo_forward(yolo_weights, x)) < NET_TOL
    ohead = O.voc_head(h // 32, w // 32)
    for i in range(b):
        want = [(PN.CLASSES[c], (l, t), (r, bt), PN.COLORS[c]) for c, l, t, r, bt, _ in O.detect(out[i], ohead)]
        assert y2t.postprocessing(out[i:i + 1]) == want
