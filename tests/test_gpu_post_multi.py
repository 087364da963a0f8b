"""GPU: dnn_yolo_postprocess_multi (csrc/postprocess_multi.hip) — several heads, one sort and one
NMS — against the reference's own recorded output (one softmax scale), the multi-scale oracle
(tests/post_multi_oracle.py) on seeded three-scale batches, score ties, the 16,128-box saturated
case, its per-image contracts on guarded buffers, and YOLO_V3.detect end to end."""
import ctypes

import numpy as np
import pytest

import dnn_hip
import plan_fuzz_checks as C
import post_head_cases as HK
import post_head_oracle as O
import post_multi_cases as K
import post_multi_oracle as MO
import synth
import yolo_post

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ 1. the reference's own output
def test_one_softmax_scale_reproduces_the_reference_goldens(post_golden):
    """class_mode 0 with one scale is the reference's postprocessing: every embedded small-grid
    case (tests/golden/post_ms_golden.json) and every 13 x 13 case (post_golden.json) gives the
    recorded boxes, a recorded ZeroDivisionError gives -2."""
    n = raised = 0
    cases = [(f"ms {k}", tuple(g["grid"]), p, g) for k, (p, g) in HK.ms_golden().items()]
    cases += [(f"13x13 {k}", (13, 13), p, g) for k, (p, g) in post_golden.items()]
    for name, grid, pred, gold in cases:
        head = yolo_post.YoloHead(grid)
        multi = yolo_post.MultiHead([head], "softmax")
        rows = yolo_post.detect_batch_multi([pred[None]], multi, raise_errors=False)[0]
        if isinstance(gold, dict) and "raises" in gold:
            assert gold["raises"] == "ZeroDivisionError" and rows == -2, name
            raised += 1
            continue
        boxes = gold["boxes"] if isinstance(gold, dict) else gold
        got = [[b[0], list(b[1]), list(b[2])] for b in yolo_post.label_boxes(rows, head)]
        assert got == [list(b[:3]) for b in boxes], name
        n += len(rows)
    assert n > 400 and raised >= 1


# ------------------------------------------------------------------ 2. three scales, logistic
@pytest.mark.parametrize("name", sorted(K.PARITY))
def test_three_scales_vs_oracle_seeded_batch(name):
    """All rows and codes equal the oracle's (classes, corners and order identical, scores to the
    suite's rtol 1e-6)."""
    grids, classes, n, _, thr = K.PARITY[name]
    preds, refs = K.parity(name)
    head = K.device_multi(K.yolov3_multi(grids, classes, score_thr=thr))
    rows = yolo_post.detect_batch_multi(preds, head, raise_errors=False)
    assert len(rows) == n
    for i, (r, ref) in enumerate(zip(rows, refs)):
        HK.same_rows(r, ref, f"{name} image {i}")
    codes = sum(isinstance(r, int) for r in refs)
    assert 1 <= codes <= n // 4  # (also checked without a GPU)
    assert sum(len(r) for r in rows if not isinstance(r, int)) >= 100
    with pytest.raises(dnn_hip.DnnHipError):
        yolo_post.detect_batch_multi(preds, head)


@pytest.mark.parametrize("mode", ["softmax", "logistic"])
def test_four_scales_with_different_anchor_counts(mode):
    """The most scales the entry takes, each with its own grid shape, cell, anchors and anchor
    COUNT (2, 5, 1, 3), 9 classes (the 8-accumulator softmax sum): rows and codes equal the
    oracle's.  Seed 4 gives [44 | 61, -2, 30 | 31, 25 | 26] detections (softmax | logistic)."""
    anchors = (1.5, 2.0, 4.0, 3.0, 8.0, 9.5, 0.7, 0.9, 2.5, 1.2)
    scales = (O.Head(1, 2, 2, 9, anchors[:4], 64.0, 0.3, 0.3), O.Head(3, 3, 5, 9, anchors, 32.0, 0.3, 0.3),
              O.Head(2, 5, 1, 9, (3.0, 2.0), 16.0, 0.3, 0.3), O.Head(4, 4, 3, 9, anchors[2:8], 8.0, 0.3, 0.3))
    multi = MO.Multi(scales, mode)
    preds = MO.batch(4, multi, 4)
    refs = [MO.detect_or_code([p[i] for p in preds], multi) for i in range(4)]
    assert [isinstance(r, int) for r in refs] == [False, True, False, False] and refs[1] == -2
    head = K.device_multi(multi)
    assert head.boxes == 4 + 45 + 10 + 48 and head.n_out == [28, 70, 14, 42]
    rows = yolo_post.detect_batch_multi(preds, head, raise_errors=False)
    for i, (r, ref) in enumerate(zip(rows, refs)):
        HK.same_rows(r, ref, f"four scales {mode} image {i}")


# ------------------------------------------------------------------ 3. ties
def test_logistic_tie_takes_the_lower_class_and_score_ties_the_lower_global_index():
    a = O.Head(1, 1, 1, 3, (0.25, 0.25), 32.0, 0.3, 0.3)   # one box: [12, 12, 20, 20]
    b = O.Head(4, 4, 1, 3, (0.5, 0.5), 16.0, 0.3, 0.3)    # 16 boxes of 8 x 8 pixels
    pa = np.zeros((1, 1, 1, 8), np.float32)
    pb = np.zeros((1, 4, 4, 8), np.float32)
    pb[..., 4] = -20.0                      # not candidates ...
    hot = (2.0, -3.0, 20.0, 30.0)           # classes 1 and 2 both round to p = 1.0f: class 1 wins
    pa[0, 0, 0, 4:] = hot
    pb[0, 3, 3, 4:] = hot                   # ... but two with scale 0's score, bit for bit: global indices 16, 6
    pb[0, 1, 1, 4:] = hot
    multi = MO.Multi((a, b), "logistic")
    want = MO.detect([pa[0], pb[0]], multi)
    assert [r[:5] for r in want] == [(1, 12, 12, 20, 20), (1, 20, 20, 28, 28), (1, 52, 52, 60, 60)]
    assert len({r[5] for r in want}) == 1
    rows = yolo_post.detect_batch_multi([pa, pb], K.device_multi(multi))[0]
    assert [r[:5] for r in rows] == [r[:5] for r in want]
    assert len({r[5] for r in rows}) == 1 and rows[0][5] == pytest.approx(want[0][5], rel=1e-6)
    # the scales swapped: the 4 x 4 scale's boxes now have the lower global indices
    rows = yolo_post.detect_batch_multi([pb, pa], K.device_multi(MO.Multi((b, a), "logistic")))[0]
    assert [r[:5] for r in rows] == [(1, 20, 20, 28, 28), (1, 52, 52, 60, 60), (1, 12, 12, 20, 20)]
    assert [r[:5] for r in rows] == [r[:5] for r in MO.detect([pb[0], pa[0]], MO.Multi((b, a), "logistic"))]


# ------------------------------------------------------------------ 4. capacity
def test_saturated_at_16128_boxes():
    """16 x 16, 32 x 32 and 64 x 64 cells x 3 anchors, every box a candidate, 2256 kept: the
    recorded oracle rows of post_multi_cases.cap (tests/golden/post_multi_cap_golden.json)."""
    preds, ref = K.cap()
    head = K.device_multi(K.cap_multi())
    assert head.boxes == 16128 and len(ref) > 2000
    rows = yolo_post.detect_batch_multi(preds, head, raise_errors=False)[0]
    HK.same_rows(rows, ref, "cap 16128")
    # two launches are byte-equal
    again = yolo_post.detect_batch_multi(preds, head, raise_errors=False)[0]
    assert again == rows


# ------------------------------------------------------------------ 5. per-image contracts
def _guarded(torch, dev, nbytes):
    t = torch.full((2 * C.GUARD_BYTES + nbytes,), C.POISON, dtype=torch.uint8, device=dev)
    return t, t[C.GUARD_BYTES:C.GUARD_BYTES + nbytes]


def test_multi_per_image_contracts_on_guarded_buffers():
    """The device entry on guarded, poisoned dets / counts / workspace: max_det below the count
    (counts is the full number, the rows after max_det keep their poison), an error image writes
    no rows and does not change its neighbours, a non-finite corner of a non-candidate in the LAST
    scale gives -1, the guards survive."""
    import torch
    dev = torch.device("cuda", 0)
    grids, classes, n, _, thr = K.PARITY["small"]
    preds, refs = K.parity("small")
    multi = K.yolov3_multi(grids, classes, score_thr=thr)
    head = K.device_multi(multi)
    bad = [p.copy() for p in preds]
    last = bad[2].reshape(n, -1, 5 + classes)
    last[1, -1, 2] = 100.0   # exp(100) = inf: int(inf) raises; objectness -20: not a candidate
    last[1, -1, 4] = -20.0
    want_bad = list(refs)
    want_bad[1] = -1
    clean = [len(r) for r in refs if not isinstance(r, int)]
    max_det = min(clean) - 3
    assert max_det > 0
    n_ws = head.workspace_bytes(n)
    assert n_ws == n * 252 * 40
    stream = torch.cuda.current_stream(dev).cuda_stream
    for ps, want in ((preds, list(refs)), (bad, want_bad)):
        dets_all, dets = _guarded(torch, dev, n * max_det * 40)
        counts_all, counts = _guarded(torch, dev, n * 4)
        ws_all, ws = _guarded(torch, dev, n_ws)
        xs = [torch.from_numpy(np.array(p)).to(dev) for p in ps]
        ptrs = (ctypes.c_void_p * 3)(*[x.data_ptr() for x in xs])
        dnn_hip._check(dnn_hip.mylib.dnn_yolo_postprocess_multi(
            ctypes.byref(head.c), ptrs, n, dets.data_ptr(), max_det, counts.data_ptr(), ws.data_ptr(), n_ws, stream),
            "dnn_yolo_postprocess_multi")
        torch.cuda.synchronize()
        got_counts = list(counts.cpu().numpy().view(np.int32))
        assert got_counts == [w if isinstance(w, int) else len(w) for w in want]
        d = dets.cpu().numpy().reshape(n, max_det, 40)
        for i, w in enumerate(want):
            if isinstance(w, int):
                assert (d[i] == C.POISON).all(), f"image {i}: rows written beside the error code"
                continue
            rows = yolo_post.DetectionBuffers.to_rows(d[i:i + 1], [max_det], max_det=max_det)[0]
            HK.same_rows(rows, list(w[:max_det]), f"image {i}")
        for buf, what in ((dets_all, "dets"), (counts_all, "counts"), (ws_all, "workspace")):
            C.check_guard(buf.cpu().numpy(), what)
    # refused before any launch: a workspace one byte short, a NULL scale pointer
    ws_all, ws = _guarded(torch, dev, n_ws)
    dets_all, dets = _guarded(torch, dev, n * max_det * 40)
    counts_all, counts = _guarded(torch, dev, n * 4)
    rc = dnn_hip.mylib.dnn_yolo_postprocess_multi(ctypes.byref(head.c), ptrs, n, dets.data_ptr(), max_det,
                                                  counts.data_ptr(), ws.data_ptr(), n_ws - 1, stream)
    assert rc == -2 and "workspace" in dnn_hip.last_error()
    ptrs[1] = None
    rc = dnn_hip.mylib.dnn_yolo_postprocess_multi(ctypes.byref(head.c), ptrs, n, dets.data_ptr(), max_det,
                                                  counts.data_ptr(), ws.data_ptr(), n_ws, stream)
    assert rc == -2 and "pred[1]" in dnn_hip.last_error()
    torch.cuda.synchronize()
    assert (counts.cpu().numpy() == C.POISON).all()
    assert yolo_post.detect_batch_multi([p[:0] for p in preds], head) == []


# ------------------------------------------------------------------ 6. end to end
def test_yolov3_detect_end_to_end():
    """YOLO_V3.detect (plan and decode on the device, the decode reading the tap buffers in place)
    == the oracle on inference()'s outputs == postprocessing(outs); the buffers it leaves pack."""
    import torch
    import yolov3
    ws = synth.yolov3_weights(width_div=8, n_out=3 * (5 + 3))
    m = yolov3.YOLO_V3([2, 64, 64, 3], ws, False)
    assert [(s.grid_h, s.cell) for s in m.head.scales] == [(2, 32.0), (4, 16.0), (8, 8.0)]
    x = synth.frames([0, 1], shape=(64, 64, 3))
    outs = [o.copy() for o in m.inference(x)]
    multi = K.yolov3_multi((2, 4, 8), 3)
    want = [MO.detect_or_code([o[i] for o in outs], multi) for i in range(2)]
    print("narrow YOLOv3 end to end:", [w if isinstance(w, int) else len(w) for w in want], "detections")
    rows = m.detect(x, raise_errors=False)
    assert len(rows) == 2
    for i in range(2):
        HK.same_rows(rows[i], want[i], f"detect image {i}")
        if isinstance(want[i], int):
            with pytest.raises(dnn_hip.DnnHipError):
                m.postprocessing([o[i:i + 1] for o in outs])
        else:
            assert m.postprocessing([o[i:i + 1] for o in outs]) == yolo_post.label_boxes(rows[i], m.head)
    assert rows == yolo_post.detect_batch_multi(outs, m.head, raise_errors=False)
    assert sum(len(r) for r in rows if not isinstance(r, int)) > 0
    # n < batch, and the buffers stay usable with dnn_yolo_pack_detections
    assert m.detect(x[1:], raise_errors=False) == rows[1:]
    rows = m.detect(x, raise_errors=False)
    stream = torch.cuda.current_stream().cuda_stream
    packed, total, counts = m.buffers.pack(2, stream)
    torch.cuda.synchronize()
    good = [r for r in rows if not isinstance(r, int)]
    assert int(total.cpu()[0]) == sum(len(r) for r in good)
    flat = yolo_post.DetectionBuffers.to_rows(packed.cpu().numpy()[None, :int(total.cpu()[0])],
                                              [int(total.cpu()[0])], max_det=int(total.cpu()[0]))[0] if good else []
    assert flat == [r for rr in good for r in rr]
