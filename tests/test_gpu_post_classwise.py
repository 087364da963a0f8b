"""GPU: the multi-scale decode with per-class NMS (dnn_yolo_postprocess_multi_nms,
csrc/postprocess_multi.hip: yolo_multi_classwise_kernel) against tests/post_classwise_oracle.py:
seeded batches, mode 0 byte for byte against the existing entry, one class, a class that owns most
of the candidates, score ties, segment boundaries, the per-image contracts on guarded buffers, and
YOLO_V3 / YOLO_V3_TINY end to end."""
import ctypes

import numpy as np
import pytest

import dnn_hip
import plan_fuzz_checks as C
import post_classwise_cases as CK
import post_classwise_oracle as CO
import post_head_cases as HK
import post_head_oracle as O
import post_multi_cases as K
import post_multi_oracle as MO
import synth
import yolo_post

pytestmark = pytest.mark.gpu


def _device_multi(multi, nms="per_class"):
    return yolo_post.MultiHead(multi.scales, multi.class_mode, nms)


# ------------------------------------------------------------------ 1. seeded batches
@pytest.mark.parametrize("name", sorted(CK.PARITY))
def test_per_class_vs_oracle_seeded_batch(name):
    """All rows and codes equal the per-class oracle's (classes, corners and order identical,
    scores to the suite's rtol 1e-6); they are not the class-agnostic rows."""
    grids, classes, n, _, thr = CK.PARITY[name]
    preds, refs = CK.parity(name)
    head = _device_multi(K.yolov3_multi(grids, classes, score_thr=thr))
    rows = yolo_post.detect_batch_multi(preds, head, raise_errors=False)
    print(f"{name}: device {CK.counts_of(rows)}, oracle {CK.counts_of(refs)}")
    assert len(rows) == n
    for i, (r, ref) in enumerate(zip(rows, refs)):
        HK.same_rows(r, ref, f"{name} image {i}")
    assert CK.counts_of(refs) == CK.PER_CLASS[name]
    with pytest.raises(dnn_hip.DnnHipError):
        yolo_post.detect_batch_multi(preds, head)
    # the same head with nms="any" is the existing path and gives the other rule's counts
    any_rows = yolo_post.detect_batch_multi(preds, _device_multi(K.yolov3_multi(grids, classes, score_thr=thr), "any"),
                                            raise_errors=False)
    assert CK.counts_of(any_rows) == CK.ANY_CLASS[name]


# ------------------------------------------------------------------ 2. mode 0 is the existing entry
def _guarded(torch, dev, nbytes):
    t = torch.full((2 * C.GUARD_BYTES + nbytes,), C.POISON, dtype=torch.uint8, device=dev)
    return t, t[C.GUARD_BYTES:C.GUARD_BYTES + nbytes]


def test_mode_0_is_byte_equal_to_the_existing_entry():
    import torch
    dev = torch.device("cuda", 0)
    grids, classes, n, _, thr = CK.PARITY["small"]
    preds, _ = CK.parity("small")
    head = _device_multi(K.yolov3_multi(grids, classes, score_thr=thr), "any")
    max_det = 60  # below some counts, above others
    n_ws = head.workspace_bytes(n)
    stream = torch.cuda.current_stream(dev).cuda_stream
    xs = [torch.from_numpy(np.array(p)).to(dev) for p in preds]
    ptrs = (ctypes.c_void_p * 3)(*[x.data_ptr() for x in xs])
    got = []
    for new in (False, True):
        dets_all, dets = _guarded(torch, dev, n * max_det * 40)
        counts_all, counts = _guarded(torch, dev, n * 4)
        ws_all, ws = _guarded(torch, dev, n_ws)
        if new:
            rc = dnn_hip.mylib.dnn_yolo_postprocess_multi_nms(
                ctypes.byref(head.c), ptrs, n, dets.data_ptr(), max_det, counts.data_ptr(), ws.data_ptr(), n_ws, 0, stream)
        else:
            rc = dnn_hip.mylib.dnn_yolo_postprocess_multi(
                ctypes.byref(head.c), ptrs, n, dets.data_ptr(), max_det, counts.data_ptr(), ws.data_ptr(), n_ws, stream)
        dnn_hip._check(rc, "decode")
        torch.cuda.synchronize()
        got.append([t.cpu().numpy() for t in (dets_all, counts_all, ws_all)])
        for buf, what in zip(got[-1], ("dets", "counts", "workspace")):
            C.check_guard(buf, what)
    for a, b, what in zip(got[0], got[1], ("dets", "counts", "workspace")):
        assert a.tobytes() == b.tobytes(), what
    counts = got[1][1][C.GUARD_BYTES:C.GUARD_BYTES + 4 * n].view(np.int32)
    assert list(counts) == CK.ANY_CLASS["small"]


# ------------------------------------------------------------------ 3. one class
def test_one_class_at_16128_boxes_equals_the_recorded_rows():
    preds, ref = K.cap()
    head = _device_multi(K.cap_multi())
    assert head.boxes == 16128 and head.n_classes == 1 and head.nms == "per_class" and len(ref) > 2000
    rows = yolo_post.detect_batch_multi(preds, head, raise_errors=False)[0]
    HK.same_rows(rows, ref, "cap 16128, per class")
    assert yolo_post.detect_batch_multi(preds, head, raise_errors=False)[0] == rows


# ------------------------------------------------------------------ 4. one class owns most candidates
def test_skewed_saturated_classes_vs_oracle():
    """4032 candidates, 2638 of them of class 0 (42 blocks) beside four segments of about 350 (six
    blocks each): all long enough for the whole-workgroup pass, one after the other: 1678 rows."""
    preds, ref, _ = CK.skew()
    head = _device_multi(CK.skew_multi())
    assert head.boxes == 4032
    rows = yolo_post.detect_batch_multi(preds, head, raise_errors=False)[0]
    print("skew:", rows if isinstance(rows, int) else len(rows), "rows, oracle", len(ref))
    HK.same_rows(rows, list(ref), "skew")
    assert len(rows) == CK.SKEW_KEPT
    assert yolo_post.detect_batch_multi(preds, head, raise_errors=False)[0] == rows


# ------------------------------------------------------------------ 5. ties
def test_score_ties_across_and_inside_classes_come_out_in_global_index_order():
    a = O.Head(1, 1, 1, 3, (0.25, 0.25), 32.0, 0.3, 0.3)              # one box: [12, 12, 20, 20]
    b = O.Head(4, 4, 2, 3, (0.5, 0.5, 0.5, 0.5), 16.0, 0.3, 0.3)      # 16 cells x 2 identical anchors of 8 x 8 px
    pa = np.zeros((1, 1, 1, 1, 8), np.float32)
    pb = np.zeros((1, 4, 4, 2, 8), np.float32)
    pb[..., 4] = -20.0                                                # not candidates ...

    def hot(c):  # objectness 2, p(class c) = 1.0f, the others 2e-9: one score, bit for bit
        v = np.full(4, -20.0, np.float32)
        v[0] = 2.0
        v[1 + c] = 20.0
        return v

    # (boxes of one class share a row of cells: the reference's IoU has no clamp, and two boxes
    # disjoint in BOTH axes have a positive "intersection")
    pa[0, 0, 0, 0, 4:] = hot(1)
    pb[0, 1, 2, 0, 4:] = hot(2)      # another place, another class
    pb[0, 1, 3, 1, 4:] = hot(1)      # another place, scale 0's class
    pb[0, 1, 1, 0, 4:] = hot(1)      # two identical boxes of different classes: both kept
    pb[0, 1, 1, 1, 4:] = hot(2)
    pb[0, 0, 3, 0, 4:] = hot(0)      # two identical boxes of one class: the lower index is kept
    pb[0, 0, 3, 1, 4:] = hot(0)
    pa, pb = pa.reshape(1, 1, 1, 8), pb.reshape(1, 4, 4, 16)
    for preds, scales, first in (([pa, pb], (a, b), 1), ([pb, pa], (b, a), 0)):
        multi = MO.Multi(scales, "logistic")
        want = CO.detect([p[0] for p in preds], multi)
        boxes = MO.decode([p[0] for p in preds], multi)
        cand = [g for g, d in enumerate(boxes) if d[1] > np.float32(0.3)]
        assert len(cand) == 7 and len({boxes[g][1] for g in cand}) == 1
        dup = [g for g in cand if boxes[g][2] == 0]
        assert len(dup) == 2 and dup[1] == dup[0] + 1 and boxes[dup[0]][0] == boxes[dup[1]][0]
        keep = [g for g in cand if g != dup[1]]  # global index order, the second duplicate dropped
        assert [r[:5] for r in want] == [(boxes[g][2],) + tuple(boxes[g][0]) for g in keep]
        twins = [r for r in want if r[1:5] == (20, 20, 28, 28)]
        assert [r[0] for r in twins] == [1, 2]
        rows = yolo_post.detect_batch_multi(preds, _device_multi(multi))[0]
        assert [r[:5] for r in rows] == [r[:5] for r in want]
        assert len({r[5] for r in rows}) == 1 and rows[0][5] == pytest.approx(want[0][5], rel=1e-6)
        assert (rows[0][1:5] == (12, 12, 20, 20)) == bool(first)


# ------------------------------------------------------------------ 6. segment boundaries
def test_class_segments_of_1_63_64_0_65_129_candidates():
    multi, preds = CK.bounds_multi(), CK.bounds_preds()
    want = CO.detect([preds[0]], multi)  # raises nothing (also asserted without a GPU)
    assert len(want) == sum(s - s // 3 for s in CK.BOUNDS_SIZES)
    rows = yolo_post.detect_batch_multi([preds], _device_multi(multi), raise_errors=False)[0]
    HK.same_rows(rows, want, "segment boundaries")


def test_class_segments_around_the_whole_workgroup_threshold():
    """256 candidates of a class are the most one wave takes alone; 257 and 320 go to the whole
    workgroup, 255 and 256 stay with a wave, in one image."""
    sizes = CK.THRESHOLD_SIZES
    multi, preds = CK.bounds_multi(sizes), CK.bounds_preds(sizes)
    want = CO.detect([preds[0]], multi)
    assert len(want) == sum(s - s // 3 for s in sizes)
    rows = yolo_post.detect_batch_multi([preds], _device_multi(multi), raise_errors=False)[0]
    HK.same_rows(rows, want, "threshold")


# ------------------------------------------------------------------ 7. per-image contracts
def test_per_class_per_image_contracts_on_guarded_buffers():
    """The device entry on guarded, poisoned dets / counts / workspace, nms_mode 1: max_det below
    the count (counts is the full number, the rows after max_det keep their poison), an error
    image writes no rows and does not change its neighbours, a non-finite corner of a
    non-candidate in the LAST scale gives -1, the guards survive."""
    import torch
    dev = torch.device("cuda", 0)
    grids, classes, n, _, thr = CK.PARITY["small"]
    preds, refs = CK.parity("small")
    head = _device_multi(K.yolov3_multi(grids, classes, score_thr=thr))
    bad = [p.copy() for p in preds]
    last = bad[2].reshape(n, -1, 5 + classes)
    last[2, -1, 2] = 100.0   # exp(100) = inf: int(inf) raises; objectness -20: not a candidate
    last[2, -1, 4] = -20.0
    want_bad = list(refs)
    assert refs[1] == -2 and not isinstance(refs[2], int)
    want_bad[2] = -1
    clean = [len(r) for r in refs if not isinstance(r, int)]
    max_det = min(clean) - 3
    assert max_det > 0
    n_ws = head.workspace_bytes(n)
    assert n_ws == n * 252 * 40
    stream = torch.cuda.current_stream(dev).cuda_stream
    entry = dnn_hip.mylib.dnn_yolo_postprocess_multi_nms
    for ps, want in ((preds, list(refs)), (bad, want_bad)):
        dets_all, dets = _guarded(torch, dev, n * max_det * 40)
        counts_all, counts = _guarded(torch, dev, n * 4)
        ws_all, ws = _guarded(torch, dev, n_ws)
        xs = [torch.from_numpy(np.array(p)).to(dev) for p in ps]
        ptrs = (ctypes.c_void_p * 3)(*[x.data_ptr() for x in xs])
        dnn_hip._check(entry(ctypes.byref(head.c), ptrs, n, dets.data_ptr(), max_det, counts.data_ptr(), ws.data_ptr(),
                             n_ws, 1, stream), "dnn_yolo_postprocess_multi_nms")
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
    # refused before any launch: a workspace one byte short, a bad nms_mode
    ws_all, ws = _guarded(torch, dev, n_ws)
    dets_all, dets = _guarded(torch, dev, n * max_det * 40)
    counts_all, counts = _guarded(torch, dev, n * 4)
    rc = entry(ctypes.byref(head.c), ptrs, n, dets.data_ptr(), max_det, counts.data_ptr(), ws.data_ptr(), n_ws - 1, 1,
               stream)
    assert rc == -2 and "workspace" in dnn_hip.last_error()
    rc = entry(ctypes.byref(head.c), ptrs, n, dets.data_ptr(), max_det, counts.data_ptr(), ws.data_ptr(), n_ws, 2,
               stream)
    assert rc == -2 and "nms_mode" in dnn_hip.last_error()
    torch.cuda.synchronize()
    assert (counts.cpu().numpy() == C.POISON).all() and (dets.cpu().numpy() == C.POISON).all()
    assert yolo_post.detect_batch_multi([p[:0] for p in preds], head) == []


# ------------------------------------------------------------------ 8. end to end
def _end_to_end(m, x):
    import torch
    assert m.head.nms == "per_class"
    outs = [o.copy() for o in m.inference(x)]
    multi = MO.Multi(tuple(m.head.scales), "logistic")
    want = [CO.detect_or_code([o[i] for o in outs], multi) for i in range(2)]
    any_want = [MO.detect_or_code([o[i] for o in outs], multi) for i in range(2)]
    print(f"narrow {type(m).__name__} end to end: per class {CK.counts_of(want)}, any class {CK.counts_of(any_want)}")
    rows = m.detect(x, raise_errors=False)
    assert len(rows) == 2
    for i in range(2):
        HK.same_rows(rows[i], want[i], f"detect image {i}")
    assert rows == yolo_post.detect_batch_multi(outs, m.head, raise_errors=False)
    stream = torch.cuda.current_stream().cuda_stream
    packed, total, counts = m.buffers.pack(2, stream)
    torch.cuda.synchronize()
    good = [r for r in rows if not isinstance(r, int)]
    t = int(total.cpu()[0])
    assert t == sum(len(r) for r in good)
    flat = yolo_post.DetectionBuffers.to_rows(packed.cpu().numpy()[None, :t], [t], max_det=t)[0] if good else []
    assert flat == [r for rr in good for r in rr]
    return rows


def test_yolov3_and_yolov3_tiny_detect_per_class_end_to_end():
    import yolov3
    import yolov3_tiny
    x = synth.frames([0, 1], shape=(64, 64, 3))
    m = yolov3.YOLO_V3([2, 64, 64, 3], synth.yolov3_weights(width_div=8, n_out=24), False,
                       head=yolo_post.MultiHead.yolov3(64, 64, 3, nms="per_class"))
    rows = _end_to_end(m, x)
    assert sum(len(r) for r in rows if not isinstance(r, int)) > 0
    t = yolov3_tiny.YOLO_V3_TINY([2, 64, 64, 3], synth.yolov3_tiny_weights(width_div=4, n_out=24), False,
                                 head=yolo_post.MultiHead.yolov3_tiny(64, 64, 3, nms="per_class"))
    _end_to_end(t, x)
