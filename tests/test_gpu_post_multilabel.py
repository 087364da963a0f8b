"""GPU: the multi-scale decode with multi-label detections (dnn_yolo_postprocess_multi_labels,
csrc/postprocess_multi.hip: yolo_multi_labels_kernel) against tests/post_multilabel_oracle.py:
seeded and dense batches, the rows of the single-label per-class head where no box has a second
label, labels_mode 0 byte for byte against the *_nms entry, one class, the candidate limit on
guarded buffers, the per-image contracts, score ties, and YOLO_V3 / YOLO_V3_TINY end to end."""
import ctypes

import numpy as np
import pytest

import dnn_hip
import plan_fuzz_checks as C
import post_classwise_cases as CK
import post_head_cases as HK
import post_head_oracle as O
import post_multi_cases as K
import post_multi_oracle as MO
import post_multilabel_cases as LK
import post_multilabel_oracle as LO
import synth
import yolo_post

pytestmark = pytest.mark.gpu


def _device_multi(multi, labels="multi"):
    return yolo_post.MultiHead(multi.scales, multi.class_mode, "per_class", labels)


def _guarded(torch, dev, nbytes):
    t = torch.full((2 * C.GUARD_BYTES + nbytes,), C.POISON, dtype=torch.uint8, device=dev)
    return t, t[C.GUARD_BYTES:C.GUARD_BYTES + nbytes]


def _run_guarded(head, preds, max_det, labels_mode=1, entry=None, short=0):
    """The device entry on guarded, poisoned dets / counts / workspace: (rc, counts as a list, dets
    as uint8 [n, max_det, 40], the workspace's bytes); the guards are checked."""
    import torch
    dev = torch.device("cuda", 0)
    n = preds[0].shape[0]
    n_ws = head.workspace_bytes(n)
    assert n_ws == n * head.boxes * 40
    stream = torch.cuda.current_stream(dev).cuda_stream
    xs = [torch.from_numpy(np.array(p)).to(dev) for p in preds]
    ptrs = (ctypes.c_void_p * len(xs))(*[x.data_ptr() for x in xs])
    dets_all, dets = _guarded(torch, dev, n * max_det * 40)
    counts_all, counts = _guarded(torch, dev, n * 4)
    ws_all, ws = _guarded(torch, dev, n_ws)
    entry = entry or dnn_hip.mylib.dnn_yolo_postprocess_multi_labels
    rc = entry(ctypes.byref(head.c), ptrs, n, dets.data_ptr(), max_det, counts.data_ptr(), ws.data_ptr(), n_ws - short,
               labels_mode, stream)
    torch.cuda.synchronize()
    for buf, what in ((dets_all, "dets"), (counts_all, "counts"), (ws_all, "workspace")):
        C.check_guard(buf.cpu().numpy(), what)
    return (rc, [int(c) for c in counts.cpu().numpy().view(np.int32)], dets.cpu().numpy().reshape(n, max_det, 40),
            ws.cpu().numpy().tobytes())


def _check_images(counts, dets, want, max_det, what):
    """counts are the full numbers or the codes, the first max_det rows are the oracle's, nothing is
    written after them or beside a code."""
    assert counts == LK.counts_of(want), what
    for i, w in enumerate(want):
        if isinstance(w, int):
            assert (dets[i] == C.POISON).all(), f"{what} image {i}: rows written beside the code {w}"
            continue
        k = min(len(w), max_det)
        rows = yolo_post.DetectionBuffers.to_rows(dets[i:i + 1, :k], [k], max_det=k)[0]
        HK.same_rows(rows, list(w[:k]), f"{what} image {i}")
        assert (dets[i, k:] == C.POISON).all(), f"{what} image {i}: rows written after the count"


# ------------------------------------------------------------------ 1. seeded and dense batches
@pytest.mark.parametrize("name", sorted(LK.SEEDED))
def test_multilabel_vs_oracle_seeded_batch(name):
    """All rows and codes equal the oracle's (classes, corners and order identical, scores to the
    suite's rtol 1e-6); raise_errors=True raises on the coded batch."""
    n = LK.SEEDED[name][2]
    preds, refs = LK.seeded(name)
    head = _device_multi(LK.seeded_multi(name))
    assert head.max_det == 252 * 3
    rows = yolo_post.detect_batch_multi(preds, head, raise_errors=False)
    print(f"{name}: device {LK.counts_of(rows)}, oracle {LK.counts_of(refs)}")
    assert len(rows) == n and LK.counts_of(refs) == LK.COUNTS[name]
    for i, (r, ref) in enumerate(zip(rows, refs)):
        HK.same_rows(r, ref, f"{name} image {i}")
    with pytest.raises(dnn_hip.DnnHipError):
        yolo_post.detect_batch_multi(preds, head)


@pytest.mark.parametrize("name", ["dense", "dense80"])
def test_multilabel_vs_oracle_dense(name):
    """More rows than boxes: every class segment above the whole-workgroup length (dense), every
    one a single wave's (dense80)."""
    preds, ref, stats = LK.dense(name)
    head = _device_multi(LK.dense_multi(name))
    assert head.boxes == 1008 and head.max_det == min(1008 * head.n_classes, 16384)
    rows = yolo_post.detect_batch_multi(preds, head, raise_errors=False)[0]
    print(f"{name}: device {rows if isinstance(rows, int) else len(rows)} rows, oracle {len(ref)} of "
          f"{stats['candidates']} candidates")
    HK.same_rows(rows, list(ref), name)
    assert len(rows) == LK.DENSE[name][5] > head.boxes
    assert yolo_post.detect_batch_multi(preds, head, raise_errors=False)[0] == rows


# ------------------------------------------------------------------ 2. where the label modes agree
def test_yolov3_rows_are_the_single_label_per_class_rows_exactly():
    """No box of this batch has a second label: the multi-label kernel gives the rows of the
    existing per-class kernel on the same device, scores bit for bit."""
    preds, _ = CK.parity("yolov3")
    multi = LK.yolov3_multi()
    rows = yolo_post.detect_batch_multi(preds, _device_multi(multi), raise_errors=False)
    single = yolo_post.detect_batch_multi(preds, _device_multi(multi, "argmax"), raise_errors=False)
    assert LK.counts_of(rows) == LK.COUNTS["yolov3"]
    assert rows == single


def test_labels_mode_0_is_byte_equal_to_the_nms_entry():
    preds, _ = CK.parity("yolov3")
    head = _device_multi(LK.yolov3_multi(), "argmax")
    max_det = 220  # below some counts, above others
    got = [_run_guarded(head, preds, max_det, 0),
           _run_guarded(head, preds, max_det, 1, entry=dnn_hip.mylib.dnn_yolo_postprocess_multi_nms)]
    assert got[0][0] == got[1][0] == 0
    assert got[0][1] == got[1][1] == LK.COUNTS["yolov3"]
    assert got[0][2].tobytes() == got[1][2].tobytes(), "dets"
    assert got[0][3] == got[1][3], "workspace"


def test_one_class_multilabel_equals_the_recorded_rows():
    preds, ref = K.cap()
    head = _device_multi(K.cap_multi())
    assert head.boxes == head.max_det == 16128 and head.n_classes == 1 and head.labels == "multi" and len(ref) > 2000
    rows = yolo_post.detect_batch_multi(preds, head, raise_errors=False)[0]
    HK.same_rows(rows, ref, "cap 16128, multi-label")


# ------------------------------------------------------------------ 3. the candidate limit
@pytest.mark.parametrize("name", sorted(LK.SANDWICH))
def test_candidate_limit_between_two_ordinary_images(name):
    """16,384 candidates are taken (128 rows, ties by index, then class), 16,385 and 16,910 give -3
    and no rows; the images before and after are the oracle's; nothing is written outside dets,
    counts and the workspace.  (The neighbours are ordinary seeded images of the case's own head:
    a batch has one description.)"""
    preds, refs = LK.sandwich(name)
    head = _device_multi(LK.sandwich_multi(name))
    assert (refs[1] == -3) == (name != "cap") and not isinstance(refs[0], int) and not isinstance(refs[2], int)
    max_det = max(len(refs[0]), len(refs[2]), 128) + 5
    rc, counts, dets, _ = _run_guarded(head, preds, max_det)
    assert rc == 0, dnn_hip.last_error()
    print(f"{name}: device {counts}, oracle {LK.counts_of(refs)}")
    _check_images(counts, dets, refs, max_det, name)
    if name == "cap":
        mid = yolo_post.DetectionBuffers.to_rows(dets[1:2], [128], max_det=max_det)[0]
        assert len(refs[1]) == 128 and len({r[5] for r in mid}) == 2
        assert [r[:5] for r in mid] == [r[:5] for r in LK.cap()[1]]


# ------------------------------------------------------------------ 4. per-image contracts
def test_multilabel_per_image_contracts_on_guarded_buffers():
    """labels_mode 1 on guarded, poisoned buffers: max_det below the count (counts is the full
    number, the rows after max_det keep their poison), an error image writes no rows and does not
    change its neighbours, a non-finite corner of a non-candidate in the LAST scale gives -1."""
    grids, classes, n = LK.SEEDED["small"][:3]
    preds, refs = LK.seeded("small")
    head = _device_multi(LK.seeded_multi("small"))
    bad = [p.copy() for p in preds]
    last = bad[2].reshape(n, -1, 5 + classes)
    last[2, -1, 2] = 100.0   # exp(100) = inf: int(inf) raises; objectness -20: not a candidate
    last[2, -1, 4] = -20.0
    want_bad = list(refs)
    assert refs[4] == -2 and not isinstance(refs[2], int)
    want_bad[2] = -1
    max_det = min(len(r) for r in refs if not isinstance(r, int)) - 3
    assert max_det > 0
    for ps, want, what in ((preds, list(refs), "small"), (bad, want_bad, "small with an infinite corner")):
        rc, counts, dets, _ = _run_guarded(head, ps, max_det)
        assert rc == 0, dnn_hip.last_error()
        _check_images(counts, dets, want, max_det, what)
    # refused before any launch: a workspace one byte short, a bad labels_mode
    rc, counts, dets, _ = _run_guarded(head, preds, max_det, short=1)
    assert rc == -2 and "workspace" in dnn_hip.last_error()
    assert counts == [-1] * n and (dets == C.POISON).all()  # (poisoned int32: 0xFFFFFFFF)
    rc, counts, dets, _ = _run_guarded(head, preds, max_det, labels_mode=2)
    assert rc == -2 and "labels_mode" in dnn_hip.last_error()
    assert counts == [-1] * n and (dets == C.POISON).all()  # (poisoned int32: 0xFFFFFFFF)
    assert yolo_post.detect_batch_multi([p[:0] for p in preds], head) == []


def test_a_bad_corner_wins_over_too_many_candidates():
    multi = LK.dense_multi("over")
    head = _device_multi(multi)
    preds = [p.copy() for p in LK.dense_preds("over")]
    assert yolo_post.detect_batch_multi(preds, head, raise_errors=False) == [-3]
    with pytest.raises(dnn_hip.DnnHipError, match="16384"):
        yolo_post.detect_batch_multi(preds, head)
    preds[2].reshape(-1, 5 + 5)[-1, 2] = 100.0  # exp(100) = inf, in the last box of the last scale
    assert LO.detect_or_code([p[0] for p in preds], multi) == -1
    assert yolo_post.detect_batch_multi(preds, head, raise_errors=False) == [-1]


# ------------------------------------------------------------------ 5. ties
def test_score_ties_come_out_in_index_then_class_order():
    """One row of 4 cells x 2 identical anchors of 8 x 8 px, 3 classes, every hot value the same
    score bit for bit: box 0 has all three classes; boxes 4 and 5 are identical and both of class 0
    (the lower index is kept); boxes 6 and 7 are identical, of classes 1 and 2 (both kept).  All
    boxes share the row, so no pair is disjoint in both axes."""
    h = O.Head(1, 4, 2, 3, (0.5, 0.5, 0.5, 0.5), 16.0, 0.3, 0.3)
    p = np.zeros((1, 4, 2, 8), np.float32)
    p[..., 4] = -20.0                                          # not candidates ...

    def hot(*cs):  # objectness 2, p(class) = 1.0f for cs, 2e-9 for the others
        v = np.full(4, -20.0, np.float32)
        v[0] = 2.0
        for c in cs:
            v[1 + c] = 20.0
        return v

    p[0, 0, 0, 4:] = hot(0, 1, 2)
    p[0, 2, 0, 4:] = hot(0)
    p[0, 2, 1, 4:] = hot(0)
    p[0, 3, 0, 4:] = hot(1)
    p[0, 3, 1, 4:] = hot(2)
    multi = MO.Multi((h,), "logistic")
    pred = p.reshape(1, 1, 4, 16)
    want = LO.detect([pred[0]], multi)
    cand = LO.candidates([pred[0]], multi)
    assert [(c[3], c[2]) for c in cand] == [(0, 0), (0, 1), (0, 2), (4, 0), (5, 0), (6, 1), (7, 2)]
    assert len({c[1] for c in cand}) == 1
    first, twin, pair = (4, 4, 12, 12), (36, 4, 44, 12), (52, 4, 60, 12)
    assert [r[:5] for r in want] == [(0,) + first, (1,) + first, (2,) + first, (0,) + twin, (1,) + pair, (2,) + pair]
    rows = yolo_post.detect_batch_multi([pred], _device_multi(multi))[0]
    assert [r[:5] for r in rows] == [r[:5] for r in want]
    assert len({r[5] for r in rows}) == 1 and rows[0][5] == pytest.approx(want[0][5], rel=1e-6)


# ------------------------------------------------------------------ 6. end to end
def _end_to_end(m, x):
    import torch
    assert m.head.nms == "per_class" and m.head.labels == "multi"
    outs = [o.copy() for o in m.inference(x)]
    multi = MO.Multi(tuple(m.head.scales), "logistic")
    want = [LO.detect_or_code([o[i] for o in outs], multi) for i in range(2)]
    print(f"narrow {type(m).__name__} end to end: multi-label {LK.counts_of(want)}")
    rows = m.detect(x, raise_errors=False)
    assert len(rows) == 2 and m.buffers.max_det == m.head.max_det  # more rows than boxes fit
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


def test_yolov3_and_yolov3_tiny_detect_multilabel_end_to_end():
    import yolov3
    import yolov3_tiny
    # (frames 2 and 3: on frames 0 and 1 the narrow YOLO_V3's many small stride-8 boxes give a zero
    # IoU denominator in both images, and a batch of two codes shows no rows)
    x = synth.frames([2, 3], shape=(64, 64, 3))
    m = yolov3.YOLO_V3([2, 64, 64, 3], synth.yolov3_weights(width_div=8, n_out=24), False,
                       head=yolo_post.MultiHead.yolov3(64, 64, 3, nms="per_class", labels="multi"))
    rows = _end_to_end(m, x)
    assert m.buffers.max_det == 756
    assert sum(len(r) for r in rows if not isinstance(r, int)) > 0
    t = yolov3_tiny.YOLO_V3_TINY([2, 64, 64, 3], synth.yolov3_tiny_weights(width_div=4, n_out=24), False,
                                 head=yolo_post.MultiHead.yolov3_tiny(64, 64, 3, nms="per_class", labels="multi"))
    _end_to_end(t, x)
