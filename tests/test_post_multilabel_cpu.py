"""Host-only checks of the multi-label decode: the conditions the cases of
tests/post_multilabel_cases.py rely on, the oracle (tests/post_multilabel_oracle.py) against
post_classwise_oracle where no box has two labels, the new entries' argument checks and the Python
surface."""
import ctypes
import os

import numpy as np
import pytest

import dnn_hip
import post_classwise_cases as CK
import post_classwise_oracle as CO
import post_multi_cases as K
import post_multi_oracle as MO
import post_multilabel_cases as LK
import post_multilabel_oracle as LO
import yolo_post

NEW_SYMBOLS = ("dnn_yolo_multi_labels_workspace", "dnn_yolo_postprocess_multi_labels",
               "dnn_yolo_postprocess_multi_labels_host")


# ------------------------------------------------------------------------------ the cases
@pytest.mark.parametrize("name", sorted(LK.SEEDED))
def test_seeded_batches_meet_their_conditions(name):
    grids, classes, n, _, thr, mode = LK.SEEDED[name]
    preds, refs = LK.seeded(name)
    multi = LK.seeded_multi(name)
    assert multi.class_mode == mode and [p.shape for p in preds] == [(n, g, g, 3 * (5 + classes)) for g in grids]
    print(f"{name}: multi-label {LK.counts_of(refs)}")
    assert LK.counts_of(refs) == LK.COUNTS[name]
    codes = [r for r in refs if isinstance(r, int)]
    assert 1 <= len(codes) <= n // 4
    if name == "small":
        single = [CO.detect_or_code([p[i] for p in preds], multi) for i in range(n)]
        assert LK.counts_of(single) == LK.SMALL_SINGLE_LABEL  # image 4 raises under multi-label only
        for i in range(n):
            if isinstance(refs[i], int):
                continue
            boxes = LO.decode([p[i] for p in preds], multi)
            cand = sum(len(b[2]) for b in boxes)
            two = sum(len(b[2]) >= 2 for b in boxes)
            assert len(boxes) == 252 and 310 <= cand <= 328 and 95 <= two <= 125, (i, cand, two)
            assert len(refs[i]) > len(single[i])
            # the rows are in (score descending, global index, class) order: scores never rise
            scores = [r[5] for r in refs[i]]
            assert scores == sorted(scores, reverse=True)


def test_yolov3_batch_has_no_second_label_and_equals_the_per_class_oracle():
    preds, refs = LK.yolov3()
    assert LK.counts_of(refs) == LK.COUNTS["yolov3"] == CK.PER_CLASS["yolov3"]
    assert refs == CK.parity("yolov3")[1]  # scores included
    multi = LK.yolov3_multi()
    stats = {}
    LO.detect([p[0] for p in preds], multi, stats)
    assert len(set(stats["boxes"])) == len(stats["boxes"]) == stats["candidates"]
    assert 1 <= sum(isinstance(r, int) for r in refs) <= len(refs) // 4


@pytest.mark.parametrize("name", sorted(LK.DENSE))
def test_dense_cases_meet_their_conditions(name):
    grids, classes, thr, boxes, cand, want = LK.DENSE[name]
    preds, rows, stats = LK.dense(name)
    multi = LK.dense_multi(name)
    assert sum(MO.scale_boxes(h) for h in multi.scales) == boxes
    assert all(np.float32(h.score_thr) == np.float32(thr) for h in multi.scales)
    assert stats["candidates"] == cand
    sizes = np.bincount(stats["classes"], minlength=classes)
    labels = np.bincount(stats["boxes"], minlength=boxes)
    print(f"{name}: {cand} candidates, {sizes.min()}-{sizes.max()} per class, up to {labels.max()} labels per box")
    if name == "over":
        assert rows == want == -3 and cand > LO.MAX_CANDIDATES
        return
    assert not isinstance(rows, int) and len(rows) == want
    assert len(rows) > boxes  # more rows than boxes
    if name == "dense":  # every segment goes to the whole workgroup (csrc/postprocess_multi.hip: PC_BIG = 256)
        assert (sizes.min(), sizes.max(), labels.max()) == (369, 414, 9)
    else:                # every segment is one wave's
        assert (sizes.min(), sizes.max()) == (14, 40)


def test_cap_cases_sit_on_the_candidate_limit():
    preds, rows, cand = LK.cap()
    assert cand == 16384 == LO.MAX_CANDIDATES == yolo_post.MULTI_MAX_CANDIDATES
    assert not isinstance(rows, int) and len(rows) == 128 and sorted(r[0] for r in rows) == list(range(128))
    assert len({r[5] for r in rows}) == 2
    # every pair of boxes overlaps far above the IoU threshold: a class keeps its best box alone
    boxes = LO.decode([preds[0][0]], LK.cap_multi())
    l, t, r, b = (np.array([bx[0][k] for bx in boxes], np.float64)[:, None] for k in range(4))
    inter = (np.minimum(r, r.T) - np.maximum(l, l.T) + 1) * (np.minimum(b, b.T) - np.maximum(t, t.T) + 1)
    area = (r - l + 1) * (b - t + 1)
    assert 0.63 < (inter / (area + area.T - inter)).min() < 0.65
    # ties: both boxes of a score come out index first, then class ascending
    best = {0: None, 1: None}
    for g, bx in enumerate(boxes):
        if best[g % 2] is None or bx[1] > boxes[best[g % 2]][1]:
            best[g % 2] = g
    order = sorted(best.values(), key=lambda g: -boxes[g][1])
    want = [(c,) + tuple(boxes[g][0]) for g in order for c in range(128) if (g + c) % 2 == 0]
    assert [r[:5] for r in rows] == want
    _, rows1, cand1 = LK.cap(True)
    assert cand1 == 16385 and rows1 == -3


@pytest.mark.parametrize("name", sorted(LK.SANDWICH))
def test_limit_cases_sit_between_two_clean_images_of_their_head(name):
    preds, refs = LK.sandwich(name)
    assert all(p.shape[0] == 3 for p in preds)
    assert not isinstance(refs[0], int) and not isinstance(refs[2], int) and min(len(refs[0]), len(refs[2])) >= 100
    assert refs[1] == (list(LK.cap()[1]) if name == "cap" else -3)
    mid = [p[1] for p in preds]
    want = LK.dense_preds("over") if name == "over" else [LK.cap_preds(name == "cap+1")]
    assert all((m == w[0]).all() for m, w in zip(mid, want))


def test_codes_keep_their_precedence():
    """-1 (any corner) before -3 (too many candidates) before -2 (NMS)."""
    multi = LK.dense_multi("over")
    preds = [p[0].copy() for p in LK.dense_preds("over")]
    assert LO.detect_or_code(preds, multi) == -3
    last = preds[2].reshape(-1, 5 + 5)
    last[-1, 2] = 100.0  # exp(100) = inf
    assert LO.detect_or_code(preds, multi) == -1
    _, refs = LK.seeded("small")
    assert refs[4] == -2


# ------------------------------------------------------------------------------ the entries
def test_both_libraries_export_the_new_entries_and_the_header_declares_them():
    for name in ("libdnn_hip.so", "libdnn_hip_avx.so"):
        lib = dnn_hip.load_library(name)
        for sym in NEW_SYMBOLS:
            assert hasattr(lib, sym), (name, sym)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "dnn_hip_post.h")) as f:
        text = f.read()
    for sym in NEW_SYMBOLS:
        assert f"int {sym}(" in text, sym
    for define in ("#define DNN_YOLO_LABELS_ARGMAX 0", "#define DNN_YOLO_LABELS_MULTI 1",
                   "#define DNN_YOLO_MULTI_MAX_CANDIDATES 16384"):
        assert define in text, define
    assert "that is not built" not in text and "-3" in text


def test_bad_labels_mode_is_refused_by_all_three_entries_and_the_workspace_is_unchanged():
    lib = yolo_post._lib
    head = yolo_post.MultiHead.yolov3(64, 64, classes=3)
    b = ctypes.c_ulonglong(77)
    preds = [np.zeros((1,) + s, np.float32) for s in head.pred_shapes]
    ptrs = (ctypes.c_void_p * 3)(*[p.ctypes.data for p in preds])
    dets = np.zeros((1, head.boxes), yolo_post.DETECTION_DTYPE)
    counts = np.full(1, 12345, np.int32)
    for mode in (2, -1):
        assert lib.dnn_yolo_multi_labels_workspace(ctypes.byref(head.c), 1, mode, ctypes.byref(b)) == -2
        assert "labels_mode" in dnn_hip.last_error() and b.value == 77
        # (refused before any device call: these run without a GPU; the device entry gets host
        # pointers it never touches)
        assert lib.dnn_yolo_postprocess_multi_labels_host(ctypes.byref(head.c), ptrs, 1, dets.ctypes.data, head.boxes,
                                                          counts.ctypes.data, mode) == -2
        assert "labels_mode" in dnn_hip.last_error()
        assert lib.dnn_yolo_postprocess_multi_labels(ctypes.byref(head.c), ptrs, 1, dets.ctypes.data, head.boxes,
                                                     counts.ctypes.data, dets.ctypes.data, 1 << 20, mode, None) == -2
        assert "labels_mode" in dnn_hip.last_error()
        assert counts[0] == 12345 and not dets.view(np.uint8).any()
    for n in (0, 1, 5):
        want = ctypes.c_ulonglong()
        assert lib.dnn_yolo_multi_workspace(ctypes.byref(head.c), n, ctypes.byref(want)) == 0
        for mode in (0, 1):
            assert lib.dnn_yolo_multi_labels_workspace(ctypes.byref(head.c), n, mode, ctypes.byref(b)) == 0
            assert b.value == want.value == n * 252 * 40
    # the description is still checked first, as in the existing entries
    bad = yolo_post.MultiStruct()
    assert lib.dnn_yolo_multi_labels_workspace(ctypes.byref(bad), 1, 7, ctypes.byref(b)) == -2
    assert "scales" in dnn_hip.last_error()
    assert lib.dnn_yolo_postprocess_multi_labels_host(ctypes.byref(bad), ptrs, 1, dets.ctypes.data, head.boxes,
                                                      counts.ctypes.data, 7) == -2
    assert "scales" in dnn_hip.last_error()
    # mode 2 of the *_nms entries stays refused
    assert lib.dnn_yolo_multi_nms_workspace(ctypes.byref(head.c), 1, 2, ctypes.byref(b)) == -2
    assert "nms_mode" in dnn_hip.last_error()


# ------------------------------------------------------------------------------ the Python surface
def test_multihead_labels_argument():
    assert yolo_post.LABEL_MODES == {"argmax": 0, "multi": 1}
    assert yolo_post.NMS_MODES == {"any": 0, "per_class": 1}
    assert "16384" in yolo_post.ERRORS[-3] and set(yolo_post.ERRORS) == {-1, -2, -3}
    h = yolo_post.MultiHead.yolov3(416, 416)
    assert h.labels == "argmax" and h.nms == "any" and h.max_det == h.boxes == 10647
    assert repr(h) == ("MultiHead(13x13x3, 26x26x3, 52x52x3; 80 classes, logistic, score > 0.3, IoU > 0.3)")
    p = yolo_post.MultiHead.yolov3(416, 416, nms="per_class")
    assert p.labels == "argmax" and p.max_det == 10647 and "labels" not in repr(p)
    m = yolo_post.MultiHead.yolov3(416, 416, nms="per_class", labels="multi")
    assert m.labels == "multi" and m.nms == "per_class" and bytes(m.c) == bytes(h.c)  # the C description is unchanged
    assert m.max_det == 16384 and m.boxes == 10647
    assert m.workspace_bytes(2) == p.workspace_bytes(2) == 2 * 10647 * 40
    assert "labels multi" in repr(m) and "per_class" in repr(m)
    s = yolo_post.MultiHead.yolov3(64, 64, 3, nms="per_class", labels="multi")
    assert s.boxes == 252 and s.max_det == 756
    t = yolo_post.MultiHead.yolov3_tiny(416, 416, nms="per_class", labels="multi")
    assert t.labels == "multi" and t.max_det == 16384 and t.boxes == 2535
    assert yolo_post.MultiHead.yolov3_tiny(416, 416).labels == "argmax"
    assert yolo_post.MultiHead(h.scales).labels == "argmax"
    assert yolo_post.MultiHead(h.scales, "logistic", "per_class", "multi").labels == "multi"
    assert yolo_post.MultiHead(h.scales, "softmax", nms="per_class", labels="multi").max_det == 16384
    for kw in (dict(labels="multi"), dict(labels="multi", nms="any"), dict(labels="all", nms="per_class"),
               dict(labels=1, nms="per_class"), dict(labels=None, nms="per_class")):
        with pytest.raises(ValueError):
            yolo_post.MultiHead(h.scales, **kw)
    with pytest.raises(ValueError):
        yolo_post.MultiHead.yolov3(416, 416, labels="multi")
    with pytest.raises(ValueError):
        yolo_post.MultiHead.yolov3_tiny(416, 416, nms="per_class", labels="both")
    one = yolo_post.MultiHead(K.cap_multi().scales, "logistic", "per_class", "multi")
    assert one.n_classes == 1 and one.max_det == one.boxes == 16128
