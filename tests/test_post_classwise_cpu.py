"""Host-only checks of the per-class NMS: the conditions the cases of tests/post_classwise_cases.py
rely on, the oracle (tests/post_classwise_oracle.py) against post_multi_oracle where they must
agree, the decomposition the kernel relies on, and the new entries' argument checks."""
import ctypes

import numpy as np
import pytest

import dnn_hip
import post_classwise_cases as CK
import post_classwise_oracle as CO
import post_head_cases as HK
import post_head_oracle as O
import post_multi_cases as K
import post_multi_oracle as MO
import post_numpy as PN
import yolo_post

NEW_SYMBOLS = ("dnn_yolo_multi_nms_workspace", "dnn_yolo_postprocess_multi_nms", "dnn_yolo_postprocess_multi_nms_host")


# ------------------------------------------------------------------------------ the cases
@pytest.mark.parametrize("name", sorted(CK.PARITY))
def test_seeded_batches_meet_their_conditions(name):
    grids, classes, n, _, thr = CK.PARITY[name]
    preds, refs = CK.parity(name)
    any_refs = CK.parity_any(name)
    assert [p.shape for p in preds] == [(n, g, g, 3 * (5 + classes)) for g in grids]
    print(f"{name}: per class {CK.counts_of(refs)}, any class {CK.counts_of(any_refs)}")
    assert CK.counts_of(refs) == CK.PER_CLASS[name] and CK.counts_of(any_refs) == CK.ANY_CLASS[name]
    codes = [r for r in refs if isinstance(r, int)]
    assert 1 <= len(codes) <= n // 4
    assert sum(len(r) for r in refs if not isinstance(r, int)) >= 100
    differ = [i for i in range(n) if refs[i] != any_refs[i]]
    assert differ
    # an image carries -2 under one rule only, in both directions
    only_pc = [i for i in range(n) if refs[i] == -2 and any_refs[i] != -2]
    only_any = [i for i in range(n) if any_refs[i] == -2 and refs[i] != -2]
    assert only_pc and only_any
    if name == "small":
        assert only_pc == [1] and only_any == [4] and len(differ) == 8  # the six clean images differ as well
    if name == "yolov3":  # empty and one-element class segments occur
        multi = K.yolov3_multi(grids, classes, score_thr=thr)
        stats = {}
        CO.detect([p[0] for p in preds], multi, stats)
        sizes = np.bincount(stats["classes"], minlength=classes)
        assert (sizes == 0).any() and (sizes == 1).any() and sizes.max() <= 16


def test_skew_case_is_saturated_and_skewed():
    preds, rows, classes = CK.skew()
    multi = CK.skew_multi()
    assert [p.shape for p in preds] == [(1, 8, 8, 30), (1, 16, 16, 30), (1, 32, 32, 30)]
    assert len(classes) == 4032 == sum(MO.scale_boxes(h) for h in multi.scales)  # every box is a candidate
    assert list(np.bincount(classes, minlength=5)) == CK.SKEW_SIZES
    assert len(rows) == CK.SKEW_KEPT
    assert len(MO.detect([p[0] for p in preds], multi)) == CK.SKEW_KEPT_ANY
    scores = [r[5] for r in rows]
    assert scores == sorted(scores, reverse=True) and len({r[0] for r in rows}) == 5
    assert [r[0] for r in rows] != sorted(r[0] for r in rows)  # global order, not class-major


def test_bounds_case_has_its_segment_sizes_and_raises_nothing():
    multi, preds = CK.bounds_multi(), CK.bounds_preds()
    stats = {}
    rows = CO.detect([preds[0]], multi, stats)  # raises nothing
    assert tuple(np.bincount(stats["classes"], minlength=6)) == CK.BOUNDS_SIZES == (1, 63, 64, 0, 65, 129)
    # every third box of a class shares its pixels with the box before it: one of the two is dropped
    kept = np.bincount([r[0] for r in rows], minlength=6)
    assert list(kept) == [s - s // 3 for s in CK.BOUNDS_SIZES]
    boxes = [d for d in MO.decode([preds[0]], multi) if d[1] > np.float32(0.3)]
    by_class = {c: [d[0] for d in boxes if d[2] == c] for c in range(6)}
    for c, bs in by_class.items():
        assert all(bs[j] == bs[j - 1] for j in range(2, len(bs), 3)), c
    assert len({float(d[1]) for d in boxes}) == len(boxes) == 322
    # the classes interleave in the output
    assert [r[0] for r in rows[:12]] != sorted(r[0] for r in rows[:12])
    # the same construction around the one-wave / whole-workgroup threshold
    stats = {}
    rows = CO.detect([CK.bounds_preds(CK.THRESHOLD_SIZES)[0]], CK.bounds_multi(CK.THRESHOLD_SIZES), stats)
    assert tuple(np.bincount(stats["classes"], minlength=4)) == CK.THRESHOLD_SIZES == (256, 257, 255, 320)
    assert list(np.bincount([r[0] for r in rows], minlength=4)) == [s - s // 3 for s in CK.THRESHOLD_SIZES]


# ------------------------------------------------------------------------------ the oracle
def test_with_one_class_the_two_rules_are_the_same_function():
    """On the embedded reference cases read as one-class heads: every box keeps its geometry and
    objectness (the first 6 of an anchor's 25 values), and the one class logit is the first."""
    n = 0
    for name, (pred, gold) in HK.ms_golden().items():
        head = O.voc_head(*gold["grid"])
        p1 = np.ascontiguousarray(O.as_boxes(pred, head)[..., :6]).reshape(head.grid_h, head.grid_w, 30)
        h1 = O.Head(head.grid_h, head.grid_w, 5, 1, head.anchors, 32.0, 0.3, 0.3)
        for mode in ("softmax", "logistic"):
            m1 = MO.Multi((h1,), mode)
            want = MO.detect_or_code([p1], m1)
            assert CO.detect_or_code([p1], m1) == want, (name, mode)
            n += 0 if isinstance(want, int) else len(want)
    assert n > 400


def test_per_class_is_the_any_class_loop_on_each_class_alone_merged_by_score():
    """The decomposition the kernel relies on, on every clean image of `small`: the class-agnostic
    loop (post_multi_oracle.detect's) on each class's candidates alone, the kept boxes merged by
    (score descending, global index)."""
    grids, classes, n, _, thr = CK.PARITY["small"]
    preds, refs = CK.parity("small")
    multi = K.yolov3_multi(grids, classes, score_thr=thr)
    head = multi.scales[0]
    clean = 0
    for i in range(n):
        if isinstance(refs[i], int):
            continue
        boxes = MO.decode([p[i] for p in preds], multi)
        cand = [(g, d) for g, d in enumerate(boxes) if d[1] > np.float32(thr)]
        merged = []
        for c in range(classes):
            seg = sorted((t for t in cand if t[1][2] == c), key=lambda t: t[1][1], reverse=True)
            kept = []
            for g, d in seg:
                hits = [PN.iou(d[0], k[1][0]) > head.iou_thr for k in kept]
                if not any(hits):
                    kept.append((g, d))
            merged += kept
        merged.sort(key=lambda t: (-t[1][1], t[0]))
        rows = [(d[2], d[0][0], d[0][1], d[0][2], d[0][3], float(d[1])) for _, d in merged]
        assert rows == refs[i], f"image {i}"
        clean += 1
    assert clean >= 6


# ------------------------------------------------------------------------------ the entries
def test_both_libraries_export_the_new_entries():
    for name in ("libdnn_hip.so", "libdnn_hip_avx.so"):
        lib = dnn_hip.load_library(name)
        for sym in NEW_SYMBOLS:
            assert hasattr(lib, sym), (name, sym)


def test_bad_nms_mode_is_refused_by_all_three_entries_and_mode_0_workspace_is_unchanged():
    lib = yolo_post._lib
    head = yolo_post.MultiHead.yolov3(64, 64, classes=3)
    b = ctypes.c_ulonglong(77)
    preds = [np.zeros((1,) + s, np.float32) for s in head.pred_shapes]
    ptrs = (ctypes.c_void_p * 3)(*[p.ctypes.data for p in preds])
    dets = np.zeros((1, head.boxes), yolo_post.DETECTION_DTYPE)
    counts = np.full(1, 12345, np.int32)
    for mode in (2, -1):
        assert lib.dnn_yolo_multi_nms_workspace(ctypes.byref(head.c), 1, mode, ctypes.byref(b)) == -2
        assert "nms_mode" in dnn_hip.last_error() and b.value == 77
        # (refused before any device call: these run without a GPU; the device entry gets host
        # pointers it never touches)
        assert lib.dnn_yolo_postprocess_multi_nms_host(ctypes.byref(head.c), ptrs, 1, dets.ctypes.data, head.boxes,
                                                       counts.ctypes.data, mode) == -2
        assert "nms_mode" in dnn_hip.last_error()
        assert lib.dnn_yolo_postprocess_multi_nms(ctypes.byref(head.c), ptrs, 1, dets.ctypes.data, head.boxes,
                                                  counts.ctypes.data, dets.ctypes.data, 1 << 20, mode, None) == -2
        assert "nms_mode" in dnn_hip.last_error()
        assert counts[0] == 12345
    for n in (0, 1, 5):
        want = ctypes.c_ulonglong()
        assert lib.dnn_yolo_multi_workspace(ctypes.byref(head.c), n, ctypes.byref(want)) == 0
        for mode in (0, 1):
            assert lib.dnn_yolo_multi_nms_workspace(ctypes.byref(head.c), n, mode, ctypes.byref(b)) == 0
            assert b.value == want.value == n * 252 * 40
    # the description is still checked first, as in the existing entries
    bad = yolo_post.MultiStruct()
    assert lib.dnn_yolo_multi_nms_workspace(ctypes.byref(bad), 1, 1, ctypes.byref(b)) == -2
    assert "scales" in dnn_hip.last_error()


def test_multihead_nms_argument():
    h = yolo_post.MultiHead.yolov3(416, 416)
    assert h.nms == "any" and yolo_post.NMS_MODES == {"any": 0, "per_class": 1}
    p = yolo_post.MultiHead.yolov3(416, 416, nms="per_class")
    assert p.nms == "per_class" and bytes(p.c) == bytes(h.c)  # the C description is unchanged
    assert p.workspace_bytes(2) == h.workspace_bytes(2) == 2 * 10647 * 40
    assert "per_class" in repr(p) and "NMS" not in repr(h)
    assert repr(h) == ("MultiHead(13x13x3, 26x26x3, 52x52x3; 80 classes, logistic, score > 0.3, IoU > 0.3)")
    assert yolo_post.MultiHead.yolov3_tiny(416, 416, nms="per_class").nms == "per_class"
    assert yolo_post.MultiHead.yolov3_tiny(416, 416).nms == "any"
    assert yolo_post.MultiHead(h.scales).nms == "any"
    assert yolo_post.MultiHead(h.scales, "logistic", "per_class").nms == "per_class"
    for bad in ("classwise", 1, None):
        with pytest.raises(ValueError):
            yolo_post.MultiHead(h.scales, nms=bad)
    with pytest.raises(ValueError):
        yolo_post.MultiHead.yolov3(416, 416, nms="classwise")
