"""TEST INFRASTRUCTURE ONLY — the multi-scale postprocessing with per-class NMS
(include/dnn_hip_post.h: DNN_YOLO_NMS_PER_CLASS) restated in numpy.  Decode, threshold and sort
are tests/post_multi_oracle.py's, imported, not copied; the IoU is post_numpy.iou.  The loop is
post_multi_oracle.detect's with one change: the kept list is filtered to the candidate's own class
BEFORE the IoUs are evaluated, so a zero denominator raises only for a pair of one class, and
every kept box of that class is evaluated (no early exit).

The rows come out in the global sorted order (score descending, ties to the lower global box
index), which is not class-major.
"""
import numpy as np

import post_multi_oracle as MO
import post_numpy as PN

_F = np.float32


def detect(preds, multi, stats=None):
    """Post-NMS detections [(class, left, top, right, bottom, score)] in output order."""
    head = multi.scales[0]
    thr = _F(head.score_thr)
    cand = [d for d in MO.decode(preds, multi) if d[1] > thr]
    cand.sort(key=lambda t: t[1], reverse=True)
    kept = []
    for c in cand:
        same = [k for k in kept if k[2] == c[2]]
        hits = [PN.iou(c[0], k[0]) > head.iou_thr for k in same]  # all of them: a zero denominator raises
        if not any(hits):
            kept.append(c)
    if stats is not None:
        stats["candidates"] = len(cand)
        stats["classes"] = [c[2] for c in cand]
    return [(k[2], k[0][0], k[0][1], k[0][2], k[0][3], float(k[1])) for k in kept]


def detect_or_code(preds, multi):
    """detect(), or the device's per-image code where the reference's arithmetic raises."""
    try:
        return detect(preds, multi)
    except ZeroDivisionError:
        return -2
    except (OverflowError, ValueError):
        return -1
