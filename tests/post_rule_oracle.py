"""TEST INFRASTRUCTURE ONLY: the multi-scale postprocessing under a dnn_yolo_rule (include/dnn_hip_post.h:
the dnn_yolo_postprocess_*_rule entries) on top of tests/post_xy_oracle.py.  Only the two new rules are
restated: the new_coords box form in numpy fp32 scalars as the header has it (with the gate conf > score_thr),
and DIoU on Python ints with math.pow in double; the rest is post_xy_oracle's pieces, order and NMS loop.
detect also returns the smallest |iou - penalty - iou_thr| over the pairs it evaluated (inf without one): the
device's pow may differ from libm's in the last place.  mode: post_xy_oracle.MODES; nms_kind "iou" or "diou"."""
import math

import numpy as np

import post_head_oracle as O
import post_multi_oracle as MO
import post_multilabel_oracle as LO
import post_numpy as PN
import post_xy_oracle as XO

_F = np.float32


def corners_new(q, row, col, b, head, s):  # [left, top, right, bottom] under new_coords = 1 and scale_x_y = s
    cell, s32, bias, two = _F(head.cell), _F(s), XO.xy_bias(s), _F(2.0)
    with np.errstate(over="ignore", invalid="ignore"):
        cx = _F(_F(_F(col) + _F(_F(q[0] * s32) + bias)) * cell)
        cy = _F(_F(_F(row) + _F(_F(q[1] * s32) + bias)) * cell)
        tw, th = _F(q[2] * two), _F(q[3] * two)
        hw = _F(_F(_F(_F(tw * tw) * _F(head.anchors[2 * b])) * cell) / two)
        hh = _F(_F(_F(_F(th * th) * _F(head.anchors[2 * b + 1])) * cell) / two)
        return [int(_F(cx - hw)), int(_F(cy - hh)), int(_F(cx + hw)), int(_F(cy + hh))]


def candidates_new(preds, multi, xy, mode):
    """[[corners, score, class, global index]] of one image under new_coords; every box's corners are converted."""
    thr = _F(multi.scales[0].score_thr)
    cand, g = [], 0
    for pred, head, s in zip(preds, multi.scales, xy):
        p = O.as_boxes(pred, head)
        for row, col, b in np.ndindex(head.grid_h, head.grid_w, head.n_anchors):
            q = p[row, col, b]
            cs, conf = corners_new(q, row, col, b, head, s), q[4]
            labels = range(head.n_classes)
            if mode != "multi":  # the first index of the largest value
                best = 0
                for c in labels[1:]:
                    best = c if q[5 + c] > q[5 + best] else best
                labels = [best]
            if conf > thr:
                cand += [[cs, _F(conf * q[5 + c]), c, g] for c in labels if _F(conf * q[5 + c]) > thr]
            g += 1
    return cand


def candidates_old(preds, multi, xy, mode):  # the same list for the logistic / exp box form, as post_xy_oracle.detect
    thr = _F(multi.scales[0].score_thr)
    cs = XO.all_corners(preds, multi, xy)
    if mode == "multi":
        return [[cs[g], sc, c, g] for g, (_, _, labels) in enumerate(LO.decode(preds, multi)) for c, sc in labels]
    return [[cs[g], d[1], d[2], g] for g, d in enumerate(MO.decode(preds, multi)) if d[1] > thr]


def diou_terms(a, b, beta):  # (iou, penalty) of two boxes [l, t, r, b]; a zero denominator raises ZeroDivisionError
    iou = PN.iou(a, b)
    d4 = ((a[0] + a[2]) - (b[0] + b[2])) ** 2 + ((a[1] + a[3]) - (b[1] + b[3])) ** 2
    w, h = max(a[2], b[2]) - min(a[0], b[0]) + 1, max(a[3], b[3]) - min(a[1], b[1]) + 1
    return iou, (math.pow(float(d4) / (4.0 * float(w * w + h * h)), beta) if d4 else 0.0)


def detect(preds, multi, xy, mode, new_coords=False, nms_kind="iou", beta=0.6):
    """(post-NMS detections [(class, left, top, right, bottom, score)] in output order, the smallest margin)."""
    assert mode in XO.MODES and nms_kind in ("iou", "diou") and not (nms_kind == "diou" and mode == "any")
    iou_thr = multi.scales[0].iou_thr
    cand = (candidates_new if new_coords else candidates_old)(preds, multi, xy, mode)
    if mode == "multi" and len(cand) > LO.MAX_CANDIDATES:
        raise LO.TooManyCandidates(len(cand))
    cand.sort(key=lambda t: t[1], reverse=True)
    kept, margin = [], math.inf
    for c in cand:
        hit = False
        for k in kept if mode == "any" else [k for k in kept if k[2] == c[2]]:  # all of them: a zero denominator raises
            iou, pen = diou_terms(c[0], k[0], beta) if nms_kind == "diou" else (PN.iou(c[0], k[0]), 0.0)
            margin = min(margin, abs(iou - pen - iou_thr))
            hit |= iou - pen > iou_thr
        if not hit:
            kept.append(c)
    return XO._rows(kept), margin


def detect_or_code(preds, multi, xy, mode, **rule):  # detect()'s rows, or the device's per-image code
    try:
        return detect(preds, multi, xy, mode, **rule)[0]
    except ZeroDivisionError:
        return -2
    except LO.TooManyCandidates:
        return -3
    except (OverflowError, ValueError):
        return -1
