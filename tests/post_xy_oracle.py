"""TEST INFRASTRUCTURE ONLY: the multi-scale postprocessing with Darknet's scale_x_y
(include/dnn_hip_post.h: the dnn_yolo_postprocess_*_xy entries) restated in numpy on top of the
existing oracles.

Darknet (forward_yolo_layer, scal_add_cpu) replaces the logistic of tx and ty by

    sig * s + b,    b = -0.5f * (s - 1.0f)

`corners` below restates tests/post_head_oracle.decode_one's geometry with that one step added,
every operation rounded to fp32 (b once per scale, then one multiply and one add).  Everything
else is imported, not copied: scores, classes and labels of every box are post_multi_oracle.decode's
and post_multilabel_oracle.decode's, whose own corners are replaced; the IoU is post_numpy.iou.  The
three NMS loops are the ones of post_multi_oracle.detect, post_classwise_oracle.detect and
post_multilabel_oracle.detect, which take no box list, restated over one; with every s = 1 this
module must equal those three (tests/test_post_xy_cpu.py).

xy: one float per scale.  mode: "any" (class-agnostic NMS, arg-max label), "per_class" (per-class
NMS, arg-max label) or "multi" (per-class NMS, multi-label)."""
import numpy as np

import post_head_oracle as O
import post_multi_oracle as MO
import post_multilabel_oracle as LO
import post_numpy as PN

_F = np.float32

MODES = ("any", "per_class", "multi")


def xy_bias(s):
    return _F(_F(-0.5) * _F(_F(s) - _F(1.0)))


def corners(p, row, col, b, head, s):
    """[left, top, right, bottom] of box (row, col, anchor) with scale_x_y = s."""
    tx, ty, tw, th = (p[row, col, b, k] for k in range(4))
    cell, s32, bias = _F(head.cell), _F(s), xy_bias(s)
    sx = _F(_F(PN._sigmoid(tx) * s32) + bias)
    sy = _F(_F(PN._sigmoid(ty) * s32) + bias)
    cx = _F(_F(_F(col) + sx) * cell)
    cy = _F(_F(_F(row) + sy) * cell)
    rw = _F(_F(np.exp(tw) * _F(head.anchors[2 * b])) * cell)
    rh = _F(_F(np.exp(th) * _F(head.anchors[2 * b + 1])) * cell)
    left = int(_F(cx - _F(rw / _F(2.0))))
    right = int(_F(cx + _F(rw / _F(2.0))))
    top = int(_F(cy - _F(rh / _F(2.0))))
    bottom = int(_F(cy + _F(rh / _F(2.0))))
    return [left, top, right, bottom]


def all_corners(preds, multi, xy):
    """The corners of every box of one image in global order (scale 0 first, row, col, anchor)."""
    assert len(preds) == len(multi.scales) == len(xy)
    out = []
    for pred, head, s in zip(preds, multi.scales, xy):
        p = O.as_boxes(pred, head)
        out += [corners(p, row, col, b, head, s) for row in range(head.grid_h) for col in range(head.grid_w)
                for b in range(head.n_anchors)]
    return out


def _rows(kept):
    return [(k[2], k[0][0], k[0][1], k[0][2], k[0][3], float(k[1])) for k in kept]


def detect(preds, multi, xy, mode):
    """Post-NMS detections [(class, left, top, right, bottom, score)] in output order."""
    assert mode in MODES
    head = multi.scales[0]
    thr = _F(head.score_thr)
    if mode == "multi":
        boxes = LO.decode(preds, multi)  # (its corners raise where a width or height does not convert)
        cs = all_corners(preds, multi, xy)
        cand = [[cs[g], sc, c, g] for g, (_, _, labels) in enumerate(boxes) for c, sc in labels]
        if len(cand) > LO.MAX_CANDIDATES:
            raise LO.TooManyCandidates(len(cand))
    else:
        boxes = MO.decode(preds, multi)
        cs = all_corners(preds, multi, xy)
        cand = [[cs[g], d[1], d[2], g] for g, d in enumerate(boxes) if d[1] > thr]
    cand.sort(key=lambda t: t[1], reverse=True)
    kept = []
    for c in cand:
        against = kept if mode == "any" else [k for k in kept if k[2] == c[2]]
        hits = [PN.iou(c[0], k[0]) > head.iou_thr for k in against]  # all of them: a zero denominator raises
        if not any(hits):
            kept.append(c)
    return _rows(kept)


def detect_or_code(preds, multi, xy, mode):
    """detect(), or the device's per-image code where the reference's arithmetic raises."""
    try:
        return detect(preds, multi, xy, mode)
    except ZeroDivisionError:
        return -2
    except LO.TooManyCandidates:
        return -3
    except (OverflowError, ValueError):
        return -1
