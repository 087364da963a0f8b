"""TEST INFRASTRUCTURE ONLY — the multi-scale postprocessing with multi-label detections
(include/dnn_hip_post.h: DNN_YOLO_LABELS_MULTI) restated in numpy from the pieces of
tests/post_multi_oracle.py, tests/post_head_oracle.py and oracle/post_numpy.py, imported, not copied:

  boxes   corners and objectness `conf` of every box are post_head_oracle.decode_one on the
          one-class objectness head (post_multi_oracle._objectness_head), global box order as there;
  labels  every class c has p[c] = post_numpy._sigmoid(logit[c]) (logistic) or decode_one's softmax
          quotient exp(logit[c] - max) / sum with post_numpy._pairwise_sum_f32 (softmax), and the
          score s[c] = fp32(conf * p[c]); (box, c) is a candidate iff s[c] > score_thr;
  order   candidates are appended box-major, class ascending, and stable-sorted on the score,
          descending: ties keep the lower global box index, then the lower class;
  NMS     post_classwise_oracle.detect's loop: the kept list filtered to the candidate's class
          before the IoUs (post_numpy.iou) are evaluated, all of them.

More than MAX_CANDIDATES candidates give the code -3, after the corners of every box were
converted (-1 comes first) and before the NMS (-2 comes last).

Logistic speed: only the classes whose float64 score conf64 * sigmoid64(logit) exceeds
score_thr (1 - 1e-5) are evaluated with the scalar fp32 formula; the fp32 formula is within a few
ulp (2^-24 each, far below 1e-5) of the float64 value, so no candidate is missed.
"""
import numpy as np

import post_head_oracle as O
import post_multi_oracle as MO
import post_numpy as PN

_F = np.float32

MAX_CANDIDATES = 16384  # DNN_YOLO_MULTI_MAX_CANDIDATES


class TooManyCandidates(Exception):
    pass


def label_scale(pred, head, class_mode):
    """Every box of one scale in (row, col, anchor) order: (corners, conf, [(class, score)] for the
    classes whose score is above score_thr, ascending)."""
    p = O.as_boxes(pred, head)
    h1 = MO._objectness_head(head)
    p1 = np.ascontiguousarray(p[..., :6])
    thr = _F(head.score_thr)
    assert class_mode in ("softmax", "logistic")
    if class_mode == "logistic":
        with np.errstate(over="ignore"):
            s64 = 1.0 / (1.0 + np.exp(-p[..., 4:].astype(np.float64)))
        maybe = s64[..., :1] * s64[..., 1:] > float(thr) * (1.0 - 1e-5)
    out = []
    for row in range(head.grid_h):
        for col in range(head.grid_w):
            for b in range(head.n_anchors):
                corners, conf, _ = O.decode_one(p1, row, col, b, h1)
                logits = p[row, col, b, 5:]
                labels = []
                if class_mode == "logistic":
                    for c in np.flatnonzero(maybe[row, col, b]):
                        sc = _F(conf * PN._sigmoid(logits[c]))
                        if sc > thr:
                            labels.append((int(c), sc))
                else:
                    e = np.exp(logits - np.max(logits))
                    s = PN._pairwise_sum_f32(e)
                    for c in range(head.n_classes):
                        sc = _F(conf * _F(e[c] / s))
                        if sc > thr:
                            labels.append((c, sc))
                out.append((corners, conf, labels))
    return out


def decode(preds, multi):
    """All boxes of one image (preds: one tensor per scale) in global order."""
    assert len(preds) == len(multi.scales)
    out = []
    for pred, head in zip(preds, multi.scales):
        out += label_scale(pred, head, multi.class_mode)
    return out


def candidates(preds, multi):
    """[[corners, score, class, global box index]] box-major, class ascending, unsorted."""
    return [[corners, sc, c, g] for g, (corners, _, labels) in enumerate(decode(preds, multi)) for c, sc in labels]


def detect(preds, multi, stats=None):
    """Post-NMS detections [(class, left, top, right, bottom, score)] in output order."""
    head = multi.scales[0]
    cand = candidates(preds, multi)
    if stats is not None:
        stats["candidates"] = len(cand)
        stats["classes"] = [c[2] for c in cand]
        stats["boxes"] = [c[3] for c in cand]
    if len(cand) > MAX_CANDIDATES:
        raise TooManyCandidates(len(cand))
    cand.sort(key=lambda t: t[1], reverse=True)
    kept, kept_of = [], {}  # (kept_of[class]: the kept list filtered to a class, kept as it grows)
    for c in cand:
        same = kept_of.setdefault(c[2], [])
        hits = [PN.iou(c[0], k[0]) > head.iou_thr for k in same]  # all of them: a zero denominator raises
        if not any(hits):
            kept.append(c)
            same.append(c)
    return [(k[2], k[0][0], k[0][1], k[0][2], k[0][3], float(k[1])) for k in kept]


def detect_or_code(preds, multi):
    """detect(), or the device's per-image code where the reference's arithmetic raises."""
    try:
        return detect(preds, multi)
    except ZeroDivisionError:
        return -2
    except TooManyCandidates:
        return -3
    except (OverflowError, ValueError):
        return -1
