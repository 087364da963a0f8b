"""TEST INFRASTRUCTURE ONLY — the multi-scale postprocessing (include/dnn_hip_post.h:
dnn_yolo_multi) restated in numpy from tests/post_head_oracle.py's pieces, which are imported,
not copied: a scale's geometry and objectness are `post_head_oracle.decode_one` with that scale's
head, the softmax class score is decode_one's, the NMS is `post_head_oracle.detect`'s loop over
`post_numpy.iou`.

A multi-head is anything with `scales` (a sequence of heads as post_head_oracle takes them, all
with the same n_classes, score_thr and iou_thr) and `class_mode` ("softmax" or "logistic").

Box order: scale 0's boxes first, each scale in (row, col, anchor) order.  The sort is Python's
stable sort on the score, descending: ties keep the lower global index first.

Logistic class scores: p[c] = post_numpy._sigmoid(logit[c]) in fp32, the class is the first index
of the largest computed p, the score conf * p[class] in fp32.  To keep an 80-class head fast only
the classes that can hold the largest computed value are evaluated with the scalar fp32 formula:
with s[c] the float64 sigmoid, a class with s[c] < max(s) (1 - 1e-6) cannot win, because the
fp32 formula is within a few ulp (2^-24 each, far below 1e-6) of the true value on both sides.
"""
import collections

import numpy as np

import post_head_oracle as O
import post_numpy as PN

_F = np.float32

Multi = collections.namedtuple("Multi", "scales class_mode")


def scale_boxes(head):
    return head.grid_h * head.grid_w * head.n_anchors


def _objectness_head(head):
    """The head with one class: decode_one's softmax of a single logit is exp(0) / exp(0) = 1, so
    its score is the objectness itself."""
    return O.Head(head.grid_h, head.grid_w, head.n_anchors, 1, head.anchors, head.cell, head.score_thr, head.iou_thr)


def decode_scale(pred, head, class_mode):
    """Every box of one scale in (row, col, anchor) order: [[l, t, r, b], score, class]."""
    p = O.as_boxes(pred, head)
    if class_mode == "softmax":
        return [O.decode_one(p, row, col, b, head) for row in range(head.grid_h) for col in range(head.grid_w)
                for b in range(head.n_anchors)]
    assert class_mode == "logistic"
    h1 = _objectness_head(head)
    p1 = np.ascontiguousarray(p[..., :6])
    with np.errstate(over="ignore"):
        s64 = 1.0 / (1.0 + np.exp(-p[..., 5:].astype(np.float64)))
    out = []
    for row in range(head.grid_h):
        for col in range(head.grid_w):
            for b in range(head.n_anchors):
                corners, conf, _ = O.decode_one(p1, row, col, b, h1)
                s = s64[row, col, b]
                best, bp = -1, None
                for c in np.flatnonzero(s >= s.max() * (1.0 - 1e-6)):  # ascending: the first index wins ties
                    pc = PN._sigmoid(p[row, col, b, 5 + c])
                    if bp is None or pc > bp:
                        best, bp = int(c), pc
                out.append([corners, _F(conf * bp), best])
    return out


def decode(preds, multi):
    """All boxes of one image (preds: one tensor per scale) in global order."""
    assert len(preds) == len(multi.scales)
    out = []
    for pred, head in zip(preds, multi.scales):
        out += decode_scale(pred, head, multi.class_mode)
    return out


def detect(preds, multi, stats=None):
    """Post-NMS detections [(class, left, top, right, bottom, score)] in output order: the loop of
    post_head_oracle.detect over the candidates of all scales."""
    head = multi.scales[0]
    thr = _F(head.score_thr)
    cand = [d for d in decode(preds, multi) if d[1] > thr]
    cand.sort(key=lambda t: t[1], reverse=True)
    kept = []
    for c in cand:
        hits = [PN.iou(c[0], k[0]) > head.iou_thr for k in kept]  # all of them: a zero denominator raises
        if not any(hits):
            kept.append(c)
    if stats is not None:
        stats["candidates"] = len(cand)
    return [(k[2], k[0][0], k[0][1], k[0][2], k[0][3], float(k[1])) for k in kept]


def detect_or_code(preds, multi):
    """detect(), or the device's per-image code where the reference raises (as post_head_oracle)."""
    try:
        return detect(preds, multi)
    except ZeroDivisionError:
        return -2
    except (OverflowError, ValueError):
        return -1


def batch(seed, multi, n, tw_every=4, **kw):
    """n seeded images as one array per scale: post_head_oracle.synthetic_predictions per scale from
    one generator, every tw_every-th image with 6x larger box-size logits."""
    rng = np.random.default_rng(seed)
    per_scale = [[] for _ in multi.scales]
    for i in range(n):
        for s, head in enumerate(multi.scales):
            per_scale[s].append(O.synthetic_predictions(rng, head, tw_scale=(1.0 if i % tw_every else 6.0), **kw))
    return [np.stack(v) for v in per_scale]
