"""TEST INFRASTRUCTURE ONLY — oracle/post_numpy.py's restatement of the reference's
postprocessing (cs492-projects/proj3/yolov2tiny.py:94-234) with the quantities the reference
names as constants turned into parameters of a head: 13 -> grid_h / grid_w, 5 -> n_anchors,
20 -> n_classes, 32.0 -> cell, 0.3 -> score_thr and iou_thr.  Every numeric rule is
post_numpy's (fp32 weak scalars, numpy's pairwise softmax sum, truncated corners for every
box, stable sort, greedy NMS without early exit); its `_pairwise_sum_f32`, `_sigmoid` and `iou`
are reused as they are.

A head is anything with grid_h, grid_w, n_anchors, n_classes, anchors, cell, score_thr and
iou_thr (yolo_post.YoloHead, or `Head` below where no library should be loaded).

Pinned by tests/test_post_head_cpu.py: equal to post_numpy.detect on every 13 x 13 fixture,
and to the reference's own function on small grids embedded in a 13 x 13 tensor
(tests/golden/make_golden_post_ms.py).
"""
import collections

import numpy as np

import post_numpy as PN

_F = np.float32

Head = collections.namedtuple("Head", "grid_h grid_w n_anchors n_classes anchors cell score_thr iou_thr")


def voc_head(grid_h, grid_w, score_thr=0.3, iou_thr=0.3):
    return Head(grid_h, grid_w, 5, 20, PN.ANCHORS, 32.0, score_thr, iou_thr)


def as_boxes(pred, head):
    return np.asarray(pred, dtype=np.float32).reshape(head.grid_h, head.grid_w, head.n_anchors, 5 + head.n_classes)


def decode_one(p, row, col, b, head):
    """Box (row, col, anchor): [[left, top, right, bottom], score, class] (yolov2tiny.py:127-152)."""
    tx, ty, tw, th, tc = (p[row, col, b, k] for k in range(5))
    cell = _F(head.cell)
    cx = _F(_F(_F(col) + PN._sigmoid(tx)) * cell)
    cy = _F(_F(_F(row) + PN._sigmoid(ty)) * cell)
    rw = _F(_F(np.exp(tw) * _F(head.anchors[2 * b])) * cell)
    rh = _F(_F(np.exp(th) * _F(head.anchors[2 * b + 1])) * cell)
    conf = PN._sigmoid(tc)
    logits = p[row, col, b, 5:]
    e = np.exp(logits - np.max(logits))
    s = PN._pairwise_sum_f32(e)
    probs = [_F(v / s) for v in e]
    best = max(range(head.n_classes), key=lambda k: (probs[k], -k))  # first index of the max quotient
    left = int(_F(cx - _F(rw / _F(2.0))))
    right = int(_F(cx + _F(rw / _F(2.0))))
    top = int(_F(cy - _F(rh / _F(2.0))))
    bottom = int(_F(cy + _F(rh / _F(2.0))))
    return [[left, top, right, bottom], _F(conf * probs[best]), best]


def decode(pred, head):
    """Every box in (row, col, anchor) order; those above score_thr, unsorted.  int() of a
    non-finite corner raises for any box, candidate or not, as in the reference."""
    p = as_boxes(pred, head)
    thr = _F(head.score_thr)
    out = []
    for row in range(head.grid_h):
        for col in range(head.grid_w):
            for b in range(head.n_anchors):
                d = decode_one(p, row, col, b, head)
                if d[1] > thr:
                    out.append(d)
    return out


def detect(pred, head, stats=None):
    """Post-NMS detections [(class, left, top, right, bottom, score)] in output order."""
    cand = decode(pred, head)
    cand.sort(key=lambda t: t[1], reverse=True)
    kept = []
    for c in cand:
        hits = [PN.iou(c[0], k[0]) > head.iou_thr for k in kept]  # all of them: a zero denominator raises
        if not any(hits):
            kept.append(c)
    if stats is not None:
        stats["candidates"] = len(cand)
    return [(k[2], k[0][0], k[0][1], k[0][2], k[0][3], float(k[1])) for k in kept]


def detect_or_code(pred, head):
    """detect(), or the device's per-image code where the reference raises: -2 for a zero IoU
    denominator, -1 for a corner int() cannot convert."""
    try:
        return detect(pred, head)
    except ZeroDivisionError:
        return -2
    except (OverflowError, ValueError):
        return -1


def embed_in_13x13(pred, head):
    """A VOC-shaped small grid (<= 13 x 13, 5 anchors, 20 classes) in the top-left of a
    [13,13,125] tensor whose other cells have objectness -20 (score < 3e-9: never candidates)
    and zeros elsewhere (finite corners): the reference's unmodified postprocessing then
    returns the small grid's detections, in the small grid's order."""
    assert head.grid_h <= 13 and head.grid_w <= 13 and head.n_anchors == 5 and head.n_classes == 20
    big = np.zeros((13, 13, 5, 25), np.float32)
    big[..., 4] = -20.0
    big[:head.grid_h, :head.grid_w] = as_boxes(pred, head)
    return big.reshape(13, 13, 125)


def synthetic_predictions(rng, head, tw_scale=1.0, saturate=False):
    """One image of head's shape, modelled on post_numpy.synthetic_predictions: normal logits,
    objectness of scale 3, one class per box boosted by U(0, 8).  saturate: objectness 8 and a
    boost of 12 on every box, so that every box is a candidate."""
    gh, gw, a, c = head.grid_h, head.grid_w, head.n_anchors, head.n_classes
    p = rng.standard_normal((gh, gw, a, 5 + c)).astype(np.float32)
    p[..., 2:4] *= np.float32(tw_scale)
    p[..., 4] = (rng.standard_normal((gh, gw, a)) * 3.0).astype(np.float32)
    hot = rng.integers(0, c, size=(gh, gw, a))
    boost = rng.uniform(0.0, 8.0, size=(gh, gw, a)).astype(np.float32)
    if saturate:
        p[..., 4] = np.float32(8.0)
        boost[...] = np.float32(12.0)
    np.put_along_axis(p[..., 5:], hot[..., None], (np.take_along_axis(p[..., 5:], hot[..., None], -1)
                                                     + boost[..., None]).astype(np.float32), -1)
    return p.reshape(gh, gw, a * (5 + c))


def batch(seed, head, n, tw_every=4, **kw):
    """n seeded images; every tw_every-th with 6x larger box-size logits (big boxes: 128-bit
    IoU products and zero denominators, as in the 13 x 13 random-batch test)."""
    rng = np.random.default_rng(seed)
    return np.stack([synthetic_predictions(rng, head, tw_scale=(1.0 if i % tw_every else 6.0), **kw)
                     for i in range(n)])
