"""Seeded cases of the multi-scale decode tests (tests/test_post_multi_cpu.py checks on the CPU
that they stay inside their conditions; tests/test_gpu_post_multi.py runs them on the GPU).
Oracle results are computed once per process and shared: callers must not modify them.

PARITY  name -> (grids, classes, images, seed, score threshold): three scales with YOLOv3's anchor
        table and strides, logistic class scores, batches from post_multi_oracle.batch (every 4th
        image with 6x box-size logits).  The seeds were chosen on the CPU so that at least one and
        at most a quarter of a batch's images make the reference raise:
          small   grids 2, 4, 8 x 3 anchors x 3 classes (252 boxes), 8 images, score > 0.3
          yolov3  grids 13, 26, 52 x 3 x 80 (10,647 boxes, the 416 x 416 model), 4 images,
                  score > 0.99
        The reference's IoU has no clamp, so two boxes disjoint in both axes whose gap product
        equals the sum of their areas give a zero denominator; with the few-pixel boxes of the
        stride-8 anchors and the 6,400 candidates that score > 0.3 leaves among 10,647 random
        boxes, every one of 16 seeded images raised.  At score > 0.99 an image has about 220
        candidates and 50 detections and most seeds leave the three ordinary images clean.
CAP     16 x 16, 32 x 32 and 64 x 64 cells x 3 anchors x 1 class = 16,128 boxes (a 512 x 512
        input), saturated: every box is a candidate.  Every box is taller than twice the image
        (anchor heights of 8192 pixels and more, box-size logits scaled by 0.5), so every pair of
        boxes overlaps vertically and no IoU denominator is zero; the nine anchor heights are a
        factor 4 apart, so boxes of different anchors over the same columns have an IoU below
        0.3 and thousands of boxes survive.  The oracle needs minutes for it, so its rows are
        recorded in tests/golden/post_multi_cap_golden.json (`python tests/post_multi_cases.py`
        rewrites the file from the oracle).
"""
import functools
import json
import os

import numpy as np

import post_head_oracle as O
import post_multi_oracle as MO

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# the public YOLOv3 anchor table: stride, (w, h) pairs in pixels
YOLOV3_ANCHORS = ((32, (116, 90, 156, 198, 373, 326)), (16, (30, 61, 62, 45, 59, 119)), (8, (10, 13, 16, 30, 33, 23)))

# name: grids (stride 32, 16, 8), classes, images, seed, score threshold
PARITY = {
    "small": ((2, 4, 8), 3, 8, 27, 0.3),
    "yolov3": ((13, 26, 52), 80, 4, 3, 0.99),
}

CAP_GRIDS = (16, 32, 64)
CAP_SEED, CAP_TW = 302, 0.5
CAP_GOLDEN = os.path.join(GOLDEN, "post_multi_cap_golden.json")


def yolov3_multi(grids, classes, score_thr=0.3, iou_thr=0.3, class_mode="logistic"):
    """The oracle's description: YOLOv3's strides and anchors (pixels / stride, in cells)."""
    scales = [O.Head(g, g, 3, classes, tuple(a / st for a in px), float(st), score_thr, iou_thr)
              for g, (st, px) in zip(grids, YOLOV3_ANCHORS)]
    return MO.Multi(tuple(scales), class_mode)


def cap_multi():
    """Anchor k of 9 (scale-major): two pixels wide, 8192 * 4^k pixels tall."""
    scales = []
    for s, (g, (st, _)) in enumerate(zip(CAP_GRIDS, YOLOV3_ANCHORS)):
        anchors = tuple(v for a in range(3) for v in (2.0 / st, 8192.0 * 4.0 ** (3 * s + a) / st))
        scales.append(O.Head(g, g, 3, 1, anchors, float(st), 0.3, 0.3))
    return MO.Multi(tuple(scales), "logistic")


def device_multi(multi):
    import yolo_post
    return yolo_post.MultiHead(multi.scales, multi.class_mode)


@functools.lru_cache(maxsize=None)
def parity(name):
    """(preds: per scale [n, g, g, n_out], per image the oracle's rows or its negative code)."""
    grids, classes, n, seed, thr = PARITY[name]
    multi = yolov3_multi(grids, classes, score_thr=thr)
    preds = MO.batch(seed, multi, n)
    for p in preds:
        p.setflags(write=False)
    return preds, tuple(MO.detect_or_code([p[i] for p in preds], multi) for i in range(n))


def cap(compute=False):
    """(preds: per scale [1, g, g, 18], rows): the recorded oracle rows, or with compute=True the
    oracle's."""
    multi = cap_multi()
    rng = np.random.default_rng(CAP_SEED)
    preds = [O.synthetic_predictions(rng, h, tw_scale=CAP_TW, saturate=True)[None] for h in multi.scales]
    if compute:
        stats = {}
        rows = MO.detect([p[0] for p in preds], multi, stats)
        assert stats["candidates"] == sum(MO.scale_boxes(h) for h in multi.scales)
        return preds, rows
    with open(CAP_GOLDEN) as f:
        return preds, [tuple(r) for r in json.load(f)["rows"]]


if __name__ == "__main__":
    _preds, _rows = cap(compute=True)
    with open(CAP_GOLDEN, "w") as _f:
        json.dump({"source": "tests/post_multi_oracle.detect on tests/post_multi_cases.cap_multi under numpy "
                             + np.__version__, "rows": _rows}, _f)
    print(len(_rows), "rows ->", CAP_GOLDEN)
