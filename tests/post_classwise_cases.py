"""Seeded and hand-built cases of the per-class NMS tests (tests/test_post_classwise_cpu.py checks
on the CPU that they stay inside their conditions; tests/test_gpu_post_classwise.py runs them on
the GPU).  Oracle results are computed once per process and shared: callers must not modify them.

PARITY  name -> (grids, classes, images, seed, score threshold), data from post_multi_oracle.batch
        on post_multi_cases.yolov3_multi, as post_multi_cases.PARITY.  The seeds were chosen on the
        CPU so that the per-class rule raises on at least one and at most a quarter of the images
        AND the two rules disagree about which image raises:
          small   grids 2, 4, 8 x 3 anchors x 3 classes, 8 images, seed 37, score > 0.3
                  per class [120, -2, 75, 69, 137, 92, 73, 82], any class [100, 55, 43, 38, -2, 49,
                  52, 53]: image 1 raises only per class, image 4 only class-agnostic
          yolov3  grids 13, 26, 52 x 3 x 80, 4 images, seed 0, score > 0.99
                  per class [232, 208, -2, 223], any class [-2, 39, 54, 57]; most of the 80 class
                  segments hold 0..5 candidates
SKEW    grids 8, 16, 32 x 3 anchors x 5 classes = 4032 boxes, saturated (every box a candidate),
        the anchors of post_multi_cases.cap_multi (2 px wide, 8192 * 4^(3 s + a) px tall: every
        pair overlaps vertically, no zero denominator).  On the stride-8 scale every box of the
        cells with (row + col) % 4 != 0 gets +30 on its class-0 logit, so class 0 owns 2638 boxes
        and the others 339 / 365 / 337 / 353: one segment of 42 blocks beside four of 6.
BOUNDS  one scale of 6 x 129 cells x 1 anchor x 6 classes, hand-built: row r holds the candidates
        of class r in its first BOUNDS_SIZES[r] cells, 1, 63, 64, 0, 65 and 129 of them (the empty
        class sits between two non-empty ones); the other cells have objectness -20.  Every box
        is 9 x 17 px.  Box j of a class sits in the middle of cell j, except that every third box
        (j % 3 == 2) sits on its cell's left edge and box j - 1 on its cell's right edge: the same
        pixels, so whichever of the two scores higher drops the other.  All other boxes of a row
        are at least 48 px apart and never overlap.  The per-class rule only evaluates pairs of
        one row, which overlap vertically, so no evaluated denominator is zero.  The scores are a
        seeded permutation of 322 distinct values, so the classes interleave in the output.
        THRESHOLD_SIZES is the same construction with 256, 257, 255 and 320 candidates per class:
        one wave takes a segment of up to 256 candidates, the whole workgroup a longer one.
"""
import functools

import numpy as np

import post_classwise_oracle as CO
import post_head_oracle as O
import post_multi_cases as K
import post_multi_oracle as MO

# name: grids (stride 32, 16, 8), classes, images, seed, score threshold
PARITY = {
    "small": ((2, 4, 8), 3, 8, 37, 0.3),
    "yolov3": ((13, 26, 52), 80, 4, 0, 0.99),
}
# what the two oracles give (detections, or the code): asserted in tests/test_post_classwise_cpu.py
PER_CLASS = {"small": [120, -2, 75, 69, 137, 92, 73, 82], "yolov3": [232, 208, -2, 223]}
ANY_CLASS = {"small": [100, 55, 43, 38, -2, 49, 52, 53], "yolov3": [-2, 39, 54, 57]}

SKEW_GRIDS, SKEW_CLASSES, SKEW_SEED = (8, 16, 32), 5, 11
SKEW_SIZES = [2638, 339, 365, 337, 353]
SKEW_KEPT, SKEW_KEPT_ANY = 1678, 893

BOUNDS_SIZES = (1, 63, 64, 0, 65, 129)  # candidates of class 0..5
# around the segment length above which the kernel hands a class to the whole workgroup
# (csrc/postprocess_multi.hip: PC_BIG = 256)
THRESHOLD_SIZES = (256, 257, 255, 320)


def counts_of(refs):
    return [r if isinstance(r, int) else len(r) for r in refs]


@functools.lru_cache(maxsize=None)
def parity(name):
    """(preds per scale [n, g, g, n_out], per image the per-class oracle's rows or code)."""
    grids, classes, n, seed, thr = PARITY[name]
    multi = K.yolov3_multi(grids, classes, score_thr=thr)
    preds = MO.batch(seed, multi, n)
    for p in preds:
        p.setflags(write=False)
    return preds, tuple(CO.detect_or_code([p[i] for p in preds], multi) for i in range(n))


@functools.lru_cache(maxsize=None)
def parity_any(name):
    """The class-agnostic oracle on the same batch."""
    grids, classes, n, _, thr = PARITY[name]
    multi = K.yolov3_multi(grids, classes, score_thr=thr)
    preds, _ = parity(name)
    return tuple(MO.detect_or_code([p[i] for p in preds], multi) for i in range(n))


def skew_multi(grids=SKEW_GRIDS, classes=SKEW_CLASSES):
    scales = []
    for s, (g, (st, _)) in enumerate(zip(grids, K.YOLOV3_ANCHORS)):
        anchors = tuple(v for a in range(3) for v in (2.0 / st, 8192.0 * 4.0 ** (3 * s + a) / st))
        scales.append(O.Head(g, g, 3, classes, anchors, float(st), 0.3, 0.3))
    return MO.Multi(tuple(scales), "logistic")


def skew_preds(grids=SKEW_GRIDS, classes=SKEW_CLASSES, seed=SKEW_SEED):
    """Per scale [1, g, g, 3 * (5 + classes)]."""
    multi = skew_multi(grids, classes)
    rng = np.random.default_rng(seed)
    preds = [O.synthetic_predictions(rng, h, tw_scale=0.5, saturate=True) for h in multi.scales]
    g = grids[2]
    v = preds[2].reshape(g, g, 3, 5 + classes)
    row, col = np.indices((g, g))
    v[(row + col) % 4 != 0, :, 5] += np.float32(30)
    return [p[None] for p in preds]


@functools.lru_cache(maxsize=None)
def skew():
    """(preds, the per-class oracle's rows, the candidates' classes in sorted order)."""
    multi = skew_multi()
    preds = skew_preds()
    for p in preds:
        p.setflags(write=False)
    stats = {}
    rows = CO.detect([p[0] for p in preds], multi, stats)
    return preds, tuple(rows), tuple(stats["classes"])


def bounds_multi(sizes=BOUNDS_SIZES):
    n = len(sizes)
    return MO.Multi((O.Head(n, max(sizes), 1, n, (9.0 / 32, 17.0 / 32), 32.0, 0.3, 0.3),), "logistic")


def bounds_preds(sizes=BOUNDS_SIZES):
    """[1, classes, max(sizes), 5 + classes]: see BOUNDS above."""
    n, w, total = len(sizes), max(sizes), sum(sizes)
    p = np.zeros((n, w, 1, 5 + n), np.float32)
    p[..., 4] = -20.0                                  # not a candidate
    rank = np.random.default_rng(5).permutation(total)
    k = 0
    for c, size in enumerate(sizes):
        for j in range(size):
            p[c, j, 0, 4] = 5.0 - 3.0 * rank[k] / total  # distinct fp32 scores in (0.88, 0.994)
            p[c, j, 0, 5:] = -20.0
            p[c, j, 0, 5 + c] = 20.0                   # p(class c) rounds to 1.0f
            if j % 3 == 2:
                p[c, j, 0, 0] = -40.0                  # sigmoid 0: the cell's left edge
                p[c, j - 1, 0, 0] = 40.0               # sigmoid 1: the previous cell's right edge
            k += 1
    return p.reshape(1, n, w, 5 + n)
