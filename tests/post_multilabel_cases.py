"""Seeded and hand-built cases of the multi-label tests (tests/test_post_multilabel_cpu.py checks on
the CPU that they stay inside their conditions; tests/test_gpu_post_multilabel.py runs them on the
GPU).  Oracle results (tests/post_multilabel_oracle.py) are computed once per process and shared:
callers must not modify them.

SEEDED  name -> (grids, classes, images, seed, score threshold, class mode), data from
        post_multi_oracle.batch on post_multi_cases.yolov3_multi:
          small          grids 2, 4, 8 x 3 anchors x 3 classes (252 boxes), 8 images, seed 8, logistic:
                         310-328 candidates per clean image, about 110 boxes with >= 2 labels; image
                         4 raises under multi-label only
          small_softmax  the same grids and classes, softmax, seed 1
        `yolov3` is post_classwise_cases.parity("yolov3") (80 classes, score > 0.99): no box has a
        second label, so the rows are the per-class oracle's.
DENSE   post_classwise_cases.skew_multi's tall anchors (every pair overlaps vertically: no zero
        denominator) on grids 4, 8, 16 = 1008 boxes, saturated predictions, no class boost:
          dense    12 classes, score > 0.6: 4788 candidates, up to 9 labels per box, 369-414 per
                   class (every segment goes to the whole workgroup), 2469 rows
          dense80  80 classes, score > 0.9: 2062 candidates, 14-40 per class (one wave each), 1925 rows
          over     grids 8, 16, 32 x 5 classes = 4032 boxes, score > 0.3: 16,910 candidates: -3
CAP     one scale of 16 x 16 cells x 1 anchor x 128 classes, every box 4096 px square around its
        cell's centre (IoU of any two > 0.63): box j has objectness 5 - 3 rank[j] / 256 and class
        logit +20 where (j + c) is even, else -20, so exactly 128 * 128 = 16,384 candidates, and
        each class keeps one box: 128 rows with two distinct scores among them (ties: index, then
        class).  `cap+1` has box 0's class-1 logit at +20 too: 16,385 candidates, -3.
"""
import functools

import numpy as np

import post_classwise_cases as CK
import post_head_oracle as O
import post_multi_cases as K
import post_multi_oracle as MO
import post_multilabel_oracle as LO

# name: grids, classes, images, seed, score threshold, class mode
SEEDED = {
    "small": ((2, 4, 8), 3, 8, 8, 0.3, "logistic"),
    "small_softmax": ((2, 4, 8), 3, 8, 1, 0.3, "softmax"),
}
# what the oracles give (rows, or the code): asserted in tests/test_post_multilabel_cpu.py
COUNTS = {
    "small": [252, 131, 140, 114, -2, 115, 123, 114],
    "small_softmax": [-2, 71, 83, 80, 120, 80, 82, 81],
    "yolov3": [232, 208, -2, 223],
}
SMALL_SINGLE_LABEL = [129, 82, 85, 69, 144, 70, 75, 77]  # the per-class oracle on `small`

# name: grids, classes, score threshold, boxes, candidates, rows (or the code)
DENSE = {
    "dense": ((4, 8, 16), 12, 0.6, 1008, 4788, 2469),
    "dense80": ((4, 8, 16), 80, 0.9, 1008, 2062, 1925),
    "over": ((8, 16, 32), 5, 0.3, 4032, 16910, -3),
}
DENSE_SEED = 11

CAP_CLASSES, CAP_GRID = 128, 16


def counts_of(refs):
    return [r if isinstance(r, int) else len(r) for r in refs]


def seeded_multi(name):
    grids, classes, _, _, thr, mode = SEEDED[name]
    return K.yolov3_multi(grids, classes, score_thr=thr, class_mode=mode)


@functools.lru_cache(maxsize=None)
def seeded(name):
    """(preds per scale [n, g, g, n_out], per image the multi-label oracle's rows or code)."""
    n, seed = SEEDED[name][2], SEEDED[name][3]
    multi = seeded_multi(name)
    preds = MO.batch(seed, multi, n)
    for p in preds:
        p.setflags(write=False)
    return preds, tuple(LO.detect_or_code([p[i] for p in preds], multi) for i in range(n))


def yolov3_multi():
    grids, classes, _, _, thr = CK.PARITY["yolov3"]
    return K.yolov3_multi(grids, classes, score_thr=thr)


@functools.lru_cache(maxsize=None)
def yolov3():
    """(post_classwise_cases.parity("yolov3")'s preds, the multi-label oracle's rows or code)."""
    preds, _ = CK.parity("yolov3")
    multi = yolov3_multi()
    return preds, tuple(LO.detect_or_code([p[i] for p in preds], multi) for i in range(preds[0].shape[0]))


def dense_multi(name):
    grids, classes, thr = DENSE[name][:3]
    m = CK.skew_multi(grids, classes)
    return MO.Multi(tuple(h._replace(score_thr=thr) for h in m.scales), m.class_mode)


def dense_preds(name):
    """Per scale [1, g, g, 3 * (5 + classes)]."""
    rng = np.random.default_rng(DENSE_SEED)
    return [O.synthetic_predictions(rng, h, tw_scale=0.5, saturate=True)[None] for h in dense_multi(name).scales]


@functools.lru_cache(maxsize=None)
def dense(name):
    """(preds, the oracle's rows or code, its stats: candidates, their classes and boxes)."""
    multi, preds = dense_multi(name), dense_preds(name)
    for p in preds:
        p.setflags(write=False)
    stats = {}
    try:
        rows = tuple(LO.detect([p[0] for p in preds], multi, stats))
    except LO.TooManyCandidates:
        rows = -3
    return preds, rows, stats


def cap_multi():
    return MO.Multi((O.Head(CAP_GRID, CAP_GRID, 1, CAP_CLASSES, (128.0, 128.0), 32.0, 0.3, 0.3),), "logistic")


def cap_preds(extra=False):
    """[1, 16, 16, 133]; extra: box 0's class-1 logit is +20 as well (one candidate too many)."""
    nb = CAP_GRID * CAP_GRID
    p = np.zeros((nb, 5 + CAP_CLASSES), np.float32)
    rank = np.random.default_rng(5).permutation(nb)
    j, c = np.indices((nb, CAP_CLASSES))
    p[:, 4] = 5.0 - 3.0 * rank / nb
    p[:, 5:] = np.where((j + c) % 2 == 0, 20.0, -20.0)
    if extra:
        p[0, 5 + 1] = 20.0
    return p.reshape(1, CAP_GRID, CAP_GRID, 5 + CAP_CLASSES)


@functools.lru_cache(maxsize=None)
def cap(extra=False):
    """(preds [one scale], the oracle's rows or code, candidates)."""
    preds = [cap_preds(extra)]
    preds[0].setflags(write=False)
    stats = {}
    try:
        rows = tuple(LO.detect([preds[0][0]], cap_multi(), stats))
    except LO.TooManyCandidates:
        rows = -3
    return preds, rows, stats["candidates"]


# name: the case in the middle, the seed of its two neighbours
SANDWICH = {"cap": 21, "cap+1": 21, "over": 22}


def sandwich_multi(name):
    return dense_multi("over") if name == "over" else cap_multi()


@functools.lru_cache(maxsize=None)
def sandwich(name):
    """A batch of three images of one head, the case between two ordinary seeded images
    (post_head_oracle.synthetic_predictions with box-size logits scaled by 0.25 and objectness
    logits lowered by 4, a few thousand candidates each): (preds per scale [3, ...], per image the oracle's rows or code)."""
    multi = sandwich_multi(name)
    mid = dense_preds("over") if name == "over" else cap_preds(name == "cap+1")[None]
    rng = np.random.default_rng(SANDWICH[name])
    side = [[O.synthetic_predictions(rng, h, tw_scale=0.25) for h in multi.scales] for _ in range(2)]
    for s, h in enumerate(multi.scales):  # objectness - 4: the oracle's NMS stays around a second
        for img in side:
            img[s].reshape(-1, 5 + h.n_classes)[:, 4] -= np.float32(4.0)
    preds = [np.stack([side[0][s], mid[s][0], side[1][s]]) for s in range(len(multi.scales))]
    for p in preds:
        p.setflags(write=False)
    return preds, tuple(LO.detect_or_code([p[i] for p in preds], multi) for i in range(3))
