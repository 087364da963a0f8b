"""Shared cases of tests/test_post_xy_cpu.py and tests/test_gpu_post_xy.py: three small heads with a
scale_x_y per scale, their inputs and the oracle's rows.

Inputs are post_multi_oracle.batch's synthetic predictions with, per image and scale, the tx and ty
of the PUSHED boxes of highest objectness set to +8 and -8 in turn: there the logistic is within
4e-4 of 1 or 0, so scale_x_y = 1.05 moves the centre by 0.8 pixels of a 32-pixel cell (1.2: 3.2
pixels) and the truncated corners change."""
import functools

import numpy as np

import post_head_oracle as O
import post_multi_oracle as MO
import post_xy_oracle as XO

CELLS = ((32.0, (81, 82, 135, 169, 344, 319)), (16.0, (10, 14, 23, 27, 37, 58)))  # YOLOv3-tiny's pixel anchors
SCORE_THR, IOU_THR = 0.3, 0.45
IMAGES, SEED, PUSHED = 4, 11, 6

# name: ((grid_h, grid_w) per scale, classes, scale_x_y per scale)
HEADS = {
    "one_scale": (((2, 3),), 3, (1.05,)),
    "two_scales": (((2, 2), (4, 4)), 4, (1.2, 1.1)),
    "one_and_1.05": (((2, 2), (4, 4)), 4, (1.0, 1.05)),
}

# mode -> (nms, labels) of a yolo_post.MultiHead
MODE_ARGS = {"any": ("any", "argmax"), "per_class": ("per_class", "argmax"), "multi": ("per_class", "multi")}


def multi_of(name):
    grids, classes, _ = HEADS[name]
    scales = [O.Head(gh, gw, 3, classes, tuple(a / cell for a in px), cell, SCORE_THR, IOU_THR)
              for (gh, gw), (cell, px) in zip(grids, CELLS)]
    return MO.Multi(tuple(scales), "logistic")


def xy_of(name):
    return HEADS[name][2]


@functools.lru_cache(maxsize=None)
def inputs(name):
    """One read-only array per scale, [IMAGES, gh, gw, 3 * (5 + classes)]."""
    multi = multi_of(name)
    preds = MO.batch(SEED, multi, IMAGES)
    for pred, head in zip(preds, multi.scales):
        for i in range(IMAGES):
            p = pred[i].reshape(-1, 5 + head.n_classes)  # a view: (row, col, anchor) order
            top = np.argsort(-p[:, 4], kind="stable")[:PUSHED]
            for k, box in enumerate(top):
                p[box, 0] = np.float32(8.0 if k % 2 == 0 else -8.0)
                p[box, 1] = np.float32(-8.0 if k % 3 == 0 else 8.0)
        pred.setflags(write=False)
    return tuple(preds)


@functools.lru_cache(maxsize=None)
def refs(name, mode, xy=None):
    """Per image the oracle's rows, or its code, for scale_x_y `xy` (default: the head's own)."""
    multi, preds = multi_of(name), inputs(name)
    xy = xy_of(name) if xy is None else xy
    return tuple(XO.detect_or_code([p[i] for p in preds], multi, xy, mode) for i in range(IMAGES))


def counts_of(rs):
    return [r if isinstance(r, int) else len(r) for r in rs]


def device_head(name, mode, cls=None, xy="own"):
    """The yolo_post.MultiHead (or `cls`) of a case; xy "own": the case's scale_x_y, else as given."""
    import yolo_post
    multi = multi_of(name)
    nms, labels = MODE_ARGS[mode]
    return (cls or yolo_post.MultiHead)(multi.scales, multi.class_mode, nms, labels,
                                        scale_x_y=xy_of(name) if xy == "own" else xy)
