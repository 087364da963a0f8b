"""Seeded cases of the grid-wide multi-scale decode (yolo_post.WideHead, csrc/postprocess_wide.hip):
tests/test_post_wide_cpu.py checks on the CPU that they stay inside their conditions,
tests/test_gpu_post_wide.py runs them on the GPU.  Oracle results are computed once per process and
shared: callers must not modify them.  The oracles are the existing ones, which have no box limit.

MODES   the three (nms, labels) pairs and each one's oracle.
ABOVE   heads above the old 16,384-box cap, the smallest that set bit 14 of the box index:
          four    9, 18, 36, 64 cells x 3 anchors x 3 classes = 17,391 boxes over four scales (no
                  multiple of a decode chunk; the scale boundaries 243, 1,215 and 5,103 fall inside
                  chunks)
          yolov3  19, 38, 76 x 3 x 3 = 22,743 boxes, the 608 x 608 model's grids
        post_multi_oracle.batch inputs of 4 images (image 0 with 6x box-size logits), score > 0.997,
        IoU > 0.45: about 70 to 120 candidates an image.  At 0.99 every image of `four` has a zero
        IoU denominator under the class-agnostic rule.  The seeds were chosen on the CPU
        (`python tests/post_wide_cases.py` searches) so that in every mode exactly one image of the
        batch yields a code and at least one kept row is a box with global index >= 16,384.
COCO608 one image of 19, 38, 76 x 3 x 80 classes (22,743 boxes), score > 0.99.
CAP     the candidate cap on `four`'s grids: every anchor a side of 10^6 pixels and zero size
        logits, so all boxes overlap; objectness +20 on a seeded subset of the boxes and -20
        elsewhere, class logits in [3, 6] (every class of an "on" box is a label), or for a
        single-label box -20 on all classes but one.
EDGE    one scale of 128 x 128 cells x 4 anchors x 1 class = 65,536 boxes, the wide limit, with a
        handful of boxes on, box 65,535 among them.
E2E     the narrow YOLOv3-tiny of tests/test_gpu_darknet.py at 1088 x 1088 (17,340 boxes), frame 0.
        Its random weights give every box an objectness near 0.5, so Darknet's 0.5 leaves no row;
        E2E_LOW_THR was chosen on the CPU from darknet_oracle.forward: at 0.34 the multi-label
        oracle gives about a hundred rows, some of boxes >= 16,384 (at 0.32 an IoU denominator is
        zero, at 0.2 there are more than 16,384 candidates).
"""
import functools

import numpy as np

import post_classwise_oracle as CO
import post_head_oracle as O
import post_multi_cases as K
import post_multi_oracle as MO
import post_multilabel_oracle as LO

OLD_CAP = 16384  # DNN_YOLO_MULTI_MAX_BOXES, DNN_YOLO_MULTI_MAX_CANDIDATES

# name -> (nms, labels, oracle module)
MODES = {"any": ("any", "argmax", MO), "per_class": ("per_class", "argmax", CO), "multi": ("per_class", "multi", LO)}

# the fourth scale of `four`: stride 4, anchors in pixels
STRIDE4_ANCHORS = (4, (5, 7, 8, 15, 16, 11))

# name: grids, classes, images, seed, score threshold, IoU threshold
ABOVE = {
    "four": ((9, 18, 36, 64), 3, 4, 5, 0.997, 0.45),
    "yolov3": ((19, 38, 76), 3, 4, 9, 0.997, 0.45),
}
COCO608 = ((19, 38, 76), 80, 1, 5, 0.99, 0.45)

CAP_GRIDS, CAP_CLASSES, CAP_SIDE, CAP_SEED = (9, 18, 36, 64), 3, 1.0e6, 7
EDGE_GRID, EDGE_ANCHORS = 128, 4
EDGE_ON = (0, 1, 511, 16383, 16384, 40000, 65534, 65535)
E2E_SIZE, E2E_WIDTH_DIV, E2E_CLASSES, E2E_FRAME, E2E_LOW_THR = 1088, 16, 3, 0, 0.34


def counts_of(refs):
    return [r if isinstance(r, int) else len(r) for r in refs]


def multi_of(grids, classes, score_thr, iou_thr, anchors=None):
    """post_multi_oracle's description: YOLOv3's strides and anchors, a fourth scale at stride 4;
    `anchors` (w, h in pixels) replaces every anchor."""
    table = K.YOLOV3_ANCHORS + (STRIDE4_ANCHORS,)
    scales = []
    for g, (st, px) in zip(grids, table):
        px = px if anchors is None else anchors * 3
        scales.append(O.Head(g, g, 3, classes, tuple(a / st for a in px), float(st), score_thr, iou_thr))
    return MO.Multi(tuple(scales), "logistic")


def device_head(multi, mode, cls=None):
    """The yolo_post.WideHead (or `cls`) of an oracle description in one of MODES."""
    import yolo_post
    nms, labels, _ = MODES[mode]
    return (cls or yolo_post.WideHead)(multi.scales, multi.class_mode, nms, labels)


def boxes_of(multi):
    return sum(MO.scale_boxes(h) for h in multi.scales)


def refs_of(preds, multi, mode):
    """Per image the mode's oracle rows, or its code."""
    oracle = MODES[mode][2]
    return tuple(oracle.detect_or_code([p[i] for p in preds], multi) for i in range(preds[0].shape[0]))


def high_corners(preds, multi, image):
    """The corner tuples that only boxes of global index >= 16,384 of one image have."""
    boxes = MO.decode([p[image] for p in preds], multi)
    low = {tuple(b[0]) for b in boxes[:OLD_CAP]}
    return {tuple(b[0]) for b in boxes[OLD_CAP:]} - low


def above_multi(name):
    grids, classes, _, _, thr, iou = ABOVE[name]
    return multi_of(grids, classes, thr, iou)


def above_preds(name, seed=None):
    _, _, n, s, _, _ = ABOVE[name]
    preds = MO.batch(s if seed is None else seed, above_multi(name), n)
    for p in preds:
        p.setflags(write=False)
    return preds


@functools.lru_cache(maxsize=None)
def above(name, seed=None):
    """(preds per scale [n, g, g, n_out], {mode: per image the oracle's rows or code}, {mode: rows
    of clean images that are boxes of index >= 16,384})."""
    multi, preds = above_multi(name), above_preds(name, seed)
    refs = {mode: refs_of(preds, multi, mode) for mode in MODES}
    high = {mode: 0 for mode in MODES}
    for i in range(preds[0].shape[0]):
        if all(isinstance(refs[mode][i], int) for mode in MODES):
            continue
        hc = high_corners(preds, multi, i)
        for mode in MODES:
            if not isinstance(refs[mode][i], int):
                high[mode] += sum(tuple(r[1:5]) in hc for r in refs[mode][i])
    return preds, refs, high


def above_ok(refs, high):
    """The conditions of ABOVE: per mode 1 <= coded images <= a quarter, a kept row of a high box."""
    for mode in MODES:
        codes = sum(isinstance(r, int) for r in refs[mode])
        if not 1 <= codes <= len(refs[mode]) // 4 or high[mode] < 1:
            return False
    return True


def coco608_multi():
    grids, classes, _, _, thr, iou = COCO608
    return multi_of(grids, classes, thr, iou)


@functools.lru_cache(maxsize=None)
def coco608():
    """(preds [1, ...] per scale, {mode: (rows or code,)})."""
    multi = coco608_multi()
    preds = MO.batch(COCO608[3], multi, COCO608[2], tw_every=10 ** 9)
    for p in preds:
        p.setflags(write=False)
    return preds, {mode: refs_of(preds, multi, mode) for mode in MODES}


# ------------------------------------------------------------------ the candidate cap
def cap_multi():
    return multi_of(CAP_GRIDS, CAP_CLASSES, 0.3, 0.45, anchors=(CAP_SIDE, CAP_SIDE))


def cap_image(on, single=0, seed=CAP_SEED, bad=False):
    """One image per scale [g, g, 3 * (5 + 3)]: `on` boxes of a seeded order have objectness +20 and
    all three classes as labels, the next `single` boxes of that order objectness +20 and class 1
    alone; everything else is off.  bad: the LAST box's width logit is 100 (an infinite corner)."""
    multi = cap_multi()
    nb, c = boxes_of(multi), CAP_CLASSES
    rng = np.random.default_rng(seed)
    order = rng.permutation(nb)
    p = np.zeros((nb, 5 + c), np.float32)
    p[:, 0:2] = rng.standard_normal((nb, 2)).astype(np.float32)
    p[:, 4] = -20.0
    p[:, 5:] = rng.uniform(3.0, 6.0, size=(nb, c)).astype(np.float32)
    p[order[:on + single], 4] = 20.0
    lone = order[on:on + single]
    p[lone, 5:] = -20.0
    p[lone, 5 + 1] = 4.0
    if bad:
        p[nb - 1, 2] = 100.0
    out, at = [], 0
    for h in multi.scales:
        n = MO.scale_boxes(h)
        out.append(p[at:at + n].reshape(h.grid_h, h.grid_w, h.n_anchors * (5 + c)))
        at += n
    return out


def cap_batch(images):
    """Images (lists of per-scale tensors) stacked into one read-only array per scale."""
    preds = [np.stack([im[s] for im in images]) for s in range(len(images[0]))]
    for p in preds:
        p.setflags(write=False)
    return preds


# what every mode's batch holds: name -> cap_image's arguments.  In the single-label modes a box
# is one candidate, in multi-label mode a three-label box is three.
CAP_IMAGES = {
    "any": {"at": (16384, 0), "over": (16385, 0)},
    "per_class": {"at": (16384, 0), "over": (16385, 0)},
    "multi": {"at": (5461, 1), "over": (5461, 2)},
}


@functools.lru_cache(maxsize=None)
def cap(mode):
    """(preds of the batch [at the cap, over, clean, bad corner, empty], the oracle's rows or codes).
    The single-label oracles have no candidate limit: `over` is -3 by the entry's contract (one
    candidate more than `at`, whose count the CPU test checks)."""
    multi = cap_multi()
    at, over = CAP_IMAGES[mode]["at"], CAP_IMAGES[mode]["over"]
    images = [cap_image(*at), cap_image(*over), cap_image(40, 3), cap_image(40, 3, bad=True), cap_image(0)]
    preds = cap_batch(images)
    oracle = MODES[mode][2]
    refs = [oracle.detect_or_code([p[i] for p in preds], multi) if i != 1 else -3 for i in range(len(images))]
    return preds, tuple(refs)


# ------------------------------------------------------------------ the wide limit
def edge_multi():
    head = O.Head(EDGE_GRID, EDGE_GRID, EDGE_ANCHORS, 1, (1.0, 1.0, 2.0, 1.0, 1.0, 2.0, 3.0, 3.0), 8.0, 0.3, 0.45)
    return MO.Multi((head,), "logistic")


@functools.lru_cache(maxsize=None)
def edge():
    """(preds [1, 128, 128, 24], (rows,)): EDGE_ON's boxes on with seeded objectness, the rest off."""
    multi = edge_multi()
    nb = boxes_of(multi)
    rng = np.random.default_rng(3)
    p = rng.standard_normal((nb, 6)).astype(np.float32)
    p[:, 4] = -20.0
    p[list(EDGE_ON), 4] = rng.uniform(2.0, 6.0, size=len(EDGE_ON)).astype(np.float32)
    p[list(EDGE_ON), 5] = 3.0
    preds = [p.reshape(1, EDGE_GRID, EDGE_GRID, EDGE_ANCHORS * 6)]
    preds[0].setflags(write=False)
    return preds, (MO.detect_or_code([preds[0][0]], multi),)


# ------------------------------------------------------------------ the one-workgroup entries' small cases
# The per-class phases are one set of device helpers for both index widths (csrc/post_multi_dev.h), so
# the wide entry also runs the cases that were built for the one-workgroup kernels: name -> mode.
#   dense, dense80   post_multilabel_cases.DENSE: every segment above the whole-workgroup threshold
#                    and a merge of three chunks; every segment one wave's and a merge of two
#   bounds           post_classwise_cases: segments of 1, 63, 64, 0, 65 and 129 candidates
#   threshold        the same around the whole-workgroup threshold: 256, 257, 255, 320
#   small_softmax    post_multilabel_cases.SEEDED's softmax case (no seeded softmax case has more than
#                    1024 rows): the merge's softmax scores
SMALL = {"dense": "multi", "dense80": "multi", "bounds": "per_class", "threshold": "per_class",
         "small_softmax": "multi"}


@functools.lru_cache(maxsize=None)
def small(name):
    """(description, preds per scale [n, ...], mode, per image the mode's oracle rows or code, the
    oracle's stats of a one-image case: candidates and their classes)."""
    import post_classwise_cases as CK
    import post_multilabel_cases as LK
    mode = SMALL[name]
    if name in ("dense", "dense80"):
        preds, rows, stats = LK.dense(name)
        return LK.dense_multi(name), preds, mode, (rows,), stats
    if name == "small_softmax":
        preds, refs = LK.seeded(name)
        return LK.seeded_multi(name), preds, mode, refs, None
    sizes = CK.BOUNDS_SIZES if name == "bounds" else CK.THRESHOLD_SIZES
    multi, preds, stats = CK.bounds_multi(sizes), [CK.bounds_preds(sizes)], {}
    preds[0].setflags(write=False)
    return multi, preds, mode, (tuple(CO.detect([preds[0][0]], multi, stats)),), stats


# ------------------------------------------------------------------ end to end
def e2e_model():
    """(cfg text, sections, layers, frame [1, 1088, 1088, 3])."""
    import darknet_cases as DC
    import darknet_import as D
    import synth
    cfg = D.cfg_text("yolov3-tiny", classes=E2E_CLASSES, width=E2E_SIZE, height=E2E_SIZE, width_div=E2E_WIDTH_DIV)
    secs = D.parse_cfg(cfg)
    return cfg, secs, DC.darknet_layers(secs), synth.frames([E2E_FRAME], shape=(E2E_SIZE, E2E_SIZE, 3))


def e2e_oracle(head):
    """(the multi-label oracle's rows or code on darknet_oracle.forward's outputs for `head`'s
    thresholds, how many rows are boxes of index >= 16,384)."""
    import darknet_oracle as DO
    _, secs, layers, x = e2e_model()
    preds = [np.asarray(o, np.float32) for o in DO.forward(secs, layers, x)]
    multi = MO.Multi(tuple(head.scales), "logistic")
    rows = LO.detect_or_code([p[0] for p in preds], multi)
    if isinstance(rows, int):
        return rows, 0
    hc = high_corners(preds, multi, 0)
    return rows, sum(tuple(r[1:5]) in hc for r in rows)


if __name__ == "__main__":
    for _name in ABOVE:
        for _seed in range(12):
            _, _refs, _high = above(_name, _seed)
            print(_name, "seed", _seed, {m: counts_of(r) for m, r in _refs.items()}, "high rows", _high,
                  "ok" if above_ok(_refs, _high) else "", flush=True)
            if above_ok(_refs, _high):
                break
