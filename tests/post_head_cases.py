"""Seeded cases of the multi-scale postprocessing tests (tests/test_post_head_cpu.py checks on
the CPU that they stay inside their conditions; tests/test_gpu_post_head.py runs them on the
GPU).  Oracle results are computed once per process and shared: callers must not modify them.

PARITY     head name -> (head parameters, images, seed): ordinary-density batches from
           post_head_oracle.batch (every 4th image with 6x box-size logits).  The seeds were
           chosen on the CPU so that at most a quarter of a head's images make the reference
           raise and every multi-cell head yields at least 100 detections:
             voc19 940 detections, 1 of 8 raises    coco13 325, 0 of 4    tiny3x5 243, 0 of 16
             wide6 405, 1 of 8                      one 4, 0 of 8
           lds2048 / ws2050 are the largest head whose boxes stay in LDS and the smallest
           that uses the workspace.
SATURATED  name -> (head parameters, seed, raises): every box a candidate (objectness 8,
           class boost 12).  At 40 x 40 (8000 boxes) most seeds make the reference raise on a
           zero IoU denominator, so one raising and one non-raising seed are kept.
CAP        the largest head the library takes, 1 x 1024 cells x 8 anchors x 1 class = 8192
           boxes, saturated.  In one row of cells with boxes taller than two cells every pair
           of boxes overlaps vertically, so no IoU denominator is zero, and 2402 of the 8192
           candidates survive: a kept list far longer than one 64-candidate block.  The
           oracle needs 11 s for it, so its rows are recorded in
           tests/golden/post_cap8192_golden.json (`python tests/post_head_cases.py` rewrites
           the file from the oracle) instead of being computed in the test.
DENSE      every candidate kept, the tightest case for a kept list written in place over its own
           keys (it grows by 64 for every 64 keys consumed; saturated inputs suppress most boxes
           and never reach this): 1 x n cells for n around the 64-candidate block, one anchor
           (0.25, 0.25), two classes, tx = ty = tw = th = 0, class logits (6, 0), objectness a
           seeded permutation of linspace(2, 8, n).  The boxes are 8 pixels wide in 32-pixel
           cells of one row: disjoint horizontally, overlapping vertically, so no IoU denominator
           is zero and no pair exceeds the threshold.
"""
import functools
import json
import os

import numpy as np

import post_head_oracle as O
import post_numpy as PN

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

ANCHORS3 = (1.5, 2.0, 4.0, 3.0, 8.0, 9.5)
ANCHORS9 = tuple(float(v) for v in np.round(np.linspace(0.5, 9.0, 18), 2))
ANCHORS8 = tuple(v for i in range(8) for v in (0.75 + 0.75 * i, 4.0 + 0.5 * i))

# name: ((grid_h, grid_w), anchors, classes), images, seed
PARITY = {
    "voc19": (((19, 19), PN.ANCHORS, 20), 8, 102),
    "coco13": (((13, 13), PN.ANCHORS, 80), 4, 101),
    "tiny3x5": (((3, 5), ANCHORS3, 7), 16, 101),
    "wide6": (((6, 6), ANCHORS9, 3), 8, 101),
    "one": (((1, 1), (2.0, 3.0), 1), 8, 101),
    "lds2048": (((16, 16), ANCHORS9[:16], 2), 2, 101),
    "ws2050": (((41, 10), PN.ANCHORS, 2), 2, 101),
}
MULTI_CELL = ("voc19", "coco13", "tiny3x5", "wide6")

# name: ((grid_h, grid_w), anchors, classes), seed, the reference raises ZeroDivisionError
SATURATED = {
    "voc19": (((19, 19), PN.ANCHORS, 20), 201, False),
    "voc19_zero_den": (((19, 19), PN.ANCHORS, 20), 204, True),
    "voc40": (((40, 40), PN.ANCHORS, 20), 205, False),
    "voc40_zero_den": (((40, 40), PN.ANCHORS, 20), 201, True),
}

CAP = (((1, 1024), ANCHORS8, 1), 302, 0.5)  # head parameters, seed, scale of the box-size logits
CAP_GOLDEN = os.path.join(GOLDEN, "post_cap8192_golden.json")

DENSE = (63, 64, 65, 128, 129)  # n: one block short by one, one block, one over, two, two and one
DENSE_SEED = 401


def dense_spec(n):
    return ((1, n), (0.25, 0.25), 2)


def oracle_head(spec, score_thr=0.3, iou_thr=0.3):
    (gh, gw), anchors, classes = spec
    return O.Head(gh, gw, len(anchors) // 2, classes, tuple(anchors), 32.0, score_thr, iou_thr)


def device_head(spec, score_thr=0.3, iou_thr=0.3):
    import yolo_post
    grid, anchors, classes = spec
    return yolo_post.YoloHead(grid, anchors=anchors, classes=classes, score_thr=score_thr, iou_thr=iou_thr)


@functools.lru_cache(maxsize=None)
def parity(name, score_thr=0.3, iou_thr=0.3):
    """(preds [n, gh, gw, n_out], per image the oracle's rows or its negative code)."""
    spec, n, seed = PARITY[name]
    head = oracle_head(spec, score_thr, iou_thr)
    preds = O.batch(seed, head, n)
    preds.setflags(write=False)
    return preds, tuple(O.detect_or_code(p, head) for p in preds)


@functools.lru_cache(maxsize=None)
def saturated(name):
    """(pred [gh, gw, n_out], the oracle's rows or -2, candidates)."""
    spec, seed, _ = SATURATED[name]
    head = oracle_head(spec)
    pred = O.synthetic_predictions(np.random.default_rng(seed), head, saturate=True)
    pred.setflags(write=False)
    stats = {}
    try:
        rows = O.detect(pred, head, stats)
    except ZeroDivisionError:
        rows = -2
    return pred, rows, stats.get("candidates")


@functools.lru_cache(maxsize=None)
def dense(n):
    """(pred [1, n, 7], the oracle's rows or its negative code)."""
    head = oracle_head(dense_spec(n))
    pred = np.zeros((1, n, 7), np.float32)
    pred[0, :, 4] = np.random.default_rng(DENSE_SEED + n).permutation(np.linspace(2.0, 8.0, n)).astype(np.float32)
    pred[0, :, 5] = 6.0
    pred.setflags(write=False)
    return pred, O.detect_or_code(pred, head)


def cap8192(compute=False):
    """(pred [1, 1024, 48], rows): the recorded oracle rows, or with compute=True the oracle's."""
    spec, seed, tw = CAP
    head = oracle_head(spec)
    pred = O.synthetic_predictions(np.random.default_rng(seed), head, tw_scale=tw, saturate=True)
    if compute:
        return pred, O.detect(pred, head)
    with open(CAP_GOLDEN) as f:
        return pred, [tuple(r) for r in json.load(f)["rows"]]


def ms_golden():
    """The embedded reference goldens (tests/golden/make_golden_post_ms.py):
    name -> (pred [gh, gw, 125], {"grid", "boxes" | "raises"})."""
    with open(os.path.join(GOLDEN, "post_ms_golden.json")) as f:
        gold = json.load(f)["cases"]
    d = np.load(os.path.join(GOLDEN, "post_ms_cases.npz"))
    assert sorted(d.files) == sorted(gold)
    return {k: (d[k], gold[k]) for k in sorted(gold)}


def same_rows(got, want, what, rtol=1e-6):
    """Classes, corners and order identical; scores equal to the suite's rtol (the last bits
    of exp / pow differ between numpy and the device)."""
    if isinstance(want, int) or isinstance(got, int):
        assert got == want, f"{what}: {got if isinstance(got, int) else 'rows'} != {want if isinstance(want, int) else 'rows'}"
        return
    assert [r[:5] for r in got] == [r[:5] for r in want], what
    np.testing.assert_allclose([r[5] for r in got], [r[5] for r in want], rtol=rtol, err_msg=what)


if __name__ == "__main__":
    _pred, _rows = cap8192(compute=True)
    with open(CAP_GOLDEN, "w") as _f:
        json.dump({"source": "tests/post_head_oracle.detect on tests/post_head_cases.CAP under numpy "
                             + np.__version__, "rows": _rows}, _f)
    print(len(_rows), "rows ->", CAP_GOLDEN)
