"""Cases of the DFL head decode (yolo_post.DflHead, csrc/postprocess_dfl.hip) for tests/test_gpu_post_dfl.py.
Inputs and oracle results are built once per process and shared: callers must not modify them.

Decision-stable inputs: class logits are "off" (uniform in [-8, -4]) or "on" (0.3 + 0.001 i, every i once per
case: scores 2e-4 apart, far from score_thr); a side's logits are two adjacent bins within 2 of each other and
the rest 3 to 6 below (spread <= 8), redrawn until no corner of the point is within 2 CORNER_PX of a whole
pixel.  want() asserts the margins, at import for every case and mode, so a bad seed fails there.

CORNER_PX, the bound on |device corner - float64 corner| before truncation, for logit spreads L <= 8, strides
that are powers of two <= 32 and corners within 32 cells of the origin.  In units of u = 2**-24: exp within
2.6 ulp = 5.2 u (numpy's fp32 exp, which np_expf restates), its argument x - m off by L u: e[k] within (5.2 + L) u;
the ascending sum of <= 16 positive terms adds 15 u; p[k] = e[k] / sum is within 2 (5.2 + L) + 16 u; the
product p[k] * k adds 1 and the ascending sum of the products 15: d is within (2 (5.2 + L) + 32) u = 58.4 u
= 3.5e-6 of itself, and d <= 15 cells, so 5.2e-5 cells = 1.7e-3 px at stride 32.  (col + 0.5) -+ d rounds once
(<= 32 cells: 2e-6 cells = 6e-5 px) and the power-of-two stride is exact: below 1.8e-3 px, rounded up."""
import collections
import functools

import numpy as np

import post_dfl_oracle as O

CORNER_PX = 2.0e-3
SCORE_THR, IOU_THR = 0.25, 0.45
MODES = {"any": ("any", "argmax"), "per_class": ("per_class", "argmax"), "multi": ("per_class", "multi")}
THREE = ((2, 3, 32.0), (4, 6, 16.0), (7, 9, 8.0))  # 93 points: nothing a multiple of the wave or of 4

Case = collections.namedtuple("Case", "scales reg_max classes batch seed kind")
CASES = {
    "cell_r16_c1": Case(((1, 1, 8.0),), 16, 1, 1, 1, ""),
    "odd_r5_c3": Case(((3, 5, 16.0),), 5, 3, 3, 2, ""),
    "three_r16_c80": Case(THREE, 16, 80, 3, 3, ""),
    "three_r2_c128": Case(THREE, 2, 128, 1, 4, ""),
    "three_r5_c1": Case(THREE, 5, 1, 3, 5, ""),
    "empty": Case(((3, 5, 16.0),), 16, 3, 1, 6, "empty"),  # no candidate
    "ties": Case(THREE, 16, 80, 1, 7, "ties"),             # points 10 and 40 carry the same class logits
    "nan": Case(THREE, 16, 3, 3, 18, "nan"),               # a NaN box logit in a candidate of image 1: -1 there only
    # two decode workgroups; image 0: 129 x 128 = 16,512 multi-label candidates (-3), image 1 clean, point 288 on
    "cap": Case(((17, 17, 8.0),), 16, 128, 2, 9, "cap"),
}


def head_of(name):
    c = CASES[name]
    return O.Dfl(c.scales, c.classes, c.reg_max, SCORE_THR, IOU_THR)


def device_head(name, mode):
    import yolo_post
    c = CASES[name]
    return yolo_post.DflHead(c.scales, c.classes, c.reg_max, SCORE_THR, IOU_THR, *MODES[mode])


def _side(rng, n):
    x = rng.uniform(-6.0, -3.0, n)
    b = int(rng.integers(n - 1))
    x[b], x[b + 1] = 0.0, rng.uniform(-2.0, 2.0)
    return x


@functools.lru_cache(maxsize=None)
def preds(name):
    """One read-only fp32 array [batch, grid_h, grid_w, 4 * reg_max + classes] per scale."""
    c, head = CASES[name], head_of(name)
    rng = np.random.default_rng(c.seed)
    out = [np.zeros((c.batch, gh, gw, 4 * c.reg_max + c.classes), np.float32) for gh, gw, _ in c.scales]
    pts = O.points(head)
    on_ids = iter(rng.permutation(1024))
    for b in range(c.batch):
        image = [p[b] for p in out]
        for k, (s, row, col) in enumerate(pts):
            q = image[s][row, col]
            while True:
                q[:4 * c.reg_max] = np.concatenate([_side(rng, c.reg_max) for _ in range(4)])
                if all(abs(v - round(v)) > 2 * CORNER_PX for v in O.corners(image, head, (s, row, col))):
                    break
            q[4 * c.reg_max:] = rng.uniform(-8.0, -4.0, c.classes)
            on = rng.random() < 0.6 or k in (10, 40, len(pts) - 1)
            if c.kind == "cap" and b == 0:
                on = False
                if k < 129:
                    q[4 * c.reg_max:] = 1.0  # every class a label, all scores equal
            if on and c.kind != "empty":
                for cl in rng.choice(c.classes, 1 + int(rng.integers(min(c.classes, 3))), replace=False):
                    q[4 * c.reg_max + cl] = 0.3 + 0.001 * next(on_ids)
        if c.kind == "ties":
            (s, row, col), (s2, row2, col2) = pts[40], pts[10]
            image[s][row, col, 4 * c.reg_max:] = image[s2][row2, col2, 4 * c.reg_max:]
        if c.kind == "nan" and b == 1:
            s, row, col = pts[40]
            image[s][row, col, c.reg_max + 1] = np.nan
    for p in out:
        p.setflags(write=False)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def want(name, mode):
    """Per image the oracle's rows or code, with the margins of every decision asserted."""
    head, ps, seen = head_of(name), preds(name), {}
    out = tuple(O.detect_or_code([p[i] for p in ps], head, *MODES[mode], seen=seen) for i in range(CASES[name].batch))
    for p in ps:  # every class probability, candidate or not
        prob = 1.0 / (1.0 + np.exp(-p[..., 4 * head.reg_max:].astype(np.float64)))
        assert np.nanmin(np.abs(prob - SCORE_THR)) > 1e-5, name
    scores = np.unique(seen.get("score", []))
    assert len(scores) < 2 or np.diff(scores).min() > 1e-6, name
    assert all(abs(q - IOU_THR) > 1e-4 for q in seen.get("iou", [])), name
    assert all(abs(v - round(v)) > CORNER_PX and abs(v) < 1024 for v in seen.get("corner", [])), name
    assert all(st in (8.0, 16.0, 32.0) for _, _, st in head.scales)
    return out


def counts_of(rows):
    return [r if isinstance(r, int) else len(r) for r in rows]


for _name in CASES:
    for _mode in MODES:
        want(_name, _mode)
assert counts_of(want("empty", "multi")) == [0]
assert counts_of(want("nan", "any"))[1] == -1 and min(counts_of(want("nan", "any"))[::2]) > 0
assert counts_of(want("cap", "multi"))[0] == -3 and counts_of(want("cap", "multi"))[1] > 0
assert counts_of(want("cap", "per_class"))[0] > 0
_ties = sorted(O.candidates([p[0] for p in preds("ties")], head_of("ties"), "argmax"), key=lambda t: t[1])
assert [(a[0], a[2]) for a in _ties if a[1] == 10] == [(a[0], a[2]) for a in _ties if a[1] == 40] != []
