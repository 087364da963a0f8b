"""Float64 restatement of the instance masks of a DFL head (include/dnn_hip_post.h: dnn_yolo_seg), plain numpy;
shares no code with yolo_post.  Rows come from the DFL oracle (tests/post_dfl_oracle.py), which does not say
which grid point a row came from: rows_points recomputes it from the oracle's own candidates."""
import numpy as np

import post_dfl_oracle as O

U = 2.0 ** -24


def margin(nm):
    """2 gamma_(nm + 1): twice the standard bound on an fp32 dot product of length nm relative to sum |a b|,
    doubled because the order and rounding of the MFMA's four products are not documented."""
    return 2.0 * (nm + 1) * U / (1.0 - (nm + 1) * U)


def rows_points(image, head, nms, labels):
    """(rows, points) of one image, or (code, None): points[k] is the global grid point of row k.  A row's
    (score, class) must name one candidate."""
    rows = O.detect_or_code(image, head, nms, labels)
    if isinstance(rows, int):
        return rows, None
    at = {}
    for v, k, cl in O.candidates(image, head, labels):
        assert (v, cl) not in at, "two candidates share a score and a class"
        at[(v, cl)] = k
    return rows, [at[(r[5], r[0])] for r in rows]


def crop(corners, mask_hw, net_hw):
    """bool [mask_h, mask_w]: the pixels inside (left, top, right, bottom) by the integer rule."""
    (mh, mw), (nh, nw) = mask_hw, net_hw
    left, top, right, bottom = corners
    left, right = min(max(left, 0), nw), min(max(right, 0), nw)
    top, bottom = min(max(top, 0), nh), min(max(bottom, 0), nh)
    xs = np.array([left * mw <= x * nw < right * mw for x in range(mw)], bool)
    ys = np.array([top * mh <= y * nh < bottom * mh for y in range(mh)], bool)
    return ys[:, None] & xs[None, :]


def logits(coefs, proto, head, point):
    """(logit64, S) [mask_h, mask_w] of a grid point: coefs one [grid_h, grid_w, nm] array per scale, proto
    [mask_h, mask_w, nm]; S = sum_c |coef[c] proto[y][x][c]|."""
    s, r, c = O.points(head)[point]
    terms = proto.astype(np.float64) * coefs[s][r, c].astype(np.float64)
    return terms.sum(axis=2), np.abs(terms).sum(axis=2)
