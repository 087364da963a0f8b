"""TEST INFRASTRUCTURE ONLY: the squeeze-and-excitation gate in float64, by the four formulas of
include/dnn_hip_plan.h (dnn_plan_add_squeeze_excite), and the seeded tensors of its tests."""
import numpy as np

from act_oracle import act64

# name: (n, h, w, c, cr).  The kernel's range rule (squeeze_excite.hip, se_range_pixels): a range is
# max(128 KB / (4 c), ceil(h w / 64)) positions; at c = 8 that is 4,096, so the 65 x 65 = 4,225 positions of
# "two_ranges_ragged" make P = 2 ranges, the second one of 129 positions.
CASES = {
    "one_pixel": (1, 1, 1, 4, 1),
    "scalar_odd": (3, 3, 5, 6, 2),
    "wide_c320": (2, 7, 7, 320, 20),
    "two_ranges_ragged": (2, 65, 65, 8, 3),
    "b0_widest": (1, 9, 9, 1152, 48),
}


def gate64(x, w1, b1, act1, w2, b2, act2):
    x = np.asarray(x, np.float64)
    m = x.sum(axis=(1, 2)) / (x.shape[1] * x.shape[2])
    h = act64(act1, m @ np.asarray(w1, np.float64) + np.asarray(b1, np.float64))
    return act64(act2, h @ np.asarray(w2, np.float64) + np.asarray(b2, np.float64))


def forward64(x, w1, b1, act1, w2, b2, act2):
    return np.asarray(x, np.float64) * gate64(x, w1, b1, act1, w2, b2, act2)[:, None, None, :]


def tensors(name):
    """x standard normal.  The channel means are then N(0, 1 / (h w)), so w1 is N(0, h w / c): FC1's sums are
    N(0, 1) like b1; w2 is N(0, 4 / cr) and b2 N(0, 1): FC2's sums have a spread of a few units, which puts the
    logistic gates all over (0, 1) without saturating them."""
    n, h, w, c, cr = CASES[name]
    rng = np.random.default_rng(4200 + list(CASES).index(name))
    x = rng.standard_normal((n, h, w, c)).astype(np.float32)
    w1 = (rng.standard_normal((c, cr)) * np.sqrt(h * w / c)).astype(np.float32)
    w2 = (rng.standard_normal((cr, c)) * 2 / np.sqrt(cr)).astype(np.float32)
    return x, w1, rng.standard_normal(cr).astype(np.float32), w2, rng.standard_normal(c).astype(np.float32)
