"""Shared cases of tests/test_letterbox_cpu.py and tests/test_gpu_letterbox.py: the size table and
a seeded uint8 image generator."""
import numpy as np

# (src_h, src_w, net_h, net_w) -> (new_h, new_w, pad_y, pad_x), worked by hand from the size rule
GEOMETRY = {
    (5, 7, 32, 32): (22, 32, 5, 0),
    (33, 17, 32, 64): (32, 16, 0, 24),
    (37, 53, 64, 96): (64, 91, 0, 2),
    (48, 64, 64, 64): (48, 64, 8, 0),
    (64, 64, 64, 64): (64, 64, 0, 0),          # identity
    (480, 640, 416, 416): (312, 416, 52, 0),
    (1080, 1920, 416, 416): (234, 416, 91, 0),
    (1, 8, 32, 32): (4, 32, 14, 0),            # a one-row source: H == 1
    (8, 1, 32, 32): (32, 4, 0, 14),            # a one-column source: W == 1
    (16, 8, 96, 96): (96, 48, 0, 24),          # the last-row rule: row 95 has iy = 14
    (100, 37, 64, 64): (64, 23, 0, 20),        # shrinking, odd pads
    (3, 2, 40, 24): (36, 24, 2, 0),            # 12 x enlargement
    (9, 33, 16, 33): (9, 33, 3, 0),            # 3 * net_w = 99: the one-float store path, same width
    (31, 19, 35, 33): (35, 21, 0, 6),          # 3 * net_w = 99, resized
}
REFUSED = [(100, 3, 64, 64), (3, 100, 64, 64)]  # a one-pixel side

SMALL = [k for k in GEOMETRY if max(k[:2]) <= 100]  # the cases the pixel tests run (<= 100 pixels a side)


def image(h, w, seed=0):
    """A seeded uint8 [h, w, 3] image with the extremes present: noise, with 0 and 255 corners."""
    rng = np.random.default_rng([h, w, seed])
    im = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    im[0, 0], im[-1, -1] = 0, 255
    return im
