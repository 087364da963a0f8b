"""CPU: the scale_x_y decode oracle alone (tests/post_xy_oracle.py), no device: it equals the existing
multi, class-wise and multi-label oracles at s = 1, and on the decode test inputs
(tests/post_xy_cases.py) the rows for the heads' own scale_x_y differ from the rows at s = 1, so the
GPU comparison in tests/test_gpu_post_xy.py cannot pass vacuously."""
import numpy as np
import pytest

import post_classwise_oracle as CO
import post_multi_oracle as MO
import post_multilabel_oracle as LO
import post_xy_cases as XK
import post_xy_oracle as XO

OLD = {"any": MO, "per_class": CO, "multi": LO}


def test_the_bias_is_darknets_in_fp32():
    assert XO.xy_bias(1.0) == 0 and np.signbit(XO.xy_bias(1.0))  # -0.5f * 0.0f = -0.0f
    s = np.float32(1.05)
    assert XO.xy_bias(1.05) == np.float32(np.float32(-0.5) * np.float32(s - np.float32(1.0)))
    assert XO.xy_bias(1.05).dtype == np.float32 and abs(float(XO.xy_bias(1.05)) + 0.025) < 1e-7
    assert XO.xy_bias(2.0) == np.float32(-0.5)


@pytest.mark.parametrize("mode", XO.MODES)
@pytest.mark.parametrize("name", sorted(XK.HEADS))
def test_at_one_the_oracle_is_the_existing_one(name, mode):
    multi, preds = XK.multi_of(name), XK.inputs(name)
    ones = (1.0,) * len(multi.scales)
    want = tuple(OLD[mode].detect_or_code([p[i] for p in preds], multi) for i in range(XK.IMAGES))
    assert XK.refs(name, mode, ones) == want
    assert any(not isinstance(w, int) and len(w) > 0 for w in want)


@pytest.mark.parametrize("mode", XO.MODES)
@pytest.mark.parametrize("name", sorted(XK.HEADS))
def test_the_heads_own_scale_moves_a_corner(name, mode):
    multi = XK.multi_of(name)
    own, one = XK.refs(name, mode), XK.refs(name, mode, (1.0,) * len(multi.scales))
    moved = 0
    for a, b in zip(own, one):
        if isinstance(a, int) or isinstance(b, int) or len(a) != len(b):
            moved += a != b
            continue
        moved += sum(ra[1:5] != rb[1:5] for ra, rb in zip(a, b))
    print(f"{name} {mode}: counts {XK.counts_of(own)} at {XK.xy_of(name)}, {XK.counts_of(one)} at 1; {moved} rows differ")
    assert moved >= 1
    assert any(not isinstance(r, int) and len(r) > 0 for r in own)


def test_a_scale_at_one_leaves_its_own_boxes_alone():
    """(1.0, 1.05): scale 0's corners are the plain decode's, scale 1's move."""
    name = "one_and_1.05"
    multi, preds = XK.multi_of(name), XK.inputs(name)
    n0 = MO.scale_boxes(multi.scales[0])
    moved0 = moved1 = 0
    for i in range(XK.IMAGES):
        img = [p[i] for p in preds]
        own, one = XO.all_corners(img, multi, XK.xy_of(name)), XO.all_corners(img, multi, (1.0, 1.0))
        assert one == [d[0] for d in MO.decode(img, multi)]
        moved0 += sum(a != b for a, b in zip(own[:n0], one[:n0]))
        moved1 += sum(a != b for a, b in zip(own[n0:], one[n0:]))
    assert moved0 == 0 and moved1 > 0


def test_pushed_centres_cross_the_cell_border():
    """sigmoid(8) * 1.2 - 0.1 > 1: the centre leaves its cell, which no s = 1 decode can do."""
    name = "two_scales"
    multi, preds = XK.multi_of(name), XK.inputs(name)
    head = multi.scales[0]
    p = preds[0][1].reshape(head.grid_h, head.grid_w, head.n_anchors, -1)
    hits = 0
    for row in range(head.grid_h):
        for col in range(head.grid_w):
            for b in range(head.n_anchors):
                if p[row, col, b, 0] == 8:
                    l, _, r, _ = XO.corners(p, row, col, b, head, 1.2)
                    l1, _, r1, _ = XO.corners(p, row, col, b, head, 1.0)
                    assert (l + r) - (l1 + r1) >= 4  # centre 3.2 pixels right: the corner sum moves by about 6.4
                    hits += 1
    assert hits >= 1
