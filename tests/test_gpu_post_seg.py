"""GPU: instance masks of a DFL head (dnn_yolo_postprocess_dfl_seg, csrc/postprocess_seg.hip; yolo_post.SegSpec,
detect_batch_masks, MaskDetectionBuffers) against the float64 oracle of tests/post_seg_oracle.py.

Every case is a batch of three: image 0 is built to give `rows` rows, image 1 none and image 2 the code -1 (a NaN
box logit in a candidate).  Scores are 0.3 + 0.001 i logits, every i once, so the order of the rows is stable;
at iou_thr 0.9 the NMS drops none of them on the 20-point head and 7 of 160 on the dense 80-point one (the counts
are asserted on the oracle).  Coefficients and prototypes are standard normal.  A bit may differ from the oracle only where |logit64| <= m S, m = 2 gamma_(nm + 1) (post_seg_oracle.margin:
the fp32 dot product bound, doubled for the MFMA's undocumented inner order); that share is capped at 0.1 % of the
in-crop pixels, on the oracle alone, before any device call (expected: about 1e-5)."""
import collections
import ctypes
import functools

import numpy as np
import pytest

import post_dfl_oracle as O
import post_seg_oracle as SO
import yolo_post

pytestmark = pytest.mark.gpu

SMALL = ((4, 4, 8.0), (2, 2, 16.0))  # 20 points, net 32 x 32: rows come from both scales' coefficient tensors
LARGE = ((8, 8, 4.0), (4, 4, 8.0))   # 80 points: more rows than one staged chunk of 128
MODES = {"any": ("any", "argmax"), "per_class": ("per_class", "argmax"), "multi": ("per_class", "multi")}
NET, CLASSES, REG, FILL = (32, 32), 4, 4, 0xA5A5A5A5

Case = collections.namedtuple("Case", "nm mask_hw rows mode max_masks scales cands", defaults=(None,))
CASES = [
    Case(16, (5, 33), 17, "any", 17, SMALL),          # a word with one valid bit; max_masks at the count
    Case(32, (8, 40), 16, "per_class", 20, SMALL),    # a word with half a tile; exactly one row tile; above
    Case(64, (3, 16), 40, "multi", 33, SMALL),        # one N tile only; three row tiles; below
    Case(32, (9, 64), 1, "per_class", 1, SMALL),      # exact words; one row
    Case(16, (9, 64), 0, "per_class", 4, SMALL),      # no row in the whole batch
    Case(64, (5, 33), 40, "multi", 40, SMALL),
    Case(32, (3, 16), 17, "any", 16, SMALL),          # below, at the tile boundary
    # two chunks of staged rows: 160 candidates on a dense grid, of which the oracle's NMS keeps 153
    Case(32, (8, 40), 153, "multi", 160, LARGE, 160),
]


@functools.lru_cache(maxsize=None)
def inputs(case):
    """(preds, coefs, proto): read-only fp32 arrays [3, ...]; image 0 has case.cands (default: case.rows) candidates."""
    rng = np.random.default_rng(case.nm * 1000 + (case.cands or case.rows))
    npts = sum(gh * gw for gh, gw, _ in case.scales)
    per = 2 if case.mode == "multi" else 1
    cands = case.rows if case.cands is None else case.cands
    assert cands % per == 0 and cands // per <= npts
    on_ids = iter(rng.permutation(1024))
    preds = [np.zeros((3, gh, gw, 4 * REG + CLASSES), np.float32) for gh, gw, _ in case.scales]
    pts = [(s, r, c) for s, (gh, gw, _) in enumerate(case.scales) for r in range(gh) for c in range(gw)]
    for b in range(3):
        on = set(rng.choice(npts, (cands // per, 0, 3)[b], replace=False).tolist())
        for k, (s, r, c) in enumerate(pts):
            q = preds[s][b, r, c]
            for side in range(4):  # two adjacent bins near the top, the others 3 to 6 below (post_dfl_cases._side)
                x = rng.uniform(-6.0, -3.0, REG)
                at = int(rng.integers(REG - 1))
                x[at], x[at + 1] = 0.0, rng.uniform(-2.0, 2.0)
                q[side * REG:(side + 1) * REG] = x
            q[4 * REG:] = rng.uniform(-8.0, -4.0, CLASSES)
            if k in on:
                for cl in rng.choice(CLASSES, per, replace=False):
                    q[4 * REG + cl] = 0.3 + 0.001 * next(on_ids)
                if b == 2:
                    q[REG + 1] = np.nan  # the top side of a candidate: a bad corner
    coefs = [rng.standard_normal((3, gh, gw, case.nm)).astype(np.float32) for gh, gw, _ in case.scales]
    proto = rng.standard_normal((3,) + case.mask_hw + (case.nm,)).astype(np.float32)
    for a in preds + coefs + [proto]:
        a.setflags(write=False)
    return tuple(preds), tuple(coefs), proto


def device_head(case):
    return yolo_post.DflHead(case.scales, CLASSES, REG, 0.25, 0.9, *MODES[case.mode], mask_dim=case.nm)


@functools.lru_cache(maxsize=None)
def want(case):
    """Image 0 by the oracle: (rows, per row k < min(rows, max_masks) its (logit64, S))."""
    preds, coefs, proto = inputs(case)
    head = O.Dfl(case.scales, CLASSES, REG, 0.25, 0.9)
    nms, labels = MODES[case.mode]
    rows, points = SO.rows_points([p[0] for p in preds], head, nms, labels)
    assert len(rows) == case.rows, (case, len(rows))
    assert O.detect_or_code([p[1] for p in preds], head, nms, labels) == []
    assert O.detect_or_code([p[2] for p in preds], head, nms, labels) == -1
    n = min(len(rows), case.max_masks)
    return rows, [SO.logits([c[0] for c in coefs], proto[0], head, points[k]) for k in range(n)]


def host_call(case, preds, coefs, proto, max_det):
    """dnn_yolo_postprocess_dfl_seg_host on mask words prefilled with FILL -> (rows, counts, words)."""
    head, n = device_head(case), len(proto)
    spec = head.seg(case.mask_hw, NET, case.max_masks)
    dets, counts = np.zeros((n, max_det), yolo_post.DETECTION_DTYPE), np.zeros(n, np.int32)
    words = np.full((n, spec.max_masks, spec.mask_h, spec.w32), FILL, np.uint32)
    ps, cs = [np.ascontiguousarray(p) for p in preds], [np.ascontiguousarray(c) for c in coefs]
    pp = (ctypes.c_void_p * len(ps))(*[p.ctypes.data for p in ps])
    cp = (ctypes.c_void_p * len(cs))(*[c.ctypes.data for c in cs])
    rc = yolo_post._lib.dnn_yolo_postprocess_dfl_seg_host(
        ctypes.byref(head.c), ctypes.byref(spec.c), pp, cp, np.ascontiguousarray(proto).ctypes.data, n,
        dets.ctypes.data, max_det, counts.ctypes.data, words.ctypes.data, yolo_post.NMS_MODES[head.nms],
        yolo_post.LABEL_MODES[head.labels])
    assert rc == 0, yolo_post.dnn_hip.last_error()
    return yolo_post._rows(dets, counts, max_det, raise_errors=False), counts, words


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"nm{c.nm}-{c.mask_hw[0]}x{c.mask_hw[1]}-{c.rows}rows-{c.mode}")
def test_masks_match_the_oracle(case):
    preds, coefs, proto = inputs(case)
    ref_rows, ref = want(case)
    m, n = SO.margin(case.nm), len(ref)
    crops = [SO.crop(r[1:5], case.mask_hw, NET) for r in ref_rows[:n]]
    unsure = sum(int((np.abs(lg) <= m * s)[cr].sum()) for (lg, s), cr in zip(ref, crops))
    inside = sum(int(cr.sum()) for cr in crops)
    print(f"{case}: {n} masks, {inside} in-crop pixels, {unsure} within the margin")
    assert unsure <= 1e-3 * inside  # on the oracle alone, before any device call

    head = device_head(case)
    rows, counts, words = host_call(case, preds, coefs, proto, head.max_det)
    assert rows == yolo_post.detect_batch_multi(preds, head, raise_errors=False)
    assert list(counts) == [case.rows, 0, -1]
    assert (words[0, n:] == FILL).all() and (words[1:] == FILL).all()  # rows beyond the masks, and the other images
    assert [r[0] for r in rows[0]] == [r[0] for r in ref_rows], "the oracle's rows are other rows"
    assert np.allclose([r[5] for r in rows[0]], [r[5] for r in ref_rows], rtol=0, atol=1e-6)

    spec = head.seg(case.mask_hw, NET, case.max_masks)
    pad = np.unpackbits(words[0, :n].view(np.uint8), axis=2, bitorder="little")[:, :, spec.mask_w:]
    assert not pad.any(), "a padding bit is set"
    got = spec.unpack(words[0], n)
    wrong = 0
    for k, (lg, s) in enumerate(ref):
        cr = SO.crop(rows[0][k][1:5], case.mask_hw, NET)  # the row's own corners
        assert not got[k][~cr].any(), f"row {k}: a bit outside the crop"
        wrong += int(((got[k] != (lg > 0)) & cr & (np.abs(lg) > m * s)).sum())
    assert wrong == 0

    if case.rows == 17 or case.scales is LARGE:  # an image's words do not depend on its batch; the device form gives the host's
        _, c1, w1 = host_call(case, [p[:1] for p in preds], [c[:1] for c in coefs], proto[:1], head.max_det)
        assert list(c1) == [case.rows] and np.array_equal(w1[0], words[0])
        r2, masks = yolo_post.detect_batch_masks(preds, coefs, proto, head, spec, raise_errors=False)
        assert r2 == rows and [len(x) for x in masks] == [n, 0, 0] and np.array_equal(masks[0], got)
        import torch
        dev = torch.device("cuda", 0)
        bufs = yolo_post.MaskDetectionBuffers(3, dev, head, spec)
        bufs.masks.fill_(FILL - (1 << 32))
        xs = [[torch.from_numpy(np.array(a)).to(dev) for a in group] for group in (preds, coefs, [proto])]
        for _ in range(2):  # twice on the same buffers
            bufs.run([x.data_ptr() for x in xs[0]], [x.data_ptr() for x in xs[1]], xs[2][0].data_ptr(), 3,
                     torch.cuda.current_stream(dev).cuda_stream)
        torch.cuda.synchronize()
        assert np.array_equal(bufs.masks.cpu().numpy().view(np.uint32), words)
        assert bufs.to_rows(bufs.dets.cpu().numpy(), bufs.counts.cpu().numpy(), head.max_det, False) == rows
        assert np.array_equal(bufs.masks_to_host(3)[0], got)
