"""TEST INFRASTRUCTURE ONLY — the letterbox ingest and the box correction
(include/dnn_hip_ingest.h: dnn_letterbox_frames; include/dnn_hip_post.h:
dnn_yolo_correct_detections) restated in numpy.

The arithmetic is the original Darknet's letterbox_image / resize_image / load_image scaling and
draw_detections' clamp as the headers state them; Darknet itself is not readable here, so this
restatement is the yardstick and parity with a Darknet binary is unpinned.

  geometry       the size rule: two fp32 quotients compared, integer divisions
  letterbox_f32  every operation in np.float32, rounded on its own; two passes with a `part` image,
                 as Darknet does it (the kernel forms the two part values it needs per output)
  letterbox_f64  the same sampling positions in float64 WITHOUT the last-row rule: a sanity bound
  correct_rows   the box mapping in Python ints
"""
import numpy as np

F = np.float32


def geometry(src_h, src_w, net_h, net_w):
    """(new_h, new_w, pad_y, pad_x), or None where a new side is below 2 (the refusal)."""
    if F(net_w) / F(src_w) < F(net_h) / F(src_h):
        new_w, new_h = net_w, (src_h * net_w) // src_w
    else:
        new_h, new_w = net_h, (src_w * net_h) // src_h
    if new_w < 2 or new_h < 2:
        return None
    assert new_w <= net_w and new_h <= net_h
    return new_h, new_w, (net_h - new_h) // 2, (net_w - new_w) // 2


def scaled(im, order):
    """load_image's scaling, (float)((double)byte / 255.0), in RGB order: fp32 [H, W, 3]."""
    assert im.dtype == np.uint8 and im.ndim == 3 and im.shape[2] == 3 and order in ("bgr", "rgb")
    s = (im.astype(np.float64) / 255.0).astype(F)
    return s[:, :, ::-1] if order == "bgr" else s


def _positions(src, new):
    """Per new index: (i, d) = ((int)s, s - i) with s = (float)k * scale, scale = (src-1)/(new-1) in fp32."""
    scale = F(src - 1) / F(new - 1)
    s = np.arange(new, dtype=F) * scale
    assert s.dtype == F
    i = s.astype(np.int64)
    return i, s - i.astype(F)


def resize_f32(S, h, w):
    """Darknet's resize_image on fp32 S [H, W, 3] -> [h, w, 3], every fp32 operation on its own."""
    H, W = S.shape[:2]
    one = F(1)
    part = np.empty((H, w, 3), F)
    ix, dx = _positions(W, w)
    for c in range(w):
        if c == w - 1 or W == 1:
            part[:, c] = S[:, W - 1]
        else:
            part[:, c] = (one - dx[c]) * S[:, ix[c]] + dx[c] * S[:, ix[c] + 1]
    out = np.empty((h, w, 3), F)
    iy, dy = _positions(H, h)
    for r in range(h):
        out[r] = (one - dy[r]) * part[iy[r]]
        if not (r == h - 1 or H == 1):
            out[r] = out[r] + dy[r] * part[iy[r] + 1]
    assert part.dtype == F and out.dtype == F
    return out


def letterbox_f32(im, net_h, net_w, order="bgr"):
    """uint8 [H, W, 3] -> fp32 [net_h, net_w, 3]: the resized image in a 0.5 canvas."""
    new_h, new_w, pad_y, pad_x = geometry(im.shape[0], im.shape[1], net_h, net_w)
    out = np.full((net_h, net_w, 3), F(0.5), F)
    out[pad_y:pad_y + new_h, pad_x:pad_x + new_w] = resize_f32(scaled(im, order), new_h, new_w)
    return out


def letterbox_f64(im, net_h, net_w, order="bgr"):
    """The same sampling positions (the fp32 ones, so both sample the same source pixels) combined
    in float64, the second row always added where it exists: float64 [net_h, net_w, 3]."""
    new_h, new_w, pad_y, pad_x = geometry(im.shape[0], im.shape[1], net_h, net_w)
    H, W = im.shape[:2]
    S = im.astype(np.float64) / 255.0
    S = S[:, :, ::-1] if order == "bgr" else S
    ix, dx = _positions(W, new_w)
    iy, dy = _positions(H, new_h)
    dx, dy = dx.astype(np.float64)[None, :, None], dy.astype(np.float64)[:, None, None]
    ix1, iy1 = np.minimum(ix + 1, W - 1), np.minimum(iy + 1, H - 1)
    part = (1 - dx) * S[:, ix] + dx * S[:, ix1]
    part[:, new_w - 1] = S[:, W - 1]
    res = (1 - dy) * part[iy] + dy * part[iy1]
    out = np.full((net_h, net_w, 3), 0.5, np.float64)
    out[pad_y:pad_y + new_h, pad_x:pad_x + new_w] = res
    return out


def _axis(v, pad, new, src):
    v = min(max(int(v), pad), pad + new)
    return min(((v - pad) * src) // new, src - 1)


def correct_row(row, size, net_hw):
    """One (class, left, top, right, bottom, score) row from network pixels into the size = (h, w) image's."""
    new_h, new_w, pad_y, pad_x = geometry(size[0], size[1], net_hw[0], net_hw[1])
    c, l, t, r, b, s = row
    return (c, _axis(l, pad_x, new_w, size[1]), _axis(t, pad_y, new_h, size[0]), _axis(r, pad_x, new_w, size[1]),
            _axis(b, pad_y, new_h, size[0]), s)


def correct_rows(rows, sizes, net_hw):
    """Per image: its rows corrected, or its negative error code as it is."""
    return [r if isinstance(r, (int, np.integer)) else [correct_row(x, sz, net_hw) for x in r]
            for r, sz in zip(rows, sizes)]


def correct_dets(dets, counts, sizes, net_hw):
    """correct_rows on the device layout: a copy of the structured `dets` [n, max_det] with rows
    [0, min(counts[i], max_det)) of every image with a non-negative count rewritten."""
    out = dets.copy()
    for i, (cnt, sz) in enumerate(zip(counts, sizes)):
        for j in range(max(min(int(cnt), dets.shape[1]), 0)):
            d = out[i, j]
            _, l, t, r, b, _ = correct_row((0, d["left"], d["top"], d["right"], d["bottom"], 0), sz, net_hw)
            d["left"], d["top"], d["right"], d["bottom"] = l, t, r, b
    return out
