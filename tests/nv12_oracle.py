"""TEST INFRASTRUCTURE ONLY — the NV12 conversion of include/dnn_hip_ingest.h restated in numpy
(int32, exactly the header's table); the letterbox after it is tests/letterbox_oracle.py's."""
import numpy as np

# matrix -> (y0, cy, rv, gu, gv, bu): C = cy (Y - y0), R = C + rv E, G = C - gu D - gv E, B = C + bu D
MATRICES = {"bt601_limited": (16, 298, 409, 100, 208, 516), "bt709_limited": (16, 298, 459, 55, 136, 541),
            "bt601_full": (0, 256, 359, 88, 183, 454)}


def nv12_to_rgb(y, uv, matrix="bt601_limited"):
    """y uint8 [H, W], uv uint8 [(H + 1) // 2, (W + 1) // 2, 2] -> uint8 RGB [H, W, 3]; chroma of
    pixel (r, c) is uv[r >> 1][c >> 1], no interpolation."""
    y0, cy, rv, gu, gv, bu = MATRICES[matrix]
    h, w = y.shape
    assert y.dtype == np.uint8 and uv.dtype == np.uint8 and uv.shape == ((h + 1) // 2, (w + 1) // 2, 2)
    up = uv.astype(np.int32).repeat(2, axis=0).repeat(2, axis=1)[:h, :w]
    c, d, e = cy * (y.astype(np.int32) - y0), up[:, :, 0] - 128, up[:, :, 1] - 128
    rgb = np.stack([c + rv * e + 128, c - gu * d - gv * e + 128, c + bu * d + 128], axis=2) >> 8
    return np.clip(rgb, 0, 255).astype(np.uint8)


def frame(h, w, seed=0):
    """A seeded (y, uv) pair of full-range random bytes."""
    rng = np.random.default_rng([h, w, seed, 12])
    return (rng.integers(0, 256, (h, w), dtype=np.uint8),
            rng.integers(0, 256, ((h + 1) // 2, (w + 1) // 2, 2), dtype=np.uint8))


def surface(y, uv, pitch=None, gap_rows=0, offset=0, fill=0xAB):
    """The pair as one pitched surface: (uint8 buffer, (y_offset, uv_offset, h, w, pitch)), the UV
    plane `gap_rows` pitches after the Y plane's end, everything else `fill`."""
    h, w = y.shape
    pitch = pitch or 2 * ((w + 1) // 2)
    uv_at = offset + (h + gap_rows) * pitch
    buf = np.full(uv_at + uv.shape[0] * pitch, fill, np.uint8)
    for r in range(h):
        buf[offset + r * pitch:offset + r * pitch + w] = y[r]
    for r in range(uv.shape[0]):
        buf[uv_at + r * pitch:uv_at + r * pitch + uv.shape[1] * 2] = uv[r].reshape(-1)
    return buf, (offset, uv_at, h, w, pitch)
