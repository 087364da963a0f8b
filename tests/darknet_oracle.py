"""TEST INFRASTRUCTURE ONLY: a float64 numpy restatement of the Darknet forward for the section
types darknet_import handles, working from the parsed cfg and the raw Darknet-order arrays of a
weight file.  It shares nothing with darknet_import but parse_cfg's output format: padding, BN
fold, route / shortcut indexing and the max pool's window placement are restated here from
Darknet's definitions.

Per layer the accumulation and the element-wise steps run in float64 and the layer's output is
rounded once to fp32 (what the next layer reads, as on the device).  The BatchNorm fold is the
one the importer documents: alpha = scales / (sqrt(rolling_variance) + 1e-6), shift = biases -
rolling_mean * alpha in float64, each rounded once to fp32, y = conv * alpha + shift."""
import numpy as np

import ref_numpy as R

LEAKY_SLOPE = float(np.float32(0.1))  # Darknet's .1f


def fold(layer):
    beta = np.asarray(layer["biases"], np.float64)
    if "scales" not in layer:
        return np.ones_like(beta), beta.astype(np.float32).astype(np.float64)
    alpha = np.asarray(layer["scales"], np.float64) / (np.sqrt(np.asarray(layer["rolling_variance"], np.float64)) + 1e-6)
    shift = beta - np.asarray(layer["rolling_mean"], np.float64) * alpha
    return alpha.astype(np.float32).astype(np.float64), shift.astype(np.float32).astype(np.float64)


def affine_leaky(v, scale, shift, leaky):
    """leaky(v * scale + shift) in float64 on fp32 inputs, rounded once to fp32."""
    y = np.asarray(v, np.float64)
    if scale is not None:
        y = y * np.asarray(scale, np.float64) + np.asarray(shift, np.float64)
    if leaky:
        y = np.where(y > 0, y, LEAKY_SLOPE * y)
    return y.astype(np.float32)


def conv_padded(x, kernel_hwio, stride, pad_h, pad_w):
    """Zero padding by np.pad on every side, then ref_numpy's VALID conv in float64."""
    xp = np.pad(np.asarray(x, np.float32), [(0, 0), (pad_h, pad_h), (pad_w, pad_w), (0, 0)], "constant")
    return R.conv2d(xp, kernel_hwio, strides=(1, stride, stride, 1), padding="VALID", acc=np.float64)


def conv_layer(x, sec, layer):
    size, stride = int(sec.get("size", 1)), int(sec.get("stride", 1))
    pad = size // 2 if int(sec.get("pad", 0)) else int(sec.get("padding", 0))
    w = np.asarray(layer["weights"], np.float32)            # [n][c][kh][kw]
    kernel = np.einsum("nchw->hwcn", w)                     # HWIO, by index names rather than axis numbers
    scale, shift = fold(layer)
    return affine_leaky(conv_padded(x, kernel, stride, pad, pad), scale, shift, sec["activation"] == "leaky")


def maxpool_layer(x, sec):
    """Darknet's maxpool: padding = size - 1, out = (in + padding - size) / stride + 1, window of
    output o over input rows o * stride - padding / 2 + [0, size), cells outside the map skipped."""
    stride = int(sec.get("stride", 1))
    size = int(sec.get("size", stride))
    padding = int(sec.get("padding", size - 1))
    n, h, w, c = x.shape
    oh, ow = (h + padding - size) // stride + 1, (w + padding - size) // stride + 1
    off = -(padding // 2)
    out = np.full((n, oh, ow, c), -np.inf, np.float32)
    for i in range(oh):
        for j in range(ow):
            y0, x0 = max(i * stride + off, 0), max(j * stride + off, 0)
            y1, x1 = min(i * stride + off + size, h), min(j * stride + off + size, w)
            out[:, i, j, :] = x[:, y0:y1, x0:x1, :].max(axis=(1, 2))
    return out


def forward(sections, layers, x):
    """The tensors the [yolo] sections read (the conv before each), in cfg order, fp32."""
    outs, heads = [], []
    weights = iter(layers)
    cur = np.asarray(x, np.float32)
    for at, sec in enumerate(sections[1:]):
        kind = sec["type"]

        def ref(v):
            v = int(v)
            return outs[at + v if v < 0 else v]

        if kind == "convolutional":
            cur = conv_layer(cur, sec, next(weights))
        elif kind == "shortcut":
            cur = (cur.astype(np.float64) + ref(sec["from"]).astype(np.float64)).astype(np.float32)
        elif kind == "route":
            cur = np.concatenate([ref(v) for v in sec["layers"].split(",")], axis=3)
        elif kind == "upsample":
            f = int(sec.get("stride", 2))
            cur = cur.repeat(f, axis=1).repeat(f, axis=2)
        elif kind == "maxpool":
            cur = maxpool_layer(cur, sec)
        elif kind == "yolo":
            heads.append(cur)
        else:
            raise ValueError(f"section [{kind}]")
        outs.append(cur)
    return heads
