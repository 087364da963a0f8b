"""TEST INFRASTRUCTURE ONLY: the activations in float64, an fp32-ulp error count, and darknet_oracle's float64
Darknet forward with `activation = mish | swish | logistic` on [convolutional] and [shortcut]."""
import numpy as np

import darknet_oracle as DO

FLT_MIN = float(np.finfo(np.float32).tiny)


def act64(kind, v):
    v = np.asarray(v, np.float64)
    if kind == "mish":
        return v * np.tanh(np.logaddexp(0.0, v))  # ln(1 + e^v) without overflow
    e = np.exp(-np.abs(v))
    sig = np.where(v >= 0, 1, e) / (1 + e)
    return {"logistic": sig, "swish": v * sig, "leaky": np.where(v > 0, v, DO.LEAKY_SLOPE * v), "linear": v}[kind]


def ulp_err(got, ref64):
    """|got - ref| in fp32 spacings at ref, the unit never below FLT_MIN (a result flushed to zero where
    |ref| < FLT_MIN counts as under one)."""
    at = np.minimum(np.abs(ref64), 1.7e38).astype(np.float32)  # (the top binade counts in the one below: no inf spacing)
    return np.abs(np.asarray(got, np.float64) - ref64) / np.maximum(np.spacing(at).astype(np.float64), FLT_MIN)


def forward(sections, layers, x):
    """The tensors the [yolo] sections read, in cfg order, fp32: each layer in float64, rounded once.
    (For cfg_text's definitions: every conv has pad=1, every upsample stride 2.)"""
    outs, heads, weights = [], [], iter(layers)
    cur = np.asarray(x, np.float32)
    for at, sec in enumerate(sections[1:]):
        kind = sec["type"]
        ref = lambda v: outs[at + int(v) if int(v) < 0 else int(v)]  # noqa: E731
        if kind == "convolutional":
            layer, pad = next(weights), int(sec["size"]) // 2
            scale, shift = DO.fold(layer)
            y = DO.conv_padded(cur, np.einsum("nchw->hwcn", layer["weights"]), int(sec["stride"]), pad, pad)
            cur = act64(sec["activation"], y.astype(np.float64) * scale + shift).astype(np.float32)
        elif kind == "shortcut":
            cur = act64(sec["activation"], cur.astype(np.float64) + ref(sec["from"])).astype(np.float32)
        elif kind == "route":
            cur = np.concatenate([ref(v) for v in sec["layers"].split(",")], axis=3)
        elif kind == "upsample":
            cur = cur.repeat(2, axis=1).repeat(2, axis=2)
        elif kind == "maxpool":
            cur = DO.maxpool_layer(cur, sec)
        else:  # yolo: the conv before it is a head
            heads.append(cur)
        outs.append(cur)
    return heads
