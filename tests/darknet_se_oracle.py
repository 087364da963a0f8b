"""TEST INFRASTRUCTURE ONLY: a float64 Darknet forward for the MBConv classifiers: [convolutional] with groups and any
activation (torch's float64 conv2d), [shortcut], [avgpool], [scale_channels] and [softmax], every layer's output
rounded once to fp32.  The BatchNorm fold and the activations are darknet_oracle's and act_oracle's, imported."""
import numpy as np
import torch
import torch.nn.functional as F

import darknet_oracle as DO
from act_oracle import act64

f8 = np.float64


def seeded_layers(shapes, seed):
    """load_weights' dicts for weight_shapes' tuples: weights N(0, 1 / fan_in) times 1.5, biases N(0, 0.25), and under
    BatchNorm scales in +-[0.5, 1.5), means N(0, 0.25), variances in [0.5, 1.5)."""
    rng = np.random.default_rng(seed)
    out = []
    for _, n, c, size, bn in shapes:
        layer = {"biases": (0.5 * rng.standard_normal(n)).astype(np.float32),
                 "weights": (1.5 * rng.standard_normal((n, c, size, size)) / np.sqrt(c * size * size)).astype(np.float32)}
        if bn:
            layer.update(scales=(rng.uniform(0.5, 1.5, n) * np.where(np.arange(n) % 3, 1, -1)).astype(np.float32),
                         rolling_mean=(0.5 * rng.standard_normal(n)).astype(np.float32),
                         rolling_variance=rng.uniform(0.5, 1.5, n).astype(np.float32))
        out.append(layer)
    return out


def forward(sections, layers, x):
    outs, weights = [], iter(layers)
    cur = np.asarray(x, np.float32)
    for at, sec in enumerate(sections[1:]):
        kind = sec["type"]
        if kind == "convolutional":
            layer, size = next(weights), int(sec.get("size", 1))
            pad = size // 2 if int(sec.get("pad", 0)) else int(sec.get("padding", 0))
            v = F.conv2d(torch.from_numpy(cur).double().permute(0, 3, 1, 2), torch.from_numpy(layer["weights"]).double(),
                         stride=int(sec.get("stride", 1)), padding=pad, groups=int(sec.get("groups", 1)))
            scale, shift = DO.fold(layer)
            cur = act64(sec["activation"], v.permute(0, 2, 3, 1).numpy() * scale + shift).astype(np.float32)
        elif kind == "shortcut":
            cur = (cur.astype(f8) + outs[at + int(sec["from"])].astype(f8)).astype(np.float32)
        elif kind == "avgpool":
            cur = cur.astype(f8).mean((1, 2), keepdims=True).astype(np.float32)
        elif kind == "scale_channels":
            cur = (outs[at + int(sec["from"])].astype(f8) * cur.astype(f8)).astype(np.float32)
        elif kind == "softmax":
            e = np.exp(cur.astype(f8) - cur.astype(f8).max(3, keepdims=True))
            cur = (e / e.sum(3, keepdims=True)).astype(np.float32)
        else:
            raise ValueError(f"section [{kind}]")
        outs.append(cur)
    return cur
