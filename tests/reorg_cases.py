"""Shared by tests/test_reorg_cpu.py and tests/test_gpu_reorg.py: Darknet's reorg as the triple loop
of its definition (include/dnn_hip_plan.h, dnn_plan_add_reorg; not derived from the kernel's index
arithmetic), the narrow YOLOv2 models, and a float64 forward that walks [reorg] and [region] and
takes every other section from tests/darknet_oracle.py."""
import numpy as np

import darknet_import as D
import darknet_oracle as DO

# (model, width_div, input size): 96 / 32 = a 3 x 3 grid, so the passthrough's reorg reads a 6 x 6 x 8 map
NARROW = {"yolov2": (8, 96), "yolov2_tiny": (4, 96)}
CLASSES = 3  # 5 x (5 + 3) = 40 head outputs

# (H, W, C, stride, Cb, b_first, batch): the smallest shapes at which each piece of the kernel can go wrong
KERNEL_CASES = [
    (2, 2, 4, 2, 0, 0, 1),        # out_c = 1
    (4, 6, 8, 2, 0, 0, 1),        # H != W: swapped extents
    (6, 4, 12, 2, 5, 0, 1),       # the scalar width: 48 + 5 output channels
    (6, 4, 12, 2, 5, 1, 3),       # ... b first, a batch
    (6, 9, 9, 3, 0, 0, 2),        # stride 3
    (8, 8, 16, 2, 8, 0, 1),       # the 16-byte width
    (8, 8, 16, 2, 8, 1, 3),       # ... b first, a batch
    (5, 7, 12, 1, 20, 0, 2),      # stride 1 with a concat: a plain copy
    (26, 26, 64, 2, 1024, 0, 1),  # YOLOv2's own layer
    (26, 26, 64, 2, 1024, 1, 9),  # ... two batch slices, the second shorter
]


def reorg_loops(a, s):
    """Darknet's reorg forward of an NHWC array: the definition's loop over the input dimensions builds
    the flat CHW index map once, every image is moved through it."""
    n, h, w, c = a.shape
    out_c = c // (s * s)
    src = np.full(c * h * w, -1, np.int64)
    for k in range(c):
        for j in range(h):
            for i in range(w):
                c2, off = k % out_c, k // out_c
                w2, h2 = i * s + off % s, j * s + off // s
                src[i + w * (j + h * k)] = w2 + w * s * (h2 + h * s * c2)
    out_flat = a.transpose(0, 3, 1, 2).reshape(n, -1)[:, src]  # in_flat is [c][h][w]
    return np.ascontiguousarray(out_flat.reshape(n, c * s * s, h // s, w // s).transpose(0, 2, 3, 1))


def arange_inputs(n, h, w, ca, stride, cb):
    """a and b (None without cb) with values unique per element, exact in fp32."""
    na, nb = n * h * w * ca, n * (h // stride) * (w // stride) * cb
    assert na + nb < 1 << 24
    a = np.arange(na, dtype=np.float32).reshape(n, h, w, ca)
    return a, (na + np.arange(nb, dtype=np.float32)).reshape(n, h // stride, w // stride, cb) if cb else None


def parse(text):
    return D.parse_cfg(text, D.ACTIVATIONS, D.SECTION_TYPES)


def narrow_cfg(model):
    div, size = NARROW[model]
    return D.cfg_text(model, classes=CLASSES, width=size, height=size, width_div=div)


def forward(sections, layers, x):
    """The tensor the [region] section reads, fp32: darknet_oracle's layers plus [reorg]."""
    outs, weights, cur = [], iter(layers), np.asarray(x, np.float32)
    for at, sec in enumerate(sections[1:]):
        kind = sec["type"]
        if kind == "convolutional":
            cur = DO.conv_layer(cur, sec, next(weights))
        elif kind == "maxpool":
            cur = DO.maxpool_layer(cur, sec)
        elif kind == "route":
            cur = np.concatenate([outs[at + int(v)] for v in sec["layers"].split(",")], axis=3)
        elif kind == "reorg":
            cur = reorg_loops(cur, int(sec.get("stride", 1)))
        elif kind != "region":
            raise ValueError(f"section [{kind}]")
        outs.append(cur)
    return cur
