"""Portable, bit-reproducible synthetic weights and frames for YOLOv2-tiny.

The reference's weights pickle (`proj3/yolov2tiny.py:15-23`, `../y2t_weights.pickle`)
is not in the reference repo, so every test and benchmark runs on synthetic data
(SURVEY.md §8d).  The generator uses only exact integer arithmetic plus correctly
rounded IEEE operations (add, multiply, sqrt), so the same bytes come out on any
machine and any numpy version: the GPU box regenerates the 63.5 MB of weights
that the golden fixtures were computed from without shipping them.

Generator spec (also written into tests/golden/spec.json):
  * stream key   k = mix64(seed * 0x100000001B3 + stream_id)
  * raw draw  x[i] = mix64(k + (i + 1) * 0x9E3779B97F4A7C15)   (splitmix64 finaliser)
  * uniform   u[i] = (x[i] >> 40) * 2**-24                       (exact in fp32)
  * approx-normal  n[i] = (u[4i] + u[4i+1] + u[4i+2] + u[4i+3] - 2) * sqrt(3)
                                                                  (Irwin-Hall, mean 0, var 1)
Layer parameters (stream ids 10*L + j):
  kernel  HWIO  n * sqrt(2 / (kh*kw*ic))      (He-normal-like)
  biases        n * 0.1
  mean          n * 0.1
  variance      0.5 + u
  gamma         0.5 + u
Frames: uniform [0, 1) NHWC 416x416x3, seed 1 + frame index, stream 0.
"""
import numpy as np

GOLDEN = np.uint64(0x9E3779B97F4A7C15)
M1 = np.uint64(0xBF58476D1CE4E5B9)
M2 = np.uint64(0x94D049BB133111EB)

# tiny-yolo-voc channel plan; the final 125 is pinned by
# proj3/yolov2tiny.py:120 (13x13x5x25), the rest is the standard VOC plan.
CHANNELS = (16, 32, 64, 128, 256, 512, 1024, 1024, 125)
IN_SHAPE = (416, 416, 3)
WEIGHT_SEED = 0


def _mix64(z):
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * M1
        z = (z ^ (z >> np.uint64(27))) * M2
        z = z ^ (z >> np.uint64(31))
    return z


def _key(seed, stream):
    with np.errstate(over="ignore"):
        return _mix64(np.uint64(seed) * np.uint64(0x100000001B3) + np.uint64(stream))


def uniform(seed, stream, n, chunk=1 << 23):
    """n uniform draws in [0, 1) as float64 (each exactly representable in fp32)."""
    key = _key(seed, stream)
    out = np.empty(n, dtype=np.float64)
    for s in range(0, n, chunk):
        e = min(n, s + chunk)
        idx = np.arange(s + 1, e + 1, dtype=np.uint64)
        with np.errstate(over="ignore"):
            x = _mix64(key + idx * GOLDEN)
        out[s:e] = (x >> np.uint64(40)).astype(np.float64) * (2.0 ** -24)
    return out


def normal(seed, stream, n):
    u = uniform(seed, stream, 4 * n).reshape(n, 4)
    # left-to-right adds of 24-bit fractions are exact in float64
    s = ((u[:, 0] + u[:, 1]) + u[:, 2]) + u[:, 3]
    return (s - 2.0) * np.sqrt(3.0)


def layer_weights(layer, ic, od, k=3, seed=WEIGHT_SEED, bn=True):
    """One conv layer's parameters in the pickle's dict format
    (`proj3/yolov2tiny.py:30-77`: kernel HWIO, biases, moving_mean,
    moving_variance, gamma), fp32."""
    base = 10 * layer
    fan_in = k * k * ic
    w = {
        "kernel": (normal(seed, base + 0, k * k * ic * od) * np.sqrt(2.0 / fan_in))
        .astype(np.float32).reshape(k, k, ic, od),
        "biases": (normal(seed, base + 1, od) * 0.1).astype(np.float32),
    }
    if bn:
        w["moving_mean"] = (normal(seed, base + 2, od) * 0.1).astype(np.float32)
        w["moving_variance"] = (0.5 + uniform(seed, base + 3, od)).astype(np.float32)
        w["gamma"] = (0.5 + uniform(seed, base + 4, od)).astype(np.float32)
    return w


def yolo_weights(seed=WEIGHT_SEED, channels=CHANNELS, in_c=IN_SHAPE[2]):
    """The 9-entry weight list `build_graph` consumes (`proj3/yolov2tiny.py:26`)."""
    ws = []
    ic = in_c
    for i, od in enumerate(channels):
        last = i == len(channels) - 1
        ws.append(layer_weights(i, ic, od, k=1 if last else 3, seed=seed, bn=not last))
        ic = od
    return ws


# full YOLOv2 (yolov2.py): (output channels, kernel size) of the 23 convs in the order yolov2.YOLO_V2
# consumes them: Darknet-19's 18 trunk convs, conv19 / conv20, the 1x1 passthrough conv on the
# 512-channel activation, the 3x3 conv after the concat and the linear 1x1 head
YOLOV2_TRUNK = ((32, 3), (64, 3), (128, 3), (64, 1), (128, 3), (256, 3), (128, 1), (256, 3), (512, 3), (256, 1),
                (512, 3), (256, 1), (512, 3), (1024, 3), (512, 1), (1024, 3), (512, 1), (1024, 3))
YOLOV2_TAIL = ((1024, 3), (1024, 3))
YOLOV2_PASSTHROUGH = (64, 1)
YOLOV2_PASSTHROUGH_FROM = 12  # the passthrough reads trunk conv 12's output (26 x 26 x 512 at 416)
YOLOV2_JOINED = (1024, 3)
YOLOV2_N_OUT = 425            # 5 anchors x (5 + 80 COCO classes)


def yolov2_weights(seed=WEIGHT_SEED, width_div=1, n_out=YOLOV2_N_OUT, in_c=IN_SHAPE[2]):
    """The 23-entry weight list yolov2.YOLO_V2 consumes, from the same counter-based generators
    (layer i draws from streams 10 i + j).  width_div divides every channel count except the
    input's and the head's n_out (a narrow model of the same topology for tests)."""
    def wd(c):
        if c % width_div:
            raise ValueError(f"width_div {width_div} does not divide {c}")
        return c // width_div

    ws = []
    ic = in_c
    for od, k in YOLOV2_TRUNK + YOLOV2_TAIL:
        ws.append(layer_weights(len(ws), ic, wd(od), k=k, seed=seed))
        ic = wd(od)
    pt_in = wd(YOLOV2_TRUNK[YOLOV2_PASSTHROUGH_FROM][0])
    ws.append(layer_weights(len(ws), pt_in, wd(YOLOV2_PASSTHROUGH[0]), k=YOLOV2_PASSTHROUGH[1], seed=seed))
    ic = 4 * wd(YOLOV2_PASSTHROUGH[0]) + ic
    ws.append(layer_weights(len(ws), ic, wd(YOLOV2_JOINED[0]), k=YOLOV2_JOINED[1], seed=seed))
    ws.append(layer_weights(len(ws), wd(YOLOV2_JOINED[0]), n_out, k=1, seed=seed, bn=False))
    return ws


# Darknet-53 + YOLOv3's stride-32 branch (darknet53.py): the stem, then per stage (width, residual
# blocks): a 3x3 stride-2 conv to `width`, then blocks of 1x1 x width/2, 3x3 x width and a shortcut;
# then the branch's (width, kernel) convs and a linear 1x1 head
DARKNET53_STEM = 32
DARKNET53_STAGES = ((64, 1), (128, 2), (256, 8), (512, 8), (1024, 4))
DARKNET53_BRANCH = ((512, 1), (1024, 3), (512, 1), (1024, 3), (512, 1), (1024, 3))
DARKNET53_RESIDUAL_GAIN = 0.25  # gamma of each block's second conv: x + f(x) grows by 1 + gain^2 in variance


def darknet53_weights(seed=WEIGHT_SEED, width_div=1, n_out=YOLOV2_N_OUT, in_c=IN_SHAPE[2]):
    """The 59-entry weight list darknet53.DARKNET53 consumes (52 trunk convs, the stride-32
    branch's 6 convs and its linear head), from the same counter-based generators as
    yolov2_weights (layer i draws from streams 10 i + j) with the same width_div.  He-scaled
    kernels keep a conv chain at O(1); a residual sum x + f(x) would double the variance per
    block, so the gamma of each block's second conv is scaled by DARKNET53_RESIDUAL_GAIN (23 blocks
    then grow the variance by 1.0625^23, about 4).  n_out defaults to a YOLOv2-format head (5
    anchors x 85), which yolo_post decodes; YOLOv3's own layer 81 has 255 outputs."""
    def wd(c):
        if c % width_div:
            raise ValueError(f"width_div {width_div} does not divide {c}")
        return c // width_div

    ws = [layer_weights(0, in_c, wd(DARKNET53_STEM), k=3, seed=seed)]
    ic = wd(DARKNET53_STEM)
    for width, blocks in DARKNET53_STAGES:
        ws.append(layer_weights(len(ws), ic, wd(width), k=3, seed=seed))
        ic = wd(width)
        for _ in range(blocks):
            ws.append(layer_weights(len(ws), ic, wd(width // 2), k=1, seed=seed))
            w = layer_weights(len(ws), wd(width // 2), ic, k=3, seed=seed)
            w["gamma"] = (w["gamma"] * np.float32(DARKNET53_RESIDUAL_GAIN)).astype(np.float32)
            ws.append(w)
    for width, k in DARKNET53_BRANCH:
        ws.append(layer_weights(len(ws), ic, wd(width), k=k, seed=seed))
        ic = wd(width)
    ws.append(layer_weights(len(ws), ic, n_out, k=1, seed=seed, bn=False))
    return ws


# YOLOv3's three detection branches (yolov3.py), per scale (stride 32, 16, 8): the branch width w;
# five alternating 1x1 x w / 3x3 x 2w convs, a 3x3 x 2w conv and the linear 1x1 head.  Between two
# scales a 1x1 x w/2 reduce conv, an upsample and the concat with the trunk's stage output
YOLOV3_BRANCH_WIDTHS = (512, 256, 128)
YOLOV3_N_OUT = 255            # 3 anchors x (5 + 80 COCO classes)


def yolov3_weights(seed=WEIGHT_SEED, width_div=1, n_out=YOLOV3_N_OUT, in_c=IN_SHAPE[2]):
    """The 75-entry weight list yolov3.YOLO_V3 consumes, in Darknet layer order: darknet53's 52
    trunk convs (the same values as darknet53_weights gives them), then per scale the branch's five
    alternating 1x1 / 3x3 convs, its 3x3 conv and its linear 1x1 head with n_out outputs, with the
    1x1 reduce conv in front of each of the two upsamples after the first and the second scale's
    head.  Same counter-based generators (layer i draws from streams 10 i + j) and width_div as
    darknet53_weights.  The SAME-padding caveat of darknet53.py applies unchanged: the stride-2
    convs pad as TensorFlow does, so weights converted from a Darknet checkpoint would compute
    something else at those five layers (darknet_import.DarknetModel pads as Darknet does; its
    tests turn these generators' draws into Darknet-order weight files)."""
    def wd(c):
        if c % width_div:
            raise ValueError(f"width_div {width_div} does not divide {c}")
        return c // width_div

    n_trunk = 1 + sum(1 + 2 * b for _, b in DARKNET53_STAGES)
    ws = darknet53_weights(seed=seed, width_div=width_div, n_out=n_out, in_c=in_c)[:n_trunk]
    ic = wd(DARKNET53_STAGES[-1][0])
    skips = [wd(DARKNET53_STAGES[-2][0]), wd(DARKNET53_STAGES[-3][0])]  # the stage outputs the concats take
    for s, width in enumerate(YOLOV3_BRANCH_WIDTHS):
        for j in range(5):
            od, k = (wd(width), 1) if j % 2 == 0 else (wd(2 * width), 3)
            ws.append(layer_weights(len(ws), ic, od, k=k, seed=seed))
            ic = od
        ws.append(layer_weights(len(ws), ic, wd(2 * width), k=3, seed=seed))
        ws.append(layer_weights(len(ws), wd(2 * width), n_out, k=1, seed=seed, bn=False))
        if s < 2:
            ws.append(layer_weights(len(ws), ic, wd(width // 2), k=1, seed=seed))
            ic = wd(width // 2) + skips[s]
    return ws


# YOLOv3-SPP (yolov3_spp.py): YOLOv3 with a pyramid pooling block in the stride-32 branch, whose
# neck becomes 1x1, 3x3, 1x1, SPP (x4 channels), 1x1, 3x3, 1x1: one conv more than YOLOv3's
YOLOV3_SPP_POOLS = (13, 9, 5)


def yolov3_spp_weights(seed=WEIGHT_SEED, width_div=1, n_out=YOLOV3_N_OUT, in_c=IN_SHAPE[2]):
    """The 76-entry weight list yolov3_spp.YOLO_V3_SPP consumes, in Darknet layer order: as
    yolov3_weights, but the stride-32 branch has six neck convs (1x1, 3x3, 1x1, then after the SPP
    block a 1x1 on 4 x the width, 3x3, 1x1) before its 3x3 conv and head.  Same generators (layer
    i draws from streams 10 i + j), width_div and padding caveat as yolov3_weights; the 52 trunk
    layers have yolov3_weights' values."""
    def wd(c):
        if c % width_div:
            raise ValueError(f"width_div {width_div} does not divide {c}")
        return c // width_div

    n_trunk = 1 + sum(1 + 2 * b for _, b in DARKNET53_STAGES)
    ws = darknet53_weights(seed=seed, width_div=width_div, n_out=n_out, in_c=in_c)[:n_trunk]
    ic = wd(DARKNET53_STAGES[-1][0])
    skips = [wd(DARKNET53_STAGES[-2][0]), wd(DARKNET53_STAGES[-3][0])]
    for s, width in enumerate(YOLOV3_BRANCH_WIDTHS):
        neck = [(wd(width), 1), (wd(2 * width), 3)] * 2 + [(wd(width), 1)]
        if s == 0:  # the SPP block after the third conv: the next one reads (pools + 1) x width channels
            neck = neck[:3] + [None] + neck[2:]
        for item in neck:
            if item is None:
                ic *= len(YOLOV3_SPP_POOLS) + 1
                continue
            od, k = item
            ws.append(layer_weights(len(ws), ic, od, k=k, seed=seed))
            ic = od
        ws.append(layer_weights(len(ws), ic, wd(2 * width), k=3, seed=seed))
        ws.append(layer_weights(len(ws), wd(2 * width), n_out, k=1, seed=seed, bn=False))
        if s < 2:
            ws.append(layer_weights(len(ws), ic, wd(width // 2), k=1, seed=seed))
            ic = wd(width // 2) + skips[s]
    return ws


# YOLOv3-tiny (yolov3_tiny.py): (output channels, kernel size) of the 13 convs in Darknet order:
# the six 3x3 convs of the pooled stack, 3x3 x 1024, 1x1 x 256 (= y), head 0's 3x3 x 512 and linear
# head, the merge's 1x1 x 128, head 1's 3x3 x 256 and linear head (None: n_out)
YOLOV3_TINY_CONVS = ((16, 3), (32, 3), (64, 3), (128, 3), (256, 3), (512, 3), (1024, 3), (256, 1), (512, 3),
                     (None, 1), (128, 1), (256, 3), (None, 1))
YOLOV3_TINY_SKIP_FROM = 4  # the concat takes conv 4's output (26 x 26 x 256 at 416)


def yolov3_tiny_weights(seed=WEIGHT_SEED, width_div=1, n_out=YOLOV3_N_OUT, in_c=IN_SHAPE[2]):
    """The 13-entry weight list yolov3_tiny.YOLO_V3_TINY consumes, in Darknet layer order, from
    the same counter-based generators (layer i draws from streams 10 i + j).  width_div divides
    every channel count except the input's and the heads' n_out."""
    def wd(c):
        if c % width_div:
            raise ValueError(f"width_div {width_div} does not divide {c}")
        return c // width_div

    ws = []
    ic = in_c
    y_c = skip_c = None
    for i, (od, k) in enumerate(YOLOV3_TINY_CONVS):
        head = od is None
        if i == 10:  # the merge's reduce conv reads y
            ic = y_c
        elif i == 11:  # the first conv after the concat
            ic += skip_c
        od = n_out if head else wd(od)
        ws.append(layer_weights(i, ic, od, k=k, seed=seed, bn=not head))
        ic = od
        if i == YOLOV3_TINY_SKIP_FROM:
            skip_c = od
        if i == 7:
            y_c = od
    return ws


def yolo_zero_weights(channels=CHANNELS, in_c=IN_SHAPE[2]):
    """yolo_weights' shapes with zero values, without running the generator: what a
    non-root rank lays its plan out with before the weight broadcast fills it."""
    ws, ic = [], in_c
    for i, od in enumerate(channels):
        last = i == len(channels) - 1
        k = 1 if last else 3
        w = {"kernel": np.zeros((k, k, ic, od), np.float32), "biases": np.zeros(od, np.float32)}
        if not last:
            for key in ("moving_mean", "moving_variance", "gamma"):
                w[key] = np.zeros(od, np.float32)
        ws.append(w)
        ic = od
    return ws


def frame(index, shape=IN_SHAPE):
    """Synthetic frame `index`: uniform [0,1) fp32 NHWC [1,H,W,C]
    (the range of `proj3/__init__.py:8-12` resize_input output)."""
    n = int(np.prod(shape))
    return uniform(1 + index, 0, n).astype(np.float32).reshape((1,) + tuple(shape))


def frames(indices, shape=IN_SHAPE):
    return np.concatenate([frame(i, shape) for i in indices], axis=0)


def weights_digest(ws):
    import hashlib
    h = hashlib.sha256()
    for w in ws:
        for key in ("kernel", "biases", "moving_mean", "moving_variance", "gamma"):
            if key in w:
                h.update(np.ascontiguousarray(w[key]).tobytes())
    return h.hexdigest()
