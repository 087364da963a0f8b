"""Darknet import: a network from a `.cfg` text and a `.weights` file, on the MI355X engine.

    m = DarknetModel(open("yolov3.cfg").read(), "yolov3.weights")
    outs = m.inference(frame)             # one tensor per [yolo] section, in cfg order
    boxes = m.postprocessing(outs)        # one image's label boxes
    rows = m.detect(frames)               # plan + decode on the device
    rows = m.detect_images(images)        # uint8 images of any sizes: letterbox, plan, decode and
                                          # the boxes back in each image's pixels, on the device

The whole network lowers to ONE device plan (dnn_hip.lower_graph).  Every [convolutional]
section is one dnn_plan_add_conv_padded entry: Darknet's padding (`pad` zeros on every side, so a
3x3 / stride-2 conv on an even map reads one row and column before the frame and none after it,
where the engine's SAME convs read none before and one after), the BatchNorm folded on the host
into a per-channel scale / shift, and the fp32 leaky max(v, 0.1f v), which is Darknet's
x > 0 ? x : .1f * x for every non-NaN x.

BatchNorm fold (fold_batchnorm): in float64, rounded once to fp32,

    alpha = gamma / (sqrt(var) + 1e-6)      shift = beta - mean * alpha

and without batch_normalize scale = 1, shift = bias.  This is the inference form of the original
Darknet (normalize_cpu: (x - mean) / (sqrt(var) + .000001f), then scale_bias and add_bias); forks
use sqrt(var + eps) instead.  The outputs are held to a tolerance against a float64 restatement
of that forward (tests/darknet_oracle.py), not to Darknet's bits: Darknet rounds each of its
steps in fp32, the fold rounds once.

Sections: [net] (width, height, channels; the caller's in_shape overrides width and height, as
Darknet's own resizing does), [convolutional] (activation leaky or linear), [shortcut] (linear),
[route] (one layer: that tensor again, or with groups / group_id its channels
[group_id * c / groups, (group_id + 1) * c / groups), one dnn_hip.ChannelSlice node: the split of a
CSP block; two: their channel concat; four: the SPP pattern, three stride-1 max pools of one tensor
plus the tensor, which is one dnn_hip.Spp node in Darknet's order), [upsample], [maxpool] (where
Darknet's window placement is the engine's SAME pool's: 2/2, 2/1 and odd sizes at stride 1) and
[yolo] (mask, anchors, classes, scale_x_y; new_coords must be 0 and nms_kind absent, default or
greedynms).  The conv before each [yolo] is an output of the plan, in cfg order (at most 4, what
the decode takes: the last one the plan's output, the others taps).  The head is a
yolo_post.MultiHead with logistic class scores, the masked anchors divided by the scale's stride,
per-class NMS, multi-label output, score 0.5 and IoU 0.45 (Darknet's detector defaults); a
scale_x_y other than 1 goes into the head per scale
(yolo_post.MultiHead's scale_x_y: the box centre's logistic becomes sig * s - 0.5 * (s - 1)).
Importable stock models: YOLOv3, YOLOv3-SPP, YOLOv3-tiny and YOLOv4-tiny (cfg_text has their public
definitions).

Weight files (load_weights / save_weights): three int32 `major, minor, revision`, then `seen` (8
bytes when major * 10 + minor >= 2, else 4), then per [convolutional] in cfg order biases[n],
with batch_normalize=1 scales[n], rolling_mean[n], rolling_variance[n], then
weights[n][c][kh][kw], all fp32 little-endian.  The reader is numpy.frombuffer on the file's
bytes: nothing in a weight file executes.

Out of scope:

  * YOLOv2's [reorg] and [region]: Darknet's reorg channel order is not the route kernel's
    (TensorFlow's space_to_depth), so yolov2.py's weights are not Darknet's either;
  * grouped convs (`groups` > 1 in a [convolutional]);
  * the mish activation and with it full YOLOv4 (cfg_text("yolov4") raises);
  * [route] with groups > 1 over more than one layer (Darknet slices each layer then; no stock cfg
    does it);
  * [yolo] with new_coords = 1 (the scaled-YOLOv4 box form) and nms_kind = diounms (DIoU NMS): both
    raise DarknetError, since ignoring either gives wrong boxes;
  * image file decoding: detect_images takes H x W x 3 uint8 arrays of any sizes, letterboxes them
    on the device as Darknet's letterbox_image does and returns boxes in each image's own pixels
    (ingest.RaggedIngest, yolo_post.DetectionBuffers.correct); reading a JPEG into such an array
    is the caller's.  inference and detect still take [n, h, w, 3] fp32 arrays, already resized;
  * fp16 plans: dnn_plan_add_conv_padded is an fp32 entry;
  * heads above 16,384 boxes (608 x 608 YOLOv3 has 22,743) BY DEFAULT: the model is built with
    head=None, inference works and detect raises the decode's error.  DarknetModel(..., wide=True)
    builds a yolo_post.WideHead instead (up to 65,536 boxes, at most 16,384 candidates per image)
    and detect, detect_images and postprocessing work; heads above 65,536 boxes stay out.
"""
import struct

import numpy as np

import dnn_hip
import yolo_post
import yolov3

SECTION_TYPES = ("net", "convolutional", "shortcut", "route", "upsample", "maxpool", "yolo")
BN_EPS = 1e-6  # normalize_cpu's .000001f, added to sqrt(var)
SCORE_THR, IOU_THR = 0.5, 0.45  # Darknet's detector defaults (-thresh .5, nms .45)
MODELS = ("yolov3", "yolov3-spp", "yolov3-tiny", "yolov4-tiny")
NMS_KINDS = ("default", "greedynms")  # [yolo] nms_kind values that are the decode's greedy NMS


class DarknetError(ValueError):
    """A cfg or weight file this importer cannot read, or a layer it cannot express."""


# ------------------------------------------------------------------------------------- cfg text
def parse_cfg(text):
    """The sections of a Darknet cfg, in order: one dict per section with "type" (the name in
    brackets), "line" (its 1-based line number) and every `key = value` of the section as strings
    (keys and values stripped).  `#` and `;` start comment lines; blank lines are skipped.  A
    section type outside SECTION_TYPES raises DarknetError naming the type and the line; unknown
    keys inside a known section are kept and ignored by the importer."""
    sections = []
    for no, raw in enumerate(text.splitlines(), start=1):
        line = raw.strip()
        if not line or line[0] in "#;":
            continue
        if line[0] == "[":
            if line[-1] != "]":
                raise DarknetError(f"line {no}: malformed section header {line!r}")
            kind = line[1:-1].strip()
            if kind not in SECTION_TYPES:
                raise DarknetError(f"line {no}: section type [{kind}] is not supported "
                                   f"(supported: {', '.join(SECTION_TYPES)})")
            sections.append({"type": kind, "line": no})
            continue
        if "=" not in line:
            raise DarknetError(f"line {no}: expected `key = value`, got {line!r}")
        if not sections:
            raise DarknetError(f"line {no}: `{line}` before the first section")
        key, value = line.split("=", 1)
        sections[-1][key.strip()] = value.strip()
    if not sections or sections[0]["type"] != "net":
        raise DarknetError("a cfg starts with a [net] section")
    if any(s["type"] == "net" for s in sections[1:]):
        raise DarknetError("more than one [net] section")
    return sections


def _int(sec, key, default=None):
    if key not in sec:
        if default is None:
            raise DarknetError(f"[{sec['type']}] at line {sec['line']}: `{key}` is missing")
        return default
    try:
        return int(sec[key])
    except ValueError:
        raise DarknetError(f"[{sec['type']}] at line {sec['line']}: {key} = {sec[key]!r} is not an integer")


def _ints(sec, key):
    if key not in sec:
        raise DarknetError(f"[{sec['type']}] at line {sec['line']}: `{key}` is missing")
    try:
        return [int(v) for v in sec[key].split(",") if v.strip()]
    except ValueError:
        raise DarknetError(f"[{sec['type']}] at line {sec['line']}: {key} = {sec[key]!r} is not a list of integers")


def _layer_index(sec, value, at, what):
    """A `from` / `layers` entry as an absolute layer index: negative values count back from layer
    `at`; it must name an earlier layer."""
    idx = at + value if value < 0 else value
    if not 0 <= idx < at:
        raise DarknetError(f"[{sec['type']}] at line {sec['line']} (layer {at}): {what} {value} names layer {idx}, "
                           f"which is not one of the {at} layers before it")
    return idx


def net_shape(sections, in_shape=None):
    """(height, width, channels) of the input: [net]'s, with height and width from in_shape
    ([batch, h, w, c]) when given."""
    net = sections[0]
    h, w, c = _int(net, "height"), _int(net, "width"), _int(net, "channels", 3)
    if in_shape is not None:
        if len(in_shape) != 4:
            raise ValueError(f"in_shape {in_shape!r}: [batch, height, width, channels] expected")
        if in_shape[3] != c:
            raise DarknetError(f"in_shape {in_shape!r}: [net] has channels = {c}")
        h, w = int(in_shape[1]), int(in_shape[2])
    if h <= 0 or w <= 0 or c <= 0:
        raise DarknetError(f"input {h} x {w} x {c}: positive sizes expected")
    return h, w, c


def conv_params(sec):
    """(filters, size, stride, pad, batch_normalize, activation) of a [convolutional] section:
    pad=1 means size // 2, else the `padding` key (default 0)."""
    n, size, stride = _int(sec, "filters"), _int(sec, "size", 1), _int(sec, "stride", 1)
    pad = size // 2 if _int(sec, "pad", 0) else _int(sec, "padding", 0)
    act = sec.get("activation", "logistic")
    where = f"[convolutional] at line {sec['line']}"
    if act not in ("leaky", "linear"):
        raise DarknetError(f"{where}: activation {act!r} is not supported (leaky, linear)")
    if _int(sec, "groups", 1) != 1:
        raise DarknetError(f"{where}: grouped convs are not supported")
    if n < 1 or size < 1 or stride < 1 or not 0 <= pad < size:
        raise DarknetError(f"{where}: filters {n}, size {size}, stride {stride}, padding {pad}: need filters, size, "
                           "stride >= 1 and 0 <= padding < size")
    return n, size, stride, pad, bool(_int(sec, "batch_normalize", 0)), act


def maxpool_params(sec, in_h, in_w):
    """(size, stride) of a [maxpool] section the engine's SAME pool computes exactly.  Darknet's
    rule: out = (in + padding - size) / stride + 1 with padding = size - 1 and the window starting
    at -padding / 2.  TensorFlow's SAME has the same output size for that padding; the windows
    coincide when its front pad for this input size is (size - 1) // 2, which holds for 2/2, 2/1
    and odd sizes at stride 1 on any map.  Anything else raises DarknetError."""
    stride = _int(sec, "stride", 1)
    size = _int(sec, "size", stride)
    padding = _int(sec, "padding", size - 1)
    where = f"[maxpool] at line {sec['line']}"
    if size < 1 or stride < 1:
        raise DarknetError(f"{where}: size {size}, stride {stride}: need >= 1")
    if padding != size - 1:
        raise DarknetError(f"{where}: padding = {padding} is not supported (only Darknet's default, size - 1 = "
                           f"{size - 1})")
    for n in (in_h, in_w):
        out = (n + padding - size) // stride + 1
        same_out, front, _ = dnn_hip.get_out_pads(n, size, stride, "SAME")
        if out != same_out or front != (size - 1) // 2:
            raise DarknetError(f"{where}: a {size}/{stride} max pool on a map of {n} is not supported: Darknet "
                               f"starts its windows at {-((size - 1) // 2)}, the engine's SAME pool at {-front}")
    return size, stride


def route_group(sec, n_layers, c):
    """(first, channels) of the channel range a [route] section takes of its c input channels:
    groups (default 1) and group_id (default 0) select [group_id * c / groups, (group_id + 1) * c /
    groups).  DarknetError, naming the line, when groups does not divide c, group_id is outside
    0..groups-1, or groups > 1 comes with more than one layer."""
    groups, gid = _int(sec, "groups", 1), _int(sec, "group_id", 0)
    where = f"[route] at line {sec['line']}"
    if groups < 1:
        raise DarknetError(f"{where}: groups = {groups}: need >= 1")
    if not 0 <= gid < groups:
        raise DarknetError(f"{where}: group_id = {gid} is outside 0..{groups - 1} (groups = {groups})")
    if groups > 1 and n_layers != 1:
        raise DarknetError(f"{where}: groups = {groups} with {n_layers} layers is not supported (one layer only)")
    if c % groups:
        raise DarknetError(f"{where}: groups = {groups} does not divide the layer's {c} channels")
    return gid * (c // groups), c // groups


def yolo_params(sec):
    """scale_x_y (default 1) of a [yolo] section, after refusing what the decode does not implement:
    new_coords other than 0 and an nms_kind outside NMS_KINDS."""
    where = f"[yolo] at line {sec['line']}"
    if _int(sec, "new_coords", 0) != 0:
        raise DarknetError(f"{where}: new_coords = {sec['new_coords']} is not supported (only 0)")
    kind = sec.get("nms_kind", "default")
    if kind not in NMS_KINDS:
        raise DarknetError(f"{where}: nms_kind = {kind} is not supported ({', '.join(NMS_KINDS)})")
    try:
        s = float(sec.get("scale_x_y", 1))
    except ValueError:
        raise DarknetError(f"{where}: scale_x_y = {sec['scale_x_y']!r} is not a number")
    if not (s > 0 and s < float("inf")):
        raise DarknetError(f"{where}: scale_x_y = {s}: need a finite value > 0")
    return s


def layer_shapes(sections, in_shape=None):
    """Per layer (every section after [net]) its output's (h, w, c), walking the cfg as Darknet's
    parser does; raises DarknetError for a section that does not fit its input."""
    h, w, c = net_shape(sections, in_shape)
    shapes = []
    for at, sec in enumerate(sections[1:]):
        kind = sec["type"]
        if kind == "convolutional":
            n, size, stride, pad, _, _ = conv_params(sec)
            if h + 2 * pad < size or w + 2 * pad < size:
                raise DarknetError(f"[convolutional] at line {sec['line']}: a {size}x{size} kernel on a "
                                   f"{h} x {w} map with padding {pad} has no output")
            h, w, c = (h + 2 * pad - size) // stride + 1, (w + 2 * pad - size) // stride + 1, n
        elif kind == "shortcut":
            if sec.get("activation", "linear") != "linear":
                raise DarknetError(f"[shortcut] at line {sec['line']}: activation {sec['activation']!r} is not "
                                   "supported (linear)")
            src = shapes[_layer_index(sec, _int(sec, "from"), at, "from")]
            if src != (h, w, c):
                raise DarknetError(f"[shortcut] at line {sec['line']}: layer shapes {src} and {(h, w, c)} differ")
        elif kind == "route":
            idx = [_layer_index(sec, v, at, "layers") for v in _ints(sec, "layers")]
            if len(idx) not in (1, 2, 4):
                raise DarknetError(f"[route] at line {sec['line']}: {len(idx)} layers are not supported (1, 2, or "
                                   "the 4 of an SPP block)")
            srcs = [shapes[i] for i in idx]
            if any(s[:2] != srcs[0][:2] for s in srcs):
                raise DarknetError(f"[route] at line {sec['line']}: layers of sizes {srcs} cannot be concatenated")
            h, w = srcs[0][:2]
            c = route_group(sec, len(idx), sum(s[2] for s in srcs))[1]
        elif kind == "upsample":
            f = _int(sec, "stride", 2)
            if not 1 <= f <= dnn_hip.MAX_UPSAMPLE_FACTOR:
                raise DarknetError(f"[upsample] at line {sec['line']}: stride {f} outside 1..{dnn_hip.MAX_UPSAMPLE_FACTOR}")
            h, w = h * f, w * f
        elif kind == "maxpool":
            size, stride = maxpool_params(sec, h, w)
            h, w = (h + stride - 1) // stride, (w + stride - 1) // stride
        elif kind == "yolo":
            if at == 0 or sections[at]["type"] != "convolutional":
                raise DarknetError(f"[yolo] at line {sec['line']}: it must follow a [convolutional] section")
            yolo_params(sec)
        shapes.append((h, w, c))
    return shapes


def conv_shapes(sections):
    """Per [convolutional] section in cfg order: (filters, input channels, size, batch_normalize).
    (Channel counts do not depend on the input size.)"""
    net = sections[0]
    shapes = layer_shapes(sections, [1, max(_int(net, "height"), 1), max(_int(net, "width"), 1), _int(net, "channels", 3)])
    out = []
    c_in = _int(net, "channels", 3)
    for sec, shape in zip(sections[1:], shapes):
        if sec["type"] == "convolutional":
            n, size, _, _, bn, _ = conv_params(sec)
            out.append((n, c_in, size, bn))
        c_in = shape[2]
    return out


# --------------------------------------------------------------------------------- weight files
class WeightList(list):
    """load_weights' result: the per-conv dicts, plus the file's header fields."""
    major = minor = revision = seen = 0


def _header_seen_bytes(major, minor):
    return 8 if major * 10 + minor >= 2 else 4


def load_weights(path, sections, partial=False):
    """The parameters of every [convolutional] section of `sections`, in cfg order, from a Darknet
    weight file: a WeightList of dicts with fp32 arrays in Darknet's own order, "biases" [n], with
    batch_normalize=1 "scales", "rolling_mean" and "rolling_variance" [n], and "weights"
    [n][c][kh][kw] (kernel_hwio gives the engine's layout).  A file that ends early and a file with
    bytes left over are both DarknetError unless `partial`: then the layers the file holds whole
    are returned and the rest of the file is ignored."""
    with open(path, "rb") as f:
        data = f.read()
    if len(data) < 12:
        raise DarknetError(f"{path}: {len(data)} bytes: too short for a Darknet header")
    major, minor, revision = struct.unpack_from("<3i", data, 0)
    nseen = _header_seen_bytes(major, minor)
    if len(data) < 12 + nseen:
        raise DarknetError(f"{path}: {len(data)} bytes: too short for a Darknet header")
    seen = struct.unpack_from("<q" if nseen == 8 else "<i", data, 12)[0]
    at = 12 + nseen
    out = WeightList()
    out.major, out.minor, out.revision, out.seen = major, minor, revision, seen

    def take(count, shape, what):
        nonlocal at
        end = at + 4 * count
        if end > len(data):
            raise EOFError(what)
        a = np.frombuffer(data, dtype="<f4", count=count, offset=at).reshape(shape).astype(np.float32)
        at = end
        return a

    for k, (n, c, size, bn) in enumerate(conv_shapes(sections)):
        start = at
        try:
            layer = {"biases": take(n, (n,), "biases")}
            if bn:
                for key in ("scales", "rolling_mean", "rolling_variance"):
                    layer[key] = take(n, (n,), key)
            layer["weights"] = take(n * c * size * size, (n, c, size, size), "weights")
        except EOFError as e:
            if partial:
                at = start
                break
            raise DarknetError(f"{path}: the file ends inside the {e} of convolutional layer {k} "
                               f"({n} filters of {c} x {size} x {size}): {len(data)} bytes, at least "
                               f"{start + 4 * ((4 if bn else 1) * n + n * c * size * size)} expected")
        out.append(layer)
    if at != len(data) and not partial:
        raise DarknetError(f"{path}: {len(data) - at} bytes left after the last convolutional layer "
                           "(the cfg does not match the file)")
    return out


def save_weights(path, layers, major=0, minor=2, revision=0, seen=0):
    """Write `layers` (dicts as load_weights returns them, in cfg order) as a Darknet weight file."""
    with open(path, "wb") as f:
        f.write(struct.pack("<3i", major, minor, revision))
        f.write(struct.pack("<q" if _header_seen_bytes(major, minor) == 8 else "<i", seen))
        for k, layer in enumerate(layers):
            w = np.asarray(layer["weights"])
            if w.ndim != 4 or w.shape[2] != w.shape[3]:
                raise DarknetError(f"layer {k}: weights of shape {w.shape}, [n][c][size][size] expected")
            keys = ("biases",) + (("scales", "rolling_mean", "rolling_variance") if "scales" in layer else ())
            for key in keys:
                a = np.asarray(layer[key])
                if a.shape != (w.shape[0],):
                    raise DarknetError(f"layer {k}: {key} of shape {a.shape}, ({w.shape[0]},) expected")
                f.write(np.ascontiguousarray(a, dtype="<f4").tobytes())
            f.write(np.ascontiguousarray(w, dtype="<f4").tobytes())


def kernel_hwio(layer):
    """A layer's Darknet weights [n][c][kh][kw] as the engine's HWIO kernel [kh][kw][c][n]."""
    return np.ascontiguousarray(np.asarray(layer["weights"], np.float32).transpose(2, 3, 1, 0))


def fold_batchnorm(layer):
    """(scale, shift) fp32 of a layer's epilogue y = conv * scale + shift: with BatchNorm
    alpha = scales / (sqrt(rolling_variance) + 1e-6) and shift = biases - rolling_mean * alpha,
    computed in float64 and rounded once; without it scale = 1 and shift = biases.  The inference
    form of the original Darknet (normalize_cpu); forks use sqrt(var + eps)."""
    beta = np.asarray(layer["biases"], np.float64)
    if "scales" not in layer:
        return np.ones(beta.shape, np.float32), beta.astype(np.float32)
    var = np.asarray(layer["rolling_variance"], np.float64)
    if (var < 0).any():
        raise DarknetError("a rolling_variance is negative")
    alpha = np.asarray(layer["scales"], np.float64) / (np.sqrt(var) + BN_EPS)
    shift = beta - np.asarray(layer["rolling_mean"], np.float64) * alpha
    return alpha.astype(np.float32), shift.astype(np.float32)


def check_layers(sections, layers):
    """`layers` (load_weights' format) against the cfg's conv shapes: DarknetError on a mismatch."""
    shapes = conv_shapes(sections)
    if len(layers) != len(shapes):
        raise DarknetError(f"{len(layers)} weight layers for {len(shapes)} [convolutional] sections")
    for k, (layer, (n, c, size, bn)) in enumerate(zip(layers, shapes)):
        keys = ("biases", "weights") + (("scales", "rolling_mean", "rolling_variance") if bn else ())
        if any(key not in layer for key in keys):
            raise DarknetError(f"convolutional layer {k}: expected a dict with {keys}")
        if tuple(np.asarray(layer["weights"]).shape) != (n, c, size, size):
            raise DarknetError(f"convolutional layer {k}: weights of shape {np.asarray(layer['weights']).shape}, "
                               f"{(n, c, size, size)} expected")


# ------------------------------------------------------------------------------------- the graph
class _LazyPool(object):
    """A stride-1 odd-size [maxpool]: a MaxPool2D node when something reads it, a block of an Spp
    node when a four-layer [route] reads it beside its own input."""

    def __init__(self, src, size):
        self.src, self.size, self.node = src, size, None


def build_graph(builder_cls, sections, layers, in_shape):
    """Return (graph, outs, yolos): outs the head nodes (the conv before each [yolo], in cfg
    order; all but the last are the graph's extra outputs, the last its primary one), yolos the
    [yolo] sections with "grid" = that tensor's (h, w).  `layers` is load_weights' list."""
    check_layers(sections, layers)
    shapes = layer_shapes(sections, in_shape)
    g = builder_cls()
    x = g.create_input([int(v) for v in in_shape])
    out = []       # per layer: a node or a _LazyPool; a one-layer route repeats its source's object
    outs, yolos = [], []
    weights = iter(layers)

    def node(v):
        if isinstance(v, _LazyPool):
            if v.node is None:
                v.node = g.create_max_pool2d(node(v.src), [1, v.size, v.size, 1], [1, 1, 1, 1], "SAME")
            return v.node
        return v

    prev = x
    for at, sec in enumerate(sections[1:]):
        kind = sec["type"]
        if kind == "convolutional":
            n, size, stride, pad, _, act = conv_params(sec)
            layer = next(weights)
            scale, shift = fold_batchnorm(layer)
            t = g.create_conv2d_padded(node(prev), kernel_hwio(layer), [1, stride, stride, 1], (pad, pad))
            t = g.create_scale_shift(t, scale, shift)
            cur = g.create_leaky_relu_f32(t) if act == "leaky" else t
        elif kind == "shortcut":
            src = out[_layer_index(sec, _int(sec, "from"), at, "from")]
            cur = g.create_add([node(src), node(prev)])
        elif kind == "route":
            srcs = [out[_layer_index(sec, v, at, "layers")] for v in _ints(sec, "layers")]
            if len(srcs) == 1:
                src_c = shapes[_layer_index(sec, _ints(sec, "layers")[0], at, "layers")][2]
                first, channels = route_group(sec, 1, src_c)
                cur = srcs[0] if channels == src_c else g.create_channel_slice(node(srcs[0]), first, channels)
            elif len(srcs) == 2:
                cur = g.create_concat([node(srcs[0]), node(srcs[1])])
            else:
                cur = _spp(g, sec, srcs)
        elif kind == "upsample":
            cur = g.create_upsample(node(prev), _int(sec, "stride", 2))
        elif kind == "maxpool":
            h, w, _ = shapes[at - 1] if at else net_shape(sections, in_shape)
            size, stride = maxpool_params(sec, h, w)
            if stride == 1 and size % 2 == 1 and 3 <= size <= dnn_hip.MAX_SPP_K:
                cur = _LazyPool(prev, size)
            else:
                cur = g.create_max_pool2d(node(prev), [1, size, size, 1], [1, stride, stride, 1], "SAME")
        else:  # yolo: the conv before it is an output; the layer itself repeats that tensor
            outs.append(node(prev))
            yolos.append(dict(sec, grid=shapes[at][:2]))
            cur = prev
        out.append(cur)
        prev = cur
    if not outs:
        raise DarknetError("the cfg has no [yolo] section: nothing to output")
    if outs[-1] is not node(prev):
        raise DarknetError("the last [yolo] section must end the cfg (the plan's output is the last tensor computed)")
    if len(outs) > yolo_post.MAX_SCALES or len(set(map(id, outs))) != len(outs):
        raise DarknetError(f"{len(outs)} [yolo] sections: at most {yolo_post.MAX_SCALES}, each on its own conv")
    for o in outs[:-1]:
        g.add_out_node(o)
    g.set_out_node(outs[-1])
    return g, outs, yolos


def _spp(g, sec, srcs):
    """The Spp node of a four-layer route: three unread stride-1 pools of one tensor, then that
    tensor (Darknet's order)."""
    xs, pools = srcs[3], srcs[:3]
    if not isinstance(xs, _LazyPool) and all(isinstance(p, _LazyPool) and p.node is None and p.src is xs for p in pools):
        return g.create_spp(xs, [p.size for p in pools])
    raise DarknetError(f"[route] at line {sec['line']}: four layers are supported only as an SPP block (three "
                       "stride-1 max pools of one tensor, then that tensor)")


def multi_head(yolos, in_h, in_w, score_thr=SCORE_THR, iou_thr=IOU_THR, nms="per_class", labels="multi", wide=False):
    """The yolo_post.MultiHead of build_graph's `yolos` for an in_h x in_w input: per [yolo] the
    anchors its mask picks, in pixels, divided by the scale's stride (input / grid).  With `wide`
    a yolo_post.WideHead (up to 65,536 boxes, the grid-wide decode), whatever the box count."""
    scales, xy = [], []
    for y in yolos:
        xy.append(yolo_params(y))
        gh, gw = y["grid"]
        if in_h % gh or in_w % gw or in_h // gh != in_w // gw:
            raise DarknetError(f"[yolo] at line {y['line']}: a {gh} x {gw} grid does not divide the {in_h} x {in_w} "
                               "input into square cells")
        stride = in_h // gh
        try:
            anchors = [float(v) for v in y["anchors"].split(",") if v.strip()]
        except (KeyError, ValueError):
            raise DarknetError(f"[yolo] at line {y['line']}: `anchors` is missing or not a list of numbers")
        mask = _ints(y, "mask") if "mask" in y else list(range(len(anchors) // 2))
        if len(anchors) % 2 or any(not 0 <= m < len(anchors) // 2 for m in mask) or not mask:
            raise DarknetError(f"[yolo] at line {y['line']}: mask {mask} does not fit {len(anchors) // 2} anchors")
        px = [a for m in mask for a in anchors[2 * m:2 * m + 2]]
        scales.append(yolo_post.Scale(gh, gw, len(mask), _int(y, "classes", 20), tuple(a / stride for a in px),
                                      float(stride), score_thr, iou_thr))
    kw = {} if all(s == 1.0 for s in xy) else {"scale_x_y": tuple(xy)}
    return (yolo_post.WideHead if wide else yolo_post.MultiHead)(scales, "logistic", nms, labels, **kw)


_AUTO = object()


class DarknetModel(yolov3.YOLO_V3):
    """A Darknet network with the MI355X engine underneath.  `cfg_text` is the cfg's text,
    `weights` a weight file's path or load_weights' list; `in_shape` [batch, h, w, c] overrides
    [net]'s width and height (default [1, height, width, channels]).  `head` is a
    yolo_post.MultiHead; left out, multi_head's (Darknet's detector defaults; score_thr, iou_thr,
    nms and labels override them), or None where the cfg's boxes exceed the decode's 16,384: then
    inference works and postprocessing / detect raise the decode's error.  `wide=True` makes that
    head a yolo_post.WideHead instead (up to 65,536 boxes, the grid-wide decode), so the stock
    608 x 608 cfgs give detections.  `latency` as
    dnn_hip.DnnInferenceEngine's.  inference, postprocessing and detect are yolov3.YOLO_V3's, on
    one tensor per [yolo] section in cfg order."""

    def __init__(self, cfg_text, weights, in_shape=None, debug=False, device=None, head=_AUTO, latency=None,
                 score_thr=SCORE_THR, iou_thr=IOU_THR, nms="per_class", labels="multi", wide=False):
        self.sections = parse_cfg(cfg_text)
        h, w, c = net_shape(self.sections, in_shape)
        self.in_shape = (int(in_shape[0]) if in_shape is not None else 1, h, w, c)
        self.layers = load_weights(weights, self.sections) if isinstance(weights, (str, bytes)) or hasattr(
            weights, "__fspath__") else list(weights)
        self.g, self.outs, self.yolos = build_graph(dnn_hip.DnnGraphBuilder, self.sections, self.layers, self.in_shape)
        self._head_error = None
        if head is _AUTO:
            try:
                head = multi_head(self.yolos, h, w, score_thr, iou_thr, nms, labels, wide)
            except DarknetError:
                raise
            except ValueError as e:
                boxes = sum(y["grid"][0] * y["grid"][1] * (len(_ints(y, "mask")) if "mask" in y else 1)
                            for y in self.yolos)
                if boxes <= yolo_post.MULTI_MAX_BOXES:
                    raise
                head, self._head_error = None, str(e)
        if head is not None:
            shapes = [tuple(o.result.shape[1:]) for o in self.outs]
            if list(head.pred_shapes) != shapes:
                raise ValueError(f"head {head!r} does not fit the outputs {shapes}")
        self.head = head
        self.sess = dnn_hip.DnnInferenceEngine(self.g, debug, device=device, latency=latency)
        self._dev = None
        self._ingest = {}  # detect_images' RaggedIngest per pixel order

    def _need_head(self):
        if self.head is None:
            raise ValueError(self._head_error or "the model was built with head=None: pass head=")

    def postprocessing(self, outs):
        self._need_head()
        return super().postprocessing(outs)

    def detect(self, frames, raise_errors=True):
        self._need_head()
        return super().detect(frames, raise_errors)

    def detect_images(self, images, order="bgr", raise_errors=True):
        """Detections of up to `batch` H x W x 3 uint8 images of any sizes, each in its own
        image's pixels: per image the (class, left, top, right, bottom, score) rows of `detect`,
        mapped back.  On the device throughout: the 8-bit pixels are uploaded and letterboxed as
        Darknet's letterbox_image does (ingest.RaggedIngest) into the plan's input, the plan and
        the multi-scale decode run as in `detect`, and the rows are corrected in place
        (yolo_post.DetectionBuffers.correct).  order "bgr" (cv2 frames) or "rgb".  Leaves dets /
        counts in self.buffers, ready for its pack().  (AlexeyAB's detector stretches an image to
        the network's size by default where this letterboxes, so boxes for YOLOv4-tiny compare
        with its -letter_box runs; not pinned by a test.)"""
        import torch
        import ingest
        self._need_head()
        images = list(images)
        batch, net_hw = self.in_shape[0], self.in_shape[1:3]
        if self.in_shape[3] != 3:
            raise ValueError(f"detect_images needs a 3-channel network, [net] has channels = {self.in_shape[3]}")
        if order not in ingest.PIXEL_ORDERS:
            raise ValueError(f"order {order!r}: need one of {sorted(ingest.PIXEL_ORDERS)}")
        _, _, sizes, nbytes = ingest.ragged_layout(images, batch, 1 << 62, net_hw)  # (raises before any device work)
        n = len(images)
        plan = self.sess.plan()
        device = torch.device("cuda", plan.device)
        d = self._device_buffers(plan, device)
        with torch.cuda.device(device):
            compute = torch.cuda.current_stream()
            stream = compute.cuda_stream
            ing = self._ingest.get(order)
            if ing is None or ing.max_bytes < nbytes or ing.compute != compute:
                ing = ingest.RaggedIngest(batch, max(nbytes, 1), net_hw, device, compute, order)
                self._ingest[order] = ing
            ing.submit(images, out_ptr=d["in"].data_ptr())
            plan.run_device(n, d["in"].data_ptr(), d["out"].data_ptr(), stream)
            self.buffers.run(d["taps"] + [d["out"].data_ptr()], n, stream)
            self.buffers.correct(sizes, net_hw, n, stream)
            dets = self.buffers.dets[:n].cpu().numpy()
            counts = self.buffers.counts[:n].cpu().numpy()
        return yolo_post.DetectionBuffers.to_rows(dets, counts, self.buffers.max_det, raise_errors)


# ----------------------------------------------------------------------------- the public cfgs
_STAGES = ((64, 1), (128, 2), (256, 8), (512, 8), (1024, 4))  # Darknet-53: (width, residual blocks)
_ANCHORS = "10,13,  16,30,  33,23,  30,61,  62,45,  59,119,  116,90,  156,198,  373,326"
_TINY_ANCHORS = "10,14,  23,27,  37,58,  81,82,  135,169,  344,319"


class _Cfg(object):
    """Text of a cfg under construction, counting layers as Darknet does."""

    def __init__(self, width, height, div):
        self.div, self.n = div, 0
        self.lines = ["[net]", "# Testing", "batch=1", "subdivisions=1", f"width={width}", f"height={height}",
                      "channels=3", "momentum=0.9", "decay=0.0005", "angle=0", "saturation = 1.5",
                      "exposure = 1.5", "hue=.1", "", "learning_rate=0.001", "burn_in=1000", "max_batches = 500200",
                      "policy=steps", "steps=400000,450000", "scales=.1,.1", ""]

    def wd(self, c):
        if c % self.div:
            raise ValueError(f"width_div {self.div} does not divide {c}")
        return c // self.div

    def add(self, kind, *pairs):
        self.lines += [f"[{kind}]"] + [f"{k}={v}" for k, v in pairs] + [""]
        self.n += 1
        return self.n - 1

    def conv(self, filters, size, stride=1, head=False):
        if head:  # a linear conv with a bias, 3 x (5 + classes) filters whatever the width
            pairs = [("size", size), ("stride", stride), ("pad", 1), ("filters", filters), ("activation", "linear")]
        else:
            pairs = [("batch_normalize", 1), ("filters", self.wd(filters)), ("size", size), ("stride", stride),
                     ("pad", 1), ("activation", "leaky")]
        return self.add("convolutional", *pairs)

    def yolo(self, mask, anchors, classes):
        return self.add("yolo", ("mask", mask), ("anchors", anchors), ("classes", classes),
                        ("num", len(anchors.split(",")) // 2), ("jitter", ".3"), ("ignore_thresh", ".7"),
                        ("truth_thresh", 1), ("random", 1))

    def yolo_v4(self, mask, anchors, classes):
        return self.add("yolo", ("mask", mask), ("anchors", anchors), ("classes", classes),
                        ("num", len(anchors.split(",")) // 2), ("jitter", ".3"), ("scale_x_y", "1.05"),
                        ("cls_normalizer", "1.0"), ("iou_normalizer", "0.07"), ("iou_loss", "ciou"),
                        ("ignore_thresh", ".7"), ("truth_thresh", 1), ("random", 0), ("resize", "1.5"),
                        ("nms_kind", "greedynms"), ("beta_nms", "0.6"))

    def text(self):
        return "\n".join(self.lines)


def cfg_text(model, classes=80, width=416, height=416, width_div=1):
    """The public definition of `model` ("yolov3", "yolov3-spp", "yolov3-tiny" or "yolov4-tiny") as cfg
    text, for `classes` classes and a width x height input; width_div divides every channel count
    except the heads' 3 x (5 + classes) (a narrow model of the same topology)."""
    if model not in MODELS:
        raise ValueError(f"model {model!r}: one of {MODELS} expected")
    n_out = 3 * (5 + int(classes))
    c = _Cfg(width, height, int(width_div))
    if model == "yolov3-tiny":
        for k, f in enumerate((16, 32, 64, 128, 256, 512)):
            at = c.conv(f, 3)
            if f == 256:
                lateral = at
            c.add("maxpool", ("size", 2), ("stride", 2 if k < 5 else 1))
        c.conv(1024, 3)
        c.conv(256, 1)
        c.conv(512, 3)
        c.conv(n_out, 1, head=True)
        c.yolo("3,4,5", _TINY_ANCHORS, classes)
        c.add("route", ("layers", "-4"))
        c.conv(128, 1)
        c.add("upsample", ("stride", 2))
        c.add("route", ("layers", f"-1, {lateral}"))
        c.conv(256, 3)
        c.conv(n_out, 1, head=True)
        c.yolo("0,1,2", _TINY_ANCHORS, classes)
        return c.text()
    if model == "yolov4-tiny":
        c.conv(32, 3, stride=2)
        c.conv(64, 3, stride=2)
        for f in (64, 128, 256):  # CSP blocks: A, B = conv(second half of A), C, D = conv 1x1 of [C, B], [A, D], pool
            c.conv(f, 3)
            c.add("route", ("layers", "-1"), ("groups", 2), ("group_id", 1))
            c.conv(f // 2, 3)
            c.conv(f // 2, 3)
            c.add("route", ("layers", "-1,-2"))
            lateral = c.conv(f, 1)
            c.add("route", ("layers", "-6,-1"))
            c.add("maxpool", ("size", 2), ("stride", 2))
        c.conv(512, 3)
        c.lines.append("##################################")
        c.conv(256, 1)
        c.conv(512, 3)
        c.conv(n_out, 1, head=True)
        c.yolo_v4("3,4,5", _TINY_ANCHORS, classes)
        c.add("route", ("layers", "-4"))
        c.conv(128, 1)
        c.add("upsample", ("stride", 2))
        c.add("route", ("layers", f"-1, {lateral}"))
        c.conv(256, 3)
        c.conv(n_out, 1, head=True)
        c.yolo_v4("1,2,3", _TINY_ANCHORS, classes)
        return c.text()
    c.conv(32, 3)
    stage_end = []
    for f, blocks in _STAGES:
        c.lines.append("# Downsample")
        c.conv(f, 3, stride=2)
        for _ in range(blocks):
            c.conv(f // 2, 1)
            c.conv(f, 3)
            stage_end.append(c.add("shortcut", ("from", -3), ("activation", "linear")))
    ends = []  # the last layer of each stage
    at = 0
    for _, blocks in _STAGES:
        at += blocks
        ends.append(stage_end[at - 1])
    laterals = (ends[3], ends[2])
    for k, (f, mask) in enumerate(((512, "6,7,8"), (256, "3,4,5"), (128, "0,1,2"))):
        c.conv(f, 1)
        c.conv(2 * f, 3)
        c.conv(f, 1)
        if k == 0 and model == "yolov3-spp":
            c.lines.append("### SPP ###")
            c.add("maxpool", ("stride", 1), ("size", 5))
            c.add("route", ("layers", "-2"))
            c.add("maxpool", ("stride", 1), ("size", 9))
            c.add("route", ("layers", "-4"))
            c.add("maxpool", ("stride", 1), ("size", 13))
            c.add("route", ("layers", "-1,-3,-5,-6"))
            c.lines.append("### End SPP ###")
            c.conv(f, 1)
        c.conv(2 * f, 3)
        c.conv(f, 1)
        c.conv(2 * f, 3)
        c.conv(n_out, 1, head=True)
        c.yolo(mask, _ANCHORS, classes)
        if k < 2:
            c.add("route", ("layers", "-4"))
            c.conv(f // 2, 1)
            c.add("upsample", ("stride", 2))
            c.add("route", ("layers", f"-1, {laterals[k]}"))
    return c.text()
