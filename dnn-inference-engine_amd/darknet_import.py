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
Darknet's own resizing does), [convolutional] (activation leaky, linear, mish, swish or logistic: the last
three a dnn_hip.Activation node, in the plan the conv's epilogue; DarknetModel parses with ACTIVATIONS, parse_cfg
on its own lets only leaky and linear through unless given the set), [shortcut] (linear, mish, swish, logistic),
[route] (one layer: that tensor again, or with groups / group_id its channels
[group_id * c / groups, (group_id + 1) * c / groups), one dnn_hip.ChannelSlice node: the split of a
CSP block; two: their channel concat; four: the SPP pattern, three stride-1 max pools of one tensor
plus the tensor, which is one dnn_hip.Spp node in Darknet's order), [upsample], [maxpool] (where
Darknet's window placement is the engine's SAME pool's: 2/2, 2/1 and odd sizes at stride 1) and
[yolo] (mask, anchors, classes, scale_x_y; new_coords 0 or 1, the latter only after a conv with
activation = logistic, whose values the decode then takes as they are; nms_kind absent, default or
greedynms, or beside new_coords = 1 diounms with beta_nms: the DIoU NMS (diounms with new_coords = 0
still raises, as it always did here); all [yolo] sections of a cfg must agree on the
three).  The conv before each [yolo] is an output of the plan, in cfg order (at most 4, what
the decode takes: the last one the plan's output, the others taps).  The head is a
yolo_post.MultiHead with logistic class scores, the masked anchors divided by the scale's stride,
per-class NMS, multi-label output, score 0.5 and IoU 0.45 (Darknet's detector defaults); a
scale_x_y other than 1 goes into the head per scale
(yolo_post.MultiHead's scale_x_y: the box centre's logistic becomes sig * s - 0.5 * (s - 1)).
Importable stock models: YOLOv3, YOLOv3-SPP, YOLOv3-tiny, YOLOv4-tiny and YOLOv4 (cfg_text has their public
definitions; "yolov4" is CSPDarknet53 with mish, the SPP + PAN neck with leaky and three [yolo] sections with
scale_x_y 1.2 / 1.1 / 1.05 and greedy NMS; iou_thresh, max_delta and the loss keys are training matters and
are ignored like every unknown key; beta_nms is read under nms_kind = diounms only).

YOLOv2: [reorg] (stride, default 1: a dnn_hip.Reorg node, Darknet's permutation of the flat CHW buffer, which
is not space_to_depth; in the plan one dnn_plan_add_reorg entry together with the two-layer [route] that
follows it, reorg.hip) and [region] as the last section (region_params: coords = 4, softmax = 1, num = the
anchor count): the conv before it, filters = num * (5 + classes) and activation = linear, is the plan's
output and the head a one-scale yolo_post.MultiHead with softmax class scores, per-class NMS, multi-label
output and the thresholds above; its anchors are `anchors` as they stand, since region anchors are in
cells, and the cell is input / grid.  cfg_text has "yolov2", "yolov2_voc", "yolov2_tiny" and
"yolov2_tiny_voc" (416 x 416).  yolov2.py's hand-written model keeps TensorFlow's space_to_depth order, so
its weights are not Darknet's; an imported yolov2.cfg is.  Parity with a Darknet binary is not pinned by a
test (none is at hand): the tests pin the reorg definition and a float64 restatement of the forward.

Classifiers: [avgpool] (a dnn_hip.GlobalAvgPool node, dnn_plan_add_avgpool), [softmax] (groups 1,
temperature 1, no tree, on a 1 x 1 map: a dnn_hip.Softmax node, dnn_plan_add_softmax), [connected]
(output, activation linear or leaky, optional batch_normalize; only on a 1 x 1 map, where Darknet's
CHW flattening and the engine's NHWC agree: a 1x1 padded conv entry), and [dropout] / [cost], which
count as layers for [route] / [shortcut] indices and compute nothing.  A cfg without [yolo] builds
with head=None and the last tensor computed as the plan's output: `inference` returns that tensor,
and for a net ending in a 1 x 1 map

    idx, prob = m.classify(frames, k=5)   # [n, k] best classes and their scores, top-k on the device

Squeeze-and-excitation: [scale_channels] (activation linear, no scale_wh) is read only as the end of the SE block
of the MBConv networks, [avgpool], two 1x1 stride-1 [convolutional] sections (a bias or a folded BatchNorm, any
supported activation), then [scale_channels] with `from` naming the [avgpool]'s input (se_block).  The four sections
count as four layers and the two convs' weights are read in file order like any conv's, but they make ONE
dnn_hip.SqueezeExcite node (dnn_plan_add_squeeze_excite: two kernels, no slot, squeeze_excite.hip); nothing else
may read the three inner layers.  cfg_text("efficientnet_b0") is EfficientNet-B0 built from the paper's table.

cfg_text has the Darknet-19 and Darknet-53 classifier definitions ("darknet19", "darknet53").  The
frames are [n, h, w, c] fp32 at the network's size: the classifier demo's resize and centre crop are
the caller's.

Weight files (load_weights / save_weights): three int32 `major, minor, revision`, then `seen` (8
bytes when major * 10 + minor >= 2, else 4), then per [convolutional] in cfg order biases[n],
with batch_normalize=1 scales[n], rolling_mean[n], rolling_variance[n], then
weights[n][c / groups][kh][kw], all fp32 little-endian (a [convolutional] with groups > 1 is a grouped
conv: one dnn_plan_add_conv_grouped entry, its kernel [kh][kw][c / groups][n]).  A [connected] section
has its own order (load_connected_weights): biases[outputs], weights[outputs][inputs], then with
batch_normalize=1 scales, rolling_mean, rolling_variance; its dict holds 2-D "weights", which is how
save_weights knows it.  The reader is numpy.frombuffer on the file's
bytes: nothing in a weight file executes.

Out of scope:

  * YOLO9000 and the other [region] forms: softmax_tree, background = 1, classfix, softmax = 0, coords
    other than 4; [reorg] with reverse = 1, flatten = 1 or extra;
  * activations other than leaky, linear, mish, swish and logistic (relu, elu, tanh);
  * [sam] (spatial attention) and [scale_channels] with scale_wh = 1 or outside the SE block above;
  * [shortcut] with activation=leaky (Darknet's ResNet / ResNeXt classifiers), [connected] on a map
    larger than 1 x 1, [softmax] with groups, a temperature or a tree;
  * [route] with groups > 1 over more than one layer (Darknet slices each layer then; no stock cfg
    does it);
  * [route] over more than two layers outside an SPP block (YOLOv7's four-layer concat), so of the
    cfgs with new_coords = 1 and nms_kind = diounms, which the head decodes, yolov4-csp and its
    scaled relatives are expected to import and yolov7 is not;
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

BASE_SECTION_TYPES = ("net", "convolutional", "shortcut", "route", "upsample", "maxpool", "yolo", "avgpool", "softmax",
                      "connected", "dropout", "cost")              # what parse_cfg lets through unless told otherwise
SECTION_TYPES = BASE_SECTION_TYPES + ("reorg", "region", "scale_channels")  # ... and with YOLOv2's two sections and the
#                                                     squeeze-and-excitation gate's closing one: DarknetModel's set
BN_EPS = 1e-6  # normalize_cpu's .000001f, added to sqrt(var)
BASE_ACTIVATIONS = ("leaky", "linear")                         # what parse_cfg lets through unless told otherwise
ACTIVATIONS = BASE_ACTIVATIONS + ("mish", "swish", "logistic")  # of [convolutional]; [shortcut]: all but leaky
SCORE_THR, IOU_THR = 0.5, 0.45  # Darknet's detector defaults (-thresh .5, nms .45)
MODELS = ("yolov3", "yolov3-spp", "yolov3-tiny", "yolov4-tiny", "yolov4", "darknet19", "darknet53",
          "yolov2", "yolov2_voc", "yolov2_tiny", "yolov2_tiny_voc", "efficientnet_b0")
CLASSIFIERS = {"darknet19": 224, "darknet53": 256, "efficientnet_b0": 224}  # the classifier definitions and their default input size
NMS_KINDS = ("default", "greedynms")  # [yolo] nms_kind values that are the decode's greedy NMS
DIOU_KINDS = ("diounms",)             # ... and those that are its DIoU NMS (yolo_post.MultiHead's nms_kind "diou")


class DarknetError(ValueError):
    """A cfg or weight file this importer cannot read, or a layer it cannot express."""


# ------------------------------------------------------------------------------------- cfg text
def parse_cfg(text, activations=BASE_ACTIVATIONS, section_types=BASE_SECTION_TYPES):
    """The sections of a Darknet cfg, in order: one dict per section with "type" (the name in
    brackets), "line" (its 1-based line number) and every `key = value` of the section as strings
    (keys and values stripped; a key named `type` or `line`, as in [cost]'s `type = sse`, is kept as
    "type_" / "line_").  `#` and `;` start comment lines; blank lines are skipped.  A
    section type outside `section_types` raises DarknetError naming the type and the line; unknown
    keys inside a known section are kept and ignored by the importer.  Like `activations` below, the
    default is what every walker of the sections knows: [reorg] and [region] pass only when the caller
    names them (SECTION_TYPES, as DarknetModel does), since code that walks the sections itself would
    take a [reorg] it does not know for a layer that changes nothing.

    `activations`: the `activation` values a [convolutional] (Darknet's default there: logistic) or a
    [shortcut] (default linear) may have; any other raises DarknetError naming the value and the line.
    The default is leaky and linear, what every reader of these sections computes: code that walks
    the sections itself and knows only those two would take a mish layer for a linear one without
    a word.  DarknetModel parses with ACTIVATIONS; so does a caller whose own code handles mish,
    swish and logistic."""
    sections = []
    for no, raw in enumerate(text.splitlines(), start=1):
        line = raw.strip()
        if not line or line[0] in "#;":
            continue
        if line[0] == "[":
            if line[-1] != "]":
                raise DarknetError(f"line {no}: malformed section header {line!r}")
            kind = line[1:-1].strip()
            if kind not in section_types:
                raise DarknetError(f"line {no}: section type [{kind}] is not supported "
                                   f"(supported: {', '.join(section_types)})")
            sections.append({"type": kind, "line": no})
            continue
        if "=" not in line:
            raise DarknetError(f"line {no}: expected `key = value`, got {line!r}")
        if not sections:
            raise DarknetError(f"line {no}: `{line}` before the first section")
        key, value = line.split("=", 1)
        key = key.strip()
        if key in ("type", "line"):  # ([cost] has `type = sse`: kept beside the section's own "type")
            key += "_"
        sections[-1][key] = value.strip()
    if not sections or sections[0]["type"] != "net":
        raise DarknetError("a cfg starts with a [net] section")
    if any(s["type"] == "net" for s in sections[1:]):
        raise DarknetError("more than one [net] section")
    for sec in sections:
        if sec["type"] in ("convolutional", "shortcut"):
            act = sec.get("activation", "logistic" if sec["type"] == "convolutional" else "linear")
            if act not in activations:
                raise DarknetError(f"[{sec['type']}] at line {sec['line']}: activation {act!r} is not supported "
                                   f"({', '.join(activations)})")
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
    if act not in ACTIVATIONS:
        raise DarknetError(f"{where}: activation {act!r} is not supported ({', '.join(ACTIVATIONS)})")
    if n < 1 or size < 1 or stride < 1 or not 0 <= pad < size:
        raise DarknetError(f"{where}: filters {n}, size {size}, stride {stride}, padding {pad}: need filters, size, "
                           "stride >= 1 and 0 <= padding < size")
    return n, size, stride, pad, bool(_int(sec, "batch_normalize", 0)), act


def conv_groups(sec, c):
    """`groups` of a [convolutional] section on `c` input channels (default 1): above 1 a grouped
    conv, one dnn_plan_add_conv_grouped entry whose Darknet weights are [n][c / groups][size][size].
    DarknetError when it does not divide the input channels or `filters`."""
    groups, n = _int(sec, "groups", 1), _int(sec, "filters")
    if groups < 1 or c % groups or n % groups:
        raise DarknetError(f"[convolutional] at line {sec['line']}: grouped conv with groups = {groups} needs "
                           f"groups >= 1 dividing the {c} input channels and the {n} filters")
    return groups


def shortcut_activation(sec):
    """activation of a [shortcut] section (default linear): linear, mish, swish or logistic."""
    act = sec.get("activation", "linear")
    if act not in ACTIVATIONS or act == "leaky":
        raise DarknetError(f"[shortcut] at line {sec['line']}: activation {act!r} is not supported "
                           "(linear, mish, swish, logistic)")
    return act


def _activated(g, t, act):
    """The node of `act` applied to node t: the fp32 leaky, one of dnn_hip.ACTIVATIONS, or t itself (linear)."""
    if act == "leaky":
        return g.create_leaky_relu_f32(t)
    return t if act == "linear" else g.create_activation(t, act)


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


def yolo_rule(sec, before=None):
    """(new_coords, nms_kind, beta_nms) of a [yolo] section as yolo_post.MultiHead takes them: new_coords
    0 or 1, nms_kind "iou" (Darknet's default and greedynms) or "diou" (diounms, accepted beside
    new_coords = 1 only) with beta_nms (default 0.6; read under diounms only, as every other kind
    ignores it).  `before`, the section the [yolo] follows, is checked where given: with new_coords = 1
    Darknet reads the conv's values as they are, so that conv must be activation = logistic."""
    where = f"[yolo] at line {sec['line']}"
    new_coords = _int(sec, "new_coords", 0)
    if new_coords not in (0, 1):
        raise DarknetError(f"{where}: new_coords = {sec['new_coords']} is not supported (0 or 1)")
    if new_coords and before is not None and before.get("activation", "logistic") != "logistic":
        raise DarknetError(f"{where}: new_coords = 1 after a [convolutional] with activation = "
                           f"{before.get('activation')}: Darknet reads raw values there, the conv must be logistic")
    kind = sec.get("nms_kind", "default")
    if kind not in NMS_KINDS + DIOU_KINDS:
        raise DarknetError(f"{where}: nms_kind = {kind} is not supported ({', '.join(NMS_KINDS + DIOU_KINDS)})")
    if kind in DIOU_KINDS and not new_coords:
        # what the importer did before it read the scaled heads stays as it was: DIoU NMS is read with
        # new_coords = 1 only (yolo_post.MultiHead itself takes nms_kind "diou" with either box form)
        raise DarknetError(f"{where}: nms_kind = {kind} without new_coords = 1 is not supported (the DIoU NMS is "
                           "imported for the scaled-YOLOv4 head only)")
    if kind not in DIOU_KINDS:
        return bool(new_coords), "iou", 0.6
    try:
        beta = float(sec.get("beta_nms", 0.6))
    except ValueError:
        raise DarknetError(f"{where}: beta_nms = {sec['beta_nms']!r} is not a number")
    if not (beta > 0 and beta < float("inf")):
        raise DarknetError(f"{where}: beta_nms = {beta}: need a finite value > 0")
    return bool(new_coords), "diou", beta


def yolo_params(sec):
    """scale_x_y (default 1) of a [yolo] section."""
    where = f"[yolo] at line {sec['line']}"
    try:
        s = float(sec.get("scale_x_y", 1))
    except ValueError:
        raise DarknetError(f"{where}: scale_x_y = {sec['scale_x_y']!r} is not a number")
    if not (s > 0 and s < float("inf")):
        raise DarknetError(f"{where}: scale_x_y = {s}: need a finite value > 0")
    return s


def reorg_params(sec, in_h, in_w, in_c):
    """stride (default 1) of a [reorg] section on an in_h x in_w x in_c map: the non-reverse forward only.
    DarknetError naming the key for reverse = 1, flatten = 1 or extra, and for a map the stride does not divide."""
    where = f"[reorg] at line {sec['line']}"
    for key in ("reverse", "flatten", "extra"):
        if _int(sec, key, 0):
            raise DarknetError(f"{where}: {key} = {sec[key]} is not supported (the plain forward reorg only)")
    s = _int(sec, "stride", 1)
    if not 1 <= s <= dnn_hip.MAX_ROUTE_BLOCK:
        raise DarknetError(f"{where}: stride {s} outside 1..{dnn_hip.MAX_ROUTE_BLOCK}")
    if in_h % s or in_w % s or in_c % (s * s):
        raise DarknetError(f"{where}: stride {s} does not divide the {in_h} x {in_w} map, or stride^2 its {in_c} channels")
    return s


def region_params(sec, before=None):
    """(num, classes, anchors) of a [region] section the one-scale softmax decode computes: coords = 4,
    softmax = 1, num (default 1) pairs in `anchors`, at most yolo_post.MAX_ANCHORS of them and
    yolo_post.MAX_CLASSES classes.  softmax_tree, background = 1 and classfix (YOLO9000's forms) raise
    DarknetError naming the key.  `before`, the section the [region] follows, is checked where given: a
    [convolutional] with filters = num * (5 + classes) and activation = linear."""
    where = f"[region] at line {sec['line']}"
    if "softmax_tree" in sec:
        raise DarknetError(f"{where}: softmax_tree = {sec['softmax_tree']} (YOLO9000's class tree) is not supported")
    for key in ("background", "classfix"):
        if _int(sec, key, 0):
            raise DarknetError(f"{where}: {key} = {sec[key]} is not supported")
    if _int(sec, "coords", 4) != 4:
        raise DarknetError(f"{where}: coords = {sec['coords']} is not supported (only 4)")
    if _int(sec, "softmax", 0) != 1:
        raise DarknetError(f"{where}: softmax = {sec.get('softmax', 0)} is not supported (only 1: softmax class scores)")
    num, classes = _int(sec, "num", 1), _int(sec, "classes", 20)
    try:
        anchors = tuple(float(v) for v in sec["anchors"].split(",") if v.strip())
    except (KeyError, ValueError):
        raise DarknetError(f"{where}: `anchors` is missing or not a list of numbers")
    if not 1 <= num <= yolo_post.MAX_ANCHORS or len(anchors) != 2 * num:
        raise DarknetError(f"{where}: num = {num} with {len(anchors)} anchor values: need num (w, h) pairs, num in "
                           f"1..{yolo_post.MAX_ANCHORS} (DNN_YOLO_MAX_ANCHORS)")
    if not 1 <= classes <= yolo_post.MAX_CLASSES:
        raise DarknetError(f"{where}: classes = {classes}: need 1..{yolo_post.MAX_CLASSES} (DNN_YOLO_MAX_CLASSES)")
    if before is not None:
        if before["type"] != "convolutional":
            raise DarknetError(f"{where}: it must follow a [convolutional] section")
        if _int(before, "filters") != num * (5 + classes) or before.get("activation", "logistic") != "linear":
            raise DarknetError(f"{where}: the [convolutional] before it has filters = {before.get('filters')}, activation "
                               f"= {before.get('activation', 'logistic')}: need filters = num * (5 + classes) = "
                               f"{num * (5 + classes)} and activation = linear")
    return num, classes, anchors


def connected_params(sec, in_h, in_w):
    """(output, batch_normalize, activation) of a [connected] section on an in_h x in_w map.  Darknet
    flattens its input as CHW and this engine's tensors are NHWC, so only a 1 x 1 map (after an
    [avgpool]) has the same element order in both; anything else raises DarknetError."""
    where = f"[connected] at line {sec['line']}"
    n = _int(sec, "output")
    act = sec.get("activation", "logistic")
    if act not in ("leaky", "linear"):
        raise DarknetError(f"{where}: activation {act!r} is not supported (leaky, linear)")
    if n < 1:
        raise DarknetError(f"{where}: output = {n}: need >= 1")
    if (in_h, in_w) != (1, 1):
        raise DarknetError(f"{where}: its input is {in_h} x {in_w}: only a 1 x 1 map is supported (Darknet flattens "
                           "channels first, the engine's tensors are channels last)")
    return n, bool(_int(sec, "batch_normalize", 0)), act


def softmax_params(sec, in_h, in_w):
    """Refuses what the softmax kernel does not compute: groups other than 1, a temperature other
    than 1, a tree, an input that is not 1 x 1 spatially."""
    where = f"[softmax] at line {sec['line']}"
    if _int(sec, "groups", 1) != 1:
        raise DarknetError(f"{where}: groups = {sec['groups']} is not supported (only 1)")
    try:
        temperature = float(sec.get("temperature", 1))
    except ValueError:
        raise DarknetError(f"{where}: temperature = {sec['temperature']!r} is not a number")
    if temperature != 1:
        raise DarknetError(f"{where}: temperature = {temperature} is not supported (only 1)")
    if "tree" in sec:
        raise DarknetError(f"{where}: tree = {sec['tree']} (a hierarchical softmax) is not supported")
    if (in_h, in_w) != (1, 1):
        raise DarknetError(f"{where}: its input is {in_h} x {in_w}: only a 1 x 1 map is supported (put an [avgpool] "
                           "before it)")


def se_block(sections, at):
    """The squeeze-and-excitation block that the [scale_channels] section at layer `at` closes: the layer index of
    its input x.  The one supported form is

        x, [avgpool], [convolutional] 1x1 stride 1, [convolutional] 1x1 stride 1, [scale_channels] from = x

    with activation = linear and no scale_wh on the closing section, groups = 1 on both convs and `from` naming the
    layer right before the [avgpool].  Anything else (a gate of another depth, a `from` elsewhere, scale_wh = 1,
    Darknet's [sam]) raises DarknetError with the line and the rule."""
    sec = sections[at + 1]
    where = f"[scale_channels] at line {sec['line']} (layer {at})"
    rule = ("it is supported only as the end of a squeeze-and-excitation block: [avgpool], two 1x1 stride-1 "
            "[convolutional] sections, then [scale_channels] with `from` naming the [avgpool]'s input")
    if _int(sec, "scale_wh", 0):
        raise DarknetError(f"{where}: scale_wh = {sec['scale_wh']} (a spatial gate) is not supported; {rule}")
    if sec.get("activation", "linear") != "linear":
        raise DarknetError(f"{where}: activation {sec['activation']!r} is not supported (linear only); {rule}")
    src = _layer_index(sec, _int(sec, "from"), at, "from")
    kinds = [s["type"] for s in sections[max(at - 2, 1):at + 1]]  # the three layers before this one
    if at < 4 or kinds != ["avgpool", "convolutional", "convolutional"]:
        raise DarknetError(f"{where}: the three layers before it are {kinds}; {rule}")
    if src != at - 4:
        raise DarknetError(f"{where}: from = {sec['from']} names layer {src}, the [avgpool]'s input is layer {at - 4}; {rule}")
    for conv in sections[at - 1:at + 1]:
        _, size, stride, _, _, _ = conv_params(conv)
        if size != 1 or stride != 1 or _int(conv, "groups", 1) != 1:
            raise DarknetError(f"{where}: the [convolutional] at line {conv['line']} has size {size}, stride {stride}, "
                               f"groups {_int(conv, 'groups', 1)}; {rule}")
    return src


def layer_shapes(sections, in_shape=None):
    """Per layer (every section after [net]) its output's (h, w, c), walking the cfg as Darknet's
    parser does; raises DarknetError for a section that does not fit its input."""
    h, w, c = net_shape(sections, in_shape)
    shapes = []
    for at, sec in enumerate(sections[1:]):
        kind = sec["type"]
        if kind == "convolutional":
            n, size, stride, pad, _, _ = conv_params(sec)
            conv_groups(sec, c)
            if h + 2 * pad < size or w + 2 * pad < size:
                raise DarknetError(f"[convolutional] at line {sec['line']}: a {size}x{size} kernel on a "
                                   f"{h} x {w} map with padding {pad} has no output")
            h, w, c = (h + 2 * pad - size) // stride + 1, (w + 2 * pad - size) // stride + 1, n
        elif kind == "shortcut":
            shortcut_activation(sec)
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
            yolo_rule(sec, sections[at])
        elif kind == "reorg":
            s = reorg_params(sec, h, w, c)
            h, w, c = h // s, w // s, c * s * s
        elif kind == "region":
            if at + 2 != len(sections):
                raise DarknetError(f"[region] at line {sec['line']}: it must be the last section of the cfg")
            region_params(sec, sections[at] if at else {"type": "net"})
        elif kind == "avgpool":
            h, w = 1, 1
        elif kind == "scale_channels":
            src = shapes[se_block(sections, at)]
            if (h, w, c) != (1, 1, src[2]) or not 1 <= shapes[at - 2][2] <= dnn_hip.SE_MAX_CR or c > dnn_hip.SE_MAX_C:
                raise DarknetError(f"[scale_channels] at line {sec['line']}: a {h} x {w} x {c} gate (squeezed width "
                                   f"{shapes[at - 2][2]}) on a {src} tensor: need 1 x 1 x {src[2]}, at most "
                                   f"{dnn_hip.SE_MAX_C} channels and a squeezed width of at most {dnn_hip.SE_MAX_CR}")
            h, w, c = src
        elif kind == "softmax":
            softmax_params(sec, h, w)
            if c > dnn_hip.SOFTMAX_MAX_CLASSES:
                raise DarknetError(f"[softmax] at line {sec['line']}: {c} classes, at most {dnn_hip.SOFTMAX_MAX_CLASSES}")
        elif kind == "connected":
            c = connected_params(sec, h, w)[0]
        # (dropout and cost: layers that compute nothing at inference; the tensor passes through)
        shapes.append((h, w, c))
    return shapes


def conv_shapes(sections):
    """Per [convolutional] section in cfg order: (filters, input channels, size, batch_normalize),
    the input channels being those of one group (c / groups: the weights' second axis).
    (Channel counts do not depend on the input size.)"""
    net = sections[0]
    shapes = layer_shapes(sections, [1, max(_int(net, "height"), 1), max(_int(net, "width"), 1), _int(net, "channels", 3)])
    out = []
    c_in = _int(net, "channels", 3)
    for sec, shape in zip(sections[1:], shapes):
        if sec["type"] == "convolutional":
            n, size, _, _, bn, _ = conv_params(sec)
            out.append((n, c_in // conv_groups(sec, c_in), size, bn))
        c_in = shape[2]
    return out


def weight_shapes(sections):
    """Per section with weights, [convolutional] and [connected], in cfg order: (kind, filters or
    outputs, input channels, size, batch_normalize): conv_shapes' tuples behind the section type,
    a [connected] with size 0 (its weights are [outputs][inputs])."""
    net = sections[0]
    shapes = layer_shapes(sections, [1, max(_int(net, "height"), 1), max(_int(net, "width"), 1), _int(net, "channels", 3)])
    convs = iter(conv_shapes(sections))
    out = []
    c_in = _int(net, "channels", 3)
    for sec, shape in zip(sections[1:], shapes):
        if sec["type"] == "convolutional":
            out.append(("convolutional",) + next(convs))
        elif sec["type"] == "connected":
            out.append(("connected", shape[2], c_in, 0, bool(_int(sec, "batch_normalize", 0))))
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

    for k, (kind, n, c, size, bn) in enumerate(weight_shapes(sections)):
        start = at
        fc = kind == "connected"
        w_count, w_shape = (n * c, (n, c)) if fc else (n * c * size * size, (n, c, size, size))
        try:
            layer = {"biases": take(n, (n,), "biases")}
            if fc:  # load_connected_weights: the weights come before the BatchNorm vectors
                layer["weights"] = take(w_count, w_shape, "weights")
            if bn:
                for key in ("scales", "rolling_mean", "rolling_variance"):
                    layer[key] = take(n, (n,), key)
            if not fc:
                layer["weights"] = take(w_count, w_shape, "weights")
        except EOFError as e:
            if partial:
                at = start
                break
            raise DarknetError(f"{path}: the file ends inside the {e} of {kind} layer {k} "
                               f"({n} filters of {' x '.join(map(str, w_shape[1:]))}): {len(data)} bytes, at least "
                               f"{start + 4 * ((4 if bn else 1) * n + w_count)} expected")
        out.append(layer)
    if at != len(data) and not partial:
        raise DarknetError(f"{path}: {len(data) - at} bytes left after the last convolutional layer "
                           "(the cfg does not match the file)")
    return out


def save_weights(path, layers, major=0, minor=2, revision=0, seen=0):
    """Write `layers` (dicts as load_weights returns them, in cfg order) as a Darknet weight file.  A
    layer whose weights are 2-D, [outputs][inputs], is a [connected] layer and is written in
    save_connected_weights' order: biases, weights, then the BatchNorm vectors."""
    with open(path, "wb") as f:
        f.write(struct.pack("<3i", major, minor, revision))
        f.write(struct.pack("<q" if _header_seen_bytes(major, minor) == 8 else "<i", seen))
        for k, layer in enumerate(layers):
            w = np.asarray(layer["weights"])
            if w.ndim != 2 and (w.ndim != 4 or w.shape[2] != w.shape[3]):
                raise DarknetError(f"layer {k}: weights of shape {w.shape}, [n][c][size][size] (or a connected layer's "
                                   "[outputs][inputs]) expected")
            keys = ("biases",) + (("scales", "rolling_mean", "rolling_variance") if "scales" in layer else ())
            for key in keys:
                a = np.asarray(layer[key])
                if a.shape != (w.shape[0],):
                    raise DarknetError(f"layer {k}: {key} of shape {a.shape}, ({w.shape[0]},) expected")
                f.write(np.ascontiguousarray(a, dtype="<f4").tobytes())
                if key == "biases" and w.ndim == 2:
                    f.write(np.ascontiguousarray(w, dtype="<f4").tobytes())
            if w.ndim == 4:
                f.write(np.ascontiguousarray(w, dtype="<f4").tobytes())


def kernel_hwio(layer):
    """A layer's Darknet weights [n][c][kh][kw] as the engine's HWIO kernel [kh][kw][c][n]; a
    connected layer's [outputs][inputs] as the 1x1 kernel [1][1][inputs][outputs]."""
    w = np.asarray(layer["weights"], np.float32)
    if w.ndim == 2:
        w = w[:, :, None, None]
    return np.ascontiguousarray(w.transpose(2, 3, 1, 0))


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
    """`layers` (load_weights' format) against the cfg's conv and connected shapes: DarknetError on
    a mismatch."""
    shapes = weight_shapes(sections)
    if len(layers) != len(shapes):
        raise DarknetError(f"{len(layers)} weight layers for {len(shapes)} [convolutional] sections")
    for k, (layer, (kind, n, c, size, bn)) in enumerate(zip(layers, shapes)):
        keys = ("biases", "weights") + (("scales", "rolling_mean", "rolling_variance") if bn else ())
        if any(key not in layer for key in keys):
            raise DarknetError(f"{kind} layer {k}: expected a dict with {keys}")
        want = (n, c) if kind == "connected" else (n, c, size, size)
        if tuple(np.asarray(layer["weights"]).shape) != want:
            raise DarknetError(f"{kind} layer {k}: weights of shape {np.asarray(layer['weights']).shape}, "
                               f"{want} expected")


# ------------------------------------------------------------------------------------- the graph
class _LazyPool(object):
    """A stride-1 odd-size [maxpool]: a MaxPool2D node when something reads it, a block of an Spp
    node when a four-layer [route] reads it beside its own input."""

    def __init__(self, src, size):
        self.src, self.size, self.node = src, size, None


class _SePart(object):
    """A layer inside a squeeze-and-excitation block (its [avgpool] or one of its two convs, with that conv's
    weights): no node of its own, and nothing but the block's [scale_channels] may read it."""

    def __init__(self, sec, layer):
        self.sec, self.layer = sec, layer


def _se_fc(layer):
    """(matrix [inputs, outputs], bias [outputs]) fp32 of a 1x1 conv on a 1 x 1 map as one of the gate's two small
    matrices: y = x @ matrix + bias.  A folded BatchNorm's per-output scale (fold_batchnorm) goes into the matrix's
    columns, in float64 and rounded once; without BatchNorm the matrix is the conv's weights as they are."""
    scale, shift = fold_batchnorm(layer)
    w = kernel_hwio(layer)[0, 0]
    if "scales" in layer:
        w = (w.astype(np.float64) * scale.astype(np.float64)).astype(np.float32)
    return np.ascontiguousarray(w), shift


def build_graph(builder_cls, sections, layers, in_shape):
    """Return (graph, outs, yolos): outs the head nodes (the conv before each [yolo], in cfg
    order; all but the last are the graph's extra outputs, the last its primary one), yolos the
    [yolo] sections with "grid" = that tensor's (h, w).  A cfg without [yolo] (a classifier ending
    in [softmax], or any prefix of a network as a feature extractor) has one output, the last
    tensor computed, and no yolos.  `layers` is load_weights' list."""
    check_layers(sections, layers)
    shapes = layer_shapes(sections, in_shape)
    g = builder_cls()
    x = g.create_input([int(v) for v in in_shape])
    out = []       # per layer: a node or a _LazyPool; a one-layer route repeats its source's object
    outs, yolos = [], []
    weights = iter(layers)

    # the [avgpool] and the two convs of every squeeze-and-excitation block: layers that exist only inside the
    # SqueezeExcite node their [scale_channels] makes (se_block has checked the pattern in layer_shapes)
    se_parts = {k for at, sec in enumerate(sections[1:]) if sec["type"] == "scale_channels" for k in (at - 3, at - 2, at - 1)}

    def node(v):
        if isinstance(v, _SePart):
            raise DarknetError(f"[{v.sec['type']}] at line {v.sec['line']} is inside a squeeze-and-excitation block: only "
                               "the block's [scale_channels] may read it")
        if isinstance(v, _LazyPool):
            if v.node is None:
                v.node = g.create_max_pool2d(node(v.src), [1, v.size, v.size, 1], [1, 1, 1, 1], "SAME")
            return v.node
        return v

    prev = x
    c_in = int(in_shape[3])
    for at, sec in enumerate(sections[1:]):
        kind = sec["type"]
        if at in se_parts:  # (its conv's weights are read here, in file order like any conv's)
            cur = _SePart(sec, next(weights) if kind == "convolutional" else None)
        elif kind == "scale_channels":
            fc1, fc2 = out[at - 2], out[at - 1]
            (w1, b1), (w2, b2) = _se_fc(fc1.layer), _se_fc(fc2.layer)
            cur = g.create_squeeze_excite(node(out[se_block(sections, at)]), w1, b1, conv_params(fc1.sec)[5],
                                          w2, b2, conv_params(fc2.sec)[5])
        elif kind == "convolutional":
            n, size, stride, pad, _, act = conv_params(sec)
            layer = next(weights)
            scale, shift = fold_batchnorm(layer)
            t = g.create_conv2d_padded(node(prev), kernel_hwio(layer), [1, stride, stride, 1], (pad, pad),
                                       groups=conv_groups(sec, c_in))
            t = g.create_scale_shift(t, scale, shift)
            cur = _activated(g, t, act)
        elif kind == "shortcut":
            src = out[_layer_index(sec, _int(sec, "from"), at, "from")]
            cur = _activated(g, g.create_add([node(src), node(prev)]), shortcut_activation(sec))
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
        elif kind == "reorg":
            h, w, c = shapes[at - 1] if at else net_shape(sections, in_shape)
            cur = g.create_reorg(node(prev), reorg_params(sec, h, w, c))
        elif kind == "avgpool":
            cur = g.create_global_avg_pool(node(prev))
        elif kind == "softmax":
            cur = g.create_softmax(node(prev))
        elif kind == "connected":  # on a 1 x 1 map (connected_params): a 1x1 conv of [outputs][inputs]
            _, _, act = connected_params(sec, 1, 1)
            layer = next(weights)
            scale, shift = fold_batchnorm(layer)
            t = g.create_conv2d_padded(node(prev), kernel_hwio(layer), [1, 1, 1, 1], (0, 0))
            t = g.create_scale_shift(t, scale, shift)
            cur = g.create_leaky_relu_f32(t) if act == "leaky" else t
        elif kind in ("dropout", "cost"):  # a layer for [route] / [shortcut] indices, nothing at inference
            cur = prev
        else:  # yolo / region: the conv before it is an output; the layer itself repeats that tensor
            outs.append(node(prev))
            yolos.append(dict(sec, grid=shapes[at][:2]))
            cur = prev
        out.append(cur)
        prev = cur
        c_in = shapes[at][2]
    if not outs:  # a classifier or a feature extractor: the last tensor computed is the output
        if prev is x:
            raise DarknetError("the cfg has no layer that computes: nothing to output")
        g.set_out_node(node(prev))
        return g, [node(prev)], []
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
        gh, gw = y["grid"]
        if in_h % gh or in_w % gw or in_h // gh != in_w // gw:
            raise DarknetError(f"[{y['type']}] at line {y['line']}: a {gh} x {gw} grid does not divide the {in_h} x {in_w} "
                               "input into square cells")
        stride = in_h // gh
        if y["type"] == "region":  # its anchors are in cells already, the unit of the decode
            num, classes, anchors = region_params(y)
            scales.append(yolo_post.Scale(gh, gw, num, classes, anchors, float(stride), score_thr, iou_thr))
            continue
        xy.append(yolo_params(y))
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
    if [y["type"] for y in yolos] == ["region"]:
        return (yolo_post.WideHead if wide else yolo_post.MultiHead)(scales, "softmax", nms, labels)
    kw = {} if all(s == 1.0 for s in xy) else {"scale_x_y": tuple(xy)}
    rules = [yolo_rule(y) for y in yolos]
    for y, r in zip(yolos, rules):  # one decode and one NMS serve every scale (beta_nms matters under DIoU only)
        if r != rules[0]:
            raise DarknetError(f"[yolo] at line {y['line']}: new_coords, nms_kind, beta_nms = {r}; the first [yolo] "
                               f"has {rules[0]} (all sections must agree)")
    if rules and (rules[0][0] or rules[0][1] != "iou"):
        kw.update(new_coords=rules[0][0], nms_kind=rules[0][1], beta_nms=rules[0][2])
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
        self.sections = parse_cfg(cfg_text, ACTIVATIONS, SECTION_TYPES)
        h, w, c = net_shape(self.sections, in_shape)
        self.in_shape = (int(in_shape[0]) if in_shape is not None else 1, h, w, c)
        self.layers = load_weights(weights, self.sections) if isinstance(weights, (str, bytes)) or hasattr(
            weights, "__fspath__") else list(weights)
        self.g, self.outs, self.yolos = build_graph(dnn_hip.DnnGraphBuilder, self.sections, self.layers, self.in_shape)
        self._head_error = None
        self._cls = None  # classify's device tensors and its TopK, made on first use
        if not self.yolos:
            if head is not _AUTO and head is not None:
                raise ValueError("the cfg has no [yolo] section: there is nothing for a head to decode")
            head, self._head_error = None, "the cfg has no [yolo] section: the model has no detection head"
        if head is _AUTO:
            try:
                head = multi_head(self.yolos, h, w, score_thr, iou_thr, nms, labels, wide)
            except DarknetError:
                raise
            except ValueError as e:
                boxes = sum(y["grid"][0] * y["grid"][1] * (_int(y, "num", 1) if y["type"] == "region" else
                                                           len(_ints(y, "mask")) if "mask" in y else 1)
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
        self._ingest = {}  # detect_images' RaggedIngest per pixel order, detect_frames_nv12's per matrix

    def _need_head(self):
        if self.head is None:
            raise ValueError(self._head_error or "the model was built with head=None: pass head=")

    def inference(self, im):
        """One tensor per [yolo] section, in cfg order; for a cfg without [yolo] the one output
        tensor itself (a classifier's [n, 1, 1, classes] probabilities)."""
        outs = super().inference(im)
        return outs if self.yolos else outs[0]

    def classify(self, frames, k=5, raise_errors=True):
        """(indices [n, k] int32, probabilities [n, k] fp32) of a classifier cfg for [n <= batch, h, w,
        c] fp32 frames already at the network's size (Darknet's resize and centre crop are the
        caller's): the plan, then the top-k of its [n, 1, 1, classes] output on the device
        (classify.TopK), best class first, equal scores in index order.  An image whose scores hold
        a NaN raises ValueError, or with raise_errors=False gets index -1 and NaN."""
        import torch
        import classify as topk
        plan = self.sess.plan()
        if self.yolos or plan.out_shape[:2] != (1, 1):
            raise ValueError(f"classify needs a cfg without [yolo] that ends in a 1 x 1 map, this one's output is "
                             f"{plan.out_shape}" + (" with [yolo] sections" if self.yolos else ""))
        x = np.ascontiguousarray(frames, dtype=np.float32)
        n = x.shape[0]
        if tuple(x.shape[1:]) != plan.in_shape or n > plan.batch:
            raise ValueError(f"frames {x.shape} do not fit plan [{plan.batch}, {plan.in_shape}]")
        device = torch.device("cuda", plan.device)
        if self._cls is None or self._cls["topk"].k != int(k):
            self._cls = {"in": torch.empty((plan.batch,) + plan.in_shape, dtype=torch.float32, device=device),
                         "out": torch.empty((plan.batch,) + plan.out_shape, dtype=torch.float32, device=device),
                         "topk": topk.TopK(plan.batch, plan.out_shape[2], k, device)}
        d, tk = self._cls, self._cls["topk"]
        with torch.cuda.device(device):
            stream = torch.cuda.current_stream().cuda_stream
            d["in"][:n].copy_(torch.from_numpy(x))
            plan.run_device(n, d["in"].data_ptr(), d["out"].data_ptr(), stream)
            tk.run(d["out"].data_ptr(), n, stream)
            host = [t[:n].cpu().numpy() for t in (tk.index, tk.score, tk.status)]
        return topk.TopK.to_rows(*host, raise_errors=raise_errors)

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
        import ingest
        self._need_head()
        images = list(images)
        batch, net_hw = self.in_shape[0], self.in_shape[1:3]
        if self.in_shape[3] != 3:
            raise ValueError(f"detect_images needs a 3-channel network, [net] has channels = {self.in_shape[3]}")
        if order not in ingest.PIXEL_ORDERS:
            raise ValueError(f"order {order!r}: need one of {sorted(ingest.PIXEL_ORDERS)}")
        _, _, sizes, nbytes = ingest.ragged_layout(images, batch, 1 << 62, net_hw)  # (raises before any device work)
        return self._detect_ingested(order, dict(order=order), images, sizes, nbytes, raise_errors)

    def detect_frames_nv12(self, frames, matrix="bt601_limited", raise_errors=True):
        """detect_images for decoder surfaces: up to `batch` NV12 frames of any sizes, each a
        (y [H, W], uv [(H + 1) // 2, (W + 1) // 2, 2]) pair of uint8 arrays, converted to RGB under
        `matrix` (ingest.YUV_MATRICES; include/dnn_hip_ingest.h has the integer conversion) and
        letterboxed in one kernel (dnn_letterbox_frames_nv12).  The rows are those of detect_images on
        the RGB image that conversion gives, in each frame's own pixels."""
        import ingest
        self._need_head()
        frames = list(frames)
        batch, net_hw = self.in_shape[0], self.in_shape[1:3]
        if self.in_shape[3] != 3:
            raise ValueError(f"detect_frames_nv12 needs a 3-channel network, [net] has channels = {self.in_shape[3]}")
        ingest._matrix(matrix)
        _, _, sizes, nbytes = ingest.nv12_layout(frames, batch, 1 << 62, net_hw)  # (raises before any device work)
        return self._detect_ingested(("nv12", matrix), dict(pixel_format="nv12", matrix=matrix), frames, sizes, nbytes,
                                     raise_errors)

    def _detect_ingested(self, key, ingest_kw, images, sizes, nbytes, raise_errors):
        """detect_images' device part: upload + letterbox into the plan's input through the
        RaggedIngest kept under `key`, the plan, the decode, the correction."""
        import torch
        import ingest
        batch, net_hw = self.in_shape[0], self.in_shape[1:3]
        n = len(images)
        plan = self.sess.plan()
        device = torch.device("cuda", plan.device)
        d = self._device_buffers(plan, device)
        with torch.cuda.device(device):
            compute = torch.cuda.current_stream()
            stream = compute.cuda_stream
            ing = self._ingest.get(key)
            if ing is None or ing.max_bytes < nbytes or ing.compute != compute:
                ing = ingest.RaggedIngest(batch, max(nbytes, 1), net_hw, device, compute, **ingest_kw)
                self._ingest[key] = ing
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

    def conv(self, filters, size, stride=1, head=False, act="leaky"):
        if head:  # a conv with a bias, 3 x (5 + classes) filters whatever the width: linear, or logistic as given
            pairs = [("size", size), ("stride", stride), ("pad", 1), ("filters", filters),
                     ("activation", "logistic" if act == "logistic" else "linear")]
        else:
            pairs = [("batch_normalize", 1), ("filters", self.wd(filters)), ("size", size), ("stride", stride),
                     ("pad", 1), ("activation", act)]
        return self.add("convolutional", *pairs)

    def yolo(self, mask, anchors, classes):
        return self.add("yolo", ("mask", mask), ("anchors", anchors), ("classes", classes),
                        ("num", len(anchors.split(",")) // 2), ("jitter", ".3"), ("ignore_thresh", ".7"),
                        ("truth_thresh", 1), ("random", 1))

    def yolo_v4(self, mask, anchors, classes, scale_x_y="1.05", scaled=False):
        return self.add("yolo", ("mask", mask), ("anchors", anchors), ("classes", classes),
                        ("num", len(anchors.split(",")) // 2), ("jitter", ".3"), ("scale_x_y", scale_x_y),
                        ("cls_normalizer", "1.0"), ("iou_normalizer", "0.07"), ("iou_loss", "ciou"),
                        ("ignore_thresh", ".7"), ("truth_thresh", 1), ("random", 0), ("resize", "1.5"),
                        ("nms_kind", "diounms" if scaled else "greedynms"), ("beta_nms", "0.6"),
                        *((("new_coords", 1),) if scaled else ()))

    def region(self, anchors, classes):
        return self.add("region", ("anchors", anchors), ("bias_match", 1), ("classes", classes), ("coords", 4),
                        ("num", len(anchors.split(",")) // 2), ("softmax", 1), ("jitter", ".3"), ("rescore", 1),
                        ("object_scale", 5), ("noobject_scale", 1), ("class_scale", 1), ("coord_scale", 1),
                        ("absolute", 1), ("thresh", " .6"), ("random", 1))

    def text(self):
        return "\n".join(self.lines)


# [region] anchors, in cells of the 13 x 13 grid: yolov2.cfg and yolov2-tiny.cfg (COCO), yolov2-voc.cfg, yolov2-tiny-voc.cfg
_V2_COCO_ANCHORS = "0.57273, 0.677385, 1.87446, 2.06253, 3.33843, 5.47434, 7.88282, 3.52778, 9.77052, 9.16828"
_V2_VOC_ANCHORS = "1.3221, 1.73145, 3.19275, 4.00944, 5.05587, 8.09892, 9.47112, 4.84053, 11.2364, 10.0071"
_V2_TINY_VOC_ANCHORS = "1.08,1.19,  3.42,4.41,  6.63,11.38,  9.42,5.11,  16.62,10.52"
_V4_ANCHORS = "12, 16, 19, 36, 40, 28, 36, 75, 76, 55, 72, 146, 142, 110, 192, 243, 459, 401"


def _yolov4(c, n_out, classes, scaled=False):
    """YOLOv4: CSPDarknet53 with mish, the SPP + PAN neck with leaky, three heads from the finest scale up.
    scaled: the heads of the scaled-YOLOv4 cfgs on that topology (logistic head convs, new_coords,
    scale_x_y 2.0, DIoU NMS)."""
    def mish(filters, size, stride=1):
        return c.conv(filters, size, stride, act="mish")

    mish(32, 3)
    stage_out = []
    for k, (f, blocks) in enumerate(_STAGES):  # a CSP stage: down, B = 1x1(down); A = 1x1(down), blocks, 1x1; 1x1 of [A, B]
        half = f if k == 0 else f // 2         # (the first stage keeps the full width in both halves)
        c.lines.append("# Downsample")
        mish(f, 3, stride=2)
        mish(half, 1)
        c.add("route", ("layers", "-2"))
        mish(half, 1)
        for _ in range(blocks):
            mish(f // 2, 1)
            mish(half, 3)
            c.add("shortcut", ("from", -3), ("activation", "linear"))
        mish(half, 1)
        c.add("route", ("layers", f"-1,-{3 * blocks + 4}"))
        stage_out.append(mish(f, 1))
    c.lines.append("##########################")

    def five(f, first=True):  # 1x1 f, 3x3 2f, 1x1 f(, 3x3 2f, 1x1 f): returns the last layer
        at = None
        for j in range(5 if first else 3):
            at = c.conv(2 * f if j % 2 else f, 3 if j % 2 else 1)
        return at

    five(512, first=False)
    c.lines.append("### SPP ###")
    c.add("maxpool", ("stride", 1), ("size", 5))
    c.add("route", ("layers", "-2"))
    c.add("maxpool", ("stride", 1), ("size", 9))
    c.add("route", ("layers", "-4"))
    c.add("maxpool", ("stride", 1), ("size", 13))
    c.add("route", ("layers", "-1,-3,-5,-6"))
    c.lines.append("### End SPP ###")
    tops = [five(512, first=False)]  # the neck's tensor of each scale on the way up, coarsest first
    for f, lateral in ((256, stage_out[3]), (128, stage_out[2])):
        c.conv(f, 1)
        c.add("upsample", ("stride", 2))
        c.add("route", ("layers", lateral))
        c.conv(f, 1)
        c.add("route", ("layers", "-1, -3"))
        tops.append(five(f))
    for k, (f, mask, sxy) in enumerate(((128, "0,1,2", "1.2"), (256, "3,4,5", "1.1"), (512, "6,7,8", "1.05"))):
        c.conv(2 * f, 3)
        c.conv(n_out, 1, head=True, act="logistic" if scaled else "linear")
        c.yolo_v4(mask, _V4_ANCHORS, classes, "2.0" if scaled else sxy, scaled)
        if k < 2:  # the way down: a stride-2 conv of this scale joins the neck's tensor of the next coarser one
            c.add("route", ("layers", "-4"))
            at = c.conv(2 * f, 3, stride=2)
            c.add("route", ("layers", f"-1, {tops[1 - k] - at - 1}"))
            five(2 * f)
    return c.text()


# EfficientNet-B0's seven stages (Tan & Le 2019, table 1): (expansion, kernel, output width, blocks, first stride)
_B0_STAGES = ((1, 3, 16, 1, 1), (6, 3, 24, 2, 2), (6, 5, 40, 2, 2), (6, 3, 80, 3, 2), (6, 5, 112, 3, 1),
              (6, 5, 192, 4, 2), (6, 3, 320, 1, 1))


def _efficientnet_b0(c, classes):
    """EfficientNet-B0 in Darknet sections, built from the paper's table: the 3x3 stride-2 stem of 32, sixteen MBConv
    blocks, the 1x1 head of 1280, [avgpool], a 1x1 conv to `classes` and [softmax].  An MBConv block is a 1x1
    expansion (left out where the expansion is 1), a depthwise k x k conv, the squeeze-and-excitation block
    ([avgpool], a 1x1 conv with a bias and swish to a quarter of the BLOCK's input width, a 1x1 conv with a bias and
    logistic back to the expanded width, [scale_channels]), a linear 1x1 projection, and a linear [shortcut] from the
    block's input where the stride is 1 and the widths agree.  Every other conv has batch_normalize=1 and swish."""
    def conv(filters, size, stride=1, act="swish", groups=1, bn=True):
        pairs = ([("batch_normalize", 1)] if bn else []) + [("filters", filters), ("size", size), ("stride", stride),
                                                            ("pad", 1)]
        return c.add("convolutional", *pairs, *([("groups", groups)] if groups > 1 else []), ("activation", act))

    conv(c.wd(32), 3, stride=2)
    cin = c.wd(32)
    for expand, k, width, blocks, stride in _B0_STAGES:
        for b in range(blocks):
            c.lines.append(f"# MBConv{expand} {k}x{k}")
            start, cout, s = c.n, c.wd(width), stride if b == 0 else 1
            mid = cin * expand
            if expand != 1:
                conv(mid, 1)
            conv(mid, k, stride=s, groups=mid)
            c.add("avgpool")
            conv(max(1, cin // 4), 1, bn=False)
            conv(mid, 1, act="logistic", bn=False)
            c.add("scale_channels", ("from", -4), ("activation", "linear"))
            conv(cout, 1, act="linear")
            if s == 1 and cin == cout:
                c.add("shortcut", ("from", start - 1 - c.n), ("activation", "linear"))
            cin = cout
    conv(c.wd(1280), 1)
    c.add("avgpool")
    c.conv(classes, 1, head=True)
    c.add("softmax", ("groups", 1))
    return c.text()


def cfg_text(model, classes=None, width=None, height=None, width_div=1, scaled_head=False):
    """The public definition of `model` (one of MODELS) as cfg text, for `classes` classes and a
    width x height input; width_div divides every channel count except the heads' 3 x (5 + classes)
    or the classifier conv's `classes` (a narrow model of the same topology).  Defaults: 80 classes
    at 416 x 416 for the detectors (20 for "yolov2_voc" and "yolov2_tiny_voc", whose heads are 5 x (5 + classes)) ("yolov4" has no default size: ValueError without width and height); 1000 classes for the classifiers "darknet19" (224 x 224) and
    "darknet53" (256 x 256), which end in [avgpool] and [softmax].
    "efficientnet_b0" (224 x 224, 1000 classes) is a CONSTRUCTION after the table of the EfficientNet paper
    (_efficientnet_b0: stem, seven MBConv stages with squeeze-and-excitation, the 1280-wide head), not the text of
    AlexeyAB's efficientnet_b0.cfg, which is not in this repository and may differ in details (its SE widths, its
    dropout sections); a user's own cfg and .weights are theirs to pass to DarknetModel.
    scaled_head ("yolov4" only): YOLOv4's topology with the head of the scaled-YOLOv4 cfgs: the head convs
    are activation=logistic and each [yolo] carries new_coords=1, scale_x_y=2.0, nms_kind=diounms and
    beta_nms=0.6.  That is a construction for testing the head, not a public cfg: the public yolov4-csp /
    yolov7 texts are the caller's to pass in."""
    if model not in MODELS:
        raise ValueError(f"model {model!r}: one of {MODELS} expected")
    if scaled_head and model != "yolov4":
        raise ValueError('scaled_head is defined for "yolov4" only')
    if model == "yolov4" and (width is None or height is None):
        # its public cfg is 608 x 608, which has more boxes than the default head decodes (DarknetModel builds it
        # without a head unless wide=True), and 416 x 416, the other detectors' default here, is not its definition
        raise ValueError('cfg_text("yolov4") takes no default size: pass width and height (608 x 608 in the public cfg)')
    size = CLASSIFIERS.get(model, 416)
    voc = model in ("yolov2_voc", "yolov2_tiny_voc")
    classes = (1000 if model in CLASSIFIERS else 20 if voc else 80) if classes is None else int(classes)
    width, height = size if width is None else width, size if height is None else height
    n_out = 3 * (5 + classes)
    c = _Cfg(width, height, int(width_div))
    if model in ("yolov2_tiny", "yolov2_tiny_voc"):  # six conv + pool stages (the last pool stride 1), two 3x3 convs
        for k, f in enumerate((16, 32, 64, 128, 256, 512)):
            c.conv(f, 3)
            c.add("maxpool", ("size", 2), ("stride", 2 if k < 5 else 1))
        c.conv(1024, 3)
        c.lines.append("###########")
        c.conv(1024 if voc else 512, 3)
        c.conv(5 * (5 + classes), 1, head=True)
        c.region(_V2_TINY_VOC_ANCHORS if voc else _V2_COCO_ANCHORS, classes)
        return c.text()
    if model in ("yolov2", "yolov2_voc"):  # Darknet-19's trunk, two 3x3 convs, the passthrough of layer 16
        for stage, f in enumerate((32, 64, 128, 256, 512, 1024)):
            for j in range(1 if stage < 2 else 3 if stage < 4 else 5):  # 3x3 f, 1x1 f / 2, 3x3 f, ...
                at = c.conv(f // 2 if j % 2 else f, 1 if j % 2 else 3)
            if stage == 4:
                fine = at  # the 26 x 26 x 512 map (at 416 x 416)
            if stage < 5:
                c.add("maxpool", ("size", 2), ("stride", 2))
        c.lines.append("#######")
        c.conv(1024, 3)
        trunk = c.conv(1024, 3)
        c.add("route", ("layers", fine - c.n))
        c.conv(64, 1)
        c.add("reorg", ("stride", 2))
        c.add("route", ("layers", f"-1,{trunk - c.n}"))
        c.conv(1024, 3)
        c.conv(5 * (5 + classes), 1, head=True)
        c.region(_V2_VOC_ANCHORS if voc else _V2_COCO_ANCHORS, classes)
        return c.text()
    if model == "efficientnet_b0":
        return _efficientnet_b0(c, classes)
    if model == "darknet19":
        for stage, f in enumerate((32, 64, 128, 256, 512, 1024)):
            for j in range(1 if stage < 2 else 3 if stage < 4 else 5):  # 3x3 f, 1x1 f / 2, 3x3 f, ...
                c.conv(f // 2 if j % 2 else f, 1 if j % 2 else 3)
            if stage < 5:
                c.add("maxpool", ("size", 2), ("stride", 2))
        c.conv(classes, 1, head=True)
        c.add("avgpool")
        c.add("softmax", ("groups", 1))
        c.add("cost", ("type", "sse"))
        return c.text()
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
    if model == "yolov4":
        return _yolov4(c, n_out, classes, scaled_head)
    c.conv(32, 3)
    stage_end = []
    for f, blocks in _STAGES:
        c.lines.append("# Downsample")
        c.conv(f, 3, stride=2)
        for _ in range(blocks):
            c.conv(f // 2, 1)
            c.conv(f, 3)
            stage_end.append(c.add("shortcut", ("from", -3), ("activation", "linear")))
    if model == "darknet53":  # the classifier: the trunk, then the pool, the class conv and the softmax
        c.add("avgpool")
        c.conv(classes, 1, head=True)
        c.add("softmax", ("groups", 1))
        return c.text()
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
