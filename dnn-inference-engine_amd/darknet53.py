"""Darknet-53 with YOLOv3's stride-32 branch on the MI355X engine, built like yolov2.YOLO_V2:

    d53 = DARKNET53([1, 416, 416, 3], weights, debug)
    out = d53.inference(frame)            # [1, 13, 13, n_out]

The reference has no such model (its graph nodes can neither fork nor add); the topology is
layers 0-81 of the public YOLOv3 definition, as one graph:

    trunk   Darknet-53's 52 convs (BatchNorm + leaky): a 3x3 x 32 stem, then five stages, each a
            3x3 stride-2 conv to the stage width (64, 128, 256, 512, 1024) followed by 1, 2, 8, 8
            and 4 residual blocks  y = x + conv3x3(conv1x1(x)), the 1x1 at half the width; the sum
            has no activation (dnn_hip.Add, 23 of them)
    branch  1x1 x 512, 3x3 x 1024, three times
    head    a linear 1x1 x n_out conv with bias only

`weights` is a list of 59 layer dicts in the yolo_weights format (kernel HWIO, biases, and
moving_mean / moving_variance / gamma for all but the last), in layer order
(synth.darknet53_weights makes synthetic ones; its width_div gives a narrow model).  The channel
counts follow the kernels, so a narrow model is the same code.  The whole graph lowers to one
device plan: every block is stash, two convs, shortcut, release, and the blocks alternate between
two workspace regions.

Two differences from the Darknet original:

  * the stride-2 convs use the engine's SAME padding (TensorFlow's: on an even input one row and
    one column of zeros at the bottom / right only), Darknet pads 1 on every side, so weights
    converted from a Darknet checkpoint compute something else at those five layers
    (darknet_import.DarknetModel builds the network from a .cfg with Darknet's padding and reads
    .weights files; this hand-written model keeps SAME);
  * the output is the raw [n, in / 32, in / 32, n_out] tensor.  YOLOv3's own decode (logistic
    class scores, three scales) is not part of this model; an n_out in YOLOv2's format
    (anchors x (5 + classes)) decodes with yolo_post.YoloHead as before.
"""
import numpy as np

import dnn_hip
import yolo_post
import yolo_weights
import yolov2

EPS = 1e-5
STAGE_BLOCKS = (1, 2, 8, 8, 4)
N_BRANCH = 6
N_TRUNK = 1 + sum(1 + 2 * b for b in STAGE_BLOCKS)  # 52
N_LAYERS = N_TRUNK + N_BRANCH + 1                    # 59
N_SHORTCUTS = sum(STAGE_BLOCKS)                      # 23


def structure():
    """Per conv, in weight order: (kernel size, stride, role) with role "stem", "down" (a stage's
    stride-2 conv), "squeeze" / "expand" (a residual block's 1x1 and 3x3), "branch" or "head"."""
    s = [(3, 1, "stem")]
    for blocks in STAGE_BLOCKS:
        s.append((3, 2, "down"))
        s += [(1, 1, "squeeze"), (3, 1, "expand")] * blocks
    s += [(1, 1, "branch"), (3, 1, "branch")] * (N_BRANCH // 2)
    s.append((1, 1, "head"))
    return s


def validate_chain(weights, struct, ic, first=0, width=None):
    """Check the layer dicts `weights` against `struct` (entries as structure()'s) as one chain
    that starts with `ic` input channels: keys, kernel sizes, channels chaining through the
    residual sums.  `first` is the first layer's number in messages.  Returns (the layers as fp32
    contiguous arrays, the last layer's output channels, the output channels of each "down"
    conv)."""
    out, downs = [], []
    for i, (w, (ksize, _, role)) in enumerate(zip(weights, struct), start=first):
        keys = ("kernel", "biases") + (yolo_weights.BN_KEYS if role != "head" else ())
        if not isinstance(w, dict) or any(k not in w for k in keys):
            raise yolo_weights.WeightFileError(f"layer {i}: expected a dict with {keys}")
        d = {k: np.ascontiguousarray(np.asarray(w[k]), dtype=np.float32) for k in keys}
        k = d["kernel"]
        if k.ndim != 4 or k.shape[0] != ksize or k.shape[1] != ksize:
            raise yolo_weights.WeightFileError(f"layer {i} ({role}): kernel shape {k.shape}, expected "
                                               f"{ksize}x{ksize} HWIO")
        for key in keys[1:]:
            if d[key].shape != (k.shape[3],):
                raise yolo_weights.WeightFileError(f"layer {i} {key}: shape {d[key].shape}, expected ({k.shape[3]},)")
        if k.shape[2] != ic:
            raise yolo_weights.WeightFileError(f"layer {i}: {k.shape[2]} input channels, expected {ic}")
        if role == "down":
            width = k.shape[3]
            downs.append(width)
        elif role == "expand" and k.shape[3] != width:  # the sum needs the block's input shape
            raise yolo_weights.WeightFileError(f"layer {i}: a residual block's second conv has {k.shape[3]} "
                                               f"outputs, its input {width} channels")
        ic = k.shape[3]
        out.append(d)
    return out, ic, downs


def validate(weights, n_out=None):
    """Check the 59-layer structure (keys, kernel sizes, channels chaining through the residual
    sums) and return it as fp32 contiguous arrays."""
    if not isinstance(weights, (list, tuple)) or len(weights) != N_LAYERS:
        raise yolo_weights.WeightFileError(f"expected a list of {N_LAYERS} layer dicts")
    out, ic, _ = validate_chain(weights, structure(), 3)
    if n_out is not None and ic != n_out:
        raise yolo_weights.WeightFileError(f"last layer has {ic} outputs; this head needs {n_out}")
    return out


def build_graph(builder_cls, weights, in_shape=(1, 416, 416, 3)):
    """Return (graph, nodes): nodes in creation order, on any module with dnn_hip's builder API."""
    g = builder_cls()
    nodes = []

    def conv_block(x, w, stride=1, linear=False):
        x = g.create_conv2d(x, w["kernel"], strides=[1, stride, stride, 1], padding="SAME")
        nodes.append(x)
        x = g.create_bias_add(x, w["biases"])
        nodes.append(x)
        if linear:
            return x
        x = g.create_batch_norm(x, w["moving_mean"], w["moving_variance"], w["gamma"], EPS)
        nodes.append(x)
        x = g.create_leaky_relu(x)
        nodes.append(x)
        return x

    x = g.create_input(list(in_shape))
    skip = None
    for w, (_, stride, role) in zip(weights, structure()):
        if role == "squeeze":
            skip = x
        x = conv_block(x, w, stride=stride, linear=role == "head")
        if role == "expand":
            x = g.create_add([skip, x])
            nodes.append(x)
    g.set_out_node(x)
    return g, nodes


class DARKNET53(object):
    """Darknet-53 + the stride-32 branch with the MI355X engine underneath: in_shape
    [batch, h, w, 3] with h, w multiples of 32.  `head` is a yolo_post.YoloHead for a
    YOLOv2-format last layer (its grid is replaced by in_shape's); without one the COCO-anchor
    head of the last layer's width is used where that width has the format, else there is no
    postprocessing."""

    def __init__(self, in_shape, weights, debug, device=None, head=None):
        if len(in_shape) != 4:
            raise ValueError(f"in_shape {in_shape!r}: [batch, height, width, channels] expected")
        if in_shape[1] % 32 or in_shape[2] % 32 or in_shape[1] <= 0 or in_shape[2] <= 0:
            raise ValueError(f"in_shape {in_shape!r}: height and width must be multiples of 32")
        self.in_shape = tuple(in_shape)
        self.head = None if head is None else yolov2._head_for(in_shape, head, head.n_out)
        w = validate(weights, None if head is None else self.head.n_out)
        if head is None:
            try:
                self.head = yolov2._head_for(in_shape, None, w[-1]["kernel"].shape[3])
            except ValueError:
                self.head = None
        self.g, self.nodes = build_graph(dnn_hip.DnnGraphBuilder, w, in_shape=self.in_shape)
        self.sess = dnn_hip.DnnInferenceEngine(self.g, debug, device=device)

    def inference(self, im):
        return self.sess.run(im)

    def postprocessing(self, out):
        """Boxes of one image of inference()'s output (YOLOv2-format heads only)."""
        if self.head is None:
            raise ValueError("the last layer is not in YOLOv2's format: pass head=")
        return yolo_post.postprocessing(out, head=self.head)
