"""YOLOv3-tiny on the MI355X engine, built like yolov3.YOLO_V3:

    t = YOLO_V3_TINY([1, 416, 416, 3], weights, debug)
    outs = t.inference(frame)             # [1,13,13,255], [1,26,26,255]
    boxes = t.postprocessing(outs)        # one image's label boxes
    rows = t.detect(frames)               # plan + decode on the device

The reference has no such model; the topology is the public YOLOv3-tiny definition, as one graph
with two outputs (every conv but the two heads has BatchNorm + leaky):

    stack     3x3 convs of 16, 32, 64, 128, 256 and 512 channels, a 2x2 / stride-2 max pool after
              each of the first five and a 2x2 / stride-1 SAME pool after the sixth
    scale 32  3x3 x 1024, 1x1 x 256 -> y; 3x3 x 512 and the linear 1x1 x n_out head on y
                                                                              (extra output 0)
    merge     1x1 x 128 on y, upsample x 2, Concat([upsampled, the 256-channel conv's output])
    scale 16  3x3 x 256 and the linear 1x1 x n_out head                       (the primary output)

`weights` is a list of 13 layer dicts in the yolo_weights format, in Darknet layer order
(synth.yolov3_tiny_weights makes synthetic ones; its width_div gives a narrow model).  The whole
graph lowers to ONE device plan with the plan machinery YOLOv3 uses: the 256-channel conv's output
is a long skip into the Concat, the stride-32 head an output branch that ends in a tap.

The network is Darknet's exactly: it has no stride-2 conv (the padding difference noted in
yolov3.py does not arise), the stride-2 pools need no padding on the even maps of an input that is
a multiple of 32, and the stride-1 pool pads bottom / right only, as Darknet's does there.

Out of scope:

  * Darknet .cfg / .weights files: this model takes yolo_weights layer dicts
    (darknet_import.DarknetModel reads the files and lowers to the same plan entries);
  * the defaults are not Darknet's: the NMS is the reference's class-agnostic one over both
    scales (include/dnn_hip_post.h) and a box carries one class, the arg-max.  Darknet's
    per-class rule with its multi-label output (one detection per class above the threshold for
    each box) is `head=yolo_post.MultiHead.yolov3_tiny(h, w, classes, nms="per_class",
    labels="multi")`.
"""
import darknet53
import dnn_hip
import yolo_post
import yolo_weights
import yolov3

EPS = yolov3.EPS
N_STACK = 6          # the pooled 3x3 convs
N_LAYERS = 13
SKIP_FROM = 4        # the Concat takes conv 4's output (256 channels)
STRIDES = (32, 16)
HEADS = (9, 12)      # the two linear heads' layer numbers


def structure():
    """Per conv, in weight order: (kernel size, stride, role) with role "stack", "neck" (the 1024
    and 256 convs), "pre" (a head's 3x3 conv), "head" or "reduce"."""
    return ([(3, 1, "stack")] * N_STACK + [(3, 1, "neck"), (1, 1, "neck"), (3, 1, "pre"), (1, 1, "head"),
                                           (1, 1, "reduce"), (3, 1, "pre"), (1, 1, "head")])


def validate(weights, n_out=None):
    """Check the 13-layer structure (keys, kernel sizes, channels chaining through the two
    branches and the concat) and return it as fp32 contiguous arrays."""
    if not isinstance(weights, (list, tuple)) or len(weights) != N_LAYERS:
        raise yolo_weights.WeightFileError(f"expected a list of {N_LAYERS} layer dicts")
    s = structure()
    stack, skip_c, _ = darknet53.validate_chain(weights[:SKIP_FROM + 1], s[:SKIP_FROM + 1], 3)
    rest, y_c, _ = darknet53.validate_chain(weights[SKIP_FROM + 1:8], s[SKIP_FROM + 1:8], skip_c, first=SKIP_FROM + 1)
    head0, oc0, _ = darknet53.validate_chain(weights[8:10], s[8:10], y_c, first=8)
    red, r_c, _ = darknet53.validate_chain(weights[10:11], s[10:11], y_c, first=10)
    head1, oc1, _ = darknet53.validate_chain(weights[11:13], s[11:13], r_c + skip_c, first=11)
    for layer, oc, stride in ((HEADS[0], oc0, 32), (HEADS[1], oc1, 16)):
        if n_out is not None and oc != n_out:
            raise yolo_weights.WeightFileError(f"layer {layer} (the stride-{stride} head) has {oc} outputs; "
                                               f"this head needs {n_out}")
    return stack + rest + head0 + red + head1


def build_graph(builder_cls, weights, in_shape=(1, 416, 416, 3)):
    """Return (graph, nodes, outs): nodes in creation order, outs the two head nodes (stride 32,
    16); the first is the graph's extra output, the second its primary one."""
    g = builder_cls()
    nodes = []

    def conv_block(x, w, linear=False):
        x = g.create_conv2d(x, w["kernel"], strides=[1, 1, 1, 1], padding="SAME")
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
    lateral = None
    for i, w in enumerate(weights[:N_STACK]):
        x = conv_block(x, w)
        if i == SKIP_FROM:
            lateral = x
        stride = 2 if i < N_STACK - 1 else 1
        x = g.create_max_pool2d(x, [1, 2, 2, 1], [1, stride, stride, 1], "SAME")
        nodes.append(x)
    y = conv_block(conv_block(x, weights[6]), weights[7])
    head0 = conv_block(conv_block(y, weights[8]), weights[9], linear=True)
    g.add_out_node(head0)
    x = conv_block(y, weights[10])
    x = g.create_upsample(x, 2)
    nodes.append(x)
    x = g.create_concat([x, lateral])
    nodes.append(x)
    head1 = conv_block(conv_block(x, weights[11]), weights[12], linear=True)
    g.set_out_node(head1)
    return g, nodes, [head0, head1]


class YOLO_V3_TINY(yolov3.YOLO_V3):
    """YOLOv3-tiny with the MI355X engine underneath: in_shape [batch, h, w, 3] with h, w multiples
    of 32.  `head` is a yolo_post.MultiHead of two scales (grids in / 32, in / 16); without one,
    MultiHead.yolov3_tiny for the class count the last layers' width implies (n_out = 3 x (5 +
    classes)).  inference, postprocessing and detect are yolov3.YOLO_V3's, on two tensors."""

    def __init__(self, in_shape, weights, debug, device=None, head=None):
        if len(in_shape) != 4:
            raise ValueError(f"in_shape {in_shape!r}: [batch, height, width, channels] expected")
        if in_shape[1] % 32 or in_shape[2] % 32 or in_shape[1] <= 0 or in_shape[2] <= 0:
            raise ValueError(f"in_shape {in_shape!r}: height and width must be multiples of 32")
        self.in_shape = tuple(in_shape)
        w = validate(weights)
        n_out = w[HEADS[0]]["kernel"].shape[3]
        if head is None:
            if n_out % 3 or n_out // 3 < 6:
                raise ValueError(f"{n_out} head outputs are not 3 x (5 + classes): pass head=")
            head = yolo_post.MultiHead.yolov3_tiny(in_shape[1], in_shape[2], classes=n_out // 3 - 5)
        grids = [(s.grid_h, s.grid_w) for s in head.scales]
        want = [(in_shape[1] // st, in_shape[2] // st) for st in STRIDES]
        if grids != want or any(n != n_out for n in head.n_out):
            raise ValueError(f"head {head!r} does not fit {n_out} outputs on grids {want}")
        validate(weights, n_out)
        self.head = head
        self.g, self.nodes, self.outs = build_graph(dnn_hip.DnnGraphBuilder, w, in_shape=self.in_shape)
        self.sess = dnn_hip.DnnInferenceEngine(self.g, debug, device=device)
        self._dev = None
