"""YOLOv3-SPP on the MI355X engine, built like yolov3.YOLO_V3:

    y3 = YOLO_V3_SPP([1, 416, 416, 3], weights, debug)
    outs = y3.inference(frame)            # [1,13,13,255], [1,26,26,255], [1,52,52,255]
    boxes = y3.postprocessing(outs)       # one image's label boxes
    rows = y3.detect(frames)              # plan + decode on the device

The reference has no such model; the topology is the public YOLOv3-SPP definition: YOLOv3
(yolov3.py) with one spatial pyramid pooling block in the stride-32 branch, whose neck becomes

    1x1 x 512, 3x3 x 1024, 1x1 x 512,
    SPP: [maxpool13(x), maxpool9(x), maxpool5(x), x] on channels (stride 1, SAME)  -> 2048
    1x1 x 512, 3x3 x 1024, 1x1 x 512 -> y

followed by the usual 3x3 x 1024 and linear head; the merges and the other two scales are
YOLOv3's.  `weights` is a list of 76 layer dicts in the yolo_weights format, in Darknet layer
order (synth.yolov3_spp_weights makes synthetic ones; its width_div gives a narrow model).

The whole graph lowers to ONE device plan, as YOLOv3's does, and the SPP block is one plan entry
and one kernel (dnn_hip.Spp, csrc/spp.hip): 76 convs, 1 spp, 2 taps.  inference, postprocessing
and detect are yolov3.YOLO_V3's; the decode is yolo_post.MultiHead.yolov3.

Out of scope, as for yolov3.py:

  * Darknet .cfg / .weights files: this model takes yolo_weights layer dicts
    (darknet_import.DarknetModel reads the files, finds the SPP pattern in the cfg and lowers it to
    the same spp entry);
  * the defaults are not Darknet's: the NMS is the reference's class-agnostic one over all scales
    and a box carries one class, the arg-max.  Darknet's per-class rule with its multi-label
    output is `head=yolo_post.MultiHead.yolov3(h, w, classes, nms="per_class", labels="multi")`;
  * the stride-2 convs use the engine's SAME padding (bottom / right on an even input), Darknet
    pads 1 on every side, so a converted Darknet checkpoint computes something else at those five
    layers (darknet_import's convs pad as Darknet does).  The SPP pools themselves are Darknet's:
    stride 1 with size // 2 on every side.
"""
import darknet53
import dnn_hip
import yolo_post
import yolo_weights
import yolov3

EPS = yolov3.EPS
N_TRUNK = yolov3.N_TRUNK               # 52
N_SCALE = yolov3.N_SCALE               # 7
N_SPP_SCALE = N_SCALE + 1              # the stride-32 branch: six neck convs, the 3x3 conv, the head
N_LAYERS = yolov3.N_LAYERS + 1         # 76
STRIDES = yolov3.STRIDES
SPP_POOLS = (13, 9, 5)
SPP_AFTER = 3                          # the SPP block follows the stride-32 branch's third conv


def spp_scale_structure():
    return [(1, 1, "neck"), (3, 1, "neck"), (1, 1, "neck")] * 2 + [(3, 1, "pre"), (1, 1, "head")]


def structure():
    """Per conv, in weight order: (kernel size, stride, role), as yolov3.structure() with the
    stride-32 branch's six neck convs."""
    s = darknet53.structure()[:N_TRUNK] + spp_scale_structure() + [(1, 1, "reduce")]
    s += yolov3.scale_structure() + [(1, 1, "reduce")] + yolov3.scale_structure()
    return s


def validate(weights, n_out=None):
    """Check the 76-layer structure (keys, kernel sizes, channels chaining through the residual
    sums, the SPP block, the two concats and the three branches) and return it as fp32 contiguous
    arrays."""
    if not isinstance(weights, (list, tuple)) or len(weights) != N_LAYERS:
        raise yolo_weights.WeightFileError(f"expected a list of {N_LAYERS} layer dicts")
    out, ic, downs = darknet53.validate_chain(weights[:N_TRUNK], darknet53.structure()[:N_TRUNK], 3)
    skips = (downs[3], downs[2])
    at = N_TRUNK
    for k in range(3):
        if k == 0:  # three convs, the SPP block (x 4 channels), three convs
            struct = spp_scale_structure()
            pre, ic, _ = darknet53.validate_chain(weights[at:at + SPP_AFTER], struct[:SPP_AFTER], ic, first=at)
            post, y_c, _ = darknet53.validate_chain(weights[at + SPP_AFTER:at + 6], struct[SPP_AFTER:6],
                                                    ic * (len(SPP_POOLS) + 1), first=at + SPP_AFTER)
            neck, n = pre + post, N_SPP_SCALE
        else:
            struct = yolov3.scale_structure()
            neck, y_c, _ = darknet53.validate_chain(weights[at:at + 5], struct[:5], ic, first=at)
            n = N_SCALE
        tail, oc, _ = darknet53.validate_chain(weights[at + n - 2:at + n], struct[n - 2:], y_c, first=at + n - 2)
        if n_out is not None and oc != n_out:
            raise yolo_weights.WeightFileError(f"layer {at + n - 1} (the stride-{STRIDES[k]} head) has {oc} "
                                               f"outputs; this head needs {n_out}")
        out += neck + tail
        at += n
        if k < 2:
            red, r_c, _ = darknet53.validate_chain(weights[at:at + 1], [(1, 1, "reduce")], y_c, first=at)
            out += red
            at += 1
            ic = r_c + skips[k]
    return out


def build_graph(builder_cls, weights, in_shape=(1, 416, 416, 3)):
    """Return (graph, nodes, outs) as yolov3.build_graph does: nodes in creation order, outs the
    three head nodes (stride 32, 16, 8); the first two are the graph's extra outputs, the third
    its primary one."""
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
    stage_out = []  # the tensor each stage ends in
    for w, (_, stride, role) in zip(weights[:N_TRUNK], darknet53.structure()[:N_TRUNK]):
        if role == "squeeze":
            skip = x
        if role == "down":
            stage_out.append(None)
        x = conv_block(x, w, stride=stride)
        if role == "expand":
            x = g.create_add([skip, x])
            nodes.append(x)
        if stage_out:
            stage_out[-1] = x
    laterals = (stage_out[3], stage_out[2])
    outs = []
    at = N_TRUNK
    for k in range(3):
        n_neck = 6 if k == 0 else 5
        for j, w in enumerate(weights[at:at + n_neck]):
            if k == 0 and j == SPP_AFTER:
                x = g.create_spp(x, SPP_POOLS)
                nodes.append(x)
            x = conv_block(x, w)
        y = x
        head = conv_block(conv_block(y, weights[at + n_neck]), weights[at + n_neck + 1], linear=True)
        outs.append(head)
        at += n_neck + 2
        if k < 2:
            g.add_out_node(head)
            x = conv_block(y, weights[at])
            at += 1
            x = g.create_upsample(x, 2)
            nodes.append(x)
            x = g.create_concat([x, laterals[k]])
            nodes.append(x)
    g.set_out_node(outs[2])
    return g, nodes, outs


class YOLO_V3_SPP(yolov3.YOLO_V3):
    """YOLOv3-SPP with the MI355X engine underneath: in_shape [batch, h, w, 3] with h, w multiples
    of 32.  `head` is a yolo_post.MultiHead of three scales (grids in / 32, in / 16, in / 8);
    without one, MultiHead.yolov3 for the class count the last layers' width implies."""

    def __init__(self, in_shape, weights, debug, device=None, head=None):
        if len(in_shape) != 4:
            raise ValueError(f"in_shape {in_shape!r}: [batch, height, width, channels] expected")
        if in_shape[1] % 32 or in_shape[2] % 32 or in_shape[1] <= 0 or in_shape[2] <= 0:
            raise ValueError(f"in_shape {in_shape!r}: height and width must be multiples of 32")
        self.in_shape = tuple(in_shape)
        w = validate(weights)
        n_out = w[N_TRUNK + N_SPP_SCALE - 1]["kernel"].shape[3]
        if head is None:
            if n_out % 3 or n_out // 3 < 6:
                raise ValueError(f"{n_out} head outputs are not 3 x (5 + classes): pass head=")
            head = yolo_post.MultiHead.yolov3(in_shape[1], in_shape[2], classes=n_out // 3 - 5)
        grids = [(s.grid_h, s.grid_w) for s in head.scales]
        want = [(in_shape[1] // st, in_shape[2] // st) for st in STRIDES]
        if grids != want or any(n != n_out for n in head.n_out):
            raise ValueError(f"head {head!r} does not fit {n_out} outputs on grids {want}")
        validate(weights, n_out)
        self.head = head
        self.g, self.nodes, self.outs = build_graph(dnn_hip.DnnGraphBuilder, w, in_shape=self.in_shape)
        self.sess = dnn_hip.DnnInferenceEngine(self.g, debug, device=device)
        self._dev = None
