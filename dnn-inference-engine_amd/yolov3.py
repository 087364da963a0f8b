"""Full YOLOv3 on the MI355X engine, built like darknet53.DARKNET53:

    y3 = YOLO_V3([1, 416, 416, 3], weights, debug)
    outs = y3.inference(frame)            # [1,13,13,255], [1,26,26,255], [1,52,52,255]
    boxes = y3.postprocessing(outs)       # one image's label boxes
    rows = y3.detect(frames)              # plan + decode on the device, per image detect_batch's rows

The reference has no such model; the topology is the public YOLOv3 definition, as one graph with
three outputs:

    trunk     Darknet-53's 52 convs with 23 residual sums (darknet53.py)
    scale 32  five alternating 1x1 x 512 / 3x3 x 1024 convs -> y; 3x3 x 1024 and the linear
              1x1 x n_out head on y                                          (extra output 0)
    merge     1x1 x 256 on y, upsample x 2, Concat([upsampled, stage 4's output])
    scale 16  the same with 256 / 512                                         (extra output 1)
    merge     1x1 x 128, upsample x 2, Concat([upsampled, stage 3's output])
    scale 8   the same with 128 / 256                                         (the primary output)

`weights` is a list of 75 layer dicts in the yolo_weights format, in Darknet layer order: the 52
trunk convs, then per scale its seven convs, with the 1x1 reduce conv of each merge after the
scale's head (synth.yolov3_weights makes synthetic ones; its width_div gives a narrow model).
The channel counts follow the kernels, so a narrow model is the same code.

The whole graph lowers to ONE device plan (dnn_hip.lower_graph): the ends of stages 3 and 4 are
long skips into the two Concats (a stash held across the residual blocks in between, then a route
and a release), each of the first two heads is an output branch that ends in a tap, and the
stride-8 head is the plan's output.  `detect` hands the two tap buffers and the output buffer
straight to the multi-scale decode (yolo_post.MultiHead, csrc/postprocess_multi.hip): the head
tensors make no host round trip.

Two differences from the Darknet original:

  * the stride-2 convs use the engine's SAME padding (TensorFlow's: on an even input one row and
    one column of zeros at the bottom / right only), Darknet pads 1 on every side, so weights
    converted from a Darknet checkpoint compute something else at those five layers
    (darknet_import.DarknetModel builds the network from a .cfg with Darknet's padding and reads
    .weights files; this hand-written model keeps SAME);
  * the default NMS is the reference's class-agnostic one over all scales
    (include/dnn_hip_post.h).  Darknet's per-class rule is
    `head=yolo_post.MultiHead.yolov3(h, w, classes, nms="per_class")`, and with
    `labels="multi"` beside it a box gives one detection per class above the threshold, as
    Darknet's does (the default is one class per box, the arg-max).  The detection buffers are
    sized by `head.max_det`, which with "multi" is more than the boxes.
"""
import numpy as np

import darknet53
import dnn_hip
import yolo_post
import yolo_weights

EPS = darknet53.EPS
N_TRUNK = darknet53.N_TRUNK            # 52
N_SCALE = 7                            # five alternating convs, the 3x3 conv, the head
N_LAYERS = N_TRUNK + 3 * N_SCALE + 2   # 75
STRIDES = (32, 16, 8)


def scale_structure():
    return [(1, 1, "neck"), (3, 1, "neck")] * 2 + [(1, 1, "neck"), (3, 1, "pre"), (1, 1, "head")]


def structure():
    """Per conv, in weight order: (kernel size, stride, role): darknet53.structure()'s trunk, then
    per scale five "neck" convs, the "pre" 3x3 and the "head", with a "reduce" 1x1 after the first
    two heads."""
    s = darknet53.structure()[:N_TRUNK]
    for k in range(3):
        s += scale_structure()
        if k < 2:
            s.append((1, 1, "reduce"))
    return s


def validate(weights, n_out=None):
    """Check the 75-layer structure (keys, kernel sizes, channels chaining through the residual
    sums, the two concats and the three branches) and return it as fp32 contiguous arrays."""
    if not isinstance(weights, (list, tuple)) or len(weights) != N_LAYERS:
        raise yolo_weights.WeightFileError(f"expected a list of {N_LAYERS} layer dicts")
    out, ic, downs = darknet53.validate_chain(weights[:N_TRUNK], darknet53.structure()[:N_TRUNK], 3)
    skips = (downs[3], downs[2])  # stage 4's and stage 3's widths: what the two concats add
    at = N_TRUNK
    for k in range(3):
        neck, y_c, _ = darknet53.validate_chain(weights[at:at + 5], scale_structure()[:5], ic, first=at)
        tail, oc, _ = darknet53.validate_chain(weights[at + 5:at + 7], scale_structure()[5:], y_c, first=at + 5)
        if n_out is not None and oc != n_out:
            raise yolo_weights.WeightFileError(f"layer {at + 6} (the stride-{STRIDES[k]} head) has {oc} outputs; "
                                               f"this head needs {n_out}")
        out += neck + tail
        at += N_SCALE
        if k < 2:
            red, r_c, _ = darknet53.validate_chain(weights[at:at + 1], [(1, 1, "reduce")], y_c, first=at)
            out += red
            at += 1
            ic = r_c + skips[k]
    return out


def build_graph(builder_cls, weights, in_shape=(1, 416, 416, 3)):
    """Return (graph, nodes, outs): nodes in creation order, outs the three head nodes (stride 32,
    16, 8); the first two are the graph's extra outputs, the third its primary one."""
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
        for w in weights[at:at + 5]:
            x = conv_block(x, w)
        y = x
        head = conv_block(conv_block(y, weights[at + 5]), weights[at + 6], linear=True)
        outs.append(head)
        at += N_SCALE
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


class YOLO_V3(object):
    """YOLOv3 with the MI355X engine underneath: in_shape [batch, h, w, 3] with h, w multiples of
    32.  `head` is a yolo_post.MultiHead of three scales (grids in / 32, in / 16, in / 8); without
    one, MultiHead.yolov3 for the class count the last layers' width implies (n_out = 3 x (5 +
    classes))."""

    def __init__(self, in_shape, weights, debug, device=None, head=None):
        if len(in_shape) != 4:
            raise ValueError(f"in_shape {in_shape!r}: [batch, height, width, channels] expected")
        if in_shape[1] % 32 or in_shape[2] % 32 or in_shape[1] <= 0 or in_shape[2] <= 0:
            raise ValueError(f"in_shape {in_shape!r}: height and width must be multiples of 32")
        self.in_shape = tuple(in_shape)
        w = validate(weights)
        n_out = w[N_TRUNK + N_SCALE - 1]["kernel"].shape[3]
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

    def inference(self, im):
        """The three head tensors, stride 32 first."""
        return self.sess.run_all(im)

    def postprocessing(self, outs):
        """Boxes of one image of inference()'s outputs."""
        rows = yolo_post.detect_batch_multi([np.asarray(o, np.float32) for o in outs], self.head)
        if len(rows) != 1:
            raise ValueError(f"postprocessing expects one image, got {len(rows)}")
        return yolo_post.label_boxes(rows[0], self.head)

    def _device_buffers(self, plan, device):
        """detect's device tensors (input, output, the tap pointers in head order) and
        self.buffers, made on first use."""
        import torch
        if self._dev is None:
            order = [[id(e.node) for e in plan.tap_entries].index(id(o)) for o in self.outs[:-1]]
            self._dev = {
                "in": torch.empty((plan.batch,) + plan.in_shape, dtype=torch.float32, device=device),
                "out": torch.empty((plan.batch,) + plan.out_shape, dtype=torch.float32, device=device),
                "taps": [plan.tap_buffer(k)[0] for k in order],
            }
            self.buffers = yolo_post.MultiDetectionBuffers(plan.batch, device, self.head)
        return self._dev

    def detect(self, frames, raise_errors=True):
        """Plan and decode on the device for [n <= batch, h, w, 3] host frames: per image the rows
        of yolo_post.detect_batch_multi.  The decode reads the plan's two tap buffers and its
        output buffer in place.  Leaves dets / counts in self.buffers (a
        yolo_post.MultiDetectionBuffers), ready for its pack()."""
        import torch
        x = np.ascontiguousarray(frames, dtype=np.float32)
        n = x.shape[0]
        plan = self.sess.plan()
        if tuple(x.shape[1:]) != plan.in_shape or n > plan.batch:
            raise ValueError(f"frames {x.shape} do not fit plan [{plan.batch}, {plan.in_shape}]")
        device = torch.device("cuda", plan.device)
        d = self._device_buffers(plan, device)
        with torch.cuda.device(device):
            stream = torch.cuda.current_stream().cuda_stream
            d["in"][:n].copy_(torch.from_numpy(x))
            plan.run_device(n, d["in"].data_ptr(), d["out"].data_ptr(), stream)
            self.buffers.run(d["taps"] + [d["out"].data_ptr()], n, stream)
            dets = self.buffers.dets[:n].cpu().numpy()
            counts = self.buffers.counts[:n].cpu().numpy()
        return yolo_post.DetectionBuffers.to_rows(dets, counts, self.buffers.max_det, raise_errors)
