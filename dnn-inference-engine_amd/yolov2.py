"""Full YOLOv2 (Darknet-19 + passthrough) on the MI355X engine, built like
yolov2tiny.YOLO_V2_TINY:

    y2 = YOLO_V2([1, 416, 416, 3], weights, debug)
    out = y2.inference(frame)             # [1, 13, 13, 425]
    boxes = y2.postprocessing(out[0:1])

The reference has no such model (its graph nodes cannot fork); the topology is the public
YOLOv2 one:

    trunk        Darknet-19's 18 convs (3x3 and 1x1, BatchNorm + leaky) and 5 2x2/s2 pools
    tail         conv19, conv20: 3x3 x 1024 on the 13 x 13 trunk
    passthrough  a 1x1 x 64 conv on the trunk's last 512-channel activation (26 x 26, before the
                 fifth pool), SpaceToDepth(2) -> 13 x 13 x 256, Concat([passthrough, tail]) -> 1280
    head         conv 3x3 x 1024, then a linear 1x1 x n_out conv with bias only

`weights` is a list of 23 layer dicts in the yolo_weights format (kernel HWIO, biases, and
moving_mean / moving_variance / gamma for all but the last), in the order trunk, tail,
passthrough conv, joined conv, head (synth.yolov2_weights makes synthetic ones; its width_div
gives a narrow model).  The channel counts follow the kernels, so a narrow model is the same code.

SpaceToDepth uses TensorFlow's channel order ((dy*2 + dx)*C + c), not Darknet's reorg order:
weights converted from a Darknet checkpoint need the input channels of the joined conv permuted.

The default head is COCO-shaped: 5 anchors x (5 + 80 classes) = 425 outputs on an in / 32 grid.
"""
import numpy as np

import dnn_hip
import yolo_post
import yolo_weights

EPS = 1e-5
N_TRUNK, N_TAIL = 18, 2
N_LAYERS = N_TRUNK + N_TAIL + 3
POOL_AFTER = (0, 1, 4, 7, 12)  # trunk convs followed by a 2x2/s2 pool
PASSTHROUGH_FROM = 12          # the passthrough forks off this trunk conv's output, before its pool
COCO_ANCHORS = (0.57273, 0.677385, 1.87446, 2.06253, 3.33843, 5.47434, 7.88282, 3.52778, 9.77052, 9.16828)
COCO_CLASSES = 80


def validate(weights, n_out=None):
    """Check the 23-layer structure (keys, shapes chaining through the passthrough join) and
    return it as fp32 contiguous arrays."""
    if not isinstance(weights, (list, tuple)) or len(weights) != N_LAYERS:
        raise yolo_weights.WeightFileError(f"expected a list of {N_LAYERS} layer dicts")
    out = []
    for i, w in enumerate(weights):
        keys = ("kernel", "biases") + (yolo_weights.BN_KEYS if i < N_LAYERS - 1 else ())
        if not isinstance(w, dict) or any(k not in w for k in keys):
            raise yolo_weights.WeightFileError(f"layer {i}: expected a dict with {keys}")
        d = {k: np.ascontiguousarray(np.asarray(w[k]), dtype=np.float32) for k in keys}
        k = d["kernel"]
        if k.ndim != 4 or k.shape[0] != k.shape[1] or k.shape[0] not in (1, 3):
            raise yolo_weights.WeightFileError(f"layer {i}: kernel shape {k.shape}, expected 1x1 or 3x3 HWIO")
        for key in keys[1:]:
            if d[key].shape != (k.shape[3],):
                raise yolo_weights.WeightFileError(f"layer {i} {key}: shape {d[key].shape}, expected ({k.shape[3]},)")
        out.append(d)
    od = [w["kernel"].shape[3] for w in out]
    want_in = [3] + od[:N_TRUNK + N_TAIL - 1]                      # trunk and tail chain
    want_in.append(od[PASSTHROUGH_FROM])                           # passthrough conv
    want_in.append(4 * od[N_TRUNK + N_TAIL] + od[N_TRUNK + N_TAIL - 1])  # joined conv
    want_in.append(od[N_TRUNK + N_TAIL + 1])                       # head
    for i, (w, ic) in enumerate(zip(out, want_in)):
        if w["kernel"].shape[2] != ic:
            raise yolo_weights.WeightFileError(f"layer {i}: {w['kernel'].shape[2]} input channels, expected {ic}")
    if n_out is not None and od[-1] != n_out:
        raise yolo_weights.WeightFileError(f"last layer has {od[-1]} outputs; this head needs {n_out}")
    return out


def build_graph(builder_cls, weights, in_shape=(1, 416, 416, 3)):
    """Return (graph, nodes): nodes in creation order, on any module with dnn_hip's builder API."""
    g = builder_cls()
    nodes = []
    s1 = [1, 1, 1, 1]

    def conv_block(x, w, linear=False):
        x = g.create_conv2d(x, w["kernel"], strides=s1, padding="SAME")
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
    fork = None
    for i in range(N_TRUNK + N_TAIL):
        x = conv_block(x, weights[i])
        if i == PASSTHROUGH_FROM:
            fork = x
        if i in POOL_AFTER:
            x = g.create_max_pool2d(x, ksize=[1, 2, 2, 1], strides=[1, 2, 2, 1], padding="SAME")
            nodes.append(x)
    p = conv_block(fork, weights[N_TRUNK + N_TAIL])
    p = g.create_space_to_depth(p, 2)
    nodes.append(p)
    x = g.create_concat([p, x])
    nodes.append(x)
    x = conv_block(x, weights[N_TRUNK + N_TAIL + 1])
    x = conv_block(x, weights[N_TRUNK + N_TAIL + 2], linear=True)
    g.set_out_node(x)
    return g, nodes


def _head_for(in_shape, proto, n_out):
    if proto is not None:
        kw = dict(cell=proto.cell, anchors=proto.anchors, classes=proto.names or proto.n_classes,
                  score_thr=proto.score_thr, iou_thr=proto.iou_thr)
    else:
        n_anchors = len(COCO_ANCHORS) // 2
        n_cls = n_out // n_anchors - 5
        if n_out % n_anchors or n_cls < 1:
            raise ValueError(f"last layer has {n_out} outputs, not {n_anchors} anchors x (5 + classes): pass head=")
        kw = dict(anchors=COCO_ANCHORS, classes=n_cls)
    return yolo_post.YoloHead.for_input(in_shape[1], in_shape[2], **kw)


class YOLO_V2(object):
    """Full YOLOv2 with the MI355X engine underneath: in_shape [batch, h, w, 3] with h, w
    multiples of 32; `head` a yolo_post.YoloHead for other anchors / classes / thresholds (its
    grid is replaced by in_shape's), default the COCO-shaped one of the last layer's width."""

    def __init__(self, in_shape, weights, debug, device=None, head=None):
        if len(in_shape) != 4:
            raise ValueError(f"in_shape {in_shape!r}: [batch, height, width, channels] expected")
        self.in_shape = tuple(in_shape)
        self.head = _head_for(in_shape, head, COCO_CLASSES * 5 + 25)  # a bad in_shape raises before any work
        w = validate(weights, None if head is None else self.head.n_out)
        if head is None:
            self.head = _head_for(in_shape, None, w[-1]["kernel"].shape[3])
        self.g, self.nodes = build_graph(dnn_hip.DnnGraphBuilder, w, in_shape=self.in_shape)
        self.sess = dnn_hip.DnnInferenceEngine(self.g, debug, device=device)

    def inference(self, im):
        return self.sess.run(im)

    def postprocessing(self, out):
        """Boxes of one image of inference()'s output, [1, in_h / 32, in_w / 32, n_out]."""
        return yolo_post.postprocessing(out, head=self.head)
