"""YOLOv2-tiny model front-end on the MI355X engine — the reference's
`cs492-projects/proj3/yolov2tiny.py` interface for this path:

    y2t = YOLO_V2_TINY([1, 416, 416, 3], "y2t_weights.pickle", debug)   # yolov2tiny.py:7-13
    out = y2t.inference(frame)                                           # :80-82
    boxes = postprocessing(np.squeeze(out))                              # :94-176

The graph is the reference's node chain (yolo_graph.build_graph = yolov2tiny.py:25-79) on
dnn_hip's DnnGraphBuilder / DnnInferenceEngine; the weights come from the pickle through the
safe loader (yolo_weights.py; the reference's own get_y2t_w raises on Python 3.10), or a
list of layer dicts in the same format may be passed directly.  `postprocessing` runs on the
GPU (yolo_post.py).

The same weights run at any input size that is a multiple of 32 (YOLOv2's multi-scale use):
`y2t.head` is the yolo_post.YoloHead of `in_shape` (in_h / 32 x in_w / 32 cells) and
`y2t.postprocessing(out)` decodes that grid.  The class count follows the last layer's width
(5 anchors x (5 + classes); 125 = the 20 VOC names).  A model with other anchors or thresholds
passes a YoloHead as `head=` (its grid is replaced by in_shape's); its last layer must then be
head.n_out wide.
"""
import dnn_hip
import yolo_graph
import yolo_post
import yolo_weights

postprocessing = yolo_post.postprocessing


def _head_for(in_shape, proto, n_out=125):
    """The YoloHead of in_shape's grid (raises unless in_h and in_w are multiples of the cell):
    `proto`'s anchors, classes and thresholds, or the reference's 5 VOC anchors with the class
    count that makes the last layer n_out wide."""
    if proto is not None:
        kw = dict(cell=proto.cell, anchors=proto.anchors, classes=proto.names or proto.n_classes,
                  score_thr=proto.score_thr, iou_thr=proto.iou_thr)
    else:
        n_cls = n_out // 5 - 5
        if n_out % 5 or n_cls < 1:
            raise ValueError(f"last layer has {n_out} outputs, not 5 anchors x (5 + classes): pass head=")
        kw = dict(classes=yolo_post.CLASSES if n_cls == len(yolo_post.CLASSES) else n_cls)
    return yolo_post.YoloHead.for_input(in_shape[1], in_shape[2], **kw)


class YOLO_V2_TINY(object):
    """yolov2tiny.py:7-82 with the MI355X engine underneath."""

    def __init__(self, in_shape, weight_pickle, debug, device=None, head=None):
        self.weight_pickle = weight_pickle
        if len(in_shape) != 4:
            raise ValueError(f"in_shape {in_shape!r}: [batch, height, width, channels] expected")
        self.in_shape, self._head_proto = tuple(in_shape), head
        self.head = _head_for(in_shape, head)  # before anything is loaded: a bad in_shape raises here
        self.g = dnn_hip.DnnGraphBuilder()
        self.build_graph(in_shape)
        self.sess = dnn_hip.DnnInferenceEngine(self.g, debug, device=device)

    def get_y2t_w(self):
        n_out = None if self._head_proto is None else self.head.n_out
        if isinstance(self.weight_pickle, (list, tuple)):
            w = yolo_weights.validate(self.weight_pickle, n_out)
        else:
            w = yolo_weights.load_y2t_weights(self.weight_pickle, n_out)
        if n_out is None:  # the class count follows the last layer's width
            self.head = _head_for(self.in_shape, None, w[-1]["kernel"].shape[3])
        return w

    def build_graph(self, in_shape):
        y2t_w = self.get_y2t_w()
        self.g, self.nodes = yolo_graph.build_graph(lambda: self.g, y2t_w, in_shape=tuple(in_shape))

    def inference(self, im):
        return self.sess.run(im)

    def postprocessing(self, out):
        """yolov2tiny.py:94-177 on this model's grid: `out` is one image of inference()'s
        output, [1, in_h / 32, in_w / 32, n_out]."""
        return yolo_post.postprocessing(out, head=self.head)
