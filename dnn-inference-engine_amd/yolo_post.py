"""YOLOv2 postprocessing on the GPU — drop-in for the reference's host-side
`postprocessing(predictions)` (cs492-projects/proj3/yolov2tiny.py:94-234).

    from yolo_post import postprocessing          # same name, argument and return value
    label_boxes = postprocessing(engine.run(frame))  # [(name, (l, t), (r, b), color)]

The work runs in `dnn_yolo_postprocess` (include/dnn_hip_post.h, csrc/postprocess.hip):
decode + threshold + sort + greedy NMS, one workgroup per image.  `detect_batch` handles a
whole [B,13,13,125] batch in one launch, and `DetectionBuffers` keeps the outputs on the
device for the multi-GPU detection gather (dist.py).  There is no CPU fallback: a missing
library raises (dnn_hip.load_library).

Any other head — another grid (input size / 32), anchor list or class count — is described by
a `YoloHead` and passed as `head=` to the same functions; they then run
`dnn_yolo_postprocess_head` (csrc/postprocess_head.hip).  `head=None` is the path above.

    head = YoloHead.for_input(608, 608)              # 19 x 19 cells, VOC anchors and classes
    rows = detect_batch(pred, head=head)             # pred [B,19,19,125]
"""
import collections
import ctypes

import math

import numpy as np

import dnn_hip

N_BOXES = 845  # DNN_YOLO_BOXES: 13 * 13 * 5, the most detections an image can have
PRED_FLOATS = 13 * 13 * 125

MAX_BOXES, MAX_ANCHORS, MAX_CLASSES = 8192, 16, 128  # DNN_YOLO_MAX_* (include/dnn_hip_post.h)

# yolov2tiny.py:102-115 (data)
ANCHORS = (1.08, 1.19, 3.42, 4.41, 6.63, 11.38, 9.42, 5.11, 16.62, 10.52)
CLASSES = ("aeroplane", "bicycle", "bird", "boat", "bottle", "bus", "car", "cat", "chair", "cow", "diningtable",
           "dog", "horse", "motorbike", "person", "pottedplant", "sheep", "sofa", "train", "tvmonitor")
COLORS = ((254.0, 254.0, 254), (239.88888888888889, 211.66666666666669, 127),
          (225.77777777777777, 169.33333333333334, 0), (211.66666666666669, 127.0, 254),
          (197.55555555555557, 84.66666666666667, 127), (183.44444444444443, 42.33333333333332, 0),
          (169.33333333333334, 0.0, 254), (155.22222222222223, -42.33333333333335, 127),
          (141.11111111111111, -84.66666666666664, 0), (127.0, 254.0, 254),
          (112.88888888888889, 211.66666666666669, 127), (98.77777777777777, 169.33333333333334, 0),
          (84.66666666666667, 127.0, 254), (70.55555555555556, 84.66666666666667, 127),
          (56.44444444444444, 42.33333333333332, 0), (42.33333333333332, 0.0, 254),
          (28.222222222222236, -42.33333333333335, 127), (14.111111111111118, -84.66666666666664, 0),
          (0.0, 254.0, 254), (-14.111111111111118, 211.66666666666669, 127))


class Detection(ctypes.Structure):
    """dnn_detection (include/dnn_hip_post.h), 40 bytes."""
    _fields_ = [("cls", ctypes.c_int), ("score", ctypes.c_float), ("left", ctypes.c_longlong),
                ("top", ctypes.c_longlong), ("right", ctypes.c_longlong), ("bottom", ctypes.c_longlong)]


DETECTION_DTYPE = np.dtype([("cls", "<i4"), ("score", "<f4"), ("left", "<i8"), ("top", "<i8"), ("right", "<i8"),
                            ("bottom", "<i8")])
assert DETECTION_DTYPE.itemsize == ctypes.sizeof(Detection) == 40


class HeadStruct(ctypes.Structure):
    """dnn_yolo_head (include/dnn_hip_post.h)."""
    _fields_ = [("grid_h", ctypes.c_int), ("grid_w", ctypes.c_int), ("n_anchors", ctypes.c_int),
                ("n_classes", ctypes.c_int), ("cell", ctypes.c_float), ("score_thr", ctypes.c_float),
                ("iou_thr", ctypes.c_double), ("anchors", ctypes.c_float * 32)]


MAX_SCALES, MULTI_MAX_BOXES = 4, 16384  # DNN_YOLO_MAX_SCALES, DNN_YOLO_MULTI_MAX_BOXES
CLASS_MODES = {"softmax": 0, "logistic": 1}
NMS_MODES = {"any": 0, "per_class": 1}  # DNN_YOLO_NMS_ANY_CLASS, DNN_YOLO_NMS_PER_CLASS
LABEL_MODES = {"argmax": 0, "multi": 1}  # DNN_YOLO_LABELS_ARGMAX, DNN_YOLO_LABELS_MULTI
MULTI_MAX_CANDIDATES = 16384  # DNN_YOLO_MULTI_MAX_CANDIDATES: (box, class) pairs above the threshold
WIDE_MAX_BOXES = 65536  # DNN_YOLO_WIDE_MAX_BOXES: the box limit of a WideHead


class MultiStruct(ctypes.Structure):
    """dnn_yolo_multi (include/dnn_hip_post.h)."""
    _fields_ = [("n_scales", ctypes.c_int), ("class_mode", ctypes.c_int), ("scale", HeadStruct * MAX_SCALES)]


class ImageSize(ctypes.Structure):
    """dnn_image_size (include/dnn_hip_post.h)."""
    _fields_ = [("h", ctypes.c_int), ("w", ctypes.c_int)]


def _sizes(sizes):
    """[(h, w), ...] as a ctypes array of ImageSize (one spare element, so an empty list has an address)."""
    arr = (ImageSize * (len(sizes) + 1))()
    for k, (h, w) in enumerate(sizes):
        arr[k] = ImageSize(int(h), int(w))
    return arr


def _bind(lib):
    vp, i, u64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_ulonglong
    hp, mp, pp = ctypes.POINTER(HeadStruct), ctypes.POINTER(MultiStruct), ctypes.POINTER(vp)
    fp, sp, bp = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ImageSize), ctypes.POINTER(u64)
    for name, argtypes in {  # every entry returns int
            "dnn_yolo_head_voc": [i, i, hp],
            "dnn_yolo_head_boxes": [hp],
            "dnn_yolo_head_workspace": [hp, i, bp],
            "dnn_yolo_postprocess_head": [hp, vp, i, vp, i, vp, vp, u64, vp],
            "dnn_yolo_postprocess_head_host": [hp, vp, i, vp, i, vp],
            "dnn_yolo_postprocess": [vp, i, vp, i, vp, vp],
            "dnn_yolo_postprocess_host": [vp, i, vp, i, vp],
            "dnn_yolo_pack_detections": [vp, vp, i, i, vp, vp, vp],
            "dnn_yolo_multi_boxes": [mp],
            "dnn_yolo_multi_workspace": [mp, i, bp],
            "dnn_yolo_postprocess_multi": [mp, pp, i, vp, i, vp, vp, u64, vp],
            "dnn_yolo_postprocess_multi_host": [mp, pp, i, vp, i, vp],
            "dnn_yolo_multi_nms_workspace": [mp, i, i, bp],
            "dnn_yolo_postprocess_multi_nms": [mp, pp, i, vp, i, vp, vp, u64, i, vp],
            "dnn_yolo_postprocess_multi_nms_host": [mp, pp, i, vp, i, vp, i],
            "dnn_yolo_multi_labels_workspace": [mp, i, i, bp],
            "dnn_yolo_postprocess_multi_labels": [mp, pp, i, vp, i, vp, vp, u64, i, vp],
            "dnn_yolo_postprocess_multi_labels_host": [mp, pp, i, vp, i, vp, i],
            "dnn_yolo_wide_boxes": [mp],
            "dnn_yolo_wide_workspace": [mp, i, bp],
            "dnn_yolo_postprocess_wide": [mp, pp, i, vp, i, vp, vp, u64, i, i, vp],
            "dnn_yolo_postprocess_wide_host": [mp, pp, i, vp, i, vp, i, i],
            "dnn_yolo_postprocess_multi_xy": [mp, fp, pp, i, vp, i, vp, vp, u64, i, i, vp],
            "dnn_yolo_postprocess_multi_xy_host": [mp, fp, pp, i, vp, i, vp, i, i],
            "dnn_yolo_postprocess_wide_xy": [mp, fp, pp, i, vp, i, vp, vp, u64, i, i, vp],
            "dnn_yolo_postprocess_wide_xy_host": [mp, fp, pp, i, vp, i, vp, i, i],
            "dnn_yolo_correct_detections": [vp, vp, i, i, sp, i, i, vp],
            "dnn_yolo_correct_detections_host": [vp, vp, i, i, sp, i, i],
    }.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = i, argtypes
    return lib


_lib = _bind(dnn_hip.mylib)


ERRORS = {-1: "a box corner is not finite or out of int64 range (the reference's int() raises there)",
          -2: "an IoU denominator is zero (the reference raises ZeroDivisionError)",
          -3: f"more than {MULTI_MAX_CANDIDATES} multi-label candidates (box, class) above the score threshold"}


class YoloHead(object):
    """What yolov2tiny.py:96-162 fixes for the 416 x 416 VOC model, as parameters: `grid` cells
    (an int or (rows, cols)), `anchors` (w, h pairs in cells), `classes` (a tuple of names, or
    a count), `cell` pixels per cell and the two thresholds.  Validates like the C side
    (dnn_yolo_head_boxes) and raises ValueError."""

    def __init__(self, grid, anchors=ANCHORS, classes=CLASSES, cell=32.0, score_thr=0.3, iou_thr=0.3):
        try:
            gh, gw = grid
        except TypeError:
            gh = gw = grid
        if int(gh) != gh or int(gw) != gw:
            raise ValueError(f"grid {grid!r}: whole numbers of cells expected")
        self.grid_h, self.grid_w = int(gh), int(gw)
        self.anchors = tuple(float(a) for a in anchors)
        if isinstance(classes, (int, np.integer)):
            self.names, self.n_classes = None, int(classes)
        else:
            self.names = tuple(classes)
            self.n_classes = len(self.names)
        self.cell, self.score_thr, self.iou_thr = float(cell), float(score_thr), float(iou_thr)
        if len(self.anchors) % 2 or not 1 <= len(self.anchors) // 2 <= MAX_ANCHORS:
            raise ValueError(f"{len(self.anchors)} anchor values: need (w, h) pairs for 1..{MAX_ANCHORS} anchors")
        self.n_anchors = len(self.anchors) // 2
        if not 1 <= self.n_classes <= MAX_CLASSES:
            raise ValueError(f"{self.n_classes} classes: need 1..{MAX_CLASSES}")
        if self.grid_h < 1 or self.grid_w < 1 or self.grid_h * self.grid_w * self.n_anchors > MAX_BOXES:
            raise ValueError(f"{self.grid_h} x {self.grid_w} cells x {self.n_anchors} anchors: need 1..{MAX_BOXES} "
                             "boxes")
        if not (np.float32(self.score_thr) >= 0) or math.isnan(self.iou_thr):
            raise ValueError(f"score_thr {score_thr!r} must be >= 0 and iou_thr {iou_thr!r} a number")
        if not (np.float32(self.cell) > 0 and np.isfinite(np.float32(self.cell))):
            raise ValueError(f"cell {cell!r} must be a finite number of pixels > 0")
        if not np.all(np.isfinite(np.asarray(self.anchors, np.float32))):
            raise ValueError("anchors must be finite")
        self.boxes = self.grid_h * self.grid_w * self.n_anchors
        self.n_out = self.n_anchors * (5 + self.n_classes)
        self.pred_shape = (self.grid_h, self.grid_w, self.n_out)
        self.pred_floats = self.grid_h * self.grid_w * self.n_out
        self.c = HeadStruct(self.grid_h, self.grid_w, self.n_anchors, self.n_classes, self.cell, self.score_thr,
                            self.iou_thr, (ctypes.c_float * 32)(*self.anchors))
        n = _lib.dnn_yolo_head_boxes(ctypes.byref(self.c))
        if n != self.boxes:
            raise ValueError(f"dnn_yolo_head_boxes: {n}: {dnn_hip.last_error()}")

    @classmethod
    def for_input(cls, h, w, cell=32.0, **kw):
        """The head of an h x w pixel input (yolov2tiny.py:129: 416 / 13 = 32): both must be
        multiples of `cell`."""
        if h < cell or w < cell or h % cell or w % cell:
            raise ValueError(f"input {h} x {w}: height and width must be multiples of {cell:g}")
        return cls((int(h // cell), int(w // cell)), cell=cell, **kw)

    def workspace_bytes(self, n_images):
        b = ctypes.c_ulonglong(0)
        dnn_hip._check(_lib.dnn_yolo_head_workspace(ctypes.byref(self.c), n_images, ctypes.byref(b)),
                       "dnn_yolo_head_workspace")
        return int(b.value)

    def __repr__(self):
        return (f"YoloHead({self.grid_h}x{self.grid_w} cells, {self.n_anchors} anchors, {self.n_classes} classes, "
                f"cell {self.cell:g}, score > {self.score_thr:g}, IoU > {self.iou_thr:g})")


Scale = collections.namedtuple("Scale", "grid_h grid_w n_anchors n_classes anchors cell score_thr iou_thr")
Scale.__doc__ = """One scale of a MultiHead: a YoloHead's fields without its own 8192-box limit."""

# the public YOLOv3 anchor table: stride -> (w, h) pairs in pixels
YOLOV3_ANCHORS = ((32, (116, 90, 156, 198, 373, 326)), (16, (30, 61, 62, 45, 59, 119)), (8, (10, 13, 16, 30, 33, 23)))


# the public YOLOv3-tiny anchor table, two scales
YOLOV3_TINY_ANCHORS = ((32, (81, 82, 135, 169, 344, 319)), (16, (10, 14, 23, 27, 37, 58)))


class MultiHead(object):
    """Several heads whose boxes compete in one sort and one NMS (dnn_yolo_multi): `scales` is a
    sequence of 1..4 heads (YoloHead, Scale, or anything with their fields), scale 0's boxes
    first; class_mode "logistic" (YOLOv3: one sigmoid per class) or "softmax" (YOLOv2).  All
    scales must agree on classes and thresholds and have at most 16384 boxes together.  nms "any"
    is the reference's class-agnostic greedy NMS; "per_class" is Darknet's / torchvision
    batched_nms's rule, where a box is suppressed only by a kept box of its own class.  labels
    "argmax" gives a box one class, the arg-max; "multi" is Darknet's multi-label output, one
    detection per class whose score conf * p[class] is above the threshold, so an image can have
    more rows than boxes (`max_det`; at most 16384 candidates, else the image's code is -3).  It
    needs nms="per_class": under the class-agnostic rule a box's second label is always suppressed
    by its first.  scale_x_y is Darknet's [yolo] key of that name (YOLOv4, YOLOv4-tiny): None, or
    one finite float > 0 per scale; the box centre's logistic becomes sig * s - 0.5 * (s - 1) in
    fp32 (the dnn_yolo_postprocess_*_xy entries).  None calls exactly the entries without it.
    Validates like the C side (dnn_yolo_multi_boxes) and raises ValueError."""

    MAX_BOXES = MULTI_MAX_BOXES         # the most boxes over all scales (WideHead: WIDE_MAX_BOXES)
    BOXES_ENTRY = "dnn_yolo_multi_boxes"  # the C function that validates the description and counts them

    def __init__(self, scales, class_mode="logistic", nms="any", labels="argmax", scale_x_y=None):
        scales = list(scales)
        if scale_x_y is not None:
            scale_x_y = tuple(float(v) for v in scale_x_y)
            if len(scale_x_y) != len(scales):
                raise ValueError(f"{len(scale_x_y)} scale_x_y values for {len(scales)} scales")
            if not all(np.float32(v) > 0 and np.isfinite(np.float32(v)) for v in scale_x_y):
                raise ValueError(f"scale_x_y {scale_x_y!r}: finite values > 0 expected")
        self.scale_x_y = scale_x_y
        # the host array the _xy entries read (NULL: every scale 1, the entries without the argument)
        self.xy = None if scale_x_y is None else (ctypes.c_float * len(scale_x_y))(*scale_x_y)
        if not 1 <= len(scales) <= MAX_SCALES:
            raise ValueError(f"{len(scales)} scales: need 1..{MAX_SCALES}")
        if class_mode not in CLASS_MODES:
            raise ValueError(f"class_mode {class_mode!r}: need one of {sorted(CLASS_MODES)}")
        if nms not in NMS_MODES:
            raise ValueError(f"nms {nms!r}: need one of {sorted(NMS_MODES)}")
        if not isinstance(labels, str) or labels not in LABEL_MODES:
            raise ValueError(f"labels {labels!r}: need one of {sorted(LABEL_MODES)}")
        if labels == "multi" and nms != "per_class":
            raise ValueError('labels "multi" needs nms "per_class": under the class-agnostic rule a box\'s second '
                             "label is always suppressed by its first")
        self.class_mode, self.nms, self.labels = class_mode, nms, labels
        self.scales = []
        for s in scales:
            anchors = tuple(float(a) for a in s.anchors)
            if len(anchors) % 2 or not 1 <= len(anchors) // 2 <= MAX_ANCHORS or len(anchors) != 2 * s.n_anchors:
                raise ValueError(f"{len(anchors)} anchor values: need (w, h) pairs for {s.n_anchors} of 1.."
                                 f"{MAX_ANCHORS} anchors")
            if int(s.grid_h) != s.grid_h or int(s.grid_w) != s.grid_w or s.grid_h < 1 or s.grid_w < 1:
                raise ValueError(f"grid {s.grid_h} x {s.grid_w}: whole numbers of cells >= 1 expected")
            if not 1 <= s.n_classes <= MAX_CLASSES:
                raise ValueError(f"{s.n_classes} classes: need 1..{MAX_CLASSES}")
            if not (np.float32(s.score_thr) >= 0) or math.isnan(s.iou_thr):
                raise ValueError(f"score_thr {s.score_thr!r} must be >= 0 and iou_thr {s.iou_thr!r} a number")
            if not (np.float32(s.cell) > 0 and np.isfinite(np.float32(s.cell))):
                raise ValueError(f"cell {s.cell!r} must be a finite number of pixels > 0")
            if not np.all(np.isfinite(np.asarray(anchors, np.float32))):
                raise ValueError("anchors must be finite")
            self.scales.append(Scale(int(s.grid_h), int(s.grid_w), int(s.n_anchors), int(s.n_classes), anchors,
                                     float(s.cell), float(s.score_thr), float(s.iou_thr)))
        s0 = self.scales[0]
        for k, s in enumerate(self.scales):
            if (s.n_classes, np.float32(s.score_thr), s.iou_thr) != (s0.n_classes, np.float32(s0.score_thr), s0.iou_thr):
                raise ValueError(f"scale {k}: classes and thresholds must be those of scale 0")
        self.names = getattr(scales[0], "names", None)
        self.n_classes, self.score_thr, self.iou_thr = s0.n_classes, s0.score_thr, s0.iou_thr
        self.scale_boxes = [s.grid_h * s.grid_w * s.n_anchors for s in self.scales]
        self.boxes = sum(self.scale_boxes)
        if self.boxes > self.MAX_BOXES:
            raise ValueError(f"{self.boxes} boxes over {len(self.scales)} scales: need <= {self.MAX_BOXES}")
        # the most rows an image can have: the default row capacity of detect_batch_multi and the buffers
        # (a candidate per box, or with "multi" per box and class; a WideHead has more boxes than candidates)
        self.max_det = min(self.boxes * (1 if labels == "argmax" else self.n_classes), MULTI_MAX_CANDIDATES)
        self.n_out = [s.n_anchors * (5 + s.n_classes) for s in self.scales]
        self.pred_shapes = [(s.grid_h, s.grid_w, n) for s, n in zip(self.scales, self.n_out)]
        self.pred_floats = [h * w * c for h, w, c in self.pred_shapes]
        self.c = MultiStruct()
        self.c.n_scales, self.c.class_mode = len(self.scales), CLASS_MODES[class_mode]
        for k, s in enumerate(self.scales):
            self.c.scale[k] = HeadStruct(s.grid_h, s.grid_w, s.n_anchors, s.n_classes, s.cell, s.score_thr, s.iou_thr,
                                         (ctypes.c_float * 32)(*s.anchors))
        n = getattr(_lib, self.BOXES_ENTRY)(ctypes.byref(self.c))
        if n != self.boxes:
            raise ValueError(f"{self.BOXES_ENTRY}: {n}: {dnn_hip.last_error()}")

    @classmethod
    def yolov3(cls, in_h, in_w, classes=80, score_thr=0.3, iou_thr=0.3, nms="any", labels="argmax"):
        """YOLOv3's three heads for an in_h x in_w input (multiples of 32): strides 32, 16, 8 with
        the public anchor table, the pixel anchors divided by the stride (exact in fp32: every
        stride is a power of two), logistic class scores."""
        if in_h < 32 or in_w < 32 or in_h % 32 or in_w % 32:
            raise ValueError(f"input {in_h} x {in_w}: height and width must be multiples of 32")
        n_classes = classes if isinstance(classes, (int, np.integer)) else len(classes)
        scales = [Scale(in_h // st, in_w // st, 3, int(n_classes), tuple(a / st for a in px), float(st), score_thr,
                        iou_thr) for st, px in YOLOV3_ANCHORS]
        head = cls(scales, "logistic", nms, labels)
        head.names = None if isinstance(classes, (int, np.integer)) else tuple(classes)
        return head

    @classmethod
    def yolov3_tiny(cls, in_h, in_w, classes=80, score_thr=0.3, iou_thr=0.3, nms="any", labels="argmax"):
        """YOLOv3-tiny's two heads for an in_h x in_w input (multiples of 32): strides 32 and 16
        with the public anchor table (the stride-16 head takes the three smallest anchors, the
        official cfg's mask 0,1,2), the pixel anchors divided by the stride (exact in fp32),
        logistic class scores."""
        if in_h < 32 or in_w < 32 or in_h % 32 or in_w % 32:
            raise ValueError(f"input {in_h} x {in_w}: height and width must be multiples of 32")
        n_classes = classes if isinstance(classes, (int, np.integer)) else len(classes)
        scales = [Scale(in_h // st, in_w // st, 3, int(n_classes), tuple(a / st for a in px), float(st), score_thr,
                        iou_thr) for st, px in YOLOV3_TINY_ANCHORS]
        head = cls(scales, "logistic", nms, labels)
        head.names = None if isinstance(classes, (int, np.integer)) else tuple(classes)
        return head

    def _entry(self, form):
        """form "device", "host" or "workspace" -> (the C entry of that form for this head's modes, its
        trailing mode arguments): the _xy entry with scale_x_y, else the _labels entry for labels
        "multi", else the _nms entry."""
        nms, labels = NMS_MODES[self.nms], LABEL_MODES[self.labels]
        if self.xy is not None and form != "workspace":
            kind, tail = "_xy", (nms, labels)
        else:
            kind, tail = ("_labels", (labels,)) if self.labels == "multi" else ("_nms", (nms,))
        if form == "workspace":
            return f"dnn_yolo_multi{kind}_workspace", tail
        return "dnn_yolo_postprocess_multi" + kind + ("_host" if form == "host" else ""), tail

    def _call(self, form, args, last=()):
        """Calls _entry(form): the description (and scale_x_y, where the entry takes it), args, the mode
        arguments, last."""
        name, tail = self._entry(form)
        lead = (ctypes.byref(self.c),) if self.xy is None or form == "workspace" else (ctypes.byref(self.c), self.xy)
        dnn_hip._check(getattr(_lib, name)(*lead, *args, *tail, *last), name)

    def workspace_bytes(self, n_images):
        b = ctypes.c_ulonglong(0)
        self._call("workspace", (n_images,), (ctypes.byref(b),))
        return int(b.value)

    def __repr__(self):
        grids = ", ".join(f"{s.grid_h}x{s.grid_w}x{s.n_anchors}" for s in self.scales)
        nms = "" if self.nms == "any" else f", NMS {self.nms}"
        labels = "" if self.labels == "argmax" else f", labels {self.labels}"
        xy = "" if self.scale_x_y is None else ", scale_x_y " + ",".join(f"{v:g}" for v in self.scale_x_y)
        return (f"{type(self).__name__}({grids}; {self.n_classes} classes, {self.class_mode}, score > {self.score_thr:g}, "
                f"IoU > {self.iou_thr:g}{nms}{labels}{xy})")


class WideHead(MultiHead):
    """A MultiHead of up to 65536 boxes (YOLOv3 at 608 x 608 has 22,743, at 1024 x 1024 64,512) for
    the grid-wide decode (dnn_yolo_postprocess_wide, csrc/postprocess_wide.hip): the boxes are
    decoded one thread each over the whole GPU, then one workgroup per image sorts the candidates
    and runs the NMS.  Same constructor, classmethods, modes, rows and codes as MultiHead; an image
    may have at most 16384 candidates in every mode (else its code is -3), which is also the most
    rows (`max_det`).  detect_batch_multi and MultiDetectionBuffers take either class."""

    MAX_BOXES = WIDE_MAX_BOXES
    BOXES_ENTRY = "dnn_yolo_wide_boxes"

    def _entry(self, form):
        if form == "workspace":
            return "dnn_yolo_wide_workspace", ()
        return ("dnn_yolo_postprocess_wide" + ("" if self.xy is None else "_xy") + ("_host" if form == "host" else ""),
                (NMS_MODES[self.nms], LABEL_MODES[self.labels]))


def detect_batch_multi(preds, head, max_det=None, raise_errors=True):
    """preds: one fp32 host array per scale of `head` (a MultiHead), [B, *head.pred_shapes[s]] ->
    per image the rows detect_batch returns, from one sort and one NMS over all scales (the NMS
    rule is head.nms, the labels of a box head.labels; max_det defaults to head.max_det)."""
    if len(preds) != len(head.scales):
        raise ValueError(f"{len(preds)} prediction tensors for {len(head.scales)} scales")
    ps = [np.ascontiguousarray(p, dtype=np.float32) for p in preds]
    if any(p.size % f for p, f in zip(ps, head.pred_floats)):
        raise ValueError(f"predictions of shapes {[p.shape for p in ps]} are not [B, ...] of {head.pred_shapes}")
    ns = {p.size // f for p, f in zip(ps, head.pred_floats)}
    if len(ns) != 1:
        raise ValueError(f"the scales hold different numbers of images: {sorted(ns)}")
    n = ns.pop()
    max_det = head.max_det if max_det is None else max_det
    dets = np.zeros((n, max_det), DETECTION_DTYPE)
    counts = np.zeros(n, np.int32)
    ptrs = (ctypes.c_void_p * len(ps))(*[p.ctypes.data for p in ps])
    head._call("host", (ptrs, n, dets.ctypes.data, max_det, counts.ctypes.data))
    return _rows(dets, counts, max_det, raise_errors)


def _rows(dets, counts, max_det, raise_errors=True):
    out = []
    for i, n in enumerate(counts):
        if n < 0:
            if not raise_errors:
                out.append(int(n))
                continue
            raise dnn_hip.DnnHipError(f"image {i}: " + ERRORS.get(int(n), f"error {n}"))
        if n > max_det:
            raise dnn_hip.DnnHipError(f"image {i}: {n} detections > max_det {max_det}")
        out.append([(int(d["cls"]), int(d["left"]), int(d["top"]), int(d["right"]), int(d["bottom"]),
                     float(d["score"])) for d in dets[i, :n]])
    return out


def detect_batch(predictions, max_det=None, raise_errors=True, head=None):
    """[B,13,13,125] (or [13,13,125]) fp32 host predictions -> per image a list of
    (class, left, top, right, bottom, score) in the reference's output order.  An image on
    which the reference raises raises DnnHipError, or with raise_errors=False yields its
    negative error code (ERRORS) in place of the list.  With `head` (a YoloHead) the
    predictions are [B, *head.pred_shape] and max_det defaults to head.boxes."""
    p = np.ascontiguousarray(predictions, dtype=np.float32)
    if head is not None:
        if p.size % head.pred_floats:
            raise ValueError(f"predictions of shape {p.shape} are not [B,{','.join(map(str, head.pred_shape))}]")
        n = p.size // head.pred_floats
        max_det = head.boxes if max_det is None else max_det
        dets = np.zeros((n, max_det), DETECTION_DTYPE)
        counts = np.zeros(n, np.int32)
        dnn_hip._check(_lib.dnn_yolo_postprocess_head_host(ctypes.byref(head.c), p.ctypes.data, n, dets.ctypes.data,
                                                           max_det, counts.ctypes.data),
                       "dnn_yolo_postprocess_head_host")
        return _rows(dets, counts, max_det, raise_errors)
    max_det = N_BOXES if max_det is None else max_det
    if p.size % PRED_FLOATS:
        raise ValueError(f"predictions of shape {p.shape} are not [B,13,13,125]")
    n = p.size // PRED_FLOATS
    dets = np.zeros((n, max_det), DETECTION_DTYPE)
    counts = np.zeros(n, np.int32)
    dnn_hip._check(_lib.dnn_yolo_postprocess_host(p.ctypes.data, n, dets.ctypes.data, max_det,
                                                  counts.ctypes.data), "dnn_yolo_postprocess_host")
    return _rows(dets, counts, max_det, raise_errors)


def correct_rows_host(dets, counts, sizes, net_hw):
    """dnn_yolo_correct_detections_host: `dets` a writable DETECTION_DTYPE array [n, max_det] and
    `counts` int32 [n] as the decode entries fill them (host); rows [0, min(counts[i], max_det))
    of image i are rewritten in place from net_hw network pixels into the pixels of the
    sizes[i] = (h, w) image that was letterboxed.  Returns dets."""
    if not isinstance(dets, np.ndarray) or dets.dtype != DETECTION_DTYPE or dets.ndim != 2 or \
            not dets.flags.c_contiguous or not dets.flags.writeable:
        raise ValueError("dets: a writable C-contiguous [n, max_det] array of DETECTION_DTYPE expected")
    c = np.ascontiguousarray(counts, dtype=np.int32)
    n, max_det = dets.shape
    if c.shape != (n,) or len(sizes) != n:
        raise ValueError(f"{c.shape[0] if c.ndim == 1 else c.shape} counts and {len(sizes)} sizes for {n} images")
    dnn_hip._check(_lib.dnn_yolo_correct_detections_host(dets.ctypes.data, c.ctypes.data, n, max_det, _sizes(sizes),
                                                         int(net_hw[0]), int(net_hw[1])),
                   "dnn_yolo_correct_detections_host")
    return dets


def label_boxes(rows, head=None):
    """(class, l, t, r, b, score) rows -> the reference's label_boxes tuples.  A head with
    other classes than the 20 VOC names gives its own name (the class index where it has only
    a count) and None as the colour: the reference's colours belong to the VOC list."""
    if head is None or head.names == CLASSES:
        return [(CLASSES[c], (l, t), (r, b), COLORS[c]) for c, l, t, r, b, _ in rows]
    return [(head.names[c] if head.names else c, (l, t), (r, b), None) for c, l, t, r, b, _ in rows]


def postprocessing(predictions, head=None):
    """yolov2tiny.py:94-176: one image's [1,13,13,125] output -> [(class name, (left, top),
    (right, bottom), color)] after the 0.3 threshold and greedy NMS.  With `head`, one image of
    head.pred_shape and that head's thresholds."""
    p = np.asarray(predictions, dtype=np.float32)
    if head is not None:
        if p.size != head.pred_floats:
            raise ValueError(f"postprocessing expects one {'x'.join(map(str, head.pred_shape))} prediction, "
                             f"got shape {p.shape}")
        return label_boxes(detect_batch(p, head=head)[0], head)
    if p.size != PRED_FLOATS:
        raise ValueError(f"postprocessing expects one 13x13x125 prediction, got shape {p.shape}")
    return label_boxes(detect_batch(p)[0])


class DetectionBuffers(object):
    """Device-side outputs for `n` images (torch tensors on `device`): dets [n, max_det, 40 B]
    as uint8 and counts [n] int32, filled by `run(pred_ptr, n, stream)` asynchronously;
    `pack(n, stream)` then compacts them image-major into packed [n * max_det, 40] with the
    row count in total[0] (dnn_yolo_pack_detections), ready for dist.gather_detections.
    With `head` (a YoloHead) `run` goes through dnn_yolo_postprocess_head, max_det defaults to
    head.boxes and the buffers also own the workspace that entry needs."""

    def __init__(self, n, device, max_det=None, head=None):
        import torch
        if max_det is None:
            max_det = N_BOXES if head is None else head.boxes
        self.n, self.max_det, self.head = n, max_det, head
        if head is not None:
            self.workspace = torch.zeros(head.workspace_bytes(n), dtype=torch.uint8, device=device)
        self.dets = torch.zeros((n, max_det, DETECTION_DTYPE.itemsize), dtype=torch.uint8, device=device)
        self.counts = torch.zeros(n, dtype=torch.int32, device=device)
        self.packed = torch.zeros((n * max_det, DETECTION_DTYPE.itemsize), dtype=torch.uint8, device=device)
        self.total = torch.zeros(1, dtype=torch.int32, device=device)

    def run(self, pred_ptr, n, stream):
        if self.head is not None:
            if n > self.n:
                raise ValueError(f"{n} images > the {self.n} these buffers were sized for")
            dnn_hip._check(_lib.dnn_yolo_postprocess_head(
                ctypes.byref(self.head.c), pred_ptr, n, self.dets.data_ptr(), self.max_det, self.counts.data_ptr(),
                self.workspace.data_ptr(), self.workspace.numel(), stream), "dnn_yolo_postprocess_head")
            return
        dnn_hip._check(_lib.dnn_yolo_postprocess(pred_ptr, n, self.dets.data_ptr(), self.max_det,
                                                 self.counts.data_ptr(), stream), "dnn_yolo_postprocess")

    def pack(self, n, stream):
        dnn_hip._check(_lib.dnn_yolo_pack_detections(self.dets.data_ptr(), self.counts.data_ptr(), n, self.max_det,
                                                     self.packed.data_ptr(), self.total.data_ptr(), stream),
                       "dnn_yolo_pack_detections")
        return self.packed, self.total, self.counts

    def correct(self, sizes, net_hw, n, stream):
        """After `run` on letterboxed inputs (ingest.RaggedIngest) and before `pack`: rewrite the
        rows of images 0..n-1 in place from net_hw network pixels into each image's own pixels,
        sizes[i] = (h, w) of image i (dnn_yolo_correct_detections; asynchronous on `stream`)."""
        if n > self.n or len(sizes) != n:
            raise ValueError(f"{len(sizes)} sizes for {n} images in buffers sized for {self.n}")
        dnn_hip._check(_lib.dnn_yolo_correct_detections(self.dets.data_ptr(), self.counts.data_ptr(), n, self.max_det,
                                                        _sizes(sizes), int(net_hw[0]), int(net_hw[1]), stream),
                       "dnn_yolo_correct_detections")

    @staticmethod
    def to_rows(dets_u8, counts, max_det=None, raise_errors=True, head=None):
        """Host copies (numpy uint8 [n, max_det, 40], int32 [n]) -> per-image rows; max_det
        defaults to head.boxes when a head is given."""
        if max_det is None:
            max_det = N_BOXES if head is None else head.boxes
        d = np.ascontiguousarray(dets_u8).view(DETECTION_DTYPE).reshape(len(counts), max_det)
        return _rows(d, np.asarray(counts), max_det, raise_errors)


class MultiDetectionBuffers(DetectionBuffers):
    """DetectionBuffers for a MultiHead: `run(pred_ptrs, n, stream)` takes one device pointer per
    scale and goes through dnn_yolo_postprocess_multi_nms with head.nms, or with head.labels
    "multi" through dnn_yolo_postprocess_multi_labels, or for a WideHead through
    dnn_yolo_postprocess_wide, and for a head with scale_x_y through the _xy entry of its kind;
    dets, counts, `pack` and `to_rows` are the
    base class's (max_det defaults to head.max_det: head.boxes, or with "multi" the most
    candidates an image can have), so dnn_yolo_pack_detections and dist.gather_detections apply
    unchanged."""

    def __init__(self, n, device, head, max_det=None):
        import torch
        max_det = head.max_det if max_det is None else max_det
        self.n, self.max_det, self.head = n, max_det, head
        self.workspace = torch.zeros(head.workspace_bytes(n), dtype=torch.uint8, device=device)
        self.dets = torch.zeros((n, max_det, DETECTION_DTYPE.itemsize), dtype=torch.uint8, device=device)
        self.counts = torch.zeros(n, dtype=torch.int32, device=device)
        self.packed = torch.zeros((n * max_det, DETECTION_DTYPE.itemsize), dtype=torch.uint8, device=device)
        self.total = torch.zeros(1, dtype=torch.int32, device=device)

    def run(self, pred_ptrs, n, stream):
        if n > self.n:
            raise ValueError(f"{n} images > the {self.n} these buffers were sized for")
        if len(pred_ptrs) != len(self.head.scales):
            raise ValueError(f"{len(pred_ptrs)} prediction pointers for {len(self.head.scales)} scales")
        ptrs = (ctypes.c_void_p * len(pred_ptrs))(*[int(p) for p in pred_ptrs])
        self.head._call("device", (ptrs, n, self.dets.data_ptr(), self.max_det, self.counts.data_ptr(),
                                   self.workspace.data_ptr(), self.workspace.numel()), (stream,))
