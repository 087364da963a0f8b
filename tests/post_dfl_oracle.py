"""Float64 restatement of the DFL head decode (include/dnn_hip_post.h: dnn_yolo_dfl), plain loops; shares no
code with yolo_post.  A head is Dfl(scales, classes, reg_max, score_thr, iou_thr), scales (grid_h, grid_w,
stride); an image is one array [grid_h, grid_w, 4 * reg_max + classes] per scale.  Rows are (class, left,
top, right, bottom, score)."""
import collections
import math

Dfl = collections.namedtuple("Dfl", "scales classes reg_max score_thr iou_thr")
CAP = 16384  # DNN_YOLO_MULTI_MAX_CANDIDATES
LIMIT = 2.0 ** 61


def sigmoid(x):
    return 0.0 if x < -700.0 else 1.0 / (1.0 + math.exp(-x))


def distance(x):
    """sum_k softmax(x)[k] * k, ascending in k; NaN when a logit is NaN or +inf or all are -inf."""
    m = math.nan if any(math.isnan(v) for v in x) else max(x)
    if math.isnan(m) or math.isinf(m):
        return math.nan
    e = [math.exp(v - m) for v in x]
    total, d = 0.0, 0.0
    for v in e:
        total += v
    for k, v in enumerate(e):
        d += v / total * k
    return d


def points(head):
    """(scale, row, col) of every grid point in the global order."""
    return [(s, r, c) for s, (gh, gw, _) in enumerate(head.scales) for r in range(gh) for c in range(gw)]


def corners(image, head, point):
    """The four float64 corners of a point's box."""
    s, r, c = point
    q, st, n = image[s][r, c], head.scales[s][2], head.reg_max
    d = [distance([float(v) for v in q[i * n:(i + 1) * n]]) for i in range(4)]
    return ((c + 0.5 - d[0]) * st, (r + 0.5 - d[1]) * st, (c + 0.5 + d[2]) * st, (r + 0.5 + d[3]) * st)


def candidates(image, head, labels):
    """(score, point index, class) of every candidate, unordered."""
    out = []
    for k, (s, r, c) in enumerate(points(head)):
        p = [sigmoid(float(v)) for v in image[s][r, c, 4 * head.reg_max:]]
        if labels == "multi":
            out += [(v, k, cl) for cl, v in enumerate(p) if v > head.score_thr]
            continue
        best = 0  # class_argmax's loop: a NaN p[0] stays, a later NaN never wins
        for cl in range(1, len(p)):
            if p[cl] > p[best]:
                best = cl
        if p[best] > head.score_thr:
            out.append((p[best], k, best))
    return out


def iou(a, b):
    """Integer corners, inclusive + 1 widths, unclamped overlap; None for a zero denominator."""
    w, h = min(a[2], b[2]) - max(a[0], b[0]) + 1, min(a[3], b[3]) - max(a[1], b[1]) + 1
    den = (a[2] - a[0] + 1) * (a[3] - a[1] + 1) + (b[2] - b[0] + 1) * (b[3] - b[1] + 1) - w * h
    return None if den == 0 else w * h / float(den)


def detect_or_code(image, head, nms, labels, seen=None):
    """The rows of one image, or its code -1 / -3 / -2.  seen (a dict of lists) collects what the decisions were
    made on: the candidates' scores, their float corners and every evaluated IoU."""
    seen = {} if seen is None else seen
    cand = candidates(image, head, labels)
    pts, boxes = points(head), {}
    for _, k, _ in cand:
        if k not in boxes:
            f = corners(image, head, pts[k])
            if not all(-LIMIT < v < LIMIT for v in f):  # also NaN
                return -1
            seen.setdefault("corner", []).extend(f)
            boxes[k] = tuple(int(v) for v in f)  # truncation toward zero
    if len(cand) > CAP:
        return -3
    seen.setdefault("score", []).extend(v for v, _, _ in cand)
    cand.sort(key=lambda t: (-t[0], t[1], t[2]))
    kept = []
    for v, k, cl in cand:
        drop = False
        for _, kk, kc in kept:  # every kept box the rule names, no early exit
            if nms == "per_class" and kc != cl:
                continue
            q = iou(boxes[k], boxes[kk])
            if q is None:
                return -2
            seen.setdefault("iou", []).append(q)
            drop = drop or q > head.iou_thr
        if not drop:
            kept.append((v, k, cl))
    return [(cl,) + boxes[k] + (v,) for v, k, cl in kept]
