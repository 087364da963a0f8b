/* dnn_hip_post.h — on-GPU YOLOv2 postprocessing (decode, score threshold, sort, greedy NMS)
 * exported by both libdnn_hip.so and libdnn_hip_avx.so.
 *
 * Replaces the host-side `postprocessing(predictions)` of the reference
 * (cs492-projects/proj3/yolov2tiny.py:94-234, with iou :179-195 and
 * non_maximal_suppression :197-226), which runs after DnnInferenceEngine.run() on the
 * [1,13,13,125] output.  The Python mirror keeps that name and return value
 * (dnn-inference-engine_amd/yolo_post.py); this C-ABI is what it binds, and what a
 * multi-GPU caller uses to gather detections instead of whole output tensors.
 *
 * Semantics (oracle/post_numpy.py restates them; tests/golden/post_golden.json pins them):
 * per image, all 13*13*5 boxes decoded in (row, col, anchor) order in fp32, kept when
 * conf * p(best class) > 0.3f, sorted by score descending (ties: lower box index first,
 * = Python's stable sort), then greedy NMS at IoU > 0.3 against every kept box.  Corners are
 * the truncated int() of fp32 values; IoU uses exact integer areas (+1 widths, no clamp).
 *
 * Error channel: int return (0 ok, < 0 error, message from dnn_last_error()).
 * Per image, counts[i] = number of detections (only the first max_det are written), or
 *   -1 when a box corner is not finite or beyond +-2^61 (the reference's int() raises), or
 *   -2 when an evaluated IoU has a zero denominator (the reference raises ZeroDivisionError;
 *      possible because its overlaps are not clamped).
 */
#ifndef DNN_HIP_POST_H
#define DNN_HIP_POST_H

#ifdef __cplusplus
extern "C" {
#endif

#pragma GCC visibility push(default)

/* one detection, 40 bytes: class index into the 20 VOC names, fp32 score, corners */
typedef struct dnn_detection {
  int cls;
  float score;
  long long left, top, right, bottom;
} dnn_detection;

#define DNN_YOLO_BOXES 845 /* 13 * 13 * 5: no image can have more detections */

/* Device pointers, asynchronous on `stream` (hipStream_t, NULL = default stream).
 * pred: [n_images][13][13][125] fp32; dets: [n_images][max_det]; counts: [n_images]. */
int dnn_yolo_postprocess(const float* pred, int n_images, dnn_detection* dets, int max_det, int* counts,
                         void* stream);

/* Device pointers, asynchronous: image-major compaction of the per-image lists written by
 * dnn_yolo_postprocess, packed = dets[0][:counts[0]] ++ dets[1][:counts[1]] ++ ... (images
 * with an error code contribute nothing; counts are clamped to max_det), total[0] = rows.
 * packed needs room for n_images * max_det rows.  Used before a multi-GPU gather so only
 * the detections travel. */
int dnn_yolo_pack_detections(const dnn_detection* dets, const int* counts, int n_images, int max_det,
                             dnn_detection* packed, int* total, void* stream);

/* Host pointers, synchronous (copies in, runs, copies out). */
int dnn_yolo_postprocess_host(const float* pred, int n_images, dnn_detection* dets, int max_det, int* counts);

/* ---- any YOLOv2 head: grid, anchors, classes -------------------------------------------
 * yolov2tiny.py:94-177 fixes n_grid_cells = 13, n_classes = 20, the anchor list (:115),
 * `* 32.0` (:132-136) and the two 0.3 thresholds (:154, :162) as named quantities; this
 * struct carries them, so one set of weights can be postprocessed at any input size that is
 * a multiple of 32.  Semantics are those above with 13 -> grid_h / grid_w, 5 -> n_anchors,
 * 20 -> n_classes, 32.0 -> cell; anchors and cell are fp32, the softmax sum keeps numpy's
 * float32 add.reduce order for the class count (sequential below 8, else 8 accumulators). */
#define DNN_YOLO_MAX_BOXES 8192 /* grid_h * grid_w * n_anchors: 1280-pixel inputs, 5 anchors */
#define DNN_YOLO_MAX_ANCHORS 16
#define DNN_YOLO_MAX_CLASSES 128 /* numpy's add.reduce is unblocked up to 128 elements */

typedef struct dnn_yolo_head {
  int grid_h, grid_w; /* cells (yolov2tiny.py:97 n_grid_cells, per axis) */
  int n_anchors;      /* 1..16  (yolov2tiny.py:98 n_b_boxes) */
  int n_classes;      /* 1..128 (yolov2tiny.py:96 n_classes) */
  float cell;         /* pixels per cell, 32 (yolov2tiny.py:132-136); > 0 */
  float score_thr;    /* 0.3f (yolov2tiny.py:154); >= 0 so candidate scores are positive */
  double iou_thr;     /* 0.3 (yolov2tiny.py:162, :218) */
  float anchors[32];  /* (w, h) per anchor, in cells (yolov2tiny.py:115) */
} dnn_yolo_head;

/* yolov2tiny.py:96-115: the reference's constants (5 VOC anchors, 20 classes, 32 pixels per
 * cell, both thresholds 0.3) at a grid_h x grid_w grid. */
int dnn_yolo_head_voc(int grid_h, int grid_w, dnn_yolo_head* head);

/* yolov2tiny.py:123-125 (the three nested loops): grid_h * grid_w * n_anchors, the most
 * detections an image can have, or < 0 (message in dnn_last_error()) for an invalid head. */
int dnn_yolo_head_boxes(const dnn_yolo_head* head);

/* Bytes of device scratch dnn_yolo_postprocess_head needs for n_images images of this head:
 * 40 bytes per decoded box (yolov2tiny.py:149-155: corners, score, class) when the boxes of
 * one image do not fit in LDS beside the sort keys, else 0. */
int dnn_yolo_head_workspace(const dnn_yolo_head* head, int n_images, unsigned long long* bytes);

/* yolov2tiny.py:94-227 for any head.  Device pointers, asynchronous on `stream`.
 * pred: [n_images][grid_h][grid_w][n_anchors * (5 + n_classes)] fp32; dets: [n_images][max_det];
 * counts: [n_images], with the meaning above; workspace: 8-byte aligned, at least
 * dnn_yolo_head_workspace() bytes (may be NULL when that is 0). */
int dnn_yolo_postprocess_head(const dnn_yolo_head* head, const float* pred, int n_images, dnn_detection* dets,
                              int max_det, int* counts, void* workspace, unsigned long long workspace_bytes,
                              void* stream);

/* yolov2tiny.py:94-227 for any head.  Host pointers, synchronous (allocates its scratch,
 * copies in, runs, copies out). */
int dnn_yolo_postprocess_head_host(const dnn_yolo_head* head, const float* pred, int n_images, dnn_detection* dets,
                                   int max_det, int* counts);

/* ---- several heads, one NMS: YOLOv3's three scales --------------------------------------
 * The reference has one head.  YOLOv3 predicts at strides 32, 16 and 8, each with its own grid,
 * cell size and anchors, and logistic class scores; all boxes of an image then compete in one
 * sort and one NMS.  A dnn_yolo_multi lists the heads ("scales").
 *
 * Box order: the image's boxes are the scales' boxes concatenated, scale 0 first, each scale in
 * (row, col, anchor) order; the global box index is the position in that list.  Geometry and
 * objectness of a box are the single-head rules above with its scale's grid, cell and anchors
 * (anchors in cells: YOLOv3's pixel anchors divided by the stride, exact in fp32).  Class
 * scores: class_mode 0 is the single-head softmax; class_mode 1 gives every class
 * p[c] = 1 / (1 + e ** -logit[c]) in fp32 (the objectness formula), the class is the first index
 * of the largest computed p (the rounded values are compared, not the logits) and the score is
 * conf * p[class], one fp32 multiply.  Candidates (score > score_thr) of all scales go through
 * one sort (score descending, ties: lower global index) and one greedy NMS with the integer-area
 * IoU, as above.
 *
 * NMS rule (nms_mode of the *_nms entries; the entries without it use DNN_YOLO_NMS_ANY_CLASS):
 *   DNN_YOLO_NMS_ANY_CLASS  the reference's: a candidate is kept unless an earlier kept box of ANY
 *     class has IoU > iou_thr with it.  A person box suppresses the bicycle box it overlaps.
 *   DNN_YOLO_NMS_PER_CLASS  Darknet's do_nms_sort / torchvision's batched_nms rule: candidates are
 *     visited in the same order, and a candidate is kept unless an earlier kept box OF ITS OWN
 *     CLASS has IoU > iou_thr with it.  The evaluated IoUs are those of a candidate against every
 *     kept box of its class (all of them, no early exit), so an image can carry -2 under one rule
 *     and be clean under the other, in either direction.  The rows are the kept boxes in the
 *     global sorted order (score descending, ties: lower global index), which is not class-major.
 *     With n_classes == 1 the two rules are the same function.
 *   In these entries a box has ONE class, the arg-max.
 *
 * Labels (labels_mode of the *_labels entries, whose NMS rule is DNN_YOLO_NMS_PER_CLASS; defined for
 * class_mode 0 and 1):
 *   DNN_YOLO_LABELS_ARGMAX  one class per box, as above.
 *   DNN_YOLO_LABELS_MULTI   Darknet's multi-label output: every class c of a box has the score
 *     s[c] = conf * p[c], one fp32 multiply, with p[c] the per-class value above (the sigmoid of
 *     logit[c], or the softmax quotient with its sum order), and (box, c) is a candidate iff
 *     s[c] > score_thr.  Darknet's extra gate objectness > thresh is implied: p[c] <= 1 and fp32
 *     multiplication is monotone, so s[c] <= conf.  Boxes, conf and the global box index are those
 *     above.  Candidates are ordered by (score descending, global box index ascending, class
 *     ascending) and go through the per-class NMS: a candidate is kept unless an earlier kept
 *     candidate of its own class has IoU > iou_thr with it, every kept box of that class evaluated.
 *     The rows are the kept candidates in that order: cls the candidate's class, score its s[c], the
 *     corners the box's.  One box gives up to n_classes rows, so an image can have more rows than
 *     boxes, but at most DNN_YOLO_MULTI_MAX_CANDIDATES candidates (their sort keys live in LDS):
 *     an image with more gets counts[i] = -3 and no rows.  With n_classes == 1 the two label modes
 *     are the same function.
 * counts[i]: as above, -1 when any box of any scale (candidate or not) has a corner that is not
 * finite or out of range, else -3 when the image has too many multi-label candidates (no NMS runs),
 * else -2 when an evaluated IoU denominator is zero; such an image does not touch the other images'
 * results.
 *
 * Every scale must be a valid dnn_yolo_head, except that its own boxes may exceed
 * DNN_YOLO_MAX_BOXES: only the sum over scales is bounded, by DNN_YOLO_MULTI_MAX_BOXES.  All
 * scales must agree on n_classes, score_thr and iou_thr. */
#define DNN_YOLO_MAX_SCALES 4
#define DNN_YOLO_MULTI_MAX_BOXES 16384 /* 416 x 416 YOLOv3: 10,647; 512 x 512: 16,128 */

typedef struct dnn_yolo_multi {
  int n_scales;   /* 1..4 */
  int class_mode; /* 0 softmax (YOLOv2), 1 logistic (YOLOv3) */
  dnn_yolo_head scale[DNN_YOLO_MAX_SCALES];
} dnn_yolo_multi;

/* Boxes of one image, summed over the scales, or < 0 (message in dnn_last_error()) for an
 * invalid description.  Host only: no device is touched. */
int dnn_yolo_multi_boxes(const dnn_yolo_multi* multi);

/* Bytes of device scratch dnn_yolo_postprocess_multi needs for n_images images: 40 bytes per
 * decoded box (the sort keys fill the LDS, so the box store is always here). */
int dnn_yolo_multi_workspace(const dnn_yolo_multi* multi, int n_images, unsigned long long* bytes);

/* Device pointers, asynchronous on `stream`.  pred: a HOST array of n_scales device pointers,
 * pred[s] = [n_images][grid_h][grid_w][n_anchors * (5 + n_classes)] fp32 of scale s;
 * dets: [n_images][max_det]; counts: [n_images]; workspace: 8-byte aligned, at least
 * dnn_yolo_multi_workspace() bytes.  dets / counts have the layout of the single-head entries,
 * so dnn_yolo_pack_detections applies unchanged. */
int dnn_yolo_postprocess_multi(const dnn_yolo_multi* multi, const float* const* pred, int n_images,
                               dnn_detection* dets, int max_det, int* counts, void* workspace,
                               unsigned long long workspace_bytes, void* stream);

/* Host pointers (pred: n_scales host tensors), synchronous: allocates its scratch, copies in,
 * runs, copies out. */
int dnn_yolo_postprocess_multi_host(const dnn_yolo_multi* multi, const float* const* pred, int n_images,
                                    dnn_detection* dets, int max_det, int* counts);

/* The same three entries with the NMS rule as an argument (see "NMS rule" above).  nms_mode 0 goes
 * through dnn_yolo_postprocess_multi's launcher: the same dets, counts and workspace contents, byte
 * for byte, and the same workspace size.  Any other value than these two returns -2 ("nms_mode" in
 * dnn_last_error()) before anything is launched; all other checks are those of the entries above.
 * Both rules need the same workspace, 40 bytes per box. */
#define DNN_YOLO_NMS_ANY_CLASS 0 /* the reference's */
#define DNN_YOLO_NMS_PER_CLASS 1

int dnn_yolo_multi_nms_workspace(const dnn_yolo_multi* multi, int n_images, int nms_mode, unsigned long long* bytes);

int dnn_yolo_postprocess_multi_nms(const dnn_yolo_multi* multi, const float* const* pred, int n_images,
                                   dnn_detection* dets, int max_det, int* counts, void* workspace,
                                   unsigned long long workspace_bytes, int nms_mode, void* stream);

int dnn_yolo_postprocess_multi_nms_host(const dnn_yolo_multi* multi, const float* const* pred, int n_images,
                                        dnn_detection* dets, int max_det, int* counts, int nms_mode);

/* The same three entries for the per-class NMS rule with the label mode as an argument (see
 * "Labels" above).  labels_mode 0 goes through the *_nms launcher with DNN_YOLO_NMS_PER_CLASS: the
 * same dets, counts and workspace contents, byte for byte, and the same workspace size.  Any other
 * value than these two returns -2 ("labels_mode" in dnn_last_error()) before anything is launched;
 * all other checks are those of the entries above.  Both modes need the same workspace, 40 bytes
 * per box; a multi-label image can have up to min(boxes * n_classes,
 * DNN_YOLO_MULTI_MAX_CANDIDATES) rows, which is what max_det should allow for. */
#define DNN_YOLO_LABELS_ARGMAX 0
#define DNN_YOLO_LABELS_MULTI 1
#define DNN_YOLO_MULTI_MAX_CANDIDATES 16384 /* (box, class) pairs above the threshold, per image */

int dnn_yolo_multi_labels_workspace(const dnn_yolo_multi* multi, int n_images, int labels_mode,
                                    unsigned long long* bytes);

int dnn_yolo_postprocess_multi_labels(const dnn_yolo_multi* multi, const float* const* pred, int n_images,
                                      dnn_detection* dets, int max_det, int* counts, void* workspace,
                                      unsigned long long workspace_bytes, int labels_mode, void* stream);

int dnn_yolo_postprocess_multi_labels_host(const dnn_yolo_multi* multi, const float* const* pred, int n_images,
                                           dnn_detection* dets, int max_det, int* counts, int labels_mode);

/* ---- heads above DNN_YOLO_MULTI_MAX_BOXES: grid-wide decode, one NMS workgroup per image ----
 * The entries above decode an image in ONE workgroup and keep a sort key per box in LDS, which is
 * where their 16,384-box limit comes from; a stock 608 x 608 YOLOv3 has 22,743 boxes.  Only
 * candidates are sorted, so these entries bound the two counts separately: up to
 * DNN_YOLO_WIDE_MAX_BOXES boxes per image (YOLOv3 at 1024 x 1024: 64,512), decoded one thread per
 * box over the whole grid, and up to DNN_YOLO_MULTI_MAX_CANDIDATES candidates per image IN EVERY
 * MODE (for multi-label the (box, class) pairs, else the boxes above the threshold): an image with
 * more gets counts[i] = -3 and no rows, after -1 and before -2 as above.  Everything else is the
 * semantics above, bit for bit: the same boxes, scores, order, rows and codes as the *_multi
 * entries give for a head both accept.  A call clears the per-image counters, then runs the
 * decode kernel and the NMS kernel, three launches in that order on `stream`; it may be captured
 * in a HIP graph.
 *
 * nms_mode / labels_mode: (ANY_CLASS, ARGMAX), (PER_CLASS, ARGMAX) or (PER_CLASS, MULTI);
 * (ANY_CLASS, MULTI) returns -2 (a box's second label would always be suppressed by its first).
 * With n_classes == 1 all three are the same function.
 * Workspace: per image 40 bytes per box, DNN_YOLO_MULTI_MAX_CANDIDATES 8-byte keys and one
 * 64-byte counter block; 8-byte aligned.  All other arguments and checks are those of
 * dnn_yolo_postprocess_multi_labels. */
#define DNN_YOLO_WIDE_MAX_BOXES 65536

/* As dnn_yolo_multi_boxes with the sum bounded by DNN_YOLO_WIDE_MAX_BOXES. */
int dnn_yolo_wide_boxes(const dnn_yolo_multi* multi);

int dnn_yolo_wide_workspace(const dnn_yolo_multi* multi, int n_images, unsigned long long* bytes);

int dnn_yolo_postprocess_wide(const dnn_yolo_multi* multi, const float* const* pred, int n_images,
                              dnn_detection* dets, int max_det, int* counts, void* workspace,
                              unsigned long long workspace_bytes, int nms_mode, int labels_mode, void* stream);

int dnn_yolo_postprocess_wide_host(const dnn_yolo_multi* multi, const float* const* pred, int n_images,
                                   dnn_detection* dets, int max_det, int* counts, int nms_mode, int labels_mode);

/* ---- scale_x_y: Darknet's stretch of the box centre (YOLOv4, YOLOv4-tiny) ---------------
 * Darknet's [yolo] key scale_x_y = s replaces the logistic of tx and ty (forward_yolo_layer,
 * scal_add_cpu) by
 *   sig * s + b,   b = -0.5f * (s - 1.0f)
 * so that a centre can reach its cell's border: b is computed on the host in fp32 once per scale,
 * and the device does one fp32 multiply then one fp32 add, never contracted, in place of
 * sigmoid(tx) and sigmoid(ty).  Width, height, objectness and the class scores do not change.
 *
 * scale_x_y: a HOST array of multi->n_scales floats, read before the call returns; NULL means all
 * 1.  Each value must be finite and > 0: otherwise the call returns -2 before any launch, like an
 * invalid description, and dnn_last_error() names scale_x_y.  dnn_yolo_multi and dnn_yolo_head
 * keep their layouts.  With s == 1, b is -0.0f and sig * 1.0f + -0.0f is sig bit for bit for every
 * non-NaN sig: the entries above run the same kernels with that pair, and with every scale at 1
 * (or NULL) an _xy entry gives their dets, counts and workspace byte for byte.
 *
 * nms_mode / labels_mode are the wide entry's pairs, for the _multi_xy entries too, each run by
 * the kernel of the entry named:
 *   (ANY_CLASS, ARGMAX)  dnn_yolo_postprocess_multi          / _wide in that mode
 *   (PER_CLASS, ARGMAX)  dnn_yolo_postprocess_multi_nms      / _wide in that mode
 *   (PER_CLASS, MULTI)   dnn_yolo_postprocess_multi_labels   / _wide in that mode
 *   (ANY_CLASS, MULTI)   none: returns -2
 * Limits, workspaces (dnn_yolo_multi_workspace and its _nms / _labels twins, all the same size;
 * dnn_yolo_wide_workspace), codes and every other argument are those of the entries above. */
int dnn_yolo_postprocess_multi_xy(const dnn_yolo_multi* multi, const float* scale_x_y, const float* const* pred,
                                  int n_images, dnn_detection* dets, int max_det, int* counts, void* workspace,
                                  unsigned long long workspace_bytes, int nms_mode, int labels_mode, void* stream);

int dnn_yolo_postprocess_multi_xy_host(const dnn_yolo_multi* multi, const float* scale_x_y,
                                       const float* const* pred, int n_images, dnn_detection* dets, int max_det,
                                       int* counts, int nms_mode, int labels_mode);

int dnn_yolo_postprocess_wide_xy(const dnn_yolo_multi* multi, const float* scale_x_y, const float* const* pred,
                                 int n_images, dnn_detection* dets, int max_det, int* counts, void* workspace,
                                 unsigned long long workspace_bytes, int nms_mode, int labels_mode, void* stream);

int dnn_yolo_postprocess_wide_xy_host(const dnn_yolo_multi* multi, const float* scale_x_y,
                                      const float* const* pred, int n_images, dnn_detection* dets, int max_det,
                                      int* counts, int nms_mode, int labels_mode);

/* ---- boxes back to each image's own pixels ----------------------------------------------
 * The reference's frames are stretched to the network's size and its boxes stay in network
 * pixels.  After a letterbox ingest (include/dnn_hip_ingest.h: dnn_letterbox_frames) image i of
 * size sizes[i] occupies [pad_y, pad_y + new_h) x [pad_x, pad_x + new_w) of the network input
 * (dnn_letterbox_geometry), and Darknet's correct_yolo_boxes / draw_detections map a box back
 * and clamp it to the image.  Restated on the integer corners, integer arithmetic only:
 *   xc = min(max(x, pad_x), pad_x + new_w);  x' = min(((xc - pad_x) * src_w) / new_w, src_w - 1)
 *   yc = min(max(y, pad_y), pad_y + new_h);  y' = min(((yc - pad_y) * src_h) / new_h, src_h - 1)
 * for left / right and top / bottom (clamping first bounds the product whatever the corner
 * held).  Rows [0, min(counts[i], max_det)) of image i are rewritten in place, class and score
 * untouched; an image with a negative count (an error code) and the rows past the count are left
 * alone; a box wholly in the padding becomes a zero-width row and stays.  Darknet maps before
 * its NMS, this runs after the decode's NMS on network pixels.
 * sizes: a HOST array of n_images sizes, fully read before the call returns; dets / counts:
 * device, the layout of every decode entry above.  Bad arguments (NULL pointers, negative
 * counts of images or rows, a non-positive size, a letterbox with a side below 2 pixels: the
 * message names the image) return nonzero before any device call.  Asynchronous on `stream`. */
typedef struct dnn_image_size {
  int h, w;
} dnn_image_size;

int dnn_yolo_correct_detections(dnn_detection* dets, const int* counts, int n_images, int max_det,
                                const dnn_image_size* sizes, int net_h, int net_w, void* stream);

/* Host pointers, synchronous (copies in, runs, copies out). */
int dnn_yolo_correct_detections_host(dnn_detection* dets, const int* counts, int n_images, int max_det,
                                     const dnn_image_size* sizes, int net_h, int net_w);

#pragma GCC visibility pop

#ifdef __cplusplus
}
#endif

#endif /* DNN_HIP_POST_H */
