// YOLOv2 postprocessing for any head (include/dnn_hip_post.h: dnn_yolo_head): the reference's
// decode + threshold + sort + greedy NMS (cs492-projects/proj3/yolov2tiny.py:94-227) with its
// named constants (13 cells, 5 anchors, 20 classes, 32 pixels per cell, the two 0.3
// thresholds) as parameters, one workgroup per image, up to DNN_YOLO_MAX_BOXES boxes.  The kernel
// is a sequence of calls into post_dev.h, the helpers that the multi-scale decodes call too:
//
//   phase 1  thread per box: decode_corners and class_argmax, the fp32 decode of postprocess.hip
//            (post_math.h) with the class vector read from memory in three passes (max,
//            numpy-order sum of exp, first index of the largest quotient) instead of a register
//            array: 128 classes do not fit in registers.  Every box's corners, score and class go
//            to the box store: LDS when an image's boxes fit beside the keys (<= PH_LDS_BOXES),
//            else the caller's workspace (box_store: 40 bytes per box, read back through L2).
//            Candidates append a sort key (key_any).
//   phases 2, 3 and the emit  nms_any_emit: the bitonic sort of the keys (score descending, then
//            box index: the append order of phase 1 does not matter), the blocked greedy NMS in
//            O(boxes) memory with the kept list in place over the consumed keys, the rows.
#include "post_dev.h"

namespace dnnhip {

constexpr int PH_THREADS = 512;
constexpr int PH_LDS_BOXES = 2048;  // 16 K keys + 80 K boxes = 96 KiB of LDS

// CAP: capacity of the key array (>= boxes, power of two).  WS: the box store is the workspace
// (true) or LDS (false, boxes <= CAP).
template <int CAP, bool WS>
__global__ void __launch_bounds__(PH_THREADS)
yolo_head_kernel(const dnn_yolo_head head, const float* __restrict__ pred, dnn_detection* __restrict__ dets,
                 int max_det, int* __restrict__ counts, char* workspace) {
  __shared__ unsigned long long keys[CAP];
  __shared__ long long lds_box[WS ? 1 : CAP][4];
  __shared__ float lds_score[WS ? 1 : CAP];
  __shared__ int lds_cls[WS ? 1 : CAP];
  __shared__ float anchors[2 * DNN_YOLO_MAX_ANCHORS];
  __shared__ NmsState st;
  __shared__ int n_cand, bad;

  const int img = blockIdx.x, tid = threadIdx.x;
  const int A = head.n_anchors, C = head.n_classes, gw = head.grid_w;
  const int nb = head.grid_h * gw * A, stride = 5 + C;
  const float cell_px = head.cell, score_thr = head.score_thr;
  const float* p = pred + (size_t)img * nb * stride;
  const BoxStore bs = WS ? box_store(workspace + (size_t)img * nb * POST_BOX_BYTES, nb)
                         : BoxStore{lds_box, lds_score, lds_cls};

  int nsort = 1;  // keys that the sort can touch: pow2 >= nb, <= CAP
  while (nsort < nb) nsort <<= 1;
  if (tid == 0) {
    n_cand = 0;
    bad = 0;
  }
  reset_state(st, tid);
  if (tid < 2 * A) anchors[tid] = head.anchors[tid];
  for (int i = tid; i < nsort; i += PH_THREADS) keys[i] = ~0ull;
  __syncthreads();

  // ---- phase 1: decode (yolov2tiny.py:123-155); a bad corner sets the flag before the stores,
  // which come after the class loop (post_multi_dev.h: decode_corners_at has the reason)
  for (int k = tid; k < nb; k += PH_THREADS) {
    const float* q = p + (size_t)k * stride;
    const int b = k % A, cell = k / A, col = cell % gw, row = cell / gw;
    long long c4[4];
    float conf;
    int best;
    if (!decode_corners(q, b, col, row, anchors, cell_px, 1.0f, -0.0f, c4, &conf)) bad = 1;
    const float sc = conf * class_argmax(q + 5, C, false, &best);
    bs.box[k][0] = c4[0];
    bs.box[k][1] = c4[1];
    bs.box[k][2] = c4[2];
    bs.box[k][3] = c4[3];
    bs.score[k] = sc;
    bs.cls[k] = best;
    if (sc > score_thr) {
      const int pos = atomicAdd(&n_cand, 1);
      keys[pos] = key_any(sc, k);
    }
  }
  __syncthreads();
  if (bad) {
    if (tid == 0) counts[img] = -1;
    return;
  }

  // ---- phases 2 and 3 (yolov2tiny.py:158, 200-227), the kept list in place over keys[0 .. base); emit
  nms_any_emit<PH_THREADS>(keys, n_cand, bs, head.iou_thr, st, dets + (size_t)img * max_det, max_det, &counts[img],
                           tid);
}

// < 0 with the error set, else grid_h * grid_w * n_anchors (at most max_boxes: postprocess_multi.hip has its own cap)
int yolo_head_boxes(const dnn_yolo_head* h, const char* who, long long max_boxes) {
  if (!h) {
    set_error("%s: NULL head", who);
    return -2;
  }
  if (h->grid_h < 1 || h->grid_w < 1 || h->grid_h > max_boxes || h->grid_w > max_boxes ||
      h->n_anchors < 1 || h->n_anchors > DNN_YOLO_MAX_ANCHORS || h->n_classes < 1 ||
      h->n_classes > DNN_YOLO_MAX_CLASSES) {
    set_error("%s: head %d x %d cells, %d anchors, %d classes: need >= 1 cell, 1..%d anchors, 1..%d classes", who,
              h->grid_h, h->grid_w, h->n_anchors, h->n_classes, DNN_YOLO_MAX_ANCHORS, DNN_YOLO_MAX_CLASSES);
    return -2;
  }
  const long long nb = (long long)h->grid_h * h->grid_w * h->n_anchors;
  if (nb > max_boxes) {
    set_error("%s: %d x %d cells x %d anchors = %lld boxes > %lld", who, h->grid_h, h->grid_w, h->n_anchors, nb,
              max_boxes);
    return -2;
  }
  if (!(h->score_thr >= 0.0f) || h->iou_thr != h->iou_thr || !(h->cell > 0.0f) || h->cell > 3.0e38f) {
    set_error("%s: need score_thr >= 0 (got %g), iou_thr not NaN (got %g), finite cell > 0 (got %g)", who,
              (double)h->score_thr, h->iou_thr, (double)h->cell);
    return -2;
  }
  for (int i = 0; i < 2 * h->n_anchors; ++i) {
    if (!(h->anchors[i] > -3.0e38f && h->anchors[i] < 3.0e38f)) {
      set_error("%s: anchor value %d is not finite", who, i);
      return -2;
    }
  }
  return (int)nb;
}

static int head_boxes(const dnn_yolo_head* h, const char* who) { return yolo_head_boxes(h, who, DNN_YOLO_MAX_BOXES); }

static unsigned long long head_workspace(int nb, int n_images) {
  return nb > PH_LDS_BOXES ? (unsigned long long)n_images * nb * POST_BOX_BYTES : 0ull;
}

int launch_yolo_head(const dnn_yolo_head* head, const float* pred, int n_images, dnn_detection* dets, int max_det,
                     int* counts, void* workspace, unsigned long long workspace_bytes, hipStream_t stream) {
  const char* who = "dnn_yolo_postprocess_head";
  const int nb = head_boxes(head, who);
  if (nb < 0) return nb;
  if (n_images < 0 || max_det < 0 || (n_images > 0 && (!pred || !counts || (max_det > 0 && !dets)))) {
    set_error("%s: bad arguments (n_images=%d max_det=%d)", who, n_images, max_det);
    return -2;
  }
  const unsigned long long need = head_workspace(nb, n_images);
  if (need && (!workspace || workspace_bytes < need || (reinterpret_cast<uintptr_t>(workspace) & 7u))) {
    set_error("%s: workspace %p of %llu bytes; %d images of %d boxes need %llu bytes, 8-byte aligned", who,
              workspace, workspace_bytes, n_images, nb, need);
    return -2;
  }
  if (n_images == 0) return 0;
  char* ws = static_cast<char*>(workspace);
  if (nb > PH_LDS_BOXES)
    hipLaunchKernelGGL((yolo_head_kernel<DNN_YOLO_MAX_BOXES, true>), dim3(n_images), dim3(PH_THREADS), 0, stream,
                       *head, pred, dets, max_det, counts, ws);
  else
    hipLaunchKernelGGL((yolo_head_kernel<PH_LDS_BOXES, false>), dim3(n_images), dim3(PH_THREADS), 0, stream, *head,
                       pred, dets, max_det, counts, ws);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("launch yolo_head: %s", hipGetErrorString(e));
    return -1;
  }
  return 0;
}

}  // namespace dnnhip

extern "C" {

int dnn_yolo_head_voc(int grid_h, int grid_w, dnn_yolo_head* head) {
  DNN_REQUIRE(head, "dnn_yolo_head_voc: NULL head");
  dnn_yolo_head h = {};
  h.grid_h = grid_h;
  h.grid_w = grid_w;
  h.n_anchors = 5;
  h.n_classes = 20;
  h.cell = 32.0f;
  h.score_thr = 0.3f;
  h.iou_thr = 0.3;
  for (int i = 0; i < 10; ++i) h.anchors[i] = dnnhip::VOC_ANCHORS[i];
  const int nb = dnnhip::head_boxes(&h, "dnn_yolo_head_voc");
  if (nb < 0) return nb;
  *head = h;
  return 0;
}

int dnn_yolo_head_boxes(const dnn_yolo_head* head) { return dnnhip::head_boxes(head, "dnn_yolo_head_boxes"); }

int dnn_yolo_head_workspace(const dnn_yolo_head* head, int n_images, unsigned long long* bytes) {
  const int nb = dnnhip::head_boxes(head, "dnn_yolo_head_workspace");
  if (nb < 0) return nb;
  DNN_REQUIRE(n_images >= 0 && bytes, "dnn_yolo_head_workspace: bad arguments (n_images=%d)", n_images);
  *bytes = dnnhip::head_workspace(nb, n_images);
  return 0;
}

int dnn_yolo_postprocess_head(const dnn_yolo_head* head, const float* pred, int n_images, dnn_detection* dets,
                              int max_det, int* counts, void* workspace, unsigned long long workspace_bytes,
                              void* stream) {
  return dnnhip::launch_yolo_head(head, pred, n_images, dets, max_det, counts, workspace, workspace_bytes,
                                  static_cast<hipStream_t>(stream));
}

int dnn_yolo_postprocess_head_host(const dnn_yolo_head* head, const float* pred, int n_images, dnn_detection* dets,
                                   int max_det, int* counts) {
  const int nb = dnnhip::head_boxes(head, "dnn_yolo_postprocess_head_host");
  if (nb < 0) return nb;
  DNN_REQUIRE(n_images >= 0 && max_det >= 0, "dnn_yolo_postprocess_head_host: bad arguments");
  if (n_images == 0) return 0;
  DNN_REQUIRE(pred && counts && (max_det == 0 || dets), "dnn_yolo_postprocess_head_host: NULL pointer");
  return dnnhip::yolo_single_host(
      {"dnn_yolo_postprocess_head_host", head, n_images, max_det, (size_t)dnnhip::head_workspace(nb, n_images)}, pred,
      (size_t)n_images * nb * (5 + head->n_classes) * sizeof(float), dets,
      (size_t)n_images * max_det * sizeof(dnn_detection), counts, (size_t)n_images * sizeof(int),
      [](const dnnhip::SingleCall& c, const float* d_pred, dnn_detection* d_dets, int* d_counts, void* ws) {
        return dnnhip::launch_yolo_head(c.head, d_pred, c.n_images, d_dets, c.max_det, d_counts, ws, c.ws_bytes,
                                        nullptr);
      });
}

}  // extern "C"
