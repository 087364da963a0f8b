// YOLOv2 postprocessing for any head (include/dnn_hip_post.h: dnn_yolo_head): the reference's
// decode + threshold + sort + greedy NMS (cs492-projects/proj3/yolov2tiny.py:94-227) with its
// named constants (13 cells, 5 anchors, 20 classes, 32 pixels per cell, the two 0.3
// thresholds) as parameters, one workgroup per image, up to DNN_YOLO_MAX_BOXES boxes.
//
//   phase 1  thread per box: the fp32 decode of postprocess.hip (post_math.h), with the class
//            vector read from memory in three passes (max, numpy-order sum of exp, first index
//            of the largest quotient) instead of a register array: 128 classes do not fit in
//            registers.  Every box's corners, score and class go to the box store: LDS when an
//            image's boxes fit beside the keys (<= PH_LDS_BOXES), else the caller's workspace
//            (40 bytes per box, read back through L2).  Candidates append a sort key.
//   phase 2  bitonic sort of the keys (score descending, then box index: the append order of
//            phase 1 does not matter).
//   phase 3  greedy NMS in O(boxes) memory: candidates in sorted order, 64 at a time.  All
//            waves test the block (lane = candidate) against the boxes kept from earlier
//            blocks (wave w takes kept entries w, w + waves, ...) and ballot one word each;
//            then wave 0 resolves the 64 x 64 triangle inside the block in order and appends
//            the survivors to the kept list.  Two barriers per block.  A zero IoU denominator
//            counts for every pair (candidate, kept box before it), dropped candidates
//            included: the reference tests every candidate against the whole kept list
//            without early exit (yolov2tiny.py:210-225).
#include <hip/hip_runtime.h>
#include <cstdint>
#include "dnn_common.h"
#include "post_math.h"
#include "../../include/dnn_hip_post.h"

namespace dnnhip {

constexpr int PH_THREADS = 512;
constexpr int PH_WAVES = PH_THREADS / 64;
constexpr int PH_LDS_BOXES = 2048;  // 16 K keys + 8 K kept + 80 K boxes = 104 KiB of LDS
constexpr int PH_BOX_BYTES = 40;    // 4 x int64 corners + fp32 score + int class

// CAP: capacity of the key and kept arrays (>= boxes, power of two).  WS: the box store is the
// workspace (true) or LDS (false, boxes <= CAP).
template <int CAP, bool WS>
__global__ void __launch_bounds__(PH_THREADS)
yolo_head_kernel(const dnn_yolo_head head, const float* __restrict__ pred, dnn_detection* __restrict__ dets,
                 int max_det, int* __restrict__ counts, char* workspace) {
  __shared__ unsigned long long keys[CAP];
  __shared__ int kept[CAP];  // box indices of the kept candidates, in output order
  __shared__ long long lds_box[WS ? 1 : CAP][4];
  __shared__ float lds_score[WS ? 1 : CAP];
  __shared__ int lds_cls[WS ? 1 : CAP];
  __shared__ float anchors[2 * DNN_YOLO_MAX_ANCHORS];
  __shared__ unsigned long long hitw[PH_WAVES];
  __shared__ int n_cand, bad, n_kept, zero_den;

  const int img = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int A = head.n_anchors, C = head.n_classes, gw = head.grid_w;
  const int nb = head.grid_h * gw * A, stride = 5 + C;
  const float cell_px = head.cell, score_thr = head.score_thr;
  const double iou_thr = head.iou_thr;
  const float* p = pred + (size_t)img * nb * stride;

  long long (*box)[4];
  float* score_of;
  int* cls_of;
  if constexpr (WS) {
    char* w = workspace + (size_t)img * nb * PH_BOX_BYTES;
    box = reinterpret_cast<long long (*)[4]>(w);
    score_of = reinterpret_cast<float*>(w + (size_t)nb * 32);
    cls_of = reinterpret_cast<int*>(w + (size_t)nb * 36);
  } else {
    box = lds_box;
    score_of = lds_score;
    cls_of = lds_cls;
  }

  int nsort = 1;  // keys that the sort can touch: pow2 >= nb, <= CAP
  while (nsort < nb) nsort <<= 1;
  if (tid == 0) {
    n_cand = 0;
    bad = 0;
    n_kept = 0;
    zero_den = 0;
  }
  if (tid < 2 * A) anchors[tid] = head.anchors[tid];
  for (int i = tid; i < nsort; i += PH_THREADS) keys[i] = ~0ull;
  __syncthreads();

  // ---- phase 1: decode (yolov2tiny.py:123-155)
  for (int k = tid; k < nb; k += PH_THREADS) {
    const float* q = p + (size_t)k * stride;
    const int b = k % A, cell = k / A, col = cell % gw, row = cell / gw;
    const float cx = ((float)col + sigmoid_ref(q[0])) * cell_px;
    const float cy = ((float)row + sigmoid_ref(q[1])) * cell_px;
    const float rw = (np_expf(q[2]) * anchors[2 * b]) * cell_px;
    const float rh = (np_expf(q[3]) * anchors[2 * b + 1]) * cell_px;
    const float conf = sigmoid_ref(q[4]);
    const float* lg = q + 5;
    float m = lg[0];
    for (int c = 1; c < C; ++c) m = lg[c] > m ? lg[c] : m;
    const float s = softmax_sum(lg, C, m);
    int best = 0;
    float bp = np_expf(lg[0] - m) / s;
    for (int c = 1; c < C; ++c) {
      const float pc = np_expf(lg[c] - m) / s;
      if (pc > bp) {  // first index of the max quotient
        bp = pc;
        best = c;
      }
    }
    const float hw = rw / 2.0f, hh = rh / 2.0f;
    long long l = 0, t = 0, r = 0, bt = 0;
    const bool ok = trunc_i64(cx - hw, &l) && trunc_i64(cx + hw, &r) && trunc_i64(cy - hh, &t) &&
                    trunc_i64(cy + hh, &bt);
    if (!ok) bad = 1;
    box[k][0] = l;
    box[k][1] = t;
    box[k][2] = r;
    box[k][3] = bt;
    const float sc = conf * bp;
    score_of[k] = sc;
    cls_of[k] = best;
    if (sc > score_thr) {  // score_thr >= 0: sc is positive, larger float bits = larger score
      const int pos = atomicAdd(&n_cand, 1);
      keys[pos] = ((unsigned long long)(~__float_as_uint(sc)) << 32) | (unsigned)k;
    }
  }
  __syncthreads();
  const int n = n_cand;
  if (bad) {
    if (tid == 0) counts[img] = -1;
    return;
  }

  // ---- phase 2: bitonic sort of the first pow2 >= n keys (yolov2tiny.py:158)
  int ns = 1;
  while (ns < n) ns <<= 1;
  for (int kk = 2; kk <= ns; kk <<= 1) {
    for (int j = kk >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < ns; i += PH_THREADS) {
        const int ij = i ^ j;
        if (ij > i) {
          const unsigned long long a = keys[i], c = keys[ij];
          if (((i & kk) == 0) == (a > c)) {
            keys[i] = c;
            keys[ij] = a;
          }
        }
      }
      __syncthreads();
    }
  }

  // ---- phase 3: blocked greedy NMS (yolov2tiny.py:200-227)
  for (int base = 0; base < n; base += 64) {
    const int m = n - base < 64 ? n - base : 64;
    const int nk = n_kept;  // kept from earlier blocks: final
    const bool live = lane < m;
    const int mine = live ? (int)(keys[base + lane] & 0xffffffffu) : 0;
    long long bi[4] = {0, 0, 0, 0};
    if (live) {
      bi[0] = box[mine][0];
      bi[1] = box[mine][1];
      bi[2] = box[mine][2];
      bi[3] = box[mine][3];
    }
    bool hit = false, zd = false;
    for (int j = wid; j < nk; j += PH_WAVES) {
      const int kj = kept[j];  // wave-uniform
      const long long bj[4] = {box[kj][0], box[kj][1], box[kj][2], box[kj][3]};
      if (live && iou_gt(bi, bj, iou_thr, &zd)) hit = true;
    }
    const unsigned long long hw_ = __ballot(hit);
    if (lane == 0) hitw[wid] = hw_;
    if (__any(zd) && lane == 0) zero_den = 1;
    __syncthreads();
    if (wid == 0) {
      unsigned long long dropped = m < 64 ? ~((1ull << m) - 1ull) : 0ull;
#pragma unroll
      for (int w = 0; w < PH_WAVES; ++w) dropped |= hitw[w];
      bool zt = false;
      for (int i = 0; i < m; ++i) {
        if ((dropped >> i) & 1ull) continue;  // wave-uniform: candidate i is kept
        const int ki = (int)(keys[base + i] & 0xffffffffu);
        const long long bk[4] = {box[ki][0], box[ki][1], box[ki][2], box[ki][3]};
        const bool h = live && lane > i && iou_gt(bi, bk, iou_thr, &zt);
        dropped |= __ballot(h);
      }
      const unsigned long long keep = ~dropped;
      if ((keep >> lane) & 1ull) kept[nk + __popcll(keep & ((1ull << lane) - 1ull))] = mine;
      if (__any(zt) && lane == 0) zero_den = 1;
      if (lane == 0) n_kept = nk + __popcll(keep);
    }
    __syncthreads();
  }

  if (zero_den) {
    if (tid == 0) counts[img] = -2;
    return;
  }
  const int nk = n_kept, nw = nk < max_det ? nk : max_det;
  for (int r = tid; r < nw; r += PH_THREADS) {
    const int k = kept[r];
    dnn_detection d;
    d.cls = cls_of[k];
    d.score = score_of[k];
    d.left = box[k][0];
    d.top = box[k][1];
    d.right = box[k][2];
    d.bottom = box[k][3];
    dets[(size_t)img * max_det + r] = d;
  }
  if (tid == 0) counts[img] = nk;
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
  return nb > PH_LDS_BOXES ? (unsigned long long)n_images * nb * PH_BOX_BYTES : 0ull;
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
  static const float voc[10] = {1.08f, 1.19f, 3.42f, 4.41f, 6.63f, 11.38f, 9.42f, 5.11f, 16.62f, 10.52f};
  dnn_yolo_head h = {};
  h.grid_h = grid_h;
  h.grid_w = grid_w;
  h.n_anchors = 5;
  h.n_classes = 20;
  h.cell = 32.0f;
  h.score_thr = 0.3f;
  h.iou_thr = 0.3;
  for (int i = 0; i < 10; ++i) h.anchors[i] = voc[i];
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
  const size_t pf = (size_t)n_images * nb * (5 + head->n_classes) * sizeof(float);
  const size_t pb = (pf + 7) & ~(size_t)7;  // keeps dets and the workspace 8-byte aligned
  const size_t db = (size_t)n_images * max_det * sizeof(dnn_detection);
  const size_t cb = ((size_t)n_images * sizeof(int) + 7) & ~(size_t)7;
  const size_t wb = (size_t)dnnhip::head_workspace(nb, n_images);
  char* buf = nullptr;
  DNN_HIP_TRY(hipMalloc(&buf, pb + db + cb + wb));
  float* d_pred = reinterpret_cast<float*>(buf);
  dnn_detection* d_dets = reinterpret_cast<dnn_detection*>(buf + pb);
  int* d_counts = reinterpret_cast<int*>(buf + pb + db);
  int rc = 0;
  if (hipMemcpy(d_pred, pred, pf, hipMemcpyHostToDevice) != hipSuccess) {
    dnnhip::set_error("dnn_yolo_postprocess_head_host: copy in failed");
    rc = -1;
  }
  if (!rc)
    rc = dnnhip::launch_yolo_head(head, d_pred, n_images, d_dets, max_det, d_counts, wb ? buf + pb + db + cb : nullptr,
                                  wb, nullptr);
  if (!rc && (hipMemcpy(counts, d_counts, (size_t)n_images * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess ||
              (db && hipMemcpy(dets, d_dets, db, hipMemcpyDeviceToHost) != hipSuccess))) {
    dnnhip::set_error("dnn_yolo_postprocess_head_host: copy out failed");
    rc = -1;
  }
  (void)hipFree(buf);
  return rc;
}

}  // extern "C"
