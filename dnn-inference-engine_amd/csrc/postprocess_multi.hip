// Multi-scale YOLO postprocessing (include/dnn_hip_post.h: dnn_yolo_multi): the boxes of up to
// DNN_YOLO_MAX_SCALES heads of one image (YOLOv3: strides 32, 16, 8) decoded, thresholded, sorted
// and put through ONE greedy NMS, one workgroup per image, up to DNN_YOLO_MULTI_MAX_BOXES boxes.
// The per-box arithmetic and the three phases are postprocess_head.hip's (post_math.h):
//
//   phase 1  thread per global box index (scale 0's boxes first, each scale in row, col, anchor
//            order): that scale's grid, cell and anchors; class scores by softmax in numpy's
//            add.reduce order (class_mode 0) or one sigmoid_ref per class (class_mode 1, the
//            first index of the largest rounded value wins).  Corners, score and class of every
//            box go to the caller's workspace (40 bytes per box); candidates append a sort key.
//   phase 2  bitonic sort of the keys in LDS (score descending, then global box index).
//   phase 3  the blocked greedy NMS of postprocess_head.hip, 64 candidates at a time.
//
// LDS: the 16384 eight-byte keys are 128 KiB of the CU's 160 KiB, so neither the box store nor
// a separate kept list fits beside them.  The boxes live in the workspace (read back through
// L2).  The kept list (int box indices) is written IN PLACE over the keys that the NMS has
// already consumed: after the block starting at candidate `base` the list has at most
// base + 64 entries, 4 (base + 64) bytes from the start of the array, and the first key still
// to be read sits at byte 8 (base + 64).  Inside a block every key of the block is read into
// registers (one per lane) before the first barrier and the list grows only after it.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "dnn_common.h"
#include "post_math.h"
#include "../../include/dnn_hip_post.h"

namespace dnnhip {

int yolo_head_boxes(const dnn_yolo_head* h, const char* who, long long max_boxes);  // postprocess_head.hip

constexpr int PM_THREADS = 1024;
constexpr int PM_WAVES = PM_THREADS / 64;
constexpr int PM_CAP = DNN_YOLO_MULTI_MAX_BOXES;  // keys: 16384 x 8 B = 128 KiB; + 640 B of per-scale
                                                  // parameters, 128 B of ballot words, 16 B of counters
constexpr int PM_BOX_BYTES = 40;                  // 4 x int64 corners + fp32 score + int class
static_assert((PM_CAP & (PM_CAP - 1)) == 0, "the bitonic sort needs a power of two");

struct MultiPred {
  const float* p[DNN_YOLO_MAX_SCALES];
};

__global__ void __launch_bounds__(PM_THREADS)
yolo_multi_kernel(const dnn_yolo_multi mh, const MultiPred pred, dnn_detection* __restrict__ dets, int max_det,
                  int* __restrict__ counts, char* workspace, int nb) {
  __shared__ unsigned long long keys[PM_CAP];
  __shared__ float anchors[DNN_YOLO_MAX_SCALES][2 * DNN_YOLO_MAX_ANCHORS];
  __shared__ const float* s_pred[DNN_YOLO_MAX_SCALES];
  __shared__ int s_off[DNN_YOLO_MAX_SCALES + 1], s_gw[DNN_YOLO_MAX_SCALES], s_na[DNN_YOLO_MAX_SCALES];
  __shared__ float s_cell[DNN_YOLO_MAX_SCALES];
  __shared__ unsigned long long hitw[PM_WAVES];
  __shared__ int n_cand, bad, n_kept, zero_den;
  int* kept = reinterpret_cast<int*>(keys);  // in place over the consumed keys (see above)

  const int img = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int S = mh.n_scales, C = mh.scale[0].n_classes, stride = 5 + C;
  const bool logistic = mh.class_mode == 1;
  const float score_thr = mh.scale[0].score_thr;
  const double iou_thr = mh.scale[0].iou_thr;

  char* w = workspace + (size_t)img * nb * PM_BOX_BYTES;
  long long (*box)[4] = reinterpret_cast<long long (*)[4]>(w);
  float* score_of = reinterpret_cast<float*>(w + (size_t)nb * 32);
  int* cls_of = reinterpret_cast<int*>(w + (size_t)nb * 36);

  int nsort = 1;  // keys that the sort can touch: pow2 >= nb, <= PM_CAP
  while (nsort < nb) nsort <<= 1;
  if (tid == 0) {
    n_cand = 0;
    bad = 0;
    n_kept = 0;
    zero_den = 0;
    int off = 0;
#pragma unroll
    for (int s = 0; s < DNN_YOLO_MAX_SCALES; ++s) {
      const bool on = s < S;
      const int b = on ? mh.scale[s].grid_h * mh.scale[s].grid_w * mh.scale[s].n_anchors : 0;
      s_off[s] = off;
      s_gw[s] = on ? mh.scale[s].grid_w : 1;
      s_na[s] = on ? mh.scale[s].n_anchors : 1;
      s_cell[s] = on ? mh.scale[s].cell : 1.0f;
      s_pred[s] = on ? pred.p[s] + (size_t)img * b * stride : nullptr;
      off += b;
    }
    s_off[DNN_YOLO_MAX_SCALES] = off;
  }
  if (tid < 2 * DNN_YOLO_MAX_ANCHORS) {
#pragma unroll
    for (int s = 0; s < DNN_YOLO_MAX_SCALES; ++s) anchors[s][tid] = mh.scale[s].anchors[tid];
  }
  for (int i = tid; i < nsort; i += PM_THREADS) keys[i] = ~0ull;
  __syncthreads();

  // ---- phase 1: decode
  for (int k = tid; k < nb; k += PM_THREADS) {
    int s = 0;
    while (s + 1 < S && k >= s_off[s + 1]) ++s;
    const int kk = k - s_off[s], A = s_na[s], gw = s_gw[s];
    const float cell_px = s_cell[s];
    const float* q = s_pred[s] + (size_t)kk * stride;
    const int b = kk % A, cell = kk / A, col = cell % gw, row = cell / gw;
    const float cx = ((float)col + sigmoid_ref(q[0])) * cell_px;
    const float cy = ((float)row + sigmoid_ref(q[1])) * cell_px;
    const float rw = (np_expf(q[2]) * anchors[s][2 * b]) * cell_px;
    const float rh = (np_expf(q[3]) * anchors[s][2 * b + 1]) * cell_px;
    const float conf = sigmoid_ref(q[4]);
    const float* lg = q + 5;
    int best = 0;
    float bp;
    if (logistic) {
      bp = sigmoid_ref(lg[0]);
      for (int c = 1; c < C; ++c) {
        const float pc = sigmoid_ref(lg[c]);
        if (pc > bp) {  // first index of the largest rounded value
          bp = pc;
          best = c;
        }
      }
    } else {
      float m = lg[0];
      for (int c = 1; c < C; ++c) m = lg[c] > m ? lg[c] : m;
      const float sum = softmax_sum(lg, C, m);
      bp = np_expf(lg[0] - m) / sum;
      for (int c = 1; c < C; ++c) {
        const float pc = np_expf(lg[c] - m) / sum;
        if (pc > bp) {  // first index of the max quotient
          bp = pc;
          best = c;
        }
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

  // ---- phase 2: bitonic sort of the first pow2 >= n keys
  int ns = 1;
  while (ns < n) ns <<= 1;
  for (int kk = 2; kk <= ns; kk <<= 1) {
    for (int j = kk >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < ns; i += PM_THREADS) {
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

  // ---- phase 3: blocked greedy NMS, the kept list in place over keys[0 .. base)
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
    for (int j = wid; j < nk; j += PM_WAVES) {
      const int kj = kept[j];  // wave-uniform
      const long long bj[4] = {box[kj][0], box[kj][1], box[kj][2], box[kj][3]};
      if (live && iou_gt(bi, bj, iou_thr, &zd)) hit = true;
    }
    const unsigned long long hw_ = __ballot(hit);
    if (lane == 0) hitw[wid] = hw_;
    if (__any(zd) && lane == 0) zero_den = 1;
    __syncthreads();  // every wave has read its keys of this block and the kept list
    if (wid == 0) {
      unsigned long long dropped = m < 64 ? ~((1ull << m) - 1ull) : 0ull;
#pragma unroll
      for (int wv = 0; wv < PM_WAVES; ++wv) dropped |= hitw[wv];
      bool zt = false;
      for (int i = 0; i < m; ++i) {
        if ((dropped >> i) & 1ull) continue;  // wave-uniform: candidate i is kept
        const int ki = __shfl(mine, i);       // (no key is read here: the list below overwrites them)
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
  for (int r = tid; r < nw; r += PM_THREADS) {
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

// < 0 with the error set, else the boxes of one image over all scales
static int multi_boxes(const dnn_yolo_multi* m, const char* who) {
  if (!m) {
    set_error("%s: NULL description", who);
    return -2;
  }
  if (m->n_scales < 1 || m->n_scales > DNN_YOLO_MAX_SCALES) {
    set_error("%s: %d scales: need 1..%d", who, m->n_scales, DNN_YOLO_MAX_SCALES);
    return -2;
  }
  if (m->class_mode != 0 && m->class_mode != 1) {
    set_error("%s: class_mode %d: need 0 (softmax) or 1 (logistic)", who, m->class_mode);
    return -2;
  }
  long long total = 0;
  for (int s = 0; s < m->n_scales; ++s) {
    // (the per-scale limit of the single-head entry does not apply: only the sum is bounded)
    const int nb = yolo_head_boxes(&m->scale[s], who, DNN_YOLO_MULTI_MAX_BOXES);
    if (nb < 0) return nb;
    const dnn_yolo_head& h = m->scale[s];
    const dnn_yolo_head& h0 = m->scale[0];
    if (h.n_classes != h0.n_classes || h.score_thr != h0.score_thr || h.iou_thr != h0.iou_thr) {
      set_error("%s: scale %d has %d classes, score_thr %g, iou_thr %g; scale 0 has %d, %g, %g (they must agree)", who,
                s, h.n_classes, (double)h.score_thr, h.iou_thr, h0.n_classes, (double)h0.score_thr, h0.iou_thr);
      return -2;
    }
    total += nb;
  }
  if (total > DNN_YOLO_MULTI_MAX_BOXES) {
    set_error("%s: %lld boxes over %d scales > %d", who, total, m->n_scales, DNN_YOLO_MULTI_MAX_BOXES);
    return -2;
  }
  return (int)total;
}

static unsigned long long multi_workspace(int nb, int n_images) {
  return (unsigned long long)n_images * nb * PM_BOX_BYTES;
}

static int launch_yolo_multi(const dnn_yolo_multi* m, const float* const* pred, int n_images, dnn_detection* dets,
                             int max_det, int* counts, void* workspace, unsigned long long workspace_bytes,
                             hipStream_t stream) {
  const char* who = "dnn_yolo_postprocess_multi";
  const int nb = multi_boxes(m, who);
  if (nb < 0) return nb;
  if (n_images < 0 || max_det < 0 || (n_images > 0 && (!pred || !counts || (max_det > 0 && !dets)))) {
    set_error("%s: bad arguments (n_images=%d max_det=%d)", who, n_images, max_det);
    return -2;
  }
  if (n_images == 0) return 0;
  MultiPred mp = {};
  for (int s = 0; s < m->n_scales; ++s) {
    if (!pred[s]) {
      set_error("%s: pred[%d] is NULL", who, s);
      return -2;
    }
    mp.p[s] = pred[s];
  }
  const unsigned long long need = multi_workspace(nb, n_images);
  if (!workspace || workspace_bytes < need || (reinterpret_cast<uintptr_t>(workspace) & 7u)) {
    set_error("%s: workspace %p of %llu bytes; %d images of %d boxes need %llu bytes, 8-byte aligned", who,
              workspace, workspace_bytes, n_images, nb, need);
    return -2;
  }
  hipLaunchKernelGGL(yolo_multi_kernel, dim3(n_images), dim3(PM_THREADS), 0, stream, *m, mp, dets, max_det, counts,
                     static_cast<char*>(workspace), nb);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("launch yolo_multi: %s", hipGetErrorString(e));
    return -1;
  }
  return 0;
}

}  // namespace dnnhip

extern "C" {

int dnn_yolo_multi_boxes(const dnn_yolo_multi* m) { return dnnhip::multi_boxes(m, "dnn_yolo_multi_boxes"); }

int dnn_yolo_multi_workspace(const dnn_yolo_multi* m, int n_images, unsigned long long* bytes) {
  const int nb = dnnhip::multi_boxes(m, "dnn_yolo_multi_workspace");
  if (nb < 0) return nb;
  DNN_REQUIRE(n_images >= 0 && bytes, "dnn_yolo_multi_workspace: bad arguments (n_images=%d)", n_images);
  *bytes = dnnhip::multi_workspace(nb, n_images);
  return 0;
}

int dnn_yolo_postprocess_multi(const dnn_yolo_multi* m, const float* const* pred, int n_images, dnn_detection* dets,
                               int max_det, int* counts, void* workspace, unsigned long long workspace_bytes,
                               void* stream) {
  return dnnhip::launch_yolo_multi(m, pred, n_images, dets, max_det, counts, workspace, workspace_bytes,
                                   static_cast<hipStream_t>(stream));
}

int dnn_yolo_postprocess_multi_host(const dnn_yolo_multi* m, const float* const* pred, int n_images,
                                    dnn_detection* dets, int max_det, int* counts) {
  const char* who = "dnn_yolo_postprocess_multi_host";
  const int nb = dnnhip::multi_boxes(m, who);
  if (nb < 0) return nb;
  DNN_REQUIRE(n_images >= 0 && max_det >= 0, "dnn_yolo_postprocess_multi_host: bad arguments");
  if (n_images == 0) return 0;
  DNN_REQUIRE(pred && counts && (max_det == 0 || dets), "dnn_yolo_postprocess_multi_host: NULL pointer");
  const int stride = 5 + m->scale[0].n_classes;
  size_t pf[DNN_YOLO_MAX_SCALES] = {0}, poff[DNN_YOLO_MAX_SCALES] = {0}, pb = 0;
  for (int s = 0; s < m->n_scales; ++s) {
    DNN_REQUIRE(pred[s], "dnn_yolo_postprocess_multi_host: pred[%d] is NULL", s);
    const dnn_yolo_head& h = m->scale[s];
    pf[s] = (size_t)n_images * h.grid_h * h.grid_w * h.n_anchors * stride * sizeof(float);
    poff[s] = pb;
    pb += (pf[s] + 7) & ~(size_t)7;  // keeps every tensor, dets and the workspace 8-byte aligned
  }
  const size_t db = (size_t)n_images * max_det * sizeof(dnn_detection);
  const size_t cb = ((size_t)n_images * sizeof(int) + 7) & ~(size_t)7;
  const size_t wb = (size_t)dnnhip::multi_workspace(nb, n_images);
  char* buf = nullptr;
  DNN_HIP_TRY(hipMalloc(&buf, pb + db + cb + wb));
  const float* d_pred[DNN_YOLO_MAX_SCALES] = {nullptr, nullptr, nullptr, nullptr};
  dnn_detection* d_dets = reinterpret_cast<dnn_detection*>(buf + pb);
  int* d_counts = reinterpret_cast<int*>(buf + pb + db);
  int rc = 0;
  for (int s = 0; s < m->n_scales && !rc; ++s) {
    d_pred[s] = reinterpret_cast<const float*>(buf + poff[s]);
    if (hipMemcpy(buf + poff[s], pred[s], pf[s], hipMemcpyHostToDevice) != hipSuccess) {
      dnnhip::set_error("dnn_yolo_postprocess_multi_host: copy in failed");
      rc = -1;
    }
  }
  if (!rc) rc = dnnhip::launch_yolo_multi(m, d_pred, n_images, d_dets, max_det, d_counts, buf + pb + db + cb, wb, nullptr);
  if (!rc && (hipMemcpy(counts, d_counts, (size_t)n_images * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess ||
              (db && hipMemcpy(dets, d_dets, db, hipMemcpyDeviceToHost) != hipSuccess))) {
    dnnhip::set_error("dnn_yolo_postprocess_multi_host: copy out failed");
    rc = -1;
  }
  (void)hipFree(buf);
  return rc;
}

}  // extern "C"
