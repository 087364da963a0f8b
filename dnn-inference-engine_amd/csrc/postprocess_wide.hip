// Multi-scale YOLO postprocessing for heads of up to DNN_YOLO_WIDE_MAX_BOXES boxes
// (include/dnn_hip_post.h: the *_wide entries).  postprocess_multi.hip keeps one sort key per BOX
// in LDS and decodes an image in one workgroup; only candidates (scores above the threshold) are
// ever sorted, so here the two counts are separate and the decode is spread over the grid:
//
//   yolo_wide_clear_kernel   zeroes the per-image counter blocks (candidates, bad corner): 64 B
//                            each.  A kernel, not hipMemsetAsync: a memset node captured into a
//                            HIP graph replayed stale bytes into the counters once other copies
//                            had run between capture and replay (seen on ROCm 7).
//   yolo_wide_decode_kernel  grid (chunk of PW_DEC_THREADS boxes, image), one thread per box: the
//                            per-box arithmetic of post_multi_dev.h, corners (and score / class, or
//                            conf / softmax sum) to the workspace's 40 bytes per box; a candidate
//                            appends its 8-byte key to the image's list of PM_CAP keys in GLOBAL
//                            memory, one device-scope atomic per wave with the wave's candidate
//                            count.  The counter counts every candidate, a key is stored only
//                            while its position is below PM_CAP.  Class scores are evaluated only
//                            where conf > score_thr: p[c] <= 1 and fp32 multiplication is monotone,
//                            so conf * p[c] <= conf and no candidate is lost, in every mode.
//   yolo_wide_nms_kernel     one workgroup per image: -1 for a bad corner, -3 for more than PM_CAP
//                            candidates, else the keys go to LDS (padded to a power of two, the
//                            per-class counts rebuilt from them) and phases 2 to 4 run on them:
//                            the helpers of post_multi_dev.h that postprocess_multi.hip's
//                            kernels call, here with the index field PW_IDX_BITS wide.
//
// The kernel boundary orders the decode's writes before the NMS's reads; nothing waits inside a
// kernel.  The keys are unique (they hold the box index, and in multi-label mode the class), so the
// sorted order, and with it every row, does not depend on the order in which the waves appended.
// The three key layouts are post_multi_dev.h's (key_any, key_class, key_merge).
//
// Workspace, n images of nb boxes: n counter blocks of 64 bytes, then per image 40 nb bytes of
// boxes (the layout of postprocess_multi.hip), then per image PM_CAP keys.
#include "post_multi_dev.h"

namespace dnnhip {

constexpr int PW_DEC_THREADS = 256;
constexpr int PW_CTR_BYTES = 64;  // int 0: candidates, int 1: a corner was not finite or out of range
constexpr unsigned long long PW_KEY_BYTES = (unsigned long long)PM_CAP * 8ull;
constexpr int PW_ANY = 0, PW_PER_CLASS = 1, PW_MULTI = 2;
// Logistic class scores: 1 = a wave with few gated boxes shares their classes across its lanes,
// 0 = a box's thread always loops over its classes itself.  The results are the same bits;
// DESIGN.md §8 has the measurement behind the default.
#ifndef PW_SHARE_LOGITS
#define PW_SHARE_LOGITS 1
#endif
static_assert(PW_DEC_THREADS % 64 == 0 && PW_DEC_THREADS >= 2 * DNN_YOLO_MAX_ANCHORS, "whole waves; the anchor copy");

// the parts of an image's workspace (see the top of the file)
__device__ __forceinline__ int* ws_counters(char* ws, int img) {
  return reinterpret_cast<int*>(ws + (size_t)img * PW_CTR_BYTES);
}
__device__ __forceinline__ char* ws_boxes(char* ws, int img, int nb, int n_images) {
  return ws + (size_t)n_images * PW_CTR_BYTES + (size_t)img * nb * PM_BOX_BYTES;
}
__device__ __forceinline__ unsigned long long* ws_keys(char* ws, int img, int nb, int n_images) {
  return reinterpret_cast<unsigned long long*>(ws + (size_t)n_images * (PW_CTR_BYTES + (size_t)nb * PM_BOX_BYTES) +
                                               (size_t)img * PW_KEY_BYTES);
}

// Position of this lane's candidate in the image's list, or -1 without one: one atomic per wave
// with the number of lanes that have a candidate.  Every lane of the wave calls it together.
__device__ __forceinline__ int wave_append(int* counter, bool want, int lane) {
  const unsigned long long m = __ballot(want);
  if (m == 0) return -1;  // wave-uniform
  const int leader = __ffsll((long long)m) - 1;
  int base = 0;
  if (lane == leader) base = atomicAdd(counter, __popcll(m));  // device scope
  base = __shfl(base, leader);
  return want ? base + __popcll(m & ((1ull << lane) - 1ull)) : -1;
}

__global__ void __launch_bounds__(PW_DEC_THREADS) yolo_wide_clear_kernel(int* counters, int n_ints) {
  const int i = blockIdx.x * PW_DEC_THREADS + threadIdx.x;
  if (i < n_ints) counters[i] = 0;
}

template <int MODE>
__global__ void __launch_bounds__(PW_DEC_THREADS)
yolo_wide_decode_kernel(const dnn_yolo_multi mh, const XyScale xy, const MultiPred pred, char* workspace, int nb,
                        int n_images) {
  __shared__ ScaleTab t;
  const int img = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
  const int S = mh.n_scales, C = mh.scale[0].n_classes, stride = 5 + C;
  const bool logistic = mh.class_mode == 1;
  const float score_thr = mh.scale[0].score_thr;

  int* ctr = ws_counters(workspace, img);
  const BoxStore bs = box_store(ws_boxes(workspace, img, nb, n_images), nb);  // multi-label: score is the conf
  unsigned long long* keys = ws_keys(workspace, img, nb, n_images);

  fill_scale_tab(t, mh, &xy, pred, img, stride, tid);
  __syncthreads();

  // every thread stays to the end: the appends below are whole-wave operations
  const int k = blockIdx.x * PW_DEC_THREADS + tid;
  const bool in = k < nb;
  BoxAt at = {};
  float conf = 0.0f;
  bool gate = false;  // conf > score_thr: only then can a class score be above it
  if (in) {
    at = box_at(t, S, k, stride);
    decode_corners_at(t, at, bs, k, &conf, &ctr[1]);
    gate = conf > score_thr;
  }
  const float* q = at.q;
  float sc = 0.0f;  // single-label modes: this box's score and class
  int best = 0;
  if (MODE == PW_MULTI && in) bs.score[k] = conf;
  if (!__any(gate)) return;  // wave-uniform: no box of this wave can be a candidate

  // Logistic classes are independent, so a wave with FEW gated boxes takes them one at a time, lane l
  // the classes l, l + 64, ...: a load is 64 consecutive logits and a skipped box costs nothing.
  // That is G (ceil(C / 64) + 1) steps for G gated boxes (the + 1: the arg-max reduction) against
  // the C steps of every gated thread looping over its own classes, so it is taken while it is
  // fewer (measured both ways, DESIGN.md §8: sharing loses once most boxes pass the gate).
  unsigned long long todo = __ballot(gate);
  if (PW_SHARE_LOGITS && logistic && __popcll(todo) * ((C + 63) / 64 + 1) <= C) {
    while (todo) {  // wave-uniform
      const int g = __ffsll((long long)todo) - 1;
      todo &= todo - 1ull;
      const int sg = __shfl(at.s, g), kg = __shfl(k, g);
      const float cg = __shfl(conf, g);
      const float* lg = box_values(t, sg, kg, stride) + 5;
      if (MODE == PW_MULTI) {
        for (int c0 = 0; c0 < C; c0 += 64) {
          const int c = c0 + lane;
          const float sl = c < C ? label_score(lg[c], true, cg, 0.0f, 1.0f) : 0.0f;
          const int pos = wave_append(ctr, c < C && sl > score_thr, lane);
          if (pos >= 0 && pos < PM_CAP) keys[pos] = key_class<PW_IDX_BITS>(c, sl, kg);
        }
        continue;
      }
      // class_argmax over the lanes: the largest rounded p, the first index among equals
      float bp = -1.0f, p0 = 0.0f;  // (every p is >= 0)
      int bc = 0x7fffffff;
      for (int c = lane; c < C; c += 64) {
        const float pc = sigmoid_ref(lg[c]);
        if (c == 0) p0 = pc;
        if (pc > bp) {
          bp = pc;
          bc = c;
        }
      }
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) {
        const float obp = __shfl_xor(bp, d);
        const int obc = __shfl_xor(bc, d);
        if (obp > bp || (obp == bp && obc < bc)) {
          bp = obp;
          bc = obc;
        }
      }
      p0 = __shfl(p0, 0);
      if (p0 != p0) {  // a NaN in class 0 stays class_argmax's result: no later class compares above it
        bp = p0;
        bc = 0;
      }
      if (lane == g) {
        sc = conf * bp;
        best = bc;
      }
    }
    if (MODE == PW_MULTI) return;
  } else if (MODE == PW_MULTI) {
    float m = 0.0f, sum = 1.0f;
    if (gate && !logistic) {
      m = logit_max(q + 5, C);
      sum = softmax_sum(q + 5, C, m);
      bs.sum()[k] = sum;
    }
    for (int c = 0; c < C; ++c) {  // wave-uniform trip count: one key per (box, class) above the threshold
      float sl = 0.0f;
      if (gate) sl = label_score(q[5 + c], logistic, conf, m, sum);
      const int pos = wave_append(ctr, gate && sl > score_thr, lane);
      if (pos >= 0 && pos < PM_CAP) keys[pos] = key_class<PW_IDX_BITS>(c, sl, k);
    }
    return;
  } else if (gate) {
    sc = conf * class_argmax(q + 5, C, logistic, &best);  // decode_box's score
  }

  if (gate) {
    bs.score[k] = sc;
    bs.cls[k] = best;
  }
  const int pos = wave_append(ctr, gate && sc > score_thr, lane);
  if (pos >= 0 && pos < PM_CAP)  // beyond it only the count matters: the image ends with -3
    keys[pos] = MODE == PW_ANY ? key_any(sc, k) : key_class<PW_IDX_BITS>(best, sc, k);
}

template <int MODE>
__global__ void __launch_bounds__(PM_THREADS)
yolo_wide_nms_kernel(const dnn_yolo_multi mh, const MultiPred pred, dnn_detection* __restrict__ dets, int max_det,
                     int* __restrict__ counts, char* workspace, int nb, int n_images) {
  __shared__ unsigned long long keys[PM_CAP];
  __shared__ ScaleTab t;  // the multi-label merge reads the logits again
  __shared__ typename std::conditional<MODE == PW_ANY, NmsState, ClassState>::type st;

  const int img = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int S = mh.n_scales, C = mh.scale[0].n_classes, stride = 5 + C;
  const double iou_thr = mh.scale[0].iou_thr;

  const int* ctr = ws_counters(workspace, img);
  const BoxStore bs = box_store(ws_boxes(workspace, img, nb, n_images), nb);  // multi-label: score is the conf
  const unsigned long long* gkeys = ws_keys(workspace, img, nb, n_images);
  dnn_detection* rows = dets + (size_t)img * max_det;

  const int n = ctr[0];  // workgroup-uniform, like the two exits below
  if (ctr[1]) {
    if (tid == 0) counts[img] = -1;
    return;
  }
  if (n > PM_CAP) {
    if (tid == 0) counts[img] = -3;
    return;
  }
  reset_state(st, tid);
  if (MODE == PW_MULTI) fill_scale_tab(t, mh, nullptr, pred, img, stride, tid);
  __syncthreads();

  // the keys into LDS, padded to the power of two that the sort touches
  int ns = 1;
  while (ns < n) ns <<= 1;
  for (int i = tid; i < ns; i += PM_THREADS) {
    const unsigned long long key = i < n ? gkeys[i] : ~0ull;
    keys[i] = key;
    if constexpr (MODE != PW_ANY)
      if (i < n) atomicAdd(&st.cls_cnt[key_class_class<PW_IDX_BITS>(key)], 1);
  }
  __syncthreads();

  if constexpr (MODE == PW_ANY) {
    nms_any_emit<PM_THREADS>(keys, n, bs, iou_thr, st, rows, max_det, &counts[img], tid);
  } else {
    if (wid == 0) wave_scan_128(st.cls_cnt, C, st.seg_start, lane);

    // ---- phase 2: class-major bitonic sort
    bitonic_sort<PM_THREADS>(keys, ns, tid);
    __syncthreads();  // seg_start too (the sort has no barrier when n <= 1)

    // ---- phase 3: every class segment alone; phase 4: merge by (score, global index[, class])
    const int nk = nms_segments<PW_IDX_BITS>(keys, C, bs.box, iou_thr, st, tid);
    if (nk < 0) {
      if (tid == 0) counts[img] = -2;
      return;
    }
    int mine[16];
    gather_kept<PW_IDX_BITS, MODE == PW_MULTI>(keys, C, nk, st, mine, tid);
    if (MODE == PW_PER_CLASS)
      merge_single(keys, mine, nk, bs, rows, max_det, &counts[img], tid);
    else
      merge_labels<PW_IDX_BITS>(keys, mine, nk, t, S, C, stride, mh.class_mode == 1, bs, rows, max_det, &counts[img],
                                tid);
  }
}

static unsigned long long wide_workspace(int nb, int n_images) {
  return (unsigned long long)n_images * ((unsigned long long)nb * PM_BOX_BYTES + PW_KEY_BYTES + PW_CTR_BYTES);
}

template <int MODE>
static void launch_wide_kernels(const dnn_yolo_multi& m, const XyScale& xy, const MultiPred& mp, int n_images,
                                dnn_detection* dets, int max_det, int* counts, char* ws, int nb, hipStream_t stream) {
  const dim3 grid((nb + PW_DEC_THREADS - 1) / PW_DEC_THREADS, n_images);
  hipLaunchKernelGGL(yolo_wide_decode_kernel<MODE>, grid, dim3(PW_DEC_THREADS), 0, stream, m, xy, mp, ws, nb,
                     n_images);
  hipLaunchKernelGGL(yolo_wide_nms_kernel<MODE>, dim3(n_images), dim3(PM_THREADS), 0, stream, m, mp, dets, max_det,
                     counts, ws, nb, n_images);
}

static int launch_yolo_wide(const MultiCall& c, hipStream_t stream);
// (65535 images: the decode grid's second dimension)
static const MultiKind WIDE = {DNN_YOLO_WIDE_MAX_BOXES, 65535, wide_workspace, launch_yolo_wide};

static int launch_yolo_wide(const MultiCall& c, hipStream_t stream) {
  MultiArgs a;
  const int go = check_multi_call(c, WIDE, false, &a);
  if (go <= 0) return go;
  char* ws = static_cast<char*>(c.workspace);
  const int n_ints = c.n_images * (PW_CTR_BYTES / 4);
  hipLaunchKernelGGL(yolo_wide_clear_kernel, dim3((n_ints + PW_DEC_THREADS - 1) / PW_DEC_THREADS),
                     dim3(PW_DEC_THREADS), 0, stream, reinterpret_cast<int*>(ws), n_ints);
  // with one class the rules and the label modes are the same function: the class-agnostic kernels
  // serve them all
  const bool one = c.m->scale[0].n_classes == 1;
  const auto launch = c.labels_mode == DNN_YOLO_LABELS_MULTI && !one   ? launch_wide_kernels<PW_MULTI>
                      : c.nms_mode == DNN_YOLO_NMS_PER_CLASS && !one ? launch_wide_kernels<PW_PER_CLASS>
                                                                      : launch_wide_kernels<PW_ANY>;
  launch(*c.m, a.xy, a.mp, c.n_images, c.dets, c.max_det, c.counts, ws, a.nb, stream);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("launch yolo_wide: %s", hipGetErrorString(e));
    return -1;
  }
  return 0;
}

}  // namespace dnnhip

extern "C" {

using dnnhip::WIDE;

int dnn_yolo_wide_boxes(const dnn_yolo_multi* m) {
  return dnnhip::multi_boxes_upto(m, "dnn_yolo_wide_boxes", WIDE.max_boxes);
}

int dnn_yolo_wide_workspace(const dnn_yolo_multi* m, int n_images, unsigned long long* bytes) {
  const int nb = dnnhip::multi_boxes_upto(m, "dnn_yolo_wide_workspace", WIDE.max_boxes);
  if (nb < 0) return nb;
  DNN_REQUIRE(n_images >= 0 && bytes, "dnn_yolo_wide_workspace: bad arguments (n_images=%d)", n_images);
  *bytes = dnnhip::wide_workspace(nb, n_images);
  return 0;
}

int dnn_yolo_postprocess_wide(const dnn_yolo_multi* m, const float* const* pred, int n_images, dnn_detection* dets,
                              int max_det, int* counts, void* workspace, unsigned long long workspace_bytes,
                              int nms_mode, int labels_mode, void* stream) {
  return WIDE.launch({"dnn_yolo_postprocess_wide", m, nullptr, pred, n_images, dets, max_det, counts, workspace,
                      workspace_bytes, nms_mode, labels_mode}, static_cast<hipStream_t>(stream));
}

int dnn_yolo_postprocess_wide_host(const dnn_yolo_multi* m, const float* const* pred, int n_images,
                                   dnn_detection* dets, int max_det, int* counts, int nms_mode, int labels_mode) {
  return dnnhip::yolo_multi_host({"dnn_yolo_postprocess_wide_host", m, nullptr, pred, n_images, dets, max_det, counts,
                                  nullptr, 0, nms_mode, labels_mode}, WIDE);
}

int dnn_yolo_postprocess_wide_xy(const dnn_yolo_multi* m, const float* scale_x_y, const float* const* pred,
                                 int n_images, dnn_detection* dets, int max_det, int* counts, void* workspace,
                                 unsigned long long workspace_bytes, int nms_mode, int labels_mode, void* stream) {
  return WIDE.launch({"dnn_yolo_postprocess_wide_xy", m, scale_x_y, pred, n_images, dets, max_det, counts, workspace,
                      workspace_bytes, nms_mode, labels_mode}, static_cast<hipStream_t>(stream));
}

int dnn_yolo_postprocess_wide_xy_host(const dnn_yolo_multi* m, const float* scale_x_y, const float* const* pred,
                                      int n_images, dnn_detection* dets, int max_det, int* counts, int nms_mode,
                                      int labels_mode) {
  return dnnhip::yolo_multi_host({"dnn_yolo_postprocess_wide_xy_host", m, scale_x_y, pred, n_images, dets, max_det,
                                  counts, nullptr, 0, nms_mode, labels_mode}, WIDE);
}

}  // extern "C"
