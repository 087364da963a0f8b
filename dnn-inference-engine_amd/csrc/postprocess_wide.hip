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
//                            per-class counts rebuilt from them) and postprocess_multi.hip's
//                            phases 2 to 4 run on them through the same helpers.
//
// The kernel boundary orders the decode's writes before the NMS's reads; nothing waits inside a
// kernel.  The keys are unique (they hold the box index, and in multi-label mode the class), so the
// sorted order, and with it every row, does not depend on the order in which the waves appended.
//
// Keys, the index field 16 bits wide:
//   class-agnostic      ~score (32) | index (32)
//   per-class           class (7) | ~score (32) | index (16)
//   multi-label merge   ~score (32) | index (16) | class (7)
//
// Workspace, n images of nb boxes: n counter blocks of 64 bytes, then per image 40 nb bytes of
// boxes (the layout of postprocess_multi.hip), then per image PM_CAP keys.
#include "post_multi_dev.h"

namespace dnnhip {

constexpr int PW_DEC_THREADS = 256;
constexpr int PW_IDX_BITS = 16;
constexpr int PW_CTR_BYTES = 64;  // int 0: candidates, int 1: a corner was not finite or out of range
constexpr unsigned long long PW_KEY_BYTES = (unsigned long long)PM_CAP * 8ull;
constexpr int PW_ANY = 0, PW_PER_CLASS = 1, PW_MULTI = 2;
// Logistic class scores: 1 = a wave with few gated boxes shares their classes across its lanes,
// 0 = a box's thread always loops over its classes itself.  The results are the same bits;
// DESIGN.md §8 has the measurement behind the default.
#ifndef PW_SHARE_LOGITS
#define PW_SHARE_LOGITS 1
#endif
constexpr int PW_IDX_MASK = (1 << PW_IDX_BITS) - 1, PW_CLS_MASK = (1 << PC_CLS_BITS) - 1;
static_assert(DNN_YOLO_WIDE_MAX_BOXES <= (1 << PW_IDX_BITS), "the global box index does not fit its key field");
static_assert(PC_CLS_BITS + 32 + PW_IDX_BITS < 64, "a candidate's key must stay below ~0ull");
static_assert(PC_CLS_BITS + PW_IDX_BITS < 31, "a kept entry (index | class) is an int");
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

// Per-scale parameters of one image in LDS (what postprocess_multi.hip's kernels set up inline).
struct ScaleTab {
  float anchors[DNN_YOLO_MAX_SCALES][2 * DNN_YOLO_MAX_ANCHORS];
  const float* pred[DNN_YOLO_MAX_SCALES];
  int off[DNN_YOLO_MAX_SCALES + 1], gw[DNN_YOLO_MAX_SCALES], na[DNN_YOLO_MAX_SCALES];
  float cell[DNN_YOLO_MAX_SCALES];
};

// By the whole workgroup; the caller's next barrier publishes it.
__device__ __forceinline__ void fill_scale_tab(ScaleTab& t, const dnn_yolo_multi& mh, const MultiPred& pred, int img,
                                               int stride, int tid) {
  if (tid == 0) {
    int off = 0;
#pragma unroll
    for (int s = 0; s < DNN_YOLO_MAX_SCALES; ++s) {
      const bool on = s < mh.n_scales;
      const int b = on ? mh.scale[s].grid_h * mh.scale[s].grid_w * mh.scale[s].n_anchors : 0;
      t.off[s] = off;
      t.gw[s] = on ? mh.scale[s].grid_w : 1;
      t.na[s] = on ? mh.scale[s].n_anchors : 1;
      t.cell[s] = on ? mh.scale[s].cell : 1.0f;
      t.pred[s] = on ? pred.p[s] + (size_t)img * b * stride : nullptr;
      off += b;
    }
    t.off[DNN_YOLO_MAX_SCALES] = off;
  }
  if (tid < 2 * DNN_YOLO_MAX_ANCHORS) {
#pragma unroll
    for (int s = 0; s < DNN_YOLO_MAX_SCALES; ++s) t.anchors[s][tid] = mh.scale[s].anchors[tid];
  }
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
  __shared__ float s_xs[DNN_YOLO_MAX_SCALES], s_xb[DNN_YOLO_MAX_SCALES];
  const int img = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
  const int S = mh.n_scales, C = mh.scale[0].n_classes, stride = 5 + C;
  const bool logistic = mh.class_mode == 1;
  const float score_thr = mh.scale[0].score_thr;

  int* ctr = ws_counters(workspace, img);
  char* w = ws_boxes(workspace, img, nb, n_images);
  long long (*box)[4] = reinterpret_cast<long long (*)[4]>(w);
  float* score_of = reinterpret_cast<float*>(w + (size_t)nb * 32);  // multi-label: conf
  int* cls_of = reinterpret_cast<int*>(w + (size_t)nb * 36);
  float* sum_of = reinterpret_cast<float*>(w + (size_t)nb * 36);  // multi-label softmax: the box's sum
  unsigned long long* keys = ws_keys(workspace, img, nb, n_images);

  fill_scale_tab(t, mh, pred, img, stride, tid);
  if (tid < DNN_YOLO_MAX_SCALES) {
    s_xs[tid] = xy.s[tid];
    s_xb[tid] = xy.b[tid];
  }
  __syncthreads();

  // every thread stays to the end: the appends below are whole-wave operations
  const int k = blockIdx.x * PW_DEC_THREADS + tid;
  const bool in = k < nb;
  const float* q = nullptr;
  float conf = 0.0f;
  bool gate = false;  // conf > score_thr: only then can a class score be above it
  int s = 0;
  if (in) {
    while (s + 1 < S && k >= t.off[s + 1]) ++s;
    const int kk = k - t.off[s], A = t.na[s], gw = t.gw[s];
    q = t.pred[s] + (size_t)kk * stride;
    const int b = kk % A, cell = kk / A, col = cell % gw, row = cell / gw;
    long long c4[4];
    if (!decode_corners(q, b, col, row, t.anchors[s], t.cell[s], s_xs[s], s_xb[s], c4, &conf)) ctr[1] = 1;
    box[k][0] = c4[0];
    box[k][1] = c4[1];
    box[k][2] = c4[2];
    box[k][3] = c4[3];
    gate = conf > score_thr;
  }
  auto label_key = [&](int c, float sc, int box_k) {  // per-class and multi-label: class-major
    return ((unsigned long long)c << (32 + PW_IDX_BITS)) | ((unsigned long long)(~__float_as_uint(sc)) << PW_IDX_BITS) |
           (unsigned)box_k;
  };
  float sc = 0.0f;  // single-label modes: this box's score and class
  int best = 0;
  if (MODE == PW_MULTI && in) score_of[k] = conf;
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
      const int sg = __shfl(s, g), kg = __shfl(k, g);
      const float cg = __shfl(conf, g);
      const float* lg = t.pred[sg] + (size_t)(kg - t.off[sg]) * stride + 5;
      if (MODE == PW_MULTI) {
        for (int c0 = 0; c0 < C; c0 += 64) {
          const int c = c0 + lane;
          const float sl = c < C ? label_score(lg[c], true, cg, 0.0f, 1.0f) : 0.0f;
          const int pos = wave_append(ctr, c < C && sl > score_thr, lane);
          if (pos >= 0 && pos < PM_CAP) keys[pos] = label_key(c, sl, kg);
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
      sum_of[k] = sum;
    }
    for (int c = 0; c < C; ++c) {  // wave-uniform trip count: one key per (box, class) above the threshold
      float sl = 0.0f;
      if (gate) sl = label_score(q[5 + c], logistic, conf, m, sum);
      const int pos = wave_append(ctr, gate && sl > score_thr, lane);
      if (pos >= 0 && pos < PM_CAP) keys[pos] = label_key(c, sl, k);
    }
    return;
  } else if (gate) {
    sc = conf * class_argmax(q + 5, C, logistic, &best);  // decode_box's score
  }

  if (gate) {
    score_of[k] = sc;
    cls_of[k] = best;
  }
  // score_thr >= 0: sc is positive, larger float bits = larger score
  const int pos = wave_append(ctr, gate && sc > score_thr, lane);
  if (pos >= 0 && pos < PM_CAP)  // beyond it only the count matters: the image ends with -3
    keys[pos] = MODE == PW_ANY ? ((unsigned long long)(~__float_as_uint(sc)) << 32) | (unsigned)k
                               : label_key(best, sc, k);
}

template <int MODE>
__global__ void __launch_bounds__(PM_THREADS)
yolo_wide_nms_kernel(const dnn_yolo_multi mh, const MultiPred pred, dnn_detection* __restrict__ dets, int max_det,
                     int* __restrict__ counts, char* workspace, int nb, int n_images) {
  __shared__ unsigned long long keys[PM_CAP];
  __shared__ ScaleTab t;  // the multi-label merge reads the logits again
  __shared__ unsigned long long hitw[PM_WAVES];
  __shared__ int cls_cnt[DNN_YOLO_MAX_CLASSES];        // candidates per class
  __shared__ int seg_start[DNN_YOLO_MAX_CLASSES + 1];  // their prefix sum: class c is keys[seg_start[c] .. seg_start[c+1])
  __shared__ int seg_kept[DNN_YOLO_MAX_CLASSES];       // kept per class
  __shared__ int out_off[DNN_YOLO_MAX_CLASSES + 1];    // their prefix sum
  __shared__ int n_kept, zero_den, ticket;

  const int img = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int S = mh.n_scales, C = mh.scale[0].n_classes, stride = 5 + C;
  const bool logistic = mh.class_mode == 1;
  const double iou_thr = mh.scale[0].iou_thr;

  const int* ctr = ws_counters(workspace, img);
  char* w = ws_boxes(workspace, img, nb, n_images);
  const long long (*box)[4] = reinterpret_cast<const long long (*)[4]>(w);
  const float* score_of = reinterpret_cast<const float*>(w + (size_t)nb * 32);  // multi-label: conf
  const int* cls_of = reinterpret_cast<const int*>(w + (size_t)nb * 36);
  const float* sum_of = reinterpret_cast<const float*>(w + (size_t)nb * 36);
  const unsigned long long* gkeys = ws_keys(workspace, img, nb, n_images);

  const int n = ctr[0];  // workgroup-uniform, like the two exits below
  if (ctr[1]) {
    if (tid == 0) counts[img] = -1;
    return;
  }
  if (n > PM_CAP) {
    if (tid == 0) counts[img] = -3;
    return;
  }
  if (tid == 0) {
    n_kept = 0;
    zero_den = 0;
    ticket = 0;
  }
  if (tid < DNN_YOLO_MAX_CLASSES) {
    cls_cnt[tid] = 0;
    seg_kept[tid] = 0;
  }
  if (MODE == PW_MULTI) fill_scale_tab(t, mh, pred, img, stride, tid);
  __syncthreads();

  // the keys into LDS, padded to the power of two that the sort touches
  int ns = 1;
  while (ns < n) ns <<= 1;
  for (int i = tid; i < ns; i += PM_THREADS) {
    const unsigned long long key = i < n ? gkeys[i] : ~0ull;
    keys[i] = key;
    if (MODE != PW_ANY && i < n) atomicAdd(&cls_cnt[(int)(key >> (32 + PW_IDX_BITS))], 1);
  }
  __syncthreads();

  if (MODE == PW_ANY) {
    int* kept = reinterpret_cast<int*>(keys);  // in place over the consumed keys
    bitonic_sort(keys, ns, tid);
    nms_workgroup<32>(keys, n, box, iou_thr, hitw, &n_kept, &zero_den, lane, wid);
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
    return;
  }

  if (wid == 0) wave_scan_128(cls_cnt, C, seg_start, lane);

  // ---- phase 2: class-major bitonic sort
  bitonic_sort(keys, ns, tid);
  __syncthreads();  // seg_start too (the sort has no barrier when n <= 1)

  // ---- phase 3a: one wave per class segment, no barrier, nobody waits
  {
    bool zd = false;
    for (;;) {
      int c = 0;
      if (lane == 0) c = atomicAdd(&ticket, 1);
      c = __builtin_amdgcn_readfirstlane(c);  // lane 0's ticket, in a scalar register
      if (c >= C) break;
      const int s0 = __builtin_amdgcn_readfirstlane(seg_start[c]);
      const int len = __builtin_amdgcn_readfirstlane(seg_start[c + 1]) - s0;
      if (len == 0 || len > PC_BIG) continue;
      const int nk = nms_wave<PW_IDX_BITS>(keys + s0, len, box, iou_thr, lane, &zd);
      if (lane == 0) seg_kept[c] = nk;
    }
    if (__any(zd) && lane == 0) zero_den = 1;
  }
  __syncthreads();

  // ---- phase 3b: the long segments, each by the whole workgroup (n_kept is 0 here)
  for (int c = 0; c < C; ++c) {
    const int s0 = __builtin_amdgcn_readfirstlane(seg_start[c]);
    const int len = __builtin_amdgcn_readfirstlane(seg_start[c + 1]) - s0;
    if (len <= PC_BIG) continue;  // workgroup-uniform
    nms_workgroup<PW_IDX_BITS>(keys + s0, len, box, iou_thr, hitw, &n_kept, &zero_den, lane, wid);
    if (tid == 0) {
      seg_kept[c] = n_kept;
      n_kept = 0;
    }
    __syncthreads();
  }

  // ---- phase 4: merge the kept lists by (score, global index[, class])
  if (wid == 0) wave_scan_128(seg_kept, C, out_off, lane);
  __syncthreads();
  if (zero_den) {
    if (tid == 0) counts[img] = -2;
    return;
  }
  const int nk = out_off[DNN_YOLO_MAX_CLASSES];
  int mine[16];  // entries tid, tid + 1024, ... of the concatenated kept lists: index | class << 16
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int p = tid + i * PM_THREADS;
    mine[i] = 0;
    if (p < nk) {
      int lo = 0, hi = C;  // the class with out_off[lo] <= p < out_off[lo + 1]
      while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (out_off[mid] <= p) lo = mid;
        else hi = mid;
      }
      mine[i] = reinterpret_cast<const int*>(keys + seg_start[lo])[p - out_off[lo]] | (lo << PW_IDX_BITS);
    }
  }
  __syncthreads();  // every list entry is in a register: the keys may be overwritten
  int ns2 = 1;
  while (ns2 < nk) ns2 <<= 1;
  const int nw = nk < max_det ? nk : max_det;

  if (MODE == PW_PER_CLASS) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int p = tid + i * PM_THREADS, k = mine[i] & PW_IDX_MASK;
      if (p < nk)
        keys[p] = ((unsigned long long)(~__float_as_uint(score_of[k])) << 32) | (unsigned)k;
      else if (p < ns2)
        keys[p] = ~0ull;
    }
    __syncthreads();
    bitonic_sort(keys, ns2, tid);
    for (int r = tid; r < nw; r += PM_THREADS) {
      const int k = (int)(keys[r] & 0xffffffffu);
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
    return;
  }

  // multi-label: a dense int list at the start of the key array, expanded in place into the merge
  // keys from the top chunk of 1024 down (the invariant of postprocess_multi.hip's phase 4)
  int* dense = reinterpret_cast<int*>(keys);
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int p = tid + i * PM_THREADS;
    if (p < nk) dense[p] = mine[i];
  }
  for (int p = nk + tid; p < ns2; p += PM_THREADS) keys[p] = ~0ull;  // bytes >= 8 nk: above the dense list
  __syncthreads();
  for (int j = (nk - 1) / PM_THREADS; j >= 0; --j) {  // workgroup-uniform
    const int p = tid + j * PM_THREADS;
    unsigned long long key = 0;
    if (p < nk) {
      const int e = dense[p], k = e & PW_IDX_MASK, c = e >> PW_IDX_BITS;
      int s = 0;
      while (s + 1 < S && k >= t.off[s + 1]) ++s;
      const float* lg = t.pred[s] + (size_t)(k - t.off[s]) * stride + 5;
      const float sum = logistic ? 1.0f : sum_of[k];
      const float sc = label_score(lg[c], logistic, score_of[k], logistic ? 0.0f : logit_max(lg, C), sum);
      key = ((unsigned long long)(~__float_as_uint(sc)) << (PW_IDX_BITS + PC_CLS_BITS)) |
            ((unsigned long long)k << PC_CLS_BITS) | (unsigned)c;
    }
    __syncthreads();
    if (p < nk) keys[p] = key;
  }
  __syncthreads();
  bitonic_sort(keys, ns2, tid);
  for (int r = tid; r < nw; r += PM_THREADS) {
    const unsigned long long key = keys[r];
    const int k = (int)(key >> PC_CLS_BITS) & PW_IDX_MASK;
    dnn_detection d;
    d.cls = (int)key & PW_CLS_MASK;
    d.score = __uint_as_float(~(unsigned)(key >> (PW_IDX_BITS + PC_CLS_BITS)));
    d.left = box[k][0];
    d.top = box[k][1];
    d.right = box[k][2];
    d.bottom = box[k][3];
    dets[(size_t)img * max_det + r] = d;
  }
  if (tid == 0) counts[img] = nk;
}

static int wide_boxes(const dnn_yolo_multi* m, const char* who) {
  return multi_boxes_upto(m, who, DNN_YOLO_WIDE_MAX_BOXES);
}

static unsigned long long wide_workspace(int nb, int n_images) {
  return (unsigned long long)n_images * ((unsigned long long)nb * PM_BOX_BYTES + PW_KEY_BYTES + PW_CTR_BYTES);
}

static bool wide_modes_ok(int nms_mode, int labels_mode, const char* who) {
  if (!nms_mode_ok(nms_mode, who) || !labels_mode_ok(labels_mode, who)) return false;
  if (labels_mode == DNN_YOLO_LABELS_MULTI && nms_mode != DNN_YOLO_NMS_PER_CLASS) {
    set_error("%s: labels_mode %d (multi-label) needs nms_mode %d (per class): under the class-agnostic rule a box's "
              "second label is always suppressed by its first", who, labels_mode, DNN_YOLO_NMS_PER_CLASS);
    return false;
  }
  return true;
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

static int launch_yolo_wide(const char* who, const dnn_yolo_multi* m, const float* scale_x_y,
                            const float* const* pred, int n_images,
                            dnn_detection* dets, int max_det, int* counts, void* workspace,
                            unsigned long long workspace_bytes, int nms_mode, int labels_mode, hipStream_t stream) {
  const int nb = wide_boxes(m, who);
  if (nb < 0) return nb;
  if (!wide_modes_ok(nms_mode, labels_mode, who)) return -2;
  XyScale xy;
  if (!xy_scale_from(scale_x_y, m->n_scales, who, &xy)) return -2;
  if (n_images < 0 || max_det < 0 || (n_images > 0 && (!pred || !counts || (max_det > 0 && !dets)))) {
    set_error("%s: bad arguments (n_images=%d max_det=%d)", who, n_images, max_det);
    return -2;
  }
  if (n_images == 0) return 0;
  if (n_images > 65535) {
    set_error("%s: %d images > 65535, the decode grid's second dimension", who, n_images);
    return -2;
  }
  MultiPred mp = {};
  for (int s = 0; s < m->n_scales; ++s) {
    if (!pred[s]) {
      set_error("%s: pred[%d] is NULL", who, s);
      return -2;
    }
    mp.p[s] = pred[s];
  }
  const unsigned long long need = wide_workspace(nb, n_images);
  if (!workspace || workspace_bytes < need || (reinterpret_cast<uintptr_t>(workspace) & 7u)) {
    set_error("%s: workspace %p of %llu bytes; %d images of %d boxes need %llu bytes, 8-byte aligned", who,
              workspace, workspace_bytes, n_images, nb, need);
    return -2;
  }
  char* ws = static_cast<char*>(workspace);
  const int n_ints = n_images * (PW_CTR_BYTES / 4);
  hipLaunchKernelGGL(yolo_wide_clear_kernel, dim3((n_ints + PW_DEC_THREADS - 1) / PW_DEC_THREADS),
                     dim3(PW_DEC_THREADS), 0, stream, reinterpret_cast<int*>(ws), n_ints);
  // with one class the rules and the label modes are the same function: the class-agnostic kernels
  // serve them all
  const bool one = m->scale[0].n_classes == 1;
  if (labels_mode == DNN_YOLO_LABELS_MULTI && !one)
    launch_wide_kernels<PW_MULTI>(*m, xy, mp, n_images, dets, max_det, counts, ws, nb, stream);
  else if (nms_mode == DNN_YOLO_NMS_PER_CLASS && !one)
    launch_wide_kernels<PW_PER_CLASS>(*m, xy, mp, n_images, dets, max_det, counts, ws, nb, stream);
  else
    launch_wide_kernels<PW_ANY>(*m, xy, mp, n_images, dets, max_det, counts, ws, nb, stream);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("launch yolo_wide: %s", hipGetErrorString(e));
    return -1;
  }
  return 0;
}

// Host pointers, synchronous: allocates the scratch, copies in, runs, copies out.
static int yolo_wide_host(const char* who, const dnn_yolo_multi* m, const float* scale_x_y,
                          const float* const* pred, int n_images,
                          dnn_detection* dets, int max_det, int* counts, int nms_mode, int labels_mode) {
  const int nb = wide_boxes(m, who);
  if (nb < 0) return nb;
  if (!wide_modes_ok(nms_mode, labels_mode, who)) return -2;
  {
    XyScale xy;
    if (!xy_scale_from(scale_x_y, m->n_scales, who, &xy)) return -2;
  }
  DNN_REQUIRE(n_images >= 0 && max_det >= 0, "%s: bad arguments", who);
  if (n_images == 0) return 0;
  DNN_REQUIRE(pred && counts && (max_det == 0 || dets), "%s: NULL pointer", who);
  const int stride = 5 + m->scale[0].n_classes;
  size_t pf[DNN_YOLO_MAX_SCALES] = {0}, poff[DNN_YOLO_MAX_SCALES] = {0}, pb = 0;
  for (int s = 0; s < m->n_scales; ++s) {
    DNN_REQUIRE(pred[s], "%s: pred[%d] is NULL", who, s);
    const dnn_yolo_head& h = m->scale[s];
    pf[s] = (size_t)n_images * h.grid_h * h.grid_w * h.n_anchors * stride * sizeof(float);
    poff[s] = pb;
    pb += (pf[s] + 7) & ~(size_t)7;  // keeps every tensor, dets and the workspace 8-byte aligned
  }
  const size_t db = (size_t)n_images * max_det * sizeof(dnn_detection);
  const size_t cb = ((size_t)n_images * sizeof(int) + 7) & ~(size_t)7;
  const size_t wb = (size_t)wide_workspace(nb, n_images);
  char* buf = nullptr;
  DNN_HIP_TRY(hipMalloc(&buf, pb + db + cb + wb));
  const float* d_pred[DNN_YOLO_MAX_SCALES] = {nullptr, nullptr, nullptr, nullptr};
  dnn_detection* d_dets = reinterpret_cast<dnn_detection*>(buf + pb);
  int* d_counts = reinterpret_cast<int*>(buf + pb + db);
  int rc = 0;
  for (int s = 0; s < m->n_scales && !rc; ++s) {
    d_pred[s] = reinterpret_cast<const float*>(buf + poff[s]);
    if (hipMemcpy(buf + poff[s], pred[s], pf[s], hipMemcpyHostToDevice) != hipSuccess) {
      set_error("%s: copy in failed", who);
      rc = -1;
    }
  }
  if (!rc) rc = launch_yolo_wide(who, m, scale_x_y, d_pred, n_images, d_dets, max_det, d_counts, buf + pb + db + cb, wb,
                                   nms_mode, labels_mode, nullptr);
  if (!rc && (hipMemcpy(counts, d_counts, (size_t)n_images * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess ||
              (db && hipMemcpy(dets, d_dets, db, hipMemcpyDeviceToHost) != hipSuccess))) {
    set_error("%s: copy out failed", who);
    rc = -1;
  }
  (void)hipFree(buf);
  return rc;
}

}  // namespace dnnhip

extern "C" {

int dnn_yolo_wide_boxes(const dnn_yolo_multi* m) { return dnnhip::wide_boxes(m, "dnn_yolo_wide_boxes"); }

int dnn_yolo_wide_workspace(const dnn_yolo_multi* m, int n_images, unsigned long long* bytes) {
  const int nb = dnnhip::wide_boxes(m, "dnn_yolo_wide_workspace");
  if (nb < 0) return nb;
  DNN_REQUIRE(n_images >= 0 && bytes, "dnn_yolo_wide_workspace: bad arguments (n_images=%d)", n_images);
  *bytes = dnnhip::wide_workspace(nb, n_images);
  return 0;
}

int dnn_yolo_postprocess_wide(const dnn_yolo_multi* m, const float* const* pred, int n_images, dnn_detection* dets,
                              int max_det, int* counts, void* workspace, unsigned long long workspace_bytes,
                              int nms_mode, int labels_mode, void* stream) {
  return dnnhip::launch_yolo_wide("dnn_yolo_postprocess_wide", m, nullptr, pred, n_images, dets, max_det, counts,
                                  workspace, workspace_bytes, nms_mode, labels_mode, static_cast<hipStream_t>(stream));
}

int dnn_yolo_postprocess_wide_host(const dnn_yolo_multi* m, const float* const* pred, int n_images,
                                   dnn_detection* dets, int max_det, int* counts, int nms_mode, int labels_mode) {
  return dnnhip::yolo_wide_host("dnn_yolo_postprocess_wide_host", m, nullptr, pred, n_images, dets, max_det, counts,
                                nms_mode, labels_mode);
}

int dnn_yolo_postprocess_wide_xy(const dnn_yolo_multi* m, const float* scale_x_y, const float* const* pred,
                                 int n_images, dnn_detection* dets, int max_det, int* counts, void* workspace,
                                 unsigned long long workspace_bytes, int nms_mode, int labels_mode, void* stream) {
  return dnnhip::launch_yolo_wide("dnn_yolo_postprocess_wide_xy", m, scale_x_y, pred, n_images, dets, max_det, counts,
                                  workspace, workspace_bytes, nms_mode, labels_mode, static_cast<hipStream_t>(stream));
}

int dnn_yolo_postprocess_wide_xy_host(const dnn_yolo_multi* m, const float* scale_x_y, const float* const* pred,
                                      int n_images, dnn_detection* dets, int max_det, int* counts, int nms_mode,
                                      int labels_mode) {
  return dnnhip::yolo_wide_host("dnn_yolo_postprocess_wide_xy_host", m, scale_x_y, pred, n_images, dets, max_det,
                                counts, nms_mode, labels_mode);
}

}  // extern "C"
