// Device helpers shared by the multi-scale YOLO decodes (postprocess_multi.hip: everything of an
// image in one workgroup; postprocess_wide.hip: a grid-wide decode kernel, then one NMS workgroup
// per image): the per-box arithmetic, the bitonic sort of the keys in LDS, the blocked greedy NMS
// by a workgroup or by one wave, and the host-side checks of a dnn_yolo_multi.  Both files include
// this, so a box decodes to the same bits and a sorted segment gives the same kept list in either.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "dnn_common.h"
#include "post_math.h"
#include "../../include/dnn_hip_post.h"

namespace dnnhip {

int yolo_head_boxes(const dnn_yolo_head* h, const char* who, long long max_boxes);  // postprocess_head.hip

// postprocess_multi.hip: < 0 with the error set, else the boxes of one image over all scales
// (at most max_boxes), and the checks of the two mode arguments
int multi_boxes_upto(const dnn_yolo_multi* m, const char* who, long long max_boxes);
bool labels_mode_ok(int labels_mode, const char* who);
bool nms_mode_ok(int nms_mode, const char* who);

constexpr int PM_THREADS = 1024;
constexpr int PM_WAVES = PM_THREADS / 64;
constexpr int PM_CAP = DNN_YOLO_MULTI_MAX_BOXES;  // keys: 16384 x 8 B = 128 KiB; + 640 B of per-scale
                                                  // parameters, 128 B of ballot words, 16 B of counters
constexpr int PM_BOX_BYTES = 40;                  // 4 x int64 corners + fp32 score + int class
static_assert((PM_CAP & (PM_CAP - 1)) == 0, "the bitonic sort needs a power of two");

struct MultiPred {
  const float* p[DNN_YOLO_MAX_SCALES];
};

// Darknet's scale_x_y per scale: the box centre's logistic becomes sig * s + b, b = -0.5f * (s - 1.0f)
// computed on the host in fp32.  s == 1 gives b == -0.0f, and sig * 1.0f + -0.0f is sig bit for bit
// for every non-NaN sig: the entries without a scale_x_y argument run the same kernels with that.
struct XyScale {
  float s[DNN_YOLO_MAX_SCALES], b[DNN_YOLO_MAX_SCALES];
};

// postprocess_multi.hip: fills *out from a host array of n_scales floats (NULL: all 1); false with
// the error set (it names scale_x_y) when a value is not finite or not > 0
bool xy_scale_from(const float* scale_x_y, int n_scales, const char* who, XyScale* out);

// Geometry and objectness of one box of one scale (q: its 5 + C values; b, col, row: its anchor and
// cell): corners truncated to int64 in out[0..3] (false when one is not finite or out of range) and
// conf = sigmoid(q[4]).  xs, xb: the scale's XyScale pair, one fp32 multiply then one fp32 add (the
// file is built without contraction).  Shared by all kernels below so that they round alike.
__device__ __forceinline__ bool decode_corners(const float* q, int b, int col, int row, const float* anchors_s,
                                               float cell_px, float xs, float xb, long long* out, float* conf) {
  const float cx = ((float)col + (sigmoid_ref(q[0]) * xs + xb)) * cell_px;
  const float cy = ((float)row + (sigmoid_ref(q[1]) * xs + xb)) * cell_px;
  const float rw = (np_expf(q[2]) * anchors_s[2 * b]) * cell_px;
  const float rh = (np_expf(q[3]) * anchors_s[2 * b + 1]) * cell_px;
  *conf = sigmoid_ref(q[4]);
  const float hw = rw / 2.0f, hh = rh / 2.0f;
  long long l = 0, t = 0, r = 0, bt = 0;
  const bool ok = trunc_i64(cx - hw, &l) && trunc_i64(cx + hw, &r) && trunc_i64(cy - hh, &t) &&
                  trunc_i64(cy + hh, &bt);
  out[0] = l;
  out[1] = t;
  out[2] = r;
  out[3] = bt;
  return ok;
}

// The ONE label of a box from its C class logits: the arg-max class in *cls and its p(class).
__device__ __forceinline__ float class_argmax(const float* lg, int C, bool logistic, int* cls) {
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
  *cls = best;
  return bp;
}

// One box with ONE label: decode_corners, the score conf * p(class) and the class (the arg-max).
__device__ __forceinline__ bool decode_box(const float* q, int C, bool logistic, int b, int col, int row,
                                           const float* anchors_s, float cell_px, float xs, float xb, long long* out,
                                           float* score, int* cls) {
  float conf;
  const bool ok = decode_corners(q, b, col, row, anchors_s, cell_px, xs, xb, out, &conf);
  const float bp = class_argmax(q + 5, C, logistic, cls);
  *score = conf * bp;
  return ok;
}

// The largest class logit of a box, the softmax's shift (class_argmax's loop).
__device__ __forceinline__ float logit_max(const float* lg, int C) {
  float m = lg[0];
  for (int c = 1; c < C; ++c) m = lg[c] > m ? lg[c] : m;
  return m;
}

// Multi-label score of a class from its logit: conf * p[c], one fp32 multiply, p[c] as class_argmax
// computes it (m and sum: the box's logit_max and softmax_sum, unused in logistic mode).  The decode
// and the merge of the multi-label kernels both call this, so an emitted score has the bits it was
// sorted on.
__device__ __forceinline__ float label_score(float logit, bool logistic, float conf, float m, float sum) {
  const float pc = logistic ? sigmoid_ref(logit) : np_expf(logit - m) / sum;
  return conf * pc;
}

// Bitonic sort of keys[0 .. ns) (ns a power of two) by the whole workgroup, ascending.
__device__ __forceinline__ void bitonic_sort(unsigned long long* keys, int ns, int tid) {
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
}

// Blocked greedy NMS of the n sorted candidates seg[0 .. n) by the whole workgroup (every thread
// calls it; *n_kept == 0 on entry, published by a barrier).  The box index is the key's low
// IDX_BITS bits.  The kept list (int box indices) is written in place over seg (see the top of
// postprocess_multi.hip); *n_kept is its length after the closing barrier.
template <int IDX_BITS>
__device__ __forceinline__ void nms_workgroup(unsigned long long* seg, int n, const long long (*box)[4],
                                              double iou_thr, unsigned long long* hitw, int* n_kept, int* zero_den,
                                              int lane, int wid) {
  int* kept = reinterpret_cast<int*>(seg);
  for (int base = 0; base < n; base += 64) {
    const int m = n - base < 64 ? n - base : 64;
    const int nk = *n_kept;  // kept from earlier blocks: final
    const bool live = lane < m;
    const int mine = live ? (int)(seg[base + lane] & ((1ull << IDX_BITS) - 1ull)) : 0;
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
    if (__any(zd) && lane == 0) *zero_den = 1;
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
      if (__any(zt) && lane == 0) *zero_den = 1;
      if (lane == 0) *n_kept = nk + __popcll(keep);
    }
    __syncthreads();
  }
}

constexpr int PC_CLS_BITS = 7;
// Candidates of one class above which the whole workgroup takes the segment.  A wave alone pays for
// every kept box of its segment itself, so long chains are cheaper split over 16 waves even with
// two barriers per block: measured at 256, 1024 and 4096, 256 was never slower.
constexpr int PC_BIG = 256;
static_assert(DNN_YOLO_MAX_CLASSES <= (1 << PC_CLS_BITS), "the class does not fit its key field");
static_assert(PM_CAP <= 16 * PM_THREADS, "phase 4 holds 16 kept entries per thread in registers");

__device__ __forceinline__ long long readlane_i64(long long v, int l) {  // l: wave-uniform
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(unsigned long long)v, l);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)((unsigned long long)v >> 32), l);
  return (long long)(((unsigned long long)hi << 32) | lo);
}

// Orders this wave's own LDS reads and writes (the hardware executes one wave's LDS operations
// in order; this keeps the compiler from moving them across).
__device__ __forceinline__ void wave_lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// start[c] = in[0] + .. + in[c - 1] for c <= 128 (in[c] counts as 0 for c >= C); one whole wave.
__device__ __forceinline__ void wave_scan_128(const int* in, int C, int* start, int lane) {
  const int a = 2 * lane < C ? in[2 * lane] : 0, b = 2 * lane + 1 < C ? in[2 * lane + 1] : 0;
  int incl = a + b;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int v = __shfl_up(incl, d);
    if (lane >= d) incl += v;
  }
  start[2 * lane] = incl - a - b;
  start[2 * lane + 1] = incl - b;
  if (lane == 63) start[128] = incl;
}

// Blocked greedy NMS of the len sorted candidates seg[0 .. len) of one class by ONE wave (all 64
// lanes call it); the box index is the key's low IDX_BITS bits.  Returns the length of the kept
// list, written in place over seg; *zd is set when an evaluated IoU had a zero denominator.
template <int IDX_BITS>
__device__ __forceinline__ int nms_wave(unsigned long long* seg, int len, const long long (*box)[4], double iou_thr,
                                        int lane, bool* zd) {
  int* kept = reinterpret_cast<int*>(seg);
  int nk = 0;
  for (int base = 0; base < len; base += 64) {
    const int m = len - base < 64 ? len - base : 64;
    const bool live = lane < m;
    const int mine = live ? (int)(seg[base + lane] & ((1ull << IDX_BITS) - 1ull)) : 0;
    wave_lds_fence();  // the block's keys are in registers before the list grows over them
    long long bi[4] = {0, 0, 0, 0};
    if (live) {
      bi[0] = box[mine][0];
      bi[1] = box[mine][1];
      bi[2] = box[mine][2];
      bi[3] = box[mine][3];
    }
    bool hit = false;
    // kept boxes of earlier blocks, 64 at a time: one gather, then lane t's box against every lane
    for (int j0 = 0; j0 < nk; j0 += 64) {
      const int cnt = nk - j0 < 64 ? nk - j0 : 64;
      const int kj = lane < cnt ? kept[j0 + lane] : 0;  // (box 0 always exists)
      const long long g0 = box[kj][0], g1 = box[kj][1], g2 = box[kj][2], g3 = box[kj][3];
      for (int t = 0; t < cnt; ++t) {
        const long long bj[4] = {readlane_i64(g0, t), readlane_i64(g1, t), readlane_i64(g2, t), readlane_i64(g3, t)};
        if (live && iou_gt(bi, bj, iou_thr, zd)) hit = true;
      }
    }
    unsigned long long dropped = (m < 64 ? ~((1ull << m) - 1ull) : 0ull) | __ballot(hit);
    for (int i = 0; i < m; ++i) {
      if ((dropped >> i) & 1ull) continue;  // wave-uniform: candidate i is kept
      const long long bk[4] = {readlane_i64(bi[0], i), readlane_i64(bi[1], i), readlane_i64(bi[2], i),
                               readlane_i64(bi[3], i)};
      const bool h = live && lane > i && iou_gt(bi, bk, iou_thr, zd);
      dropped |= __ballot(h);
    }
    const unsigned long long keep = ~dropped;
    // at most base + m entries after this: below byte 4 (base + 64) <= 8 (base + 64), the next key
    if ((keep >> lane) & 1ull) kept[nk + __popcll(keep & ((1ull << lane) - 1ull))] = mine;
    nk += __popcll(keep);
    wave_lds_fence();  // the list is written before the next block scans it
  }
  return nk;
}

}  // namespace dnnhip
