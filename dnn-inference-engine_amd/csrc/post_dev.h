// Device helpers of every YOLO decode, single-scale or multi-scale: what does not depend on there
// being several scales is written ONCE here, so a box decodes to the same bits and a sorted list of
// candidates gives the same kept list in every kernel.  The helpers that run a whole workgroup take
// its thread count as a template parameter.
//
//   per box     decode_corners, class_argmax, logit_max; BoxStore / box_store (an image's boxes, in
//               the workspace or in LDS); key_any / key_any_index; emit_row; VOC_ANCHORS
//   phase 2     bitonic_sort<THREADS>
//   phase 3     nms_workgroup<IDX_BITS, THREADS> with its state NmsState / reset_state;
//               nms_any_emit<THREADS> (the class-agnostic rule from the sort through the emit)
//
// Who uses what:
//   postprocess.hip        (845 boxes, 512 threads)  key_any, bitonic_sort, emit_row, VOC_ANCHORS; its
//                          softmax, its NMS bitmask and a copy of decode_corners' arithmetic are
//                          its own
//   postprocess_head.hip   (any head, 512 threads)   decode_corners, class_argmax, key_any, box_store,
//                          nms_any_emit; VOC_ANCHORS on the host
//   post_multi_dev.h       (1024 threads) includes this header and adds what needs a scale table or a
//                          class-major key, for postprocess_multi.hip and postprocess_wide.hip
// The host staging of the two single-scale host entries is declared here too (postprocess.hip
// defines it).
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>
#include "dnn_common.h"
#include "post_math.h"
#include "../../include/dnn_hip_post.h"

namespace dnnhip {

// ---- host side (postprocess.hip defines the function) ---------------------------------------------
// Host pointers, synchronous, for a decode that reads ONE prediction tensor: one allocation holding
// the predictions, the detections, the counts and the workspace (detections and workspace 8-byte
// aligned), copy in, `launch` on the device copies (ws NULL when ws_bytes is 0), copy out; the
// allocation is freed on every path.  0, -1 with the error set (c.who names the entry), or what
// `launch` returned.
struct SingleCall {  // what the entry's launcher needs beside the device copies
  const char* who;
  const dnn_yolo_head* head;  // NULL: the 13 x 13 kernel
  int n_images, max_det;
  size_t ws_bytes;
};
typedef int (*SingleLaunch)(const SingleCall& c, const float* pred, dnn_detection* dets, int* counts, void* ws);
int yolo_single_host(const SingleCall& c, const float* pred, size_t pred_bytes, dnn_detection* dets, size_t det_bytes,
                     int* counts, size_t count_bytes, SingleLaunch launch);

// The anchors of the VOC YOLOv2-tiny head (yolov2tiny.py:116): the 845-box kernel's, and what
// dnn_yolo_head_voc fills in.
constexpr float VOC_ANCHORS[10] = {1.08f, 1.19f, 3.42f, 4.41f, 6.63f, 11.38f, 9.42f, 5.11f, 16.62f, 10.52f};

// Geometry and objectness of one box of one scale (q: its 5 + C values; b, col, row: its anchor and
// cell): corners truncated to int64 in out[0..3] (false when one is not finite or out of range) and
// conf = sigmoid(q[4]).  xs, xb: Darknet's scale_x_y as a pair, one fp32 multiply then one fp32 add
// (the files are built without contraction); 1.0f, -0.0f where there is none: sig * 1.0f + -0.0f is
// sig bit for bit for every non-NaN sig.  Shared by all kernels so that they round alike.
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

// The largest class logit of a box, the softmax's shift (class_argmax's loop).
__device__ __forceinline__ float logit_max(const float* lg, int C) {
  float m = lg[0];
  for (int c = 1; c < C; ++c) m = lg[c] > m ? lg[c] : m;
  return m;
}

// The boxes of one image, POST_BOX_BYTES a box.  In a workspace (box_store): nb x 4 corners, then a
// plane of nb floats and a plane of nb ints.  Single-label kernels keep the score and the class
// there; the multi-label ones the conf and, in softmax mode, the box's sum (sum()).
constexpr int POST_BOX_BYTES = 40;  // 4 x int64 corners + fp32 score + int class
struct BoxStore {
  long long (*box)[4];
  float* score;
  int* cls;
  __device__ __forceinline__ float* sum() const { return reinterpret_cast<float*>(cls); }
};
__device__ __forceinline__ BoxStore box_store(char* w, int nb) {
  return {reinterpret_cast<long long (*)[4]>(w), reinterpret_cast<float*>(w + (size_t)nb * 32),
          reinterpret_cast<int*>(w + (size_t)nb * 36)};
}

// The class-agnostic sort key: ~score (32) | index (32).  A score above score_thr >= 0 is positive,
// so larger float bits are a larger score and ~bits sorts descending; every candidate's key stays
// below the padding ~0ull.
__device__ __forceinline__ unsigned long long key_any(float sc, int k) {
  return ((unsigned long long)(~__float_as_uint(sc)) << 32) | (unsigned)k;
}
__device__ __forceinline__ int key_any_index(unsigned long long key) { return (int)(key & 0xffffffffu); }

// The one place that writes a detection.
__device__ __forceinline__ void emit_row(dnn_detection* row, int cls, float score, const long long* corners) {
  dnn_detection d;
  d.cls = cls;
  d.score = score;
  d.left = corners[0];
  d.top = corners[1];
  d.right = corners[2];
  d.bottom = corners[3];
  *row = d;
}

// Bitonic sort of keys[0 .. ns) (ns a power of two) by the whole workgroup of THREADS, ascending.
template <int THREADS>
__device__ __forceinline__ void bitonic_sort(unsigned long long* keys, int ns, int tid) {
  for (int kk = 2; kk <= ns; kk <<= 1) {
    for (int j = kk >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < ns; i += THREADS) {
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

// The state of nms_workgroup in LDS: declared __shared__ in the kernel, passed by reference.
constexpr int POST_MAX_WAVES = 16;  // of a workgroup: 1024 threads
struct NmsState {
  unsigned long long hitw[POST_MAX_WAVES];
  int n_kept, zero_den;
};

// By the whole workgroup; the caller's next barrier publishes it.
__device__ __forceinline__ void reset_state(NmsState& st, int tid) {
  if (tid == 0) {
    st.n_kept = 0;
    st.zero_den = 0;
  }
}

// Blocked greedy NMS of the n sorted candidates seg[0 .. n) by the whole workgroup of THREADS (every
// thread calls it; *n_kept == 0 on entry, published by a barrier), 64 candidates at a time.  All waves
// test the block (lane = candidate) against the boxes kept from earlier blocks (wave w takes kept
// entries w, w + waves, ...) and ballot one word each; then wave 0 resolves the 64 x 64 triangle
// inside the block in order and appends the survivors.  Two barriers per block.  A zero IoU
// denominator counts for every pair (candidate, kept box before it), dropped candidates included: the
// reference tests every candidate against the whole kept list without early exit
// (yolov2tiny.py:210-225).  The box index is the key's low IDX_BITS bits.
// The kept list (int box indices) is written IN PLACE over seg, the keys that the NMS has already
// consumed: after the block starting at candidate `base` the list has at most base + 64 entries, below
// byte 4 (base + 64) of seg, and the first key still to be read sits at byte 8 (base + 64).  Inside a
// block every key of the block is read into registers (one per lane) before the first barrier and
// the list grows only after it.  *n_kept is the list's length after the closing barrier.
template <int IDX_BITS, int THREADS>
__device__ __forceinline__ void nms_workgroup(unsigned long long* seg, int n, const long long (*box)[4],
                                              double iou_thr, unsigned long long* hitw, int* n_kept, int* zero_den,
                                              int lane, int wid) {
  constexpr int WAVES = THREADS / 64;
  // i below is wave-uniform, so a kept candidate's index can be read into a scalar register: its
  // box and its share of the IoU then stay in scalar instructions.  The 1024-thread kernels keep the
  // shuffle they were measured with (DESIGN.md section 9 has the change as a step of its own).
  constexpr bool SCALAR_INDEX = THREADS != 1024;
  static_assert(THREADS % 64 == 0 && WAVES <= POST_MAX_WAVES, "whole waves, a ballot word of NmsState each");
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
    for (int j = wid; j < nk; j += WAVES) {
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
      for (int wv = 0; wv < WAVES; ++wv) dropped |= hitw[wv];
      bool zt = false;
      for (int i = 0; i < m; ++i) {
        if ((dropped >> i) & 1ull) continue;  // wave-uniform: candidate i is kept
        // (no key is read here: the list below overwrites them)
        const int ki = SCALAR_INDEX ? __builtin_amdgcn_readlane(mine, i) : __shfl(mine, i);
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

// Phases 2 and 3 of the class-agnostic rule, and the emit, by the whole workgroup of THREADS: sorts
// the n candidates of keys (key_any, padded with ~0ull to pow2 >= n), runs nms_workgroup and writes
// the first max_det kept boxes to rows and their number (-2: a zero IoU denominator) to *count.
template <int THREADS>
__device__ __forceinline__ void nms_any_emit(unsigned long long* keys, int n, const BoxStore& bs, double iou_thr,
                                             NmsState& st, dnn_detection* rows, int max_det, int* count, int tid) {
  int ns = 1;
  while (ns < n) ns <<= 1;
  bitonic_sort<THREADS>(keys, ns, tid);
  nms_workgroup<32, THREADS>(keys, n, bs.box, iou_thr, st.hitw, &st.n_kept, &st.zero_den, tid & 63, tid >> 6);
  if (st.zero_den) {
    if (tid == 0) *count = -2;
    return;
  }
  const int* kept = reinterpret_cast<const int*>(keys);  // in place over the consumed keys
  const int nk = st.n_kept, nw = nk < max_det ? nk : max_det;
  for (int r = tid; r < nw; r += THREADS) {
    const int k = kept[r];
    emit_row(rows + r, bs.cls[k], bs.score[k], bs.box[k]);
  }
  if (tid == 0) *count = nk;
}

}  // namespace dnnhip
