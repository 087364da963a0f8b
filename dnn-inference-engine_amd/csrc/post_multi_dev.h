// Shared by the multi-scale YOLO decodes (postprocess_multi.hip: everything of an image in one
// workgroup; postprocess_wide.hip: a grid-wide decode kernel, then one NMS workgroup per image):
// what needs a scale table or a class-major key.  What a single-scale decode needs too (the per-box
// arithmetic, BoxStore, key_any, emit_row, bitonic_sort, nms_workgroup, NmsState, nms_any_emit) is
// post_dev.h, included here; those two files call its workgroup helpers with PM_THREADS.  Every
// phase is written ONCE, here or there, templated on the width of the key's index field
// (PC_IDX_BITS in postprocess_multi.hip, PW_IDX_BITS in postprocess_wide.hip) where it matters:
//
//   per box     label_score; ScaleTab / fill_scale_tab (the per-scale parameters in LDS), box_at
//               (global box index -> scale, cell, anchor, values), decode_corners_at /
//               decode_single_at (decode and store), the class-major and merge key layouts
//   phase 3     nms_wave; nms_segments with its state ClassState (per class: waves on tickets, then
//               the long segments by the workgroup)
//   phase 4     gather_kept, merge_single, merge_labels (the in-place expansion and its invariant)
//
// so a box decodes to the same bits and a sorted segment gives the same kept list in either file.
// The host-side checks and the host staging of both files' entries are declared here too
// (postprocess_multi.hip defines them).
#pragma once
#include <type_traits>
#include "post_dev.h"

namespace dnnhip {

int yolo_head_boxes(const dnn_yolo_head* h, const char* who, long long max_boxes);  // postprocess_head.hip

constexpr int PM_THREADS = 1024;
constexpr int PM_CAP = DNN_YOLO_MULTI_MAX_BOXES;  // keys: 16384 x 8 B = 128 KiB; + 640 B of per-scale
                                                  // parameters, 128 B of ballot words, 16 B of counters
constexpr int PM_BOX_BYTES = POST_BOX_BYTES;
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

// ---- host side (postprocess_multi.hip defines the functions) --------------------------------------
// The arguments of a decode entry as its caller gave them (the host form: no workspace).
struct MultiCall {
  const char* who;
  const dnn_yolo_multi* m;
  const float* scale_x_y;  // NULL: every scale 1
  const float* const* pred;
  int n_images;
  dnn_detection* dets;
  int max_det;
  int* counts;
  void* workspace;
  unsigned long long workspace_bytes;
  int nms_mode, labels_mode;
};

// What the two files' entries differ in: their limits, their workspace and their launcher.
struct MultiKind {
  long long max_boxes;
  int max_images;
  unsigned long long (*workspace)(int nb, int n_images);
  int (*launch)(const MultiCall& c, hipStream_t stream);
};

// What check_multi_call makes of a call for the launcher.
struct MultiArgs {
  MultiPred mp;
  XyScale xy;
  int nb;  // boxes of one image over all scales
};

// < 0 with the error set, else the boxes of one image over all scales (at most max_boxes)
int multi_boxes_upto(const dnn_yolo_multi* m, const char* who, long long max_boxes);
// each mode a value of its own, and not (any class, multi-label): no rule of any entry
bool multi_modes_ok(int nms_mode, int labels_mode, const char* who);
// Every argument check of a decode entry, in this order: the description (multi_boxes_upto with the
// kind's limit), the modes, scale_x_y (each value finite and > 0), counts and pointers, pred[s], and
// unless `host` the workspace's size and alignment.  < 0 with the error set; 0 with nothing to do
// (no images); 1 with *out filled.
int check_multi_call(const MultiCall& c, const MultiKind& kind, bool host, MultiArgs* out);
// Host pointers, synchronous: checks, allocates the scratch, copies in, kind.launch, copies out.
int yolo_multi_host(const MultiCall& c, const MultiKind& kind);

// Multi-label score of a class from its logit: conf * p[c], one fp32 multiply, p[c] as class_argmax
// computes it (m and sum: the box's logit_max and softmax_sum, unused in logistic mode).  The decode
// and the merge of the multi-label kernels both call this, so an emitted score has the bits it was
// sorted on.
__device__ __forceinline__ float label_score(float logit, bool logistic, float conf, float m, float sum) {
  const float pc = logistic ? sigmoid_ref(logit) : np_expf(logit - m) / sum;
  return conf * pc;
}

// Per-scale parameters of one image in LDS: one 32-byte record a scale, so that a box reads its
// scale's scalars from one place, and the anchors.
struct ScaleRec {
  const float* pred;  // this image's values of the scale
  int off, gw, na;    // the scale's first global box index, its grid width and anchors
  float cell, xs, xb;
};
struct ScaleTab {
  ScaleRec sc[DNN_YOLO_MAX_SCALES];
  float anchors[DNN_YOLO_MAX_SCALES][2 * DNN_YOLO_MAX_ANCHORS];
};

// By the whole workgroup; the caller's next barrier publishes it.  xy NULL: xs, xb stay unset (for a
// kernel that decodes no geometry).
__device__ __forceinline__ void fill_scale_tab(ScaleTab& t, const dnn_yolo_multi& mh, const XyScale* xy,
                                               const MultiPred& pred, int img, int stride, int tid) {
  if (tid == 0) {
    int off = 0;
#pragma unroll
    for (int s = 0; s < DNN_YOLO_MAX_SCALES; ++s) {
      const bool on = s < mh.n_scales;
      const int b = on ? mh.scale[s].grid_h * mh.scale[s].grid_w * mh.scale[s].n_anchors : 0;
      t.sc[s].off = off;
      t.sc[s].gw = on ? mh.scale[s].grid_w : 1;
      t.sc[s].na = on ? mh.scale[s].n_anchors : 1;
      t.sc[s].cell = on ? mh.scale[s].cell : 1.0f;
      t.sc[s].pred = on ? pred.p[s] + (size_t)img * b * stride : nullptr;
      off += b;
    }
  }
  if (xy && tid < DNN_YOLO_MAX_SCALES) {  // (beside thread 0's serial loop, not in it)
    t.sc[tid].xs = xy->s[tid];
    t.sc[tid].xb = xy->b[tid];
  }
  if (tid < 2 * DNN_YOLO_MAX_ANCHORS) {
#pragma unroll
    for (int s = 0; s < DNN_YOLO_MAX_SCALES; ++s) t.anchors[s][tid] = mh.scale[s].anchors[tid];
  }
}

// The scale of global box index k (scale 0's boxes first), and the box's 5 + C values.
__device__ __forceinline__ int scale_of(const ScaleTab& t, int S, int k) {
  int s = 0;
  while (s + 1 < S && k >= t.sc[s + 1].off) ++s;
  return s;
}
__device__ __forceinline__ const float* box_values(const ScaleTab& t, int s, int k, int stride) {
  return t.sc[s].pred + (size_t)(k - t.sc[s].off) * stride;
}

// Where global box index k sits: its scale, cell and anchor (a scale's boxes are in row, col, anchor
// order) and its values q.
struct BoxAt {
  int s, row, col, b;
  const float* q;
};
__device__ __forceinline__ BoxAt box_at(const ScaleTab& t, int S, int k, int stride) {
  BoxAt at;
  at.s = scale_of(t, S, k);
  const ScaleRec& sc = t.sc[at.s];
  const int kk = k - sc.off, A = sc.na, gw = sc.gw, cell = kk / A;
  at.b = kk % A;
  at.col = cell % gw;
  at.row = cell / gw;
  at.q = sc.pred + (size_t)kk * stride;
  return at;
}

// decode_corners of the box at `at`, the corners stored as box k; a bad corner sets *bad (before
// the stores, as these kernels always had it: after them the compiler splits the stores over the
// two outcomes).
__device__ __forceinline__ void decode_corners_at(const ScaleTab& t, const BoxAt& at, const BoxStore& bs, int k,
                                                  float* conf, int* bad) {
  long long c4[4];
  if (!decode_corners(at.q, at.b, at.col, at.row, t.anchors[at.s], t.sc[at.s].cell, t.sc[at.s].xs, t.sc[at.s].xb, c4, conf))
    *bad = 1;
  bs.box[k][0] = c4[0];
  bs.box[k][1] = c4[1];
  bs.box[k][2] = c4[2];
  bs.box[k][3] = c4[3];
}

// One box with ONE label: decode_corners, the arg-max class and the score conf * p(class), all
// stored as box k; a bad corner sets *bad.  The stores come after the class loop, as they always
// did in these kernels.
__device__ __forceinline__ void decode_single_at(const ScaleTab& t, const BoxAt& at, int C, bool logistic,
                                                 const BoxStore& bs, int k, float* score, int* cls, int* bad) {
  long long c4[4];
  float conf;
  if (!decode_corners(at.q, at.b, at.col, at.row, t.anchors[at.s], t.sc[at.s].cell, t.sc[at.s].xs, t.sc[at.s].xb, c4, &conf))
    *bad = 1;
  *score = conf * class_argmax(at.q + 5, C, logistic, cls);
  bs.box[k][0] = c4[0];
  bs.box[k][1] = c4[1];
  bs.box[k][2] = c4[2];
  bs.box[k][3] = c4[3];
  bs.score[k] = *score;
  bs.cls[k] = *cls;
}

// The sort keys beside key_any (post_dev.h: ~score (32) | index (32), the class-agnostic key and the
// single-label merge's), with the same ~bits rule; every candidate's key stays below the padding ~0ull.
constexpr int PC_CLS_BITS = 7;
constexpr int PC_IDX_BITS = 14;  // postprocess_multi.hip: up to DNN_YOLO_MULTI_MAX_BOXES boxes
constexpr int PW_IDX_BITS = 16;  // postprocess_wide.hip: up to DNN_YOLO_WIDE_MAX_BOXES
static_assert(DNN_YOLO_MAX_CLASSES <= (1 << PC_CLS_BITS), "the class does not fit its key field");
static_assert(DNN_YOLO_MULTI_MAX_BOXES <= (1 << PC_IDX_BITS) && DNN_YOLO_WIDE_MAX_BOXES <= (1 << PW_IDX_BITS),
              "the global box index does not fit its key field");
static_assert(PC_CLS_BITS + 32 + PC_IDX_BITS < 64 && PC_CLS_BITS + 32 + PW_IDX_BITS < 64,
              "a candidate's key must stay below ~0ull");
static_assert(PC_CLS_BITS + PC_IDX_BITS < 31 && PC_CLS_BITS + PW_IDX_BITS < 31, "a kept entry (index | class) is an int");

// class-major, what the per-class NMS sorts: class (7) | ~score (32) | index (IDX_BITS)
template <int IDX_BITS>
__device__ __forceinline__ unsigned long long key_class(int c, float sc, int k) {
  return ((unsigned long long)c << (32 + IDX_BITS)) | ((unsigned long long)(~__float_as_uint(sc)) << IDX_BITS) |
         (unsigned)k;
}
template <int IDX_BITS>
__device__ __forceinline__ int key_class_class(unsigned long long key) {
  return (int)(key >> (32 + IDX_BITS));
}

// multi-label merge: ~score (32) | index (IDX_BITS) | class (7)
template <int IDX_BITS>
__device__ __forceinline__ unsigned long long key_merge(float sc, int k, int c) {
  return ((unsigned long long)(~__float_as_uint(sc)) << (IDX_BITS + PC_CLS_BITS)) |
         ((unsigned long long)k << PC_CLS_BITS) | (unsigned)c;
}
template <int IDX_BITS>
__device__ __forceinline__ float key_merge_score(unsigned long long key) {
  return __uint_as_float(~(unsigned)(key >> (IDX_BITS + PC_CLS_BITS)));
}
template <int IDX_BITS>
__device__ __forceinline__ int key_merge_index(unsigned long long key) {
  return (int)(key >> PC_CLS_BITS) & ((1 << IDX_BITS) - 1);
}
__device__ __forceinline__ int key_merge_class(unsigned long long key) { return (int)key & ((1 << PC_CLS_BITS) - 1); }

// Candidates of one class above which the whole workgroup takes the segment.  A wave alone pays for
// every kept box of its segment itself, so long chains are cheaper split over 16 waves even with
// two barriers per block: measured at 256, 1024 and 4096, 256 was never slower.
constexpr int PC_BIG = 256;
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

// ---- the NMS state of a per-class kernel in LDS (NmsState with the class segments): declared
// __shared__ there, passed by reference ------------------------------------------------------------
struct ClassState : NmsState {
  int cls_cnt[DNN_YOLO_MAX_CLASSES];        // candidates per class
  int seg_start[DNN_YOLO_MAX_CLASSES + 1];  // their prefix sum: class c is keys[seg_start[c] .. seg_start[c+1])
  int seg_kept[DNN_YOLO_MAX_CLASSES];       // kept per class
  int out_off[DNN_YOLO_MAX_CLASSES + 1];    // their prefix sum
  int ticket;
};

// By the whole workgroup; the caller's next barrier publishes it.
__device__ __forceinline__ void reset_state(ClassState& st, int tid) {
  reset_state(static_cast<NmsState&>(st), tid);
  if (tid == 0) st.ticket = 0;
  if (tid < DNN_YOLO_MAX_CLASSES) {
    st.cls_cnt[tid] = 0;
    st.seg_kept[tid] = 0;
  }
}

// Phase 3 of the per-class rule on the class-major sorted keys (key_class<IDX_BITS>; st.seg_start
// published, st.seg_kept, n_kept and ticket 0).  3a: waves draw classes from the ticket and run
// nms_wave on a segment ALONE, no barrier inside, nobody waits; segments longer than PC_BIG are
// left to 3b, where the whole workgroup runs nms_workgroup on each of them in turn.  Each kept list
// goes in place over its own segment.  Returns the number kept over all classes, st.out_off the
// prefix sum of the list lengths; -1 when an IoU denominator was zero.
template <int IDX_BITS>
__device__ __forceinline__ int nms_segments(unsigned long long* keys, int C, const long long (*box)[4],
                                            double iou_thr, ClassState& st, int tid) {
  const int lane = tid & 63, wid = tid >> 6;
  {
    bool zd = false;
    for (;;) {
      int c = 0;
      if (lane == 0) c = atomicAdd(&st.ticket, 1);
      c = __builtin_amdgcn_readfirstlane(c);  // lane 0's ticket, in a scalar register
      if (c >= C) break;
      const int s0 = __builtin_amdgcn_readfirstlane(st.seg_start[c]);
      const int len = __builtin_amdgcn_readfirstlane(st.seg_start[c + 1]) - s0;
      if (len == 0 || len > PC_BIG) continue;
      const int nk = nms_wave<IDX_BITS>(keys + s0, len, box, iou_thr, lane, &zd);
      if (lane == 0) st.seg_kept[c] = nk;
    }
    if (__any(zd) && lane == 0) st.zero_den = 1;
  }
  __syncthreads();
  for (int c = 0; c < C; ++c) {  // (n_kept is 0 here)
    const int s0 = __builtin_amdgcn_readfirstlane(st.seg_start[c]);
    const int len = __builtin_amdgcn_readfirstlane(st.seg_start[c + 1]) - s0;
    if (len <= PC_BIG) continue;  // workgroup-uniform
    nms_workgroup<IDX_BITS, PM_THREADS>(keys + s0, len, box, iou_thr, st.hitw, &st.n_kept, &st.zero_den, lane, wid);
    if (tid == 0) {
      st.seg_kept[c] = st.n_kept;
      st.n_kept = 0;
    }
    __syncthreads();
  }
  if (wid == 0) wave_scan_128(st.seg_kept, C, st.out_off, lane);
  __syncthreads();
  return st.zero_den ? -1 : st.out_off[DNN_YOLO_MAX_CLASSES];
}

// Phase 4, first half: the nk entries of the concatenated kept lists into registers, mine[i] the
// entry at position tid + 1024 i (its class found by a search in st.out_off), as the box index or
// WITH_CLASS as index | class << IDX_BITS.  After the closing barrier the keys may be overwritten.
template <int IDX_BITS, bool WITH_CLASS>
__device__ __forceinline__ void gather_kept(const unsigned long long* keys, int C, int nk, const ClassState& st,
                                            int (&mine)[16], int tid) {
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int p = tid + i * PM_THREADS;
    mine[i] = 0;
    if (p < nk) {
      int lo = 0, hi = C;  // the class with out_off[lo] <= p < out_off[lo + 1]
      while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (st.out_off[mid] <= p) lo = mid;
        else hi = mid;
      }
      mine[i] = reinterpret_cast<const int*>(keys + st.seg_start[lo])[p - st.out_off[lo]];
      if (WITH_CLASS) mine[i] |= lo << IDX_BITS;
    }
  }
  __syncthreads();
}

// Phase 4 with one label a box: the gathered box indices (no class) back as dense key_any keys,
// sorted over pow2 >= nk by (score descending, global index), the first max_det emitted.
__device__ __forceinline__ void merge_single(unsigned long long* keys, const int (&mine)[16], int nk, const BoxStore& bs,
                                             dnn_detection* rows, int max_det, int* count, int tid) {
  int ns2 = 1;
  while (ns2 < nk) ns2 <<= 1;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int p = tid + i * PM_THREADS;
    if (p < nk)
      keys[p] = key_any(bs.score[mine[i]], mine[i]);
    else if (p < ns2)
      keys[p] = ~0ull;
  }
  __syncthreads();
  bitonic_sort<PM_THREADS>(keys, ns2, tid);
  const int nw = nk < max_det ? nk : max_det;
  for (int r = tid; r < nw; r += PM_THREADS) {
    const int k = key_any_index(keys[r]);
    emit_row(rows + r, bs.cls[k], bs.score[k], bs.box[k]);
  }
  if (tid == 0) *count = nk;
}

// Phase 4 with multi-label detections: a kept entry's class is its segment, and its score is not
// stored (the workspace keeps a box's conf and sum), so the gathered entries (index | class <<
// IDX_BITS) go back as a DENSE int list at the start of the key array, which is expanded IN PLACE
// into the merge keys (key_merge<IDX_BITS>) from the top chunk of 1024 down.  The invariant: chunk j
// reads ints [1024 j, 1024 j + 1024) before a barrier and writes bytes [8192 j, 8192 j + 8192) =
// ints [2048 j, 2048 j + 2048) after it: at or above every int of the chunks below, which are the
// only ones still unread.  The padding of the sort starts at byte 8 nk, above the whole list.  The
// score is recomputed by label_score from the stored conf (and sum) and the box's logits, the bits
// it was sorted on.  Sorted by (score descending, global index, class), the first max_det emitted.
template <int IDX_BITS>
__device__ __forceinline__ void merge_labels(unsigned long long* keys, const int (&mine)[16], int nk, const ScaleTab& t,
                                             int S, int C, int stride, bool logistic, const BoxStore& bs,
                                             dnn_detection* rows, int max_det, int* count, int tid) {
  int* dense = reinterpret_cast<int*>(keys);
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int p = tid + i * PM_THREADS;
    if (p < nk) dense[p] = mine[i];
  }
  int ns2 = 1;
  while (ns2 < nk) ns2 <<= 1;
  for (int p = nk + tid; p < ns2; p += PM_THREADS) keys[p] = ~0ull;
  __syncthreads();
  for (int j = (nk - 1) / PM_THREADS; j >= 0; --j) {  // workgroup-uniform
    const int p = tid + j * PM_THREADS;
    unsigned long long key = 0;
    if (p < nk) {
      const int e = dense[p], k = e & ((1 << IDX_BITS) - 1), c = e >> IDX_BITS;
      const float* lg = box_values(t, scale_of(t, S, k), k, stride) + 5;
      const float sum = logistic ? 1.0f : bs.sum()[k];
      const float sc = label_score(lg[c], logistic, bs.score[k], logistic ? 0.0f : logit_max(lg, C), sum);
      key = key_merge<IDX_BITS>(sc, k, c);
    }
    __syncthreads();
    if (p < nk) keys[p] = key;
  }
  __syncthreads();
  bitonic_sort<PM_THREADS>(keys, ns2, tid);
  const int nw = nk < max_det ? nk : max_det;
  for (int r = tid; r < nw; r += PM_THREADS) {
    const unsigned long long key = keys[r];
    emit_row(rows + r, key_merge_class(key), key_merge_score<IDX_BITS>(key), bs.box[key_merge_index<IDX_BITS>(key)]);
  }
  if (tid == 0) *count = nk;
}

}  // namespace dnnhip
