// Anchor-free YOLO heads with distribution-focal-loss boxes (YOLOv8, YOLO11; include/dnn_hip_post.h:
// dnn_yolo_dfl).  A grid point has 4 * R box logits (R = reg_max bins for each of the sides left, top,
// right, bottom) followed by C class logits, NHWC, so a point's channels are one contiguous run of
// 4 R + C floats.  There is no objectness to gate on: every class of every point is scored, and a box
// is decoded only where a score passed.  Three launches on the stream:
//
//   yolo_dfl_clear_kernel   zeroes the per-image counter blocks (a kernel, not a memset node:
//                           postprocess_wide.hip has the reason).
//   yolo_dfl_decode_kernel  grid (chunk of PD_THREADS points, image), 4 waves, a WAVE owns 64 consecutive
//                           points of the global point order and runs two passes over them:
//     class pass, all 64 points.  Two points a step, one per 32-lane HALF of the wave, so the lanes run
//       over a point's classes and a load is a contiguous run of its channels.  VEC (C % 4 == 0 and
//       16-byte aligned tensors): lane j of the half loads the 16 bytes of classes 4 j .. 4 j + 3, else
//       the four floats of classes j, j + 32, j + 64, j + 96; either way a lane holds at most 4 classes,
//       in ascending order.  The next step's loads are issued before this step is scored.  A class is
//       scored by sigmoid_ref (a double exp2) only if the hardware exp puts it within 0.1 % of the
//       threshold or above (pre-gate, below): the others cannot be candidates, and cannot be the
//       arg-max of a candidate.  Arg-max: a lane's best (p, class), then the xor butterfly 16, 8, 4, 2, 1
//       inside the half with (larger p, then lower class), which is the first index of the largest
//       rounded p whatever the lanes' order; the result goes to the lane whose number is the point's, so
//       after the pass lane l holds point l's score and class and ONE ballot compacts the wave's
//       candidates: one atomic per wave on the image's counter, the keys to the image's list in global
//       memory (post_multi_dev.h: wave_append, the keys of the wide decode).  Multi-label: every lane
//       appends its classes above the threshold as (point, class) keys, one ballot per class slot, and
//       a ballot per half marks the point as a survivor.
//     distance pass, the survivors only (typically a few percent).  The whole wave takes one survivor:
//       lane l holds bin l % 16 of side l / 16 (one 256-byte load for R = 16; for R < 16 the lanes
//       l % 16 >= R are masked: -inf for the max, 0 for the sums).  Row max by the xor butterfly 8, 4, 2,
//       1 (a max does not depend on the order).  The two SUMS of a side, sum_k e[k] and sum_k p[k] * k,
//       are defined ascending in k, so they are not butterflies: lane k of a row adds its term to the
//       running sum of lane k - 1, fetched by a DPP row_shr:1, in step k of 15 steps, and lane 15 ends
//       with ((v0 + v1) + v2) + ... + v15 (masked lanes add 0.0f, which changes no bit).  No LDS.  The
//       four d's are read from lanes 15, 31, 47, 63 into scalars, the corners are computed and truncated
//       by the shared trunc_i64 and lane 0 stores them as box k of the workspace; a bad corner sets the
//       image's flag.
//   yolo_dfl_nms_kernel     one workgroup of 1024 per image: -1, then -3, else the keys to LDS, the sort,
//                           the NMS and the merges of post_multi_dev.h / post_dev.h, the very calls of
//                           postprocess_wide.hip's NMS kernel.
//
// The shared phases read a box's class logits at box_values() + 5 and a multi-label score as
// conf * p[c]: the scale table here points 4 R - 5 floats into a point's channels, so that + 5 is its
// first class logit, and a survivor's stored conf is 1.0f (1.0f * p is p, bit for bit).
//
// Pre-gate.  A class is skipped iff E = __expf(-x) > 1 / (0.999f * score_thr) - 1, computed once in fp32.
// E is within 1e-5 of e ** -x for |x| < 88 (v_exp_f32 is 1 ulp; the argument product rounds once), so
// 1 / (1 + e ** -x) < 0.999 (1 + 2e-5) score_thr, and sigmoid_ref, correct to 3 ulp, is below score_thr.  A NaN
// fails the comparison and is scored; score_thr == 0 makes the bound +inf and every class is scored.
//
// Orders.  Keys are unique (point index, and class in multi-label mode) and sorted before use, so the order
// of the appends does not matter; a side's sums have the one order above; an image's rows are a function of
// its own tensors alone, the same bits at every batch size and place in the batch.
//
// Budget.  Decode: 640 B of LDS (the scale table), no barriers after the first; a lane holds 2 x 4 logits, a
// pointer, (row, col, scale), a score and a class, and sigmoid_ref's double exp2 takes the rest: 66 to 74
// VGPRs, six waves a SIMD.  NMS: 128 KiB of keys + the table + ClassState, as postprocess_wide.hip.
#include <cfloat>
#include "post_dfl_host.h"

namespace dnnhip {

typedef float dfl_f32x4 __attribute__((ext_vector_type(4)));

constexpr int PD_THREADS = 256;  // 4 waves of 64 points
constexpr int PD_ANY = 0, PD_PER_CLASS = 1, PD_MULTI = 2;
static_assert(DNN_YOLO_DFL_MAX_REG == 16, "a side's bins are one 16-lane DPP row");
static_assert(DNN_YOLO_MAX_CLASSES <= 4 * 32, "a lane of a half holds at most 4 classes");
static_assert(4 * DNN_YOLO_DFL_MIN_REG >= 5, "the scale table points 4 R - 5 floats into a point");

__device__ __forceinline__ int dfl_channels(const dnn_yolo_dfl& h) { return 4 * h.reg_max + h.n_classes; }

// The scale table of post_multi_dev.h for a DFL head (one "anchor" per cell, cell = stride); pred points
// 4 R - 5 floats into the image's first point (see the top of the file).  By thread 0; the caller's next
// barrier publishes it.
__device__ __forceinline__ void fill_dfl_tab(ScaleTab& t, const dnn_yolo_dfl& h, const MultiPred& pred, int img,
                                             int tid) {
  if (tid != 0) return;
  const int ch = dfl_channels(h);
  int off = 0;
#pragma unroll
  for (int s = 0; s < DNN_YOLO_MAX_SCALES; ++s) {
    const bool on = s < h.n_scales;
    const int b = on ? h.scale[s].grid_h * h.scale[s].grid_w : 0;
    t.sc[s].off = off;
    t.sc[s].gw = on ? h.scale[s].grid_w : 1;
    t.sc[s].na = 1;
    t.sc[s].cell = on ? h.scale[s].stride : 1.0f;
    t.sc[s].xs = 1.0f;
    t.sc[s].xb = -0.0f;
    t.sc[s].pred = on ? pred.p[s] + (size_t)img * b * ch + (4 * h.reg_max - 5) : nullptr;
    off += b;
  }
}

__device__ __forceinline__ const float* shfl_ptr(const float* p, int src) {
  const unsigned long long v = reinterpret_cast<unsigned long long>(p);
  const unsigned lo = __shfl((unsigned)v, src), hi = __shfl((unsigned)(v >> 32), src);
  return reinterpret_cast<const float*>(((unsigned long long)hi << 32) | lo);
}

__device__ __forceinline__ float readlane_f32(float v, int l) {  // l: a constant
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}

// ((v[0] + v[1]) + v[2]) + ... + v[15] over the 16 lanes of a DPP row (kk: the lane's place in its row), in
// lane 15 of the row: in step j lane j adds its v to lane j - 1's running sum.
__device__ __forceinline__ float row_sum_ascending(float v, int kk) {
  float acc = v;
#pragma unroll
  for (int j = 1; j < 16; ++j) {
    const float prev = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(acc), 0x111 /* row_shr:1 */, 0xf,
                                                                  0xf, true));
    if (kk == j) acc = prev + v;
  }
  return acc;
}

// The logits of a half's point that this lane holds (ok: the class exists and the point is inside the image).
struct DflLogits {
  float x[4];
  bool ok[4];
};
template <bool VEC>
__device__ __forceinline__ int dfl_class(int j, int v) {
  return VEC ? 4 * j + v : j + 32 * v;
}
template <bool VEC>
__device__ __forceinline__ DflLogits dfl_load(const float* cls, bool in, int j, int C) {
  DflLogits r;
#pragma unroll
  for (int v = 0; v < 4; ++v) {
    r.ok[v] = in && dfl_class<VEC>(j, v) < C;
    r.x[v] = 0.0f;
  }
  if (VEC) {
    if (r.ok[0]) {  // C % 4 == 0: all four or none
      const dfl_f32x4 q = *reinterpret_cast<const dfl_f32x4*>(cls + 4 * j);
      r.x[0] = q.x;
      r.x[1] = q.y;
      r.x[2] = q.z;
      r.x[3] = q.w;
    }
  } else {
#pragma unroll
    for (int v = 0; v < 4; ++v)
      if (r.ok[v]) r.x[v] = cls[j + 32 * v];
  }
  return r;
}

__global__ void __launch_bounds__(PD_THREADS) yolo_dfl_clear_kernel(int* counters, int n_ints) {
  const int i = blockIdx.x * PD_THREADS + threadIdx.x;
  if (i < n_ints) counters[i] = 0;
}

template <int MODE, bool VEC>
__global__ void __launch_bounds__(PD_THREADS)
yolo_dfl_decode_kernel(const dnn_yolo_dfl h, const MultiPred pred, char* workspace, int nb, int n_images) {
  __shared__ ScaleTab t;
  const int img = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
  const int S = h.n_scales, C = h.n_classes, R = h.reg_max, ch = 4 * R + C;
  const float score_thr = h.score_thr;
  const float skip_above = 1.0f / (0.999f * score_thr) - 1.0f;  // the pre-gate's bound on __expf(-x)

  int* ctr = ws_counters(workspace, img);
  const BoxStore bs = box_store(ws_boxes(workspace, img, nb, n_images), nb);
  unsigned long long* keys = ws_keys(workspace, img, nb, n_images);

  fill_dfl_tab(t, h, pred, img, tid);
  __syncthreads();

  const int k0 = blockIdx.x * PD_THREADS + (tid & ~63);  // the wave's first point
  if (k0 >= nb) return;                                  // wave-uniform; no barrier follows
  const int k = k0 + lane;
  const bool in = k < nb;
  const BoxAt at = box_at(t, S, in ? k : k0, ch);  // lane l: point l (s, row, col; q + 5: its class logits)
  const float* my_cls = at.q + 5;

  // ---- class pass: two points a step, the half hf's lanes over the classes of point k0 + 2 it + hf
  const int hf = lane >> 5, j = lane & 31;
  const int steps = ((nb - k0 < 64 ? nb - k0 : 64) + 1) >> 1;
  float sc = -1.0f;  // single-label modes: lane l's point's score and class
  int best = 0;
  unsigned long long surv = 0;  // multi-label: the points with a candidate (wave-uniform)
  DflLogits cur = dfl_load<VEC>(shfl_ptr(my_cls, hf), k0 + hf < nb, j, C);
  for (int it = 0; it < steps; ++it) {
    const int src = 2 * it + hf;
    DflLogits nxt = cur;
    if (it + 1 < steps) nxt = dfl_load<VEC>(shfl_ptr(my_cls, src + 2), k0 + src + 2 < nb, j, C);
    bool maybe[4];
#pragma unroll
    for (int v = 0; v < 4; ++v) maybe[v] = cur.ok[v] && !(__expf(-cur.x[v]) > skip_above);

    if (MODE == PD_MULTI) {
      bool any = false;
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const float p = maybe[v] ? label_score(cur.x[v], true, 1.0f, 0.0f, 1.0f) : 0.0f;  // what merge_labels recomputes
        const bool want = maybe[v] && p > score_thr;
        any |= want;
        const int pos = wave_append(ctr, want, lane);
        if (pos >= 0 && pos < PM_CAP)  // beyond it only the count matters: the image ends with -3
          keys[pos] = key_class<PW_IDX_BITS>(dfl_class<VEC>(j, v), p, k0 + src);
      }
      const unsigned long long m = __ballot(any);
      if (m & 0xffffffffull) surv |= 1ull << (2 * it);
      if (m >> 32) surv |= 1ull << (2 * it + 1);
    } else {
      float bp = -1.0f;  // below every sigmoid
      int bc = 0x7fffffff;
#pragma unroll
      for (int v = 0; v < 4; ++v) {  // ascending classes: the first index among a lane's equals
        if (!maybe[v]) continue;
        const float p = sigmoid_ref(cur.x[v]);
        if (p > bp) {
          bp = p;
          bc = dfl_class<VEC>(j, v);
        }
      }
#pragma unroll
      for (int d = 16; d >= 1; d >>= 1) {
        const float obp = __shfl_xor(bp, d);
        const int obc = __shfl_xor(bc, d);
        if (obp > bp || (obp == bp && obc < bc)) {
          bp = obp;
          bc = obc;
        }
      }
      // class 0 is lane 0's first value in both layouts; a NaN there is class_argmax's result: no candidate
      const unsigned long long nan0 = __ballot(j == 0 && cur.ok[0] && cur.x[0] != cur.x[0]);
      const float p0 = (nan0 & 1ull) ? -1.0f : readlane_f32(bp, 0);
      const float p1 = (nan0 >> 32 & 1ull) ? -1.0f : readlane_f32(bp, 32);
      const int c0 = __builtin_amdgcn_readlane(bc, 0), c1 = __builtin_amdgcn_readlane(bc, 32);
      if ((lane >> 1) == it) {
        sc = (lane & 1) ? p1 : p0;
        best = (lane & 1) ? c1 : c0;
      }
    }
    cur = nxt;
  }

  // ---- one ballot for the wave's single-label candidates
  unsigned long long todo = surv;
  if (MODE != PD_MULTI) {
    const bool cand = in && sc > score_thr;
    todo = __ballot(cand);
    if (cand) {
      bs.score[k] = sc;
      bs.cls[k] = best;
    }
    const int pos = wave_append(ctr, cand, lane);
    if (pos >= 0 && pos < PM_CAP) keys[pos] = MODE == PD_ANY ? key_any(sc, k) : key_class<PW_IDX_BITS>(best, sc, k);
  }

  // ---- distance pass: the whole wave on one survivor at a time, lane l = bin l % 16 of side l / 16
  const int side = lane >> 4, kk = lane & 15;
  const bool bin = kk < R;
  while (todo) {  // wave-uniform
    const int g = __ffsll((long long)todo) - 1;
    todo &= todo - 1ull;
    const float* box_logits = shfl_ptr(my_cls, g) - 4 * R;
    const int sg = __shfl(at.s, g);
    const float fx = (float)__shfl(at.col, g) + 0.5f, fy = (float)__shfl(at.row, g) + 0.5f, px = t.sc[sg].cell;

    const float x = bin ? box_logits[side * R + kk] : -__builtin_inff();
    float m = x;
#pragma unroll
    for (int d = 8; d >= 1; d >>= 1) m = fmaxf(m, __shfl_xor(m, d));
    const float e = bin ? np_expf(x - m) : 0.0f;
    const float sum = __shfl(row_sum_ascending(e, kk), lane | 15);
    const float p = e / sum;
    const float dist = row_sum_ascending(bin ? p * (float)kk : 0.0f, kk);
    const float dl = readlane_f32(dist, 15), dt = readlane_f32(dist, 31), dr = readlane_f32(dist, 47),
                db = readlane_f32(dist, 63);
    long long c4[4] = {0, 0, 0, 0};
    const bool ok = trunc_i64((fx - dl) * px, &c4[0]) && trunc_i64((fy - dt) * px, &c4[1]) &&
                    trunc_i64((fx + dr) * px, &c4[2]) && trunc_i64((fy + db) * px, &c4[3]);  // (decode_corners' form)
    if (lane == 0) {
      if (!ok) ctr[1] = 1;
      const int kg = k0 + g;
      bs.box[kg][0] = c4[0];
      bs.box[kg][1] = c4[1];
      bs.box[kg][2] = c4[2];
      bs.box[kg][3] = c4[3];
      if (MODE == PD_MULTI) bs.score[kg] = 1.0f;  // the conf that merge_labels multiplies p[c] by
    }
  }
}

// postprocess_wide.hip's yolo_wide_nms_kernel for this head's description: the same calls in the same order.
template <int MODE>
__global__ void __launch_bounds__(PM_THREADS)
yolo_dfl_nms_kernel(const dnn_yolo_dfl h, const MultiPred pred, dnn_detection* __restrict__ dets, int max_det,
                    int* __restrict__ counts, char* workspace, int nb, int n_images, int* __restrict__ points) {
  __shared__ unsigned long long keys[PM_CAP];
  __shared__ ScaleTab t;  // the multi-label merge reads the class logits again
  __shared__ typename std::conditional<MODE == PD_ANY, NmsState, ClassState>::type st;

  const int img = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int S = h.n_scales, C = h.n_classes;
  const IouRule rule{h.iou_thr};

  const int* ctr = ws_counters(workspace, img);
  const BoxStore bs = box_store(ws_boxes(workspace, img, nb, n_images), nb);
  const unsigned long long* gkeys = ws_keys(workspace, img, nb, n_images);
  dnn_detection* rows = dets + (size_t)img * max_det;
  int* pts = points ? points + (size_t)img * max_det : nullptr;  // row r came from grid point pts[r]

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
  if (MODE == PD_MULTI) fill_dfl_tab(t, h, pred, img, tid);
  __syncthreads();

  int ns = 1;  // the keys into LDS, padded to the power of two that the sort touches
  while (ns < n) ns <<= 1;
  for (int i = tid; i < ns; i += PM_THREADS) {
    const unsigned long long key = i < n ? gkeys[i] : ~0ull;
    keys[i] = key;
    if constexpr (MODE != PD_ANY)
      if (i < n) atomicAdd(&st.cls_cnt[key_class_class<PW_IDX_BITS>(key)], 1);
  }
  __syncthreads();

  if constexpr (MODE == PD_ANY) {
    nms_any_emit<PM_THREADS>(keys, n, bs, rule.thr, st, rows, max_det, &counts[img], tid, pts);
  } else {
    if (wid == 0) wave_scan_128(st.cls_cnt, C, st.seg_start, lane);
    bitonic_sort<PM_THREADS>(keys, ns, tid);
    __syncthreads();  // seg_start too (the sort has no barrier when n <= 1)
    const int nk = nms_segments<PW_IDX_BITS>(keys, C, bs.box, rule, st, tid);
    if (nk < 0) {
      if (tid == 0) counts[img] = -2;
      return;
    }
    int mine[16];
    gather_kept<PW_IDX_BITS, MODE == PD_MULTI>(keys, C, nk, st, mine, tid);
    if (MODE == PD_PER_CLASS)
      merge_single(keys, mine, nk, bs, rows, max_det, &counts[img], tid, pts);
    else
      merge_labels<PW_IDX_BITS>(keys, mine, nk, t, S, C, 4 * h.reg_max + C, true, bs, rows, max_det, &counts[img], tid,
                                pts);
  }
}

// ---- host side -------------------------------------------------------------------------------------
int dfl_boxes(const dnn_yolo_dfl* h, const char* who) {
  DNN_REQUIRE(h, "%s: NULL description", who);
  DNN_REQUIRE(h->n_scales >= 1 && h->n_scales <= DNN_YOLO_MAX_SCALES, "%s: %d scales: need 1..%d", who, h->n_scales,
              DNN_YOLO_MAX_SCALES);
  DNN_REQUIRE(h->n_classes >= 1 && h->n_classes <= DNN_YOLO_MAX_CLASSES, "%s: n_classes %d: need 1..%d", who,
              h->n_classes, DNN_YOLO_MAX_CLASSES);
  DNN_REQUIRE(h->reg_max >= DNN_YOLO_DFL_MIN_REG && h->reg_max <= DNN_YOLO_DFL_MAX_REG, "%s: reg_max %d: need %d..%d",
              who, h->reg_max, DNN_YOLO_DFL_MIN_REG, DNN_YOLO_DFL_MAX_REG);
  DNN_REQUIRE(h->score_thr >= 0.0f && h->iou_thr == h->iou_thr,
              "%s: need score_thr >= 0 (got %g) and iou_thr not NaN (got %g)", who, (double)h->score_thr, h->iou_thr);
  long long total = 0;
  for (int s = 0; s < h->n_scales; ++s) {
    const dnn_yolo_dfl_scale& sc = h->scale[s];
    DNN_REQUIRE(sc.grid_h >= 1 && sc.grid_w >= 1 && sc.grid_h <= DNN_YOLO_WIDE_MAX_BOXES &&
                    sc.grid_w <= DNN_YOLO_WIDE_MAX_BOXES,
                "%s: scale %d: grid %d x %d: need >= 1 cell and at most %d points", who, s, sc.grid_h, sc.grid_w,
                DNN_YOLO_WIDE_MAX_BOXES);
    DNN_REQUIRE(sc.stride > 0.0f && sc.stride <= FLT_MAX, "%s: scale %d: stride %g: need a finite number of pixels > 0",
                who, s, (double)sc.stride);
    total += (long long)sc.grid_h * sc.grid_w;
  }
  DNN_REQUIRE(total <= DNN_YOLO_WIDE_MAX_BOXES, "%s: %lld points over %d scales > %d", who, total, h->n_scales,
              DNN_YOLO_WIDE_MAX_BOXES);
  return (int)total;
}

int check_dfl_call(const DflCall& c, bool host, int* nb, MultiPred* mp) {
  *nb = dfl_boxes(c.h, c.who);
  if (*nb < 0) return *nb;
  if (!multi_modes_ok(c.nms_mode, c.labels_mode, c.who)) return -2;
  DNN_REQUIRE(c.n_images >= 0 && c.max_det >= 0 &&
                  (c.n_images == 0 || (c.pred && c.counts && (c.max_det == 0 || c.dets))),
              "%s: bad arguments (n_images=%d max_det=%d)", c.who, c.n_images, c.max_det);
  if (c.n_images == 0) return 0;
  DNN_REQUIRE(c.n_images <= 65535, "%s: %d images > 65535, the most one launch takes", c.who, c.n_images);
  *mp = MultiPred{};
  for (int s = 0; s < c.h->n_scales; ++s) {
    DNN_REQUIRE(c.pred[s], "%s: pred[%d] is NULL", c.who, s);
    mp->p[s] = c.pred[s];
  }
  const unsigned long long need = wide_workspace(*nb, c.n_images);
  DNN_REQUIRE(host || (c.workspace && c.workspace_bytes >= need && !(reinterpret_cast<uintptr_t>(c.workspace) & 7u)),
              "%s: workspace %p of %llu bytes; %d images of %d points need %llu bytes, 8-byte aligned", c.who,
              c.workspace, c.workspace_bytes, c.n_images, *nb, need);
  return 1;
}

template <int MODE>
static void launch_dfl_kernels(const DflCall& c, const MultiPred& mp, int nb, bool vec, hipStream_t stream) {
  char* ws = static_cast<char*>(c.workspace);
  const dim3 grid((nb + PD_THREADS - 1) / PD_THREADS, c.n_images);
  const auto decode = vec ? yolo_dfl_decode_kernel<MODE, true> : yolo_dfl_decode_kernel<MODE, false>;
  hipLaunchKernelGGL(decode, grid, dim3(PD_THREADS), 0, stream, *c.h, mp, ws, nb, c.n_images);
  hipLaunchKernelGGL(yolo_dfl_nms_kernel<MODE>, dim3(c.n_images), dim3(PM_THREADS), 0, stream, *c.h, mp, c.dets,
                     c.max_det, c.counts, ws, nb, c.n_images, c.points);
}

int launch_yolo_dfl(const DflCall& c, hipStream_t stream) {
  int nb;
  MultiPred mp;
  const int go = check_dfl_call(c, false, &nb, &mp);
  if (go <= 0) return go;
  const int n_ints = c.n_images * (PW_CTR_BYTES / 4);
  hipLaunchKernelGGL(yolo_dfl_clear_kernel, dim3((n_ints + PD_THREADS - 1) / PD_THREADS), dim3(PD_THREADS), 0, stream,
                     reinterpret_cast<int*>(c.workspace), n_ints);
  // 16-byte loads: every point's class logits start on a 16-byte boundary (4 R floats into a point of
  // 4 R + C floats, C % 4 == 0, in a 16-byte aligned tensor)
  bool vec = c.h->n_classes % 4 == 0;
  for (int s = 0; s < c.h->n_scales; ++s) vec = vec && !(reinterpret_cast<uintptr_t>(mp.p[s]) & 15u);
  // with one class the rules and the label modes are the same function
  if (c.h->n_classes == 1 || (c.nms_mode == DNN_YOLO_NMS_ANY_CLASS))
    launch_dfl_kernels<PD_ANY>(c, mp, nb, vec, stream);
  else if (c.labels_mode == DNN_YOLO_LABELS_MULTI)
    launch_dfl_kernels<PD_MULTI>(c, mp, nb, vec, stream);
  else
    launch_dfl_kernels<PD_PER_CLASS>(c, mp, nb, vec, stream);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("launch yolo_dfl: %s", hipGetErrorString(e));
    return -1;
  }
  return 0;
}

// Host pointers, synchronous: one allocation holding the tensors, the detections, the counts and the workspace
// (each 8-byte aligned, the tensors 16), copy in, launch, copy out; freed on every path.
static int yolo_dfl_host(const DflCall& c) {
  int nb;
  MultiPred mp;
  const int go = check_dfl_call(c, true, &nb, &mp);
  if (go <= 0) return go;
  const int ch = 4 * c.h->reg_max + c.h->n_classes;
  size_t pf[DNN_YOLO_MAX_SCALES] = {0}, poff[DNN_YOLO_MAX_SCALES] = {0}, pb = 0;
  for (int s = 0; s < c.h->n_scales; ++s) {
    pf[s] = (size_t)c.n_images * c.h->scale[s].grid_h * c.h->scale[s].grid_w * ch * sizeof(float);
    poff[s] = pb;
    pb += (pf[s] + 15) & ~(size_t)15;
  }
  const size_t db = (size_t)c.n_images * c.max_det * sizeof(dnn_detection);
  const size_t cb = ((size_t)c.n_images * sizeof(int) + 7) & ~(size_t)7;
  const size_t wb = (size_t)wide_workspace(nb, c.n_images);
  char* buf = nullptr;
  DNN_HIP_TRY(hipMalloc(&buf, pb + db + cb + wb));
  const float* d_pred[DNN_YOLO_MAX_SCALES] = {nullptr, nullptr, nullptr, nullptr};
  DflCall d = c;  // the same call on the device copies
  d.pred = d_pred;
  d.dets = reinterpret_cast<dnn_detection*>(buf + pb);
  d.counts = reinterpret_cast<int*>(buf + pb + db);
  d.workspace = buf + pb + db + cb;
  d.workspace_bytes = wb;
  int rc = 0;
  for (int s = 0; s < c.h->n_scales && !rc; ++s) {
    d_pred[s] = reinterpret_cast<const float*>(buf + poff[s]);
    if (hipMemcpy(buf + poff[s], c.pred[s], pf[s], hipMemcpyHostToDevice) != hipSuccess) {
      set_error("%s: copy in failed", c.who);
      rc = -1;
    }
  }
  if (!rc) rc = launch_yolo_dfl(d, nullptr);
  if (!rc && (hipMemcpy(c.counts, d.counts, (size_t)c.n_images * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess ||
              (db && hipMemcpy(c.dets, d.dets, db, hipMemcpyDeviceToHost) != hipSuccess))) {
    set_error("%s: copy out failed", c.who);
    rc = -1;
  }
  (void)hipFree(buf);
  return rc;
}

}  // namespace dnnhip

extern "C" {

int dnn_yolo_dfl_boxes(const dnn_yolo_dfl* h) { return dnnhip::dfl_boxes(h, "dnn_yolo_dfl_boxes"); }

int dnn_yolo_dfl_workspace(const dnn_yolo_dfl* h, int n_images, unsigned long long* bytes) {
  const int nb = dnnhip::dfl_boxes(h, "dnn_yolo_dfl_workspace");
  if (nb < 0) return nb;
  DNN_REQUIRE(n_images >= 0 && bytes, "dnn_yolo_dfl_workspace: bad arguments (n_images=%d)", n_images);
  *bytes = dnnhip::wide_workspace(nb, n_images);
  return 0;
}

int dnn_yolo_postprocess_dfl(const dnn_yolo_dfl* h, const float* const* pred, int n_images, dnn_detection* dets,
                             int max_det, int* counts, void* workspace, unsigned long long workspace_bytes,
                             int nms_mode, int labels_mode, void* stream) {
  return dnnhip::launch_yolo_dfl({"dnn_yolo_postprocess_dfl", h, pred, n_images, dets, max_det, counts, workspace,
                                  workspace_bytes, nms_mode, labels_mode}, static_cast<hipStream_t>(stream));
}

int dnn_yolo_postprocess_dfl_host(const dnn_yolo_dfl* h, const float* const* pred, int n_images, dnn_detection* dets,
                                  int max_det, int* counts, int nms_mode, int labels_mode) {
  return dnnhip::yolo_dfl_host({"dnn_yolo_postprocess_dfl_host", h, pred, n_images, dets, max_det, counts, nullptr, 0,
                                nms_mode, labels_mode});
}

}  // extern "C"
