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
#include <cfloat>
#include "post_multi_dev.h"

namespace dnnhip {

__global__ void __launch_bounds__(PM_THREADS)
yolo_multi_kernel(const dnn_yolo_multi mh, const XyScale xy, const MultiPred pred, dnn_detection* __restrict__ dets,
                  int max_det, int* __restrict__ counts, char* workspace, int nb) {
  __shared__ unsigned long long keys[PM_CAP];
  __shared__ float anchors[DNN_YOLO_MAX_SCALES][2 * DNN_YOLO_MAX_ANCHORS];
  __shared__ const float* s_pred[DNN_YOLO_MAX_SCALES];
  __shared__ int s_off[DNN_YOLO_MAX_SCALES + 1], s_gw[DNN_YOLO_MAX_SCALES], s_na[DNN_YOLO_MAX_SCALES];
  __shared__ float s_cell[DNN_YOLO_MAX_SCALES], s_xs[DNN_YOLO_MAX_SCALES], s_xb[DNN_YOLO_MAX_SCALES];
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
      s_xs[s] = xy.s[s];
      s_xb[s] = xy.b[s];
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
    long long c4[4];
    float sc;
    int best;
    if (!decode_box(q, C, logistic, b, col, row, anchors[s], cell_px, s_xs[s], s_xb[s], c4, &sc, &best)) bad = 1;
    box[k][0] = c4[0];
    box[k][1] = c4[1];
    box[k][2] = c4[2];
    box[k][3] = c4[3];
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
  bitonic_sort(keys, ns, tid);

  // ---- phase 3: blocked greedy NMS, the kept list in place over keys[0 .. base)
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
}

// ---- per-class NMS (DNN_YOLO_NMS_PER_CLASS) ----------------------------------------------------
// The per-class result is the class-agnostic algorithm run on each class's candidates alone,
// merged by (score descending, global index).  So the candidates are sorted class-major, every
// class is a contiguous segment of the sorted keys, and the segments are independent:
//
//   phase 1  the decode above; a candidate's key is class (7 bits) | ~score (32) | global index
//            (14), and an LDS counter per class is bumped.  A prefix sum over the counters gives
//            every class's segment [seg_start[c], seg_start[c + 1]) before the sort.
//   phase 2  the same bitonic sort: class-major, score descending inside a class.
//   phase 3  waves draw classes from an LDS ticket and run the blocked greedy NMS on a segment
//            ALONE, with wave-level operations only: no barrier inside, nobody waits for anybody.
//            The kept list of a segment goes in place over the segment's own consumed keys (the
//            invariant at the top of the file with "segment start" for "array start").  Segments
//            longer than PC_BIG candidates are left to a second pass in which the whole workgroup
//            runs nms_workgroup on each of them in turn (16 waves share the scan of the kept list).
//   phase 4  the kept lists are gathered into registers (position p of the concatenated lists,
//            found by a search in the prefix sum of the list lengths), then written back as dense
//            ~score | index keys, sorted over pow2 >= kept, and emitted as above.
constexpr int PC_IDX_BITS = 14;
static_assert(DNN_YOLO_MULTI_MAX_BOXES <= (1 << PC_IDX_BITS), "the global box index does not fit its key field");
static_assert(PC_CLS_BITS + 32 + PC_IDX_BITS < 64, "a candidate's key must stay below ~0ull");

__global__ void __launch_bounds__(PM_THREADS)
yolo_multi_classwise_kernel(const dnn_yolo_multi mh, const XyScale xy, const MultiPred pred,
                            dnn_detection* __restrict__ dets, int max_det, int* __restrict__ counts, char* workspace,
                            int nb) {
  __shared__ unsigned long long keys[PM_CAP];
  __shared__ float anchors[DNN_YOLO_MAX_SCALES][2 * DNN_YOLO_MAX_ANCHORS];
  __shared__ const float* s_pred[DNN_YOLO_MAX_SCALES];
  __shared__ int s_off[DNN_YOLO_MAX_SCALES + 1], s_gw[DNN_YOLO_MAX_SCALES], s_na[DNN_YOLO_MAX_SCALES];
  __shared__ float s_cell[DNN_YOLO_MAX_SCALES], s_xs[DNN_YOLO_MAX_SCALES], s_xb[DNN_YOLO_MAX_SCALES];
  __shared__ unsigned long long hitw[PM_WAVES];
  __shared__ int cls_cnt[DNN_YOLO_MAX_CLASSES];        // candidates per class
  __shared__ int seg_start[DNN_YOLO_MAX_CLASSES + 1];  // their prefix sum: class c is keys[seg_start[c] .. seg_start[c+1])
  __shared__ int seg_kept[DNN_YOLO_MAX_CLASSES];       // kept per class
  __shared__ int out_off[DNN_YOLO_MAX_CLASSES + 1];    // their prefix sum
  __shared__ int n_cand, bad, n_kept, zero_den, ticket;

  const int img = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int S = mh.n_scales, C = mh.scale[0].n_classes, stride = 5 + C;
  const bool logistic = mh.class_mode == 1;
  const float score_thr = mh.scale[0].score_thr;
  const double iou_thr = mh.scale[0].iou_thr;

  char* w = workspace + (size_t)img * nb * PM_BOX_BYTES;
  long long (*box)[4] = reinterpret_cast<long long (*)[4]>(w);
  float* score_of = reinterpret_cast<float*>(w + (size_t)nb * 32);
  int* cls_of = reinterpret_cast<int*>(w + (size_t)nb * 36);

  int nsort = 1;  // keys that the first sort can touch: pow2 >= nb, <= PM_CAP
  while (nsort < nb) nsort <<= 1;
  if (tid == 0) {
    n_cand = 0;
    bad = 0;
    n_kept = 0;
    zero_den = 0;
    ticket = 0;
    int off = 0;
#pragma unroll
    for (int s = 0; s < DNN_YOLO_MAX_SCALES; ++s) {
      const bool on = s < S;
      const int b = on ? mh.scale[s].grid_h * mh.scale[s].grid_w * mh.scale[s].n_anchors : 0;
      s_off[s] = off;
      s_gw[s] = on ? mh.scale[s].grid_w : 1;
      s_na[s] = on ? mh.scale[s].n_anchors : 1;
      s_cell[s] = on ? mh.scale[s].cell : 1.0f;
      s_xs[s] = xy.s[s];
      s_xb[s] = xy.b[s];
      s_pred[s] = on ? pred.p[s] + (size_t)img * b * stride : nullptr;
      off += b;
    }
    s_off[DNN_YOLO_MAX_SCALES] = off;
  }
  if (tid < 2 * DNN_YOLO_MAX_ANCHORS) {
#pragma unroll
    for (int s = 0; s < DNN_YOLO_MAX_SCALES; ++s) anchors[s][tid] = mh.scale[s].anchors[tid];
  }
  if (tid < DNN_YOLO_MAX_CLASSES) {
    cls_cnt[tid] = 0;
    seg_kept[tid] = 0;
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
    long long c4[4];
    float sc;
    int best;
    if (!decode_box(q, C, logistic, b, col, row, anchors[s], cell_px, s_xs[s], s_xb[s], c4, &sc, &best)) bad = 1;
    box[k][0] = c4[0];
    box[k][1] = c4[1];
    box[k][2] = c4[2];
    box[k][3] = c4[3];
    score_of[k] = sc;
    cls_of[k] = best;
    if (sc > score_thr) {  // score_thr >= 0: sc is positive, larger float bits = larger score
      const int pos = atomicAdd(&n_cand, 1);
      atomicAdd(&cls_cnt[best], 1);
      keys[pos] = ((unsigned long long)best << (32 + PC_IDX_BITS)) |
                  ((unsigned long long)(~__float_as_uint(sc)) << PC_IDX_BITS) | (unsigned)k;
    }
  }
  __syncthreads();
  const int n = n_cand;
  if (bad) {
    if (tid == 0) counts[img] = -1;
    return;
  }
  if (wid == 0) wave_scan_128(cls_cnt, C, seg_start, lane);

  // ---- phase 2: bitonic sort of the first pow2 >= n keys: class-major
  int ns = 1;
  while (ns < n) ns <<= 1;
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
      const int nk = nms_wave<PC_IDX_BITS>(keys + s0, len, box, iou_thr, lane, &zd);
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
    nms_workgroup<PC_IDX_BITS>(keys + s0, len, box, iou_thr, hitw, &n_kept, &zero_den, lane, wid);
    if (tid == 0) {
      seg_kept[c] = n_kept;
      n_kept = 0;
    }
    __syncthreads();
  }

  // ---- phase 4: merge the kept lists by (score, global index)
  if (wid == 0) wave_scan_128(seg_kept, C, out_off, lane);
  __syncthreads();
  if (zero_den) {
    if (tid == 0) counts[img] = -2;
    return;
  }
  const int nk = out_off[DNN_YOLO_MAX_CLASSES];
  int mine[16];  // entries tid, tid + 1024, ... of the concatenated kept lists
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
      mine[i] = reinterpret_cast<const int*>(keys + seg_start[lo])[p - out_off[lo]];
    }
  }
  __syncthreads();  // every list entry is in a register: the keys may be overwritten
  int ns2 = 1;
  while (ns2 < nk) ns2 <<= 1;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int p = tid + i * PM_THREADS;
    if (p < nk)
      keys[p] = ((unsigned long long)(~__float_as_uint(score_of[mine[i]])) << 32) | (unsigned)mine[i];
    else if (p < ns2)
      keys[p] = ~0ull;
  }
  __syncthreads();
  bitonic_sort(keys, ns2, tid);

  const int nw = nk < max_det ? nk : max_det;
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
}

// ---- multi-label (DNN_YOLO_LABELS_MULTI), per-class NMS ---------------------------------------
// Every (box, class) with conf * p[class] > score_thr is a candidate of its own, so an image can
// have more candidates than boxes: up to PM_CAP of them, the keys that fit in LDS (more: -3).
// The phases are the per-class kernel's with these differences:
//
//   phase 1  a box appends one key per class above the threshold.  p[c] <= 1 and fp32
//            multiplication is monotone, so conf * p[c] <= conf: a box whose objectness is not
//            above the threshold has no candidate and its class scores are not evaluated.  In
//            logistic mode the classes of a box are independent, and the boxes that pass are
//            first queued (in the workspace), then scored one thread per (queued box, class):
//            skipped boxes are skipped arithmetic, not idle lanes, and a wave's 64 loads are 64
//            consecutive logits.  In softmax mode a box's thread scores its classes itself (they
//            share the max and the sum).  The counter counts every candidate; a key is stored
//            only while its position is below PM_CAP.  The workspace keeps the box's corners, its
//            conf (where the single-label kernels keep the score) and, where they keep the class,
//            in softmax mode the box's sum and in logistic mode the queue.
//            The ~0ull padding of the sort is written after the count is known.
//   phase 3  unchanged: the kept lists are 4-byte box indices in place over their own segment,
//            so the invariant at the top of the file holds as it stands.
//   phase 4  a kept entry's class is its segment; the entries go to registers as index | class
//            << 14, then back as a DENSE int list at the start of the key array, which is expanded
//            in place into the merge keys ~score (32) | index (14) | class (7) from the top chunk of
//            1024 down.  Chunk j reads ints [1024 j, 1024 j + 1024) before a barrier and writes
//            bytes [8192 j, 8192 j + 8192) = ints [2048 j, 2048 j + 2048) after it: at or above
//            every int of the chunks below, which are the only ones still unread.  The score is
//            recomputed by label_score from the stored conf (and sum), the bits it was sorted on.
constexpr int ML_KEY_CLS_MASK = (1 << PC_CLS_BITS) - 1, ML_KEY_IDX_MASK = (1 << PC_IDX_BITS) - 1;
static_assert(DNN_YOLO_MULTI_MAX_CANDIDATES == PM_CAP, "the candidates of an image are the keys that fit in LDS");

__global__ void __launch_bounds__(PM_THREADS)
yolo_multi_labels_kernel(const dnn_yolo_multi mh, const XyScale xy, const MultiPred pred,
                         dnn_detection* __restrict__ dets, int max_det, int* __restrict__ counts, char* workspace,
                         int nb) {
  __shared__ unsigned long long keys[PM_CAP];
  __shared__ float anchors[DNN_YOLO_MAX_SCALES][2 * DNN_YOLO_MAX_ANCHORS];
  __shared__ const float* s_pred[DNN_YOLO_MAX_SCALES];
  __shared__ int s_off[DNN_YOLO_MAX_SCALES + 1], s_gw[DNN_YOLO_MAX_SCALES], s_na[DNN_YOLO_MAX_SCALES];
  __shared__ float s_cell[DNN_YOLO_MAX_SCALES], s_xs[DNN_YOLO_MAX_SCALES], s_xb[DNN_YOLO_MAX_SCALES];
  __shared__ unsigned long long hitw[PM_WAVES];
  __shared__ int cls_cnt[DNN_YOLO_MAX_CLASSES];        // candidates per class
  __shared__ int seg_start[DNN_YOLO_MAX_CLASSES + 1];  // their prefix sum: class c is keys[seg_start[c] .. seg_start[c+1])
  __shared__ int seg_kept[DNN_YOLO_MAX_CLASSES];       // kept per class
  __shared__ int out_off[DNN_YOLO_MAX_CLASSES + 1];    // their prefix sum
  __shared__ int n_cand, n_gated, bad, n_kept, zero_den, ticket;

  const int img = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int S = mh.n_scales, C = mh.scale[0].n_classes, stride = 5 + C;
  const bool logistic = mh.class_mode == 1;
  const float score_thr = mh.scale[0].score_thr;
  const double iou_thr = mh.scale[0].iou_thr;

  char* w = workspace + (size_t)img * nb * PM_BOX_BYTES;
  long long (*box)[4] = reinterpret_cast<long long (*)[4]>(w);
  float* conf_of = reinterpret_cast<float*>(w + (size_t)nb * 32);
  float* sum_of = reinterpret_cast<float*>(w + (size_t)nb * 36);  // softmax mode, boxes with conf > score_thr
  int* gated = reinterpret_cast<int*>(w + (size_t)nb * 36);       // logistic mode: the boxes with conf > score_thr

  if (tid == 0) {
    n_cand = 0;
    n_gated = 0;
    bad = 0;
    n_kept = 0;
    zero_den = 0;
    ticket = 0;
    int off = 0;
#pragma unroll
    for (int s = 0; s < DNN_YOLO_MAX_SCALES; ++s) {
      const bool on = s < S;
      const int b = on ? mh.scale[s].grid_h * mh.scale[s].grid_w * mh.scale[s].n_anchors : 0;
      s_off[s] = off;
      s_gw[s] = on ? mh.scale[s].grid_w : 1;
      s_na[s] = on ? mh.scale[s].n_anchors : 1;
      s_cell[s] = on ? mh.scale[s].cell : 1.0f;
      s_xs[s] = xy.s[s];
      s_xb[s] = xy.b[s];
      s_pred[s] = on ? pred.p[s] + (size_t)img * b * stride : nullptr;
      off += b;
    }
    s_off[DNN_YOLO_MAX_SCALES] = off;
  }
  if (tid < 2 * DNN_YOLO_MAX_ANCHORS) {
#pragma unroll
    for (int s = 0; s < DNN_YOLO_MAX_SCALES; ++s) anchors[s][tid] = mh.scale[s].anchors[tid];
  }
  if (tid < DNN_YOLO_MAX_CLASSES) {
    cls_cnt[tid] = 0;
    seg_kept[tid] = 0;
  }
  __syncthreads();

  // ---- phase 1: decode, one key per (box, class) above the threshold
  auto append = [&](int c, float sc, int k) {  // sc > score_thr >= 0: larger float bits = larger score
    const int pos = atomicAdd(&n_cand, 1);
    if (pos < PM_CAP) {  // beyond it only the count matters: the image ends with -3 below
      atomicAdd(&cls_cnt[c], 1);
      keys[pos] = ((unsigned long long)c << (32 + PC_IDX_BITS)) |
                  ((unsigned long long)(~__float_as_uint(sc)) << PC_IDX_BITS) | (unsigned)k;
    }
  };
  for (int k = tid; k < nb; k += PM_THREADS) {
    int s = 0;
    while (s + 1 < S && k >= s_off[s + 1]) ++s;
    const int kk = k - s_off[s], A = s_na[s], gw = s_gw[s];
    const float* q = s_pred[s] + (size_t)kk * stride;
    const int b = kk % A, cell = kk / A, col = cell % gw, row = cell / gw;
    long long c4[4];
    float conf;
    if (!decode_corners(q, b, col, row, anchors[s], s_cell[s], s_xs[s], s_xb[s], c4, &conf)) bad = 1;
    box[k][0] = c4[0];
    box[k][1] = c4[1];
    box[k][2] = c4[2];
    box[k][3] = c4[3];
    conf_of[k] = conf;
    if (!(conf > score_thr)) continue;  // conf * p[c] <= conf: no class of this box is a candidate
    if (logistic) {
      gated[atomicAdd(&n_gated, 1)] = k | (s << PC_IDX_BITS);  // at most nb entries: the box and its scale
      continue;
    }
    const float* lg = q + 5;
    const float m = logit_max(lg, C), sum = softmax_sum(lg, C, m);
    sum_of[k] = sum;
    for (int c = 0; c < C; ++c) {
      const float sc = label_score(lg[c], false, conf, m, sum);
      if (sc > score_thr) append(c, sc, k);
    }
  }
  __syncthreads();
  if (bad) {
    if (tid == 0) counts[img] = -1;
    return;
  }
  if (logistic) {  // one thread per (queued box, class): pair i = tid + 1024 j is box i / C, class i % C,
                   // stepped without a division
    const int pairs = n_gated * C;  // <= 16384 * 128
    const int dq = PM_THREADS / C, dr = PM_THREADS % C;
    int g = tid / C, c = tid % C;
    for (int i = tid; i < pairs; i += PM_THREADS) {
      const int e = gated[g], k = e & ML_KEY_IDX_MASK, s = e >> PC_IDX_BITS;
      const float logit = s_pred[s][(size_t)(k - s_off[s]) * stride + 5 + c];
      const float sc = label_score(logit, true, conf_of[k], 0.0f, 1.0f);
      if (sc > score_thr) append(c, sc, k);
      g += dq;
      c += dr;
      if (c >= C) {
        c -= C;
        ++g;
      }
    }
    __syncthreads();
  }
  const int n = n_cand;
  if (n > PM_CAP) {
    if (tid == 0) counts[img] = -3;
    return;
  }
  if (wid == 0) wave_scan_128(cls_cnt, C, seg_start, lane);

  // ---- phase 2: bitonic sort of the first pow2 >= n keys (<= PM_CAP), padded now: class-major
  int ns = 1;
  while (ns < n) ns <<= 1;
  for (int i = n + tid; i < ns; i += PM_THREADS) keys[i] = ~0ull;
  __syncthreads();  // the padding and seg_start (the sort has no barrier when n <= 1)
  bitonic_sort(keys, ns, tid);

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
      const int nk = nms_wave<PC_IDX_BITS>(keys + s0, len, box, iou_thr, lane, &zd);
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
    nms_workgroup<PC_IDX_BITS>(keys + s0, len, box, iou_thr, hitw, &n_kept, &zero_den, lane, wid);
    if (tid == 0) {
      seg_kept[c] = n_kept;
      n_kept = 0;
    }
    __syncthreads();
  }

  // ---- phase 4: merge the kept lists by (score, global index, class)
  if (wid == 0) wave_scan_128(seg_kept, C, out_off, lane);
  __syncthreads();
  if (zero_den) {
    if (tid == 0) counts[img] = -2;
    return;
  }
  const int nk = out_off[DNN_YOLO_MAX_CLASSES];
  int mine[16];  // entries tid, tid + 1024, ... of the concatenated kept lists: index | class << 14
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
      mine[i] = reinterpret_cast<const int*>(keys + seg_start[lo])[p - out_off[lo]] | (lo << PC_IDX_BITS);
    }
  }
  __syncthreads();  // every list entry is in a register: the keys may be overwritten
  int* dense = reinterpret_cast<int*>(keys);
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int p = tid + i * PM_THREADS;
    if (p < nk) dense[p] = mine[i];
  }
  int ns2 = 1;
  while (ns2 < nk) ns2 <<= 1;
  for (int p = nk + tid; p < ns2; p += PM_THREADS) keys[p] = ~0ull;  // bytes >= 8 nk: above the dense list
  __syncthreads();
  for (int j = (nk - 1) / PM_THREADS; j >= 0; --j) {  // workgroup-uniform; see the invariant above
    const int p = tid + j * PM_THREADS;
    unsigned long long key = 0;
    if (p < nk) {
      const int e = dense[p], k = e & ML_KEY_IDX_MASK, c = e >> PC_IDX_BITS;
      int s = 0;
      while (s + 1 < S && k >= s_off[s + 1]) ++s;
      const float* lg = s_pred[s] + (size_t)(k - s_off[s]) * stride + 5;
      const float sum = logistic ? 1.0f : sum_of[k];
      const float sc = label_score(lg[c], logistic, conf_of[k], logistic ? 0.0f : logit_max(lg, C), sum);
      key = ((unsigned long long)(~__float_as_uint(sc)) << (PC_IDX_BITS + PC_CLS_BITS)) |
            ((unsigned long long)k << PC_CLS_BITS) | (unsigned)c;
    }
    __syncthreads();
    if (p < nk) keys[p] = key;
  }
  __syncthreads();
  bitonic_sort(keys, ns2, tid);

  const int nw = nk < max_det ? nk : max_det;
  for (int r = tid; r < nw; r += PM_THREADS) {
    const unsigned long long key = keys[r];
    const int k = (int)(key >> PC_CLS_BITS) & ML_KEY_IDX_MASK;
    dnn_detection d;
    d.cls = (int)key & ML_KEY_CLS_MASK;
    d.score = __uint_as_float(~(unsigned)(key >> (PC_IDX_BITS + PC_CLS_BITS)));
    d.left = box[k][0];
    d.top = box[k][1];
    d.right = box[k][2];
    d.bottom = box[k][3];
    dets[(size_t)img * max_det + r] = d;
  }
  if (tid == 0) counts[img] = nk;
}

// < 0 with the error set, else the boxes of one image over all scales (at most max_boxes)
int multi_boxes_upto(const dnn_yolo_multi* m, const char* who, long long max_boxes) {
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
    const int nb = yolo_head_boxes(&m->scale[s], who, max_boxes);
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
  if (total > max_boxes) {
    set_error("%s: %lld boxes over %d scales > %lld", who, total, m->n_scales, max_boxes);
    return -2;
  }
  return (int)total;
}

static int multi_boxes(const dnn_yolo_multi* m, const char* who) {
  return multi_boxes_upto(m, who, DNN_YOLO_MULTI_MAX_BOXES);
}

static unsigned long long multi_workspace(int nb, int n_images) {
  return (unsigned long long)n_images * nb * PM_BOX_BYTES;
}

bool labels_mode_ok(int labels_mode, const char* who) {
  if (labels_mode == DNN_YOLO_LABELS_ARGMAX || labels_mode == DNN_YOLO_LABELS_MULTI) return true;
  set_error("%s: labels_mode %d: need %d (arg-max) or %d (multi-label)", who, labels_mode, DNN_YOLO_LABELS_ARGMAX,
            DNN_YOLO_LABELS_MULTI);
  return false;
}

bool nms_mode_ok(int nms_mode, const char* who) {
  if (nms_mode == DNN_YOLO_NMS_ANY_CLASS || nms_mode == DNN_YOLO_NMS_PER_CLASS) return true;
  set_error("%s: nms_mode %d: need %d (any class) or %d (per class)", who, nms_mode, DNN_YOLO_NMS_ANY_CLASS,
            DNN_YOLO_NMS_PER_CLASS);
  return false;
}

bool xy_scale_from(const float* scale_x_y, int n_scales, const char* who, XyScale* out) {
  for (int s = 0; s < DNN_YOLO_MAX_SCALES; ++s) {
    const float v = scale_x_y && s < n_scales ? scale_x_y[s] : 1.0f;
    if (!(v > 0.0f) || !(v <= FLT_MAX)) {
      set_error("%s: scale_x_y[%d] = %g: each value must be finite and > 0", who, s, (double)v);
      return false;
    }
    out->s[s] = v;
    out->b[s] = -0.5f * (v - 1.0f);
  }
  return true;
}

static int launch_yolo_multi(const char* who, const dnn_yolo_multi* m, const float* scale_x_y,
                             const float* const* pred, int n_images,
                             dnn_detection* dets, int max_det, int* counts, void* workspace,
                             unsigned long long workspace_bytes, int nms_mode, int labels_mode, hipStream_t stream) {
  const int nb = multi_boxes(m, who);
  if (nb < 0) return nb;
  if (!nms_mode_ok(nms_mode, who) || !labels_mode_ok(labels_mode, who)) return -2;
  XyScale xy;
  if (!xy_scale_from(scale_x_y, m->n_scales, who, &xy)) return -2;
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
  // with one class the rules and the label modes are the same function: the class-agnostic kernel
  // serves them all
  if (labels_mode == DNN_YOLO_LABELS_MULTI && nms_mode == DNN_YOLO_NMS_PER_CLASS && m->scale[0].n_classes > 1)
    hipLaunchKernelGGL(yolo_multi_labels_kernel, dim3(n_images), dim3(PM_THREADS), 0, stream, *m, xy, mp, dets, max_det,
                       counts, static_cast<char*>(workspace), nb);
  else if (nms_mode == DNN_YOLO_NMS_PER_CLASS && m->scale[0].n_classes > 1)
    hipLaunchKernelGGL(yolo_multi_classwise_kernel, dim3(n_images), dim3(PM_THREADS), 0, stream, *m, xy, mp, dets,
                       max_det, counts, static_cast<char*>(workspace), nb);
  else
    hipLaunchKernelGGL(yolo_multi_kernel, dim3(n_images), dim3(PM_THREADS), 0, stream, *m, xy, mp, dets, max_det,
                       counts, static_cast<char*>(workspace), nb);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("launch yolo_multi: %s", hipGetErrorString(e));
    return -1;
  }
  return 0;
}

// Host pointers, synchronous: allocates the scratch, copies in, runs, copies out.
static int yolo_multi_host(const char* who, const dnn_yolo_multi* m, const float* scale_x_y,
                           const float* const* pred, int n_images,
                           dnn_detection* dets, int max_det, int* counts, int nms_mode, int labels_mode) {
  const int nb = multi_boxes(m, who);
  if (nb < 0) return nb;
  if (!nms_mode_ok(nms_mode, who) || !labels_mode_ok(labels_mode, who)) return -2;
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
  const size_t wb = (size_t)multi_workspace(nb, n_images);
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
  if (!rc)
    rc = launch_yolo_multi(who, m, scale_x_y, d_pred, n_images, d_dets, max_det, d_counts, buf + pb + db + cb, wb,
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
  return dnnhip::launch_yolo_multi("dnn_yolo_postprocess_multi", m, nullptr, pred, n_images, dets, max_det, counts,
                                   workspace, workspace_bytes, DNN_YOLO_NMS_ANY_CLASS, DNN_YOLO_LABELS_ARGMAX,
                                   static_cast<hipStream_t>(stream));
}

int dnn_yolo_postprocess_multi_host(const dnn_yolo_multi* m, const float* const* pred, int n_images,
                                    dnn_detection* dets, int max_det, int* counts) {
  return dnnhip::yolo_multi_host("dnn_yolo_postprocess_multi_host", m, nullptr, pred, n_images, dets, max_det, counts,
                                 DNN_YOLO_NMS_ANY_CLASS, DNN_YOLO_LABELS_ARGMAX);
}

int dnn_yolo_multi_nms_workspace(const dnn_yolo_multi* m, int n_images, int nms_mode, unsigned long long* bytes) {
  const char* who = "dnn_yolo_multi_nms_workspace";
  const int nb = dnnhip::multi_boxes(m, who);
  if (nb < 0) return nb;
  if (!dnnhip::nms_mode_ok(nms_mode, who)) return -2;
  DNN_REQUIRE(n_images >= 0 && bytes, "dnn_yolo_multi_nms_workspace: bad arguments (n_images=%d)", n_images);
  *bytes = dnnhip::multi_workspace(nb, n_images);  // both kernels: 40 bytes per box
  return 0;
}

int dnn_yolo_postprocess_multi_nms(const dnn_yolo_multi* m, const float* const* pred, int n_images,
                                   dnn_detection* dets, int max_det, int* counts, void* workspace,
                                   unsigned long long workspace_bytes, int nms_mode, void* stream) {
  return dnnhip::launch_yolo_multi("dnn_yolo_postprocess_multi_nms", m, nullptr, pred, n_images, dets, max_det, counts,
                                   workspace, workspace_bytes, nms_mode, DNN_YOLO_LABELS_ARGMAX,
                                   static_cast<hipStream_t>(stream));
}

int dnn_yolo_postprocess_multi_nms_host(const dnn_yolo_multi* m, const float* const* pred, int n_images,
                                        dnn_detection* dets, int max_det, int* counts, int nms_mode) {
  return dnnhip::yolo_multi_host("dnn_yolo_postprocess_multi_nms_host", m, nullptr, pred, n_images, dets, max_det,
                                 counts, nms_mode, DNN_YOLO_LABELS_ARGMAX);
}

int dnn_yolo_multi_labels_workspace(const dnn_yolo_multi* m, int n_images, int labels_mode,
                                    unsigned long long* bytes) {
  const char* who = "dnn_yolo_multi_labels_workspace";
  const int nb = dnnhip::multi_boxes(m, who);
  if (nb < 0) return nb;
  if (!dnnhip::labels_mode_ok(labels_mode, who)) return -2;
  DNN_REQUIRE(n_images >= 0 && bytes, "dnn_yolo_multi_labels_workspace: bad arguments (n_images=%d)", n_images);
  *bytes = dnnhip::multi_workspace(nb, n_images);  // every kernel: 40 bytes per box
  return 0;
}

int dnn_yolo_postprocess_multi_labels(const dnn_yolo_multi* m, const float* const* pred, int n_images,
                                      dnn_detection* dets, int max_det, int* counts, void* workspace,
                                      unsigned long long workspace_bytes, int labels_mode, void* stream) {
  return dnnhip::launch_yolo_multi("dnn_yolo_postprocess_multi_labels", m, nullptr, pred, n_images, dets, max_det,
                                   counts, workspace, workspace_bytes, DNN_YOLO_NMS_PER_CLASS, labels_mode,
                                   static_cast<hipStream_t>(stream));
}

int dnn_yolo_postprocess_multi_labels_host(const dnn_yolo_multi* m, const float* const* pred, int n_images,
                                           dnn_detection* dets, int max_det, int* counts, int labels_mode) {
  return dnnhip::yolo_multi_host("dnn_yolo_postprocess_multi_labels_host", m, nullptr, pred, n_images, dets, max_det,
                                 counts, DNN_YOLO_NMS_PER_CLASS, labels_mode);
}

// the _xy entries take the wide entry's mode pairs: (any class, multi-label) is no rule of either
static bool xy_modes_ok(int nms_mode, int labels_mode, const char* who) {
  if (!dnnhip::nms_mode_ok(nms_mode, who) || !dnnhip::labels_mode_ok(labels_mode, who)) return false;
  if (labels_mode == DNN_YOLO_LABELS_MULTI && nms_mode != DNN_YOLO_NMS_PER_CLASS) {
    dnnhip::set_error("%s: multi-label detections need per-class NMS (nms_mode %d)", who, DNN_YOLO_NMS_PER_CLASS);
    return false;
  }
  return true;
}

int dnn_yolo_postprocess_multi_xy(const dnn_yolo_multi* m, const float* scale_x_y, const float* const* pred,
                                  int n_images, dnn_detection* dets, int max_det, int* counts, void* workspace,
                                  unsigned long long workspace_bytes, int nms_mode, int labels_mode, void* stream) {
  const char* who = "dnn_yolo_postprocess_multi_xy";
  if (!xy_modes_ok(nms_mode, labels_mode, who)) return -2;
  return dnnhip::launch_yolo_multi(who, m, scale_x_y, pred, n_images, dets, max_det, counts, workspace,
                                   workspace_bytes, nms_mode, labels_mode, static_cast<hipStream_t>(stream));
}

int dnn_yolo_postprocess_multi_xy_host(const dnn_yolo_multi* m, const float* scale_x_y, const float* const* pred,
                                       int n_images, dnn_detection* dets, int max_det, int* counts, int nms_mode,
                                       int labels_mode) {
  const char* who = "dnn_yolo_postprocess_multi_xy_host";
  if (!xy_modes_ok(nms_mode, labels_mode, who)) return -2;
  return dnnhip::yolo_multi_host(who, m, scale_x_y, pred, n_images, dets, max_det, counts, nms_mode, labels_mode);
}

}  // extern "C"
