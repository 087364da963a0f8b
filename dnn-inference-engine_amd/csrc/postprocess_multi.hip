// Multi-scale YOLO postprocessing (include/dnn_hip_post.h: dnn_yolo_multi): the boxes of up to
// DNN_YOLO_MAX_SCALES heads of one image (YOLOv3: strides 32, 16, 8) decoded, thresholded, sorted
// and put through ONE greedy NMS, one workgroup per image, up to DNN_YOLO_MULTI_MAX_BOXES boxes.
// The per-box arithmetic and the three phases are postprocess_head.hip's (post_math.h); every phase
// is a helper of post_multi_dev.h, which postprocess_wide.hip's kernels call too, and the kernels
// below are sequences of those calls:
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
// (The other in-place step, the multi-label merge, has its invariant at merge_labels.)
//
// This file also defines the host side of both files' entries: the description and argument
// checks and the host staging (declared in post_multi_dev.h).
#include <cfloat>
#include <climits>
#include "post_multi_dev.h"

namespace dnnhip {

__global__ void __launch_bounds__(PM_THREADS)
yolo_multi_kernel(const dnn_yolo_multi mh, const XyScale xy, const MultiPred pred, dnn_detection* __restrict__ dets,
                  int max_det, int* __restrict__ counts, char* workspace, int nb) {
  __shared__ unsigned long long keys[PM_CAP];
  __shared__ ScaleTab t;
  __shared__ NmsState st;
  __shared__ int n_cand, bad;

  const int img = blockIdx.x, tid = threadIdx.x;
  const int S = mh.n_scales, C = mh.scale[0].n_classes, stride = 5 + C;
  const bool logistic = mh.class_mode == 1;
  const float score_thr = mh.scale[0].score_thr;
  const BoxStore bs = box_store(workspace + (size_t)img * nb * PM_BOX_BYTES, nb);

  int nsort = 1;  // keys that the sort can touch: pow2 >= nb, <= PM_CAP
  while (nsort < nb) nsort <<= 1;
  if (tid == 0) {
    n_cand = 0;
    bad = 0;
  }
  reset_state(st, tid);
  fill_scale_tab(t, mh, &xy, pred, img, stride, tid);
  for (int i = tid; i < nsort; i += PM_THREADS) keys[i] = ~0ull;
  __syncthreads();

  // ---- phase 1: decode
  for (int k = tid; k < nb; k += PM_THREADS) {
    float sc;
    int best;
    decode_single_at(t, box_at(t, S, k, stride), C, logistic, bs, k, &sc, &best, &bad);
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

  // ---- phases 2 and 3, the kept list in place over keys[0 .. base); emit
  nms_any_emit<PM_THREADS>(keys, n_cand, bs, mh.scale[0].iou_thr, st, dets + (size_t)img * max_det, max_det, &counts[img], tid);
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
//   phase 3  nms_segments: waves draw classes from an LDS ticket and run the blocked greedy NMS on
//            a segment ALONE, with wave-level operations only.  The kept list of a segment goes in
//            place over the segment's own consumed keys (the invariant at the top of the file with
//            "segment start" for "array start").  Segments longer than PC_BIG candidates are left
//            to a second pass by the whole workgroup (16 waves share the scan of the kept list).
//   phase 4  gather_kept, merge_single: the kept lists are gathered into registers (position p of
//            the concatenated lists, found by a search in the prefix sum of the list lengths), then
//            written back as dense ~score | index keys, sorted over pow2 >= kept, and emitted.
__global__ void __launch_bounds__(PM_THREADS)
yolo_multi_classwise_kernel(const dnn_yolo_multi mh, const XyScale xy, const MultiPred pred,
                            dnn_detection* __restrict__ dets, int max_det, int* __restrict__ counts, char* workspace,
                            int nb) {
  __shared__ unsigned long long keys[PM_CAP];
  __shared__ ScaleTab t;
  __shared__ ClassState st;
  __shared__ int n_cand, bad;

  const int img = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int S = mh.n_scales, C = mh.scale[0].n_classes, stride = 5 + C;
  const bool logistic = mh.class_mode == 1;
  const float score_thr = mh.scale[0].score_thr;
  const BoxStore bs = box_store(workspace + (size_t)img * nb * PM_BOX_BYTES, nb);

  int nsort = 1;  // keys that the first sort can touch: pow2 >= nb, <= PM_CAP
  while (nsort < nb) nsort <<= 1;
  if (tid == 0) {
    n_cand = 0;
    bad = 0;
  }
  reset_state(st, tid);
  fill_scale_tab(t, mh, &xy, pred, img, stride, tid);
  for (int i = tid; i < nsort; i += PM_THREADS) keys[i] = ~0ull;
  __syncthreads();

  // ---- phase 1: decode
  for (int k = tid; k < nb; k += PM_THREADS) {
    float sc;
    int best;
    decode_single_at(t, box_at(t, S, k, stride), C, logistic, bs, k, &sc, &best, &bad);
    if (sc > score_thr) {
      const int pos = atomicAdd(&n_cand, 1);
      atomicAdd(&st.cls_cnt[best], 1);
      keys[pos] = key_class<PC_IDX_BITS>(best, sc, k);
    }
  }
  __syncthreads();
  const int n = n_cand;
  if (bad) {
    if (tid == 0) counts[img] = -1;
    return;
  }
  if (wid == 0) wave_scan_128(st.cls_cnt, C, st.seg_start, lane);

  // ---- phase 2: bitonic sort of the first pow2 >= n keys: class-major
  int ns = 1;
  while (ns < n) ns <<= 1;
  bitonic_sort<PM_THREADS>(keys, ns, tid);
  __syncthreads();  // seg_start too (the sort has no barrier when n <= 1)

  // ---- phase 3: every class segment alone; phase 4: merge the kept lists by (score, global index)
  const int nk = nms_segments<PC_IDX_BITS>(keys, C, bs.box, mh.scale[0].iou_thr, st, tid);
  if (nk < 0) {
    if (tid == 0) counts[img] = -2;
    return;
  }
  int mine[16];
  gather_kept<PC_IDX_BITS, false>(keys, C, nk, st, mine, tid);
  merge_single(keys, mine, nk, bs, dets + (size_t)img * max_det, max_det, &counts[img], tid);
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
//   phase 4  gather_kept with the class, merge_labels: a kept entry's class is its segment, and the
//            merge keys are expanded in place from a dense list of the entries (the invariant is
//            documented there).
static_assert(DNN_YOLO_MULTI_MAX_CANDIDATES == PM_CAP, "the candidates of an image are the keys that fit in LDS");

__global__ void __launch_bounds__(PM_THREADS)
yolo_multi_labels_kernel(const dnn_yolo_multi mh, const XyScale xy, const MultiPred pred,
                         dnn_detection* __restrict__ dets, int max_det, int* __restrict__ counts, char* workspace,
                         int nb) {
  __shared__ unsigned long long keys[PM_CAP];
  __shared__ ScaleTab t;
  __shared__ ClassState st;
  __shared__ int n_cand, n_gated, bad;

  const int img = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int S = mh.n_scales, C = mh.scale[0].n_classes, stride = 5 + C;
  const bool logistic = mh.class_mode == 1;
  const float score_thr = mh.scale[0].score_thr;
  const BoxStore bs = box_store(workspace + (size_t)img * nb * PM_BOX_BYTES, nb);  // score: the box's conf
  int* gated = bs.cls;  // logistic mode: the boxes with conf > score_thr

  if (tid == 0) {
    n_cand = 0;
    n_gated = 0;
    bad = 0;
  }
  reset_state(st, tid);
  fill_scale_tab(t, mh, &xy, pred, img, stride, tid);
  __syncthreads();

  // ---- phase 1: decode, one key per (box, class) above the threshold
  auto append = [&](int c, float sc, int k) {
    const int pos = atomicAdd(&n_cand, 1);
    if (pos < PM_CAP) {  // beyond it only the count matters: the image ends with -3 below
      atomicAdd(&st.cls_cnt[c], 1);
      keys[pos] = key_class<PC_IDX_BITS>(c, sc, k);
    }
  };
  for (int k = tid; k < nb; k += PM_THREADS) {
    const BoxAt at = box_at(t, S, k, stride);
    float conf;
    decode_corners_at(t, at, bs, k, &conf, &bad);
    bs.score[k] = conf;
    if (!(conf > score_thr)) continue;  // conf * p[c] <= conf: no class of this box is a candidate
    if (logistic) {
      gated[atomicAdd(&n_gated, 1)] = k | (at.s << PC_IDX_BITS);  // at most nb entries: the box and its scale
      continue;
    }
    const float* lg = at.q + 5;
    const float m = logit_max(lg, C), sum = softmax_sum(lg, C, m);
    bs.sum()[k] = sum;
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
      const int e = gated[g], k = e & ((1 << PC_IDX_BITS) - 1), s = e >> PC_IDX_BITS;
      const float sc = label_score(box_values(t, s, k, stride)[5 + c], true, bs.score[k], 0.0f, 1.0f);
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
  if (wid == 0) wave_scan_128(st.cls_cnt, C, st.seg_start, lane);

  // ---- phase 2: bitonic sort of the first pow2 >= n keys (<= PM_CAP), padded now: class-major
  int ns = 1;
  while (ns < n) ns <<= 1;
  for (int i = n + tid; i < ns; i += PM_THREADS) keys[i] = ~0ull;
  __syncthreads();  // the padding and seg_start (the sort has no barrier when n <= 1)
  bitonic_sort<PM_THREADS>(keys, ns, tid);

  // ---- phase 3: every class segment alone; phase 4: merge by (score, global index, class)
  const int nk = nms_segments<PC_IDX_BITS>(keys, C, bs.box, mh.scale[0].iou_thr, st, tid);
  if (nk < 0) {
    if (tid == 0) counts[img] = -2;
    return;
  }
  int mine[16];
  gather_kept<PC_IDX_BITS, true>(keys, C, nk, st, mine, tid);
  merge_labels<PC_IDX_BITS>(keys, mine, nk, t, S, C, stride, logistic, bs, dets + (size_t)img * max_det, max_det,
                            &counts[img], tid);
}

// ---- host side -------------------------------------------------------------------------------------
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

static bool labels_mode_ok(int labels_mode, const char* who) {
  if (labels_mode == DNN_YOLO_LABELS_ARGMAX || labels_mode == DNN_YOLO_LABELS_MULTI) return true;
  set_error("%s: labels_mode %d: need %d (arg-max) or %d (multi-label)", who, labels_mode, DNN_YOLO_LABELS_ARGMAX,
            DNN_YOLO_LABELS_MULTI);
  return false;
}

static bool nms_mode_ok(int nms_mode, const char* who) {
  if (nms_mode == DNN_YOLO_NMS_ANY_CLASS || nms_mode == DNN_YOLO_NMS_PER_CLASS) return true;
  set_error("%s: nms_mode %d: need %d (any class) or %d (per class)", who, nms_mode, DNN_YOLO_NMS_ANY_CLASS,
            DNN_YOLO_NMS_PER_CLASS);
  return false;
}

bool multi_modes_ok(int nms_mode, int labels_mode, const char* who) {
  if (!nms_mode_ok(nms_mode, who) || !labels_mode_ok(labels_mode, who)) return false;
  if (labels_mode == DNN_YOLO_LABELS_MULTI && nms_mode != DNN_YOLO_NMS_PER_CLASS) {
    set_error("%s: labels_mode %d (multi-label) needs nms_mode %d (per class): under the class-agnostic rule a box's "
              "second label is always suppressed by its first", who, labels_mode, DNN_YOLO_NMS_PER_CLASS);
    return false;
  }
  return true;
}

// Fills *out from a host array of n_scales floats (NULL: all 1); false with the error set (it names
// scale_x_y) when a value is not finite or not > 0.
static bool xy_scale_from(const float* scale_x_y, int n_scales, const char* who, XyScale* out) {
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

int check_multi_call(const MultiCall& c, const MultiKind& kind, bool host, MultiArgs* out) {
  out->nb = multi_boxes_upto(c.m, c.who, kind.max_boxes);
  if (out->nb < 0) return out->nb;
  if (!multi_modes_ok(c.nms_mode, c.labels_mode, c.who)) return -2;
  if (!xy_scale_from(c.scale_x_y, c.m->n_scales, c.who, &out->xy)) return -2;
  if (c.n_images < 0 || c.max_det < 0 || (c.n_images > 0 && (!c.pred || !c.counts || (c.max_det > 0 && !c.dets)))) {
    set_error("%s: bad arguments (n_images=%d max_det=%d)", c.who, c.n_images, c.max_det);
    return -2;
  }
  if (c.n_images == 0) return 0;
  if (c.n_images > kind.max_images) {
    set_error("%s: %d images > %d, the most one launch takes", c.who, c.n_images, kind.max_images);
    return -2;
  }
  out->mp = MultiPred{};
  for (int s = 0; s < c.m->n_scales; ++s) {
    if (!c.pred[s]) {
      set_error("%s: pred[%d] is NULL", c.who, s);
      return -2;
    }
    out->mp.p[s] = c.pred[s];
  }
  const unsigned long long need = kind.workspace(out->nb, c.n_images);
  if (!host && (!c.workspace || c.workspace_bytes < need || (reinterpret_cast<uintptr_t>(c.workspace) & 7u))) {
    set_error("%s: workspace %p of %llu bytes; %d images of %d boxes need %llu bytes, 8-byte aligned", c.who,
              c.workspace, c.workspace_bytes, c.n_images, out->nb, need);
    return -2;
  }
  return 1;
}

int yolo_multi_host(const MultiCall& c, const MultiKind& kind) {
  MultiArgs a;
  const int go = check_multi_call(c, kind, true, &a);
  if (go <= 0) return go;
  const int stride = 5 + c.m->scale[0].n_classes;
  size_t pf[DNN_YOLO_MAX_SCALES] = {0}, poff[DNN_YOLO_MAX_SCALES] = {0}, pb = 0;
  for (int s = 0; s < c.m->n_scales; ++s) {
    const dnn_yolo_head& h = c.m->scale[s];
    pf[s] = (size_t)c.n_images * h.grid_h * h.grid_w * h.n_anchors * stride * sizeof(float);
    poff[s] = pb;
    pb += (pf[s] + 7) & ~(size_t)7;  // keeps every tensor, dets and the workspace 8-byte aligned
  }
  const size_t db = (size_t)c.n_images * c.max_det * sizeof(dnn_detection);
  const size_t cb = ((size_t)c.n_images * sizeof(int) + 7) & ~(size_t)7;
  const size_t wb = (size_t)kind.workspace(a.nb, c.n_images);
  char* buf = nullptr;
  DNN_HIP_TRY(hipMalloc(&buf, pb + db + cb + wb));
  const float* d_pred[DNN_YOLO_MAX_SCALES] = {nullptr, nullptr, nullptr, nullptr};
  MultiCall d = c;  // the same call on the device copies
  d.pred = d_pred;
  d.dets = reinterpret_cast<dnn_detection*>(buf + pb);
  d.counts = reinterpret_cast<int*>(buf + pb + db);
  d.workspace = buf + pb + db + cb;
  d.workspace_bytes = wb;
  int rc = 0;
  for (int s = 0; s < c.m->n_scales && !rc; ++s) {
    d_pred[s] = reinterpret_cast<const float*>(buf + poff[s]);
    if (hipMemcpy(buf + poff[s], c.pred[s], pf[s], hipMemcpyHostToDevice) != hipSuccess) {
      set_error("%s: copy in failed", c.who);
      rc = -1;
    }
  }
  if (!rc) rc = kind.launch(d, nullptr);
  if (!rc && (hipMemcpy(c.counts, d.counts, (size_t)c.n_images * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess ||
              (db && hipMemcpy(c.dets, d.dets, db, hipMemcpyDeviceToHost) != hipSuccess))) {
    set_error("%s: copy out failed", c.who);
    rc = -1;
  }
  (void)hipFree(buf);
  return rc;
}

static unsigned long long multi_workspace(int nb, int n_images) {
  return (unsigned long long)n_images * nb * PM_BOX_BYTES;
}

static int launch_yolo_multi(const MultiCall& c, hipStream_t stream);
static const MultiKind MULTI = {DNN_YOLO_MULTI_MAX_BOXES, INT_MAX, multi_workspace, launch_yolo_multi};

static int launch_yolo_multi(const MultiCall& c, hipStream_t stream) {
  MultiArgs a;
  const int go = check_multi_call(c, MULTI, false, &a);
  if (go <= 0) return go;
  // with one class the rules and the label modes are the same function: the class-agnostic kernel
  // serves them all
  const bool per_class = c.nms_mode == DNN_YOLO_NMS_PER_CLASS && c.m->scale[0].n_classes > 1;
  const auto kernel = !per_class                                ? yolo_multi_kernel
                      : c.labels_mode == DNN_YOLO_LABELS_MULTI ? yolo_multi_labels_kernel
                                                                : yolo_multi_classwise_kernel;
  hipLaunchKernelGGL(kernel, dim3(c.n_images), dim3(PM_THREADS), 0, stream, *c.m, a.xy, a.mp, c.dets, c.max_det,
                     c.counts, static_cast<char*>(c.workspace), a.nb);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("launch yolo_multi: %s", hipGetErrorString(e));
    return -1;
  }
  return 0;
}

// the *_boxes and *_workspace entries: < 0 with the error set, else the boxes of one image
static int multi_boxes(const dnn_yolo_multi* m, const char* who) {
  return multi_boxes_upto(m, who, DNN_YOLO_MULTI_MAX_BOXES);
}

// (the description is checked first, then the entry's mode argument by mode_ok, if it has one)
static int multi_workspace_entry(const char* who, const dnn_yolo_multi* m, int n_images,
                                 bool (*mode_ok)(int, const char*), int mode, unsigned long long* bytes) {
  const int nb = multi_boxes(m, who);
  if (nb < 0) return nb;
  if (mode_ok && !mode_ok(mode, who)) return -2;
  DNN_REQUIRE(n_images >= 0 && bytes, "%s: bad arguments (n_images=%d)", who, n_images);
  *bytes = multi_workspace(nb, n_images);  // every kernel: 40 bytes per box
  return 0;
}

}  // namespace dnnhip

extern "C" {

using dnnhip::MULTI;

int dnn_yolo_multi_boxes(const dnn_yolo_multi* m) { return dnnhip::multi_boxes(m, "dnn_yolo_multi_boxes"); }

int dnn_yolo_multi_workspace(const dnn_yolo_multi* m, int n_images, unsigned long long* bytes) {
  return dnnhip::multi_workspace_entry("dnn_yolo_multi_workspace", m, n_images, nullptr, 0, bytes);
}

int dnn_yolo_postprocess_multi(const dnn_yolo_multi* m, const float* const* pred, int n_images, dnn_detection* dets,
                               int max_det, int* counts, void* workspace, unsigned long long workspace_bytes,
                               void* stream) {
  return MULTI.launch({"dnn_yolo_postprocess_multi", m, nullptr, pred, n_images, dets, max_det, counts, workspace,
                       workspace_bytes, DNN_YOLO_NMS_ANY_CLASS, DNN_YOLO_LABELS_ARGMAX},
                      static_cast<hipStream_t>(stream));
}

int dnn_yolo_postprocess_multi_host(const dnn_yolo_multi* m, const float* const* pred, int n_images,
                                    dnn_detection* dets, int max_det, int* counts) {
  return dnnhip::yolo_multi_host({"dnn_yolo_postprocess_multi_host", m, nullptr, pred, n_images, dets, max_det, counts,
                                  nullptr, 0, DNN_YOLO_NMS_ANY_CLASS, DNN_YOLO_LABELS_ARGMAX}, MULTI);
}

int dnn_yolo_multi_nms_workspace(const dnn_yolo_multi* m, int n_images, int nms_mode, unsigned long long* bytes) {
  return dnnhip::multi_workspace_entry("dnn_yolo_multi_nms_workspace", m, n_images, dnnhip::nms_mode_ok, nms_mode,
                                       bytes);
}

int dnn_yolo_postprocess_multi_nms(const dnn_yolo_multi* m, const float* const* pred, int n_images,
                                   dnn_detection* dets, int max_det, int* counts, void* workspace,
                                   unsigned long long workspace_bytes, int nms_mode, void* stream) {
  return MULTI.launch({"dnn_yolo_postprocess_multi_nms", m, nullptr, pred, n_images, dets, max_det, counts, workspace,
                       workspace_bytes, nms_mode, DNN_YOLO_LABELS_ARGMAX}, static_cast<hipStream_t>(stream));
}

int dnn_yolo_postprocess_multi_nms_host(const dnn_yolo_multi* m, const float* const* pred, int n_images,
                                        dnn_detection* dets, int max_det, int* counts, int nms_mode) {
  return dnnhip::yolo_multi_host({"dnn_yolo_postprocess_multi_nms_host", m, nullptr, pred, n_images, dets, max_det,
                                  counts, nullptr, 0, nms_mode, DNN_YOLO_LABELS_ARGMAX}, MULTI);
}

int dnn_yolo_multi_labels_workspace(const dnn_yolo_multi* m, int n_images, int labels_mode,
                                    unsigned long long* bytes) {
  return dnnhip::multi_workspace_entry("dnn_yolo_multi_labels_workspace", m, n_images, dnnhip::labels_mode_ok,
                                       labels_mode, bytes);
}

int dnn_yolo_postprocess_multi_labels(const dnn_yolo_multi* m, const float* const* pred, int n_images,
                                      dnn_detection* dets, int max_det, int* counts, void* workspace,
                                      unsigned long long workspace_bytes, int labels_mode, void* stream) {
  return MULTI.launch({"dnn_yolo_postprocess_multi_labels", m, nullptr, pred, n_images, dets, max_det, counts, workspace,
                       workspace_bytes, DNN_YOLO_NMS_PER_CLASS, labels_mode}, static_cast<hipStream_t>(stream));
}

int dnn_yolo_postprocess_multi_labels_host(const dnn_yolo_multi* m, const float* const* pred, int n_images,
                                           dnn_detection* dets, int max_det, int* counts, int labels_mode) {
  return dnnhip::yolo_multi_host({"dnn_yolo_postprocess_multi_labels_host", m, nullptr, pred, n_images, dets, max_det,
                                  counts, nullptr, 0, DNN_YOLO_NMS_PER_CLASS, labels_mode}, MULTI);
}

int dnn_yolo_postprocess_multi_xy(const dnn_yolo_multi* m, const float* scale_x_y, const float* const* pred,
                                  int n_images, dnn_detection* dets, int max_det, int* counts, void* workspace,
                                  unsigned long long workspace_bytes, int nms_mode, int labels_mode, void* stream) {
  return MULTI.launch({"dnn_yolo_postprocess_multi_xy", m, scale_x_y, pred, n_images, dets, max_det, counts, workspace,
                       workspace_bytes, nms_mode, labels_mode}, static_cast<hipStream_t>(stream));
}

int dnn_yolo_postprocess_multi_xy_host(const dnn_yolo_multi* m, const float* scale_x_y, const float* const* pred,
                                       int n_images, dnn_detection* dets, int max_det, int* counts, int nms_mode,
                                       int labels_mode) {
  return dnnhip::yolo_multi_host({"dnn_yolo_postprocess_multi_xy_host", m, scale_x_y, pred, n_images, dets, max_det,
                                  counts, nullptr, 0, nms_mode, labels_mode}, MULTI);
}

}  // extern "C"
