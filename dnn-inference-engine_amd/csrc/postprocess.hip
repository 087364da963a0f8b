// YOLOv2 postprocessing on the GPU (include/dnn_hip_post.h): the reference's host-side
// decode + threshold + sort + greedy NMS (cs492-projects/proj3/yolov2tiny.py:94-234) as one
// workgroup per image, so a batch leaves the GPU as a few kB of detections instead of
// 84.5 kB of raw predictions per image.
//
//   phase 1  thread per box (845): fp32 decode exactly as the reference evaluates it under
//            numpy (weak Python scalars: everything stays fp32; softmax sum in numpy's
//            8-accumulator pairwise order); every box's corners are truncated to int64
//            (non-finite / huge -> the image is flagged, as int() raises in the reference);
//            boxes above the threshold append a sort key to LDS
//   phase 2  bitonic sort of the keys (score descending, then box index = Python's stable
//            sort of the (row, col, anchor)-ordered list)
//   phase 3  greedy NMS as a bitmask: every wave fills rows of S[i][j] = IoU(i, j) > 0.3 for
//            j < i (64 pairs per wave step, ballot into one word), then one wave walks the
//            candidates in order with the keep mask in registers (lane w holds word w):
//            candidate i is dropped iff S[i] & keep != 0 — the reference's "IoU with ANY kept
//            box" (yolov2tiny.py:197-226).  IoU is the reference's integer formula (+1 widths,
//            negative overlaps not clamped) in exact 64/128-bit integers, converted to double
//            with correct rounding like Python's int -> float.
//
// The key, the sort, the row emit and the anchor table are post_dev.h's (key_any, bitonic_sort,
// emit_row, VOC_ANCHORS), shared with every other decode.  This kernel's own: the softmax over a
// register array (20 classes fit; post_dev.h's class_argmax reads memory three times), the full
// suppression bitmask (845 x 14 words fit in LDS), and its copy of decode_corners' arithmetic:
// with the call the compiler schedules the whole decode loop of this kernel, the benchmark's,
// differently, so the seven lines stay here, split around the class loop.
//
// This file also defines the host staging of the two single-scale host entries.
#include "post_dev.h"

namespace dnnhip {

constexpr int PP_THREADS = 512;
constexpr int PP_WAVES = PP_THREADS / 64;
constexpr int PP_WORDS = (DNN_YOLO_BOXES + 63) / 64;  // 14 keep / suppression words
constexpr int PP_SORT = 1024;  // >= DNN_YOLO_BOXES, power of two

// numpy's float32 add.reduce of a contiguous 20-vector: 8 partial sums over the first 16,
// combined pairwise, then the 4 tail elements in order
__device__ __forceinline__ float pairwise_sum20(const float* e) {
  float r[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) r[j] = e[j] + e[8 + j];
  float s = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
#pragma unroll
  for (int j = 16; j < 20; ++j) s = s + e[j];
  return s;
}

__global__ void __launch_bounds__(PP_THREADS)
yolo_postprocess_kernel(const float* __restrict__ pred, dnn_detection* __restrict__ dets, int max_det,
                        int* __restrict__ counts) {
  __shared__ unsigned long long keys[PP_SORT];
  __shared__ long long box[DNN_YOLO_BOXES][4];
  __shared__ float score_of[DNN_YOLO_BOXES];
  __shared__ int cls_of[DNN_YOLO_BOXES];
  __shared__ unsigned long long sup[DNN_YOLO_BOXES][PP_WORDS];  // S[i][w]: bits j = 64w.. < i
  __shared__ unsigned char zrow[DNN_YOLO_BOXES];               // row i has a zero IoU denominator
  __shared__ int n_cand, bad;

  const int img = blockIdx.x, tid = threadIdx.x;
  const float* p = pred + (size_t)img * DNN_YOLO_BOXES * 25;
  if (tid == 0) {
    n_cand = 0;
    bad = 0;
  }
  for (int i = tid; i < PP_SORT; i += PP_THREADS) keys[i] = ~0ull;
  __syncthreads();

  // ---- phase 1: decode (yolov2tiny.py:113-143)
  for (int k = tid; k < DNN_YOLO_BOXES; k += PP_THREADS) {
    const float* q = p + k * 25;
    const int b = k % 5, cell = k / 5, col = cell % 13, row = cell / 13;
    // (decode_corners' arithmetic, kept as this kernel's own copy around the class loop: see above)
    const float cx = ((float)col + sigmoid_ref(q[0])) * 32.0f;
    const float cy = ((float)row + sigmoid_ref(q[1])) * 32.0f;
    const float rw = (np_expf(q[2]) * VOC_ANCHORS[2 * b]) * 32.0f;
    const float rh = (np_expf(q[3]) * VOC_ANCHORS[2 * b + 1]) * 32.0f;
    const float conf = sigmoid_ref(q[4]);
    float m = q[5];
#pragma unroll
    for (int c = 1; c < 20; ++c) m = q[5 + c] > m ? q[5 + c] : m;
    float e[20];
#pragma unroll
    for (int c = 0; c < 20; ++c) e[c] = np_expf(q[5 + c] - m);
    const float s = pairwise_sum20(e);
    int best = 0;
    float bp = e[0] / s;
#pragma unroll
    for (int c = 1; c < 20; ++c) {
      const float pc = e[c] / s;
      if (pc > bp) {  // first index of the max
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
    if (sc > 0.3f) {  // float32 comparison, as numpy compares a float32 with a Python float
      const int pos = atomicAdd(&n_cand, 1);
      keys[pos] = key_any(sc, k);
    }
  }
  __syncthreads();
  const int n = n_cand;
  if (bad) {
    if (tid == 0) counts[img] = -1;
    return;
  }

  // ---- phase 2: bitonic sort of the first pow2 >= n keys (yolov2tiny.py:146)
  int ns = 1;
  while (ns < n) ns <<= 1;
  bitonic_sort<PP_THREADS>(keys, ns, tid);

  // ---- phase 3a: suppression bitmask, all waves (yolov2tiny.py:197-216 evaluates every pair
  // (candidate i, kept j < i); here every pair j < i, the keep mask selects below)
  const int lane = tid & 63, wid = tid >> 6;
  for (int i = wid; i < n; i += PP_WAVES) {
    const int ki = key_any_index(keys[i]);
    const long long bi[4] = {box[ki][0], box[ki][1], box[ki][2], box[ki][3]};
    bool zany = false;
    for (int w = 0; w * 64 < i; ++w) {
      const int j = w * 64 + lane;
      bool hit = false;
      if (j < i) hit = iou_gt(bi, box[key_any_index(keys[j])], 0.3, &zany);
      const unsigned long long m = __ballot(hit);
      if (lane == 0) sup[i][w] = m;
    }
    const bool z = __any(zany);
    if (lane == 0) zrow[i] = z ? 1 : 0;
  }
  __syncthreads();

  // ---- phase 3b: greedy walk in wave 0, keep word w in lane w
  if (tid < 64) {
    unsigned long long kw = 0;
    bool zero_hit = false;
    for (int i = 0; i < n; ++i) {
      const int nwi = (i + 63) >> 6;  // words holding j < i
      const unsigned long long row = lane < nwi ? sup[i][lane] : 0ull;
      const bool drop = __any((row & kw) != 0ull);
      if (zrow[i]) {  // rare: a zero IoU denominator against a KEPT box raises in the reference
        const int ki = key_any_index(keys[i]);
        bool zd = false;
        for (unsigned long long bits = lane < nwi ? kw : 0ull; bits; bits &= bits - 1) {
          const int j = lane * 64 + __builtin_ctzll(bits);
          (void)iou_gt(box[ki], box[key_any_index(keys[j])], 0.3, &zd);
        }
        zero_hit |= zd;
      }
      if (!drop && lane == (i >> 6)) kw |= 1ull << (i & 63);
    }
    if (__any(zero_hit)) {
      if (lane == 0) counts[img] = -2;
      return;
    }
    // output in candidate order: exclusive prefix of the per-word popcounts
    const int cnt = __popcll(kw);
    int incl = cnt;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int v = __shfl_up(incl, d);
      if (lane >= d) incl += v;
    }
    const int nk = __shfl(incl, 63);
    int r = incl - cnt;
    for (unsigned long long bits = kw; bits; bits &= bits - 1, ++r) {
      const int i = lane * 64 + __builtin_ctzll(bits);
      if (r >= max_det) break;
      const int k = key_any_index(keys[i]);
      emit_row(dets + (size_t)img * max_det + r, cls_of[k], score_of[k], box[k]);
    }
    if (lane == 0) counts[img] = nk;
  }
}

// Image-major compaction of the per-image detection lists: packed = concat_i dets[i][:counts[i]]
// (error images contribute nothing), total[0] = rows written.  One workgroup: a serial
// prefix over the counts in LDS chunks, then all threads copy rows.
__global__ void __launch_bounds__(PP_THREADS)
yolo_pack_kernel(const dnn_detection* __restrict__ dets, const int* __restrict__ counts, int n, int max_det,
                 dnn_detection* __restrict__ packed, int* __restrict__ total) {
  __shared__ int off[PP_THREADS + 1];
  int base = 0;
  for (int c0 = 0; c0 < n; c0 += PP_THREADS) {
    const int i = c0 + threadIdx.x;
    int c = i < n ? counts[i] : 0;
    c = c < 0 ? 0 : (c > max_det ? max_det : c);
    off[threadIdx.x + 1] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
      off[0] = base;
      for (int k = 1; k <= PP_THREADS; ++k) off[k] += off[k - 1];
    }
    __syncthreads();
    const int lo = off[0], hi = off[PP_THREADS];
    // row r of this chunk's output belongs to the image whose [off[t], off[t+1]) holds it
    for (int r = lo + threadIdx.x; r < hi; r += PP_THREADS) {
      int t = 0, h = PP_THREADS;  // binary search: last t with off[t] <= r
      while (h - t > 1) {
        const int m = (t + h) >> 1;
        if (off[m] <= r) t = m; else h = m;
      }
      packed[r] = dets[(size_t)(c0 + t) * max_det + (r - off[t])];
    }
    base = hi;
    __syncthreads();
  }
  if (threadIdx.x == 0) total[0] = base;
}

int launch_yolo_pack(const dnn_detection* dets, const int* counts, int n, int max_det, dnn_detection* packed,
                     int* total, hipStream_t stream) {
  if (n < 0 || max_det < 0 || !total || (n > 0 && (!counts || (max_det > 0 && (!dets || !packed))))) {
    set_error("dnn_yolo_pack_detections: bad arguments (n=%d max_det=%d)", n, max_det);
    return -2;
  }
  hipLaunchKernelGGL(yolo_pack_kernel, dim3(1), dim3(PP_THREADS), 0, stream, dets, counts, n, max_det, packed,
                     total);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("launch yolo_pack: %s", hipGetErrorString(e));
    return -1;
  }
  return 0;
}

int launch_yolo_postprocess(const float* pred, int n_images, dnn_detection* dets, int max_det, int* counts,
                            hipStream_t stream) {
  if (n_images == 0) return 0;
  if (n_images < 0 || max_det < 0 || !pred || !counts || (max_det > 0 && !dets)) {
    set_error("dnn_yolo_postprocess: bad arguments (n_images=%d max_det=%d)", n_images, max_det);
    return -2;
  }
  hipLaunchKernelGGL(yolo_postprocess_kernel, dim3(n_images), dim3(PP_THREADS), 0, stream, pred, dets, max_det,
                     counts);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("launch yolo_postprocess: %s", hipGetErrorString(e));
    return -1;
  }
  return 0;
}

int yolo_single_host(const SingleCall& c, const float* pred, size_t pred_bytes, dnn_detection* dets, size_t det_bytes,
                     int* counts, size_t count_bytes, SingleLaunch launch) {
  const size_t pb = (pred_bytes + 7) & ~(size_t)7;  // keeps dets and the workspace 8-byte aligned
  const size_t cb = (count_bytes + 7) & ~(size_t)7;
  char* buf = nullptr;
  DNN_HIP_TRY(hipMalloc(&buf, pb + det_bytes + cb + c.ws_bytes));
  dnn_detection* d_dets = reinterpret_cast<dnn_detection*>(buf + pb);
  int* d_counts = reinterpret_cast<int*>(buf + pb + det_bytes);
  int rc = 0;
  if (hipMemcpy(buf, pred, pred_bytes, hipMemcpyHostToDevice) != hipSuccess) {
    set_error("%s: copy in failed", c.who);
    rc = -1;
  }
  if (!rc)
    rc = launch(c, reinterpret_cast<const float*>(buf), d_dets, d_counts,
                c.ws_bytes ? buf + pb + det_bytes + cb : nullptr);
  if (!rc && (hipMemcpy(counts, d_counts, count_bytes, hipMemcpyDeviceToHost) != hipSuccess ||
              (det_bytes && hipMemcpy(dets, d_dets, det_bytes, hipMemcpyDeviceToHost) != hipSuccess))) {
    set_error("%s: copy out failed", c.who);
    rc = -1;
  }
  (void)hipFree(buf);
  return rc;
}

}  // namespace dnnhip

extern "C" {

int dnn_yolo_postprocess(const float* pred, int n_images, dnn_detection* dets, int max_det, int* counts,
                         void* stream) {
  return dnnhip::launch_yolo_postprocess(pred, n_images, dets, max_det, counts, static_cast<hipStream_t>(stream));
}

int dnn_yolo_pack_detections(const dnn_detection* dets, const int* counts, int n_images, int max_det,
                             dnn_detection* packed, int* total, void* stream) {
  return dnnhip::launch_yolo_pack(dets, counts, n_images, max_det, packed, total, static_cast<hipStream_t>(stream));
}

int dnn_yolo_postprocess_host(const float* pred, int n_images, dnn_detection* dets, int max_det, int* counts) {
  DNN_REQUIRE(n_images >= 0 && max_det >= 0, "dnn_yolo_postprocess_host: bad arguments");
  if (n_images == 0) return 0;
  DNN_REQUIRE(pred && counts && (max_det == 0 || dets), "dnn_yolo_postprocess_host: NULL pointer");
  return dnnhip::yolo_single_host(
      {"dnn_yolo_postprocess_host", nullptr, n_images, max_det, 0}, pred,
      (size_t)n_images * DNN_YOLO_BOXES * 25 * sizeof(float), dets, (size_t)n_images * max_det * sizeof(dnn_detection),
      counts, (size_t)n_images * sizeof(int),
      [](const dnnhip::SingleCall& c, const float* d_pred, dnn_detection* d_dets, int* d_counts, void*) {
        return dnnhip::launch_yolo_postprocess(d_pred, c.n_images, d_dets, c.max_det, d_counts, nullptr);
      });
}

}  // extern "C"
