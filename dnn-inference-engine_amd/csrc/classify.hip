// The tail of a Darknet classifier (darknet19.cfg, darknet53.cfg: ... [avgpool] [convolutional 1x1]
// [softmax]) and the top-k that reads it, fp32 NHWC, no atomics, every tensor below 2 GiB.
//
// Global average pool (Darknet's forward_avgpool_layer: the sum over the h * w positions, then one
// division by h * w).  a [n, H, W, C] -> out [n, 1, 1, C].  A workgroup of four waves owns one image and
// one block of 64 lanes' channels: with C % 4 == 0 a lane owns four consecutive channels (one 16-byte
// load per position, a wave 1 KB contiguous, the block 256 channels), otherwise one channel (the block
// 64 channels).  Wave w sums positions w, w + 4, w + 8, ... in that order into one accumulator per
// channel; the four partials go through LDS and wave 0 adds them in wave order, divides once and
// stores.  The order is a function of (H, W) alone and the same in both variants, so an image's bits
// do not depend on the batch or on its place in it.
//
// Softmax (Darknet's softmax(), temperature 1, one group): p_j = exp(x_j - max x) / sum_k exp(x_k - max x).
// One workgroup per image.  The row is loaded once into LDS (16-byte loads when classes % 4 == 0 and
// the tensor is 16-byte aligned); the max, expf in place, the sum and the store pass e / sum (a true
// division per element, not a multiplication by the reciprocal) all run on that copy.  A thread owns
// elements tid, tid + T, ... in the passes between the barriers; reductions are classify_dev.h's.
// Rows up to 4,096 classes take 256 threads and 16 KB of LDS (several workgroups per CU), longer rows
// up to DNN_SOFTMAX_MAX_CLASSES = 32,768 (128 KB of the CU's 160 KB) take 1,024 threads.
//
// Top-k: per image the k largest entries of a score row (probabilities or logits), descending, ties to
// the lower index.  The same staging.  Each thread keeps the best of its own elements in registers; a
// round is one workgroup-wide (value, index) arg-max, thread 0 writes the winner, and the winner's owner
// marks it taken in LDS and rescans its own elements, so a round costs one barrier.  The mark is a NaN:
// a row that holds a NaN is refused up front (status[i] = DNN_TOPK_NAN, no rows written), which leaves
// NaN free as a mark, where -inf would collide with a -inf score (the log of a zero probability).
#include <hip/hip_runtime.h>
#include <cmath>
#include "classify_dev.h"
#include "dnn_common.h"
#include "../../include/dnn_hip_plan.h"
#include "../../include/dnn_hip_post.h"

namespace dnnhip {

constexpr int AVG_WAVES = 4;
constexpr int AVG_THREADS = AVG_WAVES * CLS_WAVE;

template <int VEC>
struct AvgVec;
template <>
struct AvgVec<4> {
  typedef cls_f32x4 type;
};
template <>
struct AvgVec<1> {
  typedef float type;
};

// workgroup -> (image, block of 64 * VEC channels); C % VEC == 0
template <int VEC>
__global__ void __launch_bounds__(AVG_THREADS)
avgpool_kernel(const float* __restrict__ a, float* __restrict__ out, int HW, int C, int cblocks) {
  typedef typename AvgVec<VEC>::type vec_t;
  __shared__ vec_t part[AVG_WAVES][CLS_WAVE];
  const int lane = threadIdx.x & (CLS_WAVE - 1), wave = threadIdx.x / CLS_WAVE;
  const int img = blockIdx.x / cblocks, cb = blockIdx.x - img * cblocks;
  const int ch = (cb * CLS_WAVE + lane) * VEC;
  const bool ok = ch < C;
  vec_t acc = 0.0f;
  if (ok) {
    const float* src = a + (size_t)img * HW * C + ch;
#pragma unroll 4
    for (int p = wave; p < HW; p += AVG_WAVES) acc += *reinterpret_cast<const vec_t*>(src + (size_t)p * C);
  }
  part[wave][lane] = acc;
  __syncthreads();
  if (wave == 0 && ok) {
    vec_t s = part[0][lane];
#pragma unroll
    for (int w = 1; w < AVG_WAVES; ++w) s += part[w][lane];
    *reinterpret_cast<vec_t*>(out + (size_t)img * C + ch) = s / (float)HW;
  }
}

constexpr int ROW_SMALL = 4096;  // rows up to here: 256 threads, 16 KB
constexpr int row_threads(int cap) { return cap > ROW_SMALL ? 1024 : 256; }

template <int CAP>
__global__ void __launch_bounds__(row_threads(CAP))
softmax_kernel(const float* __restrict__ in, float* __restrict__ out, int classes, int vec) {
  __shared__ __attribute__((aligned(16))) float row[CAP];
  __shared__ float red_max[CLS_MAX_WAVES], red_sum[CLS_MAX_WAVES];
  const int tid = threadIdx.x, T = blockDim.x;
  stage_row(in + (size_t)blockIdx.x * classes, row, classes, vec != 0);
  __syncthreads();
  float m = -INFINITY;
  for (int i = tid; i < classes; i += T) m = ClsMax::apply(m, row[i]);
  m = block_reduce<ClsMax>(m, red_max);
  float s = 0.0f;
  for (int i = tid; i < classes; i += T) {
    const float e = expf(row[i] - m);
    row[i] = e;
    s += e;
  }
  s = block_reduce<ClsSum>(s, red_sum);  // (its barrier also publishes the e's)
  float* dst = out + (size_t)blockIdx.x * classes;
  if (vec) {
    const cls_f32x4* r4 = reinterpret_cast<const cls_f32x4*>(row);
    cls_f32x4* d4 = reinterpret_cast<cls_f32x4*>(dst);
    for (int q = tid; q < (classes >> 2); q += T) d4[q] = r4[q] / s;
  } else {
    for (int i = tid; i < classes; i += T) dst[i] = row[i] / s;
  }
}

template <int CAP>
__global__ void __launch_bounds__(row_threads(CAP))
topk_kernel(const float* __restrict__ scores, int classes, int k, int vec, int* __restrict__ out_index,
            float* __restrict__ out_score, int* __restrict__ status) {
  __shared__ __attribute__((aligned(16))) float row[CAP];
  __shared__ float red_v[2][CLS_MAX_WAVES];
  __shared__ int red_i[2][CLS_MAX_WAVES];
  __shared__ int has_nan;
  const int tid = threadIdx.x, T = blockDim.x, img = blockIdx.x;
  if (tid == 0) has_nan = 0;
  stage_row(scores + (size_t)img * classes, row, classes, vec != 0);
  __syncthreads();
  // the best of this thread's own elements (tid, tid + T, ...: ascending, so a tie keeps the lower index)
  float bv = -INFINITY;
  int bi = INT_MAX;
  bool nan = false;
  for (int i = tid; i < classes; i += T) {
    const float v = row[i];
    nan = nan || v != v;
    if (cls_better(v, i, bv, bi)) bv = v, bi = i;
  }
  if (nan) has_nan = 1;
  __syncthreads();
  if (has_nan) {
    if (tid == 0) status[img] = DNN_TOPK_NAN;
    return;
  }
  for (int r = 0; r < k; ++r) {  // (round r + 2 reuses round r's partials: every thread has passed round r + 1's barrier)
    float gv = bv;
    int gi = bi;
    block_argmax(gv, gi, red_v[r & 1], red_i[r & 1]);
    if (tid == 0) {
      out_index[(size_t)img * k + r] = gi;
      out_score[(size_t)img * k + r] = gv;
    }
    if (gi % T == tid) {  // the owner: only it reads these elements again
      row[gi] = NAN;
      bv = -INFINITY;
      bi = INT_MAX;
      for (int i = tid; i < classes; i += T)
        if (cls_better(row[i], i, bv, bi)) bv = row[i], bi = i;
    }
  }
  if (tid == 0) status[img] = 0;
}

static int launched(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("launch %s: %s", what, hipGetErrorString(e));
    return -1;
  }
  return 0;
}

static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

int launch_avgpool(const float* in, float* out, int n, int H, int W, int C, hipStream_t stream) {
  DNN_REQUIRE(in && out, "launch_avgpool: NULL tensor");
  DNN_REQUIRE(n >= 0 && H > 0 && W > 0 && C > 0, "launch_avgpool: bad shape n=%d %dx%dx%d", n, H, W, C);
  DNN_REQUIRE((unsigned long long)n * H * W * C * 4 < 0x80000000ULL,
              "launch_avgpool: the input n=%d %dx%dx%d is >= 2 GiB; split the batch", n, H, W, C);
  DNN_REQUIRE(out != in, "launch_avgpool: out may not alias the input");
  if (n == 0) return 0;
  const bool vec4 = C % 4 == 0 && aligned16(in) && aligned16(out);
  const int per_block = CLS_WAVE * (vec4 ? 4 : 1);
  const int cblocks = (C + per_block - 1) / per_block;
  const dim3 grid((unsigned)((long long)n * cblocks));  // (< 2^29: a workgroup reads at least one float)
  if (vec4)
    hipLaunchKernelGGL(avgpool_kernel<4>, grid, dim3(AVG_THREADS), 0, stream, in, out, H * W, C, cblocks);
  else
    hipLaunchKernelGGL(avgpool_kernel<1>, grid, dim3(AVG_THREADS), 0, stream, in, out, H * W, C, cblocks);
  return launched("avgpool");
}

// the checks launch_softmax and launch_topk share (0, or -2 with the error set)
static int row_shape_ok(const char* who, const void* in, int n, int classes) {
  DNN_REQUIRE(in, "%s: NULL tensor", who);
  DNN_REQUIRE(n >= 0 && classes >= 1, "%s: bad shape n=%d classes=%d", who, n, classes);
  DNN_REQUIRE(classes <= DNN_SOFTMAX_MAX_CLASSES,
              "%s: a row of %d classes does not fit the workgroup's LDS (at most DNN_SOFTMAX_MAX_CLASSES = %d)", who,
              classes, DNN_SOFTMAX_MAX_CLASSES);
  DNN_REQUIRE((unsigned long long)n * classes * 4 < 0x80000000ULL, "%s: n=%d rows of %d classes are >= 2 GiB", who, n,
              classes);
  return 0;
}

int launch_softmax(const float* in, float* out, int n, int classes, hipStream_t stream) {
  if (int rc = row_shape_ok("launch_softmax", in, n, classes)) return rc;
  DNN_REQUIRE(out, "launch_softmax: NULL tensor");
  if (n == 0) return 0;
  const int vec = classes % 4 == 0 && aligned16(in) && aligned16(out) ? 1 : 0;
  if (classes <= ROW_SMALL)
    hipLaunchKernelGGL(softmax_kernel<ROW_SMALL>, dim3(n), dim3(row_threads(ROW_SMALL)), 0, stream, in, out, classes,
                       vec);
  else
    hipLaunchKernelGGL(softmax_kernel<DNN_SOFTMAX_MAX_CLASSES>, dim3(n), dim3(row_threads(DNN_SOFTMAX_MAX_CLASSES)), 0,
                       stream, in, out, classes, vec);
  return launched("softmax");
}

int launch_topk(const float* scores, int n, int classes, int k, int* out_index, float* out_score, int* status,
                hipStream_t stream) {
  if (int rc = row_shape_ok("launch_topk", scores, n, classes)) return rc;
  DNN_REQUIRE(k >= 1 && k <= DNN_TOPK_MAX && k <= classes, "launch_topk: k = %d outside 1..min(DNN_TOPK_MAX = %d, %d classes)",
              k, DNN_TOPK_MAX, classes);
  DNN_REQUIRE(out_index && out_score && status, "launch_topk: NULL output");
  if (n == 0) return 0;
  const int vec = classes % 4 == 0 && aligned16(scores) ? 1 : 0;
  if (classes <= ROW_SMALL)
    hipLaunchKernelGGL(topk_kernel<ROW_SMALL>, dim3(n), dim3(row_threads(ROW_SMALL)), 0, stream, scores, classes, k, vec,
                       out_index, out_score, status);
  else
    hipLaunchKernelGGL(topk_kernel<DNN_SOFTMAX_MAX_CLASSES>, dim3(n), dim3(row_threads(DNN_SOFTMAX_MAX_CLASSES)), 0,
                       stream, scores, classes, k, vec, out_index, out_score, status);
  return launched("topk");
}

}  // namespace dnnhip

using namespace dnnhip;

extern "C" {

int dnn_classify_topk(const float* scores, int n_images, int classes, int k, int* index, float* score, int* status,
                      void* stream) {
  return launch_topk(scores, n_images, classes, k, index, score, status, static_cast<hipStream_t>(stream));
}

int dnn_classify_topk_host(const float* scores, int n_images, int classes, int k, int* index, float* score,
                           int* status) {
  if (int rc = row_shape_ok("dnn_classify_topk_host", scores, n_images, classes)) return rc;
  DNN_REQUIRE(k >= 1 && k <= DNN_TOPK_MAX && k <= classes,
              "dnn_classify_topk_host: k = %d outside 1..min(DNN_TOPK_MAX = %d, %d classes)", k, DNN_TOPK_MAX, classes);
  DNN_REQUIRE(index && score && status, "dnn_classify_topk_host: NULL output");
  if (n_images == 0) return 0;
  // one allocation: the scores, then per image k scores, k indices and the status (4-byte words all)
  const size_t in_w = (size_t)n_images * classes, out_w = (size_t)n_images * k;
  float* d = nullptr;
  DNN_HIP_TRY(hipMalloc(&d, (in_w + 2 * out_w + n_images) * 4));
  float* d_score = d + in_w;
  int* d_index = reinterpret_cast<int*>(d_score + out_w);
  int* d_status = d_index + out_w;
  // rows of a refused image are not written: the caller's buffers keep what they held
  int rc = hipMemcpy(d, scores, in_w * 4, hipMemcpyHostToDevice) == hipSuccess &&
                   hipMemcpy(d_score, score, out_w * 4, hipMemcpyHostToDevice) == hipSuccess &&
                   hipMemcpy(d_index, index, out_w * 4, hipMemcpyHostToDevice) == hipSuccess
               ? 0
               : -1;
  if (rc) set_error("dnn_classify_topk_host: host to device copy failed");
  if (!rc) rc = launch_topk(d, n_images, classes, k, d_index, d_score, d_status, nullptr);
  if (!rc && !(hipMemcpy(score, d_score, out_w * 4, hipMemcpyDeviceToHost) == hipSuccess &&
               hipMemcpy(index, d_index, out_w * 4, hipMemcpyDeviceToHost) == hipSuccess &&
               hipMemcpy(status, d_status, (size_t)n_images * 4, hipMemcpyDeviceToHost) == hipSuccess)) {
    set_error("dnn_classify_topk_host: device to host copy failed (%s)", hipGetErrorString(hipGetLastError()));
    rc = -1;
  }
  (void)hipFree(d);
  return rc;
}

}  // extern "C"
