// Shortcut (residual add) and nearest-neighbour upsample: the two joins of detection backbones
// after YOLOv2 (Darknet-53's y = x + f(x), the top-down merge's upsample + concat).  The reference
// has neither node.  All tensors NHWC fp32, each below 2 GiB (element offsets fit an int).
//
//   shortcut   out[i] = act(a[i] + b[i]): one fp32 add, rounded once, then the conv epilogue's
//              leaky (apply_leaky, dnn_common.h) or nothing.  16 B per lane on all three tensors,
//              a grid sized to the chip and a grid-stride loop with four vectors of each input
//              in flight per lane; a scalar loop covers the last n % 4 elements (and everything
//              when a pointer is not 16-byte aligned).  out must not alias a or b.
//   upsample   out[n, h, w, c] = in[n, h / f, w / f, c].  Organised by source pixel, in route.hip's
//              style: a workgroup owns a chunk of consecutive source pixels and tabulates in LDS
//              the offset of each one's first destination (the (n, h, w) decomposition: once per
//              pixel); a thread resolves its channel column once, reads the source vector once and
//              stores it to the f x f destinations by adding constant strides.  VEC = 4 moves 16 B
//              per lane (C % 4 == 0, 16-byte aligned tensors), VEC = 1 covers every other C.
#include <hip/hip_runtime.h>
#include <algorithm>
#include "dnn_common.h"

namespace dnnhip {

typedef float sc_f32x4 __attribute__((ext_vector_type(4)));

constexpr int SC_THREADS = 256;
constexpr int SC_UNROLL = 4;

template <int FLAGS>
__device__ __forceinline__ sc_f32x4 shortcut_vec(sc_f32x4 x, sc_f32x4 y) {
  sc_f32x4 r;
  r.x = apply_leaky(x.x + y.x, FLAGS);
  r.y = apply_leaky(x.y + y.y, FLAGS);
  r.z = apply_leaky(x.z + y.z, FLAGS);
  r.w = apply_leaky(x.w + y.w, FLAGS);
  return r;
}

// n4 whole 16-byte vectors, then elements [4 * n4, n) one by one
template <int FLAGS>
__global__ void __launch_bounds__(SC_THREADS)
shortcut_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ out, int n4, int n) {
  const sc_f32x4* a4 = reinterpret_cast<const sc_f32x4*>(a);
  const sc_f32x4* b4 = reinterpret_cast<const sc_f32x4*>(b);
  sc_f32x4* o4 = reinterpret_cast<sc_f32x4*>(out);
  const int stride = gridDim.x * SC_THREADS;  // (n4 < 2^27 and stride <= 2^19: no int overflow below)
  int i = blockIdx.x * SC_THREADS + threadIdx.x;
  for (; i + (SC_UNROLL - 1) * stride < n4; i += SC_UNROLL * stride) {
    sc_f32x4 x[SC_UNROLL], y[SC_UNROLL];
#pragma unroll
    for (int u = 0; u < SC_UNROLL; ++u) {
      x[u] = a4[i + u * stride];
      y[u] = b4[i + u * stride];
    }
#pragma unroll
    for (int u = 0; u < SC_UNROLL; ++u) o4[i + u * stride] = shortcut_vec<FLAGS>(x[u], y[u]);
  }
  for (; i < n4; i += stride) o4[i] = shortcut_vec<FLAGS>(a4[i], b4[i]);
  for (int j = 4 * n4 + blockIdx.x * SC_THREADS + threadIdx.x; j < n; j += stride)
    out[j] = apply_leaky(a[j] + b[j], FLAGS);
}

int launch_shortcut(const float* a, const float* b, float* out, long long count, int leaky, hipStream_t stream) {
  DNN_REQUIRE(a && b && out, "launch_shortcut: NULL tensor");
  DNN_REQUIRE(leaky >= 0 && leaky <= 2, "launch_shortcut: leaky must be 0, 1 or 2");
  DNN_REQUIRE(count >= 0 && (unsigned long long)count * 4 < 0x80000000ULL,
              "launch_shortcut: a tensor of %lld floats is >= 2 GiB; split the batch", count);
  DNN_REQUIRE(out != a && out != b, "launch_shortcut: out may not alias an input");
  if (count == 0) return 0;
  const int n = (int)count;
  const bool vec4 =
      ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(out)) & 15) == 0;
  const int n4 = vec4 ? n / 4 : 0;
  // one lane per vector up to the resident grid (8 workgroups per CU); the rest grid-strides
  const long long lanes = std::max<long long>(n4, n - 4LL * n4);
  const long long blocks = (lanes + SC_THREADS - 1) / SC_THREADS;
  const dim3 grid((unsigned)std::max<long long>(1, std::min<long long>(blocks, (long long)device_cu_count() * 8)));
  if (leaky == 1)
    hipLaunchKernelGGL(shortcut_kernel<EPI_LEAKY_F64>, grid, dim3(SC_THREADS), 0, stream, a, b, out, n4, n);
  else if (leaky == 2)
    hipLaunchKernelGGL(shortcut_kernel<EPI_LEAKY_F32>, grid, dim3(SC_THREADS), 0, stream, a, b, out, n4, n);
  else
    hipLaunchKernelGGL(shortcut_kernel<0>, grid, dim3(SC_THREADS), 0, stream, a, b, out, n4, n);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("launch shortcut: %s", hipGetErrorString(e));
    return -1;
  }
  return 0;
}

// ------------------------------------------------------------------------------------ upsample
template <int VEC>
struct UpVec;
template <>
struct UpVec<4> {
  typedef sc_f32x4 type;
};
template <>
struct UpVec<1> {
  typedef float type;
};

struct UpsampleGeom {
  int npix;     // source pixels: n * H * W
  int H, W, C;  // source
  int f;        // factor
  int cols;     // channel columns per pixel, in VEC units: C / VEC
  int qt_log2;  // threads over columns: QT = 1 << qt_log2 (<= 64), 256 / QT pixel lanes
  int chunk;    // source pixels per workgroup pass (<= UP_MAX_CHUNK)
};

constexpr int UP_MAX_CHUNK = 256;

template <int VEC>
__global__ void __launch_bounds__(SC_THREADS)
upsample_kernel(const float* __restrict__ in, float* __restrict__ out, UpsampleGeom g) {
  typedef typename UpVec<VEC>::type vec_t;
  __shared__ int dst_base[UP_MAX_CHUNK];  // float offset of out[n, h*f, w*f, 0]
  const int tid = threadIdx.x;
  const int QT = 1 << g.qt_log2, PT = SC_THREADS >> g.qt_log2;
  const int tq = tid & (QT - 1), tp = tid >> g.qt_log2;
  const int OW = g.W * g.f;
  const int row_step = OW * g.C;  // one destination row down
  for (int p0 = blockIdx.x * g.chunk; p0 < g.npix; p0 += gridDim.x * g.chunk) {
    const int np = min(g.chunk, g.npix - p0);
    __syncthreads();  // the previous pass has finished reading the table
    for (int p = tid; p < np; p += SC_THREADS) {
      const int pix = p0 + p;
      const int w = pix % g.W, nh = pix / g.W;  // nh = n * H + h: destination row nh * f
      dst_base[p] = (nh * g.f * OW + w * g.f) * g.C;
    }
    __syncthreads();
    for (int q = tq; q < g.cols; q += QT) {
      const float* src = in + (size_t)p0 * g.C + q * VEC;
      float* dst = out + q * VEC;
#pragma unroll 2
      for (int p = tp; p < np; p += PT) {
        const vec_t v = *reinterpret_cast<const vec_t*>(src + (size_t)p * g.C);
        float* d = dst + dst_base[p];
        for (int dy = 0; dy < g.f; ++dy, d += row_step) {
          float* e = d;
          for (int dx = 0; dx < g.f; ++dx, e += g.C) *reinterpret_cast<vec_t*>(e) = v;
        }
      }
    }
  }
}

static int up_log2_ceil(int v) {
  int l = 0;
  while ((1 << l) < v) ++l;
  return l;
}

int launch_upsample(const float* in, float* out, int n, int H, int W, int C, int factor, hipStream_t stream) {
  DNN_REQUIRE(in && out, "launch_upsample: NULL tensor");
  DNN_REQUIRE(n >= 0 && H > 0 && W > 0 && C > 0, "launch_upsample: bad shape n=%d %dx%dx%d", n, H, W, C);
  DNN_REQUIRE(factor >= 1 && factor <= 8, "launch_upsample: factor %d outside 1..8", factor);
  const long long npix = (long long)n * H * W;
  DNN_REQUIRE((unsigned long long)npix * C * factor * factor * 4 < 0x80000000ULL,
              "launch_upsample: the output of n=%d %dx%dx%d factor %d is >= 2 GiB; split the batch", n, H, W, C,
              factor);
  DNN_REQUIRE(out != in, "launch_upsample: out may not alias the input");
  if (npix == 0) return 0;
  const bool vec4 = C % 4 == 0 && ((reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(out)) & 15) == 0;
  const int vec = vec4 ? 4 : 1;
  UpsampleGeom g;
  g.npix = (int)npix;
  g.H = H;
  g.W = W;
  g.C = C;
  g.f = factor;
  g.cols = C / vec;
  g.qt_log2 = std::min(6, up_log2_ceil(g.cols));
  const int PT = SC_THREADS >> g.qt_log2;
  // a workgroup pass writes about 64 KB, in whole rounds of its PT pixel lanes
  const long long per_pix = (long long)C * factor * factor;
  long long chunk = (65536 / 4 + per_pix - 1) / per_pix;
  chunk = (chunk + PT - 1) / PT * PT;
  chunk = std::max<long long>(PT, std::min<long long>(chunk, UP_MAX_CHUNK));
  g.chunk = (int)chunk;
  const long long passes = (npix + chunk - 1) / chunk;
  const long long cap = (long long)device_cu_count() * 8;  // resident workgroups; the rest grid-stride
  const dim3 grid((unsigned)std::min(passes, cap));
  if (vec4)
    hipLaunchKernelGGL(upsample_kernel<4>, grid, dim3(SC_THREADS), 0, stream, in, out, g);
  else
    hipLaunchKernelGGL(upsample_kernel<1>, grid, dim3(SC_THREADS), 0, stream, in, out, g);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("launch upsample: %s", hipGetErrorString(e));
    return -1;
  }
  return 0;
}

}  // namespace dnnhip
