// Slice: a channel range of a tensor (Darknet's [route] with groups / group_id, the CSP split).
//
//   out[n, h, w, k] = in[n, h, w, first + k]      0 <= k < channels
//
// in is [n, H, W, C], out [n, H, W, channels], both plain NHWC fp32, first + channels <= C.  Pure
// data movement: every output pixel is one contiguous run of `channels` floats of its source pixel,
// so there is no (n, h, w) decomposition at all: pixel p's run starts at in + p * C + first.
//
// One kernel, in two widths: VEC = 4 moves 16 B per lane on both sides (C, first and channels
// multiples of 4, 16-byte aligned tensors), VEC = 1 covers everything else.  A workgroup owns a
// chunk of consecutive pixels; QT of its threads span a pixel's columns and the other 256 / QT
// step through the chunk's pixels.  A thread resolves its column's source and destination once;
// the copy loop is one add per side, one load and one store per element, with no division.
#include <hip/hip_runtime.h>
#include <algorithm>
#include "dnn_common.h"

namespace dnnhip {

typedef float slice_f32x4 __attribute__((ext_vector_type(4)));

template <int VEC>
struct SliceVec;
template <>
struct SliceVec<4> {
  typedef slice_f32x4 type;
};
template <>
struct SliceVec<1> {
  typedef float type;
};

struct SliceGeom {
  int npix;      // pixels: n * H * W
  int C;         // the input's channels, in floats
  int first;     // first channel taken, in floats
  int channels;  // channels taken, in floats
  int cols;      // output columns per pixel, in VEC units: channels / VEC
  int qt_log2;   // threads over columns: QT = 1 << qt_log2 (<= 64), 256 / QT pixel lanes
  int chunk;     // pixels per workgroup pass, a multiple of the pixel lanes
};

constexpr int SLICE_THREADS = 256;

template <int VEC>
__global__ void __launch_bounds__(SLICE_THREADS)
slice_kernel(const float* __restrict__ in, float* __restrict__ out, SliceGeom g) {
  typedef typename SliceVec<VEC>::type vec_t;
  const int tid = threadIdx.x;
  const int QT = 1 << g.qt_log2, PT = SLICE_THREADS >> g.qt_log2;
  const int tq = tid & (QT - 1), tp = tid >> g.qt_log2;
  // grid-stride over chunks of pixels (every tensor is below 2 GiB: float offsets fit an int)
  for (int p0 = blockIdx.x * g.chunk; p0 < g.npix; p0 += gridDim.x * g.chunk) {
    const int np = min(g.chunk, g.npix - p0);
    for (int q = tq; q < g.cols; q += QT) {
      // this thread's column of the pixel, on both sides
      const float* src = in + (size_t)p0 * g.C + g.first + q * VEC;
      float* dst = out + (size_t)p0 * g.channels + q * VEC;
#pragma unroll 4
      for (int p = tp; p < np; p += PT) {
        const vec_t v = *reinterpret_cast<const vec_t*>(src + (size_t)p * g.C);
        *reinterpret_cast<vec_t*>(dst + (size_t)p * g.channels) = v;
      }
    }
  }
}

static int slice_log2_ceil(int v) {
  int l = 0;
  while ((1 << l) < v) ++l;
  return l;
}

int launch_slice(const float* in, float* out, int n, int H, int W, int C, int first, int channels,
                 hipStream_t stream) {
  DNN_REQUIRE(in && out, "launch_slice: NULL tensor");
  DNN_REQUIRE(n >= 0 && H > 0 && W > 0 && C > 0, "launch_slice: bad shape n=%d %dx%dx%d", n, H, W, C);
  DNN_REQUIRE(first >= 0 && channels >= 1 && (long long)first + channels <= C,
              "launch_slice: channels %d..%d outside the input's %d", first, first + channels - 1, C);
  const long long npix = (long long)n * H * W;
  DNN_REQUIRE((unsigned long long)npix * C * 4 < 0x80000000ULL,
              "launch_slice: a tensor of n=%d %dx%dx%d is >= 2 GiB; split the batch", n, H, W, C);
  if (npix == 0) return 0;
  const bool vec4 = C % 4 == 0 && first % 4 == 0 && channels % 4 == 0 &&
                    ((reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(out)) & 15) == 0;
  const int vec = vec4 ? 4 : 1;
  SliceGeom g;
  g.npix = (int)npix;
  g.C = C;
  g.first = first;
  g.channels = channels;
  g.cols = channels / vec;
  g.qt_log2 = std::min(6, slice_log2_ceil(g.cols));
  const int PT = SLICE_THREADS >> g.qt_log2;
  // a workgroup pass moves about 64 KB (each way), in whole rounds of its PT pixel lanes: at
  // least four pixels per lane where the tensor allows, so four loads are in flight per lane
  long long chunk = (65536 / 4 + channels - 1) / channels;
  chunk = (chunk + PT - 1) / PT * PT;
  chunk = std::max<long long>(chunk, 4 * PT);
  g.chunk = (int)chunk;
  const long long passes = (npix + chunk - 1) / chunk;
  const long long cap = (long long)device_cu_count() * 8;  // resident workgroups; the rest grid-stride
  const dim3 grid((unsigned)std::min(passes, cap));
  if (vec4)
    hipLaunchKernelGGL(slice_kernel<4>, grid, dim3(SLICE_THREADS), 0, stream, in, out, g);
  else
    hipLaunchKernelGGL(slice_kernel<1>, grid, dim3(SLICE_THREADS), 0, stream, in, out, g);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("launch slice: %s", hipGetErrorString(e));
    return -1;
  }
  return 0;
}

}  // namespace dnnhip
