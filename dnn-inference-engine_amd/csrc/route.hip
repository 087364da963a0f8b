// Route: space-to-depth, channel concat and the two fused (YOLOv2's passthrough join).
//
//   out[n, h, w, :] = [ s2d(a)[n, h, w, :] , b[n, h, w, :] ]      (b first with b_first)
//   s2d(a)[n, h, w, (dy*block + dx)*Ca + c] = a[n, h*block + dy, w*block + dx, c]
//
// a is [n, H, W, Ca], b is [n, H/block, W/block, Cb] (or absent, Cb == 0), all NHWC fp32.  The
// s2d channel order is TensorFlow's space_to_depth, not Darknet's reorg.  Pure data movement:
// every run of Ca (or Cb) consecutive output floats is one contiguous run of its source.
//
// One kernel, in two widths: VEC = 4 moves 16 B per lane on both sides (Ca % 4 == 0, Cb % 4 == 0,
// 16-byte aligned tensors), VEC = 1 covers every other channel count.  A workgroup owns a chunk
// of consecutive output pixels.  It tabulates each pixel's source bases in LDS (the (n, h, w)
// decomposition: once per pixel), and each thread resolves the source offset of its column of
// the output pixel (which (dy, dx) run, which channel) once per column; the copy loop itself is
// two LDS reads, one add, one load and one store per element, with no division.
#include <hip/hip_runtime.h>
#include <algorithm>
#include "dnn_common.h"

namespace dnnhip {

typedef float route_f32x4 __attribute__((ext_vector_type(4)));

template <int VEC>
struct RouteVec;
template <>
struct RouteVec<4> {
  typedef route_f32x4 type;
};
template <>
struct RouteVec<1> {
  typedef float type;
};

struct RouteGeom {
  int npix;       // output pixels: n * OH * OW
  int OH, OW;     // output spatial (H / block, W / block)
  int W;          // a's width
  int Ca, Cb;     // channels of a and b, in floats
  int block;
  int a_first_col;  // first output column (in VEC units) of the a part; the b part starts at b_first_col
  int b_first_col;
  int cols;       // output columns per pixel, in VEC units: (block*block*Ca + Cb) / VEC
  int qt_log2;    // threads over columns: QT = 1 << qt_log2 (<= 64), 256 / QT pixel lanes
  int chunk;      // output pixels per workgroup pass (<= ROUTE_MAX_CHUNK)
};

constexpr int ROUTE_THREADS = 256;
constexpr int ROUTE_MAX_CHUNK = 256;

template <int VEC>
__global__ void __launch_bounds__(ROUTE_THREADS)
route_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ out, RouteGeom g) {
  typedef typename RouteVec<VEC>::type vec_t;
  __shared__ int a_base[ROUTE_MAX_CHUNK];  // float offset of a[n, h*block, w*block, 0]
  __shared__ int b_base[ROUTE_MAX_CHUNK];  // float offset of b[n, h, w, 0]
  const int tid = threadIdx.x;
  const int QT = 1 << g.qt_log2, PT = ROUTE_THREADS >> g.qt_log2;
  const int tq = tid & (QT - 1), tp = tid >> g.qt_log2;
  const int cols_a = g.block * g.block * g.Ca / VEC, ca_cols = g.Ca / VEC;
  const int cout = g.cols * VEC;
  // grid-stride over chunks of pixels (every tensor is below 2 GiB: float offsets fit an int)
  for (int p0 = blockIdx.x * g.chunk; p0 < g.npix; p0 += gridDim.x * g.chunk) {
    const int np = min(g.chunk, g.npix - p0);
    __syncthreads();  // the previous pass has finished reading the tables
    for (int p = tid; p < np; p += ROUTE_THREADS) {
      const int pix = p0 + p;
      const int w = pix % g.OW, nh = pix / g.OW;
      const int h = nh % g.OH, n = nh / g.OH;
      a_base[p] = ((n * g.OH * g.block + h * g.block) * g.W + w * g.block) * g.Ca;
      b_base[p] = pix * g.Cb;
    }
    __syncthreads();
    for (int q = tq; q < g.cols; q += QT) {
      // this thread's column of the output pixel: its source tensor and offset inside the pixel
      const int qa = q - g.a_first_col;
      const bool from_a = qa >= 0 && qa < cols_a;
      int rel;
      if (from_a) {
        const int seg = qa / ca_cols, c = qa - seg * ca_cols;  // seg = dy * block + dx
        const int dy = seg / g.block, dx = seg - dy * g.block;
        rel = (dy * g.W + dx) * g.Ca + c * VEC;
      } else {
        rel = (q - g.b_first_col) * VEC;
      }
      const float* src = from_a ? a : b;
      const int* base = from_a ? a_base : b_base;
      float* dst = out + (size_t)p0 * cout + q * VEC;
#pragma unroll 4
      for (int p = tp; p < np; p += PT) {
        const vec_t v = *reinterpret_cast<const vec_t*>(src + base[p] + rel);
        *reinterpret_cast<vec_t*>(dst + (size_t)p * cout) = v;
      }
    }
  }
}

static int route_log2_ceil(int v) {
  int l = 0;
  while ((1 << l) < v) ++l;
  return l;
}

int launch_route(const float* a, const float* b, float* out, int n, int H, int W, int Ca, int block, int Cb,
                 int b_first, hipStream_t stream) {
  DNN_REQUIRE(a && out, "launch_route: NULL tensor");
  DNN_REQUIRE(n >= 0 && H > 0 && W > 0 && Ca > 0 && Cb >= 0, "launch_route: bad shape n=%d %dx%dx%d Cb=%d", n, H, W, Ca,
              Cb);
  DNN_REQUIRE(block >= 1 && block <= 8, "launch_route: block %d outside 1..8", block);
  DNN_REQUIRE(H % block == 0 && W % block == 0, "launch_route: %dx%d input is not a multiple of block %d", H, W, block);
  DNN_REQUIRE((b != nullptr) == (Cb > 0), "launch_route: b must be NULL exactly when Cb == 0");
  const int OH = H / block, OW = W / block;
  const long long cout = (long long)block * block * Ca + Cb;
  const long long npix = (long long)n * OH * OW;
  const unsigned long long lim = 0x80000000ULL;
  DNN_REQUIRE((unsigned long long)n * H * W * Ca * 4 < lim && (unsigned long long)npix * Cb * 4 < lim &&
                  (unsigned long long)npix * cout * 4 < lim,
              "launch_route: a tensor of n=%d %dx%dx%d block %d Cb=%d is >= 2 GiB; split the batch", n, H, W, Ca, block,
              Cb);
  if (npix == 0) return 0;
  const bool vec4 = Ca % 4 == 0 && Cb % 4 == 0 &&
                    ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(out)) & 15) == 0;
  const int vec = vec4 ? 4 : 1;
  RouteGeom g;
  g.npix = (int)npix;
  g.OH = OH;
  g.OW = OW;
  g.W = W;
  g.Ca = Ca;
  g.Cb = Cb;
  g.block = block;
  g.cols = (int)(cout / vec);
  g.a_first_col = b_first ? Cb / vec : 0;
  g.b_first_col = b_first ? 0 : block * block * Ca / vec;
  g.qt_log2 = std::min(6, route_log2_ceil(g.cols));
  const int PT = ROUTE_THREADS >> g.qt_log2;
  // a workgroup pass moves about 64 KB (each way), in whole rounds of its PT pixel lanes: at
  // least four pixels per lane where the tensor allows, so four loads are in flight per lane
  long long chunk = (65536 / 4 + cout - 1) / cout;
  chunk = (chunk + PT - 1) / PT * PT;
  chunk = std::max<long long>(PT, std::min<long long>(chunk, ROUTE_MAX_CHUNK));
  g.chunk = (int)chunk;
  const long long passes = (npix + chunk - 1) / chunk;
  const long long cap = (long long)device_cu_count() * 8;  // resident workgroups; the rest grid-stride
  const dim3 grid((unsigned)std::min(passes, cap));
  if (vec4)
    hipLaunchKernelGGL(route_kernel<4>, grid, dim3(ROUTE_THREADS), 0, stream, a, b, out, g);
  else
    hipLaunchKernelGGL(route_kernel<1>, grid, dim3(ROUTE_THREADS), 0, stream, a, b, out, g);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("launch route: %s", hipGetErrorString(e));
    return -1;
  }
  return 0;
}

}  // namespace dnnhip
