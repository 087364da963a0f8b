// Spatial pyramid pooling in one kernel: YOLOv3-SPP's x -> [maxpool13(x), maxpool9(x), maxpool5(x), x].
// The reference has no such node.  a [n, H, W, C] -> out [n, H, W, (n_sizes + 1) * C], NHWC fp32, each
// tensor below 2 GiB: channel block j is the sizes[j] x sizes[j] / stride-1 / SAME max pool of a, and a
// itself is the last block (the first with x_first).
//
// Bits.  The existing pool (maxpool_nhwc_kernel, oracle ref_numpy.max_pool2d) scans the -FLT_MAX padded
// window in row-major order with m = m >= v ? m : v, so among equal maxima (+0 and -0) the first one in
// row-major order wins.  keep(a, b) = a >= b ? a : b with a the earlier element is associative on finite
// values, so the scan may be regrouped as long as the order of the elements stays: here a row pass
// (per row of the window the first maximum, left to right) and then a column pass over the row results,
// top to bottom.  The first row that holds the maximum wins, and its result is that row's first maximum:
// the element the reference keeps.  A 2-D cascade (pool9 = pool5 of pool5) does not keep that order and
// is not used.
//
// Shape.  A workgroup owns one image tile (at most 20 x 20: the 13 x 13 and 19 x 19 maps where SPP
// occurs are one tile) and a slab of S 16-byte channel columns (S floats when C % 4 != 0).  It reads
// the tile with a halo of the largest half window once into LDS, pixels outside the image as
// -FLT_MAX (so every later read is an unconditional LDS read), copies the interior to the x block,
// and then per distinct size runs the row pass LDS -> LDS and the column pass LDS -> global.  One size
// at a time keeps the footprint at the staged tile plus ONE row-pass buffer (30 KB for a 13 x 13 map
// at S = 2, 50 KB at 19 x 19) instead of three, which is what lets three to five workgroups share a
// CU; the price is 5 + 9 + 13 LDS reads per row-pass element instead of the 13 of a nested pass.  The
// window is a template parameter, so a lane's 2h + 1 LDS reads are all issued before the compares.
// Lanes run over the slab first, so a wave's LDS accesses are consecutive 16-byte slots (no bank
// conflicts) and its global accesses are S * 16 contiguous bytes per pixel.  S is 4 where that still
// gives two workgroups per CU and fits 40 KB of LDS (measured at 64 x 13 x 13 x 512: 53.5 us with
// 30 KB workgroups at S = 2, 69.8 us with 61 KB ones at S = 4), else 2.  No atomics, no inline assembly.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cfloat>
#include "dnn_common.h"

namespace dnnhip {

typedef float spp_f32x4 __attribute__((ext_vector_type(4)));

constexpr int SPP_THREADS = 256;
constexpr int SPP_MAX_TILE = 20;              // tile edge: one tile covers a 19 x 19 map
constexpr size_t SPP_LDS_BUDGET = 64 * 1024;  // the default dynamic LDS limit
constexpr size_t SPP_LDS_SOFT = 40 * 1024;    // four workgroups per CU where 32-byte slabs allow it

template <int VEC>
struct SppVec;
template <>
struct SppVec<4> {
  typedef spp_f32x4 type;
  static __device__ __forceinline__ type lowest() { return type{-FLT_MAX, -FLT_MAX, -FLT_MAX, -FLT_MAX}; }
  // the earlier element a stays unless the later one is greater: m >= v ? m : v per channel
  static __device__ __forceinline__ type keep(type a, type b) {
    type r;
    r.x = a.x >= b.x ? a.x : b.x;
    r.y = a.y >= b.y ? a.y : b.y;
    r.z = a.z >= b.z ? a.z : b.z;
    r.w = a.w >= b.w ? a.w : b.w;
    return r;
  }
};
template <>
struct SppVec<1> {
  typedef float type;
  static __device__ __forceinline__ type lowest() { return -FLT_MAX; }
  static __device__ __forceinline__ type keep(type a, type b) { return a >= b ? a : b; }
};

struct SppGeom {
  int H, W, C;
  int cols;          // channel columns per pixel in VEC units: C / VEC
  int s_log2;        // columns per workgroup: S = 1 << s_log2
  int slabs;         // ceil(cols / S)
  int TH, TW;        // tile (<= SPP_MAX_TILE each)
  int tiles_y, tiles_x;
  int hmax;          // largest half window: the halo
  int n_sizes;
  int half[SPP_MAX_SIZES];   // half window of block j
  int first[SPP_MAX_SIZES];  // the first block with block j's size (== j: block j runs the passes)
  int OC;            // (n_sizes + 1) * C
  int x_block;       // channel block of the copy of a: n_sizes, or 0 with x_first
};

template <int VEC>
struct SppLane {
  typename SppVec<VEC>::type* st;  // [SH][SW][S]: the tile with its halo
  typename SppVec<VEC>::type* rp;  // [<= SH][TW][S]: one size's row pass
  float* dst;                      // this lane's channel column of the image's output
  int tq, tp, PT, S, SW, y0, x0;
  bool col_ok;
};

// one distinct size (half window HW): the row pass LDS -> LDS, then the column pass LDS -> global
template <int VEC, int HW>
__device__ __forceinline__ void spp_one_size(const SppGeom& g, int j, const SppLane<VEC>& ln) {
  typedef typename SppVec<VEC>::type vec_t;
  constexpr int K = 2 * HW + 1;
  const int S = ln.S, tq = ln.tq;
  const int rows = g.TH + 2 * HW;  // row results the column pass needs: tile rows -HW .. TH + HW
  // row pass: rp[r][x] = the first maximum of staged row (hmax - HW + r), columns x - HW .. x + HW
  for (int p = ln.tp; p < rows * g.TW; p += ln.PT) {
    const int r = p / g.TW, x = p - r * g.TW;
    const vec_t* s = ln.st + ((g.hmax - HW + r) * ln.SW + (x + g.hmax - HW)) * S + tq;
    vec_t v[K];
#pragma unroll
    for (int d = 0; d < K; ++d) v[d] = s[d * S];
    vec_t m = v[0];
#pragma unroll
    for (int d = 1; d < K; ++d) m = SppVec<VEC>::keep(m, v[d]);
    ln.rp[p * S + tq] = m;
  }
  __syncthreads();
  // column pass: out[y][x] = the first maximum of rp rows y .. y + 2 HW, top to bottom
  const int row_step = g.TW * S;
  for (int p = ln.tp; p < g.TH * g.TW; p += ln.PT) {
    const int y = p / g.TW, x = p - y * g.TW;
    const vec_t* s = ln.rp + p * S + tq;
    vec_t v[K];
#pragma unroll
    for (int d = 0; d < K; ++d) v[d] = s[d * row_step];
    vec_t m = v[0];
#pragma unroll
    for (int d = 1; d < K; ++d) m = SppVec<VEC>::keep(m, v[d]);
    if (ln.col_ok && ln.y0 + y < g.H && ln.x0 + x < g.W) {
      float* o = ln.dst + ((size_t)(ln.y0 + y) * g.W + ln.x0 + x) * g.OC;
      for (int b = j; b < g.n_sizes; ++b)
        if (g.first[b] == j) *reinterpret_cast<vec_t*>(o + (size_t)(b + (g.x_block == 0 ? 1 : 0)) * g.C) = m;
    }
  }
  __syncthreads();  // the next size's row pass overwrites rp
}

// workgroup -> (image, tile, slab); stage, copy x, then per distinct size: row pass, column pass
template <int VEC>
__global__ void __launch_bounds__(SPP_THREADS)
spp_kernel(const float* __restrict__ a, float* __restrict__ out, SppGeom g) {
  typedef typename SppVec<VEC>::type vec_t;
  extern __shared__ __attribute__((aligned(16))) unsigned char spp_lds[];
  const int S = 1 << g.s_log2;
  const int SH = g.TH + 2 * g.hmax, SW = g.TW + 2 * g.hmax;
  vec_t* st = reinterpret_cast<vec_t*>(spp_lds);  // [SH][SW][S]: the tile with its halo
  vec_t* rp = st + (size_t)SH * SW * S;           // [<= SH][TW][S]: one size's row pass
  const int tid = threadIdx.x;
  const int tq = tid & (S - 1), tp = tid >> g.s_log2, PT = SPP_THREADS >> g.s_log2;
  unsigned wg = blockIdx.x;
  const int slab = wg % g.slabs;
  wg /= g.slabs;
  const int tx = wg % g.tiles_x;
  wg /= g.tiles_x;
  const int ty = wg % g.tiles_y;
  const int img = wg / g.tiles_y;
  const int y0 = ty * g.TH, x0 = tx * g.TW;
  const int col = slab * S + tq;  // this lane's channel column
  const bool col_ok = col < g.cols;
  const float* src = a + (size_t)img * g.H * g.W * g.C + (size_t)col * VEC;
  float* dst = out + (size_t)img * g.H * g.W * g.OC + (size_t)col * VEC;

  // stage: every pixel of the haloed tile, -FLT_MAX outside the image (the reference's padding)
#pragma unroll 4
  for (int p = tp; p < SH * SW; p += PT) {
    const int sy = p / SW, sx = p - sy * SW;
    const int iy = y0 - g.hmax + sy, ix = x0 - g.hmax + sx;
    vec_t v = SppVec<VEC>::lowest();
    if (col_ok && (unsigned)iy < (unsigned)g.H && (unsigned)ix < (unsigned)g.W)
      v = *reinterpret_cast<const vec_t*>(src + ((size_t)iy * g.W + ix) * g.C);
    st[p * S + tq] = v;
  }
  __syncthreads();

  // the copy of a
  for (int p = tp; p < g.TH * g.TW; p += PT) {
    const int y = p / g.TW, x = p - y * g.TW;
    if (col_ok && y0 + y < g.H && x0 + x < g.W)
      *reinterpret_cast<vec_t*>(dst + ((size_t)(y0 + y) * g.W + x0 + x) * g.OC + (size_t)g.x_block * g.C) =
          st[((y + g.hmax) * SW + x + g.hmax) * S + tq];
  }

  for (int j = 0; j < g.n_sizes; ++j) {
    if (g.first[j] != j) continue;  // a repeated size: written with its first block
    const SppLane<VEC> ln{st, rp, dst, tq, tp, PT, S, SW, y0, x0, col_ok};
    switch (g.half[j]) {  // a static window: its LDS reads are all in flight before the compares
      case 1: spp_one_size<VEC, 1>(g, j, ln); break;
      case 2: spp_one_size<VEC, 2>(g, j, ln); break;
      case 3: spp_one_size<VEC, 3>(g, j, ln); break;
      case 4: spp_one_size<VEC, 4>(g, j, ln); break;
      case 5: spp_one_size<VEC, 5>(g, j, ln); break;
      default: spp_one_size<VEC, 6>(g, j, ln); break;
    }
  }
}

static size_t spp_lds_bytes(int TH, int TW, int hmax, int S, int vec) {
  const size_t SH = TH + 2 * hmax, SW = TW + 2 * hmax;
  return (SH * SW + SH * TW) * S * vec * sizeof(float);
}

int launch_spp(const float* a, float* out, int n, int H, int W, int C, int n_sizes, const int* sizes, int x_first,
               hipStream_t stream) {
  DNN_REQUIRE(a && out, "launch_spp: NULL tensor");
  DNN_REQUIRE(n >= 0 && H > 0 && W > 0 && C > 0, "launch_spp: bad shape n=%d %dx%dx%d", n, H, W, C);
  DNN_REQUIRE(sizes != nullptr, "launch_spp: sizes is NULL");
  DNN_REQUIRE(n_sizes >= 1 && n_sizes <= SPP_MAX_SIZES, "launch_spp: n_sizes %d outside 1..%d", n_sizes,
              SPP_MAX_SIZES);
  for (int j = 0; j < n_sizes; ++j)
    DNN_REQUIRE(sizes[j] >= 3 && sizes[j] <= SPP_MAX_K && sizes[j] % 2 == 1,
                "launch_spp: size %d is not odd and in 3..%d", sizes[j], SPP_MAX_K);
  const long long npix = (long long)n * H * W;
  DNN_REQUIRE((unsigned long long)npix * C * (n_sizes + 1) * 4 < 0x80000000ULL,
              "launch_spp: the output of n=%d %dx%dx%d with %d sizes is >= 2 GiB; split the batch", n, H, W, C,
              n_sizes);
  DNN_REQUIRE(out != a, "launch_spp: out may not alias the input");
  if (npix == 0) return 0;
  const bool vec4 = C % 4 == 0 && ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(out)) & 15) == 0;
  const int vec = vec4 ? 4 : 1;
  SppGeom g;
  g.H = H;
  g.W = W;
  g.C = C;
  g.cols = C / vec;
  g.tiles_y = (H + SPP_MAX_TILE - 1) / SPP_MAX_TILE;
  g.tiles_x = (W + SPP_MAX_TILE - 1) / SPP_MAX_TILE;
  g.TH = (H + g.tiles_y - 1) / g.tiles_y;  // equal tiles, the last one ragged
  g.TW = (W + g.tiles_x - 1) / g.tiles_x;
  g.n_sizes = n_sizes;
  g.hmax = 0;
  for (int j = 0; j < SPP_MAX_SIZES; ++j) {
    g.half[j] = j < n_sizes ? sizes[j] / 2 : 0;
    g.first[j] = j;
    for (int i = j - 1; i >= 0; --i)
      if (j < n_sizes && sizes[i] == sizes[j]) g.first[j] = i;
    g.hmax = std::max(g.hmax, g.half[j]);
  }
  g.OC = (n_sizes + 1) * C;
  g.x_block = x_first ? 0 : n_sizes;
  // 64 contiguous bytes per pixel (four 16-byte columns, or sixteen floats) where the LDS budget
  // allows and that still leaves two workgroups per CU; else half, and so on
  const long long units = (long long)n * g.tiles_y * g.tiles_x;
  int sl = vec4 ? 2 : 4;
  while (sl > 0 && (1 << (sl - 1)) >= g.cols) --sl;  // no wider than the tensor
  auto wgs = [&](int l) { return units * ((g.cols + (1 << l) - 1) >> l); };
  while (sl > (vec4 ? 1 : 3) && wgs(sl) < 2LL * device_cu_count()) --sl;
  while (sl > (vec4 ? 1 : 3) && spp_lds_bytes(g.TH, g.TW, g.hmax, 1 << sl, vec) > SPP_LDS_SOFT) --sl;
  while (sl > 0 && spp_lds_bytes(g.TH, g.TW, g.hmax, 1 << sl, vec) > SPP_LDS_BUDGET) --sl;
  g.s_log2 = sl;
  g.slabs = (g.cols + (1 << sl) - 1) >> sl;
  const size_t lds = spp_lds_bytes(g.TH, g.TW, g.hmax, 1 << sl, vec);
  DNN_REQUIRE(lds <= SPP_LDS_BUDGET, "launch_spp: a %dx%d tile with halo %d needs %zu bytes of LDS", g.TH, g.TW,
              g.hmax, lds);
  const long long grid = units * g.slabs;  // (< 2^29: one workgroup writes at least one float)
  DNN_REQUIRE(grid <= 0x7fffffffLL, "launch_spp: %lld workgroups", grid);
  if (vec4)
    hipLaunchKernelGGL(spp_kernel<4>, dim3((unsigned)grid), dim3(SPP_THREADS), lds, stream, a, out, g);
  else
    hipLaunchKernelGGL(spp_kernel<1>, dim3((unsigned)grid), dim3(SPP_THREADS), lds, stream, a, out, g);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("launch spp: %s", hipGetErrorString(e));
    return -1;
  }
  return 0;
}

}  // namespace dnnhip
