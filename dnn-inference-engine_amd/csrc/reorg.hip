// Reorg: Darknet's [reorg] layer (the non-reverse forward) fused with the channel concat that
// follows it in YOLOv2's passthrough.
//
//   out[n, yo, xo, :] = [ reorg(a)[n, yo, xo, :] , b[n, yo, xo, :] ]      (b first with b_first)
//
// a is [n, H, W, Ca], b is [n, H/s, W/s, Cb] (or absent, Cb == 0), all NHWC fp32, s in 1..8.
// Darknet defines the layer on the flat CHW buffers of one image (c = Ca, h = H, w = W,
// out_c = c / s^2): for every k < c, j < h, i < w
//
//   o  = i + w (j + h k)                           flat index into the OUTPUT, read as [c s^2][h/s][w/s]
//   c2 = k mod out_c ;  off = k div out_c
//   w2 = i s + off mod s ;  h2 = j s + off div s
//   f  = w2 + w s (h2 + h s c2)                    flat index into the INPUT, read as [c][h][w]
//   out_flat[o] = in_flat[f]
//
// which is a bijection on c h w elements and NOT space_to_depth (route.hip): the flat buffer is
// reinterpreted, so neighbouring output channels of a pixel come from different source pixels.
// In NHWC the element o = (co (h/s) + yo)(w/s) + xo lands at (yo (w/s) + xo)(c s^2) + co and is
// read from (yi w + xi) c + ci with f = (ci h + yi) w + xi.
//
// The permutation is the same for every image, so it is tabulated, not recomputed: a workgroup
// owns a chunk of consecutive output pixels of the map (and a slice of the batch).  Per chunk it
// builds, once, an LDS table with the source offset inside one image of every reorg element of
// the chunk (the divisions above: once per element per chunk), then each thread takes the
// offsets of its elements into registers and walks the images of its slice: per element and
// image one add, one 4-byte gathered load, and per VEC elements one contiguous store.  Stores
// are full runs of the output pixel rows, 16 B per lane where Ca s^2, Cb and the pointers allow
// (reorg_kernel<4>), 4 B otherwise (reorg_kernel<1>); the gathered loads are 4 B in both, since
// no two neighbouring output channels are neighbours in the source.  They are still coalesced:
// lane t of the 16-byte width holds output channels 4t .. 4t + 3, whose k is the same for all
// four when s = 2 and steps by one from lane to lane, so each of a wave's four load instructions
// reads runs of out_c consecutive floats.  The b part is the contiguous copy of the route kernel.
#include <hip/hip_runtime.h>
#include <algorithm>
#include "dnn_common.h"

namespace dnnhip {

typedef float reorg_f32x4 __attribute__((ext_vector_type(4)));

struct ReorgGeom {
  int n;           // images
  int H, W, Ca;    // a's shape
  int s;           // stride
  int OH, OW;      // H / s, W / s
  int Cb;          // channels of b
  int cout;        // Ca s^2 + Cb
  int a_first;     // first output channel of the reorg part; b's part starts at b_first
  int b_first;
  int tile;        // reorg channels per table pass (<= REORG_TABLE, a multiple of VEC unless it is all of them)
  int chunk;       // output pixels per workgroup item (chunk * tile <= REORG_TABLE)
  int nchunks;     // ceil(OH OW / chunk)
  int nslices;     // batch slices: an item is (chunk, slice)
  int per_slice;   // images per slice
  int qa_log2;     // threads over the columns of the reorg part: 1 << qa_log2 (<= 64), the rest over pixels
  int qb_log2;     // ... of the b part
};

constexpr int REORG_THREADS = 256;
constexpr int REORG_TABLE = 8192;  // ints of LDS: 32 KB, two workgroups per CU with room to spare

// The source offset inside one image of a (NHWC) of reorg output channel co at output pixel
// (yo, xo): the definition above, literally.
__device__ __forceinline__ int reorg_source(const ReorgGeom& g, int co, int yo, int xo) {
  const int o = (co * g.OH + yo) * g.OW + xo;
  const int i = o % g.W, oj = o / g.W;
  const int j = oj % g.H, k = oj / g.H;
  const int out_c = g.Ca / (g.s * g.s);
  const int c2 = k % out_c, off = k / out_c;
  const int w2 = i * g.s + off % g.s, h2 = j * g.s + off / g.s;
  const int f = w2 + g.W * g.s * (h2 + g.H * g.s * c2);
  const int xi = f % g.W, fy = f / g.W;
  const int yi = fy % g.H, ci = fy / g.H;
  return (yi * g.W + xi) * g.Ca + ci;
}

template <int VEC>
__global__ void __launch_bounds__(REORG_THREADS)
reorg_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ out, ReorgGeom g) {
  __shared__ int table[REORG_TABLE];  // [pixel of the chunk][channel of the tile]: a's offset inside an image
  const int tid = threadIdx.x;
  const int ohw = g.OH * g.OW, ca_out = g.Ca * g.s * g.s;
  const size_t a_img = (size_t)g.H * g.W * g.Ca;  // floats per image (every tensor is below 2 GiB)
  const int QA = 1 << g.qa_log2, PA = REORG_THREADS >> g.qa_log2;
  const int QB = 1 << g.qb_log2, PB = REORG_THREADS >> g.qb_log2;
  const int tqa = tid & (QA - 1), tpa = tid >> g.qa_log2;
  const int tqb = tid & (QB - 1), tpb = tid >> g.qb_log2;
  const int items = g.nchunks * g.nslices;
  for (int item = blockIdx.x; item < items; item += gridDim.x) {
    const int ck = item % g.nchunks, sl = item / g.nchunks;  // (per item, not per element)
    const int p0 = ck * g.chunk, np = min(g.chunk, ohw - p0);
    const int n0 = sl * g.per_slice, n1 = min(g.n, n0 + g.per_slice);
    // ---- the reorg part, a table pass per tile of its channels
    for (int c0 = 0; c0 < ca_out; c0 += g.tile) {
      const int tw = min(g.tile, ca_out - c0);  // (a multiple of VEC)
      __syncthreads();  // the previous pass has taken its offsets
      for (int e = tid; e < np * tw; e += REORG_THREADS) {
        const int p = e / tw, q = e - p * tw;
        const int pix = p0 + p;
        table[p * g.tile + q] = reorg_source(g, c0 + q, pix / g.OW, pix % g.OW);
      }
      __syncthreads();
      for (int q = tqa * VEC; q < tw; q += QA * VEC) {
        for (int p = tpa; p < np; p += PA) {
          int src[VEC];
#pragma unroll
          for (int v = 0; v < VEC; ++v) src[v] = table[p * g.tile + q + v];
          float* dst = out + ((size_t)n0 * ohw + p0 + p) * g.cout + g.a_first + c0 + q;
          const float* img = a + (size_t)n0 * a_img;
#pragma unroll 4
          for (int n = n0; n < n1; ++n) {
            if (VEC == 4) {
              reorg_f32x4 v;
              v.x = img[src[0]];
              v.y = img[src[1]];
              v.z = img[src[2]];
              v.w = img[src[3]];
              *reinterpret_cast<reorg_f32x4*>(dst) = v;
            } else {
              *dst = img[src[0]];
            }
            img += a_img;
            dst += (size_t)ohw * g.cout;
          }
        }
      }
    }
    // ---- the b part: contiguous runs on both sides
    for (int q = tqb * VEC; q < g.Cb; q += QB * VEC) {
      for (int p = tpb; p < np; p += PB) {
        const size_t pix = (size_t)n0 * ohw + p0 + p;
        const float* src = b + pix * g.Cb + q;
        float* dst = out + pix * g.cout + g.b_first + q;
#pragma unroll 4
        for (int n = n0; n < n1; ++n) {
          if (VEC == 4)
            *reinterpret_cast<reorg_f32x4*>(dst) = *reinterpret_cast<const reorg_f32x4*>(src);
          else
            *dst = *src;
          src += (size_t)ohw * g.Cb;
          dst += (size_t)ohw * g.cout;
        }
      }
    }
  }
}

static int reorg_log2_ceil(int v) {
  int l = 0;
  while ((1 << l) < v) ++l;
  return l;
}

int launch_reorg(const float* a, const float* b, float* out, int n, int H, int W, int Ca, int stride, int Cb,
                 int b_first, hipStream_t stream) {
  DNN_REQUIRE(a && out, "launch_reorg: NULL tensor");
  DNN_REQUIRE(n >= 0 && H > 0 && W > 0 && Ca > 0 && Cb >= 0, "launch_reorg: bad shape n=%d %dx%dx%d Cb=%d", n, H, W, Ca,
              Cb);
  DNN_REQUIRE(stride >= 1 && stride <= 8, "launch_reorg: stride %d outside 1..8", stride);
  DNN_REQUIRE(H % stride == 0 && W % stride == 0, "launch_reorg: %dx%d input is not a multiple of stride %d", H, W,
              stride);
  DNN_REQUIRE(Ca % (stride * stride) == 0, "launch_reorg: %d channels are not a multiple of stride^2 = %d", Ca,
              stride * stride);
  DNN_REQUIRE((b != nullptr) == (Cb > 0), "launch_reorg: b must be NULL exactly when Cb == 0");
  const int OH = H / stride, OW = W / stride;
  const long long ca_out = (long long)stride * stride * Ca;
  const long long cout = ca_out + Cb;
  const long long ohw = (long long)OH * OW, npix = (long long)n * ohw;
  const unsigned long long lim = 0x80000000ULL;
  DNN_REQUIRE((unsigned long long)n * H * W * Ca * 4 < lim && (unsigned long long)npix * Cb * 4 < lim &&
                  (unsigned long long)npix * cout * 4 < lim,
              "launch_reorg: a tensor of n=%d %dx%dx%d stride %d Cb=%d is >= 2 GiB; split the batch", n, H, W, Ca,
              stride, Cb);
  if (npix == 0) return 0;
  // the gathered loads are 4 B whatever the width: only the stores and the b copy need alignment
  const bool vec4 = ca_out % 4 == 0 && Cb % 4 == 0 &&
                    ((reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(out)) & 15) == 0;
  const int vec = vec4 ? 4 : 1;
  ReorgGeom g;
  g.n = n;
  g.H = H;
  g.W = W;
  g.Ca = Ca;
  g.s = stride;
  g.OH = OH;
  g.OW = OW;
  g.Cb = Cb;
  g.cout = (int)cout;
  g.a_first = b_first ? Cb : 0;
  g.b_first = b_first ? 0 : (int)ca_out;
  g.tile = (int)std::min<long long>(ca_out, REORG_TABLE);  // (REORG_TABLE is a multiple of 4)
  g.qa_log2 = std::min(6, reorg_log2_ceil((g.tile + vec - 1) / vec));
  g.qb_log2 = std::min(6, reorg_log2_ceil(std::max(1, Cb / vec)));
  // a chunk is one round of the reorg part's pixel lanes, as far as the table holds it: the map's
  // pixels spread over many workgroups even at batch 1, and a thread's work per chunk is its
  // offsets times the images of its slice
  const int PA = REORG_THREADS >> g.qa_log2;
  g.chunk = (int)std::max<long long>(1, std::min<long long>({(long long)PA, (long long)(REORG_TABLE / g.tile), ohw}));
  g.nchunks = (int)((ohw + g.chunk - 1) / g.chunk);
  // the batch is sliced only to fill the chip (about four workgroups per CU), and never below
  // eight images per slice: a table is built once per (chunk, slice)
  const long long target = (long long)device_cu_count() * 4;
  long long nslices = std::min<long long>(std::max<long long>(1, target / g.nchunks), (n + 7) / 8);
  g.per_slice = (int)((n + nslices - 1) / nslices);
  g.nslices = (n + g.per_slice - 1) / g.per_slice;
  const long long items = (long long)g.nchunks * g.nslices;
  const long long cap = (long long)device_cu_count() * 8;  // resident workgroups; the rest grid-stride
  const dim3 grid((unsigned)std::min(items, cap));
  if (vec4)
    hipLaunchKernelGGL(reorg_kernel<4>, grid, dim3(REORG_THREADS), 0, stream, a, b, out, g);
  else
    hipLaunchKernelGGL(reorg_kernel<1>, grid, dim3(REORG_THREADS), 0, stream, a, b, out, g);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("launch reorg: %s", hipGetErrorString(e));
    return -1;
  }
  return 0;
}

}  // namespace dnnhip
