// Grouped and depthwise convs (Darknet's [convolutional] groups=, ResNeXt's 32-group 3x3 convs, the
// depthwise half of a separable conv).  With g = groups, cg = C / g, og = OC / g:
//
//   out[n, oy, ox, j] = act(alpha[j] * sum_{ky,kx,k} in[n, oy*sh - ph + ky, ox*sw - pw + kx, (j / og)*cg + k]
//                                                     * w[ky][kx][k][j]  - beta[j])
//
// in and out are plain NHWC fp32, w is [kh][kw][cg][OC]; samples outside the frame are zeros; the
// epilogue is dnn_plan_add_conv_padded's (v * alpha - beta, never contracted, then apply_act).
// All arithmetic is fp32.  launch_conv_grouped picks one of two kernels from the shape alone, so a
// frame's rows are the same bits whatever the batch and the plan's mode.
//
// (a) cg % 4 == 0 and og % 4 == 0: the MFMA kernel, on v_mfma_f32_4x4x1_16b_f32.  One issue does
//     sixteen independent 4x4x1 products: the fp32 rate of the 16x16x4 tile, with no block-diagonal
//     zeros, whatever the group width.  A wave owns 64 output channels: block b of the instruction
//     is channels [4b, 4b + 4) of the tile, which lie in one group since og % 4 == 0, times four
//     consecutive output pixels (indices into the flattened n * OH * OW: a quad may cross a row or an
//     image).  Lane 4b + r supplies A = in[pixel r][group(b) * cg + k], lane 4b + j supplies
//     B = w[tap][k][4b + j]; D VGPR i of lane 4b + j is pixel i, channel 4b + j.  So lane l owns
//     output channel tile + l: its B values are that channel's weights, its stores for a pixel are
//     64 consecutive floats per wave.  Four consecutive k of a lane are one 16-byte load on both
//     sides: NHWC input as it lies, weights packed on the host as [tile][tap * cg / 4][lane][4]
//     (conv_grouped_pack, zero for channels past OC).
//       Resident form (3x3 and 1x1 with cg 4, 8, 16, 32): the B values of a K chunk, a run of whole
//     taps of at most 160 floats, sit in registers.  One chunk (all but 3x3 cg 32): the wave loads
//     them once and streams groups of P = 4 pixel quads; two chunks: the P accumulators persist
//     across the chunks.  Streamed form (any other kernel size or cg): the same loop with B read
//     through L1 per k quad, amortised over the P quads.
//       The taps' overlapping input rows come straight from L1 / L2, no LDS patch: a quad's four
//     pixels and the next quads' share their 16-byte runs, and DESIGN.md 8 has the measured distance
//     to the copy floor that this decision rests on.
// (b) everything else: the direct kernels, VALU.  Depthwise (cg == og == 1) with C % 4 == 0, a 3x3
//     or 5x5 kernel and stride 1 or 2: a lane owns four channels as a float4, keeps the kh * kw
//     weight vectors and the kh x kw input window in registers and walks down a strip of output rows
//     for one ox, loading only the incoming rows; neighbouring ox are neighbouring lanes of the same
//     workgroup, so their re-reads hit L1.  Any other shape (C % 4 != 0, cg = 2, 3, ..., og != cg
//     multipliers off the MFMA path): one thread per (pixel, output channel).  That one has to be
//     right, not fast.
#include <hip/hip_runtime.h>
#include <algorithm>
#include "dnn_common.h"

namespace dnnhip {

typedef float gc_f32x4 __attribute__((ext_vector_type(4)));

struct GroupedGeom {
  int M;  // output pixels: n * OH * OW
  int H, W, C, OH, OW, OC;
  int kh, kw, sh, sw, ph, pw;
  int cg, og;
  int flags;  // EPI_BN_AB | EPI_LEAKY_* or an EPI_ACT_MASK code
};

constexpr int GC_THREADS = 256;  // 4 waves
constexpr int GC_P = 4;          // pixel quads a wave has in flight
constexpr int GC_BUDGET = 160;   // resident B floats per lane (a K chunk)

__device__ __forceinline__ float gc_epilogue(float v, float a, float b, int flags) {
  if (flags & EPI_BN_AB) v = v * a - b;
  return apply_act(v, epi_act(flags));
}

// One lane's view of its A pixel in each of the P quads of a group: the input offset of tap (0, 0)
// (which may lie outside the frame) and that tap's row / column; iy = INT_MIN / 2 for a dead pixel
struct GcPixels {
  int off[GC_P], iy[GC_P], ix[GC_P];
};

__device__ __forceinline__ void gc_pixels(const GroupedGeom& g, int quad0, int r, GcPixels* px) {
#pragma unroll
  for (int p = 0; p < GC_P; ++p) {
    const int m = (quad0 + p) * 4 + r;
    const int ox = m % g.OW, t = m / g.OW, oy = t % g.OH, n = t / g.OH;
    const int iy = oy * g.sh - g.ph;
    px->ix[p] = ox * g.sw - g.pw;
    px->off[p] = ((n * g.H + iy) * g.W + px->ix[p]) * g.C;  // (only used when the tap is in the frame)
    px->iy[p] = m < g.M ? iy : -(1 << 30);
  }
}

__device__ __forceinline__ gc_f32x4 gc_mfma4(gc_f32x4 acc, gc_f32x4 a, gc_f32x4 b) {
  acc = __builtin_amdgcn_mfma_f32_4x4x1f32(a.x, b.x, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_4x4x1f32(a.y, b.y, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_4x4x1f32(a.z, b.z, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_4x4x1f32(a.w, b.w, acc, 0, 0, 0);
  return acc;
}

// D VGPR i of lane l: pixel 4 * quad + i, channel oc.  Only live pixels and channels are stored
__device__ __forceinline__ void gc_store(const GroupedGeom& g, float* __restrict__ out, int quad0, int oc, float al,
                                         float be, const gc_f32x4* acc) {
  if (oc >= g.OC) return;
#pragma unroll
  for (int p = 0; p < GC_P; ++p)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int m = (quad0 + p) * 4 + i;
      if (m < g.M) out[(size_t)m * g.OC + oc] = gc_epilogue(acc[p][i], al, be, g.flags);
    }
}

// CG4 = cg / 4 and TAPS = kh * kw at compile time; the K chunk is TC whole taps.  grid.y: channel tiles
template <int CG4, int TAPS, int TC>
__global__ void __launch_bounds__(GC_THREADS)
gconv_mfma_resident(const float* __restrict__ in, const float* __restrict__ wpk, const float* __restrict__ alpha,
                    const float* __restrict__ beta, float* __restrict__ out, GroupedGeom g, int ngroups) {
  constexpr int NCHUNK = (TAPS + TC - 1) / TC;
  const int lane = threadIdx.x & 63, r = lane & 3;
  const int tile = blockIdx.y, oc = tile * 64 + lane;
  const int blk_c = tile * 64 + (lane & ~3);  // the block's first channel
  const bool live = blk_c < g.OC;             // a dead block's lanes load no A and store nothing
  const int cbase = live ? (blk_c / g.og) * g.cg : 0;
  const gc_f32x4* wq = reinterpret_cast<const gc_f32x4*>(wpk) + (size_t)tile * (TAPS * CG4) * 64 + lane;
  const bool affine = (g.flags & EPI_BN_AB) && oc < g.OC;
  const float al = affine ? alpha[oc] : 1.f, be = affine ? beta[oc] : 0.f;
  gc_f32x4 B[TC * CG4];
  auto load_b = [&](int chunk) {
#pragma unroll
    for (int q = 0; q < TC * CG4; ++q)
      if (chunk * TC * CG4 + q < TAPS * CG4) B[q] = wq[(size_t)(chunk * TC * CG4 + q) * 64];
  };
  if (NCHUNK == 1) load_b(0);
  const int wave = blockIdx.x * (GC_THREADS / 64) + (threadIdx.x >> 6), nwaves = gridDim.x * (GC_THREADS / 64);
  for (int grp = wave; grp < ngroups; grp += nwaves) {
    GcPixels px;
    gc_pixels(g, grp * GC_P, r, &px);
    gc_f32x4 acc[GC_P];
#pragma unroll
    for (int p = 0; p < GC_P; ++p) acc[p] = gc_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int chunk = 0; chunk < NCHUNK; ++chunk) {
      if (NCHUNK > 1) load_b(chunk);
#pragma unroll
      for (int tt = 0; tt < TC; ++tt) {
        const int t = chunk * TC + tt;
        if (t >= TAPS) break;
        const int ky = t / g.kw, kx = t - ky * g.kw;
        const int toff = (ky * g.W + kx) * g.C + cbase;
        bool ok[GC_P];
#pragma unroll
        for (int p = 0; p < GC_P; ++p)
          ok[p] = live && (unsigned)(px.iy[p] + ky) < (unsigned)g.H && (unsigned)(px.ix[p] + kx) < (unsigned)g.W;
#pragma unroll
        for (int kq = 0; kq < CG4; ++kq) {
          gc_f32x4 a[GC_P];
#pragma unroll
          for (int p = 0; p < GC_P; ++p)
            a[p] = ok[p] ? *reinterpret_cast<const gc_f32x4*>(in + px.off[p] + toff + kq * 4)
                         : gc_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int p = 0; p < GC_P; ++p) acc[p] = gc_mfma4(acc[p], a[p], B[tt * CG4 + kq]);
        }
      }
    }
    gc_store(g, out, grp * GC_P, oc, al, be, acc);
  }
}

// Any kernel size and any cg % 4 == 0: B through L1, one 16-byte load per k quad for the P quads
__global__ void __launch_bounds__(GC_THREADS)
gconv_mfma_streamed(const float* __restrict__ in, const float* __restrict__ wpk, const float* __restrict__ alpha,
                    const float* __restrict__ beta, float* __restrict__ out, GroupedGeom g, int ngroups) {
  const int lane = threadIdx.x & 63, r = lane & 3;
  const int tile = blockIdx.y, oc = tile * 64 + lane;
  const int blk_c = tile * 64 + (lane & ~3);
  const bool live = blk_c < g.OC;
  const int cbase = live ? (blk_c / g.og) * g.cg : 0;
  const int cg4 = g.cg >> 2, taps = g.kh * g.kw;
  const gc_f32x4* wq = reinterpret_cast<const gc_f32x4*>(wpk) + (size_t)tile * (taps * cg4) * 64 + lane;
  const bool affine = (g.flags & EPI_BN_AB) && oc < g.OC;
  const float al = affine ? alpha[oc] : 1.f, be = affine ? beta[oc] : 0.f;
  const int wave = blockIdx.x * (GC_THREADS / 64) + (threadIdx.x >> 6), nwaves = gridDim.x * (GC_THREADS / 64);
  for (int grp = wave; grp < ngroups; grp += nwaves) {
    GcPixels px;
    gc_pixels(g, grp * GC_P, r, &px);
    gc_f32x4 acc[GC_P];
#pragma unroll
    for (int p = 0; p < GC_P; ++p) acc[p] = gc_f32x4{0.f, 0.f, 0.f, 0.f};
    int ky = 0, kx = 0;
    for (int t = 0; t < taps; ++t) {
      const int toff = (ky * g.W + kx) * g.C + cbase;
      bool ok[GC_P];
#pragma unroll
      for (int p = 0; p < GC_P; ++p)
        ok[p] = live && (unsigned)(px.iy[p] + ky) < (unsigned)g.H && (unsigned)(px.ix[p] + kx) < (unsigned)g.W;
      for (int kq = 0; kq < cg4; ++kq) {
        const gc_f32x4 b = wq[(size_t)(t * cg4 + kq) * 64];
#pragma unroll
        for (int p = 0; p < GC_P; ++p) {
          const gc_f32x4 a = ok[p] ? *reinterpret_cast<const gc_f32x4*>(in + px.off[p] + toff + kq * 4)
                                   : gc_f32x4{0.f, 0.f, 0.f, 0.f};
          acc[p] = gc_mfma4(acc[p], a, b);
        }
      }
      if (++kx == g.kw) {
        kx = 0;
        ++ky;
      }
    }
    gc_store(g, out, grp * GC_P, oc, al, be, acc);
  }
}

// ---------------------------------------------------------------- (b) direct kernels
constexpr int DW_STRIP = 8;  // output rows a lane walks down

// Depthwise, C % 4 == 0, K x K kernel, stride S both ways.  Flat thread index over (image, strip,
// ox, channel quad), channel quads fastest: a wave reads whole runs of a pixel's channels and its
// neighbours in ox sit in the same workgroup
template <int K, int S>
__global__ void __launch_bounds__(GC_THREADS)
gconv_depthwise(const float* __restrict__ in, const float* __restrict__ w, const float* __restrict__ alpha,
                const float* __restrict__ beta, float* __restrict__ out, GroupedGeom g, int nstrips, long long total) {
  const long long idx = (long long)blockIdx.x * GC_THREADS + threadIdx.x;
  if (idx >= total) return;
  const int C4 = g.C >> 2;
  const int c = (int)(idx % C4) * 4;
  long long t = idx / C4;
  const int ox = (int)(t % g.OW);
  t /= g.OW;
  const int strip = (int)(t % nstrips), n = (int)(t / nstrips);
  gc_f32x4 wv[K][K], win[K][K];
#pragma unroll
  for (int ky = 0; ky < K; ++ky)
#pragma unroll
    for (int kx = 0; kx < K; ++kx) wv[ky][kx] = *reinterpret_cast<const gc_f32x4*>(w + (size_t)(ky * K + kx) * g.C + c);
  const bool affine = g.flags & EPI_BN_AB;
  const gc_f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  const gc_f32x4 al = affine ? *reinterpret_cast<const gc_f32x4*>(alpha + c) : zero;
  const gc_f32x4 be = affine ? *reinterpret_cast<const gc_f32x4*>(beta + c) : zero;
  const int ix0 = ox * S - g.pw;
  const float* img = in + (size_t)n * g.H * g.W * g.C + c;
  auto load_row = [&](int ky, int iy) {  // the window's row ky from input row iy (zeros outside the frame)
#pragma unroll
    for (int kx = 0; kx < K; ++kx) {
      const int ix = ix0 + kx;
      win[ky][kx] = ((unsigned)iy < (unsigned)g.H && (unsigned)ix < (unsigned)g.W)
                        ? *reinterpret_cast<const gc_f32x4*>(img + ((size_t)iy * g.W + ix) * g.C)
                        : zero;
    }
  };
  const int oy0 = strip * DW_STRIP, oy1 = min(oy0 + DW_STRIP, g.OH);
  constexpr int KEEP = K > S ? K - S : 0;  // window rows a step keeps
  for (int oy = oy0; oy < oy1; ++oy) {
    const int iy0 = oy * S - g.ph;
    if (oy == oy0) {
#pragma unroll
      for (int ky = 0; ky < KEEP; ++ky) load_row(ky, iy0 + ky);
    } else {
#pragma unroll
      for (int ky = 0; ky < KEEP; ++ky)
#pragma unroll
        for (int kx = 0; kx < K; ++kx) win[ky][kx] = win[ky + S][kx];
    }
#pragma unroll
    for (int ky = KEEP; ky < K; ++ky) load_row(ky, iy0 + ky);
    gc_f32x4 acc = zero;
#pragma unroll
    for (int ky = 0; ky < K; ++ky)
#pragma unroll
      for (int kx = 0; kx < K; ++kx)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] = __builtin_fmaf(win[ky][kx][e], wv[ky][kx][e], acc[e]);
    gc_f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = gc_epilogue(acc[e], al[e], be[e], g.flags);
    *reinterpret_cast<gc_f32x4*>(out + (((size_t)n * g.OH + oy) * g.OW + ox) * g.OC + c) = o;
  }
}

// Any shape: one thread per (pixel, output channel), w as [kh][kw][cg][OC].  Right, not fast
__global__ void __launch_bounds__(GC_THREADS)
gconv_scalar(const float* __restrict__ in, const float* __restrict__ w, const float* __restrict__ alpha,
             const float* __restrict__ beta, float* __restrict__ out, GroupedGeom g) {
  const long long idx = (long long)blockIdx.x * GC_THREADS + threadIdx.x;
  if (idx >= (long long)g.M * g.OC) return;
  const int j = (int)(idx % g.OC), m = (int)(idx / g.OC);
  const int ox = m % g.OW, t = m / g.OW, oy = t % g.OH, n = t / g.OH;
  const int cbase = (j / g.og) * g.cg;
  float acc = 0.f;
  for (int ky = 0; ky < g.kh; ++ky) {
    const int iy = oy * g.sh - g.ph + ky;
    if ((unsigned)iy >= (unsigned)g.H) continue;
    for (int kx = 0; kx < g.kw; ++kx) {
      const int ix = ox * g.sw - g.pw + kx;
      if ((unsigned)ix >= (unsigned)g.W) continue;
      const float* src = in + (((size_t)n * g.H + iy) * g.W + ix) * g.C + cbase;
      const float* wk = w + (size_t)(ky * g.kw + kx) * g.cg * g.OC + j;
      for (int k = 0; k < g.cg; ++k) acc = __builtin_fmaf(src[k], wk[(size_t)k * g.OC], acc);
    }
  }
  const bool affine = g.flags & EPI_BN_AB;
  out[idx] = gc_epilogue(acc, affine ? alpha[j] : 1.f, affine ? beta[j] : 0.f, g.flags);
}

// ---------------------------------------------------------------- host side
bool conv_grouped_mfma(int C, int OC, int groups) { return (C / groups) % 4 == 0 && (OC / groups) % 4 == 0; }

size_t conv_grouped_weight_floats(int C, int OC, int groups, int kh, int kw) {
  const size_t k = (size_t)kh * kw * (C / groups);
  return conv_grouped_mfma(C, OC, groups) ? k * ((OC + 63) / 64 * 64) : k * OC;
}

void conv_grouped_pack(const float* w, float* packed, int C, int OC, int groups, int kh, int kw) {
  const int cg = C / groups, taps = kh * kw;
  if (!conv_grouped_mfma(C, OC, groups)) {
    std::copy(w, w + (size_t)taps * cg * OC, packed);
    return;
  }
  const int cg4 = cg / 4, ntiles = (OC + 63) / 64;
  for (int tile = 0; tile < ntiles; ++tile)
    for (int q = 0; q < taps * cg4; ++q)
      for (int lane = 0; lane < 64; ++lane)
        for (int e = 0; e < 4; ++e) {
          const int oc = tile * 64 + lane, t = q / cg4, k = (q % cg4) * 4 + e;
          packed[(((size_t)tile * taps * cg4 + q) * 64 + lane) * 4 + e] = oc < OC ? w[((size_t)t * cg + k) * OC + oc] : 0.f;
        }
}

template <class Kern>
static void gc_launch_mfma(Kern kern, const float* in, const float* w, const float* alpha, const float* beta, float* out,
                           const GroupedGeom& g, hipStream_t stream) {
  const int nquads = (g.M + 3) / 4, ngroups = (nquads + GC_P - 1) / GC_P, ntiles = (g.OC + 63) / 64;
  // resident workgroups over the chip, shared among the channel tiles; the waves stride the groups
  const int per_wg = GC_THREADS / 64;
  const int want = (ngroups + per_wg - 1) / per_wg;
  const int cap = std::max(1, device_cu_count() * 8 / ntiles);
  hipLaunchKernelGGL(kern, dim3(std::min(want, cap), ntiles), dim3(GC_THREADS), 0, stream, in, w, alpha, beta, out, g,
                     ngroups);
}

int launch_conv_grouped(const float* in, const float* w, const float* alpha, const float* beta, float* out, int n, int H,
                        int W, int C, int OH, int OW, int OC, int kh, int kw, int sh, int sw, int ph, int pw, int groups,
                        int flags, hipStream_t stream) {
  DNN_REQUIRE(in && w && out, "launch_conv_grouped: NULL tensor");
  DNN_REQUIRE(n >= 0 && H > 0 && W > 0 && C > 0 && OH > 0 && OW > 0 && OC > 0 && kh > 0 && kw > 0 && sh > 0 && sw > 0,
              "launch_conv_grouped: bad shape n=%d %dx%dx%d -> %dx%dx%d k%dx%d", n, H, W, C, OH, OW, OC, kh, kw);
  DNN_REQUIRE(groups >= 1 && C % groups == 0 && OC % groups == 0,
              "launch_conv_grouped: groups %d does not divide %d input and %d output channels", groups, C, OC);
  DNN_REQUIRE(!(flags & EPI_BN_AB) || (alpha && beta), "launch_conv_grouped: affine epilogue without alpha / beta");
  DNN_REQUIRE((unsigned long long)n * H * W * C * 4 < 0x80000000ULL && (unsigned long long)n * OH * OW * OC * 4 < 0x80000000ULL,
              "launch_conv_grouped: a tensor of n=%d %dx%dx%d -> %dx%dx%d is >= 2 GiB; split the batch", n, H, W, C, OH,
              OW, OC);
  if (n == 0) return 0;
  GroupedGeom g{n * OH * OW, H, W, C, OH, OW, OC, kh, kw, sh, sw, ph, pw, C / groups, OC / groups, flags};
  const bool al16 = ((reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(w) |
                      reinterpret_cast<uintptr_t>(alpha) | reinterpret_cast<uintptr_t>(beta)) & 15) == 0;
  const int taps = kh * kw;
  DNN_REQUIRE(al16 || C % 4 != 0, "launch_conv_grouped: tensors with C %% 4 == 0 must be 16-byte aligned");
  if (conv_grouped_mfma(C, OC, groups)) {
    const int cg4 = g.cg / 4;
#define GC_RES(CG4, TAPS, TC)                                                                                      \
  if (cg4 == CG4 && taps == TAPS && (TAPS == 1 || (kh == 3 && kw == 3)))                                           \
    gc_launch_mfma(gconv_mfma_resident<CG4, TAPS, TC>, in, w, alpha, beta, out, g, stream);                        \
  else
    GC_RES(1, 9, 9) GC_RES(2, 9, 9) GC_RES(4, 9, 9) GC_RES(8, 9, GC_BUDGET / 32)
    GC_RES(1, 1, 1) GC_RES(2, 1, 1) GC_RES(4, 1, 1) GC_RES(8, 1, 1)
    gc_launch_mfma(gconv_mfma_streamed, in, w, alpha, beta, out, g, stream);
#undef GC_RES
  } else if (g.cg == 1 && g.og == 1 && C % 4 == 0 && kh == kw && (kh == 3 || kh == 5) && sh == sw &&
             (sh == 1 || sh == 2)) {
    const int nstrips = (OH + DW_STRIP - 1) / DW_STRIP;
    const long long total = (long long)n * nstrips * OW * (C / 4);
    const dim3 grid((unsigned)((total + GC_THREADS - 1) / GC_THREADS)), block(GC_THREADS);
    if (kh == 3 && sh == 1)
      hipLaunchKernelGGL((gconv_depthwise<3, 1>), grid, block, 0, stream, in, w, alpha, beta, out, g, nstrips, total);
    else if (kh == 3)
      hipLaunchKernelGGL((gconv_depthwise<3, 2>), grid, block, 0, stream, in, w, alpha, beta, out, g, nstrips, total);
    else if (sh == 1)
      hipLaunchKernelGGL((gconv_depthwise<5, 1>), grid, block, 0, stream, in, w, alpha, beta, out, g, nstrips, total);
    else
      hipLaunchKernelGGL((gconv_depthwise<5, 2>), grid, block, 0, stream, in, w, alpha, beta, out, g, nstrips, total);
  } else {
    const long long total = (long long)g.M * OC;
    hipLaunchKernelGGL(gconv_scalar, dim3((unsigned)((total + GC_THREADS - 1) / GC_THREADS)), dim3(GC_THREADS), 0, stream,
                       in, w, alpha, beta, out, g);
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("launch conv_grouped: %s", hipGetErrorString(e));
    return -1;
  }
  return 0;
}

}  // namespace dnnhip
