// fp32 3x3 conv on the fp16 MFMA with two-piece operand splits ("h2"): the wide x3 conv
// (gemm_x3_acc2.h) at three MFMA products per fp32 product instead of six, device code only.
//
// Arithmetic (the error-corrected fp16 scheme of Ootomo and Yokota): an fp32 operand a is the pair
// g0 = rn16(a), g1 = rn16((a - g0) * 2^11) (split2h, gemm_f32.h), within 2^-23 |a| of a; the
// weights are split alike into h0, h1.  Per output and 32-channel step
//   accc += g1 h0;  accc += g0 h1;  accm += g0 h0
// on v_mfma_f32_16x16x32_f16 (every product exact in the fp32 accumulator's input), and the output
// is accm + accc * 2^-11 (the scaling exact), then the unchanged fp32 epilogue.  The dropped term
// g1 h1 2^-22 is below fp32's own rounding.  Summation order: per output, both accumulators over
// the steps chunk-major, tap-minor; it depends on (N, K) only, so batch rows are bit-identical to
// batch-1 runs.  Range: fp16 pieces hold |a| < 65520 only; the producers flag anything else
// (h2_store8) and the plan checks the weights when it packs them.
//
// Structure (conv_wide_dev.h): BM x 256 tiles, 8 waves of BM x 32, two per SIMD (WideFrame); the
// patch of a 32-channel chunk (per pixel 64 B of g0, then 64 B of g1: the fp16 kernel's 128-B row
// data) LDS-DMA'd into a double buffer of 160-B rows skewed by 12 units per image row (SkewPatch);
// the weights of the next tap (4 fragments) loaded while this one runs and the A fragments read two
// row blocks ahead through a ring of three sets (wide_skew_loop); the outputs through a wave-private
// LDS stage (wide_staged_tail).  This file owns the packed fragment rows, the weight addressing, the
// row block's 6 MFMAs, the fold of the two accumulators and the three output forms.
// Weights: [n/16][step][piece(2)][lane][8] halves, 2048 B per step (pack_weights_h2_kernel).
// Output: fp32 [M][N], the three bf16 planes of a following x3 layer (conv8's 1x1), or the two
// fp16 planes of a following h2 layer.
#pragma once
#include "conv_wide_dev.h"

namespace dnnhip {

typedef _Float16 h2x8 __attribute__((ext_vector_type(8)));
__device__ __forceinline__ f32x4 mfma16_h2(h2x8 a, h2x8 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
}

using X3H2Patch = SkewPatch<160, 12>;  // (conv_x3_h2_supported checks its fit)

// FL: the epilogue flag set at compile time (-1: runtime `epi.flags`), as conv3x3_x3_acc2_kernel
template <int BM, int NPR, int FL = -1>
__global__ void __launch_bounds__(512, 2)
conv3x3_x3_h2_kernel(const bf16_bits* __restrict__ in, const bf16_bits* __restrict__ Bt, float* __restrict__ out,
                     bf16_bits* __restrict__ out_split, int M, int N, int K, EpiParams epi, int tilesM, X3Geom g,
                     unsigned in_bytes, unsigned b_bytes, unsigned* __restrict__ range_flag) {
  using SP = X3H2Patch;
  constexpr int TM = BM / 16, RB = 128, NJ = 2, BUFB = SP::buf_bytes(NPR);
  static_assert(BM % 16 == 0 && SP::pieces(NPR) <= 9 && NPR <= 1023, "shape");
  // (the skewed rows need SP::units(NPR, Wp) units: conv_x3_h2_supported checks it against BUFB)
  __shared__ __attribute__((aligned(1024))) unsigned char smem[2 * BUFB];

  const WideFrame<BM> f(tilesM, g);
  const SP sp(f.Wp, f.P0);
  // The fragment bases (unit + the lane's k group) are packed two per register: the two
  // accumulator sets leave no room for one each.
  constexpr int NPK = (TM + 1) / 2;
  unsigned prk[NPK];
#pragma unroll
  for (int k = 0; k < NPK; ++k) prk[k] = 0;
#pragma unroll
  for (int i = 0; i < TM; ++i)
    prk[i / 2] |= (unsigned)(sp.unit(f.patch_row(f.padded(f.frag_m(i, M)), f.P0)) + f.fq) << (16 * (i % 2));
  auto rowoff_of = [&](int i) {
    unsigned w = prk[i / 2];
    asm volatile("" : "+v"(w));  // unpacked per use
    return (int)(((w >> (16 * (i % 2))) & 0xffffu) << 4);
  };

  const int nk = K / 32, nch = nk / 9;
  const int rowB = 4 * g.C;
  const auto rsA = __builtin_amdgcn_make_buffer_rsrc((void*)in, 0, (int)in_bytes, 0x00020000);
  const unsigned dsoff = (unsigned)(f.P0 * rowB);
  // weights [n/16][step][piece][lane][8]: the wave's two 16-column blocks, one tap ahead
  const unsigned bvo = (unsigned)((f.n0 / 16) * nk * 2048 + f.lane * 16);
  const int bjs = nk * 2048;
  const auto rsB = __builtin_amdgcn_make_buffer_rsrc((void*)Bt, 0, (int)b_bytes, 0x00020000);
  auto load_b1 = [&](int s, int p, int j, h2x8& dst) {
    dst = __builtin_bit_cast(h2x8, __builtin_amdgcn_raw_buffer_load_b128(rsB, bvo, s * 2048 + p * 1024 + j * bjs, 0));
  };

  f32x4 accm[TM][NJ], accc[TM][NJ];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      accm[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
      accc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    }

  // a row block: 6 MFMAs, per column block g1 h0 and g0 h1 onto accc, g0 h0 onto accm, the two
  // column blocks interleaved so that an accumulator's next MFMA is two issues away
  wide_skew_loop<TM, NJ, NPR, RB, h2x8>(
      smem, sp, rsA, f.wid, f.lane, rowB, dsoff, nch, load_b1, rowoff_of,
      [&](int i, const h2x8(&a)[2], const h2x8(&bb)[2][NJ], auto&& rd) {
#pragma unroll
        for (int jb = 0; jb < NJ; ++jb) accc[i][jb] = mfma16_h2(a[1], bb[0][jb], accc[i][jb]);
        rd();
#pragma unroll
        for (int jb = 0; jb < NJ; ++jb) accc[i][jb] = mfma16_h2(a[0], bb[1][jb], accc[i][jb]);
#pragma unroll
        for (int jb = 0; jb < NJ; ++jb) accm[i][jb] = mfma16_h2(a[0], bb[0][jb], accm[i][jb]);
      });

  // epilogue: the reference's fp32 epilogue on accm + accc 2^-11, then fp32 [M][N] or the planes
  // of the next layer's zero-bordered input
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int jb = 0; jb < NJ; ++jb)
#pragma unroll
      for (int r = 0; r < 4; ++r) accm[i][jb][r] = accm[i][jb][r] + accc[i][jb][r] * 0x1p-11f;
  wide_staged_tail<BM, 2 * BUFB, FL>(smem, f, M, g.out_mode != 0, epi, true, accm, [&](int o, f32x4 lo, f32x4 hi) {
    x3_wide_store8(o, lo, hi, g.out_mode, 0, f.n0, wide_c8(f.lane), N, out, out_split, range_flag);
  });
}

}  // namespace dnnhip
