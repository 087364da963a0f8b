// fp16 3x3 conv for the long-K, wide-N layers of the fp16 path (conv6/conv7 of YOLOv2-tiny,
// BASELINE config 5), device code only.  This file owns the fp16 operand format (64-channel chunks
// of 128-B rows, weights in order 4), the MFMA block of a row block and the store of eight halves;
// the tile frame, the skewed patch and its DMA, the chunk loop and the staged tail are
// conv_wide_dev.h's (WideFrame, SkewPatch, wide_skew_loop, wide_staged_tail), shared with the fp32
// kernels on the same structure.
//
// Round 4: replaces conv3x3_f16_patch_kernel (register-staged 128-B rows with an XOR swizzle,
// weights two taps ahead, one scalar fp16 store per output), which held the fp16 MFMA at 45 % of
// its peak where the x3 kernel holds the same v_mfma 16x16x32 issue at 62-65 %:
//   * the patch of one 64-channel chunk (<= NPR zero-bordered input rows) is LDS-DMA'd
//     (buffer_load ... lds, 1-KiB pieces) into the other half of a double buffer while the
//     current chunk runs: no staging registers, one barrier per chunk;
//   * LDS rows of LP = 160 bytes (the 128 data bytes + 32 never-read ones), skewed by 12 units per
//     image row (below): 0.36 extra conflict cycles per fragment read (plain 160-B rows: 3.95,
//     the old kernel's swizzle ~4) -- at 2 reads per 4 MFMAs the fp16 loop is LDS-bound
//     (~2 x 7.7 LDS cycles per 16 at full MFMA rate with the conflicts);
//   * the tap's vector-memory instructions (4 weight fragments, 1 DMA piece) spread one per row
//     block over its first blocks; the A fragments read two row blocks ahead (a ring of three);
//   * the epilogue staged through a wave-private LDS tile: one 16-B fp16 store per lane and row
//     block instead of one 2-B store per output.
// Same products in the same order as the round-3 kernel (per output: chunk, tap, 32-channel group;
// v_mfma_f32_16x16x32_f16), same weight packing (order 4: [n/16][k/32][lane][8]), same epilogue
// arithmetic: same bits (checked against it on the GPU before it was removed).  Measured at batch
// 64 (same process, interleaved): conv7 0.175 -> 0.151 ms, conv6 0.098 -> 0.083 ms; the skew
// alone -0.4 %, the two-block fragment lead -9 % (one block: conv7 0.166).
//
// The input sits in HBM zero-padded ([B][H+2][W+2][C], borders written once at plan finalize), so
// output pixel m's tap (dy, dx) is padded row p(m) + (dy-1)(W+2) + (dx-1): a tile of BM consecutive
// output pixels reads one contiguous run of padded rows per 64-channel chunk, staged once and
// reused by all 9 taps.
#pragma once
#include "gemm_f16.h"
#include "conv_wide_dev.h"

namespace dnnhip {

struct Patch16Geom {
  int H, W, C;      // conv input = output spatial size (3x3, stride 1, SAME), channels
  int out_padded;   // 1: write the output into a zero-bordered [B][H+2][W+2][N] buffer
};

// v_mfma_f32_16x16x32_f16: lane l supplies A[row l&15][k 8(l>>4)..+7] and B likewise;
// D[row][col]: col = l&15, row = 4(l>>4) + reg.  (The same FLOP per cycle as 32x32x16; on
// random data the chip holds a higher clock for it, MI355X_MICROARCH DVFS item 7.)
__device__ __forceinline__ f32x4 mfma16_f16(f16x8 a, f16x8 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
}

template <int BM, int NPR, int FL = -1>
__global__ void __launch_bounds__(512, 2)
conv3x3_f16_acc_kernel(const half_t* __restrict__ in, const half_t* __restrict__ Bt, int ldb, half_t* __restrict__ out,
                       int M, int N, int K, EpiParams epi, int tilesM, Patch16Geom g, unsigned in_bytes,
                       unsigned b_bytes) {
  using SP = SkewPatch<160, 12>;
  constexpr int TM = BM / 16, RB = 128, NJ = 2, BUFB = SP::buf_bytes(NPR);
  static_assert(BM % 16 == 0 && SP::pieces(NPR) <= 9 && NPR <= 1023, "shape");
  // (the skewed rows need SP::units(NPR, Wp) units: patch16_fits checks the tile's span against BUFB)
  __shared__ __attribute__((aligned(1024))) unsigned char smem[2 * BUFB];

  const WideFrame<BM> f(tilesM, g);
  const SP sp(f.Wp, f.P0);
  // the fragment bases are per-block registers (the fp16 kernel has the room the x3 kernels lack)
  int rowoff[TM];
#pragma unroll
  for (int i = 0; i < TM; ++i)
    rowoff[i] = sp.unit(f.patch_row(f.padded(f.frag_m(i, M)), f.P0)) * 16 + 16 * f.fq;
  auto rowoff_of = [&](int i) {
    int v = rowoff[i];
    asm volatile("" : "+v"(v));
    return v;
  };

  const int nk = K / 64, nch = nk / 9;
  const int rowB = 2 * g.C;
  const auto rsA = __builtin_amdgcn_make_buffer_rsrc((void*)in, 0, (int)in_bytes, 0x00020000);
  const unsigned dsoff = (unsigned)(f.P0 * rowB);
  // weights (order 4): 16-column block nb at nb ldb 32 bytes, K-step s group q at (2 s + q) KiB
  const unsigned bvo = (unsigned)((f.n0 / 16) * ldb * 32 + f.lane * 16);
  const int bjs = ldb * 32;
  const auto rsB = __builtin_amdgcn_make_buffer_rsrc((void*)Bt, 0, (int)b_bytes, 0x00020000);
  auto load_b1 = [&](int s, int q, int j, f16x8& dst) {
    dst = __builtin_bit_cast(f16x8, __builtin_amdgcn_raw_buffer_load_b128(rsB, bvo, (2 * s + q) * 1024 + j * bjs, 0));
  };

  f32x4 acc[TM][NJ];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // a row block: 4 MFMAs (2 32-channel groups x 2 column blocks); at 2 fragment reads per 4 MFMAs
  // the loop is LDS-bound
  wide_skew_loop<TM, NJ, NPR, RB, f16x8>(
      smem, sp, rsA, f.wid, f.lane, rowB, dsoff, nch, load_b1, rowoff_of,
      [&](int i, const f16x8(&a)[2], const f16x8(&bb)[2][NJ], auto&& rd) {
#pragma unroll
        for (int jb = 0; jb < NJ; ++jb) acc[i][jb] = mfma16_f16(a[0], bb[0][jb], acc[i][jb]);
        rd();
#pragma unroll
        for (int jb = 0; jb < NJ; ++jb) acc[i][jb] = mfma16_f16(a[1], bb[1][jb], acc[i][jb]);
      });

  // the reference's fp16-path epilogue, then one 16-B store of 8 halves per lane and row block
  typedef half_t h8v __attribute__((ext_vector_type(8)));
  wide_staged_tail<BM, 2 * BUFB, FL>(smem, f, M, g.out_padded != 0, epi, true, acc, [&](int o, f32x4 lo, f32x4 hi) {
    h8v v;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      v[e] = (half_t)lo[e];
      v[e + 4] = (half_t)hi[e];
    }
    store16_at(out, 2 * ((size_t)o * N + f.n0 + wide_c8(f.lane)), __builtin_bit_cast(u32x4, v));
  });
}

}  // namespace dnnhip
