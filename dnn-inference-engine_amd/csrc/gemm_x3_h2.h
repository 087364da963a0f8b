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
// Structure: conv3x3_f16_acc_kernel's (gemm_f16_acc.h), whose 128-B row data this layout shares
// (per pixel and 32-channel chunk 64 B of g0, then 64 B of g1): BM x 256 tiles, 8 waves of BM x 32,
// two per SIMD; the patch of a chunk LDS-DMA'd into a double buffer of 160-B rows skewed by 12
// units per image row (tools/lds_conflict_model.py: 0.36 extra conflict cycles per fragment read
// at 13-wide frames); the weights of the next tap (4 fragments) loaded while this one runs; the A
// fragments read two row blocks ahead through a ring of three sets (a row block is 6 MFMAs).
// Weights: [n/16][step][piece(2)][lane][8] halves, 2048 B per step (pack_weights_h2_kernel).
// Output: fp32 [M][N], the three bf16 planes of a following x3 layer (conv8's 1x1), or the two
// fp16 planes of a following h2 layer.
#pragma once
#include "gemm_x3_acc2.h"

namespace dnnhip {

typedef _Float16 h2x8 __attribute__((ext_vector_type(8)));
__device__ __forceinline__ f32x4 mfma16_h2(h2x8 a, h2x8 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
}

constexpr int X3H2_LP = 160, X3H2_SK = 12;  // LDS row bytes, skew units per image row (the launcher's fit check)

// FL: the epilogue flag set at compile time (-1: runtime `epi.flags`), as conv3x3_x3_acc2_kernel
template <int BM, int NPR, int FL = -1>
__global__ void __launch_bounds__(512, 2)
conv3x3_x3_h2_kernel(const bf16_bits* __restrict__ in, const bf16_bits* __restrict__ Bt, float* __restrict__ out,
                     bf16_bits* __restrict__ out_split, int M, int N, int K, EpiParams epi, int tilesM, X3Geom g,
                     unsigned in_bytes, unsigned b_bytes, unsigned* __restrict__ range_flag) {
  constexpr int BN = 256, TM = BM / 16, RB = 128, NJ = 2, NW = 8, LP = X3H2_LP;
  constexpr int NQW = (NPR * LP + NW * 1024 - 1) / (NW * 1024);  // 1-KiB DMA pieces per wave per patch
  constexpr int BUFB = NQW * NW * 1024;
  static_assert(BM % 16 == 0 && NQW <= 9 && NPR <= 1023 && TM >= 2 * NJ + 1, "shape");
  // (the skewed rows need NPR PU + SK (NPR / Wp + 2) units: the launcher checks it against BUFB)
  __shared__ __attribute__((aligned(1024))) unsigned char smem[2 * BUFB];

  const int lane = threadIdx.x & 63;
  const int wid = wave_uniform(threadIdx.x >> 6);
  const int tile = xcd_tile(blockIdx.x, gridDim.x);
  const int tn = tile / tilesM, tm = tile - tn * tilesM;
  const int m0 = tm * BM, n0 = tn * BN + wid * 32;  // this wave's 32 columns
  const int Wp = g.W + 2, HWo = g.H * g.W;
  auto padded = [&](int m) {
    const int b = m / HWo, r = m - b * HWo, oy = r / g.W, ox = r - oy * g.W;
    return (b * (g.H + 2) + oy + 1) * Wp + ox + 1;
  };
  const int P0 = padded(m0) - (Wp + 1);  // first patch row

  // Row-skewed LDS layout (gemm_f16_acc.h): patch row P (relative to P0) sits at LDS unit U(P) =
  // PU P + SK y(P), y(P) = (q0 + P) / Wp its image row (q0 = P0 % Wp); a tap (dy, dx) adds the
  // uniform PU (dy Wp + dx) + SK dy units.  The fragment bases (unit + the lane's k group) are
  // packed two per register: the two accumulator sets leave no room for one each.
  constexpr int PU = LP / 16, SK = X3H2_SK;
  const int fr = lane & 15, fq = lane >> 4;
  const int q0 = P0 % Wp;
  constexpr int NPK = (TM + 1) / 2;
  unsigned prk[NPK];
#pragma unroll
  for (int k = 0; k < NPK; ++k) prk[k] = 0;
#pragma unroll
  for (int i = 0; i < TM; ++i) {
    int m = m0 + 16 * i + fr;
    m = m < M ? m : M - 1;
    const int pr = padded(m) - P0 - (Wp + 1);
    prk[i / 2] |= (unsigned)(PU * pr + SK * ((q0 + pr) / Wp) + fq) << (16 * (i % 2));
  }
  auto rowoff_of = [&](int i) {
    unsigned w = prk[i / 2];
    asm volatile("" : "+v"(w));  // unpacked per use
    return (int)(((w >> (16 * (i % 2))) & 0xffffu) << 4);
  };
  auto tap_bytes = [&](int t) { return (PU * ((t / 3) * Wp + (t % 3)) + SK * (t / 3)) * 16; };

  // patch DMA: piece k of this wave = LDS bytes 1024 (wid + 8 k) + 16 lane = unit U; with V = U +
  // PU q0 = RU j + PU x + u (RU = PU Wp + SK units per image row): patch row P = Wp j + x - q0,
  // unit u (units 8, 9 of a row: the next 32 bytes of global memory; x >= Wp: the SK spare units,
  // given row P's last unit) -- never read
  const int nk = K / 32, nch = nk / 9;
  const int rowB = 4 * g.C;
  const auto rsA = __builtin_amdgcn_make_buffer_rsrc((void*)in, 0, (int)in_bytes, 0x00020000);
  const unsigned dsoff = (unsigned)(P0 * rowB);
  const unsigned RU = (unsigned)(PU * Wp + SK);
  auto issue_patch = [&](int chunk, int k, int buf) {
    const unsigned V = 64u * (unsigned)(wid + NW * k) + (unsigned)lane + (unsigned)(PU * q0);
    const unsigned jr = V / RU, rem = V - jr * RU;
    unsigned x = rem / PU, u = rem - x * PU;
    if (x >= (unsigned)Wp) x = Wp - 1, u = PU - 1;
    const unsigned r = (unsigned)Wp * jr + x - (unsigned)q0;
    __builtin_amdgcn_raw_ptr_buffer_load_lds(
        rsA, (__attribute__((address_space(3))) void*)(smem + buf * BUFB + 1024 * (wid + NW * k)), 16,
        (int)(__umul24(r, (unsigned)rowB) + 16 * u), (int)(dsoff + chunk * RB), 0, 0);
  };

  // weights [n/16][step][piece][lane][8]: the wave's two 16-column blocks, one tap ahead
  const unsigned bvo = (unsigned)((n0 / 16) * nk * 2048 + lane * 16);
  const int bjs = nk * 2048;
  const auto rsB = __builtin_amdgcn_make_buffer_rsrc((void*)Bt, 0, (int)b_bytes, 0x00020000);
  h2x8 bq[2][2][NJ];
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

#pragma unroll
  for (int k = 0; k < NQW; ++k) issue_patch(0, k, 0);
#pragma unroll
  for (int p = 0; p < 2; ++p)
#pragma unroll
    for (int j = 0; j < NJ; ++j) load_b1(0, p, j, bq[0][p][j]);
  vm_wait<0>();
  __syncthreads();

  // Per chunk: 9 taps x TM row blocks (b = TM t + i, all static), 6 MFMAs each: per column block
  // g1 h0 and g0 h1 onto accc, g0 h0 onto accm, the two column blocks interleaved so that an
  // accumulator's next MFMA is two issues away.  The A fragments of block b + 2 are read during
  // block b (9 TM % 3 == 0: every chunk starts at ring slot 0).  Weights of tap t + 1 and DMA piece
  // t of chunk j + 1 are issued one per row block over the tap's first blocks.  (Past the last
  // chunk both read in-range or zero-filled bytes into registers / the buffer nobody reads.)
  constexpr int LEAD = 2, RING = 3;
  static_assert((9 * TM) % RING == 0 && LEAD < RING && LEAD >= 1, "fragment ring phase per chunk");
  const unsigned char* P = smem;
  h2x8 af[RING][2];
  auto rd = [&](int slot, const unsigned char* q) {
    af[slot][0] = *reinterpret_cast<const h2x8*>(q);
    af[slot][1] = *reinterpret_cast<const h2x8*>(q + 64);
  };
  auto blk = [&](const unsigned char* Pb, int bi) { return Pb + rowoff_of(bi % TM) + tap_bytes(bi / TM); };
#pragma unroll
  for (int l = 0; l < LEAD; ++l) rd(l, blk(P, l));
  for (int j = 0; j < nch; ++j) {
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        const int bi = TM * t + i;
        static_for<0, 2 * NJ + 1>([&](auto qc) {
          constexpr int q = decltype(qc)::value;
          if (i != q) return;
          if constexpr (q < 2 * NJ)
            load_b1(9 * j + t + 1, q / NJ, q % NJ, bq[(t + 1) & 1][q / NJ][q % NJ]);
          else
            issue_patch(j + 1, t < NQW ? t : NQW - 1, (j + 1) & 1);
        });
        const h2x8(&a)[2] = af[bi % RING];
        const h2x8(&bb)[2][NJ] = bq[t & 1];
#pragma unroll
        for (int jb = 0; jb < NJ; ++jb) accc[i][jb] = mfma16_h2(a[1], bb[0][jb], accc[i][jb]);
        if (bi + LEAD < 9 * TM) rd((bi + LEAD) % RING, blk(P, bi + LEAD));  // (the next chunk's first: after its barrier)
#pragma unroll
        for (int jb = 0; jb < NJ; ++jb) accc[i][jb] = mfma16_h2(a[0], bb[1][jb], accc[i][jb]);
#pragma unroll
        for (int jb = 0; jb < NJ; ++jb) accm[i][jb] = mfma16_h2(a[0], bb[0][jb], accm[i][jb]);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    // the next chunk's tap 0 weights went to bq[9 & 1]
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
      for (int jb = 0; jb < NJ; ++jb) bq[0][p][jb] = bq[1][p][jb];
    vm_wait<0>();  // this wave's DMA pieces landed
    wait_lgkm0();
    raw_barrier();
    P = smem + ((j + 1) & 1) * BUFB;
#pragma unroll
    for (int l = 0; l < LEAD; ++l) rd(l, blk(P, l));
  }
  vm_wait<0>();
  wait_lgkm0();

  // epilogue: the reference's fp32 epilogue on accm + accc 2^-11, then fp32 [M][N] or the planes
  // of the next layer's zero-bordered input (gemm_x3_acc2.h's staged 16-B stores)
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int jb = 0; jb < NJ; ++jb)
#pragma unroll
      for (int r = 0; r < 4; ++r) accm[i][jb][r] = accm[i][jb][r] + accc[i][jb][r] * 0x1p-11f;
  int* orow = reinterpret_cast<int*>(smem);
  __syncthreads();
  if (threadIdx.x < BM) {
    const int m = m0 + threadIdx.x;
    orow[threadIdx.x] = m >= M ? -1 : (g.out_mode != 0 ? padded(m) : m);
  }
  __syncthreads();
  static_assert(BM * 4 <= 1024 && 1024 + NW * 16 * 36 * 4 <= 2 * BUFB, "row table below the stages");
  float* const stg = reinterpret_cast<float*>(smem + 1024) + wid * (16 * 36);
  float pb[NJ], pm[NJ], ps[NJ], pg[NJ];
#pragma unroll
  for (int jb = 0; jb < NJ; ++jb) {
    const X3EpiCol ec = x3_epi_col(epi, FL < 0 ? epi.flags : FL, n0 + 16 * jb + fr);
    pb[jb] = ec.pb, pm[jb] = ec.pm, ps[jb] = ec.ps, pg[jb] = ec.pg;
  }
  const int rr = lane >> 2, c8 = 8 * (lane & 3);
  static_for<0, TM>([&](auto ic) {
    constexpr int i = decltype(ic)::value;
    float v[4][NJ];
#pragma unroll
    for (int jb = 0; jb < NJ; ++jb)
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r][jb] = accm[i][jb][r];
    epilogue_batch<FL>(v, pb, pm, ps, pg, epi.flags);
#pragma unroll
    for (int jb = 0; jb < NJ; ++jb)
#pragma unroll
      for (int r = 0; r < 4; ++r) stg[(4 * fq + r) * 36 + 16 * jb + fr] = v[r][jb];
    wait_lgkm0();
    const f32x4 lo = *reinterpret_cast<const f32x4*>(stg + rr * 36 + c8);
    const f32x4 hi = *reinterpret_cast<const f32x4*>(stg + rr * 36 + c8 + 4);
    const int o = orow[16 * i + rr];
    wait_lgkm0();  // (the stage is rewritten by the next row block)
    if (o >= 0) {
      if (g.out_mode == 1) {  // three bf16 pieces (a following x3 layer)
        bool ok = true;
#pragma unroll
        for (int e = 0; e < 4; ++e) ok = ok && x3_split_ok(lo[e]) && x3_split_ok(hi[e]);
        const bool fast = __builtin_amdgcn_ballot_w64(!ok) == 0;  // (over the active lanes: uniform among them)
        u32x4 q[3];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          unsigned w0, w1, w2;
          split3_pack2(fast, e < 2 ? lo[2 * e] : hi[2 * e - 4], e < 2 ? lo[2 * e + 1] : hi[2 * e - 3], w0, w1, w2);
          q[0][e] = w0;
          q[1][e] = w1;
          q[2][e] = w2;
        }
        const size_t d = (size_t)o * (3 * N) + (n0 >> 5) * 96 + c8;  // (halves)
#pragma unroll
        for (int pc = 0; pc < 3; ++pc) store16_at(out_split, 2 * (d + 32 * pc), q[pc]);
      } else if (g.out_mode == 3) {  // two fp16 pieces (a following h2 layer)
        const float v8[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        h2_store8(v8, out_split, (size_t)o * (4 * (size_t)N) + (n0 >> 5) * 128 + 2 * c8, range_flag);
      } else {
        const size_t d = (size_t)o * N + n0 + c8;  // (floats)
        store16_at(out, 4 * d, __builtin_bit_cast(u32x4, lo));
        store16_at(out, 4 * d + 16, __builtin_bit_cast(u32x4, hi));
      }
    }
  });
}

}  // namespace dnnhip
