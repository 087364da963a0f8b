// What the wide 3x3 conv kernels share, device code (and two constexpr host functions) only: the
// BM x 256 tile frame, the row-skewed LDS patch with its DMA, the chunk loop of the two kernels on
// that patch, and the tail that leaves through a wave-private LDS stage as 16-B stores.
//   conv3x3_f16_acc_kernel  (gemm_f16_acc.h)   frame, skewed patch, chunk loop, staged tail
//   conv3x3_x3_h2_kernel    (gemm_x3_h2.h)     frame, skewed patch, chunk loop, staged tail
//   conv3x3_x3_acc2_kernel  (gemm_x3_acc2.h)   frame, staged tail (its unpooled outputs)
// Each kernel keeps its operand format, its weight addressing, its MFMA block and its stores.
#pragma once
#include <type_traits>
#include "gemm_x3_patch.h"

namespace dnnhip {

template <int I, int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (I < N) {
    f(std::integral_constant<int, I>{});
    static_for<I + 1, N>(f);
  }
}
template <int N>
__device__ __forceinline__ void vm_wait() {
  static_assert(N >= 0 && N < 64, "vmcnt range");
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// ---- The tile frame: 8 waves, wave `wid` owns the BM x 32 block at (m0, n0) of tile (tm, tn),
// tiles N-major inside each XCD's contiguous range (~31 M tiles of one N panel per XCD; round 4:
// 2 panels x ~16 M tiles per XCD, so each patch is fetched from beyond L2 by 2 XCDs instead of 4,
// measured within 0.5 % on conv4-conv7: the patch DMA's beyond-L2 bytes are not what costs).
// Output pixel m of an H x W frame is row padded(m) of the zero-bordered [B][H+2][W+2] input; its
// tap (dy, dx) is row padded(m) + (dy-1)(W+2) + (dx-1), so a tile reads one contiguous run of
// padded rows from P0 on.
// SPLITK: the grid is g.splits copies of the tiles, copy `split` takes that slice of K.  g: the
// kernel's geometry argument (H, W).
// padded() and P0 are for raster rows (row m = pixel m).  A kernel whose rows are pool-window-major
// (acc2's POOL forms) maps its rows itself: it takes neither from here, only frag_m() and
// patch_row() with its own first row.
template <int BM, bool SPLITK = false>
struct WideFrame {
  int lane, wid, fr, fq, split, tn, tm, m0, n0, H, W, Wp, HWo, P0;
  template <class G>
  __device__ __forceinline__ WideFrame(int tilesM, const G& g) {
    lane = threadIdx.x & 63;
    wid = wave_uniform(threadIdx.x >> 6);
    int tile = xcd_tile(blockIdx.x, gridDim.x);
    split = 0;
    if constexpr (SPLITK) {
      const int ntiles = gridDim.x / g.splits;
      split = tile / ntiles, tile = tile - split * ntiles;
    }
    tn = tile / tilesM, tm = tile - tn * tilesM;
    m0 = tm * BM, n0 = tn * 256 + wid * 32;  // this wave's 32 columns
    H = g.H, W = g.W, Wp = g.W + 2, HWo = g.H * g.W;
    P0 = padded(m0) - (Wp + 1);
    fr = lane & 15, fq = lane >> 4;  // the lane's row and k group of a 16 x 16 x 32 fragment
  }
  __device__ __forceinline__ int padded(int m) const {
    const int b = m / HWo, r = m - b * HWo, oy = r / W, ox = r - oy * W;
    return (b * (H + 2) + oy + 1) * Wp + ox + 1;
  }
  // padded row p as a patch row: relative to the first, P0_, and to its tap (0, 0)
  __device__ __forceinline__ int patch_row(int p, int P0_) const { return p - P0_ - (Wp + 1); }
  // the output row of row block i's A fragment (rows past M repeat row M - 1)
  __device__ __forceinline__ int frag_m(int i, int M) const {
    const int m = m0 + 16 * i + fr;
    return m < M ? m : M - 1;
  }
};

// ---- The row-skewed LDS patch (tools/lds_conflict_model.py: 3.72 -> 0.36 extra conflict cycles
// per fragment read at 13-wide frames): rows of LP bytes (128 data bytes + 32 never-read ones);
// patch row P (relative to the tile's first, P0) sits at LDS unit U(P) = PU P + SK y(P), y(P) =
// (q0 + P) / Wp its image row (q0 = P0 % Wp), so the 3-position jump of an image-row wrap inside a
// 16-row fragment lands like a 1-position step.  A tap (dy, dx) adds the uniform PU (dy Wp + dx) +
// SK dy units (a tap-(0, 0) row's column is < W, so dx never crosses a row).
template <int LP = 160, int SK = 12>
struct SkewPatch {
  static constexpr int PU = LP / 16, NW = 8;
  // 16-B units that `rows` patch rows of Wp-wide image rows take, and the bytes of one buffer of a
  // kernel compiled for NPR rows (whole 1-KiB DMA pieces per wave).  conv_patch16_supported /
  // launch_conv_patch16 (at the tile's span) and conv_x3_h2_supported (at NPR) hold 16 units(..)
  // <= buf_bytes(NPR); the kernels rely on it.
  __host__ __device__ static constexpr long long units(long long rows, int Wp) { return rows * PU + SK * (rows / Wp + 2); }
  __host__ __device__ static constexpr int pieces(int NPR) { return (NPR * LP + NW * 1024 - 1) / (NW * 1024); }
  __host__ __device__ static constexpr int buf_bytes(int NPR) { return pieces(NPR) * NW * 1024; }

  int Wp, q0;
  __device__ __forceinline__ SkewPatch(int Wp_, int P0) : Wp(Wp_), q0(P0 % Wp_) {}
  __device__ __forceinline__ int unit(int pr) const { return PU * pr + SK * ((q0 + pr) / Wp); }
  __device__ __forceinline__ int tap_bytes(int t) const { return (PU * ((t / 3) * Wp + (t % 3)) + SK * (t / 3)) * 16; }
  // DMA piece k of wave `wid` = the 1 KiB at lds + 1024 (wid + 8 k), lane's 16 B = unit U; with V =
  // U + PU q0 = RU j + PU x + u (RU = PU Wp + SK units per image row): patch row P = Wp j + x - q0,
  // unit u (units 8, 9 of a row: the next 32 bytes of global memory; x >= Wp: the SK spare units,
  // given row P's last unit) -- never read.  One 16-B unit from P rowB + 16 u + soff.
  __device__ __forceinline__ void issue(__amdgpu_buffer_rsrc_t rsA, unsigned char* lds, int k, int wid, int lane,
                                        int rowB, unsigned soff) const {
    const unsigned RU = (unsigned)(PU * Wp + SK);
    const unsigned V = 64u * (unsigned)(wid + NW * k) + (unsigned)lane + (unsigned)(PU * q0);
    const unsigned jr = V / RU, rem = V - jr * RU;
    unsigned x = rem / PU, u = rem - x * PU;
    if (x >= (unsigned)Wp) x = Wp - 1, u = PU - 1;
    const unsigned r = (unsigned)Wp * jr + x - (unsigned)q0;
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, (__attribute__((address_space(3))) void*)(lds + 1024 * (wid + NW * k)),
                                             16, (int)(__umul24(r, (unsigned)rowB) + 16 * u), (int)soff, 0, 0);
  }
};

// ---- The chunk loop on a skewed patch.  A chunk is RB bytes of every patch row (fragments of two
// Frag: q and q + 64), LDS-DMA'd into the other half of a double buffer while the current one runs:
// no staging registers, one barrier per chunk.  Per chunk 9 taps x TM row blocks (b = TM t + i, all
// static); block(i, a, bb, rd) issues row block i's MFMAs on the A fragments a[2] and the tap's
// weights bb[2][NJ] and calls rd() once among them: the A fragments of block b + 2 are read during
// block b (a ring of three sets; 9 TM % 3 == 0, so every chunk starts at slot 0; a 3-block lead
// with a ring of 9 measured equal, a one-block lead leaves the LDS latency exposed).  The 2 NJ
// weight fragments of tap t + 1 (load_b1(step, p, j, dst)) and DMA piece t of chunk j + 1 are
// issued one per row block over the tap's first blocks (a lone wave stalls ~60 cycles per
// vector-memory issue).  Past the last chunk both read in-range or zero-filled bytes into
// registers / the buffer nobody reads.  rowoff_of(i): byte offset of block i's tap-(0, 0) fragment.
template <int TM, int NJ, int NPR, int RB, class Frag, class SP, class LoadB, class RowOff, class Block>
__device__ __forceinline__ void wide_skew_loop(unsigned char* smem, const SP& sp, __amdgpu_buffer_rsrc_t rsA, int wid,
                                               int lane, int rowB, unsigned dsoff, int nch, LoadB&& load_b1,
                                               RowOff&& rowoff_of, Block&& block) {
  constexpr int NQW = SP::pieces(NPR), BUFB = SP::buf_bytes(NPR);
  constexpr int LEAD = 2, RING = 3;
  static_assert(TM >= 2 * NJ + 1, "row blocks to spread the tap's loads over");
  static_assert((9 * TM) % RING == 0 && LEAD < RING && LEAD >= 1, "fragment ring phase per chunk");
  auto issue_patch = [&](int chunk, int k, int buf) {
    sp.issue(rsA, smem + buf * BUFB, k, wid, lane, rowB, dsoff + chunk * RB);
  };
  Frag bq[2][2][NJ];
#pragma unroll
  for (int k = 0; k < NQW; ++k) issue_patch(0, k, 0);
#pragma unroll
  for (int p = 0; p < 2; ++p)
#pragma unroll
    for (int j = 0; j < NJ; ++j) load_b1(0, p, j, bq[0][p][j]);
  vm_wait<0>();
  __syncthreads();

  const unsigned char* P = smem;
  Frag af[RING][2];
  auto rd = [&](int slot, const unsigned char* q) {
    af[slot][0] = *reinterpret_cast<const Frag*>(q);
    af[slot][1] = *reinterpret_cast<const Frag*>(q + 64);
  };
  auto blk = [&](const unsigned char* Pb, int bi) { return Pb + rowoff_of(bi % TM) + sp.tap_bytes(bi / TM); };
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
        block(i, af[bi % RING], bq[t & 1], [&] {
          if (bi + LEAD < 9 * TM) rd((bi + LEAD) % RING, blk(P, bi + LEAD));  // (the next chunk's first: after its barrier)
        });
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
}

// ---- The staged tail.  The row table (output record of each of the tile's BM rows: the padded
// row or m itself, -1 past M) takes the first KiB of the patch buffers; each row block's 16 x 32
// outputs of the wave then pass through a wave-private LDS stage (fp32 rows of 36: the
// MFMA-layout writes are conflict-free) and leave through store8(o, lo, hi): lane l has row l / 4
// (record o), columns n0 + c8 .. + 7 (wide_c8), where the MFMA layout would store one scalar per output.
// `apply`: the fp32 epilogue on the way (per column x3_epi_col, epilogue_batch: same arithmetic
// per value as apply_epilogue_t).  LDSB: the bytes of the kernel's LDS.
__device__ __forceinline__ int wide_c8(int lane) { return 8 * (lane & 3); }
template <int BM, int LDSB, int FL, class Frame, int TM, int NJ, class Store8>
__device__ __forceinline__ void wide_staged_tail(unsigned char* smem, const Frame& f, int M, bool to_padded,
                                                 const EpiParams& epi, bool apply, const f32x4 (&acc)[TM][NJ],
                                                 Store8&& store8) {
  constexpr int NW = 8;
  static_assert(BM * 4 <= 1024 && 1024 + NW * 16 * 36 * 4 <= LDSB, "row table below the stages");
  int* orow = reinterpret_cast<int*>(smem);
  __syncthreads();
  if (threadIdx.x < BM) {
    const int m = f.m0 + threadIdx.x;
    orow[threadIdx.x] = m >= M ? -1 : (to_padded ? f.padded(m) : m);
  }
  __syncthreads();
  float* const stg = reinterpret_cast<float*>(smem + 1024) + f.wid * (16 * 36);
  float pb[NJ], pm[NJ], ps[NJ], pg[NJ];
#pragma unroll
  for (int jb = 0; jb < NJ; ++jb) {
    const X3EpiCol ec = x3_epi_col(epi, FL < 0 ? epi.flags : FL, f.n0 + 16 * jb + f.fr);
    pb[jb] = ec.pb, pm[jb] = ec.pm, ps[jb] = ec.ps, pg[jb] = ec.pg;
  }
  const int rr = f.lane >> 2, c8 = wide_c8(f.lane);
  static_for<0, TM>([&](auto ic) {
    constexpr int i = decltype(ic)::value;
    float v[4][NJ];
#pragma unroll
    for (int jb = 0; jb < NJ; ++jb)
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r][jb] = acc[i][jb][r];
    if (apply) epilogue_batch<FL>(v, pb, pm, ps, pg, epi.flags);
#pragma unroll
    for (int jb = 0; jb < NJ; ++jb)
#pragma unroll
      for (int r = 0; r < 4; ++r) stg[(4 * f.fq + r) * 36 + 16 * jb + f.fr] = v[r][jb];
    wait_lgkm0();
    const f32x4 lo = *reinterpret_cast<const f32x4*>(stg + rr * 36 + c8);
    const f32x4 hi = *reinterpret_cast<const f32x4*>(stg + rr * 36 + c8 + 4);
    const int o = orow[16 * i + rr];
    wait_lgkm0();  // (the stage is rewritten by the next row block)
    if (o >= 0) store8(o, lo, hi);
  });
}

// store8 of the fp32 kernels: the lane's eight values of output record o, columns n0 + c8 .. + 7, as
// the three bf16 planes of a following x3 layer (out_mode 1: 3 stores), the two fp16 planes of a
// following h2 layer (3: h2_store8, 2 stores) or fp32 at row row0 + o of [..][N] (2 stores).
__device__ __forceinline__ void x3_wide_store8(int o, f32x4 lo, f32x4 hi, int out_mode, size_t row0, int n0, int c8,
                                               int N, float* __restrict__ out, bf16_bits* __restrict__ out_split,
                                               unsigned* __restrict__ range_flag) {
  if (out_mode == 1) {
    x3_store8(lo, hi, out_split, (size_t)o * (3 * N) + (n0 >> 5) * 96 + c8);
  } else if (out_mode == 3) {
    const float v8[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    h2_store8(v8, out_split, (size_t)o * (4 * (size_t)N) + (n0 >> 5) * 128 + 2 * c8, range_flag);
  } else {
    const size_t d = (row0 + o) * N + n0 + c8;  // (floats)
    store16_at(out, 4 * d, __builtin_bit_cast(u32x4, lo));
    store16_at(out, 4 * d + 16, __builtin_bit_cast(u32x4, hi));
  }
}

}  // namespace dnnhip
