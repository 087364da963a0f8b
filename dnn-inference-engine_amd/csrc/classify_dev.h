// Device pieces the classifier tail's row kernels share (classify.hip: softmax and top-k): staging a
// score row into LDS and the workgroup-wide reductions.  A reduction runs in a fixed order that depends
// on the workgroup size alone: an xor butterfly of wave shuffles (every lane ends with the same bits,
// since each step combines the same two values on both sides), one partial per wave through LDS, and
// every thread combining the partials wave 0 first.  No atomics.
#pragma once
#include <hip/hip_runtime.h>
#include <climits>

namespace dnnhip {

typedef float cls_f32x4 __attribute__((ext_vector_type(4)));

constexpr int CLS_WAVE = 64;
constexpr int CLS_MAX_WAVES = 16;  // 1024 threads

// src[0 .. count) -> row[0 .. count), coalesced; vec: count % 4 == 0 and src 16-byte aligned (row is)
__device__ __forceinline__ void stage_row(const float* __restrict__ src, float* row, int count, bool vec) {
  const int tid = threadIdx.x, T = blockDim.x;
  if (vec) {
    const cls_f32x4* s4 = reinterpret_cast<const cls_f32x4*>(src);
    cls_f32x4* r4 = reinterpret_cast<cls_f32x4*>(row);
    for (int q = tid; q < (count >> 2); q += T) r4[q] = s4[q];
  } else {
    for (int i = tid; i < count; i += T) row[i] = src[i];
  }
}

struct ClsMax {
  static __device__ __forceinline__ float apply(float a, float b) { return a > b ? a : b; }
};
struct ClsSum {
  static __device__ __forceinline__ float apply(float a, float b) { return a + b; }
};

// Op over the workgroup's values; `red` holds CLS_MAX_WAVES floats no other reduction in flight uses.
// Contains one barrier, after which every thread has the result (and sees the LDS writes before it).
template <class Op>
__device__ __forceinline__ float block_reduce(float v, float* red) {
#pragma unroll
  for (int o = CLS_WAVE / 2; o > 0; o >>= 1) v = Op::apply(v, __shfl_xor(v, o, CLS_WAVE));
  const int wave = threadIdx.x / CLS_WAVE, nw = blockDim.x / CLS_WAVE;
  if ((threadIdx.x & (CLS_WAVE - 1)) == 0) red[wave] = v;
  __syncthreads();
  float r = red[0];
  for (int w = 1; w < nw; ++w) r = Op::apply(r, red[w]);
  return r;
}

// (value, index) order of the top-k: the larger value, among equal values the lower index.  A NaN
// value never wins (both comparisons are false): it marks an entry already taken.
__device__ __forceinline__ bool cls_better(float v, int i, float bv, int bi) { return v > bv || (v == bv && i < bi); }

// the workgroup's best (value, index); red_v / red_i as block_reduce's red, one barrier
__device__ __forceinline__ void block_argmax(float& v, int& i, float* red_v, int* red_i) {
#pragma unroll
  for (int o = CLS_WAVE / 2; o > 0; o >>= 1) {
    const float ov = __shfl_xor(v, o, CLS_WAVE);
    const int oi = __shfl_xor(i, o, CLS_WAVE);
    if (cls_better(ov, oi, v, i)) v = ov, i = oi;
  }
  const int wave = threadIdx.x / CLS_WAVE, nw = blockDim.x / CLS_WAVE;
  if ((threadIdx.x & (CLS_WAVE - 1)) == 0) red_v[wave] = v, red_i[wave] = i;
  __syncthreads();
  v = red_v[0];
  i = red_i[0];
  for (int w = 1; w < nw; ++w)
    if (cls_better(red_v[w], red_i[w], v, i)) v = red_v[w], i = red_i[w];
}

}  // namespace dnnhip
