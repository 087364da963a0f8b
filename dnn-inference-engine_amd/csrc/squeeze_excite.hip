// Squeeze-and-excitation gate (Darknet's [avgpool] [convolutional 1x1] [convolutional 1x1] [scale_channels],
// the SE block of the MBConv networks), x [n, H, W, C] NHWC fp32 -> y of the same shape:
//
//   m[n, c] = (sum over the H * W positions of x[n, h, w, c]) / (H * W)
//   h[n, j] = act1(sum_c m[n, c] * W1[c, j] + b1[j])        j < Cr
//   g[n, c] = act2(sum_j h[n, j] * W2[j, c] + b2[c])
//   y[n, h, w, c] = x[n, h, w, c] * g[n, c]
//
// Two launches, no atomics, no ticket, every tensor below 2 GiB, C <= SE_MAX_C, 1 <= Cr <= SE_MAX_CR.  Every
// summation order below is a function of (H, W, C, Cr) alone, so image i has the same bits in a batch-1 and
// in a batch-n launch and at every place in the batch.
//
// Squeeze (se_squeeze_kernel), grid (P, n).  The H * W positions are cut into P ranges of se_range_pixels()
// positions (the last one ragged): SE_RANGE_BYTES of the image each, at most SE_MAX_RANGES of them, P = 1 for
// the small maps.  P depends on H * W and C only.  A workgroup sums its range for all C channels.  With
// C % 4 == 0 and 16-byte aligned tensors a lane loads 16 bytes (four channels, COLS = C / 4 columns), otherwise
// one float (COLS = C).  Lanes run over columns first: for COLS <= 256 thread t owns column t % COLS and the
// positions t / COLS, t / COLS + R, ... of the range (R = 256 / COLS rows), so one step of the workgroup reads
// R * COLS consecutive vectors; wider tensors take R = 1 and a thread owns columns t, t + 256, ...  A lane
// has SE_UNROLL positions in flight and adds them to one accumulator in position order.  The R row sums of a
// column go through LDS and row 0 adds them in row order and writes partial[n][p][c] (fp32).
//
// Excite and scale (se_excite_scale_kernel), grid (chunks, n).  Every workgroup first rebuilds its image's
// gate in LDS (the redundant gate is the design: no second pass over a gate tensor, no grid-wide dependency):
//   m[c]   thread c, c + 256, ...: the P partials added in index order, then ONE DIVISION by (float)(H * W)
//          (the form of avgpool_kernel and of Darknet's avgpool; not a multiplication by a reciprocal);
//   h[j]   FC1, one WAVE per output j (j = wave, wave + 4, ...): lane l adds m[c] * W1t[j][c] for c = l, l + 64,
//          ... in that order, the 64 lane sums are folded by the xor butterfly 32, 16, 8, 4, 2, 1, then + b1[j]
//          and act1.  W1 is held transposed, W1t[Cr][C], so a wave reads a row in 256-byte pieces;
//   g[c]   FC2, one THREAD per output c (c = t, t + 256, ...): the Cr products h[j] * W2[j][c] added in j
//          order, then + b2[c] and act2.  W2 is [Cr][C] as given, so the workgroup reads rows.
// Products and sums are separate fp32 operations (the file is built with -ffp-contract=off like the other
// element-wise kernels).  The weights are read from global memory: the block se_pack() lays out,
// [W1t | W2 | b1 | b2], a few hundred KB at most, resident in L2.  Then the workgroup multiplies its chunk
// of the image, a run of consecutive vectors, y = x * g[c]: 16-byte vectors (or floats), SE_UNROLL loads in
// flight, a stride loop over the chunk; a lane's column advances by 256 mod COLS per step, so there is no
// division in the loop.  The chunk is max(SE_CHUNK_BYTES, half the weight block) of the image, from the shape
// alone: at C = 1152, Cr = 48 (EfficientNet-B0's widest gate, 432 KB of weights) a 7 x 7 map is two chunks,
// so the gate's L2 reads stay comparable with the chunk's own traffic; at C = 96, Cr = 4 on a 112 x 112 map
// the gate is 3 KB of weights and 14 KB of partials against 64 KB read and 64 KB written.
//
// A lane reads every vector of a round before it writes one and no two lanes touch the same vector, and
// the squeeze has finished before the scale starts (stream order), so y == x is allowed.
#include <hip/hip_runtime.h>
#include <algorithm>
#include "dnn_common.h"
#include "plan_internal.h"
#include "../../include/dnn_hip_plan.h"

namespace dnnhip {

typedef float se_f32x4 __attribute__((ext_vector_type(4)));

constexpr int SE_THREADS = 256;
constexpr int SE_WAVE = 64;
constexpr int SE_WAVES = SE_THREADS / SE_WAVE;
constexpr int SE_UNROLL = 4;
constexpr int SE_RANGE_BYTES = 128 * 1024;  // a squeeze workgroup's share of an image
constexpr int SE_MAX_RANGES = 64;           // ... unless that makes more ranges than this
constexpr int SE_CHUNK_BYTES = 64 * 1024;   // an excite workgroup's share, at least

template <int VEC>
struct SeVec;
template <>
struct SeVec<4> {
  typedef se_f32x4 type;
};
template <>
struct SeVec<1> {
  typedef float type;
};

int se_range_pixels(int HW, int C) {
  const int by_bytes = std::max(1, SE_RANGE_BYTES / (4 * C));
  return std::max(by_bytes, (HW + SE_MAX_RANGES - 1) / SE_MAX_RANGES);
}

int se_ranges(int HW, int C) {
  const int ppr = se_range_pixels(HW, C);
  return (HW + ppr - 1) / ppr;
}

size_t se_weight_floats(int C, int Cr) { return 2 * (size_t)C * Cr + Cr + C; }

void se_pack(const float* w1, const float* b1, const float* w2, const float* b2, int C, int Cr, float* packed) {
  float* w1t = packed;
  float* w2p = packed + (size_t)C * Cr;
  float* b1p = w2p + (size_t)C * Cr;
  float* b2p = b1p + Cr;
  for (int c = 0; c < C; ++c)
    for (int j = 0; j < Cr; ++j) w1t[(size_t)j * C + c] = w1[(size_t)c * Cr + j];
  std::copy(w2, w2 + (size_t)C * Cr, w2p);
  for (int j = 0; j < Cr; ++j) b1p[j] = b1 ? b1[j] : 0.f;
  for (int c = 0; c < C; ++c) b2p[c] = b2 ? b2[c] : 0.f;
}

static bool se_act_ok(int act) {
  return act == ACT_NONE || act == ACT_LEAKY_F32 || act == ACT_LOGISTIC || act == ACT_SWISH || act == ACT_MISH;
}

int se_args_ok(const char* who, int C, int Cr, int act1, int act2) {
  DNN_REQUIRE(C >= 1 && C <= DNN_SE_MAX_C, "%s: %d channels, at most DNN_SE_MAX_C = %d (the gate lives in the workgroup's LDS)",
              who, C, DNN_SE_MAX_C);
  DNN_REQUIRE(Cr >= 1 && Cr <= DNN_SE_MAX_CR, "%s: squeezed width cr = %d outside 1..DNN_SE_MAX_CR = %d", who, Cr,
              DNN_SE_MAX_CR);
  DNN_REQUIRE(se_act_ok(act1) && se_act_ok(act2),
              "%s: activations %d, %d: each must be 0 (linear), 2 (leaky, fp32), 3 (logistic), 4 (swish) or 5 (mish)", who,
              act1, act2);
  return 0;
}

// partial[img][range][c] = the sum of x[img][p][c] over the range's positions.  COLS = C / VEC
template <int VEC>
__global__ void __launch_bounds__(SE_THREADS)
se_squeeze_kernel(const float* __restrict__ x, float* __restrict__ partial, int HW, int C, int ppr) {
  typedef typename SeVec<VEC>::type vec_t;
  __shared__ vec_t part[SE_THREADS];
  const int cols = C / VEC;
  const int P = gridDim.x, range = blockIdx.x, img = blockIdx.y, t = threadIdx.x;
  const int p0 = range * ppr, p1 = min(HW, p0 + ppr);
  const vec_t* src = reinterpret_cast<const vec_t*>(x + (size_t)img * HW * C);
  vec_t* dst = reinterpret_cast<vec_t*>(partial + ((size_t)img * P + range) * C);
  if (cols > SE_THREADS) {  // one row: a thread owns columns t, t + 256, ... and the whole range
    for (int c = t; c < cols; c += SE_THREADS) {
      vec_t acc = 0.0f;
      int p = p0;
      for (; p + SE_UNROLL <= p1; p += SE_UNROLL) {
        vec_t v[SE_UNROLL];
#pragma unroll
        for (int u = 0; u < SE_UNROLL; ++u) v[u] = src[(size_t)(p + u) * cols + c];
#pragma unroll
        for (int u = 0; u < SE_UNROLL; ++u) acc += v[u];
      }
      for (; p < p1; ++p) acc += src[(size_t)p * cols + c];
      dst[c] = acc;
    }
    return;
  }
  const int rows = SE_THREADS / cols;  // (>= 1)
  const int r = t / cols, c = t - r * cols;
  const bool active = r < rows;
  vec_t acc = 0.0f;
  if (active) {
    int p = p0 + r;
    for (; p + (SE_UNROLL - 1) * rows < p1; p += SE_UNROLL * rows) {
      vec_t v[SE_UNROLL];
#pragma unroll
      for (int u = 0; u < SE_UNROLL; ++u) v[u] = src[(size_t)(p + u * rows) * cols + c];
#pragma unroll
      for (int u = 0; u < SE_UNROLL; ++u) acc += v[u];
    }
    for (; p < p1; p += rows) acc += src[(size_t)p * cols + c];
    part[t] = acc;  // (t == r * cols + c)
  }
  __syncthreads();
  if (active && r == 0) {
    vec_t s = part[c];
    for (int k = 1; k < rows; ++k) s += part[k * cols + c];
    dst[c] = s;
  }
}

struct SeGate {
  const float* w1t;  // [Cr][C]
  const float* w2;   // [Cr][C]
  const float* b1;   // [Cr]
  const float* b2;   // [C]
  int Cr, act1, act2;
};

// The gate of image blockIdx.y into LDS, then y = x * g over vectors [q0, q1) of the image, q0 = blockIdx.x * chunk.
// Dynamic LDS: g[C] (16-byte aligned), m[C], h[Cr]
template <int VEC>
__global__ void __launch_bounds__(SE_THREADS)
se_excite_scale_kernel(const float* x, float* y, const float* __restrict__ partial, SeGate gate, int HW, int C, int P,
                       int chunk) {  // (no __restrict__ on x / y: in place is allowed)
  typedef typename SeVec<VEC>::type vec_t;
  extern __shared__ __attribute__((aligned(16))) float se_lds[];
  float* g = se_lds;
  float* m = se_lds + C;
  float* h = m + C;
  const int t = threadIdx.x, lane = t & (SE_WAVE - 1), wave = t / SE_WAVE, img = blockIdx.y;
  const int Cr = gate.Cr;
  const float* part = partial + (size_t)img * P * C;
  const float hw = (float)HW;
  for (int c = t; c < C; c += SE_THREADS) {
    float s = part[c];
    for (int p = 1; p < P; ++p) s += part[(size_t)p * C + c];
    m[c] = s / hw;
  }
  __syncthreads();
  for (int j = wave; j < Cr; j += SE_WAVES) {
    const float* row = gate.w1t + (size_t)j * C;
    float s = 0.0f;
    int c = lane;
    for (; c + (SE_UNROLL - 1) * SE_WAVE < C; c += SE_UNROLL * SE_WAVE) {
      float w[SE_UNROLL];
#pragma unroll
      for (int u = 0; u < SE_UNROLL; ++u) w[u] = row[c + u * SE_WAVE];
#pragma unroll
      for (int u = 0; u < SE_UNROLL; ++u) s += m[c + u * SE_WAVE] * w[u];
    }
    for (; c < C; c += SE_WAVE) s += m[c] * row[c];
#pragma unroll
    for (int d = SE_WAVE / 2; d >= 1; d >>= 1) s += __shfl_xor(s, d, SE_WAVE);
    if (lane == 0) h[j] = apply_act(s + gate.b1[j], gate.act1);
  }
  __syncthreads();
  for (int c = t; c < C; c += SE_THREADS) {
    float s = 0.0f;
    int j = 0;
    for (; j + SE_UNROLL <= Cr; j += SE_UNROLL) {
      float w[SE_UNROLL];
#pragma unroll
      for (int u = 0; u < SE_UNROLL; ++u) w[u] = gate.w2[(size_t)(j + u) * C + c];
#pragma unroll
      for (int u = 0; u < SE_UNROLL; ++u) s += h[j + u] * w[u];
    }
    for (; j < Cr; ++j) s += h[j] * gate.w2[(size_t)j * C + c];
    g[c] = apply_act(s + gate.b2[c], gate.act2);
  }
  __syncthreads();
  // the chunk: vectors [q0, q1) of the image's HW * cols, column of vector q = q mod cols
  const int cols = C / VEC;
  const int total = HW * cols;  // (< 2^29: the tensor is below 2 GiB)
  const int q0 = blockIdx.x * chunk, q1 = min(total, q0 + chunk);
  const vec_t* xs = reinterpret_cast<const vec_t*>(x + (size_t)img * HW * C);
  vec_t* ys = reinterpret_cast<vec_t*>(y + (size_t)img * HW * C);
  const vec_t* gv = reinterpret_cast<const vec_t*>(g);
  const int step = SE_THREADS % cols;
  int q = q0 + t;
  int col = q % cols;
  for (; q + (SE_UNROLL - 1) * SE_THREADS < q1; q += SE_UNROLL * SE_THREADS) {
    vec_t v[SE_UNROLL];
    int cu[SE_UNROLL];
#pragma unroll
    for (int u = 0; u < SE_UNROLL; ++u) {
      v[u] = xs[q + u * SE_THREADS];
      cu[u] = col;
      col += step;
      col = col >= cols ? col - cols : col;
    }
#pragma unroll
    for (int u = 0; u < SE_UNROLL; ++u) ys[q + u * SE_THREADS] = v[u] * gv[cu[u]];
  }
  for (; q < q1; q += SE_THREADS) {
    ys[q] = xs[q] * gv[col];
    col += step;
    col = col >= cols ? col - cols : col;
  }
}

size_t se_partial_floats(int H, int W, int C) { return (size_t)se_ranges(H * W, C) * C; }

int launch_squeeze_excite(const float* x, float* y, float* partial, const float* packed, int n, int H, int W, int C,
                          int Cr, int act1, int act2, int phases, hipStream_t stream) {
  DNN_REQUIRE(x && y && partial && packed, "launch_squeeze_excite: NULL tensor");
  DNN_REQUIRE(n >= 0 && H > 0 && W > 0, "launch_squeeze_excite: bad shape n=%d %dx%dx%d", n, H, W, C);
  if (int rc = se_args_ok("launch_squeeze_excite", C, Cr, act1, act2)) return rc;
  DNN_REQUIRE((unsigned long long)std::max(n, 1) * H * W * C * 4 < 0x80000000ULL,
              "launch_squeeze_excite: a tensor of n=%d %dx%dx%d is >= 2 GiB; split the batch", n, H, W, C);
  DNN_REQUIRE(n <= 65535, "launch_squeeze_excite: n=%d images, at most 65535 per launch", n);
  if (n == 0) return 0;
  const int HW = H * W;
  // one decision for both phases: the same pointers give the same kernels
  const bool vec4 = C % 4 == 0 && ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y) |
                                    reinterpret_cast<uintptr_t>(partial)) & 15) == 0;
  const int ppr = se_range_pixels(HW, C), P = se_ranges(HW, C);
  if (phases & SE_SQUEEZE) {
    if (vec4)
      hipLaunchKernelGGL(se_squeeze_kernel<4>, dim3(P, n), dim3(SE_THREADS), 0, stream, x, partial, HW, C, ppr);
    else
      hipLaunchKernelGGL(se_squeeze_kernel<1>, dim3(P, n), dim3(SE_THREADS), 0, stream, x, partial, HW, C, ppr);
  }
  if (phases & SE_EXCITE) {
    // the chunk in vectors: max(SE_CHUNK_BYTES, half the weight block) of the image, a whole number of rounds
    const size_t chunk_bytes = std::max<size_t>(SE_CHUNK_BYTES, se_weight_floats(C, Cr) * 4 / 2);
    const long long round = (long long)SE_UNROLL * SE_THREADS;
    const long long total = (long long)HW * (vec4 ? C / 4 : C);
    const long long want = (long long)(chunk_bytes / (vec4 ? 16 : 4) + round - 1) / round * round;
    const long long chunk = std::min(want, (total + round - 1) / round * round);
    const unsigned chunks = (unsigned)((total + chunk - 1) / chunk);
    const size_t lds = (2 * (size_t)C + Cr) * sizeof(float);  // (at most 36 KB)
    const float* w2 = packed + (size_t)C * Cr;
    const SeGate gate{packed, w2, w2 + (size_t)C * Cr, w2 + (size_t)C * Cr + Cr, Cr, act1, act2};
    if (vec4)
      hipLaunchKernelGGL(se_excite_scale_kernel<4>, dim3(chunks, n), dim3(SE_THREADS), lds, stream, x, y, partial, gate,
                         HW, C, P, (int)chunk);
    else
      hipLaunchKernelGGL(se_excite_scale_kernel<1>, dim3(chunks, n), dim3(SE_THREADS), lds, stream, x, y, partial, gate,
                         HW, C, P, (int)chunk);
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("launch squeeze_excite: %s", hipGetErrorString(e));
    return -1;
  }
  return 0;
}

}  // namespace dnnhip

