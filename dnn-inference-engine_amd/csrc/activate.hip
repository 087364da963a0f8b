// Element-wise activation, out[i] = apply_act(in[i], act) (act_dev.h: logistic, swish, mish), for the
// places where a plan cannot make the activation a conv's or a shortcut's epilogue: behind a stash or a
// tap, behind a pool, behind a join.  Plain NHWC fp32 on both sides, each tensor below 2 GiB.
//
// Memory-bound with a heavy per-value tail (expf is ~20 VALU, the IEEE division ~10): a lane moves 16 B
// per access and keeps ACT_UNROLL loads in flight before it starts on the arithmetic, so the exponentials
// of one round overlap the loads of the next wave's; the grid is sized to the resident workgroups and
// strides.  The activation is a template argument: each kernel holds one form, no branch per value.  A
// scalar loop covers the last count % 4 elements, and everything when a pointer is not 16-byte aligned.
// A lane reads every vector of a round before it writes one and no two lanes touch the same vector, so
// out == in is allowed.
#include <hip/hip_runtime.h>
#include <algorithm>
#include "dnn_common.h"

namespace dnnhip {

typedef float act_f32x4 __attribute__((ext_vector_type(4)));

constexpr int ACT_THREADS = 256;
constexpr int ACT_UNROLL = 4;

template <int ACT>
__device__ __forceinline__ act_f32x4 activate_vec(act_f32x4 x) {
  act_f32x4 r;
  r.x = apply_act(x.x, ACT);
  r.y = apply_act(x.y, ACT);
  r.z = apply_act(x.z, ACT);
  r.w = apply_act(x.w, ACT);
  return r;
}

// n4 whole 16-byte vectors, then elements [4 * n4, n) one by one
template <int ACT>
__global__ void __launch_bounds__(ACT_THREADS)
activate_kernel(const float* in, float* out, int n4, int n) {  // (no __restrict__: in place is allowed)
  const act_f32x4* i4 = reinterpret_cast<const act_f32x4*>(in);
  act_f32x4* o4 = reinterpret_cast<act_f32x4*>(out);
  const int stride = gridDim.x * ACT_THREADS;  // (n4 < 2^27 and stride <= 2^19: no int overflow below)
  int i = blockIdx.x * ACT_THREADS + threadIdx.x;
  for (; i + (ACT_UNROLL - 1) * stride < n4; i += ACT_UNROLL * stride) {
    act_f32x4 x[ACT_UNROLL];
#pragma unroll
    for (int u = 0; u < ACT_UNROLL; ++u) x[u] = i4[i + u * stride];
#pragma unroll
    for (int u = 0; u < ACT_UNROLL; ++u) o4[i + u * stride] = activate_vec<ACT>(x[u]);
  }
  for (; i < n4; i += stride) o4[i] = activate_vec<ACT>(i4[i]);
  for (int j = 4 * n4 + blockIdx.x * ACT_THREADS + threadIdx.x; j < n; j += stride) out[j] = apply_act(in[j], ACT);
}

int launch_activate(const float* in, float* out, long long count, int act, hipStream_t stream) {
  DNN_REQUIRE(in && out, "launch_activate: NULL tensor");
  DNN_REQUIRE(act >= ACT_LOGISTIC && act <= ACT_MISH, "launch_activate: activation code %d outside %d..%d", act,
              (int)ACT_LOGISTIC, (int)ACT_MISH);
  DNN_REQUIRE(count >= 0 && (unsigned long long)count * 4 < 0x80000000ULL,
              "launch_activate: a tensor of %lld floats is >= 2 GiB; split the batch", count);
  if (count == 0) return 0;
  const int n = (int)count;
  const bool vec4 = ((reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(out)) & 15) == 0;
  const int n4 = vec4 ? n / 4 : 0;
  // one lane per vector up to the resident grid (8 workgroups per CU); the rest grid-strides
  const long long lanes = std::max<long long>(n4, n - 4LL * n4);
  const long long blocks = (lanes + ACT_THREADS - 1) / ACT_THREADS;
  const dim3 grid((unsigned)std::max<long long>(1, std::min<long long>(blocks, (long long)device_cu_count() * 8)));
  if (act == ACT_LOGISTIC)
    hipLaunchKernelGGL(activate_kernel<ACT_LOGISTIC>, grid, dim3(ACT_THREADS), 0, stream, in, out, n4, n);
  else if (act == ACT_SWISH)
    hipLaunchKernelGGL(activate_kernel<ACT_SWISH>, grid, dim3(ACT_THREADS), 0, stream, in, out, n4, n);
  else
    hipLaunchKernelGGL(activate_kernel<ACT_MISH>, grid, dim3(ACT_THREADS), 0, stream, in, out, n4, n);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("launch activate: %s", hipGetErrorString(e));
    return -1;
  }
  return 0;
}

}  // namespace dnnhip
