// The activation family of the fp32 path, one device function: apply_act(v, act).
//
//   0  none
//   1  leaky, the reference's double-rounded form  v < 0 ? (float)(0.1 * (double)v) : v
//   2  leaky in fp32                               max(v, 0.1f * v)
//   3  logistic  1 / (1 + e^-v)
//   4  swish     v * logistic(v)
//   5  mish      v * tanh(ln(1 + e^v))
//
// Codes 3..5 are DNN_ACT_LOGISTIC / _SWISH / _MISH of include/dnn_hip_plan.h.  Each costs one expf and
// one IEEE division per value; nothing is evaluated in double.  The target is the mathematical function
// (DESIGN.md has the measured error), not Darknet's bits.
//
// logistic.  With e = expf(-|v|) in (0, 1]: 1 / (1 + e) for v >= 0 and e / (1 + e) below.  The textbook
// 1 / (1 + expf(-v)) is the same value for v >= 0; for v < -88.7 its expf overflows and the quotient
// becomes 0 while the function (and v times it, swish) is still a normal fp32 number down to v = -87.3
// (-91.9 for swish).  The form here never overflows and has no cancellation.
//
// mish.  tanh(ln(1 + e^v)) = ((1 + e^v)^2 - 1) / ((1 + e^v)^2 + 1) = n / (n + 2) with e = expf(v) and
// n = e * (e + 2): no tanhf, no logf, and no cancellation for negative v (n is a product of positives).
// Two cut-offs:
//   v >= ACT_MISH_IDENT (9.02): mish(v) = v.  The factor is 1 - 2 / (n + 2).  From v = 13 ln 2 = 9.0109 on,
//     e >= 2^13 and n + 2 >= 2^26, so 2 / (n + 2) <= 2^-25, half an ulp of the fp32 numbers below 1: the
//     factor has rounded to 1 already, and v * 1 is v.  (Far above, from v = 44.4 on, n itself would overflow:
//     the cut-off is what keeps inf / inf away.)  9.02 is 13 ln 2 rounded up to two decimals.
//   v >= ACT_MISH_SPLIT (-0.6, Darknet's own switch point): v - 2 * (v / (n + 2)) instead of
//     (v / (n + 2)) * n.  Both are the same rational function; below -0.6 the product form has no subtraction
//     at all, above it the subtracted term is under 0.59 |v| (0.4 |v| from v = 0 on), so the difference
//     loses at most about one bit, and for large v the term vanishes instead of n / (n + 2) nearing inf / inf.
// One division serves both forms: q = v / (n + 2).  For v below about -87 e is denormal or 0 and the result
// is a denormal or -0: the function's value there is below FLT_MIN in magnitude.
#pragma once
#include <hip/hip_runtime.h>

namespace dnnhip {

enum ActCode : int { ACT_NONE = 0, ACT_LEAKY_F64 = 1, ACT_LEAKY_F32 = 2, ACT_LOGISTIC = 3, ACT_SWISH = 4, ACT_MISH = 5,
                     ACT_NUM = 6 };

constexpr float ACT_MISH_SPLIT = -0.6f;
constexpr float ACT_MISH_IDENT = 9.02f;

// mish and swish have a minimum (near -1.19 and -1.28): max over a pool window does not commute with them
__host__ __device__ constexpr bool act_is_monotone(int act) { return act != ACT_SWISH && act != ACT_MISH; }

__device__ __forceinline__ float act_logistic(float v) {
  const float e = expf(-__builtin_fabsf(v));
  return (v >= 0.f ? 1.f : e) / (1.f + e);
}

__device__ __forceinline__ float act_mish(float v) {
  const float e = expf(v < ACT_MISH_IDENT ? v : 0.f);  // (no overflow for the values that return v)
  const float n = e * (e + 2.f);
  const float q = v / (n + 2.f);
  const float r = v < ACT_MISH_SPLIT ? q * n : v - 2.f * q;
  return v < ACT_MISH_IDENT ? r : v;
}

__device__ __forceinline__ float apply_act(float v, int act) {
  switch (act) {
    case ACT_LEAKY_F64: return v < 0.f ? (float)(0.1 * (double)v) : v;
    case ACT_LEAKY_F32: {
      const float t = v * 0.1f;
      return v > t ? v : t;
    }
    case ACT_LOGISTIC: return act_logistic(v);
    case ACT_SWISH: return v * act_logistic(v);
    case ACT_MISH: return act_mish(v);
    default: return v;
  }
}

}  // namespace dnnhip
