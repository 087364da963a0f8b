// Arithmetic of the YOLO postprocessing kernels (postprocess.hip, postprocess_head.hip,
// postprocess_multi.hip):
// the reference's fp32 decode and integer IoU (cs492-projects/proj3/yolov2tiny.py:113-140,
// :179-195, :229-234) as numpy 2.x evaluates them, shared so both kernels round alike.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace dnnhip {

// numpy 2.x float32 exp (the AVX512F / AVX2 loop numpy dispatches to on x86, its
// loops_exponent_log "simd_exp_f32" algorithm restated): Cody-Waite reduction by
// rint(x * log2 e) (magic-number rounding), a 5th/2nd-order rational minimax, scale by 2^k.
// Matches np.exp bit for bit on all 2^32 float32 inputs (checked on x86 against numpy 2.2).
__device__ __forceinline__ float np_expf(float x) {
  if (x != x) return x;
  if (x >= 88.72283935546875f) return __builtin_inff();
  if (x <= -103.97208404541015625f) return 0.0f;
  const float magic = 12582912.0f;  // 0x1.8p+23
  float q = x * 1.442695040888963407359924681001892137f;
  q = (q + magic) - magic;
  float r = __builtin_fmaf(q, -6.93145752e-1f, x);
  r = __builtin_fmaf(q, -1.42860677e-6f, r);
  r = __builtin_fmaf(q, 0.0f, r);
  float num = __builtin_fmaf(5.082762527590693718096e-04f, r, 6.757896990527504603057e-03f);
  num = __builtin_fmaf(num, r, 5.114512081637298353406e-02f);
  num = __builtin_fmaf(num, r, 2.473615434895520810817e-01f);
  num = __builtin_fmaf(num, r, 7.257664613233124478488e-01f);
  num = __builtin_fmaf(num, r, 9.999999999980870924916e-01f);
  float den = __builtin_fmaf(2.159509375685829852307e-02f, r, -2.742335390411667452936e-01f);
  den = __builtin_fmaf(den, r, 1.0f);
  return ldexpf(num / den, (int)q);
}

// 1 / (1 + float32(e) ** -x)  (yolov2tiny.py:229-230 with numpy 2 fp32 scalar semantics: the
// power is libm powf).  e32 ** y is evaluated as exp2(y * log2(e32)) in double and rounded
// once: equal to glibc 2.35 powf(e32, y) on all but 0.004 % of float32 y (1 ulp apart there).
__device__ __forceinline__ float sigmoid_ref(float x) {
  const double log2_e32 = 0x1.715475968cddcp+0;  // log2((double)float32(np.e)) = 1.4426949970774023
  const float pw = (float)exp2((double)(-x) * log2_e32);
  return 1.0f / (1.0f + pw);
}

// the float32 add.reduce of numpy over e[c] = exp(q[c] - m), c < C <= 128 (unblocked pairwise
// sum): sequential below 8 elements, else 8 accumulators over whole groups of 8, combined
// pairwise, then the tail in order
__device__ __forceinline__ float softmax_sum(const float* __restrict__ q, int C, float m) {
  if (C < 8) {
    float s = np_expf(q[0] - m);  // 0 + e[0] = e[0] exactly
    for (int c = 1; c < C; ++c) s = s + np_expf(q[c] - m);
    return s;
  }
  float r[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) r[j] = np_expf(q[j] - m);
  const int full = C - (C % 8);
  int i = 8;
  for (; i < full; i += 8) {
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = r[j] + np_expf(q[i + j] - m);
  }
  float s = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
  for (; i < C; ++i) s = s + np_expf(q[i] - m);
  return s;
}

// int(float32) with the reference's failure cases flagged: truncation toward zero
__device__ __forceinline__ bool trunc_i64(float v, long long* out) {
  const float lim = 2305843009213693952.0f;  // 2^61: keeps every +1 width / difference in int64
  if (!(v > -lim && v < lim)) return false;   // also NaN
  *out = (long long)v;                        // fp -> int conversion truncates
  return true;
}

__device__ __forceinline__ double u64_to_f64(unsigned long long x) {
  // both terms exact, one rounding of the exact sum = correctly rounded
  return (double)(unsigned)(x >> 32) * 4294967296.0 + (double)(unsigned)x;
}

// correctly rounded (nearest-even) |v| -> double for |v| < 2^127, as Python's int -> float
__device__ __forceinline__ double i128_to_f64(__int128 v) {
  const bool neg = v < 0;
  const unsigned __int128 u = neg ? (unsigned __int128)(-v) : (unsigned __int128)v;
  const unsigned long long hi = (unsigned long long)(u >> 64), lo = (unsigned long long)u;
  double d;
  if (hi == 0) {
    d = u64_to_f64(lo);
  } else {
    const int s = 64 - __clzll((long long)hi);  // 1..63
    unsigned long long top = (unsigned long long)(u >> s);
    top |= (lo & ((1ull << s) - 1)) != 0 ? 1ull : 0ull;  // sticky bit: round-to-odd below
    d = ldexp(u64_to_f64(top), s);
  }
  return neg ? -d : d;
}

// yolov2tiny.py:179-195: iou(a, b) > thr on integer corners [l, t, r, b].  A zero
// denominator (possible: overlaps are not clamped) raises ZeroDivisionError in the reference;
// it sets *zero_den here.
__device__ __forceinline__ bool iou_gt(const long long* a, const long long* b, double thr, bool* zero_den) {
  const long long xa = a[0] > b[0] ? a[0] : b[0], ya = a[1] > b[1] ? a[1] : b[1];
  const long long xb = a[2] < b[2] ? a[2] : b[2], yb = a[3] < b[3] ? a[3] : b[3];
  // fast path: every width below 2^25 -> every product and sum below 2^53, exact in int64 and
  // in double, so the double division is the reference's int / float(int) exactly
  const long long w0 = xb - xa + 1, h0 = yb - ya + 1, wa = a[2] - a[0] + 1, ha = a[3] - a[1] + 1,
                  wb = b[2] - b[0] + 1, hb = b[3] - b[1] + 1;
  const long long lim = 1ll << 25;
  if (w0 > -lim && w0 < lim && h0 > -lim && h0 < lim && wa > -lim && wa < lim && ha > -lim && ha < lim &&
      wb > -lim && wb < lim && hb > -lim && hb < lim) {
    const long long inter = w0 * h0, den = wa * ha + wb * hb - inter;
    if (den == 0) {
      *zero_den = true;
      return false;
    }
    return (double)inter / (double)den > thr;
  }
  const __int128 inter = (__int128)(xb - xa + 1) * (__int128)(yb - ya + 1);
  const __int128 area_a = (__int128)(a[2] - a[0] + 1) * (__int128)(a[3] - a[1] + 1);
  const __int128 area_b = (__int128)(b[2] - b[0] + 1) * (__int128)(b[3] - b[1] + 1);
  const __int128 den = area_a + area_b - inter;
  if (den == 0) {
    *zero_den = true;
    return false;
  }
  return i128_to_f64(inter) / i128_to_f64(den) > thr;
}

}  // namespace dnnhip
