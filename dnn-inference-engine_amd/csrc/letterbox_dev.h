// What the letterbox kernels share (letterbox.hip: packed 8-bit BGR / RGB; letterbox_nv12.hip: NV12
// surfaces): the size rule, the by-value frame record, and the sampling and interpolation of one
// output pixel.  The arithmetic is stated at the top of letterbox.hip; a kernel supplies only how
// the six source bytes of a row's two taps are fetched, so every pixel format rounds alike.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

namespace dnnhip {

// ------------------------------------------------------------------------------ geometry (host)
struct LbGeom {
  int new_h, new_w, pad_y, pad_x;
};

// false: a side of the letterboxed image is below 2 (Darknet divides by new - 1) or, beyond the
// sizes fp32 quotients can order, above the network's
inline bool letterbox_geom(int src_h, int src_w, int net_h, int net_w, LbGeom* g) {
  long long nw, nh;
  if (((float)net_w / (float)src_w) < ((float)net_h / (float)src_h)) {
    nw = net_w;
    nh = ((long long)src_h * net_w) / src_w;
  } else {
    nh = net_h;
    nw = ((long long)src_w * net_h) / src_h;
  }
  if (nw < 2 || nh < 2 || nw > net_w || nh > net_h) return false;
  g->new_h = (int)nh;
  g->new_w = (int)nw;
  g->pad_x = (net_w - (int)nw) / 2;
  g->pad_y = (net_h - (int)nh) / 2;
  return true;
}

// What a kernel needs of one frame; the host fills it and a chunk of them travels by value as
// the kernel's argument (no device-side descriptor table, no copy to wait for).
struct LbFrame {
  unsigned long long offset;  // of the frame's first byte in the pixel buffer
  int H, W;                   // source
  int h, w;                   // letterboxed image
  int pad_y, pad_x;
  float h_scale, w_scale;
};
constexpr int LB_CHUNK = 64;  // frames per launch

// the record of a src_h x src_w frame at `offset` (a size letterbox_geom accepts)
inline LbFrame lb_frame(unsigned long long offset, int src_h, int src_w, int net_h, int net_w) {
  LbGeom g;
  letterbox_geom(src_h, src_w, net_h, net_w, &g);
  LbFrame f;
  f.offset = offset;
  f.H = src_h;
  f.W = src_w;
  f.h = g.new_h;
  f.w = g.new_w;
  f.pad_y = g.pad_y;
  f.pad_x = g.pad_x;
  f.h_scale = (float)(src_h - 1) / (float)(g.new_h - 1);
  f.w_scale = (float)(src_w - 1) / (float)(g.new_w - 1);
  return f;
}

// pixel (oy, ox) of the network input, its three channels in output order (also host code, so a
// CPU build can run the same arithmetic).  How the source bytes are fetched is the caller's: `fetch`
// is told the frame (frame), then the two source rows (rows), and returns the three bytes of pixels
// ix and ix1 of the first row as bytes 0..2 and 3..5 (first) and, where there is a second term,
// those of the second row (second).  The calls stand where letterbox_kernel's own address
// arithmetic stood, so that kernel compiles to the instructions it had before the split.
template <class Fetch>
__host__ __device__ __forceinline__ void lb_sample(Fetch& fetch, const LbFrame& f, const float* lut, int oy, int ox,
                                                   int flip, float* out) {
  const int r = oy - f.pad_y, c = ox - f.pad_x;
  if ((unsigned)r >= (unsigned)f.h || (unsigned)c >= (unsigned)f.w) {
    out[0] = out[1] = out[2] = 0.5f;
    return;
  }
  fetch.frame(f);
  const float sy = (float)r * f.h_scale;
  int iy = (int)sy;
  const float dy = sy - (float)iy;
  iy = iy < f.H - 1 ? iy : f.H - 1;                      // (addresses only: never taken for a
  const int iy1 = iy + 1 < f.H ? iy + 1 : f.H - 1;       //  size fp32 indexes exactly)
  const bool two = !(r == f.h - 1 || f.H == 1);
  const bool edge = c == f.w - 1 || f.W == 1;            // part(r, c) = S(r, W-1), no interpolation
  int ix = f.W - 1, ix1 = f.W - 1;
  float dx = 0.f;
  if (!edge) {
    const float sx = (float)c * f.w_scale;
    ix = (int)sx;
    dx = sx - (float)ix;
    ix = ix < f.W - 1 ? ix : f.W - 1;
    ix1 = ix + 1 < f.W ? ix + 1 : f.W - 1;
  }
  const float omdx = 1.f - dx;
  fetch.rows(iy, iy1);
  const unsigned long long q0 = fetch.first(ix, ix1);
  const unsigned long long q1 = two ? fetch.second(ix, ix1) : 0ull;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int sh = 8 * (flip ? 2 - k : k);
    const float s00 = lut[(q0 >> sh) & 0xff], s01 = lut[(q0 >> (sh + 24)) & 0xff];
    const float a = edge ? s00 : omdx * s00 + dx * s01;
    float v = (1.f - dy) * a;
    if (two) {
      const float s10 = lut[(q1 >> sh) & 0xff], s11 = lut[(q1 >> (sh + 24)) & 0xff];
      const float b = edge ? s10 : omdx * s10 + dx * s11;
      v += dy * b;
    }
    out[k] = v;
  }
}

// The source indices [*lo, *hi] that the letterboxed indices a..b of one axis sample (0 <= a <= b <
// n; S source pixels, scale = (S - 1) / (n - 1)): lb_sample's own fp32 positions, which grow with
// the index, and its last-column rule.  Host and device evaluate the same expressions.
__host__ __device__ __forceinline__ void lb_span(int a, int b, int n, int S, float scale, int* lo, int* hi) {
  int i0 = (int)((float)a * scale), i1 = (int)((float)b * scale);
  i0 = i0 < S - 1 ? i0 : S - 1;
  i1 = i1 + 1 < S ? i1 + 1 : S - 1;
  *lo = i0;
  *hi = b == n - 1 ? S - 1 : i1;
}

}  // namespace dnnhip
