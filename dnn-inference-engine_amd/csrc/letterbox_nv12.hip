// NV12 letterbox ingest (include/dnn_hip_ingest.h: dnn_letterbox_frames_nv12): decoder surfaces to
// the network's fp32 input in one kernel.  The result is what letterbox.hip's kernel writes for the
// 8-bit RGB image that the header's integer conversion makes of the surface; the geometry, the
// / 255 table and the two-pass bilinear are that file's, taken from letterbox_dev.h (lb_sample), and
// this file is built with -ffp-contract=off like it.
//
// A packed frame gives a pixel's three bytes in one place, so letterbox.hip gathers per output.  An
// NV12 pixel sits in two planes and has to be converted, and when a frame is enlarged or kept near
// its size every source pixel is a tap of four or more outputs.  So the kernel has two forms, one
// chosen per frame on the host and carried in the frame record (uniform over a workgroup):
//
//   staged  a workgroup owns NV_TR x NV_TC pixels of the network input.  It finds the source
//           rectangle those pixels sample (lb_span: lb_sample's own fp32 positions), loads the
//           rectangle's Y rows and UV rows four pixels a thread (one 4-byte load each where the
//           address is 4-byte aligned and the four bytes are used bytes of the row, byte loads
//           otherwise: nothing promises alignment), converts every source pixel ONCE and keeps
//           it as 0x00BBGGRR in LDS.  Then each thread interpolates its 16-byte pieces of the
//           output rows out of LDS.
//   gather  per output pixel: the 2 x 2 taps' Y bytes and, per row, the one or two UV pairs they map
//           to from memory, converted in registers.  For frames whose rectangle does not fit the LDS
//           buffer, which are the strong reductions: there a source pixel is a tap of at most one
//           output and staging would load pixels nobody reads.
//
// The rule is the footprint alone: staged where every tile's rectangle fits NV_LDS_PIXELS (with
// 16 x 64 tiles and 8192 pixels that is a reduction of up to about 2.6 on both axes), else gather.
// Both forms convert with the same integers and interpolate with the same fp32 expressions, so
// their bits are equal.  A tile that lies wholly in the pad only stores 0.5.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "dnn_common.h"
#include "letterbox_dev.h"
#include "../../include/dnn_hip_ingest.h"

namespace dnnhip {

struct NvFrame {
  LbFrame g;                      // g.offset: the Y plane's
  unsigned long long uv_offset;
  int pitch;
  int staged;                     // the form, chosen on the host
};
struct NvChunk {
  NvFrame f[LB_CHUNK];            // 64 x 56 B of kernel argument
};
// the header's table: C = cy * (Y - y0), R = C + rv E, G = C - gu D - gv E, B = C + bu D
struct NvMatrix {
  int y0, cy, rv, gu, gv, bu;
};
static const NvMatrix NV_MATRICES[3] = {{16, 298, 409, 100, 208, 516}, {16, 298, 459, 55, 136, 541},
                                        {0, 256, 359, 88, 183, 454}};

constexpr int NV_THREADS = 256;
constexpr int NV_TR = 16, NV_TC = 64;   // a tile of the network input: rows x pixels
constexpr int NV_LDS_PIXELS = 8192;     // converted source pixels a workgroup can hold (32 KiB)
static_assert(NV_THREADS == 256, "the / 255 table is filled one value a thread");
static_assert(NV_TC % 4 == 0, "a tile row starts and ends on a 16-byte piece of the output row");
static_assert(NV_LDS_PIXELS % 4 == 0, "a stage item stores four pixels, 16 bytes");
static_assert(NV_LDS_PIXELS * 4 + 256 * 4 <= 64 * 1024, "static LDS of one workgroup");
// a tile of a frame that is not reduced samples at most NV_TR + 1 rows of NV_TC + 1 pixels, widened
// to an even start and a multiple of four: enlarged and same-size frames always stage
static_assert((NV_TR + 1) * ((NV_TC + 1 + 1 + 3) / 4 * 4) <= NV_LDS_PIXELS, "an unreduced tile fits");

// The source range of tile t (T indices) of one axis: false where the tile misses the image.
__host__ __device__ __forceinline__ bool nv_axis(int t, int T, int pad, int n, int S, float scale, int* lo, int* hi) {
  long long a = (long long)t * T - pad, b = a + T - 1;
  a = a > 0 ? a : 0;
  b = b < n - 1 ? b : n - 1;
  if (a > b) return false;
  lb_span((int)a, (int)b, n, S, scale, lo, hi);
  return true;
}
// the columns kept in LDS for source columns x0..x1: from an even column (a chroma pair's first)
// in groups of four
__host__ __device__ __forceinline__ int nv_stride(int* x0, int x1) {
  *x0 &= ~1;
  return (x1 - *x0 + 4) & ~3;
}

// one pixel by the header's table, as 0x00BBGGRR (lb_sample's byte order with flip = 0).  The clip
// comes before the shift, to 0 .. 0xffff, which gives the table's clip((t) >> 8) for every t.
// Observed: written the table's way, the compiler fuses two channels' shift and clip into one
// v_ashr_pk_u8_i32, and with that build the gather form's second row differed from the table on the
// MI355X, in bytes next to a negative channel; this form emits none and is exact.  Supposed, not
// isolated: that instruction's upper half, or what the compiler assumes of it.  Only
// tests/test_gpu_nv12.py (the forced gather cases) would notice a compiler fusing it again.
__host__ __device__ __forceinline__ unsigned nv_clip8(int t) {
  t = t < 0 ? 0 : (t > 0xffff ? 0xffff : t);
  return (unsigned)t >> 8;
}
__host__ __device__ __forceinline__ unsigned nv_rgb(const NvMatrix& m, int Y, int U, int V) {
  const int C = m.cy * (Y - m.y0) + 128, D = U - 128, E = V - 128;
  return nv_clip8(C + m.rv * E) | nv_clip8(C - m.gu * D - m.gv * E) << 8 | nv_clip8(C + m.bu * D) << 16;
}

// bytes p[0..3] as one word, reading only the first `valid` of them (the rest 0)
__device__ __forceinline__ unsigned nv_load4(const uint8_t* __restrict__ p, int valid) {
  if (valid >= 4 && (reinterpret_cast<uintptr_t>(p) & 3) == 0) return *reinterpret_cast<const unsigned*>(p);
  unsigned v = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (k < valid) v |= (unsigned)p[k] << (8 * k);
  return v;
}

// staged form, load and convert: source rows y0 .. y0 + rows - 1, columns x0 .. x0 + stride - 1 (x0
// even, stride % 4 == 0, rows * stride <= NV_LDS_PIXELS) into rgb[row * stride + column].  An item
// is four pixels of one row: their Y bytes and their two UV pairs lie at the same byte offset x of
// the Y row and of the UV row.  Columns at or past W are stored as they come and never sampled.
__device__ __forceinline__ void nv_stage(const uint8_t* __restrict__ pixels, const NvFrame& f, const NvMatrix& m,
                                         unsigned* rgb, int y0, int rows, int x0, int stride) {
  const int groups = stride >> 2, items = rows * groups;
  const int uv_used = 2 * ((f.g.W + 1) / 2);
  for (int i = threadIdx.x; i < items; i += NV_THREADS) {
    const int row = i / groups, x = x0 + 4 * (i - row * groups), iy = y0 + row;
    const unsigned yy = nv_load4(pixels + f.g.offset + (size_t)iy * f.pitch + x, f.g.W - x);
    const unsigned uv = nv_load4(pixels + f.uv_offset + (size_t)(iy >> 1) * f.pitch + x, uv_used - x);
    const int u0 = uv & 0xff, v0 = (uv >> 8) & 0xff, u1 = (uv >> 16) & 0xff, v1 = uv >> 24;
    uint4 px;
    px.x = nv_rgb(m, yy & 0xff, u0, v0);
    px.y = nv_rgb(m, (yy >> 8) & 0xff, u0, v0);
    px.z = nv_rgb(m, (yy >> 16) & 0xff, u1, v1);
    px.w = nv_rgb(m, yy >> 24, u1, v1);
    *reinterpret_cast<uint4*>(rgb + i * 4) = px;  // i * 4 + 3 < rows * stride
  }
}

// lb_sample's fetches.  Staged: two LDS words a row (iy, ix, ix1 lie in the staged rectangle: lb_span).
struct NvStagedFetch {
  const unsigned* rgb;
  int y0, x0, stride;
  int r0 = 0, r1 = 0;  // first word of the two rows
  __device__ __forceinline__ void frame(const LbFrame&) {}
  __device__ __forceinline__ void rows(int iy, int iy1) {
    r0 = (iy - y0) * stride;
    r1 = (iy1 - y0) * stride;
  }
  __device__ __forceinline__ unsigned long long pair(int r, int ix, int ix1) const {
    return (unsigned long long)rgb[r + (ix - x0)] | (unsigned long long)rgb[r + (ix1 - x0)] << 24;
  }
  __device__ __forceinline__ unsigned long long first(int ix, int ix1) const { return pair(r0, ix, ix1); }
  __device__ __forceinline__ unsigned long long second(int ix, int ix1) const { return pair(r1, ix, ix1); }
};
// Gather: a row's two Y bytes and the one or two UV pairs they map to, converted in registers (a
// second row of the same chroma row finds its pairs in cache).
struct NvGatherFetch {
  const uint8_t* __restrict__ y;
  const uint8_t* __restrict__ uv;
  int pitch;
  const NvMatrix& m;
  int iy0 = 0, iy1 = 0;
  __device__ __forceinline__ void frame(const LbFrame&) {}
  __device__ __forceinline__ void rows(int a, int b) {
    iy0 = a;
    iy1 = b;
  }
  __device__ __forceinline__ unsigned long long pair(int iy, int ix, int ix1) const {
    const uint8_t* yr = y + (size_t)iy * pitch;
    const uint8_t* ur = uv + (size_t)(iy >> 1) * pitch;
    const int c0 = ix & ~1, c1 = ix1 & ~1;
    const int u0 = ur[c0], v0 = ur[c0 + 1];
    int u1 = u0, v1 = v0;
    if (c1 != c0) {
      u1 = ur[c1];
      v1 = ur[c1 + 1];
    }
    return (unsigned long long)nv_rgb(m, yr[ix], u0, v0) | (unsigned long long)nv_rgb(m, yr[ix1], u1, v1) << 24;
  }
  __device__ __forceinline__ unsigned long long first(int ix, int ix1) const { return pair(iy0, ix, ix1); }
  __device__ __forceinline__ unsigned long long second(int ix, int ix1) const { return pair(iy1, ix, ix1); }
};

// Grid: x = tiles of one frame's output (tiles_x per tile row), y = frames of the chunk.  VEC: a
// piece is 16 bytes of the flattened [net_h][3 * net_w] frame (net_w % 4 == 0; a tile's row is 48
// pieces, 768 contiguous bytes); else a piece is one float.  Every output element is written
// exactly once.
template <bool VEC>
__global__ void __launch_bounds__(NV_THREADS)
letterbox_nv12_kernel(const uint8_t* __restrict__ pixels, const NvChunk chunk, const NvMatrix m,
                      float* __restrict__ out, int net_h, int net_w, int tiles_x) {
  constexpr int PER = VEC ? 4 : 1;
  constexpr int ROW_PIECES = 3 * NV_TC / PER;  // of a tile
  __shared__ float lut[256];                   // (float)((double)v / 255.0), as letterbox_kernel's
  __shared__ __attribute__((aligned(16))) unsigned rgb[NV_LDS_PIXELS];
  const NvFrame& f = chunk.f[blockIdx.y];
  const int ty = (int)(blockIdx.x / (unsigned)tiles_x), tx = (int)(blockIdx.x - (unsigned)ty * tiles_x);
  int y0 = 0, y1 = 0, x0 = 0, x1 = 0;
  const bool rows_in = nv_axis(ty, NV_TR, f.g.pad_y, f.g.h, f.g.H, f.g.h_scale, &y0, &y1);
  const bool cols_in = nv_axis(tx, NV_TC, f.g.pad_x, f.g.w, f.g.W, f.g.w_scale, &x0, &x1);
  const bool pad_only = !(rows_in && cols_in);  // workgroup-uniform, like everything above
  int stride = 0;
  bool staged = false;
  if (!pad_only) {
    lut[threadIdx.x] = (float)((double)threadIdx.x / 255.0);
    stride = nv_stride(&x0, x1);
    const int rows = y1 - y0 + 1;
    // (the host sets f.staged only where every tile fits; a rectangle that did not would gather)
    staged = f.staged && (long long)rows * stride <= NV_LDS_PIXELS;
    if (staged) nv_stage(pixels, f, m, rgb, y0, rows, x0, stride);
    __syncthreads();
  }
  const NvStagedFetch from_lds{rgb, y0, x0, stride};
  const int row_floats = 3 * net_w, e0 = tx * (3 * NV_TC);
  float* dst = out + (size_t)blockIdx.y * net_h * row_floats;
  auto pixel = [&](int oy, int ox, float* v) {
    if (staged) {
      NvStagedFetch fetch = from_lds;
      lb_sample(fetch, f.g, lut, oy, ox, 0, v);
    } else {
      NvGatherFetch fetch{pixels + f.g.offset, pixels + f.uv_offset, f.pitch, m};
      lb_sample(fetch, f.g, lut, oy, ox, 0, v);
    }
  };
  for (int p = threadIdx.x; p < NV_TR * ROW_PIECES; p += NV_THREADS) {
    const int row = p / ROW_PIECES, oy = ty * NV_TR + row, e = e0 + (p - row * ROW_PIECES) * PER;
    if (oy >= net_h || e >= row_floats) continue;  // the frame's last tiles
    float* at = dst + (size_t)oy * row_floats + e;
    const int ox = e / 3, k = e - 3 * ox;
    if (VEC) {
      float4 v = make_float4(0.5f, 0.5f, 0.5f, 0.5f);
      if (!pad_only) {
        // 4 floats from element e of the row: the rest of pixel e / 3 and the start of the next
        // (e + 3 < 3 * net_w, so that pixel exists, and it is the tile's: e0 % 12 == 0)
        float a[3], b[3];
        pixel(oy, ox, a);
        pixel(oy, ox + 1, b);
        v = k == 0 ? make_float4(a[0], a[1], a[2], b[0])
                   : (k == 1 ? make_float4(a[1], a[2], b[0], b[1]) : make_float4(a[2], b[0], b[1], b[2]));
      }
      *reinterpret_cast<float4*>(at) = v;
    } else {
      float v = 0.5f;
      if (!pad_only) {
        float a[3];
        pixel(oy, ox, a);
        v = k == 0 ? a[0] : (k == 1 ? a[1] : a[2]);
      }
      *at = v;
    }
  }
}

// ------------------------------------------------------------------------------ host
// the largest source rectangle, in LDS pixels, that a tile of this frame stages
static long long nv_footprint(const LbFrame& g, int net_h, int net_w) {
  long long rows = 0, stride = 0;
  int lo, hi;
  for (int t = 0; t < (net_h + NV_TR - 1) / NV_TR; ++t)
    if (nv_axis(t, NV_TR, g.pad_y, g.h, g.H, g.h_scale, &lo, &hi) && hi - lo + 1 > rows) rows = hi - lo + 1;
  for (int t = 0; t < (net_w + NV_TC - 1) / NV_TC; ++t)
    if (nv_axis(t, NV_TC, g.pad_x, g.w, g.W, g.w_scale, &lo, &hi)) {
      const int s = nv_stride(&lo, hi);
      if (s > stride) stride = s;
    }
  return rows * stride;
}

static int check_nv12_args(const char* who, const void* pixels, unsigned long long pixels_bytes,
                           const dnn_frame_nv12* frames, int n, const void* out, int net_h, int net_w, int matrix) {
  DNN_REQUIRE(n >= 0, "%s: n = %d", who, n);
  DNN_REQUIRE(net_h > 0 && net_w > 0, "%s: network input %d x %d", who, net_h, net_w);
  DNN_REQUIRE(3 * (long long)net_w * net_h <= 0x7fffffffLL - NV_THREADS * 4,
              "%s: network input %d x %d: 2^31 floats a frame or more", who, net_h, net_w);
  const int force = matrix & (DNN_NV12_FORCE_GATHER | DNN_NV12_FORCE_STAGED), base = matrix & ~force;
  DNN_REQUIRE(matrix >= 0 && base <= DNN_YUV_BT601_FULL && force != (DNN_NV12_FORCE_GATHER | DNN_NV12_FORCE_STAGED),
              "%s: matrix %d is none of DNN_YUV_BT601_LIMITED, DNN_YUV_BT709_LIMITED, DNN_YUV_BT601_FULL, alone or "
              "with ONE of DNN_NV12_FORCE_GATHER, DNN_NV12_FORCE_STAGED", who, matrix);
  if (n == 0) return 0;
  DNN_REQUIRE(pixels && frames && out, "%s: NULL pointer", who);
  for (int i = 0; i < n; ++i) {
    const dnn_frame_nv12& fr = frames[i];
    DNN_REQUIRE(fr.h >= 1 && fr.w >= 1, "%s: frame %d has size %d x %d", who, i, fr.h, fr.w);
    const unsigned long long row = 2ull * (((unsigned long long)fr.w + 1) / 2);  // a UV row's used bytes
    DNN_REQUIRE(fr.pitch >= 0 && (unsigned long long)fr.pitch >= row,
                "%s: frame %d (%d x %d) has pitch %d, below the %llu bytes of a row", who, i, fr.h, fr.w, fr.pitch,
                row);
    // the bytes read: whole pitches but for the last row's used bytes
    const unsigned long long yb = ((unsigned long long)fr.h - 1) * fr.pitch + fr.w;
    const unsigned long long ub = (((unsigned long long)fr.h + 1) / 2 - 1) * fr.pitch + row;
    DNN_REQUIRE(fr.y_offset <= pixels_bytes && yb <= pixels_bytes - fr.y_offset,
                "%s: frame %d (%d x %d, pitch %d): the Y plane at byte %llu ends past the %llu pixel bytes", who, i,
                fr.h, fr.w, fr.pitch, fr.y_offset, pixels_bytes);
    DNN_REQUIRE(fr.uv_offset <= pixels_bytes && ub <= pixels_bytes - fr.uv_offset,
                "%s: frame %d (%d x %d, pitch %d): the UV plane at byte %llu ends past the %llu pixel bytes", who, i,
                fr.h, fr.w, fr.pitch, fr.uv_offset, pixels_bytes);
    LbGeom g;
    DNN_REQUIRE(letterbox_geom(fr.h, fr.w, net_h, net_w, &g),
                "%s: frame %d (%d x %d) letterboxes into %d x %d with a side below 2 pixels", who, i, fr.h, fr.w,
                net_h, net_w);
    if (force == DNN_NV12_FORCE_STAGED) {
      const long long need = nv_footprint(lb_frame(fr.y_offset, fr.h, fr.w, net_h, net_w), net_h, net_w);
      DNN_REQUIRE(need <= NV_LDS_PIXELS,
                  "%s: frame %d (%d x %d): DNN_NV12_FORCE_STAGED, but a tile's source rectangle has %lld pixels, "
                  "above the %d staged", who, i, fr.h, fr.w, need, NV_LDS_PIXELS);
    }
  }
  return 0;
}

// arguments already checked
static int launch_nv12(const uint8_t* d_pixels, const dnn_frame_nv12* frames, int n, float* d_out, int net_h,
                       int net_w, int matrix, hipStream_t stream) {
  const int force = matrix & (DNN_NV12_FORCE_GATHER | DNN_NV12_FORCE_STAGED);
  const NvMatrix m = NV_MATRICES[matrix & ~force];
  const bool vec = net_w % 4 == 0 && reinterpret_cast<uintptr_t>(d_out) % 16 == 0;
  const int tiles_x = (net_w + NV_TC - 1) / NV_TC, tiles_y = (net_h + NV_TR - 1) / NV_TR;
  const size_t frame_floats = (size_t)net_h * net_w * 3;
  for (int c0 = 0; c0 < n; c0 += LB_CHUNK) {
    const int cnt = n - c0 < LB_CHUNK ? n - c0 : LB_CHUNK;
    NvChunk chunk = {};
    for (int k = 0; k < cnt; ++k) {
      const dnn_frame_nv12& fr = frames[c0 + k];
      NvFrame& f = chunk.f[k];
      f.g = lb_frame(fr.y_offset, fr.h, fr.w, net_h, net_w);
      f.uv_offset = fr.uv_offset;
      f.pitch = fr.pitch;
      f.staged = force ? force == DNN_NV12_FORCE_STAGED : nv_footprint(f.g, net_h, net_w) <= NV_LDS_PIXELS;
    }
    const dim3 grid((unsigned)tiles_x * (unsigned)tiles_y, (unsigned)cnt);
    float* dst = d_out + (size_t)c0 * frame_floats;
    if (vec)
      hipLaunchKernelGGL(letterbox_nv12_kernel<true>, grid, dim3(NV_THREADS), 0, stream, d_pixels, chunk, m, dst,
                         net_h, net_w, tiles_x);
    else
      hipLaunchKernelGGL(letterbox_nv12_kernel<false>, grid, dim3(NV_THREADS), 0, stream, d_pixels, chunk, m, dst,
                         net_h, net_w, tiles_x);
    DNN_HIP_TRY(hipGetLastError());
  }
  return 0;
}

}  // namespace dnnhip

extern "C" {

int dnn_letterbox_frames_nv12(const uint8_t* d_pixels, unsigned long long pixels_bytes, const dnn_frame_nv12* frames,
                              int n, float* d_out, int net_h, int net_w, int matrix, void* stream) {
  const int rc = dnnhip::check_nv12_args("dnn_letterbox_frames_nv12", d_pixels, pixels_bytes, frames, n, d_out, net_h,
                                         net_w, matrix);
  if (rc || n == 0) return rc;
  return dnnhip::launch_nv12(d_pixels, frames, n, d_out, net_h, net_w, matrix, static_cast<hipStream_t>(stream));
}

int dnn_letterbox_frames_nv12_host(const uint8_t* pixels, unsigned long long pixels_bytes,
                                   const dnn_frame_nv12* frames, int n, float* out, int net_h, int net_w, int matrix) {
  int rc = dnnhip::check_nv12_args("dnn_letterbox_frames_nv12_host", pixels, pixels_bytes, frames, n, out, net_h,
                                   net_w, matrix);
  if (rc || n == 0) return rc;
  const size_t ib = ((size_t)pixels_bytes + 15) & ~(size_t)15;  // keeps the output 16-byte aligned
  const size_t ob = (size_t)n * net_h * net_w * 3 * sizeof(float);
  char* buf = nullptr;
  DNN_HIP_TRY(hipMalloc(&buf, ib + ob));
  if (hipMemcpy(buf, pixels, pixels_bytes, hipMemcpyHostToDevice) != hipSuccess) {
    dnnhip::set_error("dnn_letterbox_frames_nv12_host: copy in failed");
    rc = -1;
  }
  if (!rc)
    rc = dnnhip::launch_nv12(reinterpret_cast<const uint8_t*>(buf), frames, n, reinterpret_cast<float*>(buf + ib),
                             net_h, net_w, matrix, nullptr);
  if (!rc && hipMemcpy(out, buf + ib, ob, hipMemcpyDeviceToHost) != hipSuccess) {
    dnnhip::set_error("dnn_letterbox_frames_nv12_host: copy out failed");
    rc = -1;
  }
  (void)hipFree(buf);
  return rc;
}

}  // extern "C"
