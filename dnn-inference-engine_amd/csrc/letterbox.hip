// Letterbox ingest and its inverse on the detection rows (include/dnn_hip_ingest.h,
// include/dnn_hip_post.h): what the original Darknet does to an image before its network and to
// the boxes after it,
//     load_image:        float v = (float)byte / 255.            (here (float)((double)byte / 255.0),
//                                                                  preprocess_kernel's expression)
//     letterbox_image:   the largest size of the image's aspect that fits the network (integer
//                        division), resize_image to it, embedded centred in a 0.5 canvas
//     resize_image:      two bilinear passes, every source row horizontally, then vertically,
//                        with scale (src - 1) / (new - 1) and the last column / row special-cased
//     draw_detections:   corners clamped to [0, src - 1]
// as one kernel over a ragged batch of uint8 frames already on the device, and one kernel over
// the decode's rows.
//
// Geometry (ints; the two quotients and their comparison in fp32):
//   if (float)net_w / src_w < (float)net_h / src_h:  new_w = net_w, new_h = (src_h * net_w) / src_w
//   else:                                            new_h = net_h, new_w = (src_w * net_h) / src_h
//   pad_x = (net_w - new_w) / 2,  pad_y = (net_h - new_h) / 2
// Resize (W, H the source, w, h the new size, S the fp32 source after the / 255; every fp32
// operation rounded on its own, the file is built with -ffp-contract=off):
//   w_scale = (float)(W - 1) / (float)(w - 1),  h_scale = (float)(H - 1) / (float)(h - 1)
//   part(r, c) = S(r, W-1)                              if c == w-1 or W == 1
//              = (1 - dx) * S(r, ix) + dx * S(r, ix+1)  otherwise; sx = c * w_scale, ix = (int)sx, dx = sx - ix
//   out(r, c)  = (1 - dy) * part(iy, c)                 sy = r * h_scale, iy = (int)sy, dy = sy - iy
//   out(r, c) += dy * part(iy+1, c)                     unless r == h-1 or H == 1
// A thread forms the two part values it needs with the same three roundings each, so there is no
// part image.  The last-row rule is Darknet's and is kept: where (float)(h-1) * h_scale rounds
// below H - 1 (a 16-row source resized to 96 rows: row 95 has iy = 14, dy = 0.99999905), the second
// term is skipped and the last letterboxed row is nearly black.
//
// Darknet's source is not readable here, so parity with a Darknet binary is UNPINNED (its
// compiler may contract or reorder differently); the geometry, the / 255, the channel order, the
// arithmetic above and the fp32 rounding are exact against tests/letterbox_oracle.py, and a
// same-size letterbox is exact.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "dnn_common.h"
#include "../../include/dnn_hip_ingest.h"
#include "../../include/dnn_hip_post.h"

namespace dnnhip {

// ------------------------------------------------------------------------------ geometry (host)
struct LbGeom {
  int new_h, new_w, pad_y, pad_x;
};

// false: a side of the letterboxed image is below 2 (Darknet divides by new - 1) or, beyond the
// sizes fp32 quotients can order, above the network's
static bool letterbox_geom(int src_h, int src_w, int net_h, int net_w, LbGeom* g) {
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

// ------------------------------------------------------------------------------ letterbox kernel
// What the kernel needs of one frame; the host fills it and a chunk of them travels by value as
// the kernel's argument (no device-side descriptor table, no copy to wait for).
struct LbFrame {
  unsigned long long offset;  // of the frame's first byte in the pixel buffer
  int H, W;                   // source
  int h, w;                   // letterboxed image
  int pad_y, pad_x;
  float h_scale, w_scale;
};
constexpr int LB_CHUNK = 64;  // frames per launch: 64 x 40 B of kernel argument
struct LbChunk {
  LbFrame f[LB_CHUNK];
};

constexpr int LB_THREADS = 256;
constexpr int LB_ITERS = 4;  // stores per thread; a workgroup writes LB_THREADS * LB_ITERS pieces

// The three bytes of the source pixels at byte offsets at0 and at1 of the frame, as bytes 0..2 and
// 3..5 of the result: one 8-byte fetch where the pixels are neighbours and the fetch stays inside
// the frame, else six one-byte loads (the last column, the frame's last bytes).
__host__ __device__ __forceinline__ unsigned long long lb_fetch6(const uint8_t* __restrict__ img, size_t frame_bytes,
                                                               size_t at0, size_t at1) {
  unsigned long long q;
  if (at1 == at0 + 3 && at0 + 8 <= frame_bytes) {
    __builtin_memcpy(&q, img + at0, 8);
  } else {
    q = (unsigned long long)img[at0] | (unsigned long long)img[at0 + 1] << 8 | (unsigned long long)img[at0 + 2] << 16 |
        (unsigned long long)img[at1] << 24 | (unsigned long long)img[at1 + 1] << 32 |
        (unsigned long long)img[at1 + 2] << 40;
  }
  return q;
}

// pixel (oy, ox) of the network input, its three channels in output order (also host code, so a
// CPU build can run the same arithmetic)
__host__ __device__ __forceinline__ void lb_pixel(const uint8_t* __restrict__ img, const LbFrame& f, const float* lut,
                                                  int oy, int ox, int flip, float* out) {
  const int r = oy - f.pad_y, c = ox - f.pad_x;
  if ((unsigned)r >= (unsigned)f.h || (unsigned)c >= (unsigned)f.w) {
    out[0] = out[1] = out[2] = 0.5f;
    return;
  }
  const size_t frame_bytes = (size_t)f.H * f.W * 3;
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
  const size_t o0 = (size_t)iy * f.W * 3, o1 = (size_t)iy1 * f.W * 3;
  const unsigned long long q0 = lb_fetch6(img, frame_bytes, o0 + (size_t)ix * 3, o0 + (size_t)ix1 * 3);
  const unsigned long long q1 = two ? lb_fetch6(img, frame_bytes, o1 + (size_t)ix * 3, o1 + (size_t)ix1 * 3) : 0ull;
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

// Grid: x = pieces of one frame's output, y = frames of the chunk.  VEC: a piece is 16 bytes of
// the flattened [net_h][3 * net_w] frame (3 * net_w % 4 == 0, so no piece crosses a row, and a
// wave's 64 stores are 1 KiB contiguous); else a piece is one float.  Every output element is
// written exactly once; a workgroup whose rows all lie in the top or bottom pad only stores.
template <bool VEC>
__global__ void __launch_bounds__(LB_THREADS)
letterbox_kernel(const uint8_t* __restrict__ pixels, const LbChunk chunk, float* __restrict__ out, int net_h,
                 int net_w, int flip) {
  constexpr int PER = VEC ? 4 : 1;
  __shared__ float lut[256];  // (float)((double)v / 255.0): load_image's scaling, one division per value
  const LbFrame& f = chunk.f[blockIdx.y];
  // (32-bit piece indices: the entry refuses a network input of 2^31 floats a frame or more)
  const unsigned row_pieces = 3u * net_w / PER;                // VEC: exact
  const unsigned pieces = (unsigned)net_h * row_pieces;
  float* dst = out + (size_t)blockIdx.y * net_h * net_w * 3;
  const unsigned first = blockIdx.x * (unsigned)(LB_THREADS * LB_ITERS);
  unsigned last = first + LB_THREADS * LB_ITERS - 1;
  if (last > pieces - 1) last = pieces - 1;
  const int row_lo = (int)(first / row_pieces), row_hi = (int)(last / row_pieces);
  const bool pad_only = row_hi < f.pad_y || row_lo >= f.pad_y + f.h;  // workgroup-uniform
  if (!pad_only) {
    lut[threadIdx.x] = (float)((double)threadIdx.x / 255.0);
    __syncthreads();
  }
  const uint8_t* img = pixels + f.offset;
#pragma unroll
  for (int it = 0; it < LB_ITERS; ++it) {
    const unsigned p = first + it * LB_THREADS + threadIdx.x;
    if (p > last) break;
    if (VEC) {
      float4 v = make_float4(0.5f, 0.5f, 0.5f, 0.5f);
      if (!pad_only) {
        // 4 floats from element e of the row: the rest of pixel e / 3 and the start of the next
        // (e + 3 < 3 * net_w, so that pixel exists)
        const int oy = (int)(p / row_pieces), e = (int)(p - (unsigned)oy * row_pieces) * 4;
        const int ox = e / 3, k = e - 3 * ox;
        float a[3], b[3];
        lb_pixel(img, f, lut, oy, ox, flip, a);
        lb_pixel(img, f, lut, oy, ox + 1, flip, b);
        v = k == 0 ? make_float4(a[0], a[1], a[2], b[0])
                   : (k == 1 ? make_float4(a[1], a[2], b[0], b[1]) : make_float4(a[2], b[0], b[1], b[2]));
      }
      reinterpret_cast<float4*>(dst)[p] = v;
    } else {
      float v = 0.5f;
      if (!pad_only) {
        const int oy = (int)(p / row_pieces), e = (int)(p - (unsigned)oy * row_pieces);
        const int ox = e / 3, k = e - 3 * ox;
        float a[3];
        lb_pixel(img, f, lut, oy, ox, flip, a);
        v = k == 0 ? a[0] : (k == 1 ? a[1] : a[2]);
      }
      dst[p] = v;
    }
  }
}

static int check_letterbox_args(const char* who, const void* pixels, unsigned long long pixels_bytes,
                                const dnn_frame* frames, int n, const void* out, int net_h, int net_w, int order) {
  DNN_REQUIRE(n >= 0, "%s: n = %d", who, n);
  DNN_REQUIRE(net_h > 0 && net_w > 0, "%s: network input %d x %d", who, net_h, net_w);
  DNN_REQUIRE(3 * (long long)net_w * net_h <= 0x7fffffffLL - LB_THREADS * LB_ITERS,
              "%s: network input %d x %d: 2^31 floats a frame or more", who, net_h, net_w);  // the kernel's indices
  DNN_REQUIRE(order == DNN_PIXELS_BGR || order == DNN_PIXELS_RGB, "%s: order %d is neither DNN_PIXELS_BGR nor "
              "DNN_PIXELS_RGB", who, order);
  if (n == 0) return 0;
  DNN_REQUIRE(pixels && frames && out, "%s: NULL pointer", who);
  for (int i = 0; i < n; ++i) {
    const dnn_frame& fr = frames[i];
    DNN_REQUIRE(fr.h >= 1 && fr.w >= 1, "%s: frame %d has size %d x %d", who, i, fr.h, fr.w);
    const unsigned long long bytes = 3ull * (unsigned long long)fr.h * (unsigned long long)fr.w;
    DNN_REQUIRE(fr.offset <= pixels_bytes && bytes <= pixels_bytes - fr.offset,
                "%s: frame %d (%d x %d at byte %llu) ends past the %llu pixel bytes", who, i, fr.h, fr.w, fr.offset,
                pixels_bytes);
    LbGeom g;
    DNN_REQUIRE(letterbox_geom(fr.h, fr.w, net_h, net_w, &g),
                "%s: frame %d (%d x %d) letterboxes into %d x %d with a side below 2 pixels", who, i, fr.h, fr.w,
                net_h, net_w);
  }
  return 0;
}

// arguments already checked
static int launch_letterbox(const uint8_t* d_pixels, const dnn_frame* frames, int n, float* d_out, int net_h,
                            int net_w, int order, hipStream_t stream) {
  DNN_REQUIRE(3 * (long long)net_w * net_h <= 0x7fffffffLL - LB_THREADS * LB_ITERS,
              "dnn_letterbox_frames: network input %d x %d: 2^31 floats a frame or more", net_h, net_w);
  const bool vec = (3 * (long long)net_w) % 4 == 0 && reinterpret_cast<uintptr_t>(d_out) % 16 == 0;
  const long long pieces = (long long)net_h * (3 * (long long)net_w / (vec ? 4 : 1));
  const long long per_wg = LB_THREADS * LB_ITERS;
  const long long gx = (pieces + per_wg - 1) / per_wg;
  const size_t frame_floats = (size_t)net_h * net_w * 3;
  for (int c0 = 0; c0 < n; c0 += LB_CHUNK) {
    const int m = n - c0 < LB_CHUNK ? n - c0 : LB_CHUNK;
    LbChunk chunk = {};
    for (int k = 0; k < m; ++k) {
      const dnn_frame& fr = frames[c0 + k];
      LbGeom g;
      letterbox_geom(fr.h, fr.w, net_h, net_w, &g);
      LbFrame& f = chunk.f[k];
      f.offset = fr.offset;
      f.H = fr.h;
      f.W = fr.w;
      f.h = g.new_h;
      f.w = g.new_w;
      f.pad_y = g.pad_y;
      f.pad_x = g.pad_x;
      f.h_scale = (float)(fr.h - 1) / (float)(g.new_h - 1);
      f.w_scale = (float)(fr.w - 1) / (float)(g.new_w - 1);
    }
    const dim3 grid((unsigned)gx, (unsigned)m);
    float* dst = d_out + (size_t)c0 * frame_floats;
    const int flip = order == DNN_PIXELS_BGR;
    if (vec)
      hipLaunchKernelGGL(letterbox_kernel<true>, grid, dim3(LB_THREADS), 0, stream, d_pixels, chunk, dst, net_h,
                         net_w, flip);
    else
      hipLaunchKernelGGL(letterbox_kernel<false>, grid, dim3(LB_THREADS), 0, stream, d_pixels, chunk, dst, net_h,
                         net_w, flip);
    DNN_HIP_TRY(hipGetLastError());
  }
  return 0;
}

// ------------------------------------------------------------------------------ boxes back
struct CorrImage {
  int src_h, src_w, new_h, new_w, pad_y, pad_x;
};
constexpr int CORR_CHUNK = 64;
struct CorrChunk {
  CorrImage im[CORR_CHUNK];
};
constexpr int CORR_THREADS = 256;

__device__ __forceinline__ long long corr_axis(long long v, int pad, int nw, int src) {
  const long long lo = pad, hi = (long long)pad + nw;
  v = v < lo ? lo : (v > hi ? hi : v);  // clamp first: the product below stays under new * src
  const long long m = ((v - lo) * src) / nw;
  return m < src - 1 ? m : src - 1;
}

// one workgroup per image: rows [0, min(count, max_det)) rewritten in place, class and score
// untouched; an image with an error code (count < 0) and the rows past the count are left alone
__global__ void __launch_bounds__(CORR_THREADS)
correct_detections_kernel(dnn_detection* __restrict__ dets, const int* __restrict__ counts, int max_det,
                          const CorrChunk chunk) {
  const CorrImage& g = chunk.im[blockIdx.x];
  int cnt = counts[blockIdx.x];
  cnt = cnt > max_det ? max_det : cnt;
  dnn_detection* rows = dets + (size_t)blockIdx.x * max_det;
  for (int j = threadIdx.x; j < cnt; j += CORR_THREADS) {
    dnn_detection* d = rows + j;
    const long long l = d->left, t = d->top, r = d->right, b = d->bottom;
    d->left = corr_axis(l, g.pad_x, g.new_w, g.src_w);
    d->top = corr_axis(t, g.pad_y, g.new_h, g.src_h);
    d->right = corr_axis(r, g.pad_x, g.new_w, g.src_w);
    d->bottom = corr_axis(b, g.pad_y, g.new_h, g.src_h);
  }
}

static int check_correct_args(const char* who, const void* dets, const void* counts, int n, int max_det,
                              const dnn_image_size* sizes, int net_h, int net_w) {
  DNN_REQUIRE(n >= 0 && max_det >= 0, "%s: n_images = %d, max_det = %d", who, n, max_det);
  DNN_REQUIRE(net_h > 0 && net_w > 0, "%s: network input %d x %d", who, net_h, net_w);
  if (n == 0) return 0;
  DNN_REQUIRE(counts && sizes && (max_det == 0 || dets), "%s: NULL pointer", who);
  for (int i = 0; i < n; ++i) {
    DNN_REQUIRE(sizes[i].h >= 1 && sizes[i].w >= 1, "%s: image %d has size %d x %d", who, i, sizes[i].h, sizes[i].w);
    LbGeom g;
    DNN_REQUIRE(letterbox_geom(sizes[i].h, sizes[i].w, net_h, net_w, &g),
                "%s: image %d (%d x %d) letterboxes into %d x %d with a side below 2 pixels", who, i, sizes[i].h,
                sizes[i].w, net_h, net_w);
  }
  return 0;
}

// arguments already checked
static int launch_correct(dnn_detection* dets, const int* counts, int n, int max_det, const dnn_image_size* sizes,
                          int net_h, int net_w, hipStream_t stream) {
  if (max_det == 0) return 0;
  for (int c0 = 0; c0 < n; c0 += CORR_CHUNK) {
    const int m = n - c0 < CORR_CHUNK ? n - c0 : CORR_CHUNK;
    CorrChunk chunk = {};
    for (int k = 0; k < m; ++k) {
      LbGeom g;
      letterbox_geom(sizes[c0 + k].h, sizes[c0 + k].w, net_h, net_w, &g);
      chunk.im[k] = CorrImage{sizes[c0 + k].h, sizes[c0 + k].w, g.new_h, g.new_w, g.pad_y, g.pad_x};
    }
    hipLaunchKernelGGL(correct_detections_kernel, dim3((unsigned)m), dim3(CORR_THREADS), 0, stream,
                       dets + (size_t)c0 * max_det, counts + c0, max_det, chunk);
    DNN_HIP_TRY(hipGetLastError());
  }
  return 0;
}

}  // namespace dnnhip

extern "C" {

int dnn_letterbox_geometry(int src_h, int src_w, int net_h, int net_w, int* new_h, int* new_w, int* pad_y,
                           int* pad_x) {
  DNN_REQUIRE(new_h && new_w && pad_y && pad_x, "dnn_letterbox_geometry: NULL pointer");
  DNN_REQUIRE(src_h >= 1 && src_w >= 1 && net_h >= 1 && net_w >= 1,
              "dnn_letterbox_geometry: image %d x %d, network input %d x %d", src_h, src_w, net_h, net_w);
  dnnhip::LbGeom g;
  DNN_REQUIRE(dnnhip::letterbox_geom(src_h, src_w, net_h, net_w, &g),
              "dnn_letterbox_geometry: a %d x %d image letterboxes into %d x %d with a side below 2 pixels", src_h,
              src_w, net_h, net_w);
  *new_h = g.new_h;
  *new_w = g.new_w;
  *pad_y = g.pad_y;
  *pad_x = g.pad_x;
  return 0;
}

int dnn_letterbox_frames(const uint8_t* d_pixels, unsigned long long pixels_bytes, const dnn_frame* frames, int n,
                         float* d_out, int net_h, int net_w, int order, void* stream) {
  const int rc = dnnhip::check_letterbox_args("dnn_letterbox_frames", d_pixels, pixels_bytes, frames, n, d_out,
                                              net_h, net_w, order);
  if (rc || n == 0) return rc;
  return dnnhip::launch_letterbox(d_pixels, frames, n, d_out, net_h, net_w, order, static_cast<hipStream_t>(stream));
}

int dnn_letterbox_frames_host(const uint8_t* pixels, unsigned long long pixels_bytes, const dnn_frame* frames, int n,
                              float* out, int net_h, int net_w, int order) {
  int rc = dnnhip::check_letterbox_args("dnn_letterbox_frames_host", pixels, pixels_bytes, frames, n, out, net_h,
                                        net_w, order);
  if (rc || n == 0) return rc;
  const size_t ib = ((size_t)pixels_bytes + 15) & ~(size_t)15;  // keeps the output 16-byte aligned
  const size_t ob = (size_t)n * net_h * net_w * 3 * sizeof(float);
  char* buf = nullptr;
  DNN_HIP_TRY(hipMalloc(&buf, ib + ob));
  if (hipMemcpy(buf, pixels, pixels_bytes, hipMemcpyHostToDevice) != hipSuccess) {
    dnnhip::set_error("dnn_letterbox_frames_host: copy in failed");
    rc = -1;
  }
  if (!rc)
    rc = dnnhip::launch_letterbox(reinterpret_cast<const uint8_t*>(buf), frames, n,
                                  reinterpret_cast<float*>(buf + ib), net_h, net_w, order, nullptr);
  if (!rc && hipMemcpy(out, buf + ib, ob, hipMemcpyDeviceToHost) != hipSuccess) {
    dnnhip::set_error("dnn_letterbox_frames_host: copy out failed");
    rc = -1;
  }
  (void)hipFree(buf);
  return rc;
}

int dnn_yolo_correct_detections(dnn_detection* dets, const int* counts, int n_images, int max_det,
                                const dnn_image_size* sizes, int net_h, int net_w, void* stream) {
  const int rc = dnnhip::check_correct_args("dnn_yolo_correct_detections", dets, counts, n_images, max_det, sizes,
                                            net_h, net_w);
  if (rc || n_images == 0) return rc;
  return dnnhip::launch_correct(dets, counts, n_images, max_det, sizes, net_h, net_w,
                                static_cast<hipStream_t>(stream));
}

int dnn_yolo_correct_detections_host(dnn_detection* dets, const int* counts, int n_images, int max_det,
                                     const dnn_image_size* sizes, int net_h, int net_w) {
  int rc = dnnhip::check_correct_args("dnn_yolo_correct_detections_host", dets, counts, n_images, max_det, sizes,
                                      net_h, net_w);
  if (rc || n_images == 0 || max_det == 0) return rc;
  const size_t db = (size_t)n_images * max_det * sizeof(dnn_detection), cb = (size_t)n_images * sizeof(int);
  char* buf = nullptr;
  DNN_HIP_TRY(hipMalloc(&buf, db + cb));
  dnn_detection* d_dets = reinterpret_cast<dnn_detection*>(buf);
  int* d_counts = reinterpret_cast<int*>(buf + db);
  if (hipMemcpy(d_dets, dets, db, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(d_counts, counts, cb, hipMemcpyHostToDevice) != hipSuccess) {
    dnnhip::set_error("dnn_yolo_correct_detections_host: copy in failed");
    rc = -1;
  }
  if (!rc) rc = dnnhip::launch_correct(d_dets, d_counts, n_images, max_det, sizes, net_h, net_w, nullptr);
  if (!rc && hipMemcpy(dets, d_dets, db, hipMemcpyDeviceToHost) != hipSuccess) {
    dnnhip::set_error("dnn_yolo_correct_detections_host: copy out failed");
    rc = -1;
  }
  (void)hipFree(buf);
  return rc;
}

}  // extern "C"
