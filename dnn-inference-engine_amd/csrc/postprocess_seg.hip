// Instance masks for the anchor-free heads (YOLOv8-seg, YOLO11-seg; include/dnn_hip_post.h: dnn_yolo_seg).
// Besides the DFL head's tensors a segmentation model gives nm mask coefficients per grid point and one
// prototype tensor [mask_h][mask_w][nm]; the mask of detection row k is the sign of coef[point(k)] . proto
// at every prototype pixel, cropped to the row's box.  That is a [rows x nm] . [nm x mask_h mask_w] matrix
// product per image with a 1-bit epilogue, so it runs on the fp32 MFMA (v_mfma_f32_16x16x4_f32), M = rows,
// N = pixels, K = nm.  Five launches on the stream: the DFL decode's three (postprocess_dfl.hip, whose NMS
// kernel also writes points[k], the grid point row k came from), then
//
//   yolo_seg_gather_kernel  one thread per (image, row k < max_masks, 16-byte piece of a coefficient row):
//       points[k] -> (scale, cell) through the head's grids, the row copied to coefrows[image][k][nm] in
//       the workspace (a zero row for k >= count); the thread of piece 0 also writes the row's crop
//       rectangle in prototype pixels, (x0, x1, y0, y1) = the smallest and one-past-largest pixel of the
//       integer crop rule, all zero for an empty box.  Nothing for an image with a code.
//   yolo_seg_mask_kernel<nm / 16>  grid (strips of prototype rows, image), 256 threads = 4 waves.  A strip
//       is strip_h rows with strip_h * W32 <= 32 (y, word) UNITS; wave w takes units w, w + 4, ...  A unit
//       is 32 consecutive pixels of a row = two 16-pixel N tiles.
//     B (prototypes): lane l holds pixel l % 16 of a tile and the contiguous channels [(l / 16) nm / 4,
//       (l / 16 + 1) nm / 4): nm / 16 16-byte loads a tile, four lanes cover a pixel's 4 nm bytes.  MFMA step
//       j multiplies channel (l / 16) nm / 4 + j: a permutation of K that A shares, so it costs nothing.
//       Pixels at or beyond mask_w load nothing (zeros) and give bit 0.  B is loaded once a unit and stays
//       in registers while the wave walks every 16-row tile of the staged rows.
//     A (coefficients): the workgroup stages up to 128 rows of coefrows and their rectangles in LDS (a
//       CHUNK; an image with more rows takes several, and re-reads its prototypes once per chunk, from L2).
//       Lane l reads row l % 16 of the tile, the same channel run, as nm / 16 ds_read_b128.  Row stride
//       nm + 4 floats: the 16 lanes of a quarter then start at 16 different multiples of 4 banks modulo 64
//       (and any 8 consecutive ones modulo 32) for nm = 16, 32, 48 and 64, so the read has no conflicts.
//     skip: each 16-row tile carries the union of its rectangles (computed after staging); a (tile, y, word)
//       outside it issues no MFMA and stores zero words.  Boxes are small: most of the work is this skip.
//     epilogue: accumulator register i of lane l is row 4 (l / 16) + i, pixel l % 16; the predicate is
//       acc > 0 (false for NaN) and inside the row's rectangle; one 64-bit ballot per (i, N tile) is 16 bits
//       for each of four rows, and the two tiles' halves make the row's 32-bit word.  Lane r < 16 keeps the
//       word of row r and writes it to LDS as out[row][unit] (stride 33 words); after the units the whole
//       workgroup stores, per row, its strip_h * W32 words, which are contiguous in masks, with plain
//       vector stores.  Every word of rows k < min(count, max_masks) is written once; no atomics, no clear.
//
// Budget (nm = 64 / 32).  LDS: A 128 x (nm + 4) x 4 = 34,816 / 18,432 B, rectangles 2,048 + 128 B, out
// 128 x 33 x 4 = 16,896 B: 53,888 / 37,504 B, three / four workgroups in a CU's 160 KiB.  VGPRs: B 2 x nm / 4
// = 32 / 16, A nm / 4 = 16 / 8, the rest addresses and rectangles: 86 / 70 as compiled (76 at nm = 48, 64 at
// nm = 16), plus 8 AGPRs of accumulators, no spills.  LDS, not registers, bounds the occupancy: 3 / 4 waves
// a SIMD (5 at nm = 16).  The gather kernel: 27 VGPRs, no LDS.
#include "post_dfl_host.h"

namespace dnnhip {

typedef float seg_f32x4 __attribute__((ext_vector_type(4)));

constexpr int PS_THREADS = 256;
constexpr int PS_CHUNK = 128;  // coefficient rows staged at a time
constexpr int PS_UNITS = 32;   // the most (y, word) units of a strip
constexpr int PS_OUT_LD = PS_UNITS + 1;
constexpr int PS_PAD = 4;      // floats added to a staged row's stride (see the top of the file)
static_assert(DNN_YOLO_SEG_MAX_SIDE <= 32 * PS_UNITS, "one prototype row is at most PS_UNITS words");

struct SegCoef {
  const float* p[DNN_YOLO_MAX_SCALES];
};

// rows of a strip: about 8 units (two a wave), never more than PS_UNITS
static int seg_strip_h(int w32) { return (8 + w32 - 1) / w32; }

// The workspace after the DFL decode's: byte offsets of points [n][max_det], coefrows [n][max_masks][nm],
// rects [n][max_masks] (each 16-byte aligned), and the total.
struct SegWs {
  unsigned long long points, coefrows, rects, total;
};
static SegWs seg_ws(int nb, int n_images, int max_det, const dnn_yolo_seg& g) {
  auto up = [](unsigned long long v) { return (v + 15ull) & ~15ull; };
  SegWs w;
  w.points = up(wide_workspace(nb, n_images));
  w.coefrows = up(w.points + (unsigned long long)n_images * max_det * sizeof(int));
  w.rects = w.coefrows + (unsigned long long)n_images * g.max_masks * g.n_coef * sizeof(float);
  w.total = w.rects + (unsigned long long)n_images * g.max_masks * sizeof(int4);
  return w;
}

__device__ __forceinline__ long long clamp_i64(long long v, long long lo, long long hi) {
  return v < lo ? lo : v > hi ? hi : v;
}

__global__ void __launch_bounds__(PS_THREADS)
yolo_seg_gather_kernel(const dnn_yolo_dfl h, const dnn_yolo_seg g, const SegCoef coef,
                       const dnn_detection* __restrict__ dets, const int* __restrict__ counts,
                       const int* __restrict__ points, int max_det, float* __restrict__ coefrows,
                       int4* __restrict__ rects) {
  const int pieces = g.n_coef / 4, img = blockIdx.y;
  const int i = blockIdx.x * PS_THREADS + threadIdx.x;
  if (i >= g.max_masks * pieces) return;
  const int k = i / pieces, q = i - k * pieces;
  const int count = counts[img];
  if (count < 0) return;
  seg_f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
  int4 rc = make_int4(0, 0, 0, 0);
  if (k < count) {  // k < max_masks <= max_det: the row and its point were written
    const int p = points[(size_t)img * max_det + k];
    int s = 0, off = 0, b = h.scale[0].grid_h * h.scale[0].grid_w;
    while (s + 1 < h.n_scales && p >= off + b) {
      off += b;
      ++s;
      b = h.scale[s].grid_h * h.scale[s].grid_w;
    }
    int cell = p - off;
    cell = cell < 0 ? 0 : cell >= b ? b - 1 : cell;  // (a point index is always inside; never read outside)
    v = *reinterpret_cast<const seg_f32x4*>(coef.p[s] + ((size_t)img * b + cell) * g.n_coef + 4 * q);
    if (q == 0) {
      const dnn_detection d = dets[(size_t)img * max_det + k];
      const long long l = clamp_i64(d.left, 0, g.net_w), r = clamp_i64(d.right, 0, g.net_w);
      const long long t = clamp_i64(d.top, 0, g.net_h), bt = clamp_i64(d.bottom, 0, g.net_h);
      // the smallest x with x * net_w >= l * mask_w, and the smallest with x * net_w >= r * mask_w
      const int x0 = (int)((l * g.mask_w + g.net_w - 1) / g.net_w), x1 = (int)((r * g.mask_w + g.net_w - 1) / g.net_w);
      const int y0 = (int)((t * g.mask_h + g.net_h - 1) / g.net_h), y1 = (int)((bt * g.mask_h + g.net_h - 1) / g.net_h);
      if (x1 > x0 && y1 > y0) rc = make_int4(x0, x1, y0, y1);
    }
  }
  *reinterpret_cast<seg_f32x4*>(coefrows + ((size_t)img * g.max_masks + k) * g.n_coef + 4 * q) = v;
  if (q == 0) rects[(size_t)img * g.max_masks + k] = rc;
}

template <int NK>  // nm / 16
__global__ void __launch_bounds__(PS_THREADS)
yolo_seg_mask_kernel(const dnn_yolo_seg g, const float* __restrict__ proto, const int* __restrict__ counts,
                     const float* __restrict__ coefrows, const int4* __restrict__ rects,
                     unsigned* __restrict__ masks, int strip_h) {
  constexpr int NM = 16 * NK, Q = NM / 4, LD = NM + PS_PAD;
  __shared__ __attribute__((aligned(16))) float a_lds[PS_CHUNK * LD];
  __shared__ int4 rect_lds[PS_CHUNK];
  __shared__ int4 uni_lds[PS_CHUNK / 16];
  __shared__ unsigned out_lds[PS_CHUNK * PS_OUT_LD];

  const int img = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int count = counts[img];
  const int nrows = count < g.max_masks ? count : g.max_masks;
  if (nrows <= 0) return;  // workgroup-uniform: a code, or no detection
  const int mh = g.mask_h, mw = g.mask_w, w32 = (mw + 31) >> 5;
  const int y_first = blockIdx.x * strip_h;
  const int sh = mh - y_first < strip_h ? mh - y_first : strip_h;  // >= 1 by the grid
  const int units = sh * w32;                                      // <= PS_UNITS
  const float* crow = coefrows + (size_t)img * g.max_masks * NM;
  const int4* rrow = rects + (size_t)img * g.max_masks;
  unsigned* mrow = masks + (size_t)img * g.max_masks * mh * w32 + (size_t)y_first * w32;
  const int px = lane & 15, grp = lane >> 4;

  for (int c0 = 0; c0 < nrows; c0 += PS_CHUNK) {  // workgroup-uniform
    const int live = nrows - c0 < PS_CHUNK ? nrows - c0 : PS_CHUNK;
    const int tiles = (live + 15) >> 4;
    for (int i = tid; i < tiles * 16 * Q; i += PS_THREADS) {
      const int r = i / Q, q = i - r * Q;
      seg_f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
      if (r < live) v = *reinterpret_cast<const seg_f32x4*>(crow + (size_t)(c0 + r) * NM + 4 * q);
      *reinterpret_cast<seg_f32x4*>(&a_lds[r * LD + 4 * q]) = v;
    }
    for (int i = tid; i < tiles * 16; i += PS_THREADS) rect_lds[i] = i < live ? rrow[c0 + i] : make_int4(0, 0, 0, 0);
    __syncthreads();
    if (tid < tiles) {  // the union of the tile's non-empty rectangles; all zero when it has none
      int4 un = make_int4(0x7fffffff, 0, 0x7fffffff, 0);
      for (int r = 0; r < 16; ++r) {
        const int4 rc = rect_lds[16 * tid + r];
        if (rc.y <= rc.x) continue;
        un.x = rc.x < un.x ? rc.x : un.x;
        un.y = rc.y > un.y ? rc.y : un.y;
        un.z = rc.z < un.z ? rc.z : un.z;
        un.w = rc.w > un.w ? rc.w : un.w;
      }
      uni_lds[tid] = un.y > 0 ? un : make_int4(0, 0, 0, 0);
    }
    __syncthreads();

    for (int u = wid; u < units; u += PS_THREADS / 64) {  // no workgroup barrier inside
      const int yl = u / w32, word = u - yl * w32, y = y_first + yl;
      seg_f32x4 b[2][NK];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const int x = word * 32 + t * 16 + px;
        const float* src = proto + (((size_t)img * mh + y) * mw + (x < mw ? x : 0)) * NM + grp * Q;
#pragma unroll
        for (int j = 0; j < NK; ++j) {
          b[t][j] = seg_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
          if (x < mw) b[t][j] = *reinterpret_cast<const seg_f32x4*>(src + 4 * j);
        }
      }
      const int x_a = word * 32 + px, x_b = x_a + 16;
      for (int tile = 0; tile < tiles; ++tile) {
        const int4 un = uni_lds[tile];
        unsigned mine = 0;  // lane r < 16: the word of row 16 tile + r
        if (y >= un.z && y < un.w && word * 32 < un.y && word * 32 + 32 > un.x) {  // wave-uniform
          seg_f32x4 a[NK];
#pragma unroll
          for (int j = 0; j < NK; ++j)
            a[j] = *reinterpret_cast<const seg_f32x4*>(&a_lds[(tile * 16 + px) * LD + grp * Q + 4 * j]);
          seg_f32x4 acc0 = {0.0f, 0.0f, 0.0f, 0.0f}, acc1 = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
          for (int j = 0; j < NK; ++j) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j][e], b[0][j][e], acc0, 0, 0, 0);
              acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j][e], b[1][j][e], acc1, 0, 0, 0);
            }
          }
          const int sel = 16 * ((lane >> 2) & 3);  // lane r < 16 takes row r = 4 (r / 4) + r % 4
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int4 rc = rect_lds[tile * 16 + 4 * grp + i];
            const bool in_y = y >= rc.z && y < rc.w;
            const unsigned long long m0 = __ballot(acc0[i] > 0.0f && in_y && x_a >= rc.x && x_a < rc.y);
            const unsigned long long m1 = __ballot(acc1[i] > 0.0f && in_y && x_b >= rc.x && x_b < rc.y);
            const unsigned w = (unsigned)((m0 >> sel) & 0xffffull) | ((unsigned)((m1 >> sel) & 0xffffull) << 16);
            if ((lane & 3) == i) mine = w;
          }
        }
        if (lane < 16) out_lds[(tile * 16 + lane) * PS_OUT_LD + u] = mine;
      }
    }
    __syncthreads();
    for (int i = tid; i < live * units; i += PS_THREADS) {  // a row's words of the strip are contiguous
      const int r = i / units, u = i - r * units;
      mrow[(size_t)(c0 + r) * mh * w32 + u] = out_lds[r * PS_OUT_LD + u];
    }
    __syncthreads();  // before the next chunk is staged over this one
  }
}

// ---- host side -------------------------------------------------------------------------------------
// < 0 with the error set (it names the field), else the words of one mask
static int seg_words(const dnn_yolo_seg* g, const char* who) {
  DNN_REQUIRE(g, "%s: NULL mask description", who);
  DNN_REQUIRE(g->n_coef == 16 || g->n_coef == 32 || g->n_coef == 48 || g->n_coef == 64,
              "%s: n_coef %d: need 16, 32, 48 or 64", who, g->n_coef);
  DNN_REQUIRE(g->mask_h >= 1 && g->mask_h <= DNN_YOLO_SEG_MAX_SIDE, "%s: mask_h %d: need 1..%d", who, g->mask_h,
              DNN_YOLO_SEG_MAX_SIDE);
  DNN_REQUIRE(g->mask_w >= 1 && g->mask_w <= DNN_YOLO_SEG_MAX_SIDE, "%s: mask_w %d: need 1..%d", who, g->mask_w,
              DNN_YOLO_SEG_MAX_SIDE);
  DNN_REQUIRE(g->net_h >= 1, "%s: net_h %d: need a positive number of pixels", who, g->net_h);
  DNN_REQUIRE(g->net_w >= 1, "%s: net_w %d: need a positive number of pixels", who, g->net_w);
  DNN_REQUIRE(g->max_masks >= 1, "%s: max_masks %d: need 1..max_det", who, g->max_masks);
  return g->mask_h * ((g->mask_w + 31) / 32);
}

struct SegCall {  // what an entry takes beside the DFL decode's arguments (d)
  DflCall d;
  const dnn_yolo_seg* g;
  const float* const* coef;
  const float* proto;
  unsigned int* masks;
};

// Every argument check: the mask description, the DFL decode's checks (its workspace check aside), max_masks
// against max_det, the pointers and, unless `host`, their alignment and the workspace.  < 0 with the error
// set; 0 with nothing to do; 1 with *nb, *mp and *sc filled.
static int check_seg_call(const SegCall& c, bool host, int* nb, MultiPred* mp, SegCoef* sc) {
  const char* who = c.d.who;
  const int words = seg_words(c.g, who);
  if (words < 0) return words;
  const int go = check_dfl_call(c.d, true, nb, mp);
  if (go <= 0) return go;
  DNN_REQUIRE(c.g->max_masks <= c.d.max_det, "%s: max_masks %d: need 1..max_det = %d", who, c.g->max_masks,
              c.d.max_det);
  DNN_REQUIRE(c.coef, "%s: coef is NULL", who);
  *sc = SegCoef{};
  for (int s = 0; s < c.d.h->n_scales; ++s) {
    DNN_REQUIRE(c.coef[s] && (host || !(reinterpret_cast<uintptr_t>(c.coef[s]) & 15u)),
                "%s: coef[%d] %p: need a 16-byte aligned tensor", who, s, (const void*)c.coef[s]);
    sc->p[s] = c.coef[s];
  }
  DNN_REQUIRE(c.proto && (host || !(reinterpret_cast<uintptr_t>(c.proto) & 15u)),
              "%s: proto %p: need a 16-byte aligned tensor", who, (const void*)c.proto);
  DNN_REQUIRE(c.masks && !(reinterpret_cast<uintptr_t>(c.masks) & 3u), "%s: masks %p: need a 4-byte aligned array",
              who, (void*)c.masks);
  const unsigned long long need = seg_ws(*nb, c.d.n_images, c.d.max_det, *c.g).total;
  DNN_REQUIRE(host || (c.d.workspace && c.d.workspace_bytes >= need &&
                       !(reinterpret_cast<uintptr_t>(c.d.workspace) & 15u)),
              "%s: workspace %p of %llu bytes; %d images of %d points, %d rows and %d masks need %llu bytes, 16-byte "
              "aligned", who, c.d.workspace, c.d.workspace_bytes, c.d.n_images, *nb, c.d.max_det, c.g->max_masks, need);
  return 1;
}

static int launch_yolo_seg(const SegCall& c, hipStream_t stream) {
  int nb;
  MultiPred mp;
  SegCoef sc;
  const int go = check_seg_call(c, false, &nb, &mp, &sc);
  if (go <= 0) return go;
  const dnn_yolo_seg& g = *c.g;
  const SegWs w = seg_ws(nb, c.d.n_images, c.d.max_det, g);
  char* ws = static_cast<char*>(c.d.workspace);
  int* points = reinterpret_cast<int*>(ws + w.points);
  float* coefrows = reinterpret_cast<float*>(ws + w.coefrows);
  int4* rects = reinterpret_cast<int4*>(ws + w.rects);

  DflCall d = c.d;
  d.points = points;
  const int rc = launch_yolo_dfl(d, stream);
  if (rc) return rc;

  const int pieces = g.max_masks * (g.n_coef / 4);
  hipLaunchKernelGGL(yolo_seg_gather_kernel, dim3((pieces + PS_THREADS - 1) / PS_THREADS, c.d.n_images),
                     dim3(PS_THREADS), 0, stream, *c.d.h, g, sc, c.d.dets, c.d.counts, points, c.d.max_det, coefrows,
                     rects);
  const int strip_h = seg_strip_h((g.mask_w + 31) / 32);
  const dim3 grid((g.mask_h + strip_h - 1) / strip_h, c.d.n_images);
  const auto mask = g.n_coef == 16 ? yolo_seg_mask_kernel<1> : g.n_coef == 32 ? yolo_seg_mask_kernel<2>
                    : g.n_coef == 48 ? yolo_seg_mask_kernel<3> : yolo_seg_mask_kernel<4>;
  hipLaunchKernelGGL(mask, grid, dim3(PS_THREADS), 0, stream, g, c.proto, c.d.counts, coefrows, rects, c.masks,
                     strip_h);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("launch yolo_seg: %s", hipGetErrorString(e));
    return -1;
  }
  return 0;
}

// Host pointers, synchronous: one allocation holding the tensors, the detections, the counts, the masks and the
// workspace (each 16-byte aligned), copy in (the masks too: rows the call does not make keep what they held),
// launch, copy out; freed on every path.
static int yolo_seg_host(const SegCall& c) {
  int nb;
  MultiPred mp;
  SegCoef sc;
  const int go = check_seg_call(c, true, &nb, &mp, &sc);
  if (go <= 0) return go;
  const dnn_yolo_dfl& h = *c.d.h;
  const dnn_yolo_seg& g = *c.g;
  const int n = c.d.n_images, ch = 4 * h.reg_max + h.n_classes;
  size_t total = 0;
  auto place = [&total](size_t bytes) {
    const size_t at = total;
    total += (bytes + 15) & ~(size_t)15;
    return at;
  };
  size_t pf[DNN_YOLO_MAX_SCALES] = {0}, cf[DNN_YOLO_MAX_SCALES] = {0}, poff[DNN_YOLO_MAX_SCALES] = {0},
         coff[DNN_YOLO_MAX_SCALES] = {0};
  for (int s = 0; s < h.n_scales; ++s) {
    const size_t pts = (size_t)n * h.scale[s].grid_h * h.scale[s].grid_w;
    pf[s] = pts * ch * sizeof(float);
    cf[s] = pts * g.n_coef * sizeof(float);
    poff[s] = place(pf[s]);
    coff[s] = place(cf[s]);
  }
  const size_t prb = (size_t)n * g.mask_h * g.mask_w * g.n_coef * sizeof(float);
  const size_t db = (size_t)n * c.d.max_det * sizeof(dnn_detection), cb = (size_t)n * sizeof(int);
  const size_t mb = (size_t)n * g.max_masks * g.mask_h * ((g.mask_w + 31) / 32) * sizeof(unsigned);
  const size_t wb = (size_t)seg_ws(nb, n, c.d.max_det, g).total;
  const size_t proff = place(prb), doff = place(db), coff2 = place(cb), moff = place(mb), woff = place(wb);
  char* buf = nullptr;
  DNN_HIP_TRY(hipMalloc(&buf, total));
  const float* d_pred[DNN_YOLO_MAX_SCALES] = {nullptr, nullptr, nullptr, nullptr};
  const float* d_coef[DNN_YOLO_MAX_SCALES] = {nullptr, nullptr, nullptr, nullptr};
  SegCall d = c;  // the same call on the device copies
  d.d.pred = d_pred;
  d.coef = d_coef;
  d.proto = reinterpret_cast<const float*>(buf + proff);
  d.d.dets = reinterpret_cast<dnn_detection*>(buf + doff);
  d.d.counts = reinterpret_cast<int*>(buf + coff2);
  d.masks = reinterpret_cast<unsigned*>(buf + moff);
  d.d.workspace = buf + woff;
  d.d.workspace_bytes = wb;
  bool ok = hipMemcpy(buf + proff, c.proto, prb, hipMemcpyHostToDevice) == hipSuccess &&
            hipMemcpy(buf + moff, c.masks, mb, hipMemcpyHostToDevice) == hipSuccess;
  for (int s = 0; s < h.n_scales && ok; ++s) {
    d_pred[s] = reinterpret_cast<const float*>(buf + poff[s]);
    d_coef[s] = reinterpret_cast<const float*>(buf + coff[s]);
    ok = hipMemcpy(buf + poff[s], c.d.pred[s], pf[s], hipMemcpyHostToDevice) == hipSuccess &&
         hipMemcpy(buf + coff[s], c.coef[s], cf[s], hipMemcpyHostToDevice) == hipSuccess;
  }
  int rc = 0;
  if (!ok) {
    set_error("%s: copy in failed", c.d.who);
    rc = -1;
  }
  if (!rc) rc = launch_yolo_seg(d, nullptr);
  if (!rc && (hipMemcpy(c.d.counts, d.d.counts, cb, hipMemcpyDeviceToHost) != hipSuccess ||
              hipMemcpy(c.d.dets, d.d.dets, db, hipMemcpyDeviceToHost) != hipSuccess ||
              hipMemcpy(c.masks, d.masks, mb, hipMemcpyDeviceToHost) != hipSuccess)) {
    set_error("%s: copy out failed", c.d.who);
    rc = -1;
  }
  (void)hipFree(buf);
  return rc;
}

}  // namespace dnnhip

extern "C" {

int dnn_yolo_seg_mask_words(const dnn_yolo_seg* seg) { return dnnhip::seg_words(seg, "dnn_yolo_seg_mask_words"); }

int dnn_yolo_dfl_seg_workspace(const dnn_yolo_dfl* h, const dnn_yolo_seg* seg, int n_images, int max_det,
                               unsigned long long* bytes) {
  const char* who = "dnn_yolo_dfl_seg_workspace";
  const int nb = dnnhip::dfl_boxes(h, who);
  if (nb < 0) return nb;
  const int words = dnnhip::seg_words(seg, who);
  if (words < 0) return words;
  DNN_REQUIRE(n_images >= 0 && bytes, "%s: bad arguments (n_images=%d)", who, n_images);
  DNN_REQUIRE(seg->max_masks <= max_det, "%s: max_masks %d: need 1..max_det = %d", who, seg->max_masks, max_det);
  *bytes = dnnhip::seg_ws(nb, n_images, max_det, *seg).total;
  return 0;
}

int dnn_yolo_postprocess_dfl_seg(const dnn_yolo_dfl* h, const dnn_yolo_seg* seg, const float* const* pred,
                                 const float* const* coef, const float* proto, int n_images, dnn_detection* dets,
                                 int max_det, int* counts, unsigned int* masks, void* workspace,
                                 unsigned long long workspace_bytes, int nms_mode, int labels_mode, void* stream) {
  return dnnhip::launch_yolo_seg({{"dnn_yolo_postprocess_dfl_seg", h, pred, n_images, dets, max_det, counts, workspace,
                                   workspace_bytes, nms_mode, labels_mode},
                                  seg, coef, proto, masks}, static_cast<hipStream_t>(stream));
}

int dnn_yolo_postprocess_dfl_seg_host(const dnn_yolo_dfl* h, const dnn_yolo_seg* seg, const float* const* pred,
                                      const float* const* coef, const float* proto, int n_images,
                                      dnn_detection* dets, int max_det, int* counts, unsigned int* masks,
                                      int nms_mode, int labels_mode) {
  return dnnhip::yolo_seg_host({{"dnn_yolo_postprocess_dfl_seg_host", h, pred, n_images, dets, max_det, counts, nullptr,
                                 0, nms_mode, labels_mode},
                                seg, coef, proto, masks});
}

}  // extern "C"
