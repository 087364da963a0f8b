// Device-resident execution plan (include/dnn_hip_plan.h).
//
// The reference walks its graph node by node and round-trips every intermediate through
// host numpy arrays (proj3/dnn_openblas.py:29-57; each CUDA/cuBLAS call even mallocs and
// copies per image, dnn_cuda.cu:193-210).  Here the same node chain is lowered once to a
// list of device steps.  Each conv entry (Conv2D + its BiasAdd / BatchNorm / LeakyReLU as
// the GEMM epilogue) runs as one kernel variant (ConvVariant):
//   gemm       explicit im2col into a col buffer + LDS-tiled fp32-MFMA GEMM (the reference's
//              im2col + sgemm structure, dnn_openblas.c:160-194; generic fallback)
//   direct_a   1x1 / stride 1 / unpadded: the NHWC input IS the col matrix, GEMM only
//   implicit   implicit GEMM: the LDS-DMA loader gathers the im2col rows straight from the
//              input (per-lane source addresses), no col buffer
//   direct     3x3 conv with <= 4 input channels (conv0): direct FMA conv, weights in LDS
//   patch      3x3 SAME conv with 16/32 input channels + 2x2 pool (conv1): input patch and
//              weights DMA'd to LDS once per tile, taps are constant LDS offsets (conv_patch.hip)
//   patch16, tile16, img16   fp16 3x3 convs on a zero-bordered input: whole rows, 2-D tiles with
//              the 2x2/s2 pool, one frame per tile with a 2x2/s1 pool (conv6/conv7, conv2-conv4, conv5)
//   x3, x3_lat, x3_ktile, x3_img   fp32 3x3 convs on the bf16 MFMA with exact 3-way splits, reading
//              split zero-bordered planes: the batch tiles, the small-M K slices, the K split
//              inside the workgroup (latency plans), whole-image tiles with a 2x2/s1 pool
//   x3_1x1, x3_1x1_ktile   fp32 1x1 conv with the same arithmetic on its producer's split planes
// and a following 2x2 MaxPool2D is fused into the conv where the variant can take it (PoolFuse:
// stride 2 with pool-window-major rows, or stride 1 on the same frame), otherwise it is its own
// pool entry.  Weights are packed once
// into a device arena as Bt[Npad][Kpad] (K order kh,kw,ic; HWIO as-is for direct) plus four
// Npad-long epilogue vectors (bias, mean, sqrt(var+eps), gamma).  Activations ping-pong
// between two workspace buffers.  DNN_HIP_FUSE=0 in the environment at plan creation
// forces the explicit GEMM path with separate pools (for A/B checks); DNN_HIP_PATCH=0 keeps
// patch-eligible layers on the implicit GEMM.
//
// Layers, steps, walker: the dnn_plan_add_* entries only record layers (and rewrite the last ones:
// a pool fuses into its conv, a conv asks its producer for a zero-bordered output).  layout()
// lowers the layers to steps, one per kernel launch in launch order, each with its name, flops,
// bytes and the resolved locations it reads and writes, and fills the workspace map (WsMap).
// dnn_plan_run walks the steps: record(i), launch step i; the per-kernel timings, marks and clock
// stamps index the same list, so they cannot drift from what runs.
//
// Fork / join (fp32 plans): a stash entry names the current tensor as a slot, and the layer that
// produces it writes it into the slot's own workspace region instead of an activation buffer, so
// it outlives the ping-pong; a restore entry makes a slot the current tensor again; a route entry
// (route.hip) folds the current tensor block x block into channels and concatenates it with a
// slot's tensor.  Stash and restore launch nothing.  All three are plan layers, so the peepholes
// of dnn_plan_add_conv / dnn_plan_add_max_pool, which rewrite layers.back(), stop at them: a
// stashed tensor and both inputs of a route are always plain NHWC fp32.
//
// Residual and top-down plans: a shortcut entry (shortcut.hip) adds a slot's tensor to the current
// one, an upsample entry repeats the current tensor's pixels, a release entry ends a slot's life.
// A released slot number is handed out again by the next stash, and a region is handed out again
// once no live slot names it and the current tensor has left it, but only to a producer added
// after that point (region_free_from): a layer never writes a region that it, or a layer before
// it, still reads.  Plans without a release are laid out exactly as before.
//
// Taps: a tap entry makes the current tensor an extra output of the plan.  It is a stash without a
// slot number: the producer writes the tensor into a region (to_region), the tap holds a reference
// to that region that is never dropped, so no later producer is given it, and the caller reads the
// region's device address (dnn_plan_tap_buffer) after a run.
//
// Spatial pyramid pooling: an spp entry (spp.hip) writes up to three stride-1 SAME max pools of the
// current tensor and the tensor itself as channel blocks of one output, in one kernel.  Like the
// other join entries it reads and writes plain NHWC fp32 and stops the conv / pool peepholes.
//
// Channel slice: a slice entry (slice.hip) copies a channel range of the current tensor (Darknet's
// [route] with groups / group_id), one kernel, plain NHWC fp32 on both sides like the entries above.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "dnn_common.h"
#include "plan_internal.h"
#include "../../include/dnn_hip_plan.h"

namespace dnnhip {

static thread_local std::string g_last_error;

void set_error(const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_last_error = buf;
}
const char* last_error() { return g_last_error.c_str(); }

// The one reader of the environment (dnn_common.h: Switches holds the defaults).  DNN_HIP_LIB,
// _DEVICE, _PRECISION, _LATENCY and _NO_TORCH belong to the Python package.
Switches read_switches() {
  Switches s;
  // a switch that is on unless its variable starts with '0'
  auto on = [](const char* name) {
    const char* e = getenv(name);
    return !(e && e[0] == '0');
  };
  auto num = [](const char* name, long long unset) {
    const char* e = getenv(name);
    return e ? atoll(e) : unset;
  };
  // "K:v,K:v,..." up to the first entry that does not parse
  auto pairs = [](const char* name) {
    std::vector<std::pair<int, int>> out;
    const char* e = getenv(name);
    for (const char* q = e ? e : ""; *q;) {
      int k = 0, v = 0, n = 0;
      if (sscanf(q, "%d:%d%n", &k, &v, &n) != 2) break;
      out.emplace_back(k, v);
      q += n;
      if (*q == ',') ++q;
    }
    return out;
  };
  s.fuse = on("DNN_HIP_FUSE");
  s.patch = on("DNN_HIP_PATCH");
  s.splitk_fused = on("DNN_HIP_SPLITK_FUSED");
  s.cfg = pairs("DNN_HIP_CFG");
  s.split = pairs("DNN_HIP_SPLIT");
  s.x3 = on("DNN_HIP_X3");
  s.x3_tile = on("DNN_HIP_X3_TILE");
  s.x3_c16 = on("DNN_HIP_X3_C16");
  s.x3_img = on("DNN_HIP_X3_IMG");
  s.x3_1x1 = on("DNN_HIP_X3_1X1");
  s.x3_h2 = on("DNN_HIP_X3_H2");
  s.x3l_cpw = (int)num("DNN_HIP_X3L_CPW", s.x3l_cpw);
  s.x3_lat_minwg = num("DNN_HIP_X3_LAT_MINWG", s.x3_lat_minwg);
  s.x3_c16p = on("DNN_HIP_X3_C16P");
  s.x3_c16pp = on("DNN_HIP_X3_C16PP");
  s.x3_pp = on("DNN_HIP_X3_PP");
  s.x3_pp_prio = on("DNN_HIP_X3_PP_PRIO");
  if (const char* e = getenv("DNN_HIP_PATCH16")) s.patch16 = e[0] == '1';
  s.tile16 = on("DNN_HIP_TILE16");
  s.img16 = on("DNN_HIP_IMG16");
  s.f16_direct_out = on("DNN_HIP_F16_DIRECT_OUT");
  s.tile16_wgs = (int)num("DNN_HIP_TILE16_WGS", s.tile16_wgs);
  s.c1f16_wgs = (int)num("DNN_HIP_C1F16_WGS", s.c1f16_wgs);
  s.gemm_buf = on("DNN_HIP_GEMM_BUF");
  s.persist = (int)num("DNN_HIP_PERSIST", s.persist);
  s.im2col_rows = on("DNN_HIP_IM2COL_ROWS");
  s.c0_grid = (int)num("DNN_HIP_C0_GRID", s.c0_grid);
  s.c0_d16 = on("DNN_HIP_C0_D16");
  return s;
}

int device_cu_count() {
  // compute units of the current device (256 on MI355X), cached per device
  static int cache[64] = {0};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
  if (!cache[dev]) {
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
    cache[dev] = n;
  }
  return cache[dev];
}

void out_pads(int in, int k, int s, int same, int* out, int* pad_front) {
  // proj3/dnn_openblas.py:127-142 (TensorFlow SAME / VALID)
  if (same) {
    int o = (in + s - 1) / s;
    int pad = (o - 1) * s + k - in;
    if (pad < 0) pad = 0;
    *out = o;
    *pad_front = pad / 2;
  } else {
    int span = in - k + 1;
    *out = span > 0 ? (span + s - 1) / s : 0;
    *pad_front = 0;
  }
}

int spp_sizes_ok(const char* who, int n_sizes, const int* sizes) {
  DNN_REQUIRE(sizes != nullptr, "%s: sizes is NULL", who);
  DNN_REQUIRE(n_sizes >= 1 && n_sizes <= DNN_SPP_MAX_SIZES, "%s: n_sizes %d outside 1..%d", who, n_sizes,
              DNN_SPP_MAX_SIZES);
  for (int j = 0; j < n_sizes; ++j)
    DNN_REQUIRE(sizes[j] >= 3 && sizes[j] <= DNN_SPP_MAX_K && sizes[j] % 2 == 1,
                "%s: size %d (entry %d) is not odd and in 3..%d", who, sizes[j], j, DNN_SPP_MAX_K);
  return 0;
}

}  // namespace dnnhip

using namespace dnnhip;

// The launcher form a conv entry runs as, each named once (the header comment describes them;
// kVariantName is what dnn_plan_describe prints as mode=).
enum ConvVariant : int {
  CONV_GEMM, CONV_DIRECT_A, CONV_IMPLICIT, CONV_DIRECT, CONV_PATCH,  // both precisions
  CONV_PATCH16, CONV_TILE16, CONV_IMG16,                             // fp16, zero-bordered input
  CONV_X3, CONV_X3_LAT, CONV_X3_KTILE, CONV_X3_IMG,                  // fp32 3x3 on split planes
  CONV_X3_1X1, CONV_X3_1X1_KTILE                                     // fp32 1x1 on split planes
};
static const char* const kVariantName[] = {"gemm", "direct_a", "implicit", "direct", "patch", "patch16", "tile16",
                                           "tile16", "patch_x3", "x3_lat", "x3_ktile", "x3_img", "x3_1x1",
                                           "x3_ktile"};
// a 2x2 max pool fused into a conv, as the launchers take it: stride 2 (pool-window-major rows, the
// output frame is PH x PW) or stride 1 SAME (the same output frame)
enum PoolFuse : int { POOL_NONE = 0, POOL_S2 = 1, POOL_S1 = 2 };

static bool is_x3(int v) { return v >= CONV_X3 && v <= CONV_X3_IMG; }  // the 3x3 x3 convs
static bool is_x3_1x1(int v) { return v == CONV_X3_1X1 || v == CONV_X3_1X1_KTILE; }
static bool is_tile16(int v) { return v == CONV_TILE16 || v == CONV_IMG16; }
// the x3 arithmetic: the input is the producer's split planes (the 16-channel x3 conv alone reads
// fp32, add_conv_layer) and the weights are three bf16 pieces each
static bool reads_split_planes(int v) { return is_x3(v) || is_x3_1x1(v); }
// how upload_weights packs Bt: three bf16 pieces per weight, or launch_pack_weights' order
enum WeightPack : int { PACK_HWIO, PACK_BT, PACK_BT_TILE16, PACK_BT_PATCH16, PACK_X3 };
static WeightPack weight_pack(int v) {
  return v == CONV_DIRECT ? PACK_HWIO : reads_split_planes(v) ? PACK_X3 : is_tile16(v) ? PACK_BT_TILE16
         : v == CONV_PATCH16 ? PACK_BT_PATCH16 : PACK_BT;
}

// where a tensor of a run lives: the caller's output / input, one of the two ping-pong activation
// buffers, slot region r (LOC_REGION + r), or layer j's zero-bordered / split-plane area (LOC_PAD + j)
enum TensorLoc : int { LOC_NONE = -2, LOC_OUT = -1, LOC_ACT0 = 0, LOC_ACT1 = 1, LOC_IN = 2, LOC_REGION = 3,
                       LOC_PAD = 1 << 24 };

enum LayerType : int { LAYER_CONV = 0, LAYER_POOL = 1, LAYER_STASH = 2, LAYER_RESTORE = 3, LAYER_ROUTE = 4,
                       LAYER_SHORTCUT = 5, LAYER_UPSAMPLE = 6, LAYER_RELEASE = 7, LAYER_TAP = 8, LAYER_SPP = 9,
                       LAYER_SLICE = 10 };

struct PlanLayer {
  int type = LAYER_CONV;
  // shapes (per image): input H,W,C -> conv/pool output OH,OW,OC (-> fused pool PH,PW)
  int H = 0, W = 0, C = 0, OH = 0, OW = 0, OC = 0;
  int kh = 0, kw = 0, sh = 1, sw = 1, pt = 0, pl = 0;
  // conv
  int variant = CONV_GEMM;
  int K = 0, Kpad = 0, Npad = 0, cfg = 0, epi_flags = 0;
  int splits = 1;  // split-K partial count (> 1: GEMM writes partials, a reduce kernel finishes)
  int pool = POOL_NONE;  // a 2x2 max pool fused into this conv
  bool xpad = false;  // explicit pads (dnn_plan_add_conv_padded): shown by dnn_plan_describe
  bool out_padded = false;  // output written zero-bordered (the next layer reads_split_planes / is
                            // patch16 / tile16; fp32 plans: as x3 split planes)
  // The wide x3 conv on two fp16 pieces (gemm_x3_h2.h).  h2_ok is fixed when the layer is added
  // (Switches::x3_h2, host weights all inside fp16's range); h2 (this layer runs the h2 kernel) and
  // out_h2 (its split planes are the next layer's h2 planes) follow from the layer and its
  // neighbour (resolve_h2), never from the batch
  bool h2_ok = false, h2 = false, out_h2 = false;
  size_t pad_off = 0;       // its zero-bordered output region: float offset inside the pad area
  int PH = 0, PW = 0;
  size_t w_off = 0, epi_off = 0;  // float offsets in the weight arena
  bool have_host = false;
  std::vector<float> w, bias, mean, sq, gamma;
  // fork / join: the slot a stash defines, a restore switches to or a route reads as b (-1: none)
  int slot = -1;
  int block = 1, Cb = 0;    // route: space-to-depth block, channels of b
  bool slot_first = false;  // route: b's channels come first
  int to_region = -1;       // a writing layer followed by a stash: the slot region it writes
  int slot_loc = LOC_NONE;  // where the slot's tensor lives when this entry is added (slot numbers are reused)
  int factor = 1;           // upsample
  int first = 0;            // slice: the first channel taken (OC channels from there)
  int leaky = 0;            // shortcut: 0 none, 1 / 2 the conv epilogue's variants
  int n_sizes = 0, sizes[DNN_SPP_MAX_SIZES] = {0, 0, 0};  // spp: the pools' window sizes, in block order
  bool x_first = false;     // spp: the input's copy is the first channel block
  int dst_loc = 0;          // where this layer writes when its output is plain NHWC (LOC_*; layout())
  bool is_conv() const { return type == LAYER_CONV; }
  bool is(int v) const { return type == LAYER_CONV && variant == v; }
  int out_h() const { return pool == POOL_S2 ? PH : OH; }
  int out_w() const { return pool == POOL_S2 ? PW : OW; }
  // the GEMM's rows for n images (pool-window-major rows with a fused stride-2 pool)
  long long rows(long long n) const { return pool == POOL_S2 ? 4 * n * PH * PW : n * OH * OW; }
};

constexpr int kMaxSlots = 4;

struct PlanTap {
  int h, w, c;  // per image
  int region;   // the region that holds it, for good
};

struct PlanSlot {
  int h, w, c;  // per image
  int loc;      // LOC_IN (a stash before any layer) or LOC_REGION + r
  bool live = true;  // false once released: its number is free for the next stash
};

// One kernel launch of a run.  The step list is in launch order: a step's index is its kernel index
// in the ABI (dnn_plan_kernel_info, the timing / mark / clock calls).  Nothing here depends on a
// run's n or pointers.
enum StepKind : int {
  STEP_CVT_IN,           // fp16 plans: the fp32 frames to fp16
  STEP_IM2COL,           // src -> the col buffer
  STEP_CONV,             // the layer's conv (gemm: on the col buffer); split layers leave partials in the slab
  STEP_REDUCE,           // slab partials + epilogue -> dst (split-K without the in-GEMM combine)
  STEP_X3_COMBINE,       // an x3 conv's slab partials + its epilogue -> dst
  STEP_POOL,
  STEP_X3_COMBINE_POOL,  // a pool layer's step that also combines the partials of x3 conv `layer - 1`
  STEP_ROUTE, STEP_SHORTCUT, STEP_UPSAMPLE, STEP_SPP, STEP_SLICE,
  STEP_CVT_OUT           // fp16 plans: the last activation to the fp32 output
};

struct Step {
  std::string name;
  int layer;            // the layer it belongs to (-1: the plan's edge conversions)
  StepKind kind;
  double flops, bytes;  // algorithmic, full planned batch
  int src, dst;         // where it reads the current tensor and writes its output (TensorLoc)
};

// float offsets of the workspace's areas, in this order (layout())
struct WsMap {
  size_t act0 = 0, act1 = 0, col = 0, slab = 0, tickets = 0, pad = 0, regions = 0, zero = 0;
};

struct dnn_plan {
  int batch = 0, in_h = 0, in_w = 0, in_c = 0;
  int cur_h = 0, cur_w = 0, cur_c = 0;
  Switches sw;  // the DNN_HIP_* switches as dnn_plan_create read them: nothing later reads the environment
  int fp16 = 0;  // 1: fp16 activations/weights, fp16 MFMA, fp32 accumulate + epilogue
  bool direct_out = false;  // fp16: the last layer writes the fp32 output itself (fp16_direct_out)
  bool latency = false;  // split K by M too (dnn_plan_set_latency_mode): batch-1 latency plans
  std::vector<PlanLayer> layers;
  std::vector<Step> steps;  // what a run launches, in order (layout())
  // fork / join: slots by number (at most kMaxSlots, a released number is reused); regions (one
  // per stashed layer output unless a free one fits; slots of a restored or re-stashed tensor share
  // one) as per-image floats (the largest tensor a region ever holds), their float offsets inside
  // the slot area
  std::vector<PlanSlot> slots;
  std::vector<PlanTap> taps;  // extra outputs (at most DNN_PLAN_MAX_TAPS): each holds its region for good
  std::vector<size_t> region_elems, region_off;
  // while adding: live slots naming each region, and the first layer index that may write it again
  // (a region with no live slot whose tensor is no longer current; INT_MAX while it is still read)
  std::vector<int> region_refs, region_free_from;
  int cur_src = LOC_IN;  // while adding: where the current tensor lives, -1 = the last layer's output
  size_t slot_floats = 0;
  int device = -1;
  bool finalized = false;
  float* weights = nullptr;
  size_t weight_floats = 0;
  bool own_weights = false;
  float* ws = nullptr;
  size_t ws_floats = 0;
  bool own_ws = false;
  size_t act_floats = 0, col_floats = 0, slab_floats = 0, ticket_floats = 0, pad_floats = 0;
  WsMap at;  // where those areas start
  static constexpr size_t kZeroFloats = 64;  // zero page: source of padding taps (implicit GEMM)
  // staging for dnn_plan_run_host
  float* h_in_dev = nullptr;
  size_t h_in_floats = 0;
  // timing
  bool timing = false;
  int ev_cap = 0, ev_used = 0;
  int timing_only = -1;  // >= 0: events only around that kernel (dnn_plan_timing_begin_only)
  std::vector<hipEvent_t> ev;
  std::vector<int> ev_kernel;
  // shader-clock stamps around one kernel (dnn_plan_clock_begin): run r's stamps of the opening
  // launch at clk_buf + 2 r nwg 4, of the closing launch 4 nwg further (clock.hip)
  int clk_kernel = -1, clk_cap = 0, clk_used = 0, clk_nwg = 0;
  // mark: an event recorded on the run stream right before kernel `mark_kernel` of every run
  // (dnn_plan_set_mark / dnn_plan_wait_mark)
  int mark_kernel = -1;
  hipEvent_t mark_ev = nullptr;
  bool clk_open = false;
  unsigned long long* clk_buf = nullptr;
  // captured forward (dnn_plan_run_graph)
  hipGraph_t graph = nullptr;
  hipGraphExec_t gexec = nullptr;
  int g_n = -1;
  const float* g_in = nullptr;
  float* g_out = nullptr;
};

static void drop_graph(dnn_plan* p) {
  if (p->gexec) (void)hipGraphExecDestroy(p->gexec);
  if (p->graph) (void)hipGraphDestroy(p->graph);
  p->gexec = nullptr;
  p->graph = nullptr;
  p->g_n = -1;
}

// fp16 plans whose last layer is a dense GEMM the fp32-output launcher covers (conv8): it writes
// the plan's fp32 output itself, no output conversion kernel (Switches::f16_direct_out).
static bool fp16_direct_out(const dnn_plan* p) {
  if (!p->fp16 || p->layers.empty() || !p->sw.f16_direct_out) return false;
  const PlanLayer& L = p->layers.back();
  return L.is(CONV_DIRECT_A) && gemm16_f32out_supported(L.splits, L.Npad) && !L.out_padded;
}

// Where each layer writes its plain NHWC output.  Chains keep the ping-pong by layer parity; with
// fork / join entries a layer followed by a stash writes that slot's region, and any other one the
// activation buffer that does not hold its input (the only other live tensors are in slot regions).
// fp16 plans convert their last activation to the output, unless the last layer writes it (direct_out)
static void place_outputs(dnn_plan* p) {
  bool fork = false;
  for (auto& L : p->layers) fork = fork || L.type >= LAYER_STASH;
  int cur = LOC_IN;
  size_t last = p->layers.size();  // the last layer that is not a release writes the output
  while (last > 0 && p->layers[last - 1].type == LAYER_RELEASE) --last;
  if (p->fp16 && !p->direct_out) last = 0;
  for (size_t i = 0; i < p->layers.size(); ++i) {
    PlanLayer& L = p->layers[i];
    if (L.type == LAYER_STASH || L.type == LAYER_RELEASE || L.type == LAYER_TAP) {
      L.dst_loc = cur;
    } else if (L.type == LAYER_RESTORE) {
      L.dst_loc = cur = L.slot_loc;
    } else {
      L.dst_loc = i + 1 == last ? LOC_OUT
                  : !fork                   ? (int)(i & 1)
                  : L.to_region >= 0        ? LOC_REGION + L.to_region
                  : cur == LOC_ACT0         ? LOC_ACT1
                                            : LOC_ACT0;
      cur = L.dst_loc;
    }
  }
}

// Lowers the layers to the step list and sizes the weight arena and the workspace.  The peepholes
// rewrite layers until finalize and dnn_plan_memory / dnn_plan_num_kernels ask before it, so this
// derives everything from the layers each time it is called.
// Which wide x3 layers run on two fp16 pieces (h2): a CONV_X3 layer of the wide kernel's unpooled,
// unsplit form (the batch kernel), whose weights fit fp16's range and whose producer can write h2
// planes -- the whole-image kernel, the wide kernel's unpooled unsplit form or the h2 kernel.  A
// separate pool, the tile kernels and the implicit GEMM write bf16 planes only: their consumers stay
// on x3.  Derived from the layers each time (the peepholes fuse pools into them until finalize).
static void resolve_h2(dnn_plan* p) {
  for (auto& L : p->layers) L.h2 = L.out_h2 = false;
  // (latency plans: their own kernels, x3_lat / x3_ktile, never take h2; a layer that fills the
  // chip runs the batch kernel there too and chooses as in a batch plan)
  if (p->fp16 || !p->sw.x3_h2) return;
  auto wide = [](const PlanLayer& q) {
    return q.is(CONV_X3) && conv_x3_kind(q.OC, q.C) == 0 && q.pool == POOL_NONE && q.splits == 1;
  };
  for (size_t i = 1; i < p->layers.size(); ++i) {
    PlanLayer& L = p->layers[i];
    PlanLayer& q = p->layers[i - 1];
    if (wide(L) && L.h2_ok && q.out_padded && conv_x3_h2_supported(L.C, L.OC, L.H, L.W) &&
        (q.is(CONV_X3_IMG) || wide(q))) {
      L.h2 = true;
      q.out_h2 = true;
    }
  }
}

static void layout(dnn_plan* p) {
  resolve_h2(p);
  p->direct_out = fp16_direct_out(p);
  place_outputs(p);
  size_t off = 0, act = (size_t)p->in_h * p->in_w * p->in_c, col = 0, slab = 0, slab_fused = 0, tickets = 0;
  int nconv = 0, npool = 0, nroute = 0, nshort = 0, nup = 0, nspp = 0, nslice = 0;
  // (kernel names use conv / pool ordinals: "conv7.gemm" is YOLO's conv7)
  p->steps.clear();
  const double B = p->batch;
  const int nl = (int)p->layers.size();
  int cur = LOC_IN;  // where the current tensor lies
  char nm[64];
  auto step = [&](int layer, StepKind kind, double flops, double bytes, int src, int dst) {
    p->steps.push_back(Step{nm, layer, kind, flops, bytes, src, dst});
  };
  // fp16 plans convert at the edges: fp32 frames in (unless conv0 is direct: it reads them), fp32 out
  if (p->fp16 && !(nl && p->layers[0].is(CONV_DIRECT))) {
    snprintf(nm, sizeof(nm), "input.cvt");
    step(-1, STEP_CVT_IN, 0.0, 6.0 * B * p->in_h * p->in_w * p->in_c, LOC_IN, LOC_ACT1);  // (layer 0 writes act0)
    cur = LOC_ACT1;
  }
  for (int i = 0; i < nl; ++i) {
    PlanLayer& L = p->layers[i];
    act = std::max(act, (size_t)L.out_h() * L.out_w() * L.OC);
    const double M = B * L.OH * L.OW;
    const double in_b = 4.0 * B * L.H * L.W * L.C, out_b = 4.0 * B * L.out_h() * L.out_w() * L.OC;
    const int out = L.out_padded ? LOC_PAD + i : L.dst_loc;
    // a stash, a tap (its producer wrote the region, or it is the input), a release and a restore launch nothing
    if (L.type == LAYER_STASH || L.type == LAYER_RELEASE || L.type == LAYER_TAP) continue;
    if (L.type == LAYER_RESTORE) {
      cur = L.dst_loc;
      continue;
    }
    if (L.type == LAYER_CONV) {
      L.w_off = off;
      // fp16 GEMM layers hold Bt in halves (2 per float slot); conv0's direct kernel reads fp32
      const bool half_w = p->fp16 && L.variant != CONV_DIRECT;
      if (weight_pack(L.variant) == PACK_X3)  // three bf16 pieces per weight
        off = align_up(off + (size_t)L.Npad * L.Kpad * 3 / 2, 64);
      else
        off = align_up(off + ((size_t)L.Npad * L.Kpad + (half_w ? 1 : 0)) / (half_w ? 2 : 1), 64);
      L.epi_off = off;
      off = align_up(off + 4 * (size_t)L.Npad, 64);
      const double flops = 2.0 * M * L.OC * L.K, w_b = 4.0 * L.K * L.OC;
      const int src = p->fp16 && L.variant == CONV_DIRECT ? LOC_IN : cur;  // (conv0's direct kernel reads the fp32 frames)
      if (L.variant == CONV_GEMM) {
        col = std::max(col, (size_t)L.OH * L.OW * L.Kpad);
        snprintf(nm, sizeof(nm), "conv%d.im2col", nconv);
        // algorithmic bytes: col written once + input read once
        step(i, STEP_IM2COL, 0.0, 4.0 * M * L.K + in_b, src, LOC_NONE);
        snprintf(nm, sizeof(nm), "conv%d.gemm", nconv);
        step(i, STEP_CONV, flops, 4.0 * M * L.K + w_b + out_b, LOC_NONE, out);
      } else {  // direct_a reads the input as A; the implicit forms read it once per tap in the ideal
        snprintf(nm, sizeof(nm), L.variant == CONV_DIRECT ? "conv%d.direct" : L.variant == CONV_PATCH ? "conv%d.patch"
                                                                                                     : "conv%d.gemm", nconv);
        step(i, STEP_CONV, flops, in_b + w_b + out_b, src, out);
      }
      const double sum_flops = (L.splits - 1) * M * L.OC, sum_bytes = 4.0 * (L.splits + 1) * M * L.OC;
      if (is_x3(L.variant)) {
        if (L.splits > 1) {  // raw partials; combined by the next pool's step, or by a step of its own
          slab = std::max(slab, (size_t)L.splits * L.OH * L.OW * L.OC);
          if (!(i + 1 < nl && p->layers[i + 1].type == LAYER_POOL)) {
            snprintf(nm, sizeof(nm), "conv%d.combine", nconv);
            step(i, STEP_X3_COMBINE, sum_flops, sum_bytes, LOC_NONE, out);
          }
        }
      } else if (L.splits > 1 && p->sw.splitk_fused) {  // partials combined by the GEMM's last-arriving split
        const long long Mg = L.rows(p->batch);
        slab_fused = std::max(slab_fused, (size_t)(p->fp16 ? splitk16_fused_slab_floats(L.cfg, Mg, L.OC, L.splits)
                                                           : splitk_fused_slab_floats(L.cfg, Mg, L.OC, L.splits)));
        tickets = std::max(tickets, (size_t)(p->fp16 ? splitk16_tiles(L.cfg, Mg, L.OC)
                                                     : splitk_tiles(L.cfg, Mg, L.OC)));
        if (p->fp16 && L.cfg == GEMM16_128x512_W16)  // the launcher's 128x128 fallback has more tiles
          tickets = std::max(tickets, (size_t)splitk16_tiles(GEMM16_128x128, (long long)M, L.OC));
      } else if (L.splits > 1) {  // partials written by the GEMM, summed + epilogue by the reduce kernel
        slab = std::max(slab, (size_t)L.splits * L.OH * L.OW * L.OC);
        snprintf(nm, sizeof(nm), "conv%d.reduce", nconv);
        step(i, STEP_REDUCE, sum_flops, sum_bytes, LOC_NONE, out);
      }
      ++nconv;
      if (L.pool == POOL_S2) npool++;
    } else if (L.type == LAYER_POOL) {
      // behind a split x3 conv the pool's kernel sums that conv's partials and applies its epilogue first
      const bool combines = i > 0 && p->layers[i - 1].is_conv() && is_x3(p->layers[i - 1].variant) &&
                            p->layers[i - 1].splits > 1;
      snprintf(nm, sizeof(nm), "pool%d", npool++);
      step(i, combines ? STEP_X3_COMBINE_POOL : STEP_POOL, 0.0, in_b + out_b, cur, out);
    } else if (L.type == LAYER_ROUTE) {  // reads a and b, writes out: input bytes == output bytes
      snprintf(nm, sizeof(nm), "route%d", nroute++);
      step(i, STEP_ROUTE, 0.0, 2.0 * out_b, cur, out);
    } else if (L.type == LAYER_SHORTCUT) {  // one add per output element; reads a and b, writes out
      snprintf(nm, sizeof(nm), "shortcut%d", nshort++);
      step(i, STEP_SHORTCUT, out_b / 4.0, 3.0 * out_b, cur, out);
    } else if (L.type == LAYER_UPSAMPLE) {
      snprintf(nm, sizeof(nm), "upsample%d", nup++);
      step(i, STEP_UPSAMPLE, 0.0, in_b + out_b, cur, out);
    } else if (L.type == LAYER_SPP) {  // reads the input once, writes n_sizes + 1 blocks of its size
      snprintf(nm, sizeof(nm), "spp%d", nspp++);
      step(i, STEP_SPP, 0.0, in_b + out_b, cur, out);
    } else if (L.type == LAYER_SLICE) {  // reads the channels it writes: input bytes == output bytes
      snprintf(nm, sizeof(nm), "slice%d", nslice++);
      step(i, STEP_SLICE, 0.0, 2.0 * out_b, cur, out);
    }
    cur = out;
  }
  if (p->fp16 && !p->direct_out) {
    snprintf(nm, sizeof(nm), "output.cvt");
    step(-1, STEP_CVT_OUT, 0.0, 6.0 * B * p->cur_h * p->cur_w * p->cur_c, cur, LOC_OUT);
  }
  p->weight_floats = align_up(off, 64);
  // activation buffers hold fp16 elements on the fp16 path
  p->act_floats = align_up((act * (size_t)p->batch + (p->fp16 ? 1 : 0)) / (p->fp16 ? 2 : 1), 64);
  p->col_floats = align_up(col * (size_t)p->batch, 64);
  p->slab_floats = align_up(std::max(slab * (size_t)p->batch, slab_fused), 64);
  p->ticket_floats = align_up(tickets, 64);  // unsigned tickets of the fused split-K layers
  // zero-bordered activations feeding patch16 / tile16 (fp16, 2 B per element) / x3 (3 bf16
  // pieces, 6 B) layers: one region per producer (zeroed once at finalize; each producer
  // rewrites only its own interior, so its borders stay zero whatever the layers' shapes).  A
  // region that feeds an h2 layer (two fp16 pieces, 4 B per element) keeps the 6-B size: the
  // planes take its first two thirds and the producer's sticky range word the word after them
  // (range_word), so dnn_plan_memory does not depend on which layers take h2
  size_t pad_total = 0;
  for (auto& L : p->layers)
    if (L.out_padded) {
      const size_t elems = (size_t)p->batch * (L.out_h() + 2) * (L.out_w() + 2) * L.OC;
      L.pad_off = pad_total;
      pad_total += align_up(p->fp16 ? (elems + 1) / 2 : elems * 3 / 2, 64);
    }
  p->pad_floats = pad_total;
  // slot regions: the stashed tensors of the planned batch, after the pad area
  p->region_off.assign(p->region_elems.size(), 0);
  size_t slot_total = 0;
  for (size_t r = 0; r < p->region_elems.size(); ++r) {
    p->region_off[r] = slot_total;
    slot_total += align_up(p->region_elems[r] * (size_t)p->batch, 64);
  }
  p->slot_floats = slot_total;
  // the workspace: two activation buffers, im2col's col, the split-K slab and tickets, the
  // zero-bordered areas, the slot regions, the zero page (source of the implicit GEMM's padding taps)
  WsMap& m = p->at;
  m.act0 = 0;
  m.act1 = m.act0 + p->act_floats;
  m.col = m.act1 + p->act_floats;
  m.slab = m.col + p->col_floats;
  m.tickets = m.slab + p->slab_floats;
  m.pad = m.tickets + p->ticket_floats;
  m.regions = m.pad + p->pad_floats;
  m.zero = m.regions + p->slot_floats;
  p->ws_floats = m.zero + dnn_plan::kZeroFloats;
}

// The sticky range word of a producer of h2 planes: the first word after the planes of the planned
// batch (4 B per element) inside its 6-B-per-element region.  Zeroed with the pad area at finalize;
// no kernel writes there but the producer's wave-uniform slow branch (h2_store8).
static unsigned* range_word(const dnn_plan* p, const PlanLayer& L) {
  const size_t elems = (size_t)p->batch * (L.out_h() + 2) * (L.out_w() + 2) * L.OC;
  return reinterpret_cast<unsigned*>(p->ws + p->at.pad + L.pad_off + elems);
}

// While adding: the layer about to be pushed (index layers.size()) consumes or replaces the current
// tensor.  If that tensor sits in a region no live slot names, the region is free for the
// producers after this layer.
static void current_leaves(dnn_plan* p) {
  const int r = p->cur_src - LOC_REGION;
  if (r >= 0 && p->region_refs[r] == 0) p->region_free_from[r] = (int)p->layers.size() + 1;
}

static bool slot_is_live(const dnn_plan* p, int slot) {
  return slot >= 0 && slot < (int)p->slots.size() && p->slots[slot].live;
}

// While adding: a layer that computes replaces the current tensor with its output
static void push_computing(dnn_plan* p, PlanLayer&& L) {
  current_leaves(p);
  p->cur_h = L.out_h();
  p->cur_w = L.out_w();
  p->cur_c = L.OC;
  p->cur_src = -1;
  p->layers.push_back(std::move(L));
}

extern "C" {

const char* dnn_last_error(void) { return last_error(); }

int dnn_plan_create(int batch, int in_h, int in_w, int in_c, dnn_plan** out) {
  DNN_REQUIRE(out != nullptr, "dnn_plan_create: out is NULL");
  DNN_REQUIRE(batch >= 0 && in_h > 0 && in_w > 0 && in_c > 0, "dnn_plan_create: bad shape %d,%d,%d,%d", batch,
              in_h, in_w, in_c);
  dnn_plan* p = new dnn_plan();
  p->batch = batch;
  p->in_h = p->cur_h = in_h;
  p->in_w = p->cur_w = in_w;
  p->in_c = p->cur_c = in_c;
  p->sw = read_switches();
  *out = p;
  return 0;
}

void dnn_plan_destroy(dnn_plan* p) {
  if (!p) return;
  if (p->device >= 0) (void)hipSetDevice(p->device);
  drop_graph(p);
  for (auto e : p->ev) (void)hipEventDestroy(e);
  if (p->mark_ev) (void)hipEventDestroy(p->mark_ev);
  if (p->own_weights && p->weights) (void)hipFree(p->weights);
  if (p->own_ws && p->ws) (void)hipFree(p->ws);
  if (p->h_in_dev) (void)hipFree(p->h_in_dev);
  delete p;
}

static void set_cfg(dnn_plan* p, PlanLayer& L) {
  const long long M = (long long)p->batch * L.OH * L.OW;
  if (!p->fp16 && is_x3_1x1(L.variant)) {  // one config: 32 x 128 tiles over all of K
    L.cfg = 0;
    L.Kpad = L.K;
    L.Npad = (int)align_up(L.OC, 128);
    L.splits = 1;
    return;
  }
  if (!p->fp16 && is_x3(L.variant)) {  // one config per width (kernels_x3.hip); split-K by (N, K) only
    L.cfg = 0;
    L.Kpad = L.C == 16 ? 160 : L.K;  // (16 channels: 5 steps of two taps)
    L.Npad = L.OC;  // (a multiple of 256, or of 32 / 64 / 128 for the tile kernels)
    L.splits = L.variant == CONV_X3_KTILE ? 1 : L.variant == CONV_X3_LAT ? x3_lat_splits(p->sw, L.OC, L.K) : x3_splits(L.OC, L.K);
    return;
  }
  if (p->fp16 && L.variant == CONV_PATCH16) {  // one config: 192x256 tiles, no split
    L.cfg = 0;
    L.Kpad = L.K;
    L.Npad = (int)align_up(L.OC, 256);
    L.splits = 1;
    return;
  }
  if (p->fp16) {  // fp16 MFMA configs: BK = 64 halves, split rule on (N, K) only
    L.cfg = choose_gemm16_cfg(M, L.OC, L.K);
    L.Kpad = (int)align_up(L.K, 64);
    L.Npad = (int)align_up(L.OC, gemm16_cfg_bn(L.cfg));
    L.splits = (L.Kpad == L.K) ? choose_splitk16(L.OC, L.K) : 1;
    return;
  }
  L.cfg = L.variant == CONV_IMPLICIT ? choose_gemm_cfg_implicit(M, L.OC, L.K) : choose_gemm_cfg(M, L.OC, L.K);
  for (const auto& [k, c] : p->sw.cfg)  // tuning experiments
    if (k == L.K && c >= GEMM_128x128_K32 && c < GEMM_NUM_CFGS && c != GEMM_G64x32_K32) L.cfg = c;
  L.Kpad = (int)align_up(L.K, gemm_cfg_bk(L.cfg));
  L.Npad = (int)align_up(L.OC, gemm_cfg_bn(L.cfg));
  L.splits = (L.cfg >= GEMM_128x128_K32 && L.Kpad == L.K) ? choose_splitk(L.OC, L.K, p->sw.splitk_fused) : 1;
  // one fp32 chain of K / 2 MFMAs misses the 2e-6 per-layer bar from K of about 4608 on (measured
  // 2.1e-6 .. 4.6e-6 at K = 4608 .. 9216, 2.7e-6 at 6125: DESIGN.md §2).  Long-K layers the
  // (N, K) rule leaves whole (N < 512; the explicit GEMM's zero-padded K too) are summed in three
  // or two parts like conv5-conv7: still a function of (N, K) and the config alone
  if (L.splits == 1 && L.cfg >= GEMM_128x128_K32 && L.K >= 4608 && (p->sw.splitk_fused || L.OC % 4 == 0)) {
    const int nk = L.Kpad / 32;
    L.splits = nk % 3 == 0 ? 3 : nk % 2 == 0 ? 2 : 1;
  }
  if (p->latency && p->sw.splitk_fused && L.Kpad == L.K) {
    // a tile config and split for this M when the batch rule leaves the chip idle
    int cfg = L.cfg, sp = L.splits;
    choose_latency_plan(M, L.OC, L.K, &cfg, &sp, false);
    for (const auto& [k, v] : p->sw.split)  // tuning experiments
      if (k == L.K && v >= 1 && v <= 32 && (L.Kpad / gemm_cfg_bk(cfg)) % v == 0 && cfg >= GEMM_128x128_K32) sp = v;
    L.cfg = cfg;
    L.splits = sp;
    L.Npad = (int)align_up(L.OC, gemm_cfg_bn(L.cfg));
  }
}

int dnn_plan_set_precision(dnn_plan* p, int precision) {
  DNN_REQUIRE(p && !p->finalized && p->layers.empty(), "dnn_plan_set_precision: call before adding layers");
  DNN_REQUIRE(precision == 0 || precision == 1, "dnn_plan_set_precision: precision must be 0 (fp32) or 1 (fp16)");
  p->fp16 = precision;
  return 0;
}

int dnn_plan_set_latency_mode(dnn_plan* p, int on) {
  DNN_REQUIRE(p && !p->finalized && p->layers.empty(), "dnn_plan_set_latency_mode: call before adding layers");
  DNN_REQUIRE(on == 0 || on == 1, "dnn_plan_set_latency_mode: on must be 0 or 1");
  DNN_REQUIRE(!on || !p->fp16, "dnn_plan_set_latency_mode: fp32 plans only");
  p->latency = on != 0;
  return 0;
}

}  // extern "C"

// What a conv entry's epilogue is made of: dnn_plan_add_conv's BiasAdd / BatchNorm, or
// dnn_plan_add_conv_padded's per-channel scale / shift (EPI_BN_AB with alpha = scale, beta = -shift)
struct ConvEpilogueSpec {
  const float *biases = nullptr, *mean = nullptr, *var = nullptr, *gamma = nullptr;
  float eps = 0.f;
  const float *scale = nullptr, *shift = nullptr;
  int leaky = 0;
};

// fp16 plans: producers that can write their output zero-bordered (what patch16 / tile16 / img16
// read): a separate pool, a patch16 or tile16 conv, or the pooled conv1 patch kernel
static bool can_write_zero_bordered16(const PlanLayer& q) {
  return q.type == LAYER_POOL || q.is(CONV_PATCH16) || (q.is_conv() && is_tile16(q.variant)) ||
         (q.is(CONV_PATCH) && q.pool == POOL_S2);
}

// fp32 plans: producers that can write the x3 convs' split planes: a separate pool, another x3
// conv, a pool-fused implicit GEMM without split-K (its epilogue splits, EPI_OUT_X3) or the
// pool-fused patch conv (conv1)
static bool can_write_split_planes(const PlanLayer& q) {
  return q.type == LAYER_POOL || (q.is_conv() && is_x3(q.variant)) ||
         (q.is(CONV_IMPLICIT) && q.pool == POOL_S2 && q.splits == 1) || (q.is(CONV_PATCH) && q.pool == POOL_S2);
}

// The body both conv entries share: variant selection, config, epilogue parameters.  The caller has
// checked its arguments and worked out the geometry (OH, OW and the front pads pt, pl);
// `xpad`: the pads were given explicitly (dnn_plan_add_conv_padded), for dnn_plan_describe.
static int add_conv_layer(dnn_plan* p, int kh, int kw, int od, int stride_h, int stride_w, int OH, int pt, int OW,
                          int pl, bool xpad, const float* kernel, const ConvEpilogueSpec& ep) {
  const float *biases = ep.biases, *mean = ep.mean, *var = ep.var, *gamma = ep.gamma;
  const float eps = ep.eps;
  const int leaky = ep.leaky;
  PlanLayer L;
  L.type = LAYER_CONV;
  L.H = p->cur_h;
  L.W = p->cur_w;
  L.C = p->cur_c;
  L.kh = kh;
  L.kw = kw;
  L.sh = stride_h;
  L.sw = stride_w;
  L.OH = OH;
  L.OW = OW;
  L.pt = pt;
  L.pl = pl;
  L.xpad = xpad;
  L.OC = od;
  L.K = kh * kw * L.C;
  const bool one_by_one = kh == 1 && kw == 1 && stride_h == 1 && stride_w == 1 && L.pt == 0 && L.pl == 0 &&
                          L.OH == L.H && L.OW == L.W && L.C % (p->fp16 ? 8 : 32) == 0;
  if (p->fp16) {
    // fp16 path: 1x1 on the input, implicit GEMM (C % 8 == 0), or conv0's direct kernel (set
    // when its 2x2/s2 pool arrives); anything else is rejected at finalize
    L.variant = one_by_one ? CONV_DIRECT_A : (L.C % 8 == 0 && kh * kw <= 30) ? CONV_IMPLICIT : CONV_GEMM;
    // 3x3 wide layers whose producer (a separate pool or another such conv) can write a
    // zero-bordered output: the patch kernel (input staged once per 64-channel chunk)
    if (L.variant == CONV_IMPLICIT && !p->layers.empty() &&
        conv_patch16_supported(p->sw, L.C, od, L.H, L.W, L.OH, L.OW, kh, kw, stride_h, stride_w, L.pt, L.pl)) {
      PlanLayer& prev = p->layers.back();
      if (can_write_zero_bordered16(prev) && !prev.is(CONV_PATCH)) {  // (not behind the conv1 patch kernel)
        L.variant = CONV_PATCH16;
        prev.out_padded = true;
      }
    }
  } else if (one_by_one)
    L.variant = CONV_DIRECT_A;
  else if (p->sw.fuse && implicit_conv_supported(L.C, kh, kw) &&
           choose_gemm_cfg_implicit((long long)p->batch * L.OH * L.OW, od, L.K) >= 0)
    L.variant = CONV_IMPLICIT;
  else
    L.variant = CONV_GEMM;  // may become CONV_DIRECT when a 2x2/s2 pool follows (conv0)
  // fp32 3x3 wide layers fed by a separate pool or another such conv: the x3 conv (its producer
  // writes the split planes).  Batch plans choose it by the layer alone, so a batch-1 plan and a
  // batch-64 plan run the same arithmetic.  Latency plans (with the in-GEMM split-K combine) take
  // the batch kernel only where its tiles fill half the chip (at batch 1 a 176 x 256 tile's
  // one-chunk K slice alone takes ~26 us), elsewhere the small-M x3 kernel (gemm_x3_lat.h: 64
  // columns x one or two chunks per workgroup, 8 waves splitting rows / columns / chunks;
  // conv6 / conv7 of a one-frame plan) when it makes at least two K slices
  bool x3_cand = false, x3_lat = false, x3_k = false;
  if (!p->fp16 && L.variant == CONV_IMPLICIT && !p->layers.empty()) {
    const bool batch_ok = conv_x3_supported(p->sw, L.C, od, L.H, L.W, L.OH, L.OW, kh, kw, stride_h, stride_w, L.pt, L.pl);
    // (the narrow kernels take small tiles in latency plans: batch_ok is enough.  conv1 at one
    // frame: the 16-channel kernel's 4 x 26 tiles 10.6 us, its 16 x 26 ones 11.7, the fp32 patch
    // conv 13.8 (HIP events, same box))
    const int xk = conv_x3_kind(od, L.C);
    const bool lat = p->latency && p->sw.splitk_fused;
    // latency plans: conv3-conv5 of a frame with the K split inside the workgroup (one launch, no
    // partials), first; conv1 / conv2 on the narrow kernels' small tiles; conv6 / conv7 on the
    // small-M kernel's K slices + combine
    const bool fills = batch_ok && x3_tiles(p->batch, L.OH, L.OW, od, L.C, L.K) >= 128;  // the batch tiles fill the chip
    x3_k = lat && !fills &&
           conv_x3_ktile_supported(p->sw, p->batch, L.C, od, L.H, L.W, L.OH, L.OW, kh, kw, stride_h, stride_w, L.pt, L.pl, 0);
    if (x3_k) {
      x3_cand = true;
    } else if (lat && !(batch_ok && (xk > 0 || x3_tiles(p->batch, L.OH, L.OW, od, L.C, L.K) >= 128))) {
      x3_lat = conv_x3_lat_supported(p->sw, p->batch, L.C, od, L.H, L.W, L.OH, L.OW, kh, kw, stride_h, stride_w, L.pt,
                                     L.pl) &&
               x3_lat_splits(p->sw, od, L.K) >= 2;
      x3_cand = x3_lat;
    } else {
      x3_cand = batch_ok;
    }
  }
  // fp32 1x1 layers right after an x3 conv (conv8 after conv7): the 1x1 x3 conv on the split
  // planes that producer writes instead of its fp32 output.  Chosen by the layer alone (batch
  // plans of any size run the same arithmetic).  Latency plans keep the fp32 GEMM split over the
  // chip where this kernel's 32 x 128 tiles would not fill it (one frame's 169 rows are 6 tiles:
  // 21 us against 14)
  // (latency plans whose frame leaves those tiles few: the K-split 1x1 form, 16 x 32 tiles)
  const long long t1x1 = ((long long)p->batch * L.OH * L.OW + 31) / 32 * ((od + 127) / 128);
  const bool lat1x1 = p->latency && p->sw.splitk_fused && t1x1 < 256;
  if (!p->fp16 && L.variant == CONV_DIRECT_A && !p->layers.empty() && p->layers.back().is_conv() &&
      is_x3(p->layers.back().variant) &&
      (lat1x1 ? conv_x3_1x1_ktile_supported(p->sw, L.C, od, L.H, L.W) : conv_x3_1x1_supported(p->sw, L.C, od, L.H, L.W))) {
    L.variant = lat1x1 ? CONV_X3_1X1_KTILE : CONV_X3_1X1;
    p->layers.back().out_padded = true;
  }
  if (x3_cand) {
    PlanLayer& prev = p->layers.back();
    if (L.C == 16) {  // the 16-channel x3 kernel reads the producer's fp32 output (conv1)
      L.variant = CONV_X3;
    } else if (can_write_split_planes(prev) && (prev.type != LAYER_POOL || prev.C % 32 == 0)) {
      L.variant = x3_k ? CONV_X3_KTILE : x3_lat ? CONV_X3_LAT : CONV_X3;
      prev.out_padded = true;
    }
  }
  set_cfg(p, L);
  L.epi_flags = (biases ? EPI_BIAS : 0) | (mean ? EPI_BN : 0) |
                (leaky == 1 ? EPI_LEAKY_F64 : leaky == 2 ? EPI_LEAKY_F32 : 0);
  // fp16 plans (tolerance, not bit parity): BiasAdd + BatchNorm folded into v * alpha - beta
  // (alpha = gamma / sqrt(var + eps), beta = (mean - bias) * alpha) and the leaky as
  // max(v, 0.1f v): 4 VALU per output instead of ~30 for the reference's exact division and
  // double-rounded leaky (the VALU-bound small-channel kernels run on the epilogue)
  const bool fold16 = p->fp16 && mean;
  if (fold16)
    L.epi_flags = EPI_BN_AB | ((L.epi_flags & (EPI_LEAKY_F64 | EPI_LEAKY_F32)) ? EPI_LEAKY_F32 : 0);
  // the affine entry (fp32 plans): v * scale + shift as EPI_BN_AB's v * alpha - beta with
  // beta = -shift (the negation is exact, so both round alike)
  if (ep.scale) L.epi_flags |= EPI_BN_AB;
  // (a shape-only layer, kernel == NULL, takes the choice of in-range weights: its arena comes
  // from a plan that checked them)
  L.h2_ok = p->sw.x3_h2 && L.variant == CONV_X3;
  if (kernel) {
    L.have_host = true;
    L.w.assign(kernel, kernel + (size_t)L.K * od);
    if (L.h2_ok)  // h2's range contract: every weight finite and |w| < 65520
      for (float w : L.w) L.h2_ok = L.h2_ok && std::fabs(w) < 65520.f;  // (false for NaN)
    const int np = std::max(L.Npad, 32);
    L.bias.assign(np, 0.f);
    L.mean.assign(np, 0.f);
    L.sq.assign(np, 1.f);
    L.gamma.assign(np, 1.f);
    for (int d = 0; d < od; ++d) {
      if (biases) L.bias[d] = biases[d];
      if (mean) {
        L.mean[d] = mean[d];
        // sqrt(variance + epsilon) in fp32 as the reference (dnn_openblas.c:48-50; dnn.py:325-327)
        volatile float s = var[d] + eps;
        L.sq[d] = sqrtf(s);
        L.gamma[d] = gamma[d];
      }
      if (fold16) {  // EPI_BN_AB: mean slot = alpha, sq slot = beta
        const float alpha = L.gamma[d] / L.sq[d];
        const float beta = (L.mean[d] - (biases ? biases[d] : 0.f)) * alpha;
        L.mean[d] = alpha;
        L.sq[d] = beta;
        L.bias[d] = 0.f;
        L.gamma[d] = 1.f;
      }
      if (ep.scale) {  // EPI_BN_AB: mean slot = alpha, sq slot = beta
        L.mean[d] = ep.scale[d];
        L.sq[d] = -ep.shift[d];
      }
    }
  }
  push_computing(p, std::move(L));
  return 0;
}

extern "C" {

int dnn_plan_add_conv(dnn_plan* p, int kh, int kw, int od, int stride_h, int stride_w, int padding,
                      const float* kernel, const float* biases, const float* mean, const float* var,
                      const float* gamma, float eps, int leaky) {
  DNN_REQUIRE(p && !p->finalized, "dnn_plan_add_conv: plan is NULL or finalized");
  DNN_REQUIRE(kh > 0 && kw > 0 && od > 0 && stride_h > 0 && stride_w > 0, "dnn_plan_add_conv: bad args");
  DNN_REQUIRE((mean == nullptr) == (var == nullptr) && (var == nullptr) == (gamma == nullptr),
              "dnn_plan_add_conv: mean/var/gamma must be all set or all NULL");
  DNN_REQUIRE(leaky >= 0 && leaky <= 2, "dnn_plan_add_conv: leaky must be 0, 1 or 2");
  int OH, OW, pt, pl;
  out_pads(p->cur_h, kh, stride_h, padding, &OH, &pt);
  out_pads(p->cur_w, kw, stride_w, padding, &OW, &pl);
  DNN_REQUIRE(OH > 0 && OW > 0, "dnn_plan_add_conv: empty output (%dx%d input, %dx%d kernel)", p->cur_h, p->cur_w, kh,
              kw);
  ConvEpilogueSpec ep;
  ep.biases = biases;
  ep.mean = mean;
  ep.var = var;
  ep.gamma = gamma;
  ep.eps = eps;
  ep.leaky = leaky;
  return add_conv_layer(p, kh, kw, od, stride_h, stride_w, OH, pt, OW, pl, false, kernel, ep);
}

int dnn_plan_add_conv_padded(dnn_plan* p, int kh, int kw, int od, int stride_h, int stride_w, int pad_h, int pad_w,
                             const float* kernel, const float* scale, const float* shift, int leaky) {
  DNN_REQUIRE(p && !p->finalized, "dnn_plan_add_conv_padded: plan is NULL or finalized");
  DNN_REQUIRE(!p->fp16, "dnn_plan_add_conv_padded: fp32 plans only (this is an fp16 plan)");
  DNN_REQUIRE(kh > 0 && kw > 0 && od > 0 && stride_h > 0 && stride_w > 0, "dnn_plan_add_conv_padded: bad args");
  DNN_REQUIRE(pad_h >= 0 && pad_h < kh && pad_w >= 0 && pad_w < kw,
              "dnn_plan_add_conv_padded: pads %d,%d outside [0, kernel) for a %dx%d kernel", pad_h, pad_w, kh, kw);
  DNN_REQUIRE((scale == nullptr) == (shift == nullptr),
              "dnn_plan_add_conv_padded: scale and shift must be both set or both NULL");
  DNN_REQUIRE(leaky >= 0 && leaky <= 2, "dnn_plan_add_conv_padded: leaky must be 0, 1 or 2");
  const int span_h = p->cur_h + 2 * pad_h - kh, span_w = p->cur_w + 2 * pad_w - kw;
  DNN_REQUIRE(span_h >= 0 && span_w >= 0, "dnn_plan_add_conv_padded: empty output (%dx%d input, %dx%d kernel, pads %d,%d)",
              p->cur_h, p->cur_w, kh, kw, pad_h, pad_w);
  ConvEpilogueSpec ep;
  ep.scale = scale;
  ep.shift = shift;
  ep.leaky = leaky;
  return add_conv_layer(p, kh, kw, od, stride_h, stride_w, span_h / stride_h + 1, pad_h, span_w / stride_w + 1, pad_w,
                        true, kernel, ep);
}

int dnn_plan_add_max_pool(dnn_plan* p, int kh, int kw, int stride_h, int stride_w, int padding) {
  DNN_REQUIRE(p && !p->finalized, "dnn_plan_add_max_pool: plan is NULL or finalized");
  DNN_REQUIRE(kh > 0 && kw > 0 && stride_h > 0 && stride_w > 0, "dnn_plan_add_max_pool: bad args");
  PlanLayer L;
  L.type = LAYER_POOL;
  L.H = p->cur_h;
  L.W = p->cur_w;
  L.C = L.OC = p->cur_c;
  L.kh = kh;
  L.kw = kw;
  L.sh = stride_h;
  L.sw = stride_w;
  out_pads(L.H, kh, stride_h, padding, &L.OH, &L.pt);
  out_pads(L.W, kw, stride_w, padding, &L.OW, &L.pl);
  DNN_REQUIRE(L.OH > 0 && L.OW > 0, "dnn_plan_add_max_pool: empty output");
  // fuse a 2x2/stride-2 pool (front pads are 0 for both SAME and VALID) into the conv before it
  if (p->sw.fuse && !p->layers.empty() && kh == 2 && kw == 2 && stride_h == 2 && stride_w == 2 && L.pt == 0 &&
      L.pl == 0) {
    PlanLayer& prev = p->layers.back();
    // (latency plans: a split implicit conv keeps its split, the combine pools)
    if (prev.is_conv() && !prev.pool &&
        (prev.splits == 1 ||
         (prev.variant == CONV_IMPLICIT && !p->fp16 && p->sw.splitk_fused && generic_combine_cfg(prev.cfg)))) {
      bool ok = false;
      if (prev.variant == CONV_IMPLICIT) {
        ok = true;
        if (!p->fp16 && p->sw.patch && prev.splits == 1 && patch_conv_pool_supported(prev.C, prev.OC, prev.H, prev.W, prev.OH, prev.OW, prev.kh, prev.kw,
                                                  prev.sh, prev.sw, prev.pt, prev.pl) &&
            prev.Kpad == patch_conv_kpad(prev.C))
          prev.variant = CONV_PATCH;  // same packed weights (Bt[Npad][Kpad]) as the implicit GEMM
        if (p->fp16 && p->sw.patch &&
            conv1_patch_f16_supported(prev.C, prev.OC, prev.H, prev.W, prev.OH, prev.OW, prev.kh, prev.kw, prev.sh,
                                      prev.sw, prev.pt, prev.pl))
          prev.variant = CONV_PATCH;  // fp16 patch kernel on the same fp16 Bt
        // fp16 3x3 layers whose producer can write a zero-bordered output (a separate pool, the
        // conv1 patch kernel, another tile or patch16 conv): the 2-D tile kernel (its weights
        // packed in order 5 into the same Npad x Kpad slot)
        if (p->fp16 && prev.variant == CONV_IMPLICIT && prev.splits == 1 && p->layers.size() >= 2 &&
            conv_tile16_supported(p->sw, prev.C, prev.OC, prev.H, prev.W, prev.OH, prev.OW, prev.kh, prev.kw, prev.sh,
                                  prev.sw, prev.pt, prev.pl) &&
            prev.Kpad % 32 == 0) {
          PlanLayer& q = p->layers[p->layers.size() - 2];
          if (can_write_zero_bordered16(q)) {
            prev.variant = CONV_TILE16;
            q.out_padded = true;
          }
        }
      } else if (p->fp16 && prev.variant == CONV_PATCH16 &&
                 conv_tile16_supported(p->sw, prev.C, prev.OC, prev.H, prev.W, prev.OH, prev.OW, prev.kh, prev.kw, prev.sh,
                                       prev.sw, prev.pt, prev.pl)) {
        prev.variant = CONV_TILE16;  // (its producer already writes the zero-bordered input) the pool fused
        ok = true;
      } else if (prev.variant == CONV_GEMM && prev.pt == prev.pl && prev.pt <= 1 &&  // (VALID's or SAME's pads: the
                 // direct kernels are checked with no others; other explicit pads keep the GEMM)
                 direct_conv_pool_supported(prev.C, prev.OC, prev.kh, prev.kw, prev.sh, prev.sw)) {
        prev.variant = CONV_DIRECT;
        ok = true;
      } else if (is_x3(prev.variant) && !p->fp16 &&
                 (prev.variant == CONV_X3_KTILE ? conv_x3_ktile_supported(p->sw, p->batch, prev.C, prev.OC, prev.H, prev.W, prev.OH, prev.OW,
                                                     prev.kh, prev.kw, prev.sh, prev.sw, prev.pt, prev.pl, 1)
                           : conv_x3_pool_supported(prev.OC, prev.C, prev.H, prev.W))) {
        ok = true;  // pool-window-major rows, pooled before the epilogue in the x3 kernel
      }
      if (ok) {
        prev.pool = POOL_S2;
        prev.PH = L.OH;
        prev.PW = L.OW;
        p->cur_h = L.OH;
        p->cur_w = L.OW;
        return 0;
      }
    }
  }
  // a 2x2/stride-1 SAME pool (YOLO's pool5) into a single-frame x3_ktile conv before it: the conv
  // computes the row below each tile too and pools before its epilogue
  if (p->sw.fuse && !p->layers.empty() && kh == 2 && kw == 2 && stride_h == 1 && stride_w == 1 && L.pt == 0 &&
      L.pl == 0 && L.OH == L.H && L.OW == L.W) {
    PlanLayer& prev = p->layers.back();
    if (prev.is(CONV_X3_KTILE) && !prev.pool &&
        conv_x3_ktile_supported(p->sw, p->batch, prev.C, prev.OC, prev.H, prev.W, prev.OH, prev.OW, prev.kh, prev.kw,
                                prev.sh, prev.sw, prev.pt, prev.pl, 2)) {
      prev.pool = POOL_S1;
      return 0;
    }
    // ... into an fp16 conv of a 13 x 13 frame fed by a zero-bordered producer (conv5 + pool5 of
    // the fp16 path): the tile kernel's whole-frame form, pool taken from its fp16 stage
    if (p->fp16 && (prev.is(CONV_IMPLICIT) || prev.is(CONV_PATCH16)) && !prev.pool && p->layers.size() >= 2 &&
        prev.kh == 3 && prev.kw == 3 && prev.sh == 1 && prev.sw == 1 && prev.pt == 1 && prev.pl == 1 &&
        prev.OH == prev.H && prev.OW == prev.W && prev.Kpad % 32 == 0 &&
        conv_img16_supported(p->sw, prev.C, prev.OC, prev.H, prev.W)) {
      PlanLayer& q = p->layers[p->layers.size() - 2];
      if (can_write_zero_bordered16(q)) {
        prev.variant = CONV_IMG16;
        prev.pool = POOL_S1;
        prev.splits = 1;
        q.out_padded = true;
        return 0;
      }
    }
    // ... into a batch-tile x3 conv of a small frame (conv5 + pool5): whole-image tiles over all
    // of K (gemm_x3_img.h) instead of K slices whose partials the pool combines
    if (prev.is(CONV_X3) && !prev.pool && prev.C != 16 && conv_x3_img_supported(p->sw, prev.C, prev.OC, prev.H, prev.W)) {
      prev.variant = CONV_X3_IMG;
      prev.pool = POOL_S1;
      prev.splits = 1;
      return 0;
    }
  }
  push_computing(p, std::move(L));
  return 0;
}

static void shape_only_layer(const dnn_plan* p, PlanLayer* L, int type) {
  L->type = type;
  L->H = L->OH = p->cur_h;
  L->W = L->OW = p->cur_w;
  L->C = L->OC = p->cur_c;
}

static void current_into_region(dnn_plan* p);

int dnn_plan_add_stash(dnn_plan* p, int* slot) {
  DNN_REQUIRE(p && !p->finalized, "dnn_plan_add_stash: plan is NULL or finalized");
  DNN_REQUIRE(slot != nullptr, "dnn_plan_add_stash: slot is NULL");
  DNN_REQUIRE(!p->fp16, "dnn_plan_add_stash: fp32 plans only (this is an fp16 plan)");
  int number = 0;  // the lowest free slot number
  while (number < (int)p->slots.size() && p->slots[number].live) ++number;
  DNN_REQUIRE(number < kMaxSlots, "dnn_plan_add_stash: all %d slots are in use", kMaxSlots);
  current_into_region(p);
  if (p->cur_src >= LOC_REGION) p->region_refs[p->cur_src - LOC_REGION]++;
  PlanLayer L;
  shape_only_layer(p, &L, LAYER_STASH);
  L.slot = number;
  L.slot_loc = p->cur_src;
  const PlanSlot S{p->cur_h, p->cur_w, p->cur_c, p->cur_src, true};
  if (number == (int)p->slots.size())
    p->slots.push_back(S);
  else
    p->slots[number] = S;
  p->layers.push_back(std::move(L));
  *slot = number;
  return 0;
}

int dnn_plan_add_tap(dnn_plan* p, int* index) {
  DNN_REQUIRE(p && !p->finalized, "dnn_plan_add_tap: plan is NULL or finalized");
  DNN_REQUIRE(index != nullptr, "dnn_plan_add_tap: index is NULL");
  DNN_REQUIRE(!p->fp16, "dnn_plan_add_tap: fp32 plans only (this is an fp16 plan)");
  DNN_REQUIRE(p->cur_src != LOC_IN, "dnn_plan_add_tap: no layer has run yet (the current tensor is the plan's input)");
  DNN_REQUIRE((int)p->taps.size() < DNN_PLAN_MAX_TAPS, "dnn_plan_add_tap: all %d taps are in use",
              DNN_PLAN_MAX_TAPS);
  current_into_region(p);
  const int r = p->cur_src - LOC_REGION;
  p->region_refs[r]++;  // never dropped: the region is no later producer's
  PlanLayer L;
  shape_only_layer(p, &L, LAYER_TAP);
  L.slot = (int)p->taps.size();  // (the tap's index)
  L.slot_loc = p->cur_src;
  p->taps.push_back(PlanTap{p->cur_h, p->cur_w, p->cur_c, r});
  p->layers.push_back(std::move(L));
  *index = (int)p->taps.size() - 1;
  return 0;
}

int dnn_plan_num_taps(const dnn_plan* p) { return p ? (int)p->taps.size() : -2; }

int dnn_plan_tap_shape(const dnn_plan* p, int index, int* h, int* w, int* c) {
  DNN_REQUIRE(p, "dnn_plan_tap_shape: plan is NULL");
  DNN_REQUIRE(index >= 0 && index < (int)p->taps.size(), "dnn_plan_tap_shape: tap %d of %d", index,
              (int)p->taps.size());
  const PlanTap& T = p->taps[index];
  if (h) *h = T.h;
  if (w) *w = T.w;
  if (c) *c = T.c;
  return 0;
}

int dnn_plan_tap_buffer(const dnn_plan* p, int index, void** ptr, size_t* bytes) {
  DNN_REQUIRE(p && p->finalized, "dnn_plan_tap_buffer: plan not finalized");
  DNN_REQUIRE(index >= 0 && index < (int)p->taps.size(), "dnn_plan_tap_buffer: tap %d of %d", index,
              (int)p->taps.size());
  const PlanTap& T = p->taps[index];
  if (ptr) *ptr = p->ws + p->at.regions + p->region_off[T.region];
  if (bytes) *bytes = (size_t)p->batch * T.h * T.w * T.c * sizeof(float);
  return 0;
}

int dnn_plan_tap_read_host(const dnn_plan* p, int index, int n, float* h_out) {
  void* ptr = nullptr;
  int rc = dnn_plan_tap_buffer(p, index, &ptr, nullptr);
  if (rc) return rc;
  DNN_REQUIRE(n >= 0 && n <= p->batch && (n == 0 || h_out), "dnn_plan_tap_read_host: n=%d outside [0, %d] or NULL output",
              n, p->batch);
  if (n == 0) return 0;
  const PlanTap& T = p->taps[index];
  DNN_HIP_TRY(hipSetDevice(p->device));
  DNN_HIP_TRY(hipMemcpy(h_out, ptr, (size_t)n * T.h * T.w * T.c * sizeof(float), hipMemcpyDeviceToHost));
  return 0;
}

// While adding: the current tensor is about to be named by a slot or a tap.  If it is the last
// computing layer's output, that layer is made to write a region, and the tensor then sits there.
static void current_into_region(dnn_plan* p) {
  if (p->cur_src < 0) {  // the last computing layer's output: that layer writes a slot region
    int producer = (int)p->layers.size() - 1;  // (only release entries can follow it)
    while (p->layers[producer].type == LAYER_RELEASE) --producer;
    const size_t elems = (size_t)p->cur_h * p->cur_w * p->cur_c;
    // a region freed before the producer was added: the smallest one that is large enough, else
    // the largest one (it grows), else a new one
    int r = -1;
    for (int k = 0; k < (int)p->region_elems.size(); ++k) {
      if (p->region_refs[k] != 0 || p->region_free_from[k] > producer) continue;
      const size_t have = p->region_elems[k];
      if (r < 0) {
        r = k;
        continue;
      }
      const size_t best = p->region_elems[r];
      if (best >= elems ? (have >= elems && have < best) : have > best) r = k;
    }
    if (r < 0) {
      r = (int)p->region_elems.size();
      p->region_elems.push_back(elems);
      p->region_refs.push_back(0);
      p->region_free_from.push_back(INT_MAX);
    } else {
      p->region_elems[r] = std::max(p->region_elems[r], elems);
      p->region_free_from[r] = INT_MAX;
    }
    p->layers[producer].to_region = r;
    p->cur_src = LOC_REGION + r;
  }  // (else the plan's input, or a tensor that already sits in a region)
}

int dnn_plan_add_release(dnn_plan* p, int slot) {
  DNN_REQUIRE(p && !p->finalized, "dnn_plan_add_release: plan is NULL or finalized");
  DNN_REQUIRE(!p->fp16, "dnn_plan_add_release: fp32 plans only (this is an fp16 plan)");
  DNN_REQUIRE(slot_is_live(p, slot), "dnn_plan_add_release: slot %d is unknown or already released", slot);
  PlanSlot& S = p->slots[slot];
  S.live = false;
  const int r = S.loc - LOC_REGION;
  // its region is free for the producers after this entry, unless the current tensor still sits in
  // it: then from the layer that consumes it on (current_leaves)
  if (r >= 0 && --p->region_refs[r] == 0)
    p->region_free_from[r] = p->cur_src == S.loc ? INT_MAX : (int)p->layers.size() + 1;
  PlanLayer L;
  L.type = LAYER_RELEASE;
  L.H = L.OH = S.h;
  L.W = L.OW = S.w;
  L.C = L.OC = S.c;
  L.slot = slot;
  L.slot_loc = S.loc;
  p->layers.push_back(std::move(L));
  return 0;
}

int dnn_plan_add_restore(dnn_plan* p, int slot) {
  DNN_REQUIRE(p && !p->finalized, "dnn_plan_add_restore: plan is NULL or finalized");
  DNN_REQUIRE(!p->fp16, "dnn_plan_add_restore: fp32 plans only (this is an fp16 plan)");
  DNN_REQUIRE(slot_is_live(p, slot), "dnn_plan_add_restore: unknown or released slot %d (%d defined)", slot,
              (int)p->slots.size());
  const PlanSlot& S = p->slots[slot];
  current_leaves(p);
  p->cur_h = S.h;
  p->cur_w = S.w;
  p->cur_c = S.c;
  p->cur_src = S.loc;
  PlanLayer L;
  shape_only_layer(p, &L, LAYER_RESTORE);
  L.slot = slot;
  L.slot_loc = S.loc;
  p->layers.push_back(std::move(L));
  return 0;
}

int dnn_plan_add_route(dnn_plan* p, int block, int slot, int slot_first) {
  DNN_REQUIRE(p && !p->finalized, "dnn_plan_add_route: plan is NULL or finalized");
  DNN_REQUIRE(!p->fp16, "dnn_plan_add_route: fp32 plans only (this is an fp16 plan)");
  DNN_REQUIRE(block >= 1 && block <= 8, "dnn_plan_add_route: block %d outside 1..8", block);
  DNN_REQUIRE(slot == -1 || slot_is_live(p, slot), "dnn_plan_add_route: unknown or released slot %d (%d defined)",
              slot, (int)p->slots.size());
  DNN_REQUIRE(p->cur_h % block == 0 && p->cur_w % block == 0,
              "dnn_plan_add_route: %dx%d input is not a multiple of block %d", p->cur_h, p->cur_w, block);
  PlanLayer L;
  L.type = LAYER_ROUTE;
  L.H = p->cur_h;
  L.W = p->cur_w;
  L.C = p->cur_c;
  L.OH = L.H / block;
  L.OW = L.W / block;
  L.block = block;
  L.slot = slot;
  L.slot_first = slot >= 0 && slot_first != 0;
  if (slot >= 0) {
    const PlanSlot& S = p->slots[slot];
    DNN_REQUIRE(S.h == L.OH && S.w == L.OW, "dnn_plan_add_route: slot %d is %dx%d, the folded input %dx%d", slot, S.h,
                S.w, L.OH, L.OW);
    L.Cb = S.c;
    L.slot_loc = S.loc;
  }
  L.OC = block * block * L.C + L.Cb;
  push_computing(p, std::move(L));
  return 0;
}

int dnn_plan_add_shortcut(dnn_plan* p, int slot, int leaky) {
  DNN_REQUIRE(p && !p->finalized, "dnn_plan_add_shortcut: plan is NULL or finalized");
  DNN_REQUIRE(!p->fp16, "dnn_plan_add_shortcut: fp32 plans only (this is an fp16 plan)");
  DNN_REQUIRE(leaky >= 0 && leaky <= 2, "dnn_plan_add_shortcut: leaky must be 0, 1 or 2");
  DNN_REQUIRE(slot_is_live(p, slot), "dnn_plan_add_shortcut: unknown or released slot %d (%d defined)", slot,
              (int)p->slots.size());
  const PlanSlot& S = p->slots[slot];
  DNN_REQUIRE(S.h == p->cur_h && S.w == p->cur_w && S.c == p->cur_c,
              "dnn_plan_add_shortcut: slot %d is %dx%dx%d, the current tensor %dx%dx%d", slot, S.h, S.w, S.c, p->cur_h,
              p->cur_w, p->cur_c);
  PlanLayer L;
  shape_only_layer(p, &L, LAYER_SHORTCUT);
  L.slot = slot;
  L.slot_loc = S.loc;
  L.leaky = leaky;
  push_computing(p, std::move(L));
  return 0;
}

int dnn_plan_add_upsample(dnn_plan* p, int factor) {
  DNN_REQUIRE(p && !p->finalized, "dnn_plan_add_upsample: plan is NULL or finalized");
  DNN_REQUIRE(!p->fp16, "dnn_plan_add_upsample: fp32 plans only (this is an fp16 plan)");
  DNN_REQUIRE(factor >= 1 && factor <= 8, "dnn_plan_add_upsample: factor %d outside 1..8", factor);
  PlanLayer L;
  L.type = LAYER_UPSAMPLE;
  L.H = p->cur_h;
  L.W = p->cur_w;
  L.C = L.OC = p->cur_c;
  L.OH = L.H * factor;
  L.OW = L.W * factor;
  L.factor = factor;
  push_computing(p, std::move(L));
  return 0;
}

int dnn_plan_add_slice(dnn_plan* p, int first, int channels) {
  DNN_REQUIRE(p && !p->finalized, "dnn_plan_add_slice: plan is NULL or finalized");
  DNN_REQUIRE(!p->fp16, "dnn_plan_add_slice: fp32 plans only (this is an fp16 plan)");
  DNN_REQUIRE(first >= 0 && channels >= 1 && (long long)first + channels <= p->cur_c,
              "dnn_plan_add_slice: first %d, channels %d outside the current tensor's %d channels", first, channels,
              p->cur_c);
  PlanLayer L;
  shape_only_layer(p, &L, LAYER_SLICE);
  L.OC = channels;
  L.first = first;
  push_computing(p, std::move(L));
  return 0;
}

int dnn_plan_add_spp(dnn_plan* p, int n_sizes, const int* sizes, int x_first) {
  DNN_REQUIRE(p && !p->finalized, "dnn_plan_add_spp: plan is NULL or finalized");
  DNN_REQUIRE(!p->fp16, "dnn_plan_add_spp: fp32 plans only (this is an fp16 plan)");
  if (int rc = spp_sizes_ok("dnn_plan_add_spp", n_sizes, sizes)) return rc;
  PlanLayer L;
  shape_only_layer(p, &L, LAYER_SPP);
  L.OC = (n_sizes + 1) * L.C;
  L.n_sizes = n_sizes;
  for (int j = 0; j < n_sizes; ++j) L.sizes[j] = sizes[j];
  L.x_first = x_first != 0;
  push_computing(p, std::move(L));
  return 0;
}

int dnn_plan_output_shape(const dnn_plan* p, int* batch, int* h, int* w, int* c) {
  DNN_REQUIRE(p, "dnn_plan_output_shape: plan is NULL");
  if (batch) *batch = p->batch;
  if (h) *h = p->cur_h;
  if (w) *w = p->cur_w;
  if (c) *c = p->cur_c;
  return 0;
}

int dnn_plan_memory(const dnn_plan* pc, size_t* weight_bytes, size_t* workspace_bytes) {
  DNN_REQUIRE(pc, "dnn_plan_memory: plan is NULL");
  dnn_plan* p = const_cast<dnn_plan*>(pc);
  layout(p);
  if (weight_bytes) *weight_bytes = p->weight_floats * sizeof(float);
  if (workspace_bytes) *workspace_bytes = p->ws_floats * sizeof(float);
  return 0;
}

static int upload_weights(dnn_plan* p) {
  size_t maxw = 0, maxp = 0;
  for (auto& L : p->layers)
    if (L.is_conv()) {
      maxw = std::max(maxw, L.w.size());
      maxp = std::max(maxp, (size_t)L.Npad * L.Kpad);
    }
  float* tmp = nullptr;
  DNN_HIP_TRY(hipMalloc(&tmp, (std::max<size_t>(maxw, 1) + (p->fp16 ? maxp : 0)) * sizeof(float)));
  float* packed32 = tmp + std::max<size_t>(maxw, 1);  // fp16 plans: fp32 pack, then convert
  int rc = 0;
  for (auto& L : p->layers) {
    if (!L.is_conv()) continue;
    const size_t wb = L.w.size() * sizeof(float);
    const WeightPack pack = weight_pack(L.variant);
    if (pack == PACK_HWIO) {  // HWIO [K][N] as is: one 16-float row per (tap, cin)
      if (hipMemcpy(p->weights + L.w_off, L.w.data(), wb, hipMemcpyHostToDevice) != hipSuccess) rc = -1;
    } else {
      if (hipMemcpy(tmp, L.w.data(), wb, hipMemcpyHostToDevice) != hipSuccess) rc = -1;
      if (p->fp16) {
        if (!rc)
          rc = launch_pack_weights(tmp, packed32, L.K, L.OC, L.Kpad, L.Npad,
                                   pack == PACK_BT_TILE16 ? 5 : pack == PACK_BT_PATCH16 ? patch16_pack_order() : 0,
                                   L.kh, L.kw, L.C, 0);
        if (!rc)
          rc = launch_f32_to_f16(packed32, reinterpret_cast<half_t*>(p->weights + L.w_off),
                                 (long long)L.Npad * L.Kpad, 0);
      } else if (!rc && pack == PACK_X3 && L.h2) {  // (two fp16 pieces: 2/3 of the slot)
        rc = launch_pack_weights_h2(tmp, reinterpret_cast<unsigned short*>(p->weights + L.w_off), L.K, L.OC, L.Npad,
                                    L.C, 0);
      } else if (!rc && pack == PACK_X3) {
        rc = launch_pack_weights_x3(tmp, reinterpret_cast<unsigned short*>(p->weights + L.w_off), L.K, L.OC, L.Npad,
                                    L.C, 0);
      } else if (!rc) {
        rc = launch_pack_weights(tmp, p->weights + L.w_off, L.K, L.OC, L.Kpad, L.Npad, 0, L.kh, L.kw, L.C, 0);
      }
    }
    float* e = p->weights + L.epi_off;
    const size_t nb = (size_t)L.Npad * sizeof(float);
    if (!rc && (hipMemcpy(e, L.bias.data(), nb, hipMemcpyHostToDevice) != hipSuccess ||
                hipMemcpy(e + L.Npad, L.mean.data(), nb, hipMemcpyHostToDevice) != hipSuccess ||
                hipMemcpy(e + 2 * L.Npad, L.sq.data(), nb, hipMemcpyHostToDevice) != hipSuccess ||
                hipMemcpy(e + 3 * L.Npad, L.gamma.data(), nb, hipMemcpyHostToDevice) != hipSuccess))
      rc = -1;
    if (!rc && hipDeviceSynchronize() != hipSuccess) rc = -1;
    if (rc) {
      if (last_error()[0] == 0) set_error("dnn_plan_finalize: weight upload failed");
      break;
    }
  }
  (void)hipFree(tmp);
  if (rc) return rc;
  for (auto& L : p->layers) std::vector<float>().swap(L.w);  // host copies no longer needed
  return 0;
}

int dnn_plan_finalize(dnn_plan* p, int device, void* weights, void* workspace) {
  DNN_REQUIRE(p && !p->finalized, "dnn_plan_finalize: plan is NULL or already finalized");
  DNN_REQUIRE(!p->layers.empty(), "dnn_plan_finalize: plan has no layers");
  {
    size_t last = p->layers.size();  // (release entries after the last writer do not count)
    while (last > 0 && p->layers[last - 1].type == LAYER_RELEASE) --last;
    DNN_REQUIRE(last > 0, "dnn_plan_finalize: plan has no layer that computes");
    const int t = p->layers[last - 1].type;
    DNN_REQUIRE(t != LAYER_STASH && t != LAYER_RESTORE && t != LAYER_TAP,
                "dnn_plan_finalize: the plan ends in a %s: its output would not be written (end with a layer that "
                "computes)", t == LAYER_STASH ? "stash" : t == LAYER_TAP ? "tap" : "restore");
  }
  if (p->fp16)
    for (auto& L : p->layers) {
      DNN_REQUIRE(!L.is(CONV_GEMM),
                  "dnn_plan_finalize: fp16 plan cannot run conv %dx%dx%d k%dx%d (needs C %% 8 == 0, or <= 4 "
                  "input channels with a fused 2x2/s2 pool)", L.H, L.W, L.C, L.kh, L.kw);
      DNN_REQUIRE(L.type != LAYER_POOL || L.C % 8 == 0, "dnn_plan_finalize: fp16 pool needs C %% 8 == 0 (C=%d)", L.C);
    }
  layout(p);
  // the fused kernels' output stores take 32-bit byte offsets from their region's base (the
  // write-through buffer stores of gemm_f32.h store16_at): every region a kernel writes, the
  // caller's output included (at most one activation), must stay below 2 GiB
  {
    const unsigned long long lim = 0x80000000ULL;
    bool ok = (unsigned long long)p->act_floats * 4 < lim && (unsigned long long)p->slab_floats * 4 < lim;
    for (auto& L : p->layers)
      if (L.out_padded)
        ok = ok && (unsigned long long)p->batch * (L.out_h() + 2) * (L.out_w() + 2) * L.OC * (p->fp16 ? 2 : 6) < lim;
    for (size_t e : p->region_elems) ok = ok && (unsigned long long)p->batch * e * 4 < lim;
    DNN_REQUIRE(ok, "dnn_plan_finalize: batch %d makes an activation region >= 2 GiB; split the batch over plans",
                p->batch);
  }
  DNN_HIP_TRY(hipSetDevice(device));
  p->device = device;
  if (weights) {
    p->weights = static_cast<float*>(weights);
  } else {
    DNN_HIP_TRY(hipMalloc(&p->weights, p->weight_floats * sizeof(float)));
    p->own_weights = true;
  }
  if (workspace) {
    p->ws = static_cast<float*>(workspace);
  } else {
    DNN_HIP_TRY(hipMalloc(&p->ws, p->ws_floats * sizeof(float)));
    p->own_ws = true;
  }
  // zero page at the end of the workspace (padding taps of the implicit GEMM read it)
  DNN_HIP_TRY(hipMemset(p->ws + p->at.zero, 0, dnn_plan::kZeroFloats * sizeof(float)));
  if (p->pad_floats)  // zero borders of the padded activations (interiors are rewritten every run)
    DNN_HIP_TRY(hipMemset(p->ws + p->at.pad, 0, p->pad_floats * sizeof(float)));
  if (p->ticket_floats)  // fused split-K tickets start at zero; every launch leaves them zero
    DNN_HIP_TRY(hipMemset(p->ws + p->at.tickets, 0, p->ticket_floats * sizeof(float)));
  bool all_host = true;
  for (auto& L : p->layers)
    if (L.is_conv() && !L.have_host) all_host = false;
  if (all_host) {
    int rc = upload_weights(p);
    if (rc) return rc;
  }
  DNN_HIP_TRY(hipDeviceSynchronize());
  p->finalized = true;
  return 0;
}

int dnn_plan_range_events(dnn_plan* p, unsigned* events) {
  DNN_REQUIRE(p && p->finalized && events, "dnn_plan_range_events: plan not finalized, or events is NULL");
  *events = 0;
  bool synced = false;
  for (auto& L : p->layers) {  // one word per producer of h2 planes
    if (!L.out_h2) continue;
    if (!synced) {
      DNN_HIP_TRY(hipSetDevice(p->device));
      DNN_HIP_TRY(hipDeviceSynchronize());
      synced = true;
    }
    unsigned w = 0;
    DNN_HIP_TRY(hipMemcpy(&w, range_word(p, L), sizeof(unsigned), hipMemcpyDeviceToHost));
    if (w) DNN_HIP_TRY(hipMemset(range_word(p, L), 0, sizeof(unsigned)));
    *events += w ? 1u : 0u;
  }
  return 0;
}

int dnn_plan_weight_buffer(const dnn_plan* p, void** ptr, size_t* bytes) {
  DNN_REQUIRE(p && p->finalized, "dnn_plan_weight_buffer: plan not finalized");
  if (ptr) *ptr = p->weights;
  if (bytes) *bytes = p->weight_floats * sizeof(float);
  return 0;
}

static int record_events(dnn_plan* p, int kernel, hipStream_t s);

// before each kernel (its plan index) and after the last one (-1): HIP events (timing) and the
// clock stamps around the stamped kernel — the opening stamp before its opening event, the closing
// stamp after the event that closes it, so an event-timed kernel never contains a stamp launch
static int record(dnn_plan* p, int kernel, hipStream_t s) {
  int rc;
  if (p->mark_kernel >= 0 && kernel == p->mark_kernel) DNN_HIP_TRY(hipEventRecord(p->mark_ev, s));
  const bool close_now = p->clk_open;
  if (!close_now && p->clk_kernel >= 0 && kernel == p->clk_kernel && p->clk_used < p->clk_cap) {
    if ((rc = launch_clock_stamp(s, p->clk_buf + (size_t)p->clk_used * 8 * p->clk_nwg, p->clk_nwg))) return rc;
    p->clk_open = true;
  }
  if ((rc = record_events(p, kernel, s))) return rc;
  if (close_now) {
    if ((rc = launch_clock_stamp(s, p->clk_buf + ((size_t)p->clk_used * 8 + 4) * p->clk_nwg, p->clk_nwg))) return rc;
    p->clk_open = false;
    p->clk_used++;
  }
  return 0;
}

static int record_events(dnn_plan* p, int kernel, hipStream_t s) {
  if (!p->timing) return 0;
  if (p->timing_only >= 0) {  // one kernel: its opening event and the next one (which closes it)
    const bool closes = p->ev_used > 0 && p->ev_kernel[p->ev_used - 1] == p->timing_only;
    if (kernel != p->timing_only && !closes) return 0;
    if (kernel != p->timing_only) kernel = -1;  // a pure closer opens nothing
  }
  if (p->ev_used + 1 >= p->ev_cap) return 0;  // capacity exhausted: stop recording silently
  DNN_HIP_TRY(hipEventRecord(p->ev[p->ev_used], s));
  p->ev_kernel[p->ev_used] = kernel;
  p->ev_used++;
  return 0;
}

// What a run gives its steps: the image count (<= batch), the caller's tensors and the stream
struct RunArgs {
  int n;
  const float* d_in;
  float* d_out;
  hipStream_t s;
};

// the address of a location in this run (LOC_IN is only ever read; LOC_NONE: NULL)
static float* locate(const dnn_plan* p, const RunArgs& r, int loc) {
  if (loc >= LOC_PAD) return p->ws + p->at.pad + p->layers[loc - LOC_PAD].pad_off;
  if (loc >= LOC_REGION) return p->ws + p->at.regions + p->region_off[loc - LOC_REGION];
  switch (loc) {
    case LOC_OUT: return r.d_out;
    case LOC_IN: return const_cast<float*>(r.d_in);
    case LOC_ACT0: return p->ws + p->at.act0;
    case LOC_ACT1: return p->ws + p->at.act1;
    default: return nullptr;
  }
}

static EpiParams epilogue(const dnn_plan* p, const PlanLayer& L) {
  const float* e = p->weights + L.epi_off;
  return EpiParams{e, e + L.Npad, e + 2 * L.Npad, e + 3 * L.Npad, L.epi_flags};
}

static unsigned* ticket_area(const dnn_plan* p) {  // (NULL: split layers leave partials for a reduce step)
  return p->sw.splitk_fused ? reinterpret_cast<unsigned*>(p->ws + p->at.tickets) : nullptr;
}

// fp16 plans: fp16 activations between layers, fp32 frames in / predictions out
static int launch_step16(dnn_plan* p, const Step& st, const RunArgs& r) {
  const int n = r.n;
  hipStream_t s = r.s;
  float* src32 = locate(p, r, st.src);  // (fp32 at the plan's edges: the frames, the output)
  float* dst32 = locate(p, r, st.dst);
  const half_t* cur = reinterpret_cast<const half_t*>(src32);
  half_t* dst = reinterpret_cast<half_t*>(dst32);
  if (st.kind == STEP_CVT_IN) return launch_f32_to_f16(src32, dst, (long long)n * p->in_h * p->in_w * p->in_c, s);
  if (st.kind == STEP_CVT_OUT) return launch_f16_to_f32(cur, dst32, (long long)n * p->cur_h * p->cur_w * p->cur_c, s);
  const PlanLayer& L = p->layers[st.layer];
  const int padded = st.dst >= LOC_PAD ? 1 : 0;  // the output is written zero-bordered
  float* slab = p->ws + p->at.slab;
  const float* zero = p->ws + p->at.zero;
  const long long Mc = (long long)n * L.OH * L.OW;
  switch (st.kind) {
    case STEP_POOL: {
      PoolGeom g{n, L.H, L.W, L.C, L.OH, L.OW, L.kh, L.kw, L.sh, L.sw, L.pt, L.pl, 0};
      return launch_maxpool16(cur, dst, g, s, padded);
    }
    case STEP_REDUCE:
      return launch_splitk_reduce16(slab, L.splits, Mc, L.OC, dst, L.OC, epilogue(p, L), s);
    case STEP_CONV:
      break;  // (below)
    default:
      set_error("dnn_plan_run: fp16 plan has an unsupported step kind %d", (int)st.kind);
      return -2;
  }
  const EpiParams epi = epilogue(p, L);
  const half_t* wt = reinterpret_cast<const half_t*>(p->weights + L.w_off);
  const DirectGeom dg{n, L.H, L.W, L.OH, L.OW, L.PH, L.PW, L.pt, L.pl};
  switch (L.variant) {
    case CONV_DIRECT:  // (conv0: its source is the fp32 frames, its weights stay fp32)
      return conv0_mfma_supported(L.C, L.OC, L.kh, L.kw, L.sh, L.sw)
                 ? launch_conv0_mfma_f16(p->sw, src32, p->weights + L.w_off, dst, dg, L.C, epi, s)
                 : launch_conv3x3_pool2_direct_f16out(src32, p->weights + L.w_off, dst, dg, L.C, L.OC, epi, s);
    case CONV_PATCH:
      return launch_conv1_patch_f16(p->sw, cur, wt, L.Kpad, dst, dg, zero, epi, s, padded);
    case CONV_DIRECT_A:
      if (st.dst == LOC_OUT)  // (direct_out: the last layer writes the fp32 output)
        return launch_gemm16_f32out(cur, L.C, wt, L.Kpad, L.Npad, dst32, L.OC, Mc, L.OC, L.Kpad, epi, s);
      return launch_gemm16(p->sw, L.cfg, GEMM_DENSE, cur, L.C, ImplicitConv{}, wt, L.Kpad, dst, L.OC, Mc, L.OC, L.Kpad, epi, s,
                           L.splits, slab, ticket_area(p));
    case CONV_PATCH16:
      return launch_conv_patch16(cur, wt, L.Kpad, dst, padded, Mc, L.OC, L.K, L.H, L.W, L.C, epi, s);
    case CONV_TILE16:
    case CONV_IMG16:
      return launch_conv_tile16(p->sw, cur, wt, L.Kpad, dst, padded, n, L.OC, L.K, L.H, L.W, L.C, epi, s, L.pool);
    case CONV_IMPLICIT: {
      ImplicitConv ic{zero, L.H, L.W, L.C, L.OH, L.OW, L.PH, L.PW, L.kh, L.kw, L.sh, L.sw, L.pt, L.pl,
                      L.pool == POOL_S2 ? 1 : 0};
      return launch_gemm16(p->sw, L.cfg, L.pool == POOL_S2 ? GEMM_IMPLICIT_POOL : GEMM_IMPLICIT, cur, 0, ic, wt, L.Kpad, dst,
                           L.OC, L.rows(n), L.OC, L.Kpad, epi, s, L.splits, slab, ticket_area(p));
    }
    default:
      set_error("dnn_plan_run: fp16 plan has an unsupported conv mode %d", L.variant);
      return -2;
  }
}

// fp32 plans.  The launchers that can write x3 split planes take both outputs, one of them NULL
static int launch_step32(dnn_plan* p, const Step& st, const RunArgs& r) {
  const int n = r.n;
  hipStream_t s = r.s;
  const PlanLayer& L = p->layers[st.layer];
  const float* cur = locate(p, r, st.src);
  // dst: the layer's plain NHWC output; dsplit: its split-plane area, when that is what the step writes
  float* dst = locate(p, r, L.dst_loc);
  unsigned short* dsplit = st.dst >= LOC_PAD ? reinterpret_cast<unsigned short*>(locate(p, r, st.dst)) : nullptr;
  float* slab = p->ws + p->at.slab;
  const float* zero = p->ws + p->at.zero;
  const long long Mc = (long long)n * L.OH * L.OW;
  switch (st.kind) {
    case STEP_IM2COL: {
      ConvGeom g{n, L.H, L.W, L.C, L.OH, L.OW, L.kh, L.kw, L.sh, L.sw, L.pt, L.pl, L.K, L.Kpad};
      return launch_im2col(p->sw, cur, p->ws + p->at.col, g, s);
    }
    case STEP_CONV:
      break;  // (below)
    case STEP_REDUCE:
      return launch_splitk_reduce(slab, L.splits, Mc, L.OC, dst, L.OC, epilogue(p, L), s);
    case STEP_X3_COMBINE: {
      PoolGeom id{n, L.OH, L.OW, L.OC, L.OH, L.OW, 1, 1, 1, 1, 0, 0, 0};
      return launch_x3_combine(slab, L.splits, Mc * L.OC, epilogue(p, L), id, dsplit ? nullptr : dst, dsplit, s);
    }
    case STEP_POOL: {
      PoolGeom g{n, L.H, L.W, L.C, L.OH, L.OW, L.kh, L.kw, L.sh, L.sw, L.pt, L.pl, 0};
      return dsplit ? launch_maxpool_x3(cur, dsplit, g, s) : launch_maxpool(cur, dst, g, s);
    }
    case STEP_X3_COMBINE_POOL: {  // the conv before this pool left partials: sum, its epilogue, pool
      PoolGeom g{n, L.H, L.W, L.C, L.OH, L.OW, L.kh, L.kw, L.sh, L.sw, L.pt, L.pl, 0};
      const PlanLayer& conv = p->layers[st.layer - 1];
      return launch_x3_combine(slab, conv.splits, (long long)n * conv.OH * conv.OW * conv.OC, epilogue(p, conv), g,
                               dsplit ? nullptr : dst, dsplit, s);
    }
    case STEP_ROUTE:
      return launch_route(cur, L.slot >= 0 ? locate(p, r, L.slot_loc) : nullptr, dst, n, L.H, L.W, L.C, L.block, L.Cb,
                          L.slot_first ? 1 : 0, s);
    case STEP_SHORTCUT:
      return launch_shortcut(cur, locate(p, r, L.slot_loc), dst, (long long)n * L.H * L.W * L.C, L.leaky, s);
    case STEP_UPSAMPLE:
      return launch_upsample(cur, dst, n, L.H, L.W, L.C, L.factor, s);
    case STEP_SLICE:
      return launch_slice(cur, dst, n, L.H, L.W, L.C, L.first, L.OC, s);
    case STEP_SPP:
      return launch_spp(cur, dst, n, L.H, L.W, L.C, L.n_sizes, L.sizes, L.x_first ? 1 : 0, s);
    default:
      set_error("dnn_plan_run: fp32 plan has an unsupported step kind %d", (int)st.kind);
      return -2;
  }
  const EpiParams epi = epilogue(p, L);
  const float* wt = p->weights + L.w_off;
  const unsigned short* cur3 = reinterpret_cast<const unsigned short*>(cur);  // (x3 convs: split planes in,
  const unsigned short* wt3 = reinterpret_cast<const unsigned short*>(wt);    //  three bf16 pieces per weight)
  const DirectGeom dg{n, L.H, L.W, L.OH, L.OW, L.PH, L.PW, L.pt, L.pl};
  const int oh2 = dsplit && L.out_h2 ? 1 : 0;  // (a producer of h2 planes: it gets its range word)
  unsigned* const range = oh2 ? range_word(p, L) : nullptr;
  switch (L.variant) {
    case CONV_GEMM:
      return launch_gemm(p->sw, L.cfg, p->ws + p->at.col, L.Kpad, wt, L.Kpad, dst, L.OC, Mc, L.OC, L.Kpad, epi, s, L.splits,
                         slab, ticket_area(p));
    case CONV_DIRECT_A:
      return launch_gemm(p->sw, L.cfg, cur, L.C, wt, L.Kpad, dst, L.OC, Mc, L.OC, L.Kpad, epi, s, L.splits, slab,
                         ticket_area(p));
    case CONV_IMPLICIT: {
      ImplicitConv ic{zero, L.H, L.W, L.C, L.OH, L.OW, L.PH, L.PW, L.kh, L.kw, L.sh, L.sw, L.pt, L.pl,
                      L.pool == POOL_S2 ? 1 : 0};
      const long long M = L.rows(n);
      const int gm = L.pool == POOL_S2 ? GEMM_IMPLICIT_POOL : GEMM_IMPLICIT;
      // feeding an x3 conv: the pooled epilogue stores the split planes (EPI_OUT_X3)
      EpiParams ep = epi;
      float* o = dst;
      if (dsplit) {
        ep.flags |= EPI_OUT_X3;
        o = reinterpret_cast<float*>(dsplit);
      }
      // unsplit layers: the persistent kernel (same bits) when it covers the config
      int rc = L.splits == 1 ? launch_gemm_persist(p->sw, L.cfg, gm, cur, ic, wt, L.Kpad, o, L.OC, M, L.OC, L.Kpad, ep, s) : -3;
      if (rc == -3)
        rc = launch_gemm_implicit(p->sw, L.cfg, gm, cur, ic, wt, L.Kpad, o, L.OC, M, L.OC, L.Kpad, ep, s, L.splits, slab,
                                  ticket_area(p));
      return rc;
    }
    case CONV_DIRECT:
      return conv0_mfma_supported(L.C, L.OC, L.kh, L.kw, L.sh, L.sw)
                 ? launch_conv0_mfma(p->sw, cur, wt, dst, dg, L.C, zero, epi, s)
                 : launch_conv3x3_pool2_direct(cur, wt, dst, dg, L.C, L.OC, epi, s);
    case CONV_PATCH:
      return launch_conv3x3_patch_pool(cur, wt, L.Kpad, dst, dg, L.C, L.OC, zero, epi, s, dsplit);
    case CONV_X3_1X1:
      return launch_conv_x3_1x1(cur3, wt3, dst, Mc, L.OC, L.Npad, L.K, L.H, L.W, L.C, epi, s);
    case CONV_X3_1X1_KTILE:
      return launch_conv_x3_1x1_ktile(cur3, wt3, dst, Mc, L.OC, L.Npad, L.K, L.H, L.W, L.C, epi, s);
    case CONV_X3_IMG:
      return launch_conv_x3_img(cur3, wt3, dsplit ? nullptr : dst, dsplit, n, L.OC, L.Npad, L.K, L.H, L.W, L.C, epi, s,
                                oh2, range);
    case CONV_X3_KTILE:
      return launch_conv_x3_ktile(cur3, wt3, dsplit ? nullptr : dst, dsplit, L.rows(n), L.OC, L.Npad, L.K, L.H, L.W,
                                  L.C, epi, s, L.pool);
    case CONV_X3_LAT:  // (always split: raw partials into the slab; the next pool's step or a combine step finishes)
      return launch_conv_x3_lat(cur3, wt3, slab, Mc, L.OC, L.Npad, L.K, L.H, L.W, L.C, L.splits, s);
    case CONV_X3:
      if (L.h2)  // two fp16 pieces per operand (resolve_h2)
        return launch_conv_x3_h2(cur3, wt3, dsplit ? nullptr : dst, dsplit, oh2, Mc, L.OC, L.Npad, L.K, L.H, L.W, L.C,
                                 epi, s, range);
      if (L.splits > 1)  // raw partials into the slab, as above
        return launch_conv_x3(p->sw, cur3, wt3, slab, nullptr, Mc, L.OC, L.Npad, L.K, L.H, L.W, L.C, epi, s, L.splits);
      return launch_conv_x3(p->sw, cur3, wt3, dsplit ? nullptr : dst, dsplit, L.rows(n), L.OC, L.Npad, L.K, L.H, L.W, L.C, epi,
                            s, 1, L.pool == POOL_S2 ? 1 : 0, p->latency && p->sw.splitk_fused, oh2, range);
    default:
      set_error("dnn_plan_run: fp32 plan has an unsupported conv mode %d", L.variant);
      return -2;
  }
}

// The walker: step i is kernel i of the ABI.  Before each step (its index) and after the last one
// (-1) record() places the timing events, the mark and the clock stamps.
int dnn_plan_run(dnn_plan* p, int n, const float* d_in, float* d_out, void* stream) {
  DNN_REQUIRE(p && p->finalized, "dnn_plan_run: plan not finalized");
  DNN_REQUIRE(n >= 0 && n <= p->batch, "dnn_plan_run: n=%d outside [0, %d]", n, p->batch);
  if (n == 0) return 0;
  DNN_REQUIRE(d_in && d_out, "dnn_plan_run: NULL tensor");
  const RunArgs r{n, d_in, d_out, static_cast<hipStream_t>(stream)};
  const int ns = (int)p->steps.size();
  for (int i = 0; i < ns; ++i) {
    int rc;
    if ((rc = record(p, i, r.s))) return rc;
    if ((rc = p->fp16 ? launch_step16(p, p->steps[i], r) : launch_step32(p, p->steps[i], r))) return rc;
  }
  return record(p, -1, r.s);
}

int dnn_plan_run_host(dnn_plan* p, int n, const float* h_in, float* h_out) {
  DNN_REQUIRE(p && p->finalized, "dnn_plan_run_host: plan not finalized");
  DNN_REQUIRE(n >= 0 && n <= p->batch, "dnn_plan_run_host: n=%d outside [0, %d]", n, p->batch);
  if (n == 0) return 0;
  DNN_HIP_TRY(hipSetDevice(p->device));
  const size_t in_f = (size_t)n * p->in_h * p->in_w * p->in_c;
  const size_t out_f = (size_t)n * p->cur_h * p->cur_w * p->cur_c;
  if (p->h_in_floats < in_f + out_f) {
    if (p->h_in_dev) DNN_HIP_TRY(hipFree(p->h_in_dev));
    p->h_in_dev = nullptr;
    DNN_HIP_TRY(hipMalloc(&p->h_in_dev, (in_f + out_f) * sizeof(float)));
    p->h_in_floats = in_f + out_f;
  }
  float* d_in = p->h_in_dev;
  float* d_out = p->h_in_dev + in_f;
  DNN_HIP_TRY(hipMemcpy(d_in, h_in, in_f * sizeof(float), hipMemcpyHostToDevice));
  int rc = dnn_plan_run(p, n, d_in, d_out, nullptr);
  if (rc) return rc;
  DNN_HIP_TRY(hipMemcpy(h_out, d_out, out_f * sizeof(float), hipMemcpyDeviceToHost));
  return 0;
}

int dnn_plan_run_graph(dnn_plan* p, int n, const float* d_in, float* d_out, void* stream) {
  DNN_REQUIRE(p && p->finalized, "dnn_plan_run_graph: plan not finalized");
  DNN_REQUIRE(stream != nullptr, "dnn_plan_run_graph: needs a created stream (NULL cannot be captured)");
  DNN_REQUIRE(!p->timing, "dnn_plan_run_graph: per-kernel timing is active");
  DNN_REQUIRE(p->clk_kernel < 0, "dnn_plan_run_graph: clock stamping is active");
  DNN_REQUIRE(p->mark_kernel < 0, "dnn_plan_run_graph: a mark is set");
  DNN_REQUIRE(n >= 0 && n <= p->batch, "dnn_plan_run_graph: n=%d outside [0, %d]", n, p->batch);
  if (n == 0) return 0;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (!p->gexec || p->g_n != n || p->g_in != d_in || p->g_out != d_out) {
    drop_graph(p);
    DNN_HIP_TRY(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
    const int rc = dnn_plan_run(p, n, d_in, d_out, stream);
    hipGraph_t g = nullptr;
    const hipError_t e = hipStreamEndCapture(s, &g);
    if (rc) {
      if (e == hipSuccess && g) (void)hipGraphDestroy(g);
      return rc;
    }
    DNN_HIP_TRY(e);
    p->graph = g;
    DNN_HIP_TRY(hipGraphInstantiate(&p->gexec, g, nullptr, nullptr, 0));
    p->g_n = n;
    p->g_in = d_in;
    p->g_out = d_out;
  }
  DNN_HIP_TRY(hipGraphLaunch(p->gexec, s));
  return 0;
}

int dnn_plan_num_kernels(const dnn_plan* pc) {
  if (!pc) return -2;
  dnn_plan* p = const_cast<dnn_plan*>(pc);
  if (!p->finalized) layout(p);
  return (int)p->steps.size();
}

int dnn_plan_kernel_info(const dnn_plan* pc, int idx, char* name, int name_len, double* flops, double* bytes) {
  DNN_REQUIRE(pc, "dnn_plan_kernel_info: plan is NULL");
  dnn_plan* p = const_cast<dnn_plan*>(pc);
  if (!p->finalized) layout(p);
  DNN_REQUIRE(idx >= 0 && idx < (int)p->steps.size(), "dnn_plan_kernel_info: bad index %d", idx);
  const Step& k = p->steps[idx];
  if (name && name_len > 0) snprintf(name, name_len, "%s", k.name.c_str());
  if (flops) *flops = k.flops;
  if (bytes) *bytes = k.bytes;
  return 0;
}

int dnn_plan_describe(const dnn_plan* p, char* buf, int buf_len) {
  DNN_REQUIRE(p && buf && buf_len > 0, "dnn_plan_describe: bad args");
  std::string s;
  char line[256];
  for (size_t i = 0; i < p->layers.size(); ++i) {
    const PlanLayer& L = p->layers[i];
    if (L.type == LAYER_CONV) {
      char sk[32] = "", xp[48] = "";
      if (L.splits > 1) snprintf(sk, sizeof(sk), " splitK=%d", L.splits);
      if (L.xpad)  // dnn_plan_add_conv_padded: the pads on every side, and its scale / shift epilogue
        snprintf(xp, sizeof(xp), " pad=%d,%d%s", L.pt, L.pl, (L.epi_flags & EPI_BN_AB) ? " affine" : "");
      snprintf(line, sizeof(line), "conv %dx%dx%d -> %dx%dx%d k%dx%d s%d mode=%s cfg=%d K=%d Kpad=%d%s%s%s%s%s%s\n", L.H,
               L.W, L.C, L.out_h(), L.out_w(), L.OC, L.kh, L.kw, L.sh, kVariantName[L.variant], L.cfg, L.K, L.Kpad,
               L.pool == POOL_S2 ? " +pool2x2s2" : L.pool == POOL_S1 ? " +pool2x2s1" : "", sk,
               L.splits > 1 ? (is_x3(L.variant) ? " x3-combine" : p->sw.splitk_fused ? " combine" : "") : "",
               p->fp16 ? " fp16" : "", p->latency ? " latency" : "", xp);
    } else if (L.type == LAYER_STASH || L.type == LAYER_RESTORE) {
      snprintf(line, sizeof(line), "%s %dx%dx%d slot=%d\n", L.type == LAYER_STASH ? "stash" : "restore", L.H, L.W, L.C,
               L.slot);
    } else if (L.type == LAYER_ROUTE) {
      char sb[64] = "";
      if (L.slot >= 0)
        snprintf(sb, sizeof(sb), " slot=%d (%dx%dx%d) %s", L.slot, L.OH, L.OW, L.Cb, L.slot_first ? "first" : "last");
      snprintf(line, sizeof(line), "route %dx%dx%d -> %dx%dx%d block=%d%s\n", L.H, L.W, L.C, L.OH, L.OW, L.OC, L.block,
               sb);
    } else if (L.type == LAYER_SHORTCUT) {
      snprintf(line, sizeof(line), "shortcut %dx%dx%d slot=%d act=%s\n", L.H, L.W, L.C, L.slot,
               L.leaky == 1 ? "leaky" : L.leaky == 2 ? "leaky_f32" : "none");
    } else if (L.type == LAYER_UPSAMPLE) {
      snprintf(line, sizeof(line), "upsample %dx%dx%d -> %dx%dx%d factor=%d\n", L.H, L.W, L.C, L.OH, L.OW, L.OC,
               L.factor);
    } else if (L.type == LAYER_SLICE) {
      snprintf(line, sizeof(line), "slice %dx%dx%d -> %dx%dx%d first=%d\n", L.H, L.W, L.C, L.OH, L.OW, L.OC, L.first);
    } else if (L.type == LAYER_RELEASE) {
      snprintf(line, sizeof(line), "release %dx%dx%d slot=%d\n", L.H, L.W, L.C, L.slot);
    } else if (L.type == LAYER_TAP) {
      snprintf(line, sizeof(line), "tap %dx%dx%d index=%d\n", L.H, L.W, L.C, L.slot);
    } else if (L.type == LAYER_SPP) {
      char sz[32] = "";
      for (int j = 0; j < L.n_sizes; ++j)
        snprintf(sz + strlen(sz), sizeof(sz) - strlen(sz), j ? ",%d" : "%d", L.sizes[j]);
      snprintf(line, sizeof(line), "spp %dx%dx%d -> %dx%dx%d sizes=%s x=%s\n", L.H, L.W, L.C, L.OH, L.OW, L.OC, sz,
               L.x_first ? "first" : "last");
    } else
      snprintf(line, sizeof(line), "pool %dx%dx%d -> %dx%dx%d k%dx%d s%d%s\n", L.H, L.W, L.C, L.OH, L.OW, L.OC, L.kh,
               L.kw, L.sh, p->fp16 ? " fp16" : "");
    s += line;
  }
  snprintf(buf, buf_len, "%s", s.c_str());
  return 0;
}

// One line per conv layer, in dnn_plan_describe's order: the operand pieces of the x3 arithmetic
// ("pieces=h2", "pieces=x3") or "pieces=-" for a layer on another path.  Its own call: the text of
// dnn_plan_describe is pinned by recorded plans.
int dnn_plan_describe_pieces(const dnn_plan* pc, char* buf, int buf_len) {
  DNN_REQUIRE(pc && buf && buf_len > 0, "dnn_plan_describe_pieces: bad args");
  dnn_plan* p = const_cast<dnn_plan*>(pc);
  if (!p->finalized) resolve_h2(p);
  std::string s;
  char line[64];
  int nconv = 0;
  for (auto& L : p->layers) {
    if (!L.is_conv()) continue;
    snprintf(line, sizeof(line), "conv%d pieces=%s\n", nconv++,
             L.h2 ? "h2" : (!p->fp16 && reads_split_planes(L.variant)) ? "x3" : "-");
    s += line;
  }
  snprintf(buf, buf_len, "%s", s.c_str());
  return 0;
}

int dnn_plan_timing_begin(dnn_plan* p, int max_runs) {
  DNN_REQUIRE(p && p->finalized, "dnn_plan_timing_begin: plan not finalized");
  DNN_REQUIRE(max_runs > 0, "dnn_plan_timing_begin: max_runs must be > 0");
  DNN_HIP_TRY(hipSetDevice(p->device));
  int need = max_runs * ((int)p->steps.size() + 1) + 1;
  while ((int)p->ev.size() < need) {
    hipEvent_t e;
    DNN_HIP_TRY(hipEventCreate(&e));
    p->ev.push_back(e);
  }
  p->ev_kernel.assign(p->ev.size(), -1);
  p->ev_cap = (int)p->ev.size();
  p->ev_used = 0;
  p->timing_only = -1;
  p->timing = true;
  return 0;
}

int dnn_plan_timing_begin_only(dnn_plan* p, int max_runs, int kernel_idx) {
  DNN_REQUIRE(p && kernel_idx >= 0 && kernel_idx < (int)p->steps.size(),
              "dnn_plan_timing_begin_only: bad kernel index %d", kernel_idx);
  int rc = dnn_plan_timing_begin(p, max_runs);
  if (rc) return rc;
  p->timing_only = kernel_idx;
  return 0;
}

int dnn_plan_clock_begin(dnn_plan* p, int kernel_idx, unsigned long long* dev_buf, int max_runs, int nwg) {
  DNN_REQUIRE(p && p->finalized, "dnn_plan_clock_begin: plan not finalized");
  DNN_REQUIRE(kernel_idx >= 0 && kernel_idx < (int)p->steps.size(), "dnn_plan_clock_begin: bad kernel index %d",
              kernel_idx);
  DNN_REQUIRE(dev_buf && max_runs > 0 && nwg > 0 && nwg <= 65536, "dnn_plan_clock_begin: bad buffer / runs / nwg");
  p->clk_kernel = kernel_idx;
  p->clk_buf = dev_buf;
  p->clk_cap = max_runs;
  p->clk_nwg = nwg;
  p->clk_used = 0;
  p->clk_open = false;
  return 0;
}

int dnn_plan_set_mark(dnn_plan* p, int kernel_idx) {
  DNN_REQUIRE(p && p->finalized, "dnn_plan_set_mark: plan not finalized");
  DNN_REQUIRE(kernel_idx >= -1 && kernel_idx < (int)p->steps.size(), "dnn_plan_set_mark: bad kernel index %d",
              kernel_idx);
  if (kernel_idx >= 0 && !p->mark_ev) {
    DNN_HIP_TRY(hipSetDevice(p->device));
    DNN_HIP_TRY(hipEventCreateWithFlags(&p->mark_ev, hipEventDisableTiming));
  }
  p->mark_kernel = kernel_idx;
  return 0;
}

int dnn_plan_wait_mark(dnn_plan* p, void* stream) {
  DNN_REQUIRE(p && p->mark_kernel >= 0 && p->mark_ev, "dnn_plan_wait_mark: no mark set");
  DNN_HIP_TRY(hipStreamWaitEvent(static_cast<hipStream_t>(stream), p->mark_ev, 0));
  return 0;
}

int dnn_plan_clock_end(dnn_plan* p, int* runs) {
  DNN_REQUIRE(p && p->clk_kernel >= 0, "dnn_plan_clock_end: clock stamping not active");
  DNN_REQUIRE(!p->clk_open, "dnn_plan_clock_end: a stamped kernel was not closed");
  if (runs) *runs = p->clk_used;
  p->clk_kernel = -1;
  p->clk_buf = nullptr;
  p->clk_used = p->clk_cap = 0;
  return 0;
}

int dnn_plan_timing_end(dnn_plan* p, double* ms_sum, long long* launches) {
  DNN_REQUIRE(p && p->timing, "dnn_plan_timing_end: timing not active");
  p->timing = false;
  const int nk = (int)p->steps.size();
  for (int i = 0; i < nk; ++i) {
    if (ms_sum) ms_sum[i] = 0.0;
    if (launches) launches[i] = 0;
  }
  if (p->ev_used > 0) DNN_HIP_TRY(hipEventSynchronize(p->ev[p->ev_used - 1]));
  // event i opens kernel ev_kernel[i]; it is closed by event i+1 (same stream, in order)
  for (int i = 0; i + 1 < p->ev_used; ++i) {
    int k = p->ev_kernel[i];
    if (k < 0) continue;
    float ms = 0.f;
    DNN_HIP_TRY(hipEventElapsedTime(&ms, p->ev[i], p->ev[i + 1]));
    if (ms_sum) ms_sum[k] += ms;
    if (launches) launches[k] += 1;
  }
  p->ev_used = 0;
  return 0;
}

}  // extern "C"
