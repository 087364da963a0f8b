/* dnn_hip_plan.h — device-resident, fused execution plan for the YOLOv2-tiny Conv2D path.
 *
 * The reference has no plan object: `DnnInferenceEngine.run` (proj3/dnn_openblas.py:29-57)
 * walks the networkx graph and calls one host-pointer C function per node
 * (conv2d_mul / bias_add / batch_norm / leaky_relu / max_pool2d, dnn_openblas.c).  The
 * plan is the device-resident lowering of that same node chain: each
 * Conv2D -> BiasAdd -> BatchNorm -> LeakyReLU run becomes ONE conv entry (im2col + fp32
 * MFMA GEMM with the three element-wise ops as its epilogue, evaluated in the reference's
 * operation order), each MaxPool2D one pool entry, and activations never leave HBM.
 * It is what `dnn_hip.DnnInferenceEngine.run` (the Python mirror of dnn_openblas.py)
 * lowers the graph to.  Beyond the reference's chains, stash / restore / route entries let a
 * plan fork and join (YOLOv2's passthrough: space-to-depth + channel concat), shortcut /
 * upsample / release entries express residual and top-down networks, taps give a plan extra
 * outputs (YOLOv3's three heads), an spp entry is YOLOv3-SPP's pyramid pooling block, and
 * dnn_plan_add_conv_padded is Darknet's conv: explicit padding on every side and a folded
 * BatchNorm as a per-channel scale / shift (darknet_import.py builds whole networks from it).
 *
 * Conventions: plain C ABI, cdecl, no torch types.  All tensors NHWC fp32 contiguous,
 * conv kernels HWIO (the pickle layout of proj3/yolov2tiny.py:30-77).  Functions return
 * 0 on success and a negative code on error; dnn_last_error() describes the last error
 * of the calling thread.  Padding: 0 = VALID, 1 = SAME with TF semantics
 * (get_out_pads, proj3/dnn_openblas.py:127-142).
 */
#ifndef DNN_HIP_PLAN_H
#define DNN_HIP_PLAN_H
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

typedef struct dnn_plan dnn_plan;

/* Last error message of the calling thread ("" if none). */
const char* dnn_last_error(void);

/* First 16 hex digits of the SHA-256 of the sources this library was built from
 * (csrc/Makefile SRCS); tests/conftest.py refuses a library whose id does not match. */
const char* dnn_build_id(void);

/* Create an empty plan for inputs [batch, in_h, in_w, in_c]. */
int dnn_plan_create(int batch, int in_h, int in_w, int in_c, dnn_plan** out);
void dnn_plan_destroy(dnn_plan* plan);

/* Precision of the plan (call before adding layers): 0 = fp32 everywhere (default, the
 * reference's arithmetic); 1 = fp16 conv path (BASELINE config 5): fp16 activations and
 * weights, v_mfma_f32_32x32x16_f16 with fp32 accumulation and fp32 epilogue, fp32 frames in
 * and fp32 predictions out.  fp16 plans need C % 8 == 0 for every conv except a <= 4-channel
 * 3x3 first conv followed by a 2x2/s2 pool; tolerance vs fp32: DESIGN.md. */
int dnn_plan_set_precision(dnn_plan* plan, int precision);

/* Latency mode (call before adding layers; fp32 plans): on = 1 lets the K split of a GEMM
 * layer depend on M, so a small-M forward (one frame: BASELINE config 2, the single timed
 * frame of proj3/__init__.py:24-26) spreads conv4-conv8 over the whole chip (2..16 K splits,
 * combined in split order inside the GEMM).  Outputs stay within the fp32 tolerance of the
 * reference but are no longer bit-equal to the same frame's row of a batch plan (whose
 * summation order depends on (N, K) only).  Default 0. */
int dnn_plan_set_latency_mode(dnn_plan* plan, int on);

/* Append a Conv2D (proj3/dnn_openblas.py:144-188) with its trailing BiasAdd / BatchNorm /
 * LeakyReLU fused.  kernel: [kh][kw][in_c][od] HWIO.  biases may be NULL (no BiasAdd);
 * mean/var/gamma all NULL means no BatchNorm (else all three, eps as in
 * proj3/dnn_openblas.py:263-270); leaky: 0 none, 1 = dnn_openblas.c leaky_relu
 * (t<0 ? 0.1*t in double : t), 2 = dnn_avx.c leaky_relu (max(t, 0.1f*t)).
 * Host weight pointers are copied; pass kernel == NULL to declare the layer's shape only
 * (weights then arrive through dnn_plan_weight_buffer, e.g. an RCCL broadcast). */
int dnn_plan_add_conv(dnn_plan* plan, int kh, int kw, int od, int stride_h, int stride_w, int padding,
                      const float* kernel, const float* biases, const float* mean, const float* var,
                      const float* gamma, float eps, int leaky);

/* Append a conv with explicit zero padding and a per-channel affine epilogue (fp32 plans, batch
 * and latency mode; on an fp16 plan it fails).  The reference has no such node: it is Darknet's
 * convolutional layer with its BatchNorm folded on the host.
 *
 * Geometry: pad_h rows of zeros above AND below, pad_w columns left AND right,
 *   OH = (H + 2*pad_h - kh) / stride_h + 1 (likewise OW), 0 <= pad < k.  Unlike SAME, a 3x3 /
 *   stride-2 conv with pad 1 on an even map reads one row and column before the frame and none
 *   after it (Darknet's sampling).  An empty output fails.
 * Epilogue: y = leaky(v * scale[oc] + shift[oc]); scale and shift are both set or both NULL (no
 *   affine step).  It runs as the kernels' v * alpha - beta with alpha = scale and beta = -shift,
 *   which rounds as v * scale + shift does (one multiply, one add, never contracted).  leaky: 0
 *   none, 1, 2 as dnn_plan_add_conv; max(v, 0.1f * v) (2) equals Darknet's x > 0 ? x : .1f * x
 *   for every non-NaN x.
 * kernel: [kh][kw][in_c][od] HWIO, copied; NULL declares the shape only, as for dnn_plan_add_conv
 *   (scale / shift then only say whether the layer has the affine step).
 * The execution mode is chosen exactly as dnn_plan_add_conv chooses it for the same geometry, so
 * a 3x3 / stride-1 / pad-1 entry runs what a SAME one runs; the conv0 direct kernels take front
 * pads 0,0 and 1,1 only (other pads before a 2x2/s2 pool stay on the im2col GEMM).
 * dnn_plan_describe appends " pad=<pad_h>,<pad_w>" and, with scale / shift, " affine" to the
 * layer's line.  A failed call leaves the plan unchanged. */
int dnn_plan_add_conv_padded(dnn_plan* plan, int kh, int kw, int od, int stride_h, int stride_w, int pad_h,
                             int pad_w, const float* kernel, const float* scale, const float* shift, int leaky);

/* The affine epilogue on a host tensor (H2D copies, launches, D2H copy, synchronise):
 * out = leaky(a * scale[c] + shift[c]) over [n, h, w, c], the element-wise kernels of the per-op
 * ABI with beta = -shift; scale / shift both NULL: the activation alone (leaky 1 or 2).  The tensor
 * must be below 2 GiB (refused from the arguments, before any allocation). */
int dnn_scale_shift_host(const float* a, const float* scale, const float* shift, float* out, int n, int h, int w,
                         int c, int leaky);

/* Append a MaxPool2D (proj3/dnn_openblas.py:213-242). */
int dnn_plan_add_max_pool(dnn_plan* plan, int kh, int kw, int stride_h, int stride_w, int padding);

/* Fork / join entries (fp32 plans, batch and latency mode; on an fp16 plan each of the three
 * fails).  The reference has no such nodes: they extend its chain to YOLOv2's passthrough.
 *
 * dnn_plan_add_stash: the current tensor becomes slot *slot (the lowest free number: 0, 1, ... in
 * stash order unless a slot was released, at most 4 live slots) and execution continues on it.  No kernel: the layer that produces the tensor writes it
 * into the slot's region of the workspace (batch x H x W x C floats) instead of an activation
 * buffer; a stash as the first entry names the caller's input.  A slot is written once per run.
 * dnn_plan_add_restore: the current tensor and shape become the slot's.  No kernel.
 * dnn_plan_add_route: current = route(a = current [H, W, C], b = slot's tensor, block):
 *   space_to_depth of a, [H/block, W/block, block*block*C], in TensorFlow's NHWC channel order
 *     s2d[h, w, (dy*block + dx)*C + c] = a[h*block + dy, w*block + dx, c]
 *   (not Darknet's reorg order), concatenated on channels with b (whose spatial size must be
 *   H/block x W/block), b's channels first if slot_first.  slot == -1: no b (pure space_to_depth);
 *   block == 1: plain concat.  block in 1..8, H % block == 0, W % block == 0.  One kernel
 *   ("route%d" in dnn_plan_kernel_info, 0 flops).
 * A plan cannot end in a stash or a restore (dnn_plan_finalize fails). */
int dnn_plan_add_stash(dnn_plan* plan, int* slot);
int dnn_plan_add_restore(dnn_plan* plan, int slot);
int dnn_plan_add_route(dnn_plan* plan, int block, int slot, int slot_first);

/* The route kernel on host tensors: H2D copies, launch, D2H copy, synchronise.  a [n, h, w, ca],
 * b [n, h/block, w/block, cb] (NULL with cb == 0), out [n, h/block, w/block, block*block*ca + cb];
 * semantics as dnn_plan_add_route (b_first = slot_first).  Each tensor must be below 2 GiB. */
int dnn_route_host(const float* a, const float* b, float* out, int n, int h, int w, int ca, int block, int cb,
                   int b_first);

/* Residual and top-down entries (fp32 plans, batch and latency mode; on an fp16 plan each of the
 * three fails).  The reference has no such nodes: they extend its chain to the residual block
 * y = x + f(x) of Darknet-53 and to the upsample + concat merge of detection necks.
 *
 * dnn_plan_add_shortcut: current = act(current + slot's tensor), element by element.  The slot
 *   must be live and of the current tensor's shape.  One fp32 add, rounded once; leaky as in
 *   dnn_plan_add_conv (0 none, 1, 2).  One kernel ("shortcut%d" in dnn_plan_kernel_info, one flop
 *   per output element, three tensors of bytes).
 * dnn_plan_add_upsample: nearest neighbour, [H, W, C] -> [H*factor, W*factor, C],
 *   out[h, w, c] = in[h / factor, w / factor, c], factor in 1..8.  One kernel ("upsample%d", 0 flops).
 * dnn_plan_add_release: the slot stops being live.  No kernel.  The next dnn_plan_add_stash
 *   returns the lowest free slot number, so a plan may stash any number of tensors as long as at
 *   most 4 are live at once.  A restore, route, shortcut or second release of a released slot
 *   fails and changes nothing.  The slot's workspace region is handed back too: once no live slot
 *   names a region and the current tensor has left it, a producer added AFTER that point may be
 *   given it (the smallest free region that fits, else the largest, which grows), so no layer
 *   writes a region that it or an earlier layer reads; dnn_plan_memory sizes each region by the
 *   largest tensor it ever holds.  A chain of residual blocks alternates between two regions.
 * The inputs and outputs of all three are plain NHWC fp32 (they stop the conv / pool fusions like
 * the fork / join entries); a failed call leaves the plan unchanged. */
int dnn_plan_add_shortcut(dnn_plan* plan, int slot, int leaky);
int dnn_plan_add_upsample(dnn_plan* plan, int factor);
int dnn_plan_add_release(dnn_plan* plan, int slot);

/* Taps: extra outputs of a plan (fp32 plans, batch and latency mode).  The reference's graphs have
 * one output; YOLOv3 has three.
 *
 * dnn_plan_add_tap: the current tensor becomes extra output *index (0, 1, ... in call order, at
 *   most DNN_PLAN_MAX_TAPS) and execution continues on it.  No kernel.  A tap is a stash that is
 *   never released and takes no slot number: the layer that produces the tensor writes it into a
 *   workspace region owned by the tap (plain NHWC fp32; the conv / pool fusions stop as for a
 *   stash) and later consumers read it from there; a tensor that already sits in a region (just
 *   stashed or restored) is tapped in place.  From the tap entry on no later producer is given
 *   that region.  Fails, leaving the plan unchanged, on an fp16 plan, on a finalized plan, when no
 *   layer has run yet (the current tensor is the plan's input) and for a fifth tap.  A plan cannot
 *   end in a tap (dnn_plan_finalize fails, as for a stash): the last tensor goes to d_out.
 * dnn_plan_num_taps / dnn_plan_tap_shape: the taps so far and each one's per-image shape.
 * dnn_plan_tap_buffer (after finalize): the tap's device address and its size for the planned
 *   batch.  After a run of n images has completed on its stream the first n*h*w*c floats there
 *   are the tap's tensor, valid until the next run; the rest is not written.  The address is the
 *   same for every run (dnn_plan_run, dnn_plan_run_host, dnn_plan_run_graph) and lies inside a
 *   caller-supplied workspace.
 * dnn_plan_tap_read_host: host-pointer convenience for use after dnn_plan_run_host: a synchronous
 *   device-to-host copy of the first n images of the tap into h_out [n, h, w, c]. */
#define DNN_PLAN_MAX_TAPS 4
int dnn_plan_add_tap(dnn_plan* plan, int* index);
int dnn_plan_num_taps(const dnn_plan* plan);
int dnn_plan_tap_shape(const dnn_plan* plan, int index, int* h, int* w, int* c);
int dnn_plan_tap_buffer(const dnn_plan* plan, int index, void** ptr, size_t* bytes);
int dnn_plan_tap_read_host(const dnn_plan* plan, int index, int n, float* h_out);

/* The shortcut and upsample kernels on host tensors (H2D copies, launch, D2H copy, synchronise):
 * out = act(a + b) over [n, h, w, c]; out [n, h*factor, w*factor, c] from a [n, h, w, c].  Each
 * tensor must be below 2 GiB (refused from the arguments, before any allocation). */
int dnn_shortcut_host(const float* a, const float* b, float* out, int n, int h, int w, int c, int leaky);
int dnn_upsample_host(const float* a, float* out, int n, int h, int w, int c, int factor);

/* Spatial pyramid pooling (fp32 plans, batch and latency mode; on an fp16 plan it fails).  The
 * reference has no such node: it is the SPP block of YOLOv3-SPP's stride-32 neck,
 *   x -> [maxpool13(x), maxpool9(x), maxpool5(x), x]   concatenated on channels.
 *
 * dnn_plan_add_spp: current [H, W, C] -> [H, W, (n_sizes + 1) * C].  Channel block j is
 *   MaxPool2D(ksize = sizes[j], stride 1, SAME) of the current tensor, bit for bit what
 *   dnn_plan_add_max_pool computes (-FLT_MAX padding, the window scanned in row-major order with
 *   m = m >= v ? m : v, so the first maximal element wins, the sign of a zero included; finite
 *   inputs), in the order given; the tensor itself is the last block, or the first with x_first
 *   (13, 9, 5 with x last is Darknet's order, x first with 5, 9, 13 YOLOv5's).  n_sizes in
 *   1..DNN_SPP_MAX_SIZES, each size odd and in 3..DNN_SPP_MAX_K; sizes may repeat.  One kernel
 *   ("spp%d" in dnn_plan_kernel_info, 0 flops, n_sizes + 2 tensors of bytes: the input once, the
 *   output once), whatever n_sizes.  Input and output are plain NHWC fp32 (the entry stops the
 *   conv / pool fusions like the fork / join entries); the input may be the caller's d_in, the
 *   output goes to a slot or tap region when a stash or tap follows and to d_out when the entry is
 *   the plan's last.  Fails, leaving the plan unchanged, on an fp16 plan, on a finalized plan, for
 *   a NULL sizes, a bad n_sizes and an even or out-of-range size.
 * dnn_spp_host: the kernel on host tensors (H2D copy, launch, D2H copy, synchronise):
 *   a [n, h, w, c] -> out [n, h, w, (n_sizes + 1) * c].  Each tensor must be below 2 GiB (refused
 *   from the arguments, before any allocation). */
#define DNN_SPP_MAX_SIZES 3
#define DNN_SPP_MAX_K 13
int dnn_plan_add_spp(dnn_plan* plan, int n_sizes, const int* sizes, int x_first);
int dnn_spp_host(const float* a, float* out, int n, int h, int w, int c, int n_sizes, const int* sizes,
                 int x_first);

/* Channel slice (fp32 plans, batch and latency mode; on an fp16 plan it fails).  The reference has
 * no such node: it is Darknet's [route] with groups / group_id, the split that opens a CSP block
 * of YOLOv4-tiny (groups=2, group_id=1: the second half of the channels).
 *
 * dnn_plan_add_slice: current [H, W, C] -> [H, W, channels], out[h, w, k] = in[h, w, first + k].
 *   0 <= first, channels >= 1, first + channels <= C; the whole tensor (first 0, channels C) is
 *   allowed and still copies.  One kernel ("slice%d" in dnn_plan_kernel_info, 0 flops, two output
 *   tensors of bytes: what it reads and what it writes), 16-byte accesses when C, first and
 *   channels are multiples of 4.  Input and output are plain NHWC fp32 (the entry stops the conv /
 *   pool fusions like the fork / join entries); the input may be the caller's d_in, the output
 *   goes to a slot or tap region when a stash or tap follows and to d_out when the entry is the
 *   plan's last.  Fails, leaving the plan unchanged, on an fp16 plan, on a finalized plan and for
 *   a range outside the current tensor's channels.  The copy is real: a consumer conv reading a
 *   channel window of the wider tensor in place is not implemented.
 * dnn_slice_host: the kernel on host tensors (H2D copy, launch, D2H copy, synchronise):
 *   a [n, h, w, c] -> out [n, h, w, channels].  Each tensor must be below 2 GiB (refused from the
 *   arguments, before any allocation). */
int dnn_plan_add_slice(dnn_plan* plan, int first, int channels);
int dnn_slice_host(const float* a, float* out, int n, int h, int w, int c, int first, int channels);

/* Output shape of the plan so far (per image, plus the planned batch). */
int dnn_plan_output_shape(const dnn_plan* plan, int* batch, int* h, int* w, int* c);

/* Human-readable lowering, one line per plan entry: shapes, execution mode (gemm =
 * explicit im2col + GEMM, direct_a = 1x1 GEMM on the input, implicit = implicit GEMM,
 * direct = direct conv, patch = LDS-patch MFMA conv), GEMM config, whether a 2x2/s2 max
 * pool is fused and whether the GEMM is split along K (splitK=3: partials + an ordered
 * reduce/epilogue kernel); a stash or restore line gives the tensor's shape and its slot, a
 * route line both shapes, the block and the slot with its shape, a shortcut line the shape, the
 * slot and the activation, an upsample line both shapes and the factor, a release line the
 * slot and its tensor's shape, a tap line ("tap HxWxC index=k") the shape and the tap's index,
 * an spp line ("spp HxWxC -> HxWx(k+1)C sizes=13,9,5 x=last") both shapes, the sizes and x's place,
 * a slice line ("slice HxWxC -> HxWxK first=f") both shapes and the first channel taken.
 * A 2x2/s2 MaxPool2D directly
 * after an implicit, patch or direct conv is folded into it; set DNN_HIP_FUSE=0 in the
 * environment before dnn_plan_create to keep every conv explicit and every pool separate
 * (DNN_HIP_PATCH=0: no patch mode). */
int dnn_plan_describe(const dnn_plan* plan, char* buf, int buf_len);

/* Device bytes the plan needs: packed weights + epilogue params, and workspace
 * (two activation buffers + the im2col buffer + one region per stashed or tapped tensor) for the
 * planned batch. */
int dnn_plan_memory(const dnn_plan* plan, size_t* weight_bytes, size_t* workspace_bytes);

/* Bind device memory and upload weights.  weights / workspace may be NULL, in which case
 * the plan hipMallocs its own.  If every conv was added with host weights they are packed
 * into the weight buffer here (hipMemcpy + pack kernel, synchronous). */
int dnn_plan_finalize(dnn_plan* plan, int device, void* weights, void* workspace);

/* Device pointer and size of the packed weight buffer (for a broadcast from rank 0). */
int dnn_plan_weight_buffer(const dnn_plan* plan, void** ptr, size_t* bytes);

/* Run n <= batch images: d_in [n,in_h,in_w,in_c] -> d_out [n,oh,ow,oc], both device
 * pointers, asynchronously on `stream` (a hipStream_t; NULL = default stream). */
int dnn_plan_run(dnn_plan* plan, int n, const float* d_in, float* d_out, void* stream);

/* Which operand pieces each conv layer's arithmetic runs on, one line per conv in
 * dnn_plan_describe's order: "conv6 pieces=h2" (two fp16 pieces, three MFMA products per fp32
 * product: the wide x3 layers whose producer can write such planes), "pieces=x3" (three bf16
 * pieces, six products) or "pieces=-" (another path).  dnn_plan_describe's own text does not show
 * it.  The choice depends on the layer and its neighbour, never on the batch, and changes neither
 * dnn_plan_memory nor the kernel list. */
int dnn_plan_describe_pieces(const dnn_plan* plan, char* buf, int buf_len);

/* Range events of the two-piece fp16 ("h2", dnn_plan_describe_pieces) layers.  Their inputs
 * are held as fp16 pairs, which cover |v| < 65520 only: a producer that meets a non-finite value
 * or a larger one writes infinite pieces (the consumer's outputs become non-finite, as for an fp32
 * infinity) and raises a sticky word in the workspace.  This call synchronises the device, stores
 * that word (0: no event since the last call or finalize) in *events and clears it.  Weights are
 * checked when a layer with host weights is added: such a layer stays on three bf16 pieces.  A
 * shape-only layer (kernel == NULL) takes the choice of in-range weights, so its arena must come
 * from a plan whose dnn_plan_describe_pieces text equals its own.  DNN_HIP_X3_H2=0 at dnn_plan_create keeps every
 * layer on three bf16 pieces. */
int dnn_plan_range_events(dnn_plan* plan, unsigned* events);

/* Host-pointer convenience: H2D copy, run, D2H copy, synchronise. */
int dnn_plan_run_host(dnn_plan* plan, int n, const float* h_in, float* h_out);

/* dnn_plan_run through a HIP graph: the first call for a given (n, d_in, d_out) captures the
 * plan's kernel sequence on `stream` (hipStreamBeginCapture) and instantiates it; every call
 * then submits the whole forward with one hipGraphLaunch — the launch-bound batch-1 case.
 * A different (n, d_in, d_out) re-captures.  `stream` must be a created stream (the NULL
 * stream cannot be captured); per-kernel timing must be off. */
int dnn_plan_run_graph(dnn_plan* plan, int n, const float* d_in, float* d_out, void* stream);

/* Per-kernel timing with HIP events recorded on the run stream.
 * begin: allocate events for up to max_runs runs and start recording;
 * end: synchronise, write per-kernel summed milliseconds and launch counts (arrays of
 * dnn_plan_num_kernels() entries), stop recording. */
int dnn_plan_num_kernels(const dnn_plan* plan);
int dnn_plan_kernel_info(const dnn_plan* plan, int idx, char* name, int name_len, double* flops,
                         double* bytes);
int dnn_plan_timing_begin(dnn_plan* plan, int max_runs);
/* As dnn_plan_timing_begin, but events are recorded only around kernel `kernel_idx` (two per
 * forward instead of one per kernel: no event packets between the other kernels); the other
 * kernels report 0 launches at dnn_plan_timing_end. */
int dnn_plan_timing_begin_only(dnn_plan* plan, int max_runs, int kernel_idx);
int dnn_plan_timing_end(dnn_plan* plan, double* ms_sum, long long* launches);

/* Shader-clock measurement (rooflines against the measured clock).
 * dnn_clock_stamp: launches `nwg` one-wave workgroups on `stream`; workgroup w stores four
 * uint64 at dev_out[4 w ..]: s_memtime (shader clock counter), s_memrealtime (100 MHz), XCC_ID,
 * HW_ID.  Two stamps bracketing a region give, per XCD, the mean shader clock over it:
 * d(memtime) / d(memrealtime) x 100 MHz.
 * dnn_plan_clock_begin: the next runs (up to max_runs) bracket kernel `kernel_idx` with two such
 * launches each — run r's opening stamps at dev_buf[8 r nwg], closing ones at [(8 r + 4) nwg];
 * dev_buf holds max_runs x 8 x nwg uint64.  The stamps sit outside the kernel's HIP-event window.
 * dnn_plan_clock_end: stops stamping and returns the number of stamped runs. */
int dnn_clock_stamp(void* stream, unsigned long long* dev_out, int nwg);
int dnn_plan_clock_begin(dnn_plan* plan, int kernel_idx, unsigned long long* dev_buf, int max_runs, int nwg);
int dnn_plan_clock_end(dnn_plan* plan, int* runs);

/* Mark inside a run (scheduling other streams' work beside a forward's later layers).
 * dnn_plan_set_mark: from now on every run records an event on its stream right before kernel
 * `kernel_idx` (-1: off; not with dnn_plan_run_graph).
 * dnn_plan_wait_mark: makes `stream` wait for the mark of the most recent run enqueued (the
 * usual stream-wait-event semantics: a later run's mark does not affect an earlier wait). */
int dnn_plan_set_mark(dnn_plan* plan, int kernel_idx);
int dnn_plan_wait_mark(dnn_plan* plan, void* stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif
