#!/usr/bin/env python3
"""YOLOv2-tiny 416x416 images/s on 1..8 MI355X through the fused HIP plan.

Workload (BASELINE.json configs[2]/[3]): a step is one forward of YOLOv2-tiny (9 convs on
fp32 MFMA with fused bias/BN/leaky and 2x2 pools, the stride-1 pool) over this GPU's batch of
64 synthetic 416x416x3 fp32 frames already resident in HBM, then (default --gather
detections) the on-GPU postprocessing (decode, 0.3 threshold, sort, greedy NMS) and the
gather of every rank's packed post-NMS detections to rank 0 over RCCL — the north star's
"gather of detections"; --gather outputs gathers the raw [64,13,13,125] outputs instead.  Weights (random-init, tiny-yolo-voc
channel plan, synth.py) are broadcast from rank 0 once before timing.  Weak scaling:
64 frames per GPU at every N.

  python bench.py [--gpus N] [--steps K] [--warmup W] [--batch 64] [--dump-outputs DIR] [--full]
N>1 is launched by the driver through torch.distributed.run (one process per GPU); when
started by hand with --gpus N>1 it relaunches itself that way.

A plain run does only what the headline needs: set-up, W warm-up steps, the pre-heat, the K
timed steps, then rank 0 prints one JSON line: images/s for the whole job (`value`), the
milliseconds one timed step took (`ms_per_step`), the per-rank breakdown of those steps.
--dump-outputs DIR (rank 0) writes what the last timed step returned, as .npy: detections
[P, 6] float64 (class, score, left, top, right, bottom; image-major), counts [images]
float64 (negative: that image's error code) and outputs [B,13,13,125] float32, rank 0's raw
network output of that step; with --gather outputs, outputs is the gathered [images,13,13,125].
Frames and weights are seeded: the same arguments give the same inputs in every run.

--full adds to the line every other measurement (HIP events and clock stamps inside the timed
region, then runs of their own: the sustained window that checks the headline (`stable`; when
it is more than 2 % slower, `value` is the lower of the two rates), the dominant kernel's
shader clock, batch-1 latency, end-to-end from host frames, the unfused and fp16 plans), and
  roofline      the dominant kernel (conv7's GEMM, M=64*169, N=1024, K=9216): executed flops /
                its mean HIP-event duration inside the timed region, vs the MFMA peak it runs on
                (MI355X_MICROARCH.md): the x3 conv (default) executes 6 x 2*M*N*K bf16 MFMA flops
                against the 2517 TFLOP/s bf16 peak, the fp32 MFMA path (DNN_HIP_X3=0) 2*M*N*K
                against 157.3; traffic from the committed PMC summary (profiles/pmc_summary.json)
                when present;
  fp32_equivalent_pct  all 9 convs (and conv6+conv7, and the whole net): ALGORITHMIC fp32 flops /
                their summed time as % of the fp32 MFMA peak; the x3 layers (conv1-conv7) run on
                the bf16 MFMA, so this exceeds 100 % and is not an MFMA utilisation;
  fp32_mfma     the north star's literal metric: the same frames through a DNN_HIP_X3=0 plan
                (every conv on the fp32 MFMA), conv6/conv7 times and % of the fp32 MFMA peak,
                forward images/s;
  cpu_baseline  clean-room restatements of the reference's OpenBLAS engine (value: its per-node
                C calls via ctypes, im2col + OpenBLAS sgemm) and AVX engine (avx_equivalent: direct
                conv, 4 pthreads, and all cores), batch 1 per image, timed on this host's
                cores on a bounded sample (N=1, rank 0 only).
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(REPO, "dnn-inference-engine_amd")
ORACLE = os.path.join(REPO, "oracle")
sys.path.insert(0, PKG)

FP32_MFMA_PEAK_TFLOPS = 157.3  # MI355X_MICROARCH.md, dense fp32 matrix (= vector) peak
FP16_MFMA_PEAK_TFLOPS = 16 * FP32_MFMA_PEAK_TFLOPS  # dense F16 MFMA (MI355X_MICROARCH.md: fp32 = 1/16 of it)
BF16_MFMA_PEAK_TFLOPS = FP16_MFMA_PEAK_TFLOPS  # the bf16 forms take the F16 forms' cycles (MI355X_MICROARCH.md)
X3_PRODUCTS = 6  # x3 conv: bf16 MFMA products per fp32 product (gemm_x3_patch.h)
HBM_PEAK_GBS = 8000.0
DOMINANT = "conv7.gemm"
NOMINAL_SCLK_GHZ = 2.4  # the clock the MFMA peaks above are quoted at (MI355X_MICROARCH.md)
CLOCK_WGS = 256  # clock-stamp workgroups per launch (one per CU: every XCD sampled)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=int(os.environ.get("WORLD_SIZE", "1")))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=64, help="frames per GPU")
    ap.add_argument("--full", action="store_true",
                    help="also measure everything beside the headline (roofline, per-kernel times, sustained "
                         "window, shader clock, batch-1 latency, end-to-end, unfused / fp32-MFMA / fp16 plans, "
                         "CPU baseline); the --no-*, --kernels, --sustained and --cpu-seconds options select "
                         "among these and have no effect without it")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="rank 0 writes what the last timed step returned to DIR/<name>.npy (float32 / float64, "
                         "at most 64 MB in all: a fixed seeded sample of a larger array)")
    ap.add_argument("--cpu-seconds", type=float, default=15.0, help="bound on the CPU-baseline sample")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--no-latency", action="store_true", help="skip the batch-1 latency measurement")
    ap.add_argument("--precision", choices=("fp32", "fp16"), default="fp32",
                    help="conv path precision (fp16 = BASELINE config 5: fp16 MFMA, fp32 accumulate)")
    ap.add_argument("--no-fp16", action="store_true", help="skip the embedded fp16 (config 5) measurement")
    ap.add_argument("--no-e2e", action="store_true", help="skip the host-frames end-to-end measurement")
    ap.add_argument("--no-unfused", action="store_true", help="skip the explicit-im2col (unfused) plan measurement")
    ap.add_argument("--no-fp32-mfma", action="store_true", help="skip the fp32-MFMA-only (DNN_HIP_X3=0) plan measurement")
    ap.add_argument("--kernels", action="store_true", help="add the per-kernel table to the JSON")
    ap.add_argument("--preheat", type=float, default=2.0,
                    help="seconds of back-to-back steps before the timed region (the clock the chip holds "
                         "under sustained load: MI355X_MICROARCH DVFS give-back), independent of --warmup")
    ap.add_argument("--sustained", type=float, default=2.0,
                    help="--full: seconds of steps after the timed region for the `sustained` field (0: skip)")
    ap.add_argument("--gather", choices=("detections", "outputs"), default="detections",
                    help="per step, gather post-NMS detections (on-GPU postprocessing, the north star's "
                         "detection gather) or the raw [n,13,13,125] outputs to rank 0")
    ap.add_argument("--dump-detections", default=None,
                    help="rank 0 writes the last timed step's gathered detections (packed rows, counts) "
                         "to this .npz (tests: multi-rank detections vs a single-process run)")
    args = ap.parse_args()
    if args.kernels and not args.full:
        ap.error("--kernels needs --full")
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    return args


DUMP_BYTES = 64 << 20  # --dump-outputs: bound on all files together


def dump_outputs(path, arrays):
    """--dump-outputs: each array of `arrays` (name -> numpy) as path/<name>.npy, float32 kept,
    everything else as float64.  Above DUMP_BYTES in all, an array larger than its equal share
    is cut to a fixed sample of its elements (seeded, sorted flat indices, the same in every
    run), written flat."""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    arrays = {k: np.ascontiguousarray(v, dtype=np.float32 if v.dtype == np.float32 else np.float64)
              for k, v in arrays.items()}
    share = DUMP_BYTES // max(len(arrays), 1)
    over = sum(a.nbytes for a in arrays.values()) > DUMP_BYTES
    for k, a in arrays.items():
        if over and a.nbytes > share:
            idx = np.sort(np.random.default_rng(0).integers(0, a.size, size=share // a.itemsize))
            a = a.reshape(-1)[idx]
        np.save(os.path.join(path, k + ".npy"), a)


def detections_as_float(dets_u8, counts):
    """Gathered packed detections ([P, 40] uint8 dnn_detection rows, counts) -> ([P, 6] float64:
    class, score, left, top, right, bottom; counts as float64)."""
    import numpy as np
    import dist as D
    rows = np.ascontiguousarray(dets_u8).reshape(-1, 40).view(D.DETECTION_DTYPE).reshape(-1)
    cols = [rows[f].astype(np.float64) for f in ("cls", "score", "left", "top", "right", "bottom")]
    return np.stack(cols, 1).reshape(-1, 6), np.asarray(counts, dtype=np.float64)


def relaunch(args):
    """--gpus N>1 without torch.distributed.run's environment: start it as a child
    (nothing has touched the GPU yet in this process)."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    sys.exit(subprocess.call(cmd))


def pmc_entry(kernel, name="pmc_summary.json"):
    """The committed rocprof/PMC summary's entry for `kernel` (profiles/, tools/prof_summary.py):
    avg_us over the profiled run's timed forwards and hbm_bytes_per_launch from the separate
    FETCH_SIZE / WRITE_SIZE passes.  {} when absent."""
    try:
        with open(os.path.join(REPO, "profiles", name)) as f:
            data = json.load(f)
        entry = dict(data.get("kernels", {}).get(kernel, {}) or {})
        if entry and data.get("same_box"):  # the profile box's own bench line (HIP events, img/s)
            entry["same_box"] = data["same_box"]
        return entry
    except Exception:
        return {}


def _timed(fn, seconds, min_runs=3, max_runs=200):
    fn()  # warm
    times, t0 = [], time.perf_counter()
    while True:
        t = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t)
        if (time.perf_counter() - t0 > seconds and len(times) >= min_runs) or len(times) >= max_runs:
            break
    return sorted(times)[len(times) // 2], len(times)


def _host_info():
    model = ""
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    model = line.split(":", 1)[1].strip()
                    break
    except OSError:
        pass
    try:
        usable = len(os.sched_getaffinity(0))
    except AttributeError:
        usable = os.cpu_count() or 1
    # a shared GPU box grants this job a CPU share (OMP_NUM_THREADS) smaller than nproc
    share = os.environ.get("OMP_NUM_THREADS", "")
    if share.isdigit() and int(share) > 0:
        usable = min(usable, int(share))
    return {"nproc": os.cpu_count(), "usable_cpus": usable, "cpu": model}


def cpu_baseline(seconds):
    """Clean-room CPU restatements of proj3's two CPU engines (oracle/, test infrastructure),
    timed on this host's cores on a bounded sample (N=1, rank 0 only), batch 1 per image as
    the reference engines run:
      value          BASELINE config 1, the OpenBLAS engine via ctypes: per node one C call
                     (oracle/dnn_oracle.c restating dnn_openblas.c:9-254), conv2d_mul = im2col +
                     OpenBLAS cblas_sgemm (the OpenBLAS build scipy ships, oracle_c.openblas_sgemm);
      numpy_equivalent  oracle/ref_numpy.py im2col + numpy sgemm + numpy element-wise ops;
      avx_equivalent direct conv over 4 pthreads as dnn_avx.c:13,33-126 (oracle/dnn_oracle.c,
                     gcc -O3 -mavx2, mul+add like _mm256_mul_ps/_mm256_add_ps), folded BN,
                     leaky max(x, 0.1x), pools; plus the same on all usable cores."""
    sys.path.insert(0, ORACLE)
    import numpy as np
    import oracle_c
    import ref_numpy as R
    import synth
    try:
        from threadpoolctl import threadpool_info
        cores = max([i.get("num_threads", 1) for i in threadpool_info() if i.get("internal_api") == "openblas"]
                    or [1])
    except Exception:
        cores = os.cpu_count() or 1
    host = _host_info()
    ws = synth.yolo_weights()
    x = synth.frame(0)
    oc = oracle_c.OracleC()
    sg = oracle_c.openblas_sgemm()
    res = {"unit": "images/s", "kind": "port", "host": host}
    if sg is not None:
        kr = oracle_c.openblas_kernels(ws)
        med, n = _timed(lambda: oracle_c.yolo_forward_openblas(oc, ws, x, sg[0], kr), 0.45 * seconds)
        res.update(value=round(1.0 / med, 3), cores=int(sg[1]),
                   sample=f"{n} single-frame YOLOv2-tiny forwards (median {med * 1e3:.0f} ms) through the "
                          "OpenBLAS engine's per-node C calls via ctypes (BASELINE config 1): np.pad, "
                          "oracle_conv2d_sgemm = single-thread im2col + OpenBLAS cblas_sgemm "
                          f"({sg[1]} OpenBLAS threads), bias_add, batch_norm, leaky, max_pool2d "
                          "(oracle/dnn_oracle.c restating dnn_openblas.c)")
    med, n = _timed(lambda: R.yolo_forward(ws, x, acc=np.float32), 0.15 * seconds)
    res["numpy_equivalent"] = {"value": round(1.0 / med, 3), "unit": "images/s", "cores": int(cores),
                               "kind": "port", "sample": f"{n} single-frame forwards (median {med * 1e3:.0f} ms), "
                               "oracle/ref_numpy.py im2col + numpy/OpenBLAS sgemm"}
    if sg is None:  # no OpenBLAS build to bind: the numpy leg is the value
        res.update({k: v for k, v in res["numpy_equivalent"].items() if k != "unit"})
    for key, nt in (("avx_equivalent", 4), ("avx_equivalent_all_cores", host["usable_cpus"])):
        med, n = _timed(lambda: oracle_c.yolo_forward_avx(oc, ws, x, nt), 0.2 * seconds)
        res[key] = {"value": round(1.0 / med, 3), "unit": "images/s", "cores": int(nt), "kind": "port",
                    "sample": f"{n} single-frame forwards (median {med * 1e3:.0f} ms), direct conv "
                              f"{nt} pthreads (oracle/dnn_oracle.c)"}
    return res


def latency_b1(dnn_hip, yolo_graph, ws, dev, iters=200, latency=True):
    """BASELINE.json configs[1]: one 416x416 frame, fp32, 1 GPU — issue-to-completion time of a
    single-frame forward (frame resident in HBM), eager (one launch per kernel) and as one
    HIP-graph launch (dnn_plan_run_graph), median over `iters` synchronised runs.  latency=True:
    the latency plan (dnn_plan_set_latency_mode: conv4-conv8 K-split over the chip); False: the
    batch plan's choices at batch 1 (bit-equal to a batch-64 row)."""
    import torch
    g1, _ = yolo_graph.build_graph(dnn_hip.DnnGraphBuilder, ws, in_shape=(1, 416, 416, 3))
    entries = dnn_hip.lower_graph(g1)
    wb, sb = dnn_hip.Plan.memory(1, (416, 416, 3), entries, latency=latency)
    wbuf = torch.empty(wb, dtype=torch.uint8, device=dev)
    sbuf = torch.empty(max(sb, 1), dtype=torch.uint8, device=dev)
    p1 = dnn_hip.Plan(1, (416, 416, 3), entries, device=dev.index, weights_ptr=wbuf.data_ptr(),
                      workspace_ptr=sbuf.data_ptr(), latency=latency)
    x = torch.rand((1, 416, 416, 3), device=dev)
    y = torch.empty((1, 13, 13, 125), device=dev)
    s = torch.cuda.Stream(dev)
    sp = s.cuda_stream
    out = {}
    for mode in ("eager", "graph"):
        run = p1.run_device if mode == "eager" else p1.run_graph
        for _ in range(10):
            run(1, x.data_ptr(), y.data_ptr(), sp)
        s.synchronize()
        t = []
        for _ in range(iters):
            t0 = time.perf_counter()
            run(1, x.data_ptr(), y.data_ptr(), sp)
            s.synchronize()
            t.append(time.perf_counter() - t0)
        out[mode + "_ms"] = round(sorted(t)[len(t) // 2] * 1e3, 4)
    # device-side duration of one graph replay (HIP events on the same stream)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(s):
        e0.record(s)
        for _ in range(50):
            p1.run_graph(1, x.data_ptr(), y.data_ptr(), sp)
        e1.record(s)
    s.synchronize()
    out["graph_device_ms"] = round(e0.elapsed_time(e1) / 50, 4)
    # the same for back-to-back eager forwards: on this runtime a graph replay's device time is a
    # few us above eager issue (tools/lat_env.py), so both are reported
    with torch.cuda.stream(s):
        e0.record(s)
        for _ in range(50):
            p1.run_device(1, x.data_ptr(), y.data_ptr(), sp)
        e1.record(s)
    s.synchronize()
    out["eager_device_ms"] = round(e0.elapsed_time(e1) / 50, 4)
    out["images_per_s_graph"] = round(1e3 / out["graph_ms"], 1)
    out["images_per_s_eager"] = round(1e3 / out["eager_ms"], 1)
    p1.timing_begin(20)
    for _ in range(20):
        p1.run_device(1, x.data_ptr(), y.data_ptr(), sp)
    ms, cnt = p1.timing_end()
    out["kernel_ms"] = {k["name"]: round(m / max(c, 1), 4) for k, m, c in zip(p1.kernels(), ms, cnt)}
    out["plan"] = "latency (K splits chosen for M = 169)" if latency else "batch rules (bit-equal to batch-64 rows)"
    out["note"] = "median issue-to-completion wall time of one synchronised single-frame forward"
    if latency:  # the same frame through this plan vs the batch plan's result: fp32 tolerance
        xb = synth_frame_dev(dev)
        yl = torch.empty((1, 13, 13, 125), device=dev)
        p1.run_device(1, xb.data_ptr(), yl.data_ptr(), sp)
        torch.cuda.synchronize()
        out["_y"] = yl
        out["_x"] = xb
    p1.close()
    return out


def synth_frame_dev(dev):
    import synth
    import torch
    return torch.from_numpy(synth.frame(0)).to(dev)


def end_to_end(plan, B, dev, stream, steps=10, hw=(480, 640)):
    """PCIe-inclusive rate (not `value`): 640x480 uint8 BGR frames already in pinned host
    memory (where a frame decoder would write them: ingest.FrameIngest.next_host_buffer) ->
    8-bit upload on a copy stream -> on-GPU resize / scale / BGR->RGB (__init__.py:8-12) ->
    forward -> postprocessing -> packed detections on the host.  The next batch's upload is
    issued before waiting for the current batch's detections, so PCIe overlaps compute."""
    import numpy as np
    import torch
    import dist as D
    import ingest
    import yolo_post
    rng = np.random.default_rng(9)
    comp = torch.cuda.ExternalStream(stream, device=dev) if stream else torch.cuda.current_stream(dev)
    fi = ingest.FrameIngest(B, hw[0], hw[1], dev, compute_stream=comp)
    for k in range(2):  # stand-in for the decoder filling both pinned slots
        fi.host[k].numpy()[...] = rng.integers(0, 256, size=(B,) + hw + (3,), dtype=np.uint8)
    out = torch.empty((B, 13, 13, 125), device=dev)
    dbuf = yolo_post.DetectionBuffers(B, dev)

    def forward(x):
        plan.run_device(B, x.data_ptr(), out.data_ptr(), stream)
        fi.release()
        dbuf.run(out.data_ptr(), B, stream)
        return dbuf.pack(B, stream)

    def run(nsteps):
        x = fi.submit_host(B)
        r = None
        for k in range(nsteps):
            pk = forward(x)
            if k + 1 < nsteps:
                x = fi.submit_host(B)  # next upload in flight while this batch computes
            r = D.gather_detections(*pk, B)
        return r

    run(2)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = run(steps)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return {"value": round(B * steps / dt, 2), "unit": "images/s", "frames": f"{hw[1]}x{hw[0]} uint8 BGR, batch {B}",
            "ms_per_batch": round(dt / steps * 1e3, 3), "detections_last_batch": int(np.clip(r[1], 0, None).sum()),
            "note": "pinned host frames -> 8-bit upload (overlapped with the previous batch) -> GPU preprocess -> "
                    "forward -> postprocess -> detections on the host; PCIe-inclusive, not `value`"}


def unfused_im2col(dnn_hip, yolo_graph, ws, dev, frames, stream, B, steps=5):
    """The reference's structure (explicit im2col into a col buffer, GEMM, separate pools;
    DNN_HIP_FUSE=0 at plan creation) on the same frames: per-kernel HBM GB/s of the im2col
    kernels against the 8 TB/s peak (algorithmic bytes 4*(M*K written + B*H*W*C read),
    SURVEY.md §8d) and the unfused forward rate beside the fused `value`."""
    import torch
    g, _ = yolo_graph.build_graph(dnn_hip.DnnGraphBuilder, ws, in_shape=(B, 416, 416, 3))
    entries = dnn_hip.lower_graph(g)
    old = os.environ.get("DNN_HIP_FUSE")
    os.environ["DNN_HIP_FUSE"] = "0"
    try:
        wb, sb = dnn_hip.Plan.memory(B, (416, 416, 3), entries)
        wbuf = torch.empty(wb, dtype=torch.uint8, device=dev)
        sbuf = torch.empty(max(sb, 1), dtype=torch.uint8, device=dev)
        pu = dnn_hip.Plan(B, (416, 416, 3), entries, device=dev.index, weights_ptr=wbuf.data_ptr(),
                          workspace_ptr=sbuf.data_ptr())
    finally:
        if old is None:
            del os.environ["DNN_HIP_FUSE"]
        else:
            os.environ["DNN_HIP_FUSE"] = old
    y = torch.empty((B, 13, 13, 125), device=dev)
    for _ in range(2):
        pu.run_device(B, frames.data_ptr(), y.data_ptr(), stream)
    torch.cuda.synchronize()
    pu.timing_begin(steps)
    for _ in range(steps):
        pu.run_device(B, frames.data_ptr(), y.data_ptr(), stream)
    ms, cnt = pu.timing_end()
    kinfo = pu.kernels()
    im2col, tot_b, tot_s = {}, 0.0, 0.0
    for k, m, c in zip(kinfo, ms, cnt):
        if not k["name"].endswith(".im2col"):
            continue
        sec = m / max(c, 1) / 1e3
        gbs = k["bytes"] / sec / 1e9
        im2col[k["name"]] = {"ms": round(sec * 1e3, 4), "gbs": round(gbs, 1),
                             "frac_hbm_peak": round(gbs / HBM_PEAK_GBS, 4), "bytes": int(k["bytes"])}
        tot_b += k["bytes"]
        tot_s += sec
    fwd_ms = sum(m / max(c, 1) for m, c in zip(ms, cnt))
    pu.close()
    return {"im2col": im2col, "im2col_total": {"ms": round(tot_s * 1e3, 4), "gbs": round(tot_b / tot_s / 1e9, 1),
                                               "frac_hbm_peak": round(tot_b / tot_s / 1e9 / HBM_PEAK_GBS, 4)},
            "unfused_forward_ms": round(fwd_ms, 4), "unfused_images_per_s": round(B / (fwd_ms / 1e3), 1),
            "note": "DNN_HIP_FUSE=0 plan (explicit im2col + GEMM + separate pools, the reference's "
                    "structure), kernel time sum; the default plan uses implicit GEMM (no col buffer)"}


def fp16_config(dnn_hip, yolo_graph, ws, dev, frames, out32, plan32, stream, B, steps=20):
    """BASELINE config 5 beside the fp32 line: the same 64 frames through an fp16 plan (fp16
    MFMA, fp32 accumulate/epilogue): forward img/s (HIP events on the run stream), per-kernel
    times, and the normwise error of its predictions vs the fp32 plan's on the same frames."""
    import torch
    g, _ = yolo_graph.build_graph(dnn_hip.DnnGraphBuilder, ws, in_shape=(B, 416, 416, 3))
    entries = dnn_hip.lower_graph(g)
    wb, sb = dnn_hip.Plan.memory(B, (416, 416, 3), entries, precision="fp16")
    wbuf = torch.empty(wb, dtype=torch.uint8, device=dev)
    sbuf = torch.empty(max(sb, 1), dtype=torch.uint8, device=dev)
    p16 = dnn_hip.Plan(B, (416, 416, 3), entries, device=dev.index, weights_ptr=wbuf.data_ptr(),
                       workspace_ptr=sbuf.data_ptr(), precision="fp16")
    y16 = torch.empty((B, 13, 13, 125), device=dev)
    for _ in range(3):
        p16.run_device(B, frames.data_ptr(), y16.data_ptr(), stream)
    plan32.run_device(B, frames.data_ptr(), out32.data_ptr(), stream)
    torch.cuda.synchronize()
    err = float((y16 - out32[:B]).abs().max() / out32[:B].abs().max())
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        p16.run_device(B, frames.data_ptr(), y16.data_ptr(), stream)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / steps
    p16.timing_begin(5)
    for _ in range(5):
        p16.run_device(B, frames.data_ptr(), y16.data_ptr(), stream)
    kms, cnt = p16.timing_end()
    kinfo = p16.kernels()
    ker = {k["name"]: round(m / max(c, 1), 4) for k, m, c in zip(kinfo, kms, cnt)}
    c7 = [(k, m / max(c, 1)) for k, m, c in zip(kinfo, kms, cnt) if k["name"] == "conv7.gemm"]
    out = {"value": round(B / (ms / 1e3), 2), "unit": "images/s", "ms_per_forward": round(ms, 4),
           "dtype": "fp16 (fp32 accumulate + epilogue)", "normwise_err_vs_fp32": err,
           "net_pct_fp16_peak": round(100 * 6.971e9 * B / (ms / 1e3) / 1e12 / FP16_MFMA_PEAK_TFLOPS, 2),
           "kernels_ms": ker, "note": "forward only (no postprocess/gather), same frames as the fp32 line"}
    if c7:
        k, m = c7[0]
        out["conv7_tflops"] = round(k["flops"] / (m / 1e3) / 1e12, 1)
    p16.close()
    return out


def fp32_mfma_config(dnn_hip, yolo_graph, ws, dev, frames, out_x3, stream, B, steps=20):
    """The north star's literal metric (`conv MFMA % of fp32 peak`, BASELINE.json): the same
    frames through a plan with every conv on the fp32 MFMA (DNN_HIP_X3=0 at plan creation:
    v_mfma_f32_32x32x2f32 / 16x16x4f32, the reference's fp32 sgemm arithmetic), forward img/s
    (HIP events on the run stream), conv6/conv7 times and their % of the 157.3 TFLOP/s fp32
    MFMA peak, and the normwise distance of its output from the default (x3) plan's."""
    import torch
    g, _ = yolo_graph.build_graph(dnn_hip.DnnGraphBuilder, ws, in_shape=(B, 416, 416, 3))
    entries = dnn_hip.lower_graph(g)
    old = os.environ.get("DNN_HIP_X3")
    os.environ["DNN_HIP_X3"] = "0"
    try:
        wb, sb = dnn_hip.Plan.memory(B, (416, 416, 3), entries)
        wbuf = torch.empty(wb, dtype=torch.uint8, device=dev)
        sbuf = torch.empty(max(sb, 1), dtype=torch.uint8, device=dev)
        pf = dnn_hip.Plan(B, (416, 416, 3), entries, device=dev.index, weights_ptr=wbuf.data_ptr(),
                          workspace_ptr=sbuf.data_ptr())
    finally:
        if old is None:
            del os.environ["DNN_HIP_X3"]
        else:
            os.environ["DNN_HIP_X3"] = old
    assert "patch_x3" not in pf.describe()
    y = torch.empty((B, 13, 13, 125), device=dev)
    for _ in range(3):
        pf.run_device(B, frames.data_ptr(), y.data_ptr(), stream)
    torch.cuda.synchronize()
    err = float((y - out_x3[:B]).abs().max() / out_x3[:B].abs().max())
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        pf.run_device(B, frames.data_ptr(), y.data_ptr(), stream)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / steps
    pf.timing_begin(5)
    for _ in range(5):
        pf.run_device(B, frames.data_ptr(), y.data_ptr(), stream)
    kms, cnt = pf.timing_end()
    kinfo = pf.kernels()
    per = {k["name"]: (k, m / max(c, 1)) for k, m, c in zip(kinfo, kms, cnt)}
    out = {"images_per_s": round(B / (ms / 1e3), 2), "ms_per_forward": round(ms, 4),
           "mfma": "v_mfma_f32_32x32x2f32 / v_mfma_f32_16x16x4f32 (fp32 in, fp32 accumulate)",
           "normwise_err_vs_x3_plan": err, "peak_tflops": FP32_MFMA_PEAK_TFLOPS}
    tot_fl = tot_s = 0.0
    for name in ("conv6.gemm", "conv7.gemm"):
        if name in per:
            k, m = per[name]
            tf = k["flops"] / (m / 1e3) / 1e12
            out[name.split(".")[0] + "_ms"] = round(m, 4)
            out[name.split(".")[0] + "_pct_fp32_peak"] = round(100 * tf / FP32_MFMA_PEAK_TFLOPS, 2)
            tot_fl += k["flops"]
            tot_s += m / 1e3
    if tot_s:
        out["conv6_conv7_pct_fp32_peak"] = round(100 * tot_fl / tot_s / 1e12 / FP32_MFMA_PEAK_TFLOPS, 2)
    gem = [(k, m) for n, (k, m) in per.items() if n.endswith(".gemm") or n.endswith(".direct")]
    gfl, gs = sum(k["flops"] for k, _ in gem), sum(m for _, m in gem) / 1e3
    out["all_convs_pct_fp32_peak"] = round(100 * gfl / gs / 1e12 / FP32_MFMA_PEAK_TFLOPS, 2)
    out["note"] = "forward only, same frames as the fp32 line; kernel times from HIP events around every kernel"
    pf.close()
    return out


def main():
    args = parse()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        relaunch(args)

    import numpy as np
    import torch
    import torch.distributed as tdist

    import dist as D
    import dnn_hip
    import synth
    import yolo_graph

    rank, local_rank, world = D.env_rank()
    # rehearsal switches for a one-GPU box (never set by the driver): every rank on cuda:0
    # and gloo (host-staged collectives) instead of RCCL, so --gpus 2 exercises the relaunch,
    # weight broadcast, sharding, detection gather and max-over-ranks timing end to end
    gpu = 0 if os.environ.get("DNN_BENCH_SHARED_GPU") == "1" else local_rank
    backend = os.environ.get("DNN_BENCH_BACKEND", "nccl")
    torch.cuda.set_device(gpu)
    dev = torch.device("cuda", gpu)
    # under torch.distributed.run (any world size, including 1) the process group exists and
    # every collective below runs over it; a plain `python bench.py` runs without one
    distributed = world > 1 or "TORCHELASTIC_RUN_ID" in os.environ or os.environ.get("DNN_BENCH_DIST") == "1"
    if distributed:
        D.init(backend, device=dev)

    B = args.batch
    # rank 0 holds the weights; the other ranks only lay the plan out (zero weights of the
    # right shapes, no generator run) and receive the packed buffer by broadcast
    ws = synth.yolo_weights() if rank == 0 else synth.yolo_zero_weights()
    g, _ = yolo_graph.build_graph(dnn_hip.DnnGraphBuilder, ws, in_shape=(B, 416, 416, 3))
    entries = dnn_hip.lower_graph(g)
    wbytes, sbytes = dnn_hip.Plan.memory(B, (416, 416, 3), entries, precision=args.precision)
    wbuf = torch.empty(wbytes, dtype=torch.uint8, device=dev)
    sbuf = torch.empty(max(sbytes, 1), dtype=torch.uint8, device=dev)
    plan = dnn_hip.Plan(B, (416, 416, 3), entries, device=gpu, weights_ptr=wbuf.data_ptr(),
                        workspace_ptr=sbuf.data_ptr(), upload=(rank == 0), precision=args.precision)
    torch.cuda.synchronize()
    D.broadcast_weights(wbuf, src=0)
    torch.cuda.synchronize()

    gen = torch.Generator(device=dev)
    gen.manual_seed(1234 + rank)
    frames = torch.rand((B, 416, 416, 3), generator=gen, device=dev, dtype=torch.float32)
    # the run stream: a high-priority stream has a hardware queue of its own, so no RCCL,
    # postprocess or gather stream can share its queue and serialise with the forwards
    # (tools/stream_queue_probe.py: the null stream shares a queue with torch pool streams
    # once RCCL has taken its own)
    run_stream = torch.cuda.Stream(dev, priority=-1)
    run_stream.wait_stream(torch.cuda.current_stream(dev))
    torch.cuda.set_stream(run_stream)
    stream = run_stream.cuda_stream

    def compute(inp, out, n):
        plan.run_device(n, inp.data_ptr(), out.data_ptr(), stream)

    # each step's postprocess runs beside the NEXT forward's conv7 (a plan mark right before it):
    # conv7's 248 one-per-CU workgroups leave 8 CUs idle for 0.7 ms, where the postprocess's 64
    # workgroups (137 KB of LDS each, one per CU) fit, instead of taking 64 CUs from conv0 / conv1.
    # DNN_BENCH_POST_AT=end: right after its own forward; or another kernel name
    post_at = os.environ.get("DNN_BENCH_POST_AT", "conv7.gemm")
    post_after = None
    if args.gather == "detections" and post_at != "end" and post_at in [k["name"] for k in plan.kernels()]:
        plan.set_mark(post_at)
        post_after = plan.wait_mark
    runner = D.ShardedRunner(compute, B * world, (416, 416, 3), (13, 13, 125), dev,
                             timing=os.environ.get("DNN_BENCH_STEP_EVENTS", "1") == "1",
                             gather_mode=os.environ.get("DNN_BENCH_GATHER_MODE", "deferred"), post_after=post_after)
    if args.gather == "detections":
        import yolo_post
        dbufs = [yolo_post.DetectionBuffers(runner.shard_cap, dev) for _ in range(runner.slots)]
        dbuf = dbufs[0]

        last_out = [None]  # the output slot of the latest step whose postprocess was enqueued

        def post(out, n, slot, post_stream):
            last_out[0] = out
            dbufs[slot].run(out.data_ptr(), n, post_stream)
            return dbufs[slot].pack(n, post_stream)

        # runner.inflight (3) steps in flight: steps k+1 and k+2 are enqueued before step k's
        # detections are gathered (side stream) and collected, so gathers, D2H and rank 0's
        # wait overlap the GPU's work; every step is collected before the clock stops
        # ("deferred" gather mode: one more output slot, the gather completing a step later)
        pending = []

        def one_step():
            pending.append(runner.launch_detections(frames, post, one_step.k % runner.slots))
            one_step.k += 1
            return runner.finish_detections(pending.pop(0)) if len(pending) == runner.inflight else None

        one_step.k = 0

        def drain():
            r = None
            while pending:
                r = runner.finish_detections(pending.pop(0)) or r
            return runner.flush_detections() or r
    else:
        def one_step():
            return runner.step(frames)

        def drain():
            return None

    for _ in range(args.warmup):
        one_step()
    drain()
    torch.cuda.synchronize()
    if distributed:
        tdist.barrier()

    def steps_for(seconds):
        """Step count that fills `seconds` at the current per-step time (5 probe steps; the max
        over ranks, so every rank runs the same number of collective-bearing steps)."""
        if seconds <= 0:
            return 0
        t = time.perf_counter()
        for _ in range(5):
            one_step()
        drain()
        torch.cuda.synchronize()
        per = (time.perf_counter() - t) / 5
        n = torch.tensor([int(seconds / max(per, 1e-5)) + 1], dtype=torch.int64, device=dev)
        if distributed:
            tdist.all_reduce(n, op=tdist.ReduceOp.MAX)
        return int(n.item())

    # pre-heat: >= --preheat seconds of back-to-back steps, so the timed steps run at the clock the
    # chip holds under sustained load rather than at an early-clock rate
    t_pre = time.perf_counter()
    n_pre = steps_for(args.preheat)
    for _ in range(n_pre):
        one_step()
    drain()
    torch.cuda.synchronize()
    preheat_s = time.perf_counter() - t_pre
    if distributed:
        tdist.barrier()
    if args.gather == "detections":
        runner.reset_stats()

    # HIP events around the dominant kernel only (an event packet between every kernel costs
    # the step ~1 %); --kernels: around every kernel, for the per-kernel table.  Two clock-stamp
    # launches on the run stream bracket the timed forwards (the shader clock over the region)
    # (--full only: a plain run puts nothing but the steps themselves into the timed region)
    if args.full:
        clk = torch.zeros((2, CLOCK_WGS, 4), dtype=torch.int64, device=dev)
        dnn_hip.clock_stamp(clk[0].data_ptr(), CLOCK_WGS, stream)  # (first launch outside the timed region)
        plan.timing_begin(args.steps, only=None if args.kernels else DOMINANT)
    torch.cuda.synchronize()
    if distributed:
        tdist.barrier()
    t0 = time.perf_counter()
    if args.full:
        dnn_hip.clock_stamp(clk[0].data_ptr(), CLOCK_WGS, stream)
    last = None  # what the latest finished step returned on rank 0
    for _ in range(args.steps):
        r = one_step()
        last = r if r is not None else last
    if args.full:
        dnn_hip.clock_stamp(clk[1].data_ptr(), CLOCK_WGS, stream)
    r = drain()
    last = r if r is not None else last
    torch.cuda.synchronize()
    if distributed:
        tdist.barrier()
    elapsed = time.perf_counter() - t0
    if rank == 0 and args.dump_outputs:
        # now, before any later measurement reuses the output slots: the last timed step's result
        if args.gather == "detections":
            dets_f, counts_f = detections_as_float(*last)
            dump_outputs(args.dump_outputs, {"detections": dets_f, "counts": counts_f,
                                             "outputs": last_out[0][:runner.count].cpu().numpy()})
        else:
            dump_outputs(args.dump_outputs, {"outputs": last.cpu().numpy()})
    if args.full:
        ms_dom, cnt_dom = plan.timing_end()
        if args.kernels:
            ms, cnt = ms_dom, cnt_dom
        else:  # per-kernel table from 5 forwards after the timed region (events around every kernel)
            plan.timing_begin(5)
            for _ in range(5):
                compute(frames, runner.out, B)
            ms, cnt = plan.timing_end()
            kidx = [k["name"] for k in plan.kernels()].index(DOMINANT)
            ms[kidx], cnt[kidx] = ms_dom[kidx], cnt_dom[kidx]  # the dominant kernel: timed-region events
    # per-rank breakdown of the timed steps (means per step, ms), gathered to every rank
    keys = ("wall_ms", "forward_ms", "post_ms", "gather_ms", "gather_span_ms", "host_blocked_ms")
    st = runner.stats() if args.gather == "detections" else {}
    mine = [elapsed / args.steps * 1e3] + [float(st.get(k, float("nan"))) for k in keys[1:]]
    per_rank = [mine]
    if distributed:
        t = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        tdist.all_reduce(t, op=tdist.ReduceOp.MAX)
        elapsed = float(t.item())
        parts = [torch.zeros(len(keys), dtype=torch.float64, device=dev) for _ in range(world)]
        tdist.all_gather(parts, torch.tensor(mine, dtype=torch.float64, device=dev))
        per_rank = [p.tolist() for p in parts]

    # sustained: >= --sustained seconds of steps right after the timed region (same loop, events
    # around the dominant kernel only): the steady-state rate the headline must match
    sustained = None
    n_sus = steps_for(args.sustained) if args.full else 0
    if n_sus:
        if distributed:
            tdist.barrier()
        plan.timing_begin(n_sus, only=DOMINANT)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for _ in range(n_sus):
            one_step()
        drain()
        torch.cuda.synchronize()
        if distributed:
            tdist.barrier()
        el_sus = time.perf_counter() - t1
        ms_sus, cnt_sus = plan.timing_end()
        if distributed:
            t = torch.tensor([el_sus], dtype=torch.float64, device=dev)
            tdist.all_reduce(t, op=tdist.ReduceOp.MAX)
            el_sus = float(t.item())
        kidx = [k["name"] for k in plan.kernels()].index(DOMINANT)
        sustained = {"steps": n_sus, "seconds": round(el_sus, 3),
                     "images_per_s": round(B * world * n_sus / el_sus, 2),
                     "ms_per_step": round(el_sus / n_sus * 1e3, 4),
                     "dominant_kernel": DOMINANT,
                     "dominant_avg_launch_ms": round(ms_sus[kidx] / max(cnt_sus[kidx], 1), 4),
                     "preheat_steps": n_pre, "preheat_seconds": round(preheat_s, 3)}

    # the dominant kernel's own shader clock: clock stamps right before and after it in each of
    # a few further steps (outside its HIP-event window; a separate window, so the stamp launches
    # never touch the timed or sustained steps)
    clk_region = clk_kernel = post_ms = None
    if args.full:
        clk_region = dnn_hip.sclk_from_stamps(clk[0].cpu().numpy(), clk[1].cpu().numpy())
        n_clk = 20
        kbuf = torch.zeros((n_clk, 2, CLOCK_WGS, 4), dtype=torch.int64, device=dev)
        plan.clock_begin(DOMINANT, kbuf.data_ptr(), n_clk, CLOCK_WGS)
        for _ in range(n_clk):
            one_step()
        drain()
        torch.cuda.synchronize()
        runs_clk = plan.clock_end()
        kb = kbuf.cpu().numpy()
        per_run = [dnn_hip.sclk_from_stamps(kb[i, 0], kb[i, 1]) for i in range(runs_clk)]
        per_run = [c for c in per_run if c]
        if per_run:
            med = lambda v: sorted(v)[len(v) // 2]
            clk_kernel = {"mean": med([c["mean"] for c in per_run]), "min": med([c["min"] for c in per_run]),
                          "max": med([c["max"] for c in per_run]), "runs": len(per_run),
                          "window_us": med([c["window_us"] for c in per_run]),
                          "per_xcd": {str(x): round(med([c["per_xcd"][x] for c in per_run if x in c["per_xcd"]]), 4)
                                      for x in per_run[0]["per_xcd"]}}

        if args.gather == "detections":  # the postprocess kernel alone, for the per-kernel table
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(10):
                dbuf.run(runner.out.data_ptr(), runner.count, stream)
            e1.record()
            torch.cuda.synchronize()
            post_ms = e0.elapsed_time(e1) / 10
    x3 = False
    if rank == 0:
        if args.gather == "detections":
            dets_u8, counts = last
            assert len(counts) == B * world
            n_det = int(np.clip(counts, 0, None).sum())
            if args.dump_detections:
                np.savez(args.dump_detections, dets=np.ascontiguousarray(dets_u8), counts=np.asarray(counts))
        else:
            assert last is not None and last.shape[0] == B * world
        # the x3 conv (default for conv6/conv7 on the fp32 path) executes 6 bf16 MFMA products
        # per fp32 product
        desc = plan.describe().splitlines()
        dom_layer = [ln for ln in desc if ln.startswith("conv")][int(DOMINANT[4:DOMINANT.index(".")])]
        x3 = "patch_x3" in dom_layer
        value = timed_value = B * world * args.steps / elapsed
        value_source = f"{args.steps} timed steps after a {preheat_s:.1f} s pre-heat"
        stable = None  # (--full: whether the sustained window agrees with the timed steps)
        if sustained:
            stable = True
            if abs(value - sustained["images_per_s"]) > 0.02 * sustained["images_per_s"]:
                # the two windows disagree: the run is marked unstable, and the headline is the LOWER of
                # the two rates (a faster sustained window never replaces the timed one)
                stable = False
                if sustained["images_per_s"] < value:
                    value = sustained["images_per_s"]
                    value_source = (f"sustained ({sustained['steps']} steps): more than 2 % below the "
                                    f"{args.steps} timed steps, the lower of the two")
                else:
                    value_source += " (the sustained window ran more than 2 % faster; the timed value is kept)"
        res = {
            "metric": "YOLOv2-tiny 416×416 images/sec at 1/2/4/8 GPU; conv MFMA % of fp32 peak",
            "value": round(value, 2),
            "unit": "images/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(elapsed / args.steps * 1e3, 4),  # one timed step (max over ranks)
            "value_source": value_source,
            "timed_value": round(timed_value, 2),
            "stable": stable,
            "sustained": sustained,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": ("fp32 (conv1-conv8: fp32 operands split exactly into 3 bf16 pieces, 6 bf16 MFMA "
                      "products, fp32 accumulate; error <= the fp32 MFMA path's; conv0: fp32 MFMA)"
                      if x3 else args.precision),
            "data": "synthetic (uniform [0,1) frames, random-init weights, tiny-yolo-voc channel plan)",
            "config": {"workload": "YOLOv2-tiny forward, 416x416x3 NHWC fp32, 64 frames per GPU in HBM, "
                                   + ("on-GPU postprocessing (decode, 0.3 threshold, sort, NMS), post-NMS "
                                      "detections gathered to rank 0" if args.gather == "detections"
                                      else "raw outputs gathered to rank 0"),
                       "model": "yolov2-tiny (9 conv, 6 maxpool)", "global_batch": B * world,
                       "per_gpu_batch": B, "seq_len": None, "parallelism": f"dp{world}"},
            "full": args.full,
            "dist_backend": ("rccl" if backend == "nccl" else backend) if distributed else None,
            "per_rank": [dict(rank=r, **{k: (round(v, 4) if v == v else None) for k, v in zip(keys, vals)})
                         for r, vals in enumerate(per_rank)],
        }
        if args.gather == "detections":
            res["postprocess"] = {"detections_last_step": n_det,
                                  "gathered_bytes_last_step": int(dets_u8.nbytes + counts.nbytes)}
    if rank == 0 and args.full:
        kinfo = plan.kernels()
        by_name = {k["name"]: (k, ms[i], cnt[i]) for i, k in enumerate(kinfo)}
        k, kms, kc = by_name[DOMINANT]
        avg_s = kms / max(kc, 1) / 1e3
        # the x3 conv's roofline is the bf16 MFMA peak over the executed flops
        mult, peak = (X3_PRODUCTS, BF16_MFMA_PEAK_TFLOPS) if x3 else (1, FP32_MFMA_PEAK_TFLOPS)
        if args.precision == "fp16":  # (config 5 as the main line: one fp16 MFMA product per product)
            mult, peak = 1, FP16_MFMA_PEAK_TFLOPS
        achieved = mult * k["flops"] / avg_s / 1e12
        prof = pmc_entry(DOMINANT, "pmc_summary_fp16.json" if args.precision == "fp16" else "pmc_summary.json")
        traffic = prof.get("hbm_bytes_per_launch")
        # split-K layers (conv6/conv7) finish in a separate ordered reduce + epilogue kernel:
        # the conv-level figures below charge its time to the GEMM
        red = by_name.get(DOMINANT.replace(".gemm", ".reduce"))
        red_s = red[1] / max(red[2], 1) / 1e3 if red else 0.0
        mfma = (".gemm", ".patch", ".reduce")  # the MFMA conv kernels (+ their split-K reduces)
        gemm_fl = sum(v[0]["flops"] for n, v in by_name.items() if n.endswith(mfma))
        gemm_s = sum(v[1] / max(v[2], 1) for n, v in by_name.items() if n.endswith(mfma)) / 1e3
        conv67 = [by_name[n] for n in ("conv6.gemm", "conv6.reduce", "conv7.gemm", "conv7.reduce") if n in by_name]
        c67_fl = sum(v[0]["flops"] for v in conv67)
        c67_s = sum(v[1] / max(v[2], 1) for v in conv67) / 1e3
        total_kernel_ms = sum(m / max(c, 1) for m, c in zip(ms, cnt))
        res.update({
            "roofline": {"kernel": DOMINANT, "bound": "mfma", "achieved": round(achieved, 2),
                         "peak": peak, "unit": "TFLOP/s", "frac": round(achieved / peak, 4), "traffic": traffic,
                         "mfma": ("v_mfma_f32_16x16x32_bf16, executed flops = 6 x algorithmic (x3 splits)" if x3
                                  else "v_mfma_f32_32x32x2f32"),
                         "algorithmic_fp32_tflops": round(k["flops"] / avg_s / 1e12, 2),
                         "algorithmic_bytes": int(k["bytes"]),
                         "traffic_over_algorithmic": round(traffic / k["bytes"], 2) if traffic else None,
                         "flops_per_launch": k["flops"], "avg_launch_ms": round(avg_s * 1e3, 4),
                         "duration_source": "HIP events on the run stream around each launch, timed region",
                         "rocprof_avg_launch_ms": round(prof["avg_us"] / 1e3, 4) if prof.get("avg_us") else None,
                         "rocprof_frac": round(mult * k["flops"] / (prof["avg_us"] / 1e6) / 1e12 / peak, 4)
                         if prof.get("avg_us") else None,
                         "rocprof_source": ("profiles/pmc_summary.json: rocprofv3 --kernel-trace of bench.py on "
                                            "the profile box, whose own HIP-event duration and img/s the file "
                                            "records beside it (`same_box`); boxes differ by up to ~8 % in "
                                            "clock, so this frac and `frac` come from different boxes"),
                         "rocprof_same_box": prof.get("same_box"),
                         "with_reduce_achieved": round(mult * k["flops"] / (avg_s + red_s) / 1e12, 2),
                         "reduce_ms": round(red_s * 1e3, 4),
                         # the measured shader clock (clock.hip stamps) and the fraction against
                         # the peak at that clock: peak x sclk / 2.4 GHz
                         "sclk_ghz": round(clk_kernel["mean"], 4) if clk_kernel else None,
                         "sclk_ghz_xcd_min": round(clk_kernel["min"], 4) if clk_kernel else None,
                         "sclk_ghz_xcd_max": round(clk_kernel["max"], 4) if clk_kernel else None,
                         "sclk_ghz_per_xcd": clk_kernel["per_xcd"] if clk_kernel else None,
                         "sclk_ghz_timed_region": round(clk_region["mean"], 4) if clk_region else None,
                         "frac_at_measured_clock": round(achieved / (peak * clk_kernel["mean"] / NOMINAL_SCLK_GHZ), 4)
                         if clk_kernel else None,
                         "sclk_source": (f"s_memtime / s_memrealtime stamps (one workgroup per CU) right before "
                                         f"and after {DOMINANT} in {clk_kernel['runs'] if clk_kernel else 0} "
                                         "steps after the sustained window, per XCD, median over steps; "
                                         "sclk_ghz = the mean over XCDs; sclk_ghz_timed_region: stamps "
                                         "bracketing the timed steps; nominal 2.4 GHz")},
            # ALGORITHMIC fp32 flops over the fp32 MFMA peak: the x3 layers exceed 100 % by running on
            # the bf16 MFMA, so this is a speed figure, not an MFMA utilisation (that is `roofline`
            # for the dominant kernel, and `fp32_mfma` for the fp32-MFMA-only plan)
            "fp32_equivalent_pct": {"all_gemms_pct_fp32_peak": round(100 * gemm_fl / gemm_s / 1e12 / FP32_MFMA_PEAK_TFLOPS, 2),
                          "conv6_conv7_pct_fp32_peak": round(100 * c67_fl / c67_s / 1e12 / FP32_MFMA_PEAK_TFLOPS, 2),
                          "net_pct_fp32_peak": round(100 * 6.971e9 * value / world / 1e12 / FP32_MFMA_PEAK_TFLOPS,
                                                     2)},
            "kernel_ms_per_step": round(total_kernel_ms, 4),
            "kernel_timing": ("HIP events around every kernel in the timed region" if args.kernels else
                              f"{DOMINANT}: HIP events around it in the timed region; the other kernels: "
                              "5 forwards after it, events around every kernel"),
        })
        if args.gather == "detections":
            res["postprocess"]["ms"] = round(post_ms, 4)
        if args.kernels:
            res["kernels"] = {n: {"ms": round(v[1] / max(v[2], 1), 4),
                                  "tflops": round(v[0]["flops"] / (v[1] / max(v[2], 1) / 1e3) / 1e12, 2)
                                  if v[0]["flops"] else None,
                                  "gbs": round(v[0]["bytes"] / (v[1] / max(v[2], 1) / 1e3) / 1e9, 1)}
                              for n, v in by_name.items()}

    extras = rank == 0 and world == 1 and args.full  # single-GPU measurements beside the headline
    if extras and not args.no_latency:
        lat = latency_b1(dnn_hip, yolo_graph, ws, dev)
        inv = latency_b1(dnn_hip, yolo_graph, ws, dev, latency=False)
        yb = torch.empty((B, 13, 13, 125), device=dev)
        plan.run_device(1, lat["_x"].data_ptr(), yb.data_ptr(), stream)
        torch.cuda.synchronize()
        lat["normwise_err_vs_batch_plan"] = float((lat.pop("_y") - yb[:1]).abs().max() / yb[:1].abs().max())
        lat.pop("_x")
        lat["batch_plan_at_batch1"] = inv
        res["latency_b1"] = lat
    if extras and not args.no_e2e:
        res["end_to_end_host_frames"] = end_to_end(plan, B, dev, stream)
    if extras and args.precision == "fp32" and not args.no_unfused:
        res["unfused"] = unfused_im2col(dnn_hip, yolo_graph, ws, dev, frames, stream, B)
    if extras and args.precision == "fp32" and not args.no_fp32_mfma and x3:
        res["fp32_mfma"] = fp32_mfma_config(dnn_hip, yolo_graph, ws, dev, frames, runner.out, stream, B)
    if extras and args.precision == "fp32" and not args.no_fp16:
        res["fp16"] = fp16_config(dnn_hip, yolo_graph, ws, dev, frames, runner.out, plan, stream, B)
    if rank == 0 and args.full:
        res["cpu_baseline"] = None if (world > 1 or args.no_cpu) else cpu_baseline(args.cpu_seconds)
    if rank == 0:
        print(json.dumps(res), flush=True)

    plan.close()
    if distributed:
        tdist.destroy_process_group()


if __name__ == "__main__":
    main()
