#!/usr/bin/env python3
"""The letterbox ingest kernel against the stretch kernel and a plain copy (needs an MI355X).

Shape: 64 frames of 480 x 640 x 3 uint8 into [64, 416, 416, 3] fp32.  Three arms on the same
buffers, in the same process and on the same stream:

  letterbox   dnn_letterbox_frames (csrc/letterbox.hip): 64 descriptors, one launch
  stretch     dnn_preprocess_frames (csrc/ingest.hip) on the same frames and output size
  copy        a device-to-device hipMemcpyAsync (torch's copy_) of as many bytes as the letterbox
              kernel reads and writes together: (in + out) / 2 bytes read and as many written

and the box correction, dnn_yolo_correct_detections, on 64 x max_det rows with every count at
max_det (max_det = 10647, a 416 x 416 YOLOv3's boxes).

Each figure is the median over `rounds` of the device time of one call: HIP events around `reps`
back-to-back calls on one stream, after a warm-up round, the arms interleaved per round; the
shader clock is stamped around the whole timed region (csrc/clock.hip).  The letterbox kernel's
bytes are the frames read once (59 MB) plus the output written once (133 MB); the source rows it
reads twice come from cache.  The letterbox output is checked once against
tests/letterbox_oracle.py on frame 0, bit for bit.

    python tools/letterbox_bench.py [--reps 20] [--rounds 5] [--out profiles/letterbox_bench.json]
"""
import argparse
import json
import os
import socket
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "dnn-inference-engine_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import dnn_hip  # noqa: E402
import ingest  # noqa: E402
import yolo_post  # noqa: E402

N, H, W, NET = 64, 480, 640, (416, 416)
MAX_DET = 10647


def timed(fn, reps, stream):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    for _ in range(reps):
        fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "letterbox_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "letterbox_bench needs a GPU"
    import letterbox_oracle as LB
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    frames_np = rng.integers(0, 256, size=(N, H, W, 3), dtype=np.uint8)
    px = torch.from_numpy(frames_np).to(dev)
    out = torch.empty((N,) + NET + (3,), dtype=torch.float32, device=dev)
    in_bytes, out_bytes = px.numel(), out.numel() * 4
    half = (in_bytes + out_bytes) // 2
    c_src = torch.empty(half, dtype=torch.uint8, device=dev)
    c_dst = torch.empty(half, dtype=torch.uint8, device=dev)
    desc = (ingest.Frame * N)(*[ingest.Frame(k * H * W * 3, H, W) for k in range(N)])
    dets = torch.zeros((N, MAX_DET, 40), dtype=torch.uint8, device=dev)
    counts = torch.full((N,), MAX_DET, dtype=torch.int32, device=dev)
    sizes = yolo_post._sizes([(H, W)] * N)
    stream = torch.cuda.Stream(dev)
    s = stream.cuda_stream
    clk = torch.zeros((2, 256, 4), dtype=torch.int64, device=dev)

    arms = {
        "letterbox": lambda: ingest.letterbox_device(px.data_ptr(), in_bytes, desc, N, out.data_ptr(), s, NET),
        "stretch": lambda: ingest.preprocess_device(px.data_ptr(), N, H, W, out.data_ptr(), s, NET),
        "copy": lambda: c_dst.copy_(c_src, non_blocking=True),
        "correct": lambda: dnn_hip._check(yolo_post._lib.dnn_yolo_correct_detections(
            dets.data_ptr(), counts.data_ptr(), N, MAX_DET, sizes, NET[0], NET[1], s), "dnn_yolo_correct_detections"),
    }
    ms = {k: [] for k in arms}
    with torch.cuda.stream(stream):
        for r in range(a.rounds + 1):
            if r == 1:
                dnn_hip.clock_stamp(clk[0].data_ptr(), 256, s)
            for k, fn in arms.items():
                t = timed(fn, a.reps, stream)
                if r:
                    ms[k].append(t)
        dnn_hip.clock_stamp(clk[1].data_ptr(), 256, s)
        arms["letterbox"]()
    stream.synchronize()
    assert np.array_equal(out[0].cpu().numpy(), LB.letterbox_f32(frames_np[0], NET[0], NET[1])), \
        "the letterbox output differs from the oracle"
    c = dnn_hip.sclk_from_stamps(clk[0].cpu().numpy(), clk[1].cpu().numpy())
    med = {k: statistics.median(v) for k, v in ms.items()}
    res = {
        "what": f"{N} frames of {H} x {W} x 3 uint8 -> [{N}, {NET[0]}, {NET[1]}, 3] fp32: dnn_letterbox_frames vs "
                "dnn_preprocess_frames (the stretch; unchanged code) vs a device-to-device copy of the same bytes; "
                f"dnn_yolo_correct_detections on {N} x {MAX_DET} rows, every count at max_det",
        "method": f"HIP events around {a.reps} back-to-back calls, one warm-up round, median of {a.rounds} rounds, "
                  "arms interleaved per round, same process, stream and buffers; one machine, one run",
        "letterbox_bytes": {"read": in_bytes, "written": out_bytes},
        "copy_bytes": {"read": half, "written": half},
        "us": {k: round(v * 1e3, 2) for k, v in med.items()},
        "us_min_max": {k: [round(min(v) * 1e3, 2), round(max(v) * 1e3, 2)] for k, v in ms.items()},
        "letterbox_GBps": round((in_bytes + out_bytes) / med["letterbox"] / 1e6, 1),
        "stretch_GBps": round((in_bytes + out_bytes) / med["stretch"] / 1e6, 1),
        "copy_GBps": round(2 * half / med["copy"] / 1e6, 1),
        "letterbox_over_copy": round(med["letterbox"] / med["copy"], 3),
        "letterbox_over_stretch": round(med["letterbox"] / med["stretch"], 3),
        "correct_rows": N * MAX_DET,
        "shader_clock_GHz": round(c["mean"], 3) if c else None,
        "device": torch.cuda.get_device_name(0),
        "box": socket.gethostname(),
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
