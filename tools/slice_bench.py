#!/usr/bin/env python3
"""Slice kernel against a device-to-device copy of the same size (needs an MI355X).

Shape: the split of YOLOv4-tiny's first CSP block at batch 64: [64, 104, 104, 64] sliced to channels
32..63, out = 64 x 104 x 104 x 32: 88.6 MB read and 88.6 MB written.  The yardstick is
hipMemcpyAsync(device to device) of the output's byte count: the slice moves the same bytes but
reads them in 128-byte runs, every other one of the input.  Bar: slice <= 1.25 x memcpy, the route
kernel's bar (tools/route_bench.py): the same kind of kernel against the same yardstick.

The slice runs as the only entry of a plan, on the caller's tensors, and is timed with the plan's
own HIP events (dnn_plan_timing_begin_only); the copy is timed with HIP events on the same stream,
in the same process.  5 warm-ups, then the median of 20, the two arms interleaved.

    python tools/slice_bench.py [--out profiles/slice_bench.json]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "dnn-inference-engine_amd"))

import torch  # noqa: E402

import dnn_hip  # noqa: E402

B, H, W, C, FIRST, CHANNELS = 64, 104, 104, 64, 32, 32
WARMUP, RUNS = 5, 20
BAR = 1.25


def hip_runtime():
    for name in ("libamdhip64.so.7", "libamdhip64.so"):  # the runtime torch already loaded, by SONAME
        try:
            lib = ctypes.CDLL(name)
        except OSError:
            continue
        lib.hipMemcpyAsync.restype = ctypes.c_int
        lib.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
        return lib
    raise RuntimeError("no HIP runtime found")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "slice_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "slice_bench needs a GPU"
    dev = torch.device("cuda", 0)
    plan = dnn_hip.Plan(B, (H, W, C), [dnn_hip.SliceEntry(FIRST, CHANNELS)], device=0)
    names = [k["name"] for k in plan.kernels()]
    assert names == ["slice0"], names
    out_shape = (B, H, W, CHANNELS)
    assert plan.out_shape == out_shape[1:], plan.out_shape
    d_in = torch.rand((B, H, W, C), device=dev)
    d_out = torch.empty(out_shape, device=dev)
    src = torch.rand(out_shape, device=dev)
    dst = torch.empty(out_shape, device=dev)
    nbytes = d_out.numel() * 4
    hip = hip_runtime()
    stream = torch.cuda.Stream(dev)
    slice_ms, copy_ms = [], []
    with torch.cuda.stream(stream):
        for i in range(WARMUP + RUNS):
            plan.timing_begin(1, only="slice0")
            plan.run_device(B, d_in.data_ptr(), d_out.data_ptr(), stream.cuda_stream)
            ms, cnt = plan.timing_end()
            assert cnt[0] == 1
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            rc = hip.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), nbytes, 3, stream.cuda_stream)  # 3: device to device
            assert rc == 0, rc
            e1.record(stream)
            e1.synchronize()
            if i >= WARMUP:
                slice_ms.append(ms[0])
                copy_ms.append(e0.elapsed_time(e1))
    # the slice's result, once, against torch on the same device
    assert torch.equal(d_out, d_in[..., FIRST:FIRST + CHANNELS]), "slice output differs from torch's slicing"
    assert torch.equal(dst, src)
    s, c = statistics.median(slice_ms), statistics.median(copy_ms)
    res = {
        "what": "slice kernel (YOLOv4-tiny's first CSP split, batch 64) vs hipMemcpyAsync device-to-device of the "
                "output's bytes",
        "in": [B, H, W, C], "first": FIRST, "channels": CHANNELS, "out": list(out_shape),
        "bytes_read": nbytes, "bytes_written": nbytes,
        "method": f"HIP events, same process and stream, {WARMUP} warm-ups, median of {RUNS}, arms interleaved; "
                  "the slice is the only kernel of a plan on the caller's tensors",
        "slice_ms": s, "memcpy_ms": c, "ratio": s / c, "bar": BAR, "within_bar": s <= BAR * c,
        "slice_GBps": 2 * nbytes / s / 1e6, "memcpy_GBps": 2 * nbytes / c / 1e6,
        "slice_ms_min_max": [min(slice_ms), max(slice_ms)], "memcpy_ms_min_max": [min(copy_ms), max(copy_ms)],
        "device": torch.cuda.get_device_name(0),
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
    plan.close()


if __name__ == "__main__":
    main()
