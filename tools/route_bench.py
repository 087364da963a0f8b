#!/usr/bin/env python3
"""Route kernel against a device-to-device copy of the same size (needs an MI355X).

Shape: the YOLOv2 join at batch 64: a = 64 x 26 x 26 x 64, b = 64 x 13 x 13 x 1024, block 2,
out = 64 x 13 x 13 x 1280: 55.4 MB read and 55.4 MB written.  The yardstick is
hipMemcpyAsync(device to device) of the output's byte count: the route moves the same bytes but
gathers them from two sources in 256-byte runs.  Bar: route <= 1.25 x memcpy.

The route runs as the last entry of a plan (stash the input, pool + 1x1 conv make b, stash,
restore, route) and is timed alone with the plan's own HIP events (dnn_plan_timing_begin_only);
the copy is timed with HIP events on the same stream, in the same process.  5 warm-ups, then the
median of 20, the two arms interleaved.

    python tools/route_bench.py [--out profiles/route_bench.json]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "dnn-inference-engine_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import dnn_hip  # noqa: E402

B, H, W, CA, CB, BLOCK = 64, 26, 26, 64, 1024, 2
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
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "route_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "route_bench needs a GPU"
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    g = dnn_hip.DnnGraphBuilder()
    x = g.create_input([B, H, W, CA])
    t = g.create_max_pool2d(x, [1, 2, 2, 1], [1, 2, 2, 1], "SAME")
    t = g.create_conv2d(t, (rng.standard_normal((1, 1, CA, CB)) * 0.1).astype(np.float32), [1, 1, 1, 1], "SAME")
    y = g.create_concat([g.create_space_to_depth(x, BLOCK), t])
    g.set_out_node(y)
    entries = dnn_hip.lower_graph(g)
    plan = dnn_hip.Plan(B, (H, W, CA), entries, device=0)
    names = [k["name"] for k in plan.kernels()]
    ridx = names.index("route0")
    out_shape = (B, H // BLOCK, W // BLOCK, BLOCK * BLOCK * CA + CB)
    assert plan.out_shape == out_shape[1:], plan.out_shape
    d_in = torch.rand((B, H, W, CA), device=dev)
    d_out = torch.empty(out_shape, device=dev)
    src = torch.rand(out_shape, device=dev)
    dst = torch.empty(out_shape, device=dev)
    nbytes = d_out.numel() * 4
    hip = hip_runtime()
    stream = torch.cuda.Stream(dev)
    route_ms, copy_ms = [], []
    with torch.cuda.stream(stream):
        for i in range(WARMUP + RUNS):
            plan.timing_begin(1, only="route0")
            plan.run_device(B, d_in.data_ptr(), d_out.data_ptr(), stream.cuda_stream)
            ms, cnt = plan.timing_end()
            assert cnt[ridx] == 1
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            rc = hip.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), nbytes, 3, stream.cuda_stream)  # 3: device to device
            assert rc == 0, rc
            e1.record(stream)
            e1.synchronize()
            if i >= WARMUP:
                route_ms.append(ms[ridx])
                copy_ms.append(e0.elapsed_time(e1))
    # the route's result, once, against torch on the same device
    a = d_in.reshape(B, H // BLOCK, BLOCK, W // BLOCK, BLOCK, CA).permute(0, 1, 3, 2, 4, 5).reshape(
        B, H // BLOCK, W // BLOCK, BLOCK * BLOCK * CA)
    assert torch.equal(d_out[..., :BLOCK * BLOCK * CA], a), "route output differs from torch's space_to_depth"
    assert torch.equal(dst, src)
    r, c = statistics.median(route_ms), statistics.median(copy_ms)
    res = {
        "what": "route kernel (YOLOv2 join, batch 64) vs hipMemcpyAsync device-to-device of the output's bytes",
        "a": [B, H, W, CA], "b": [B, H // BLOCK, W // BLOCK, CB], "block": BLOCK, "out": list(out_shape),
        "bytes_read": nbytes, "bytes_written": nbytes,
        "method": f"HIP events, same process and stream, {WARMUP} warm-ups, median of {RUNS}, arms interleaved; "
                  "the route is the last kernel of a plan (its pool and 1x1 conv run untimed before it)",
        "route_ms": r, "memcpy_ms": c, "ratio": r / c, "bar": BAR, "within_bar": r <= BAR * c,
        "route_GBps": 2 * nbytes / r / 1e6, "memcpy_GBps": 2 * nbytes / c / 1e6,
        "route_ms_min_max": [min(route_ms), max(route_ms)], "memcpy_ms_min_max": [min(copy_ms), max(copy_ms)],
        "device": torch.cuda.get_device_name(0),
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
    plan.close()


if __name__ == "__main__":
    main()
