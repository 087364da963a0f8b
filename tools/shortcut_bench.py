#!/usr/bin/env python3
"""Shortcut and upsample kernels against a device-to-device copy (needs an MI355X).

Cases, all at batch 64:
    shortcut  208 x 208 x 64     (708.8 MB per tensor: HBM-bound)
    shortcut  13 x 13 x 1024     (44.3 MB per tensor: resident in the 256 MB last-level cache)
    upsample  13 x 13 x 256, x2  (11.1 MB read, 44.3 MB written)

The yardstick is hipMemcpyAsync(device to device) of the output's byte count, which moves two
tensors of that size (one read, one written).  The project holds the route kernel to 1.25 x that
copy; per byte moved the same margin gives
    shortcut  three tensors where the copy moves two: <= 1.25 x 1.5 x memcpy
    upsample  <= 1.25 x memcpy (it reads a quarter and writes the whole)

Each kernel runs as an entry of a plan (shortcut: stash the input, a factor-1 upsample makes a
second tensor, shortcut, release; upsample: the plan's only entry) and is timed alone with the
plan's own HIP events (dnn_plan_timing_begin_only); the copy is timed with HIP events on the same
stream, in the same process.  5 warm-ups, then the median of 20, the two arms interleaved.

    python tools/shortcut_bench.py [--out profiles/shortcut_bench.json]
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

B = 64
WARMUP, RUNS = 5, 20
ROUTE_BAR = 1.25
CASES = (
    # name, kernel, input shape, factor, tensors moved relative to the copy's two
    ("shortcut_208x208x64", "shortcut0", (208, 208, 64), 1, 1.5),
    ("shortcut_13x13x1024", "shortcut0", (13, 13, 1024), 1, 1.5),
    ("upsample2_13x13x256", "upsample0", (13, 13, 256), 2, 1.0),
)


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


def run_case(hip, dev, stream, name, kernel, shape, factor, moved):
    E = dnn_hip
    if kernel == "shortcut0":
        entries = [E.StashEntry(0), E.UpsampleEntry(1), E.ShortcutEntry(0), E.ReleaseEntry(0)]
    else:
        entries = [E.UpsampleEntry(factor)]
    plan = E.Plan(B, shape, entries, device=0)
    names = [k["name"] for k in plan.kernels()]
    kidx = names.index(kernel)
    out_shape = (B, shape[0] * factor, shape[1] * factor, shape[2])
    assert plan.out_shape == out_shape[1:], plan.out_shape
    d_in = torch.rand((B,) + tuple(shape), device=dev)
    d_out = torch.empty(out_shape, device=dev)
    src = torch.rand(out_shape, device=dev)
    dst = torch.empty(out_shape, device=dev)
    nbytes = d_out.numel() * 4
    k_ms, c_ms = [], []
    with torch.cuda.stream(stream):
        for i in range(WARMUP + RUNS):
            plan.timing_begin(1, only=kernel)
            plan.run_device(B, d_in.data_ptr(), d_out.data_ptr(), stream.cuda_stream)
            ms, cnt = plan.timing_end()
            assert cnt[kidx] == 1
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            rc = hip.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), nbytes, 3, stream.cuda_stream)  # 3: device to device
            assert rc == 0, rc
            e1.record(stream)
            e1.synchronize()
            if i >= WARMUP:
                k_ms.append(ms[kidx])
                c_ms.append(e0.elapsed_time(e1))
    # the result, once, against torch on the same device
    if kernel == "shortcut0":
        assert torch.equal(d_out, d_in + d_in), "shortcut output differs from torch's x + x"
        bytes_moved = 3 * nbytes
    else:
        want = d_in.repeat_interleave(factor, dim=1).repeat_interleave(factor, dim=2)
        assert torch.equal(d_out, want), "upsample output differs from torch's repeat_interleave"
        bytes_moved = nbytes + d_in.numel() * 4
    assert torch.equal(dst, src)
    plan.close()
    k, c = statistics.median(k_ms), statistics.median(c_ms)
    bar = ROUTE_BAR * moved
    return {
        "case": name, "kernel": kernel, "in": [B] + list(shape), "out": list(out_shape), "factor": factor,
        "bytes_moved": bytes_moved, "memcpy_bytes_moved": 2 * nbytes,
        "kernel_ms": k, "memcpy_ms": c, "ratio": k / c, "bar": bar, "within_bar": k <= bar * c,
        "kernel_GBps": bytes_moved / k / 1e6, "memcpy_GBps": 2 * nbytes / c / 1e6,
        "kernel_ms_min_max": [min(k_ms), max(k_ms)], "memcpy_ms_min_max": [min(c_ms), max(c_ms)],
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "shortcut_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "shortcut_bench needs a GPU"
    dev = torch.device("cuda", 0)
    hip = hip_runtime()
    stream = torch.cuda.Stream(dev)
    res = {
        "what": "shortcut and upsample kernels (batch 64) vs hipMemcpyAsync device-to-device of the output's bytes",
        "method": f"HIP events, same process and stream, {WARMUP} warm-ups, median of {RUNS}, arms interleaved; "
                  "each kernel is an entry of a plan and is timed alone by the plan's own events",
        "bars": "the route's 1.25 x memcpy per byte moved: shortcut (three tensors to the copy's two) "
                "1.25 x 1.5, upsample 1.25",
        "device": torch.cuda.get_device_name(0),
        "cases": [run_case(hip, dev, stream, *c) for c in CASES],
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
