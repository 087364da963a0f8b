#!/usr/bin/env python3
"""The element-wise activation kernel (csrc/activate.hip) against a device-to-device copy (needs an MI355X).

Cases, all at batch 64, for logistic, swish and mish:
    208 x 208 x 64     (708.8 MB per tensor: HBM-bound)
    13 x 13 x 1024     (44.3 MB per tensor: resident in the 256 MB last-level cache)

The yardstick is hipMemcpyAsync(device to device) of the tensor's byte count: like the kernel it reads one
tensor and writes one.  The project holds the route kernel to 1.25 x that copy; the same bar is reported here.

The kernel runs as the only entry of a plan (so it is the stand-alone form, not an epilogue) and is timed by
the plan's own HIP events (dnn_plan_timing_begin_only); the copy is timed with HIP events on the same stream,
in the same process.  5 warm-ups, then the median of 20, the two arms interleaved.  The result is checked once
against torch's float64 evaluation on the same device (a few ulp, the bound of tests/test_gpu_activation.py).

    python tools/activation_bench.py [--out profiles/activation_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "dnn-inference-engine_amd"))
sys.path.insert(0, os.path.join(REPO, "tools"))

import torch  # noqa: E402

import dnn_hip  # noqa: E402
from shortcut_bench import hip_runtime  # noqa: E402

B = 64
WARMUP, RUNS = 5, 20
BAR = 1.25
SHAPES = ((208, 208, 64), (13, 13, 1024))
REFERENCE = {"logistic": torch.sigmoid, "swish": lambda v: v * torch.sigmoid(v),
             "mish": lambda v: v * torch.tanh(torch.nn.functional.softplus(v, threshold=700))}


def run_case(hip, dev, stream, kind, shape):
    plan = dnn_hip.Plan(B, shape, [dnn_hip.ActivationEntry(kind)], device=0)
    assert [k["name"] for k in plan.kernels()] == ["activate0"] and plan.out_shape == shape
    d_in = torch.randn((B,) + shape, device=dev) * 3
    d_out, dst = torch.empty_like(d_in), torch.empty_like(d_in)
    nbytes = d_in.numel() * 4
    k_ms, c_ms = [], []
    with torch.cuda.stream(stream):
        for i in range(WARMUP + RUNS):
            plan.timing_begin(1, only="activate0")
            plan.run_device(B, d_in.data_ptr(), d_out.data_ptr(), stream.cuda_stream)
            ms, cnt = plan.timing_end()
            assert cnt[0] == 1
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            rc = hip.hipMemcpyAsync(dst.data_ptr(), d_in.data_ptr(), nbytes, 3, stream.cuda_stream)  # 3: device to device
            assert rc == 0, rc
            e1.record(stream)
            e1.synchronize()
            if i >= WARMUP:
                k_ms.append(ms[0])
                c_ms.append(e0.elapsed_time(e1))
    want = REFERENCE[kind](d_in[:4].double())
    err = ((d_out[:4].double() - want).abs() / want.abs().clamp_min(1e-30)).max().item() / 2.0 ** -23
    assert err < 8, f"{kind}: {err} ulp (relative) against float64"
    plan.close()
    k, c = statistics.median(k_ms), statistics.median(c_ms)
    return {"kind": kind, "shape": [B] + list(shape), "bytes_moved": 2 * nbytes, "kernel_ms": k, "memcpy_ms": c,
            "ratio": k / c, "bar": BAR, "within_bar": k <= BAR * c, "kernel_GBps": 2 * nbytes / k / 1e6,
            "memcpy_GBps": 2 * nbytes / c / 1e6, "kernel_ms_min_max": [min(k_ms), max(k_ms)],
            "memcpy_ms_min_max": [min(c_ms), max(c_ms)], "max_rel_err_in_2^-23": err}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "activation_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "activation_bench needs a GPU"
    dev = torch.device("cuda", 0)
    hip, stream = hip_runtime(), torch.cuda.Stream(dev)
    res = {
        "what": "the stand-alone activation kernel (batch 64) vs hipMemcpyAsync device-to-device of the same bytes",
        "method": f"HIP events, same process and stream, {WARMUP} warm-ups, median of {RUNS}, arms interleaved; the "
                  "kernel is the only entry of a plan and is timed by the plan's own events",
        "device": torch.cuda.get_device_name(0),
        "cases": [run_case(hip, dev, stream, kind, shape) for shape in SHAPES for kind in sorted(dnn_hip.ACTIVATIONS)],
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
