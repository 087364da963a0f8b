#!/usr/bin/env python3
"""The squeeze-and-excitation kernels (csrc/squeeze_excite.hip) against a device-to-device copy (needs an MI355X).

Cases, at batch 1 and batch 64, both with swish and logistic:
    112 x 112 x 96, cr 4     (an early MBConv block of EfficientNet-B0: a large map, a tiny gate)
    7 x 7 x 1152, cr 48      (its widest gate: a small map, 432 KB of gate weights)

The yardstick is hipMemcpyAsync(device to device) of the tensor's byte count, the project's yardstick for movement
kernels, whose 1.25 x bar is for one read and one write.  This operation reads x twice (the squeeze, then the
multiply) and writes it once, so the comparable figure is 1.5 copies: the ratio reported is (squeeze + excite) /
(1.5 x copy), and the bar 1.25 of that.

The two kernels run as the only entry of a plan and are timed by the plan's own HIP events (one event between them,
so their sum is what a forward pays); the copy is timed with HIP events on the same stream, in the same process.
5 warm-ups, then the median of 20, the two arms interleaved.  The result is checked once against torch's float64
evaluation of the definition on the same device.

    python tools/se_bench.py [--out profiles/se_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "dnn-inference-engine_amd"))
sys.path.insert(0, os.path.join(REPO, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import dnn_hip  # noqa: E402
from shortcut_bench import hip_runtime  # noqa: E402

WARMUP, RUNS = 5, 20
BAR, COPIES = 1.25, 1.5
CASES = ((112, 112, 96, 4), (7, 7, 1152, 48))
BATCHES = (1, 64)


def run_case(hip, dev, stream, batch, h, w, c, cr):
    rng = np.random.default_rng(c)
    w1 = (rng.standard_normal((c, cr)) * np.sqrt(h * w / c)).astype(np.float32)
    w2 = (rng.standard_normal((cr, c)) * 2 / np.sqrt(cr)).astype(np.float32)
    b1, b2 = rng.standard_normal(cr).astype(np.float32), rng.standard_normal(c).astype(np.float32)
    g = dnn_hip.DnnGraphBuilder()
    node = g.create_squeeze_excite(g.create_input([batch, h, w, c]), w1, b1, "swish", w2, b2, "logistic")
    plan = dnn_hip.Plan(batch, (h, w, c), [dnn_hip.SqueezeExciteEntry(node)], device=0)
    assert [k["name"] for k in plan.kernels()] == ["se0.squeeze", "se0.excite"]
    d_in = torch.randn((batch, h, w, c), device=dev)
    d_out, dst = torch.empty_like(d_in), torch.empty_like(d_in)
    nbytes = d_in.numel() * 4
    sq_ms, ex_ms, c_ms = [], [], []
    with torch.cuda.stream(stream):
        for i in range(WARMUP + RUNS):
            plan.timing_begin(1)
            plan.run_device(batch, d_in.data_ptr(), d_out.data_ptr(), stream.cuda_stream)
            ms, cnt = plan.timing_end()
            assert list(cnt) == [1, 1]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            rc = hip.hipMemcpyAsync(dst.data_ptr(), d_in.data_ptr(), nbytes, 3, stream.cuda_stream)  # 3: device to device
            assert rc == 0, rc
            e1.record(stream)
            e1.synchronize()
            if i >= WARMUP:
                sq_ms.append(ms[0])
                ex_ms.append(ms[1])
                c_ms.append(e0.elapsed_time(e1))
    x = d_in.double()
    t = lambda a: torch.from_numpy(a).to(dev).double()  # noqa: E731
    hid = x.mean((1, 2)) @ t(w1) + t(b1)
    gate = torch.sigmoid((hid * torch.sigmoid(hid)) @ t(w2) + t(b2))
    want = x * gate[:, None, None, :]
    err = ((d_out.double() - want).abs().max() / want.abs().max()).item()
    assert err < 2e-6, f"normwise error {err} against float64"
    plan.close()
    sq, ex, cp = statistics.median(sq_ms), statistics.median(ex_ms), statistics.median(c_ms)
    both = statistics.median(a + b for a, b in zip(sq_ms, ex_ms))
    return {"shape": [batch, h, w, c], "cr": cr, "tensor_bytes": nbytes, "squeeze_ms": sq, "excite_ms": ex,
            "both_ms": both, "memcpy_ms": cp, "copies": COPIES, "ratio_to_1.5_copies": both / (COPIES * cp), "bar": BAR,
            "within_bar": both <= BAR * COPIES * cp, "GBps_of_3_tensors": 3 * nbytes / both / 1e6,
            "memcpy_GBps": 2 * nbytes / cp / 1e6, "both_ms_min_max": [min(a + b for a, b in zip(sq_ms, ex_ms)),
                                                                      max(a + b for a, b in zip(sq_ms, ex_ms))],
            "memcpy_ms_min_max": [min(c_ms), max(c_ms)], "normwise_err": err}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "se_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "se_bench needs a GPU"
    dev = torch.device("cuda", 0)
    hip, stream = hip_runtime(), torch.cuda.Stream(dev)
    res = {
        "what": "the squeeze-and-excitation entry's two kernels vs 1.5 x hipMemcpyAsync device-to-device of the tensor",
        "method": f"HIP events, same process and stream, {WARMUP} warm-ups, median of {RUNS}, arms interleaved; the "
                  "kernels are the only entry of a plan and are timed by the plan's own events",
        "device": torch.cuda.get_device_name(0),
        "cases": [run_case(hip, dev, stream, b, *case) for case in CASES for b in BATCHES],
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
