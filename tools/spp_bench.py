#!/usr/bin/env python3
"""The fused SPP kernel against the three max pools it replaces (needs an MI355X).

Shapes: the maps where SPP occurs, [B, 13, 13, 512] (416 x 416 input) and [B, 19, 19, 512]
(608 x 608), at B = 1, 8 and 64, sizes 13, 9, 5 with x last.  Two arms on the same input, in the
same process and on the same stream:

  fused   one plan whose only entry is the spp entry: one kernel writes all four channel blocks
  pools   three plans of one MaxPool2D each (5, 9, 13; stride 1, SAME), run back to back: the
          engine's existing pool kernel, three launches, and no concat (so the arm is cheaper than
          what a graph built from pools and routes would run)

Each figure is the median over `rounds` of the device time of one run: HIP events around `reps`
back-to-back runs on one stream, after a warm-up round, the arms interleaved per round (as
tools/yolov3_time.py measures).  The fused kernel's bytes are counted as n_sizes + 2 tensors of the
input's size (the input read once, the output written once).  Condition: fused <= pools in every
row.  The fused output is checked once per shape against the pools' outputs, bit for bit.

    python tools/spp_bench.py [--reps 20] [--rounds 5] [--out profiles/spp_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "dnn-inference-engine_amd"))

import torch  # noqa: E402

import dnn_hip  # noqa: E402

SIZES = (13, 9, 5)
MAPS = ((13, 13, 512), (19, 19, 512))
BATCHES = (1, 8, 64)


def pool_plan(B, shape, k):
    g = dnn_hip.DnnGraphBuilder()
    x = g.create_input([B] + list(shape))
    g.set_out_node(g.create_max_pool2d(x, [1, k, k, 1], [1, 1, 1, 1], "SAME"))
    return dnn_hip.Plan(B, shape, dnn_hip.lower_graph(g), device=0)


def timed(fn, reps, stream):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    for _ in range(reps):
        fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b) / reps


def bench(B, shape, reps, rounds):
    h, w, c = shape
    dev = torch.device("cuda", 0)
    fused = dnn_hip.Plan(B, shape, [dnn_hip.SppEntry(SIZES)], device=0)
    pools = [pool_plan(B, shape, k) for k in SIZES]
    assert [k["name"] for k in fused.kernels()] == ["spp0"]
    assert all([k["name"] for k in p.kernels()] == ["pool0"] for p in pools)
    x = torch.randn((B, h, w, c), device=dev)
    y = torch.empty((B, h, w, (len(SIZES) + 1) * c), device=dev)
    ys = [torch.empty((B, h, w, c), device=dev) for _ in SIZES]
    stream = torch.cuda.Stream(dev)
    s = stream.cuda_stream

    def run_fused():
        fused.run_device(B, x.data_ptr(), y.data_ptr(), s)

    def run_pools():
        for p, o in zip(pools, ys):
            p.run_device(B, x.data_ptr(), o.data_ptr(), s)

    f_ms, p_ms = [], []
    with torch.cuda.stream(stream):
        for r in range(rounds + 1):
            f, p = timed(run_fused, reps, stream), timed(run_pools, reps, stream)
            if r:
                f_ms.append(f)
                p_ms.append(p)
    stream.synchronize()
    want = torch.cat(ys + [x], dim=3)
    assert torch.equal(y.view(torch.int32), want.view(torch.int32)), "the fused output differs from the pools'"
    for p in pools + [fused]:
        p.close()
    f, p = statistics.median(f_ms), statistics.median(p_ms)
    nbytes = (len(SIZES) + 2) * B * h * w * c * 4
    return {"shape": [B, h, w, c], "fused_us": round(f * 1e3, 2), "pools_us": round(p * 1e3, 2),
            "ratio": round(f / p, 3), "not_slower": f <= p, "fused_bytes": nbytes,
            "fused_GBps": round(nbytes / f / 1e6, 1),
            "fused_us_min_max": [round(min(f_ms) * 1e3, 2), round(max(f_ms) * 1e3, 2)],
            "pools_us_min_max": [round(min(p_ms) * 1e3, 2), round(max(p_ms) * 1e3, 2)]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "spp_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "spp_bench needs a GPU"
    rows = [bench(B, shape, a.reps, a.rounds) for shape in MAPS for B in BATCHES]
    res = {
        "what": "fused SPP kernel (sizes 13, 9, 5, x last) vs three MaxPool2D launches (5, 9, 13) on the same input",
        "method": f"HIP events around {a.reps} back-to-back runs, one warm-up round, median of {a.rounds} rounds, "
                  "arms interleaved per round, same process and stream",
        "rows": rows, "all_not_slower": all(r["not_slower"] for r in rows),
        "device": torch.cuda.get_device_name(0),
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
