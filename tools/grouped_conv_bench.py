#!/usr/bin/env python3
"""The grouped-conv entry (dnn_plan_add_conv_grouped, csrc/conv_grouped.hip) against the two things
it can be compared with (needs an MI355X):

  grouped  the gconv step of a one-entry plan
  dense    the same layer as it had to run before the entry existed: dnn_plan_add_conv_padded with the
           weights expanded to a block-diagonal dense kernel (groups x the arithmetic and weights)
  copy     a dnn_plan_add_slice copy of a tensor of (input + output) / 2 bytes: the slice reads and
           writes that many, so it moves what the layer moves, its input once in and its output once
           out: a measured floor for the layer's activation traffic (at stride 2 a smaller tensor
           than the input)

Shapes at batch 8: 3x3 with 32 groups of cg = og in 4, 8, 16, 32 on 104, 52, 26 and 13 maps, and the
depthwise 3x3 at 256 channels on a 52 map at stride 1 and 2.

Each figure is the median over `rounds` of a step's device time: HIP events around that step alone
(dnn_plan_timing_begin_only) in `reps` runs of its plan on one stream, after a warm-up round, the
arms interleaved per round; the spread is the min and max over the rounds.  Two clock-stamp launches
bracket the timed rounds of a shape (the shader clock over them).  The grouped and the dense outputs
are compared once per shape (normwise, against each other).

    python tools/grouped_conv_bench.py [--reps 20] [--rounds 5] [--out profiles/grouped_conv_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "dnn-inference-engine_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import dnn_hip  # noqa: E402

B = 8
# (name, map, channels, groups, stride)
SHAPES = [(f"3x3 g32 cg{cg} {hw}x{hw}", hw, 32 * cg, 32, 1) for cg, hw in ((4, 104), (8, 52), (16, 26), (32, 13))]
SHAPES += [("depthwise 3x3 c256 52x52 s1", 52, 256, 256, 1), ("depthwise 3x3 c256 52x52 s2", 52, 256, 256, 2)]


def conv_entry(x_shape, kern, stride, groups):
    g = dnn_hip.DnnGraphBuilder()
    t = g.create_conv2d_padded(g.create_input(list(x_shape)), kern, [1, stride, stride, 1], (1, 1), groups=groups)
    od = kern.shape[3]
    e = (dnn_hip.GroupedConvEntry if groups > 1 else dnn_hip.PaddedConvEntry)(t, (1, 1))
    e.affine = g.create_scale_shift(t, np.linspace(0.5, 1.5, od, dtype=np.float32), np.linspace(-1, 1, od, dtype=np.float32))
    e.leaky = 2
    return e


def block_diagonal(kern, groups):
    kh, kw, cg, od = kern.shape
    og = od // groups
    dense = np.zeros((kh, kw, cg * groups, od), np.float32)
    for g in range(groups):
        dense[:, :, g * cg:(g + 1) * cg, g * og:(g + 1) * og] = kern[:, :, :, g * og:(g + 1) * og]
    return dense


def bench(name, hw, c, groups, stride, reps, rounds, dev, stream):
    rng = np.random.default_rng(1)
    cg = c // groups
    kern = (rng.standard_normal((3, 3, cg, c)) / np.sqrt(9 * cg)).astype(np.float32)
    shape = (B, hw, hw, c)
    ohw = (hw + 2 - 3) // stride + 1
    copy_shape = (1, (hw * hw + ohw * ohw) // 2, c)  # (input + output) / 2 pixels of c channels
    plans = {
        "grouped": (dnn_hip.Plan(B, shape[1:], [conv_entry(shape, kern, stride, groups)], device=0), "gconv0", shape),
        "dense": (dnn_hip.Plan(B, shape[1:], [conv_entry(shape, block_diagonal(kern, groups), stride, 1)], device=0),
                  None, shape),
        "copy": (dnn_hip.Plan(B, copy_shape, [dnn_hip.SliceEntry(0, c)], device=0), "slice0", (B,) + copy_shape),
    }
    x = torch.from_numpy(rng.standard_normal(shape).astype(np.float32)).to(dev)
    outs = {k: torch.empty((B,) + p.out_shape, device=dev) for k, (p, _, _) in plans.items()}
    clk = torch.zeros((2, 256, 4), dtype=torch.int64, device=dev)
    ms = {k: [] for k in plans}
    steps = {}
    with torch.cuda.stream(stream):
        for r in range(rounds + 1):
            if r == 1:
                dnn_hip.clock_stamp(clk[0].data_ptr(), 256, stream.cuda_stream)
            for k, (p, only, _) in plans.items():
                names = [q["name"] for q in p.kernels()]
                steps[k] = names
                p.timing_begin(reps, only=only if only else None)
                for _ in range(reps):
                    p.run_device(B, x.data_ptr(), outs[k].data_ptr(), stream.cuda_stream)
                t, cnt = p.timing_end()
                if r:
                    ms[k].append(sum(t) / reps)  # (the dense arm: every step of its plan, im2col included if it has one)
        dnn_hip.clock_stamp(clk[1].data_ptr(), 256, stream.cuda_stream)
    stream.synchronize()
    sclk = dnn_hip.sclk_from_stamps(clk[0].cpu().numpy(), clk[1].cpu().numpy())
    a, d = outs["grouped"].cpu().numpy().astype(np.float64), outs["dense"].cpu().numpy().astype(np.float64)
    med = {k: statistics.median(v) for k, v in ms.items()}
    info = plans["grouped"][0].kernels()[0]
    row = {"shape": name, "in": list(shape), "out": [B, ohw, ohw, c], "groups": groups, "stride": stride,
           "grouped_mode": plans["grouped"][0].describe().split("mode=")[1].split()[0],
           "dense_steps": steps["dense"], "flops": info["flops"], "bytes": info["bytes"],
           "copy_bytes_moved": 2 * 4 * B * int(np.prod(copy_shape))}
    for k in plans:
        row[f"{k}_us"] = round(med[k] * 1e3, 2)
        row[f"{k}_us_min_max"] = [round(min(ms[k]) * 1e3, 2), round(max(ms[k]) * 1e3, 2)]
    row["dense_over_grouped"] = round(med["dense"] / med["grouped"], 3)
    row["grouped_over_copy"] = round(med["grouped"] / med["copy"], 3)
    row["grouped_faster_than_dense"] = med["grouped"] < med["dense"]
    row["grouped_tflops"] = round(info["flops"] / med["grouped"] / 1e9, 2)
    row["grouped_GBps"] = round(info["bytes"] / med["grouped"] / 1e6, 1)
    row["grouped_vs_dense_normwise"] = float(np.abs(a - d).max() / np.abs(d).max())
    row["sclk_ghz"] = round(sclk["mean"], 3) if sclk else None
    for p, _, _ in plans.values():
        p.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "grouped_conv_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "grouped_conv_bench needs a GPU"
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    rows = []
    for shape in SHAPES:
        rows.append(bench(*shape, a.reps, a.rounds, dev, stream))
        print(json.dumps(rows[-1]), flush=True)
    res = {
        "what": "grouped / depthwise 3x3 convs at batch 8: the gconv step vs the same layer as a dense "
                "dnn_plan_add_conv_padded on block-diagonal zero-expanded weights vs a dnn_plan_add_slice copy that moves "
                "the layer's input + output bytes; the convs with the affine + leaky epilogue",
        "library": dnn_hip.LIB_NAME,
        "method": f"HIP events around the step in {a.reps} runs per round, one warm-up round, median of {a.rounds} rounds, "
                  "arms interleaved per round, same process, stream and input; one machine, one run",
        "condition": "grouped_us < dense_us at every shape",
        "condition_met": all(r["grouped_faster_than_dense"] for r in rows),
        "rows": rows,
        "device": torch.cuda.get_device_name(0),
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
