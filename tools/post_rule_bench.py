#!/usr/bin/env python3
"""The scaled-YOLOv4 head rule (new_coords decode, DIoU NMS with beta 0.6: the dnn_yolo_postprocess_*_rule
entries) against the logistic / IoU rule of the existing entries, per-class NMS with multi-label output, on
the same box (needs an MI355X).

Input: tools/post_wide_bench.py's 416 x 416 head (grids 13, 26, 52 x 3 anchors x 80 classes: 10,647 boxes),
batch 1 and 8, sparse (score > 0.99) and saturated (score > 0.3).  The existing arm reads the logits; the
rule arm reads their logistic, computed in float64 and rounded to fp32: the values in [0, 1] that a
logistic head conv would have produced, so both arms see the same boxes up to that rounding.  Both kernel
families are timed: the one-workgroup entries (`multi`) and the grid-wide ones (`wide`).

The method is tools/post_wide_bench.py's: the median over `rounds` of the device time of one call, HIP
events around `reps` back-to-back calls on one stream after a warm-up round, the arms interleaved per round;
an arm's spread is its min and max over the rounds.

    python tools/post_rule_bench.py [--reps 20] [--rounds 5] [--out profiles/post_rule_bench.json]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))

import post_wide_bench as WB  # noqa: E402  (puts the package, the oracle and the tests on sys.path)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import dnn_hip  # noqa: E402
import yolo_post  # noqa: E402


def squashed(preds):
    with np.errstate(over="ignore"):
        return [(1.0 / (1.0 + np.exp(-p.astype(np.float64)))).astype(np.float32) for p in preds]


def bench(name, multi, preds, kind, reps, rounds):
    dev = torch.device("cuda", 0)
    cls = yolo_post.WideHead if kind == "wide" else yolo_post.MultiHead
    heads = {"logistic_iou": cls(multi.scales, "logistic", "per_class", "multi"),
             "new_coords_diou": cls(multi.scales, "logistic", "per_class", "multi", new_coords=True, nms_kind="diou",
                                    beta_nms=0.6)}
    data = {"logistic_iou": preds, "new_coords_diou": squashed(preds)}
    n, max_det = preds[0].shape[0], heads["logistic_iou"].max_det
    ws = torch.zeros(heads["logistic_iou"].workspace_bytes(n), dtype=torch.uint8, device=dev)
    dets = torch.zeros((n, max_det, 40), dtype=torch.uint8, device=dev)
    counts = torch.zeros(n, dtype=torch.int32, device=dev)
    stream = torch.cuda.Stream(dev)
    arms, keep = {}, []
    for k, head in heads.items():
        xs = [torch.from_numpy(np.ascontiguousarray(p)).to(dev) for p in data[k]]
        ptrs = (ctypes.c_void_p * len(xs))(*[x.data_ptr() for x in xs])
        keep.append(xs)
        arms[k] = (lambda head=head, ptrs=ptrs: head._call(
            "device", (ptrs, n, dets.data_ptr(), max_det, counts.data_ptr(), ws.data_ptr(), ws.numel()),
            (stream.cuda_stream,)))
    ms, got = {k: [] for k in arms}, {}
    with torch.cuda.stream(stream):
        for r in range(rounds + 1):
            for k, fn in arms.items():
                t = WB.timed(fn, reps, stream)
                if r:
                    ms[k].append(t)
                else:
                    got[k] = [int(c) for c in counts.cpu()]
    stream.synchronize()
    us = lambda v: round(v * 1e3, 2)  # noqa: E731
    row = {"input": name, "kernels": kind, "images": n, "boxes": heads["logistic_iou"].boxes, "classes": WB.CLASSES}
    for k in arms:
        row[f"{k}_us"] = us(statistics.median(ms[k]))
        row[f"{k}_us_min_max"] = [us(min(ms[k])), us(max(ms[k]))]
        row[f"{k}_counts"] = got[k]
    row["rule_over_existing"] = round(statistics.median(ms["new_coords_diou"]) / statistics.median(ms["logistic_iou"]), 3)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "post_rule_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "post_rule_bench needs a GPU"
    rows = []
    for name, multi, preds, with_existing in WB.inputs():
        if not with_existing:  # the 608 head: the one-workgroup entries refuse it
            continue
        for kind in ("multi", "wide"):
            for n in (1, 8):
                rows.append(bench(f"{name} B={n}", multi, [p[:n] for p in preds], kind, a.reps, a.rounds))
                print(json.dumps(rows[-1]), flush=True)
    res = {
        "what": "multi-scale YOLO decode, 10,647 boxes x 80 classes, per-class NMS, multi-label: new_coords + DIoU "
                "(beta 0.6) through the _rule entries vs the logistic decode + IoU NMS of the existing entries, device "
                "time of one call",
        "method": f"HIP events around {a.reps} back-to-back calls, one warm-up round, median of {a.rounds} rounds, "
                  "arms interleaved per round, same process and stream; the rule arm reads the logistic of the other "
                  "arm's logits; one machine, one run",
        "rows": rows,
        "device": torch.cuda.get_device_name(0),
        "hardware": f"one GPU, {torch.cuda.get_device_properties(0).gcnArchName}; 'device' is the name the runtime "
                    "reports",
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
