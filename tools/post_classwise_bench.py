#!/usr/bin/env python3
"""The multi-scale decode with per-class NMS against the class-agnostic one (needs an MI355X).

Two arms on the same device buffers, in the same process and on the same stream:

  any        dnn_yolo_postprocess_multi_nms, nms_mode 0: the class-agnostic kernel, one serial chain
             of 64-candidate blocks
  per_class  nms_mode 1: class-major sort, one wave per class segment, merge

Inputs, all at grids 13, 26, 52 x 3 anchors (the 416 x 416 model, 10,647 boxes):

  typical    80 classes, tests/post_head_oracle.synthetic_predictions, score > 0.3, batch 1 and 8
  saturated  80 classes, every box a candidate, the hot class uniform over the classes; and the
             same with 3 classes: three segments of about 3500 candidates, each above the length
             at which the whole workgroup takes a segment
  skew       5 classes, every box a candidate, tests/post_classwise_cases' skew case at these grids:
             class 0 owns about three quarters of the stride-8 boxes

Each figure is the median over `rounds` of the device time of one launch: HIP events around `reps`
back-to-back launches on one stream, after a warm-up round, the arms interleaved per round (as
tools/spp_bench.py measures).  The spread of an arm is its min and max over the rounds.  counts are
what each arm left in `counts` (detections per image, or the error code).

    python tools/post_classwise_bench.py [--reps 20] [--rounds 5] [--out profiles/post_classwise_bench.json]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("dnn-inference-engine_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(REPO, p))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import dnn_hip  # noqa: E402
import post_classwise_cases as CK  # noqa: E402
import post_head_oracle as O  # noqa: E402
import post_multi_cases as K  # noqa: E402
import yolo_post  # noqa: E402

GRIDS = (13, 26, 52)


def inputs():
    """name -> (oracle description, per scale [B, g, g, n_out])."""
    m80 = K.yolov3_multi(GRIDS, 80, score_thr=0.3)
    rng = np.random.default_rng(0)
    typical = [np.stack([O.synthetic_predictions(rng, h) for _ in range(8)]) for h in m80.scales]
    rng = np.random.default_rng(1)
    saturated = [O.synthetic_predictions(rng, h, saturate=True)[None] for h in m80.scales]
    m3 = K.yolov3_multi(GRIDS, 3, score_thr=0.3)
    rng = np.random.default_rng(2)
    few = [O.synthetic_predictions(rng, h, saturate=True)[None] for h in m3.scales]
    return [("typical B=1", m80, [p[:1] for p in typical]), ("typical B=8", m80, typical),
            ("saturated B=1", m80, saturated), ("saturated, 3 classes B=1", m3, few),
            ("skew B=1", CK.skew_multi(GRIDS, 5), CK.skew_preds(GRIDS, 5))]


def timed(fn, reps, stream):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    for _ in range(reps):
        fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b) / reps


def bench(name, multi, preds, reps, rounds):
    dev = torch.device("cuda", 0)
    head = yolo_post.MultiHead(multi.scales, multi.class_mode)
    n = preds[0].shape[0]
    xs = [torch.from_numpy(np.ascontiguousarray(p)).to(dev) for p in preds]
    ptrs = (ctypes.c_void_p * len(xs))(*[x.data_ptr() for x in xs])
    ws = torch.zeros(head.workspace_bytes(n), dtype=torch.uint8, device=dev)
    dets = torch.zeros((n, head.boxes, 40), dtype=torch.uint8, device=dev)
    counts = torch.zeros(n, dtype=torch.int32, device=dev)
    stream = torch.cuda.Stream(dev)
    s = stream.cuda_stream

    def arm(mode):
        def run():
            dnn_hip._check(yolo_post._lib.dnn_yolo_postprocess_multi_nms(
                ctypes.byref(head.c), ptrs, n, dets.data_ptr(), head.boxes, counts.data_ptr(), ws.data_ptr(),
                ws.numel(), mode, s), "dnn_yolo_postprocess_multi_nms")
        return run

    arms = {"any": arm(0), "per_class": arm(1)}
    ms = {k: [] for k in arms}
    got = {}
    with torch.cuda.stream(stream):
        for r in range(rounds + 1):
            for k, fn in arms.items():
                t = timed(fn, reps, stream)
                if r:
                    ms[k].append(t)
                else:
                    got[k] = [int(c) for c in counts.cpu()]
    stream.synchronize()
    a, b = statistics.median(ms["any"]), statistics.median(ms["per_class"])
    us = lambda v: round(v * 1e3, 2)  # noqa: E731
    return {"input": name, "images": n, "boxes": head.boxes, "classes": head.n_classes,
            "any_us": us(a), "per_class_us": us(b), "per_class_over_any": round(b / a, 3),
            "any_us_min_max": [us(min(ms["any"])), us(max(ms["any"]))],
            "per_class_us_min_max": [us(min(ms["per_class"])), us(max(ms["per_class"]))],
            "per_class_within_any_spread": min(ms["any"]) <= b <= max(ms["any"]),
            "any_counts": got["any"], "per_class_counts": got["per_class"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "post_classwise_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "post_classwise_bench needs a GPU"
    rows = [bench(name, multi, preds, a.reps, a.rounds) for name, multi, preds in inputs()]
    res = {
        "what": "multi-scale YOLO decode at 13/26/52 x 3 anchors: per-class NMS (nms_mode 1) vs the class-agnostic "
                "kernel (nms_mode 0), device time of one launch",
        "method": f"HIP events around {a.reps} back-to-back launches, one warm-up round, median of {a.rounds} rounds, "
                  "arms interleaved per round, same process, stream and device buffers; one machine, one run",
        "rows": rows,
        "device": torch.cuda.get_device_name(0),
        "hardware": f"one GPU, {torch.cuda.get_device_properties(0).gcnArchName}; 'device' is the name the runtime "
                    "reports",
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
