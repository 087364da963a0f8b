#!/usr/bin/env python3
"""The multi-scale decode with multi-label detections against the single-label per-class decode
(needs an MI355X).

Two arms on the same device buffers, in the same process and on the same stream:

  per_class  dnn_yolo_postprocess_multi_nms, nms_mode 1: one class per box, the arg-max (the baseline)
  multi      dnn_yolo_postprocess_multi_labels, labels_mode 1: one candidate per (box, class) above
             the threshold, the same per-class NMS, the merge with the class in the key

Inputs, all at grids 13, 26, 52 x 3 anchors x 80 classes (the 416 x 416 model, 10,647 boxes), batch 1
and batch 8:

  score > 0.99  tests/post_multi_oracle.batch(seed 0), the batch of tests/post_classwise_cases'
                `yolov3` case: no box has a second label, so both arms sort and suppress the same
                candidates and the ratio is the price of the multi-label decode and merge
  tall          tests/post_classwise_cases.skew_multi's tall anchors, saturated predictions, score >
                0.95: every box is a candidate through its hot class and about one in eight carries a
                second label; the candidates per image are counted by the oracle and recorded

Each figure is the median over `rounds` of the device time of one launch: HIP events around `reps`
back-to-back launches on one stream, after a warm-up round, the arms interleaved per round (as
tools/post_classwise_bench.py measures).  The spread of an arm is its min and max over the rounds.
counts are what each arm left in `counts` (rows per image, or the code).

    python tools/post_multilabel_bench.py [--reps 20] [--rounds 5] [--out profiles/post_multilabel_bench.json]
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
import post_multi_oracle as MO  # noqa: E402
import post_multilabel_oracle as LO  # noqa: E402
import yolo_post  # noqa: E402

GRIDS, CLASSES = (13, 26, 52), 80


def inputs():
    """(name, oracle description, per scale [8, g, g, n_out])."""
    m99 = K.yolov3_multi(GRIDS, CLASSES, score_thr=0.99)
    sparse = MO.batch(0, m99, 8)
    skew = CK.skew_multi(GRIDS, CLASSES)
    tall = MO.Multi(tuple(h._replace(score_thr=0.95) for h in skew.scales), skew.class_mode)
    rng = np.random.default_rng(11)
    images = [[O.synthetic_predictions(rng, h, tw_scale=0.5, saturate=True) for h in tall.scales] for _ in range(8)]
    dense = [np.stack([img[s] for img in images]) for s in range(3)]
    return [("score > 0.99", m99, sparse), ("tall, score > 0.95", tall, dense)]


def timed(fn, reps, stream):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    for _ in range(reps):
        fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b) / reps


def bench(name, multi, preds, candidates, reps, rounds):
    dev = torch.device("cuda", 0)
    head = yolo_post.MultiHead(multi.scales, multi.class_mode, "per_class", "multi")
    n, max_det = preds[0].shape[0], head.max_det
    xs = [torch.from_numpy(np.ascontiguousarray(p)).to(dev) for p in preds]
    ptrs = (ctypes.c_void_p * len(xs))(*[x.data_ptr() for x in xs])
    ws = torch.zeros(head.workspace_bytes(n), dtype=torch.uint8, device=dev)
    dets = torch.zeros((n, max_det, 40), dtype=torch.uint8, device=dev)
    counts = torch.zeros(n, dtype=torch.int32, device=dev)
    stream = torch.cuda.Stream(dev)
    s = stream.cuda_stream

    def per_class():
        dnn_hip._check(yolo_post._lib.dnn_yolo_postprocess_multi_nms(
            ctypes.byref(head.c), ptrs, n, dets.data_ptr(), max_det, counts.data_ptr(), ws.data_ptr(), ws.numel(), 1, s),
            "dnn_yolo_postprocess_multi_nms")

    def multi_label():
        dnn_hip._check(yolo_post._lib.dnn_yolo_postprocess_multi_labels(
            ctypes.byref(head.c), ptrs, n, dets.data_ptr(), max_det, counts.data_ptr(), ws.data_ptr(), ws.numel(), 1, s),
            "dnn_yolo_postprocess_multi_labels")

    arms = {"per_class": per_class, "multi": multi_label}
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
    a, b = statistics.median(ms["per_class"]), statistics.median(ms["multi"])
    us = lambda v: round(v * 1e3, 2)  # noqa: E731
    return {"input": name, "images": n, "boxes": head.boxes, "classes": head.n_classes,
            "multi_label_candidates": candidates,
            "per_class_us": us(a), "multi_us": us(b), "multi_over_per_class": round(b / a, 3),
            "per_class_us_min_max": [us(min(ms["per_class"])), us(max(ms["per_class"]))],
            "multi_us_min_max": [us(min(ms["multi"])), us(max(ms["multi"]))],
            "multi_within_per_class_spread": min(ms["per_class"]) <= b <= max(ms["per_class"]),
            "per_class_counts": got["per_class"], "multi_counts": got["multi"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "post_multilabel_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "post_multilabel_bench needs a GPU"
    rows = []
    for name, multi, preds in inputs():
        cand = [len(LO.candidates([p[i] for p in preds], multi)) for i in range(8)]
        assert max(cand) <= LO.MAX_CANDIDATES, cand
        for n in (1, 8):
            rows.append(bench(f"{name} B={n}", multi, [p[:n] for p in preds], cand[:n], a.reps, a.rounds))
    res = {
        "what": "multi-scale YOLO decode at 13/26/52 x 3 anchors x 80 classes: multi-label (labels_mode 1) vs the "
                "single-label per-class kernel (nms_mode 1), device time of one launch",
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
