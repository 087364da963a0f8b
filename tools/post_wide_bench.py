#!/usr/bin/env python3
"""The grid-wide multi-scale decode (dnn_yolo_postprocess_wide: a memset, a decode kernel over the
whole grid, one NMS workgroup per image) against the existing one-workgroup-per-image entries
(needs an MI355X).

Two arms on the same input arrays, in the same process and on the same stream, in the three modes
(class-agnostic, per-class, multi-label on per-class):

  existing  dnn_yolo_postprocess_multi_nms (nms_mode 0 / 1) or dnn_yolo_postprocess_multi_labels
  wide      dnn_yolo_postprocess_wide with the same modes

Inputs, batch 1 and batch 8:

  416, score > 0.99  grids 13, 26, 52 x 3 anchors x 80 classes (10,647 boxes),
                     tests/post_multi_oracle.batch(seed 0): a few hundred candidates an image
  416, saturated     the same head at score > 0.3, post_multi_oracle.batch(seed 0, saturate=True):
                     every box is a candidate (in multi-label mode more than 16,384: both arms end
                     with -3 after the decode)
  608, ...           the same two inputs at grids 19, 38, 76 (22,743 boxes): the wide arm alone,
                     the existing entries refuse the head

With --alt-lib PATH a third arm `wide_alt` runs the wide entry of a second build of the library
(built with -DPW_SHARE_LOGITS=0: a box's thread loops over its classes itself instead of the wave
sharing them across its lanes), which is how that switch was decided.

Each figure is the median over `rounds` of the device time of one call: HIP events around `reps`
back-to-back calls on one stream, after a warm-up round, the arms interleaved per round (as
tools/post_multilabel_bench.py measures).  The spread of an arm is its min and max over the rounds.
counts are what each arm left in `counts` (rows per image, or the code).

    python tools/post_wide_bench.py [--reps 20] [--rounds 5] [--alt-lib PATH] [--out profiles/post_wide_bench.json]
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
import post_multi_cases as K  # noqa: E402
import post_multi_oracle as MO  # noqa: E402
import yolo_post  # noqa: E402

CLASSES = 80
MODES = {"any": ("any", "argmax"), "per_class": ("per_class", "argmax"), "multi": ("per_class", "multi")}


def inputs():
    """(name, oracle description, per scale [8, g, g, n_out], whether the existing entries take it)."""
    out = []
    for size, grids in ((416, (13, 26, 52)), (608, (19, 38, 76))):
        m99 = K.yolov3_multi(grids, CLASSES, score_thr=0.99)
        m30 = K.yolov3_multi(grids, CLASSES, score_thr=0.3)
        out.append((f"{size}, score > 0.99", m99, MO.batch(0, m99, 8), size == 416))
        out.append((f"{size}, saturated", m30, MO.batch(0, m30, 8, saturate=True), size == 416))
    return out


def timed(fn, reps, stream):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    for _ in range(reps):
        fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b) / reps


def bench(name, multi, preds, mode, with_existing, alt, reps, rounds):
    dev = torch.device("cuda", 0)
    nms, labels = MODES[mode]
    wide = yolo_post.WideHead(multi.scales, multi.class_mode, nms, labels)
    n, max_det = preds[0].shape[0], wide.max_det
    xs = [torch.from_numpy(np.ascontiguousarray(p)).to(dev) for p in preds]
    ptrs = (ctypes.c_void_p * len(xs))(*[x.data_ptr() for x in xs])
    ws = torch.zeros(wide.workspace_bytes(n), dtype=torch.uint8, device=dev)  # (covers the existing 40 B per box)
    dets = torch.zeros((n, max_det, 40), dtype=torch.uint8, device=dev)
    counts = torch.zeros(n, dtype=torch.int32, device=dev)
    stream = torch.cuda.Stream(dev)
    s = stream.cuda_stream
    modes = (yolo_post.NMS_MODES[nms], yolo_post.LABEL_MODES[labels])

    def wide_arm(lib):
        def run():
            dnn_hip._check(lib.dnn_yolo_postprocess_wide(
                ctypes.byref(wide.c), ptrs, n, dets.data_ptr(), max_det, counts.data_ptr(), ws.data_ptr(), ws.numel(),
                modes[0], modes[1], s), "dnn_yolo_postprocess_wide")
        return run

    arms = {}
    if with_existing:
        old = yolo_post.MultiHead(multi.scales, multi.class_mode, nms, labels)
        assert old.max_det == max_det
        entry = (yolo_post._lib.dnn_yolo_postprocess_multi_labels if labels == "multi"
                 else yolo_post._lib.dnn_yolo_postprocess_multi_nms)

        def existing():
            dnn_hip._check(entry(ctypes.byref(old.c), ptrs, n, dets.data_ptr(), max_det, counts.data_ptr(), ws.data_ptr(),
                                 ws.numel(), modes[1] if labels == "multi" else modes[0], s), "the existing entry")
        arms["existing"] = existing
    arms["wide"] = wide_arm(yolo_post._lib)
    if alt is not None:
        arms["wide_alt"] = wide_arm(alt)

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
    us = lambda v: round(v * 1e3, 2)  # noqa: E731
    row = {"input": name, "mode": mode, "images": n, "boxes": wide.boxes, "classes": wide.n_classes}
    for k in arms:
        row[f"{k}_us"] = us(statistics.median(ms[k]))
        row[f"{k}_us_min_max"] = [us(min(ms[k])), us(max(ms[k]))]
        row[f"{k}_counts"] = got[k]
    if with_existing:
        row["wide_over_existing"] = round(statistics.median(ms["wide"]) / statistics.median(ms["existing"]), 3)
        row["same_counts"] = got["wide"] == got["existing"]
    if alt is not None:
        row["wide_over_wide_alt"] = round(statistics.median(ms["wide"]) / statistics.median(ms["wide_alt"]), 3)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--alt-lib", default=None, help="a second build of libdnn_hip.so to time as `wide_alt`")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "post_wide_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "post_wide_bench needs a GPU"
    alt = yolo_post._bind(ctypes.CDLL(os.path.abspath(a.alt_lib))) if a.alt_lib else None
    rows = []
    for name, multi, preds, with_existing in inputs():
        for mode in MODES:
            for n in (1, 8):
                rows.append(bench(f"{name} B={n}", multi, [p[:n] for p in preds], mode, with_existing, alt, a.reps,
                                  a.rounds))
                print(json.dumps(rows[-1]), flush=True)
    res = {
        "what": "multi-scale YOLO decode x 3 anchors x 80 classes: the grid-wide entry (dnn_yolo_postprocess_wide: "
                "memset + decode kernel + NMS kernel) vs the existing one-workgroup-per-image entries, device time of "
                "one call",
        "method": f"HIP events around {a.reps} back-to-back calls, one warm-up round, median of {a.rounds} rounds, "
                  "arms interleaved per round, same process, stream and input arrays; one machine, one run",
        "wide_alt": "the wide entry built with -DPW_SHARE_LOGITS=0 (per-thread class loops)" if alt is not None else None,
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
