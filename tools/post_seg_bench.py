#!/usr/bin/env python3
"""The DFL decode with instance masks (dnn_yolo_postprocess_dfl_seg) beside the DFL decode alone
(dnn_yolo_postprocess_dfl) on the same inputs in one process: 640 x 640, 8,400 points x 80 classes at strides 8,
16, 32, 160 x 160 x 32 prototypes, per-class NMS with one label a box, a seeded share of points with a class above
the threshold (about 50 rows an image).  Device pointers, one stream; a call is timed by device events around
CALLS back-to-back calls after WARMUP, the two arms alternate for ROUNDS rounds and the median is reported.
Prints one JSON line; --out also writes it to a file."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "dnn-inference-engine_amd"))

GRIDS, CLASSES, REG, NM, MASK, NET, SHARE, SEED = ((80, 8.0), (40, 16.0), (20, 32.0)), 80, 16, 32, 160, 640, 0.007, 1
WARMUP, CALLS, ROUNDS, MAX_DET = 20, 200, 5, 300


def inputs(batch):
    """(preds, coefs, proto): a SHARE of the points has one class logit at +2, the others are at -6; box logits
    put the weight on bins 0..3 (boxes up to 6 cells wide); coefficients and prototypes are standard normal."""
    rng = np.random.default_rng(SEED)
    preds, coefs = [], []
    for g, _ in GRIDS:
        p = rng.standard_normal((batch, g, g, 4 * REG + CLASSES)).astype(np.float32)
        p[..., :4 * REG] -= np.where(np.arange(4 * REG) % REG >= 4, 8.0, 0.0).astype(np.float32)
        p[..., 4 * REG:] = -6.0
        b, r, c = np.nonzero(rng.random((batch, g, g)) < SHARE)
        p[b, r, c, 4 * REG + rng.integers(CLASSES, size=len(b))] = 2.0 + rng.random(len(b)).astype(np.float32)
        preds.append(p)
        coefs.append(rng.standard_normal((batch, g, g, NM)).astype(np.float32))
    return preds, coefs, rng.standard_normal((batch, MASK, MASK, NM)).astype(np.float32)


def main():
    import torch
    import yolo_post
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    result = {"what": "640 x 640: 8400 points x 80 classes, 160 x 160 x 32 prototypes, per-class NMS, score > 0.25: us "
                      f"per call, median of {ROUNDS} rounds of {CALLS} calls", "share_on": SHARE}
    for batch in (1, 8):
        head = yolo_post.DflHead([(g, g, st) for g, st in GRIDS], CLASSES, REG, 0.25, 0.45, mask_dim=NM)
        spec = head.seg((MASK, MASK), (NET, NET), MAX_DET)
        host = inputs(batch)
        preds, coefs = ([torch.from_numpy(a).to(dev) for a in group] for group in host[:2])
        proto = torch.from_numpy(host[2]).to(dev)
        pp, cp = [x.data_ptr() for x in preds], [x.data_ptr() for x in coefs]
        plain = yolo_post.MultiDetectionBuffers(batch, dev, head, max_det=MAX_DET)
        seg = yolo_post.MaskDetectionBuffers(batch, dev, head, spec, max_det=MAX_DET)
        arms = {"dfl": lambda: plain.run(pp, batch, stream),
                "dfl_seg": lambda: seg.run(pp, cp, proto.data_ptr(), batch, stream)}
        times = {k: [] for k in arms}
        for rnd in range(ROUNDS + 1):  # round 0 warms both arms up
            for name, call in arms.items():
                n = WARMUP if rnd == 0 else CALLS
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(n):
                    call()
                t1.record()
                torch.cuda.synchronize()
                if rnd:
                    times[name].append(t0.elapsed_time(t1) * 1000.0 / n)
        rows = seg.counts.cpu().numpy().tolist()
        assert rows == plain.counts.cpu().numpy().tolist() and min(rows) > 0, rows
        assert torch.equal(seg.dets, plain.dets)
        set_bits = int(sum(m.sum() for m in seg.masks_to_host(batch)))
        result[f"batch{batch}"] = {k: {"us": round(statistics.median(v), 2), "min": round(min(v), 2),
                                       "max": round(max(v), 2)} for k, v in times.items()}
        result[f"batch{batch}"].update(rows=rows, mask_bits_set=set_bits)
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
