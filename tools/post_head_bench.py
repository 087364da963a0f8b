"""Times of the two postprocessing kernels and of the batch-64 forward at three input sizes
(DESIGN.md §8 "Multi-scale postprocessing"), HIP events in one process:

    python tools/post_head_bench.py [--reps 200] [--rounds 5] [--no-forward]

post   64 images of tests/post_head_oracle.synthetic_predictions (ordinary density) through
       dnn_yolo_postprocess (13 x 13 only) and dnn_yolo_postprocess_head at 13 x 13 and
       19 x 19, and one saturated 40 x 40 image (8000 candidates) through the latter.
forward  the batch-64 x3 plan at 320, 416 and 608 pixels.
A round times each case once: the median over --reps launches after 5 warm-up launches, with
the shader clock stamped around the timed launches (csrc/clock.hip).  The post cases run in
--rounds alternating rounds (existing kernel, head kernel, ..., again), so that a drift of the
clock or of the box shows as spread; "ms" is the median of the round medians and "ms_range"
their minimum and maximum.  Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("dnn-inference-engine_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(REPO, p))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-forward", action="store_true")
    a = ap.parse_args()

    import numpy as np
    import torch

    import dnn_hip
    import post_head_oracle as O
    import synth
    import yolo_graph
    import yolo_post

    dev = torch.device("cuda", 0)
    s = torch.cuda.Stream(dev)
    stream = s.cuda_stream
    clk = torch.zeros((2, 256, 4), dtype=torch.int64, device=dev)

    def timed(launch):
        """Median ms per launch, and the mean shader clock over the timed launches."""
        for _ in range(5):
            launch()
        s.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.reps)]
        dnn_hip.clock_stamp(clk[0].data_ptr(), 256, stream)
        with torch.cuda.stream(s):
            for e0, e1 in ev:
                e0.record(s)
                launch()
                e1.record(s)
        dnn_hip.clock_stamp(clk[1].data_ptr(), 256, stream)
        s.synchronize()
        c = dnn_hip.sclk_from_stamps(clk[0].cpu().numpy(), clk[1].cpu().numpy())
        return (round(statistics.median(e0.elapsed_time(e1) for e0, e1 in ev), 4),
                round(c["mean"], 3) if c else None)

    out = {"reps": a.reps, "rounds": a.rounds, "post_ms": {}, "forward_ms": {}}
    cases = []

    def post_case(name, head, preds, old=False):
        n = len(preds)
        x = torch.from_numpy(np.ascontiguousarray(preds)).to(dev)
        buf = yolo_post.DetectionBuffers(n, dev, head=None if old else head)
        cases.append((name, head, x, buf, []))

    rng = np.random.default_rng(7)
    h13, h19, h40 = (yolo_post.YoloHead(g) for g in (13, 19, 40))
    p13 = np.stack([O.synthetic_predictions(rng, h13) for _ in range(64)])
    p19 = np.stack([O.synthetic_predictions(rng, h19) for _ in range(64)])
    p40 = O.synthetic_predictions(np.random.default_rng(205), h40, saturate=True)[None]
    post_case("13x13_existing_kernel", h13, p13, old=True)
    post_case("13x13_head_kernel", h13, p13)
    post_case("19x19_head_kernel", h19, p19)
    post_case("40x40_saturated_1_image", h40, p40)
    for _ in range(a.rounds):
        for name, head, x, buf, got in cases:
            got.append(timed(lambda: buf.run(x.data_ptr(), len(x), stream)))
    for name, head, x, buf, got in cases:
        counts = buf.counts.cpu().numpy()
        ms = [g[0] for g in got]
        out["post_ms"][name] = {"ms": round(statistics.median(ms), 4), "ms_range": [min(ms), max(ms)],
                                "sclk_ghz": [g[1] for g in got], "images": len(x), "boxes": head.boxes,
                                "detections": int(counts[counts > 0].sum()), "error_images": int((counts < 0).sum())}

    if not a.no_forward:
        ws = synth.yolo_weights()
        B = 64
        for hw in (320, 416, 608):
            shape = (hw, hw, 3)
            g, _ = yolo_graph.build_graph(dnn_hip.DnnGraphBuilder, ws, in_shape=(B,) + shape)
            entries = dnn_hip.lower_graph(g)
            wbytes, sbytes = dnn_hip.Plan.memory(B, shape, entries)
            wbuf = torch.empty(wbytes, dtype=torch.uint8, device=dev)
            sbuf = torch.empty(max(sbytes, 1), dtype=torch.uint8, device=dev)
            plan = dnn_hip.Plan(B, shape, entries, device=0, weights_ptr=wbuf.data_ptr(), workspace_ptr=sbuf.data_ptr())
            x = torch.rand((B,) + shape, device=dev)
            y = torch.empty((B, hw // 32, hw // 32, 125), device=dev)
            torch.cuda.synchronize()
            ms, ghz = timed(lambda: plan.run_device(B, x.data_ptr(), y.data_ptr(), stream))
            out["forward_ms"][str(hw)] = {"ms": ms, "sclk_ghz": ghz, "img_per_s": round(B / ms * 1e3)}
            del plan, wbuf, sbuf, x, y
    print(json.dumps(out))


if __name__ == "__main__":
    main()
