"""Times the full YOLOv3 at 416 x 416 on one GPU: the plan (75 convs, 23 shortcuts, 2 upsamples,
2 routes, 2 taps), darknet53.py's plan beside it (what the trunk and the stride-32 branch cost
alone), and the three-scale decode of the 10,647 boxes on typical inputs (a few hundred
candidates per image) and on inputs where every box is a candidate.  --model picks the network:
yolov3 (the default, as above), yolov3_spp (76 convs and the spp entry; the decode is YOLOv3's),
yolov3_tiny (13 convs, two scales, 2,535 boxes), yolov4_tiny (the Darknet import of the public
cfg with random weights: 21 convs, 3 slices, 7 routes; its decode with scale_x_y = 1.05) or all
(the three YOLOv3 models).

  python tools/yolov3_time.py [--model yolov3] [--batch 1] [--reps 20] [--rounds 5] [--decode-only]

Each figure is the median over `rounds` of the device time of one run: HIP events around `reps`
back-to-back runs on one stream, after a warm-up.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(R, "dnn-inference-engine_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import darknet53  # noqa: E402
import darknet_import  # noqa: E402
import dnn_hip  # noqa: E402
import synth  # noqa: E402
import yolo_post  # noqa: E402
import yolov3  # noqa: E402
import yolov3_spp  # noqa: E402
import yolov3_tiny  # noqa: E402


def device_ms(fn, reps, rounds):
    """Median over rounds of (HIP-event time of reps calls) / reps, after one warm-up round."""
    out = []
    for r in range(rounds + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        if r:
            out.append(a.elapsed_time(b) / reps)
    return statistics.median(out)


def time_plan(g, batch, reps, rounds):
    plan = dnn_hip.Plan.from_graph(g, device=0)
    x = torch.from_numpy(synth.frames(range(batch))).cuda()
    y = torch.empty((batch,) + plan.out_shape, dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    ms = device_ms(lambda: plan.run_device(batch, x.data_ptr(), y.data_ptr(), stream), reps, rounds)
    nk = len(plan.kernels())
    wb = plan.weight_buffer()[1]
    plan.close()
    return {"ms": round(ms, 3), "kernels": nk, "weight_MiB": round(wb / 2 ** 20, 1)}


def predictions(head, batch, saturate, seed=0):
    """Random head tensors: normal logits; typical: objectness N(-6, 2) (about 1 box in 400 above
    0.3 before the class score); saturate: objectness 8 and one class logit of 12 on every box."""
    rng = np.random.default_rng(seed)
    out = []
    for s in head.scales:
        p = rng.standard_normal((batch, s.grid_h, s.grid_w, s.n_anchors, 5 + s.n_classes)).astype(np.float32)
        p[..., 4] = 8.0 if saturate else (rng.standard_normal(p.shape[:-1]) * 2.0 - 6.0)
        hot = rng.integers(0, s.n_classes, size=p.shape[:-1])
        np.put_along_axis(p[..., 5:], hot[..., None], np.float32(12.0 if saturate else 6.0), -1)
        out.append(torch.from_numpy(p.reshape(batch, s.grid_h, s.grid_w, -1)).cuda())
    return out


def time_decode(batch, reps, rounds, head=None):
    head = head or yolo_post.MultiHead.yolov3(416, 416)
    buf = yolo_post.MultiDetectionBuffers(batch, torch.device("cuda", 0), head)
    stream = torch.cuda.current_stream().cuda_stream
    out = {"boxes": head.boxes}
    for name, sat in (("typical", False), ("saturated", True)):
        preds = predictions(head, batch, sat)
        ptrs = [p.data_ptr() for p in preds]
        ms = device_ms(lambda: buf.run(ptrs, batch, stream), reps, rounds)
        counts = buf.counts.cpu().numpy()
        out[name] = {"ms": round(ms, 3), "counts": [int(c) for c in counts]}
    return out


def random_darknet_layers(sections, seed=0):
    """He-scaled kernels and BatchNorm statistics near the identity for every conv of a cfg, in
    load_weights' format (timing only: the values do not change what runs)."""
    rng = np.random.default_rng(seed)
    layers = []
    for n, c, size, bn in darknet_import.conv_shapes(sections):
        layer = {"biases": (rng.standard_normal(n) * 0.1).astype(np.float32),
                 "weights": (rng.standard_normal((n, c, size, size)) * np.sqrt(2.0 / (c * size * size))).astype(np.float32)}
        if bn:
            layer.update(scales=rng.uniform(0.75, 1.25, n).astype(np.float32),
                         rolling_mean=(rng.standard_normal(n) * 0.1).astype(np.float32),
                         rolling_variance=rng.uniform(0.5, 1.5, n).astype(np.float32))
        layers.append(layer)
    return layers


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--decode-only", action="store_true")
    ap.add_argument("--model", choices=("yolov3", "yolov3_spp", "yolov3_tiny", "yolov4_tiny", "all"), default="yolov3")
    a = ap.parse_args()
    shape = (a.batch, 416, 416, 3)
    res = {"batch": a.batch}
    if a.model in ("yolov3", "yolov3_spp", "all"):
        res["decode"] = time_decode(a.batch, a.reps, a.rounds)
    if a.model in ("yolov3_tiny", "all"):
        res["decode_tiny"] = time_decode(a.batch, a.reps, a.rounds, yolo_post.MultiHead.yolov3_tiny(416, 416))
    if a.model == "yolov4_tiny":
        secs = darknet_import.parse_cfg(darknet_import.cfg_text("yolov4-tiny"))
        g, _, yolos = darknet_import.build_graph(dnn_hip.DnnGraphBuilder, secs, random_darknet_layers(secs), shape)
        res["decode_v4_tiny"] = time_decode(a.batch, a.reps, a.rounds, darknet_import.multi_head(yolos, 416, 416))
        if not a.decode_only:
            res["yolov4_tiny_plan"] = time_plan(g, a.batch, a.reps, a.rounds)
    if not a.decode_only and a.model in ("yolov3_spp", "all"):
        ws = yolov3_spp.validate(synth.yolov3_spp_weights())
        res["yolov3_spp_plan"] = time_plan(yolov3_spp.build_graph(dnn_hip.DnnGraphBuilder, ws, in_shape=shape)[0],
                                           a.batch, a.reps, a.rounds)
    if not a.decode_only and a.model in ("yolov3_tiny", "all"):
        wt = yolov3_tiny.validate(synth.yolov3_tiny_weights())
        res["yolov3_tiny_plan"] = time_plan(yolov3_tiny.build_graph(dnn_hip.DnnGraphBuilder, wt, in_shape=shape)[0],
                                            a.batch, a.reps, a.rounds)
    if not a.decode_only and a.model in ("yolov3", "all"):
        w3 = yolov3.validate(synth.yolov3_weights())
        res["yolov3_plan"] = time_plan(yolov3.build_graph(dnn_hip.DnnGraphBuilder, w3, in_shape=shape)[0], a.batch,
                                       a.reps, a.rounds)
        wd = darknet53.validate(synth.darknet53_weights(n_out=255))
        res["darknet53_plan"] = time_plan(darknet53.build_graph(dnn_hip.DnnGraphBuilder, wd, in_shape=shape)[0],
                                          a.batch, a.reps, a.rounds)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
