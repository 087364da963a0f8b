"""Generate the multi-scale postprocessing fixtures under tests/golden/ from the REFERENCE's
own, unmodified function (build container only; /root/reference never exists on the GPU box):

    python tests/golden/make_golden_post_ms.py

The reference's postprocessing (cs492-projects/proj3/yolov2tiny.py:94-177) is fixed at
13 x 13 cells.  A smaller VOC-shaped grid (5 anchors, 20 classes) can still be pinned against
it: embedded in the top-left of a [13,13,125] tensor whose other cells have objectness -20
(tests/post_head_oracle.embed_in_13x13), the boxes of the small grid keep their cell
coordinates and their (row, col, anchor) order, and no other box reaches the threshold, so
the reference returns exactly the small grid's detections.  As make_golden_post.py does, this
script parses the reference file, compiles only its postprocessing functions with numpy in
scope and calls them; nothing of the reference is copied into the repository.

Writes  post_ms_cases.npz    inputs: one fp32 array [grid_h, grid_w, 125] per case name
        post_ms_golden.json  per case {"grid": [grid_h, grid_w], "boxes": the reference's
                             label_boxes as [class name, [left, top], [right, bottom]]}, or
                             "raises": "ZeroDivisionError" in place of "boxes"
Cases: 10 x 10, 7 x 13, 2 x 3 and 1 x 1 cells at 3 seeds each, from
post_head_oracle.synthetic_predictions (the third seed of each with 6x box-size logits).
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(REPO, "oracle"))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, HERE)
import post_head_oracle as O  # noqa: E402
from make_golden_post import load_reference_postprocessing  # noqa: E402

GRIDS = ((10, 10), (7, 13), (2, 3), (1, 1))
SEEDS = (11, 12, 13)


def cases():
    out = {}
    for gh, gw in GRIDS:
        head = O.voc_head(gh, gw)
        for i, seed in enumerate(SEEDS):
            rng = np.random.default_rng(1000 * gh + 10 * gw + seed)
            out[f"grid{gh}x{gw}_seed{seed}"] = O.synthetic_predictions(rng, head, tw_scale=(6.0 if i == 2 else 1.0))
    return out


def main():
    ref_post = load_reference_postprocessing()
    preds = cases()
    gold = {}
    for name, p in preds.items():
        gh, gw = p.shape[:2]
        try:
            boxes = ref_post(O.embed_in_13x13(p, O.voc_head(gh, gw)))
        except ZeroDivisionError:
            gold[name] = {"grid": [gh, gw], "raises": "ZeroDivisionError"}
            print(f"{name:22s} raises ZeroDivisionError")
            continue
        gold[name] = {"grid": [gh, gw], "boxes": [[b[0], list(b[1]), list(b[2])] for b in boxes]}
        print(f"{name:22s} {len(boxes):4d} detections")
    np.savez_compressed(os.path.join(HERE, "post_ms_cases.npz"), **preds)
    with open(os.path.join(HERE, "post_ms_golden.json"), "w") as f:
        json.dump({"source": "cs492-projects/proj3/yolov2tiny.py:94-234 (postprocessing, unmodified, on the "
                             "13 x 13 embedding) under numpy " + np.__version__, "cases": gold}, f, indent=0)


if __name__ == "__main__":
    main()
