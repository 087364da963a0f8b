"""GPU: new_coords and DIoU NMS in the multi-scale decode (the dnn_yolo_postprocess_*_rule entries, MultiHead /
WideHead): rows equal to tests/post_rule_oracle.py in class, corners and score bits through the device and host
entries of both decodes; the codes; the refusals; the neutral rule; a narrow YOLOv4 with the scaled head.  Inputs lie
in [0, 1]; their seeds were chosen on the CPU so that the oracle's smallest margin is at least MIN_MARGIN."""
import collections
import ctypes

import numpy as np
import pytest

import act_oracle as AO
import darknet_import as D
import dnn_hip
import post_head_oracle as O
import post_multi_cases as MK
import post_multi_oracle as MO
import post_rule_oracle as RO
import ref_numpy as R
import v4tiny_cases as VK
import yolo_post

pytestmark = pytest.mark.gpu

KINDS = {"multi": yolo_post.MultiHead, "wide": yolo_post.WideHead}
MODES = {"per_class": ("per_class", "argmax"), "multi": ("per_class", "multi")}
SCORE_THR, IOU_THR, MIN_MARGIN, POISON = 0.1, 0.45, 1e-9, 0xA5
TALL = (1.0, 7.5, 2.0, 8.0, 3.0, 9.0)  # anchors taller than the image: every pair overlaps vertically, no zero denominator
# name: ((grid, cell, anchors in cells) per scale, classes, seed).  paths: 540 boxes, the class values scaled so that
# one class has more than PC_BIG = 256 candidates (the workgroup NMS) and another 65 to 256 (the wave NMS over a
# 64-candidate block); wide: every width above 2^25, the int128 paths; one: DIoU with one class, the per-class kernels
HEADS = {"paths": (((6, 32.0, TALL), (12, 16.0, (1.0, 15.0, 2.0, 16.0, 4.0, 18.0))), 3, 4),
         "wide": (((2, 32.0, (3.0e6, 2.0e6, 4.0e6, 5.0e6)),), 2, 2),
         "one": (((6, 32.0, TALL),), 1, 1)}


def _case(name):
    """(the oracle's description, one [1, g, g, n_out] array per scale, scale_x_y 2.0 per scale)."""
    scales, classes, seed = HEADS[name]
    multi = MO.Multi(tuple(O.Head(g, g, len(a) // 2, classes, a, cell, SCORE_THR, IOU_THR) for g, cell, a in scales), "logistic")
    rng, preds = np.random.default_rng(seed), []
    for h in multi.scales:
        p = rng.random((1, h.grid_h, h.grid_w, h.n_anchors, 5 + classes), dtype=np.float32)
        p[..., 5:] *= np.asarray((1.0, 0.8, 0.3)[:classes], np.float32)
        p[..., 2:4] = np.float32(0.5) + np.float32(0.5) * p[..., 2:4]  # sizes of 1 to 4 anchors
        preds.append(p.reshape(1, h.grid_h, h.grid_w, -1))
    return multi, preds, (2.0,) * len(scales)


def _device(head, preds, entry, lead):
    """One call of device entry `entry` (lead: its arguments before pred) on poisoned buffers: (rc, counts, dets' bytes, rows)."""
    import torch
    n, max_det = preds[0].shape[0], head.max_det
    xs = [torch.from_numpy(np.array(p)).cuda() for p in preds]
    ptrs = (ctypes.c_void_p * len(xs))(*[x.data_ptr() for x in xs])
    dets = torch.full((n, max_det, 40), POISON, dtype=torch.uint8, device="cuda")
    counts = torch.full((n * 4,), POISON, dtype=torch.uint8, device="cuda")
    ws = torch.full((head.workspace_bytes(n),), POISON, dtype=torch.uint8, device="cuda")
    rc = getattr(dnn_hip.mylib, entry)(ctypes.byref(head.c), *lead, ptrs, n, dets.data_ptr(), max_det, counts.data_ptr(),
                             ws.data_ptr(), ws.numel(), yolo_post.NMS_MODES[head.nms], yolo_post.LABEL_MODES[head.labels],
                             torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    c, d = counts.cpu().numpy().view(np.int32), dets.cpu().numpy()
    if rc:
        assert (c.view(np.uint8) == POISON).all() and (d == POISON).all() and (ws.cpu().numpy() == POISON).all()  # nothing ran
        return rc, None, None, None
    return rc, [int(v) for v in c], d.tobytes(), yolo_post.DetectionBuffers.to_rows(d, c, max_det, raise_errors=False)


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("name,beta", [("paths", 0.6), ("paths", 1.0), ("wide", 0.6), ("one", 0.6)])
def test_rows_equal_the_oracles(name, beta, mode):
    multi, preds, xy = _case(name)
    img = [p[0] for p in preds]
    want, margin = RO.detect(img, multi, xy, mode, True, "diou", beta)
    assert want and margin >= MIN_MARGIN  # a condition on the inputs: the device's pow may differ from libm's in the last place
    if name == "paths":
        assert want != RO.detect(img, multi, xy, mode, True, "iou")[0]  # the penalty decides: it cannot be ignored
        sizes = sorted(collections.Counter(c[2] for c in RO.candidates_new(img, multi, xy, mode)).values())
        assert sizes[-1] > 256 and any(65 <= n <= 256 for n in sizes), sizes
    assert name != "wide" or max(abs(v) for r in want for v in r[1:5]) > 2 ** 25
    for kind, cls in sorted(KINDS.items()):
        head = cls(multi.scales, "logistic", *MODES[mode], scale_x_y=xy, new_coords=True, nms_kind="diou", beta_nms=beta)
        rc, _, _, rows = _device(head, preds, f"dnn_yolo_postprocess_{kind}_rule", (head.xy, ctypes.byref(head.rule)))
        assert rc == 0 and rows == [want], (kind, dnn_hip.last_error())
        assert yolo_post.detect_batch_multi(preds, head) == [want], kind  # the _rule_host entry, through the head


@pytest.mark.parametrize("mode", sorted(MODES))
def test_codes_per_image_and_the_objectness_gate(mode):
    """1 x 1 x 3 boxes, cell 4, q = (x, y, w, h, conf, p0, p1).  Image 0: zero-size boxes at (0, 0) and (2, 3), whose
    unclamped intersection (-1)(-2) equals the sum of their areas; image 1: a NaN in q[2]; image 2: clean.  The third
    box has p0 = 8 and conf 0.05 <= score_thr: conf * p0 is above the threshold and the gate alone keeps it out."""
    multi = MO.Multi((O.Head(1, 1, 3, 2, (1.0,) * 6, 4.0, SCORE_THR, IOU_THR),), "logistic")
    a, b = (0.0, 0.0, 0.0, 0.0, 0.9, 0.9, 0.0), (0.5, 0.75, 0.0, 0.0, 0.8, 0.9, 0.0)
    far, gated = (0.5, 0.75, 0.5, 0.5, 0.8, 0.9, 0.0), (0.25, 0.25, 0.5, 0.5, 0.05, 8.0, 0.0)
    preds = [np.array([a + b + gated, (0.0, 0.0, np.nan) + a[3:] + far + gated, a + far + gated], np.float32).reshape(3, 1, 1, 21)]
    want = [RO.detect_or_code([preds[0][i]], multi, (1.0,), mode, new_coords=True, nms_kind="diou") for i in range(3)]
    assert want[:2] == [-2, -1] and len(want[2]) == 2
    for kind, cls in sorted(KINDS.items()):
        head = cls(multi.scales, "logistic", *MODES[mode], new_coords=True, nms_kind="diou")
        rc, counts, _, rows = _device(head, preds, f"dnn_yolo_postprocess_{kind}_rule", (None, ctypes.byref(head.rule)))
        assert rc == 0 and counts == [-2, -1, 2] and rows == want, kind


@pytest.mark.parametrize("kind", sorted(KINDS))
@pytest.mark.parametrize("class_mode,nms,rule,word", [("logistic", "any", (1, 1, 0.6), "per class"),
                                                      ("softmax", "per_class", (1, 0, 0.6), "class_mode"),
                                                      ("logistic", "per_class", (1, 1, 0.0), "beta_nms")])
def test_a_bad_rule_returns_minus_two_before_any_launch(class_mode, nms, rule, word, kind):
    multi, preds, _ = _case("wide")
    head = KINDS[kind](multi.scales, class_mode, nms)
    rc = _device(head, preds, f"dnn_yolo_postprocess_{kind}_rule", (None, ctypes.byref(yolo_post.RuleStruct(*rule))))[0]
    assert rc == -2 and word in dnn_hip.last_error(), dnn_hip.last_error()


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_a_neutral_rule_gives_the_xy_entrys_bytes(kind):
    grids, classes, _, _, thr = MK.PARITY["small"]
    multi, (preds, _) = MK.yolov3_multi(grids, classes, score_thr=thr), MK.parity("small")
    head = KINDS[kind](multi.scales, multi.class_mode, "per_class", "multi")
    rc0, counts0, dets0, _ = _device(head, preds, f"dnn_yolo_postprocess_{kind}_xy", (None,))
    assert rc0 == 0 and any(c > 0 for c in counts0)
    for rule in (None, ctypes.byref(yolo_post.RuleStruct())):
        assert _device(head, preds, f"dnn_yolo_postprocess_{kind}_rule", (None, rule))[:3] == (0, counts0, dets0)


def test_imported_narrow_yolov4_with_the_scaled_head(tmp_path):
    cfg = D.cfg_text("yolov4", width=64, height=64, width_div=8, classes=3, scaled_head=True)
    secs = D.parse_cfg(cfg, D.ACTIVATIONS)
    layers = VK.random_layers(secs)
    for layer in layers:  # gamma x 0.7, as the stock head's test: the signal neither grows nor dies over 110 layers
        if "scales" in layer:
            layer["scales"] = layer["scales"] * np.float32(0.7)
    x = np.random.default_rng(5).uniform(0, 1, (2, 64, 64, 3)).astype(np.float32)
    want = AO.forward(secs, layers, x)
    D.save_weights(tmp_path / "v4s.weights", layers)
    m = D.DarknetModel(cfg, str(tmp_path / "v4s.weights"), in_shape=[2, 64, 64, 3], score_thr=0.3)
    assert (m.head.new_coords, m.head.nms_kind, m.head.beta_nms, m.head.scale_x_y) == (True, "diou", 0.6, (2.0,) * 3)
    outs = [o.copy() for o in m.inference(x)]
    for o, w in zip(outs, want):
        assert o.shape == w.shape and 0 <= o.min() and o.max() <= 1 and R.normwise_err(o, w) < 1e-4
    multi, rows = MO.Multi(tuple(m.head.scales), "logistic"), m.detect(x, raise_errors=False)
    for i in range(2):
        ref = RO.detect([o[i] for o in outs], multi, m.head.scale_x_y, "multi", True, "diou", 0.6)[0]
        assert ref and rows[i] == ref, i
