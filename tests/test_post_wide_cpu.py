"""Host-only checks of the grid-wide decode: the four dnn_yolo_*wide* entries in both libraries,
dnn_yolo_wide_boxes' validation and the workspace size, WideHead beside MultiHead, the importer's
`wide` switch, and the conditions the seeded GPU cases of tests/post_wide_cases.py rely on."""
import ctypes
import os
import re

import numpy as np
import pytest

import darknet_cases as DC
import darknet_import as D
import dnn_hip
import post_multi_oracle as MO
import post_multilabel_oracle as LO
import post_wide_cases as W
import yolo_post
from conftest import LIBS, REPO

lib = dnn_hip.mylib
WIDE_ENTRIES = ("dnn_yolo_wide_boxes", "dnn_yolo_wide_workspace", "dnn_yolo_postprocess_wide",
                "dnn_yolo_postprocess_wide_host")


def _head(grid, anchors=(1.0, 2.0, 3.0, 4.0, 5.0, 6.0), classes=80, cell=32.0, score_thr=0.3, iou_thr=0.3):
    return yolo_post.HeadStruct(grid, grid, len(anchors) // 2, classes, cell, score_thr, iou_thr,
                                (ctypes.c_float * 32)(*anchors))


def _multi(heads, class_mode=1, n_scales=None):
    m = yolo_post.MultiStruct()
    m.n_scales = len(heads) if n_scales is None else n_scales
    m.class_mode = class_mode
    for k, h in enumerate(heads[:4]):
        m.scale[k] = h
    return m


def _boxes(m):
    return lib.dnn_yolo_wide_boxes(ctypes.byref(m))


@pytest.mark.parametrize("path", LIBS)
def test_both_libraries_export_the_wide_entries(path):
    so = ctypes.CDLL(path)
    for name in WIDE_ENTRIES:
        assert hasattr(so, name), f"{os.path.basename(path)} lacks {name}"


def test_the_header_and_python_agree_on_the_limit():
    with open(os.path.join(REPO, "include", "dnn_hip_post.h")) as f:
        text = f.read()
    assert int(re.search(r"#define DNN_YOLO_WIDE_MAX_BOXES (\d+)", text).group(1)) == yolo_post.WIDE_MAX_BOXES == 65536
    assert int(re.search(r"#define DNN_YOLO_MULTI_MAX_BOXES (\d+)", text).group(1)) == yolo_post.MULTI_MAX_BOXES == 16384
    for name in WIDE_ENTRIES:
        assert re.search(r"\bint " + name + r"\(", text), name


def test_wide_boxes_counts_and_refusals():
    assert _boxes(_multi([_head(19), _head(38), _head(76)])) == 22743
    assert _boxes(_multi([_head(32), _head(64), _head(128)])) == 64512   # YOLOv3 at 1024 x 1024
    assert _boxes(_multi([_head(13)], class_mode=0)) == 507
    assert lib.dnn_yolo_wide_boxes(None) < 0
    for bad, word in (  # everything dnn_yolo_multi_boxes refuses (tests/test_post_multi_cpu.py)
            (_multi([_head(13)], n_scales=0), "scales"),
            (_multi([_head(2)] * 4, n_scales=5), "scales"),
            (_multi([_head(13), _head(26, classes=79)]), "agree"),
            (_multi([_head(13), _head(26, score_thr=0.5)]), "agree"),
            (_multi([_head(13), _head(26, iou_thr=0.45)]), "agree"),
            (_multi([_head(13)], class_mode=2), "class_mode"),
            (_multi([_head(13), _head(0)]), "cell"),
            (_multi([_head(13, classes=129)]), "classes"),
            (_multi([_head(13, cell=0.0)]), "cell"),
    ):
        assert _boxes(bad) == -2
        assert word in dnn_hip.last_error(), (word, dnn_hip.last_error())
        assert lib.dnn_yolo_multi_boxes(ctypes.byref(bad)) == -2
    four = (1.0,) * 8
    at_limit = _multi([_head(128, anchors=four)])
    assert _boxes(at_limit) == 65536
    above = _multi([_head(128, anchors=four), _head(1, anchors=(1.0, 1.0))])
    assert _boxes(above) == -2 and "65537 boxes" in dnn_hip.last_error()
    assert _boxes(_multi([_head(148)])) == -2 and "65712" in dnn_hip.last_error()  # one scale alone
    b = ctypes.c_ulonglong()
    assert lib.dnn_yolo_wide_workspace(ctypes.byref(at_limit), 3, ctypes.byref(b)) == 0
    assert b.value == 3 * (65536 * 40 + 16384 * 8 + 64) and b.value % 8 == 0
    assert lib.dnn_yolo_wide_workspace(ctypes.byref(at_limit), 0, ctypes.byref(b)) == 0 and b.value == 0
    assert lib.dnn_yolo_wide_workspace(ctypes.byref(above), 3, ctypes.byref(b)) == -2
    assert lib.dnn_yolo_wide_workspace(ctypes.byref(at_limit), -1, ctypes.byref(b)) != 0
    # the existing entries keep their limit
    assert lib.dnn_yolo_multi_boxes(ctypes.byref(_multi([_head(19), _head(38), _head(76)]))) == -2
    assert "> 16384" in dnn_hip.last_error()  # (the stride-8 scale alone is above it)


def test_wide_entry_refuses_bad_modes_before_any_launch():
    m = _multi([_head(19), _head(38), _head(76)])
    ptrs = (ctypes.c_void_p * 3)(8, 8, 8)  # never read: every call below is refused on the host
    entry = lib.dnn_yolo_postprocess_wide
    for nms, labels, word in ((0, 1, "labels_mode"), (2, 0, "nms_mode"), (1, 2, "labels_mode"), (-1, 0, "nms_mode")):
        assert entry(ctypes.byref(m), ptrs, 1, 8, 4, 8, 8, 1 << 40, nms, labels, None) == -2
        assert word in dnn_hip.last_error(), (word, dnn_hip.last_error())
        assert lib.dnn_yolo_postprocess_wide_host(ctypes.byref(m), ptrs, 1, 8, 4, 8, nms, labels) == -2
    need = 22743 * 40 + 16384 * 8 + 64
    assert entry(ctypes.byref(m), ptrs, 1, 8, 4, 8, 8, need - 1, 1, 1, None) == -2 and "workspace" in dnn_hip.last_error()
    assert entry(ctypes.byref(m), ptrs, 1, 8, 4, 8, 12, need, 1, 1, None) == -2 and "aligned" in dnn_hip.last_error()
    assert entry(ctypes.byref(m), ptrs, 1, 8, 4, 8, None, need, 1, 1, None) == -2
    assert entry(ctypes.byref(m), ptrs, -1, 8, 4, 8, 8, need, 1, 1, None) == -2
    assert entry(ctypes.byref(m), (ctypes.c_void_p * 3)(8, None, 8), 1, 8, 4, 8, 8, need, 1, 1, None) == -2
    assert "pred[1]" in dnn_hip.last_error()
    assert entry(ctypes.byref(m), ptrs, 0, None, 4, None, None, 0, 1, 1, None) == 0  # no images: nothing to do


def test_widehead_beside_multihead():
    h = yolo_post.WideHead.yolov3(608, 608)
    assert isinstance(h, yolo_post.MultiHead) and h.boxes == 22743 and h.max_det == 16384
    assert h.scale_boxes == [1083, 4332, 17328] and h.pred_shapes == [(19, 19, 255), (38, 38, 255), (76, 76, 255)]
    assert repr(h).startswith("WideHead(19x19x3, 38x38x3, 76x76x3; 80 classes, logistic")
    assert h.workspace_bytes(2) == 2 * (22743 * 40 + 16384 * 8 + 64)
    m = yolo_post.WideHead.yolov3(608, 608, nms="per_class", labels="multi")
    assert (m.nms, m.labels, m.max_det) == ("per_class", "multi", 16384) and m.workspace_bytes(1) == h.workspace_bytes(1)
    small = yolo_post.WideHead.yolov3_tiny(64, 64, 3, nms="per_class", labels="multi")
    assert small.boxes == 60 and small.max_det == 180 and yolo_post.WideHead.yolov3_tiny(64, 64, 3).max_det == 60
    assert yolo_post.WideHead.yolov3(1024, 1024).boxes == 64512
    with pytest.raises(ValueError, match="68607 boxes over 3 scales: need <= 65536"):
        yolo_post.WideHead.yolov3(1056, 1056)
    with pytest.raises(ValueError, match='labels "multi" needs nms "per_class"'):
        yolo_post.WideHead.yolov3(608, 608, labels="multi")
    # MultiHead is what it was
    with pytest.raises(ValueError, match="22743 boxes over 3 scales: need <= 16384"):
        yolo_post.MultiHead.yolov3(608, 608)
    old = yolo_post.MultiHead.yolov3(416, 416)
    assert repr(old).startswith("MultiHead(13x13x3") and old.max_det == 10647 and old.workspace_bytes(1) == 10647 * 40
    assert yolo_post.MultiHead.yolov3(416, 416, nms="per_class", labels="multi").max_det == 16384
    assert sorted(yolo_post.ERRORS) == [-3, -2, -1]
    with pytest.raises(ValueError, match="2 prediction tensors for 3 scales"):
        yolo_post.detect_batch_multi([np.zeros(1), np.zeros(1)], h)
    assert yolo_post.detect_batch_multi([np.zeros((0,) + s, np.float32) for s in h.pred_shapes], h) == []


def test_importer_builds_a_widehead_on_request():
    """The narrow 608 x 608 cfg of test_model_above_the_box_limit_is_built_without_a_head."""
    cfg = D.cfg_text("yolov3", classes=3, width=608, height=608, width_div=8)
    secs = D.parse_cfg(cfg)
    layers = DC.darknet_layers(secs)
    m = D.DarknetModel(cfg, layers, wide=True)
    assert isinstance(m.head, yolo_post.WideHead) and m.head.boxes == 22743 and m.head.max_det == 16384
    assert (m.head.score_thr, m.head.iou_thr, m.head.nms, m.head.labels, m.head.class_mode) == \
        (0.5, 0.45, "per_class", "multi", "logistic")
    assert m.head.pred_shapes == [(19, 19, 24), (38, 38, 24), (76, 76, 24)]
    m = D.DarknetModel(cfg, layers, wide=True, score_thr=0.25, nms="any", labels="argmax")
    assert (m.head.score_thr, m.head.nms, m.head.labels) == (0.25, "any", "argmax")
    small = D.DarknetModel(cfg, layers, in_shape=[1, 416, 416, 3], wide=True)
    assert isinstance(small.head, yolo_post.WideHead) and small.head.boxes == 10647  # whatever the box count
    # the default is what it was
    m = D.DarknetModel(cfg, layers)
    assert m.head is None
    with pytest.raises(ValueError, match="22743 boxes"):
        m.detect(np.zeros((1, 608, 608, 3), np.float32))
    assert type(D.DarknetModel(cfg, layers, in_shape=[1, 416, 416, 3]).head) is yolo_post.MultiHead
    assert type(D.multi_head(small.yolos, 416, 416)) is yolo_post.MultiHead
    assert type(D.multi_head(m.yolos, 608, 608, wide=True)) is yolo_post.WideHead
    # YOLO_V3 takes a WideHead as any other head
    import synth
    import yolov3
    y = yolov3.YOLO_V3([1, 608, 608, 3], synth.yolov3_weights(width_div=8, n_out=24), False,
                       head=yolo_post.WideHead.yolov3(608, 608, 3))
    assert isinstance(y.head, yolo_post.WideHead)


# ------------------------------------------------------------------ the seeded cases stay inside their conditions
@pytest.mark.parametrize("name", sorted(W.ABOVE))
def test_above_cases_have_a_coded_image_and_rows_of_high_boxes(name):
    multi = W.above_multi(name)
    assert W.boxes_of(multi) == {"four": 17391, "yolov3": 22743}[name] > W.OLD_CAP
    preds, refs, high = W.above(name)
    print(name, {m: W.counts_of(r) for m, r in refs.items()}, high)
    assert preds[0].shape[0] in (3, 4)
    for mode in W.MODES:
        codes = sum(isinstance(r, int) for r in refs[mode])
        assert 1 <= codes <= len(refs[mode]) / 4, mode
        assert high[mode] >= 1, mode
        assert max(W.counts_of(refs[mode])) <= 512  # the GPU test's max_det
    assert W.above_ok(refs, high)
    if name == "four":  # the scale boundaries and the total fall inside decode chunks, whatever their size
        offs = np.cumsum([MO.scale_boxes(h) for h in multi.scales])
        assert all(int(o) % 64 for o in offs)


def test_small_cases_keep_the_properties_they_were_chosen_for():
    """From the oracles: what each case of post_wide_cases.SMALL sends through the device's phases
    (csrc/post_multi_dev.h: PC_BIG = 256 candidates, merge chunks of 1024 rows)."""
    big, chunk = 256, 1024
    per, rows = {}, {}
    for name in W.SMALL:
        multi, preds, mode, want, stats = W.small(name)
        assert W.boxes_of(multi) <= W.OLD_CAP and mode == W.SMALL[name] and len(want) == preds[0].shape[0]
        rows[name] = W.counts_of(want)
        if stats is not None:
            per[name] = tuple(np.bincount(stats["classes"], minlength=multi.scales[0].n_classes))
    # every segment goes to the whole workgroup; the merge expands three chunks from the top down
    assert len(per["dense"]) == 12 and min(per["dense"]) > big and rows["dense"][0] > 2 * chunk
    # every segment is one wave's, none empty; the merge has a second chunk
    assert len(per["dense80"]) == 80 and 1 <= min(per["dense80"]) and max(per["dense80"]) <= big
    assert rows["dense80"][0] > chunk
    assert per["bounds"] == (1, 63, 64, 0, 65, 129) and rows["bounds"][0] > 0
    assert per["threshold"] == (big, big + 1, big - 1, 320) and rows["threshold"][0] > chunk // 2
    # softmax multi-label rows beside a code; small_softmax stands in for a softmax case of more than
    # 1024 rows only while post_multilabel_cases.SEEDED has none
    import post_multilabel_cases as LK
    for seeded, spec in LK.SEEDED.items():
        if spec[5] == "softmax":
            assert max(LK.counts_of(LK.seeded(seeded)[1])) <= chunk, seeded
    assert W.small("small_softmax")[0].class_mode == "softmax"
    assert any(c > 0 for c in rows["small_softmax"]) and any(c < 0 for c in rows["small_softmax"])


def test_608_x_80_case_gives_rows_in_every_mode():
    preds, refs = W.coco608()
    assert W.boxes_of(W.coco608_multi()) == 22743 and preds[2].shape == (1, 76, 76, 255)
    for mode in W.MODES:
        assert not isinstance(refs[mode][0], int) and 100 <= len(refs[mode][0]) <= 1024, mode


def test_cap_cases_sit_exactly_at_and_one_above_the_cap():
    multi = W.cap_multi()
    assert W.boxes_of(multi) == 17391
    for mode, want in (("any", [1, -3, 1, -1, 0]), ("per_class", [3, -3, 3, -1, 0]), ("multi", [3, -3, 3, -1, 0])):
        preds, refs = W.cap(mode)
        assert W.counts_of(refs) == want, mode
    # the candidate counts: score = sigmoid(20) * sigmoid([3, 6]) > 0.3 for every label of an "on" box
    thr = np.float32(0.3)
    for on, want in ((16384, 16384), (16385, 16385)):
        assert sum(b[1] > thr for b in MO.decode(W.cap_image(on), multi)) == want
    for single, want in ((1, 16384), (2, 16385)):
        assert len(LO.candidates(W.cap_image(5461, single), multi)) == want


def test_edge_case_reaches_the_last_box():
    preds, refs = W.edge()
    multi = W.edge_multi()
    assert W.boxes_of(multi) == 65536 and W.EDGE_ON[-1] == 65535
    assert not isinstance(refs[0], int) and len(refs[0]) >= 3
    boxes = MO.decode([preds[0][0]], multi)
    last = tuple(boxes[65535][0])
    assert boxes[65535][1] > np.float32(0.3) and any(tuple(r[1:5]) == last for r in refs[0])


def test_end_to_end_threshold_gives_rows_of_high_boxes_on_the_darknet_oracle():
    cfg, _, layers, _ = W.e2e_model()
    m = D.DarknetModel(cfg, layers, wide=True, score_thr=W.E2E_LOW_THR)
    assert isinstance(m.head, yolo_post.WideHead) and m.head.boxes == 17340
    assert D.DarknetModel(cfg, layers).head is None
    rows, high = W.e2e_oracle(m.head)
    assert not isinstance(rows, int) and len(rows) >= 1 and high >= 1
    rows, _ = W.e2e_oracle(D.DarknetModel(cfg, layers, wide=True).head)
    assert not isinstance(rows, int)  # Darknet's 0.5: rows (here none), not a code
