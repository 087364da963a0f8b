"""Host-only checks of the multi-scale decode: dnn_yolo_multi_boxes' validation, MultiHead's
mirror of it, the numpy oracle (tests/post_multi_oracle.py) against post_head_oracle where they
must agree, and the conditions the seeded GPU batches of tests/post_multi_cases.py rely on."""
import ctypes
import json

import numpy as np
import pytest

import dnn_hip
import post_head_cases as HK
import post_head_oracle as O
import post_multi_cases as K
import post_multi_oracle as MO
import post_numpy as PN
import yolo_post

lib = dnn_hip.mylib


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
    return lib.dnn_yolo_multi_boxes(ctypes.byref(m))


def test_multi_boxes_counts_and_refusals():
    assert _boxes(_multi([_head(13), _head(26), _head(52)])) == 10647
    assert _boxes(_multi([_head(16), _head(32), _head(64)])) == 16128  # 64 * 64 * 3 alone is above 8192
    assert _boxes(_multi([_head(13)], class_mode=0)) == 507
    assert _boxes(_multi([_head(2)] * 4)) == 48
    assert lib.dnn_yolo_multi_boxes(None) < 0
    for bad, word in (
            (_multi([_head(13)], n_scales=0), "scales"),
            (_multi([_head(2)] * 4, n_scales=5), "scales"),
            (_multi([_head(13), _head(26, classes=79)]), "agree"),
            (_multi([_head(13), _head(26, score_thr=0.5)]), "agree"),
            (_multi([_head(13), _head(26, iou_thr=0.45)]), "agree"),
            (_multi([_head(16), _head(32), _head(64), _head(17, anchors=(1.0, 1.0))]), "16417 boxes"),  # 16128 + 289
            (_multi([_head(13)], class_mode=2), "class_mode"),
            (_multi([_head(13), _head(0)]), "cell"),
            (_multi([_head(13, classes=129)]), "classes"),
            (_multi([_head(13, cell=0.0)]), "cell"),
    ):
        assert _boxes(bad) == -2
        assert word in dnn_hip.last_error(), (word, dnn_hip.last_error())
    # exactly at the cap, and one box above it
    at_cap = _multi([_head(64), _head(32), _head(32, anchors=(1.0, 1.0))])       # 12288 + 3072 + 1024
    assert _boxes(at_cap) == 16384
    above = _multi([_head(64), _head(32), _head(32, anchors=(1.0, 1.0)), _head(1, anchors=(1.0, 1.0))])
    assert _boxes(above) == -2 and "16385 boxes" in dnn_hip.last_error()
    b = ctypes.c_ulonglong()
    assert lib.dnn_yolo_multi_workspace(ctypes.byref(at_cap), 3, ctypes.byref(b)) == 0 and b.value == 3 * 16384 * 40
    assert lib.dnn_yolo_multi_workspace(ctypes.byref(above), 3, ctypes.byref(b)) == -2
    # the single-head entry keeps its own limit
    assert lib.dnn_yolo_head_boxes(ctypes.byref(_head(64))) == -2
    assert yolo_post.MAX_BOXES == 8192


def test_multihead_mirrors_the_c_checks():
    h = yolo_post.MultiHead.yolov3(416, 416)
    assert h.boxes == 10647 and h.scale_boxes == [507, 2028, 8112] and h.n_out == [255] * 3
    assert h.pred_shapes == [(13, 13, 255), (26, 26, 255), (52, 52, 255)] and h.class_mode == "logistic"
    assert h.scales[0].anchors == (116 / 32, 90 / 32, 156 / 32, 198 / 32, 373 / 32, 326 / 32)
    assert h.scales[2].anchors[:2] == (10 / 8, 13 / 8) and [s.cell for s in h.scales] == [32.0, 16.0, 8.0]
    for s in h.scales:  # pixels / stride is exact in fp32
        assert all(np.float32(a) * np.float32(s.cell) == np.float32(a * s.cell) for a in s.anchors)
    assert yolo_post.MultiHead.yolov3(512, 512, classes=1).boxes == 16128
    assert h.workspace_bytes(2) == 2 * 10647 * 40
    s0 = h.scales[0]
    V = ValueError
    with pytest.raises(V):
        yolo_post.MultiHead.yolov3(608, 608)  # 22,743 boxes
    with pytest.raises(V):
        yolo_post.MultiHead.yolov3(416, 400)
    with pytest.raises(V):
        yolo_post.MultiHead([])
    with pytest.raises(V):
        yolo_post.MultiHead([s0] * 5)
    with pytest.raises(V):
        yolo_post.MultiHead([s0], class_mode="sigmoid")
    with pytest.raises(V):
        yolo_post.MultiHead([s0, h.scales[1]._replace(n_classes=3)])
    with pytest.raises(V):
        yolo_post.MultiHead([s0, h.scales[1]._replace(score_thr=0.5)])
    with pytest.raises(V):
        yolo_post.MultiHead([s0, h.scales[1]._replace(iou_thr=0.5)])
    with pytest.raises(V):
        yolo_post.MultiHead([s0._replace(n_classes=129)])
    with pytest.raises(V):
        yolo_post.MultiHead([s0._replace(cell=float("inf"))])
    with pytest.raises(V):
        yolo_post.MultiHead([s0._replace(anchors=s0.anchors[:5])])
    with pytest.raises(V):
        yolo_post.MultiHead([s0._replace(grid_h=0)])
    # YoloHead objects are scales too, softmax heads included
    m = yolo_post.MultiHead([yolo_post.YoloHead(13), yolo_post.YoloHead(7)], "softmax")
    assert m.boxes == (169 + 49) * 5 and m.names == yolo_post.CLASSES
    with pytest.raises(V):
        yolo_post.detect_batch_multi([np.zeros((1, 13, 13, 125), np.float32)], m)


# ------------------------------------------------------------------------------ the oracle
def test_oracle_with_one_softmax_scale_is_the_head_oracle():
    n = 0
    for name, (pred, gold) in HK.ms_golden().items():
        head = O.voc_head(*gold["grid"])
        want = O.detect_or_code(pred, head)
        assert MO.detect_or_code([pred], MO.Multi((head,), "softmax")) == want, name
        assert (want == -2) == ("raises" in gold), name
        n += 0 if isinstance(want, int) else len(want)
    assert n > 400


def test_oracle_global_order_and_logistic_rule():
    """Two scales: the global index is scale 0's boxes first; the logistic class is the first index
    of the largest ROUNDED probability (logits 20 and 30 both give 1.0f) and the score conf * p."""
    a = O.Head(1, 2, 1, 3, (1.0, 1.0), 32.0, 0.3, 0.3)
    b = O.Head(2, 1, 1, 3, (1.0, 1.0), 16.0, 0.3, 0.3)
    pa = np.zeros((1, 2, 8), np.float32)
    pb = np.zeros((2, 1, 8), np.float32)
    pa[0, 1, 4:] = (2.0, -1.0, 20.0, 30.0)
    pb[1, 0, 4:] = (1.0, 3.0, 0.5, 3.0)
    multi = MO.Multi((a, b), "logistic")
    boxes = MO.decode([pa, pb], multi)
    assert len(boxes) == 4
    assert boxes[1][2] == 1 and boxes[1][1] == PN._sigmoid(np.float32(2.0)) * np.float32(1.0)
    assert PN._sigmoid(np.float32(20.0)) == PN._sigmoid(np.float32(30.0)) == np.float32(1.0)
    assert boxes[3][2] == 0 and boxes[3][1] == np.float32(PN._sigmoid(np.float32(1.0)) * PN._sigmoid(np.float32(3.0)))
    assert boxes[0][0] == [0, 0, 32, 32] and boxes[2][0] == [0, 0, 16, 16] and boxes[3][0] == [0, 16, 16, 32]
    assert boxes[0][2] == 0 and boxes[0][1] == np.float32(0.25)  # all-zero logits: 0.5 * 0.5, class 0
    # the brute-force logistic rule on every class agrees with the pruned evaluation
    rng = np.random.default_rng(0)
    head = K.yolov3_multi((2, 4, 8), 80).scales[1]
    pred = O.synthetic_predictions(rng, head)
    p = O.as_boxes(pred, head)
    for (row, col, anc), got in zip(np.ndindex(4, 4, 3), MO.decode_scale(pred, head, "logistic")):
        probs = [PN._sigmoid(v) for v in p[row, col, anc, 5:]]
        best = max(range(80), key=lambda k: (probs[k], -k))
        conf = PN._sigmoid(p[row, col, anc, 4])
        assert got[2] == best and got[1] == np.float32(conf * probs[best])


@pytest.mark.parametrize("name", sorted(K.PARITY))
def test_seeded_batches_meet_their_conditions(name):
    """At most a quarter of a batch's images carry an error code and at least one does; the clean
    images yield detections from more than one scale."""
    grids, classes, n, _, thr = K.PARITY[name]
    preds, refs = K.parity(name)
    assert [p.shape for p in preds] == [(n, g, g, 3 * (5 + classes)) for g in grids]
    codes = [r for r in refs if isinstance(r, int)]
    print(f"{name}: {len(codes)} of {n} images carry an error code {codes}; detections "
          f"{[r if isinstance(r, int) else len(r) for r in refs]}")
    assert 1 <= len(codes) <= n // 4
    assert sum(len(r) for r in refs if not isinstance(r, int)) >= 100
    multi = K.yolov3_multi(grids, classes, score_thr=thr)
    sizes = [MO.scale_boxes(h) for h in multi.scales]
    assert sum(sizes) == {"small": 252, "yolov3": 10647}[name]


def test_cap_case_is_saturated_and_recorded():
    multi = K.cap_multi()
    assert [MO.scale_boxes(h) for h in multi.scales] == [768, 3072, 12288]
    preds, rows = K.cap()
    assert [p.shape for p in preds] == [(1, 16, 16, 18), (1, 32, 32, 18), (1, 64, 64, 18)]
    assert len(rows) > 2000 and len(set(r[1:5] for r in rows)) == len(rows)
    with open(K.CAP_GOLDEN) as f:
        assert "post_multi_oracle" in json.load(f)["source"]
    # every box is a candidate: objectness 8 and a class logit near 12
    assert all((p[..., 4::6] == 8.0).all() and (p[..., 5::6] > 6.0).all() for p in preds)
    # every pair of boxes overlaps vertically: all are at least 512 pixels tall (a sample of the
    # decoded boxes, and the recorded rows)
    for r in rows:
        assert r[4] - r[2] >= 512
    h0 = multi.scales[0]
    for d in MO.decode_scale(preds[0][0], h0, "logistic")[::7]:
        assert d[0][3] - d[0][1] >= 512 and d[1] > np.float32(0.3)
