"""CPU-only checks of the multi-scale postprocessing (any grid, anchors, classes):
  * tests/post_head_oracle.py equals oracle/post_numpy.py on every 13 x 13 fixture and the
    reference's own function on small grids embedded in a 13 x 13 tensor;
  * the seeded GPU cases stay inside the conditions that keep them from passing vacuously;
  * YoloHead, the front-end and the weight loader validate like the C side;
  * the C entries reject a bad head, or a short workspace, before any GPU call (this machine
    has none: a GPU call would fail with another code)."""
import ctypes

import numpy as np
import pytest

import dnn_hip
import post_head_cases as K
import post_head_oracle as O
import post_numpy as PN
import synth
import yolo_post


def test_head_oracle_equals_post_numpy_on_13x13_fixtures(post_golden):
    head = O.voc_head(13, 13)
    for name, (pred, gold) in post_golden.items():
        if isinstance(gold, dict):
            with pytest.raises(ZeroDivisionError):
                O.detect(pred, head)
            assert O.detect_or_code(pred, head) == -2
            continue
        assert O.detect(pred, head) == PN.detect(pred), name
    # a YoloHead is a head for the oracle too
    pred = post_golden["synthetic_dense0"][0]
    assert O.detect(pred, yolo_post.YoloHead(13)) == PN.detect(pred)


def test_head_oracle_equals_reference_on_embedded_small_grids():
    cases = K.ms_golden()
    assert sorted({tuple(g["grid"]) for _, g in cases.values()}) == [(1, 1), (2, 3), (7, 13), (10, 10)]
    n = 0
    for name, (pred, gold) in cases.items():
        gh, gw = gold["grid"]
        assert pred.shape == (gh, gw, 125)
        got = O.detect_or_code(pred, O.voc_head(gh, gw))
        if "raises" in gold:
            assert got == -2, name
            continue
        assert [[PN.CLASSES[r[0]], [r[1], r[2]], [r[3], r[4]]] for r in got] == gold["boxes"], name
        n += len(got)
    assert n > 400


@pytest.mark.parametrize("name", sorted(K.PARITY))
def test_parity_cases_are_not_vacuous(name):
    _, n, _ = K.PARITY[name]
    preds, refs = K.parity(name)
    assert len(preds) == n
    raised = sum(isinstance(r, int) for r in refs)
    assert raised <= n // 4, (name, raised)
    if name in K.MULTI_CELL:
        assert sum(len(r) for r in refs if not isinstance(r, int)) >= 100, name
    assert all(r == -2 for r in refs if isinstance(r, int))


def test_parity_cases_cover_a_zero_denominator_and_both_box_stores():
    assert any(isinstance(r, int) for r in K.parity("voc19")[1])
    small, large = K.device_head(K.PARITY["lds2048"][0]), K.device_head(K.PARITY["ws2050"][0])
    assert (small.boxes, large.boxes) == (2048, 2050)
    assert small.workspace_bytes(3) == 0 and large.workspace_bytes(3) == 3 * 2050 * 40


@pytest.mark.parametrize("name", ["voc19", "voc19_zero_den"])
def test_saturated_19x19_cases(name):
    _, _, raises = K.SATURATED[name]
    _, rows, cand = K.saturated(name)
    if raises:
        assert rows == -2
    else:
        assert cand == 1805 and 100 < len(rows) < 400


@pytest.mark.parametrize("n", K.DENSE)
def test_dense_cases_keep_every_candidate(n):
    """n rows with n distinct scores and no error code: what makes the kept list grow as fast as the
    keys are consumed."""
    pred, rows = K.dense(n)
    assert pred.shape == (1, n, 7)
    assert not isinstance(rows, int), rows
    assert len(rows) == n
    assert len({r[5] for r in rows}) == n


def test_yolo_head_properties_and_validation():
    h = yolo_post.YoloHead.for_input(608, 608)
    assert (h.grid_h, h.grid_w, h.boxes, h.pred_shape, h.n_out) == (19, 19, 1805, (19, 19, 125), 125)
    assert yolo_post.YoloHead.for_input(64, 96).pred_shape == (2, 3, 125)
    assert yolo_post.YoloHead(13).boxes == yolo_post.N_BOXES
    h = yolo_post.YoloHead((6, 4), anchors=(1, 2, 3, 4, 5, 6), classes=7, score_thr=0.5, iou_thr=0.45)
    assert (h.n_anchors, h.n_classes, h.names, h.pred_shape) == (3, 7, None, (6, 4, 36))
    assert (h.c.score_thr, h.c.iou_thr, h.c.cell) == (np.float32(0.5), 0.45, 32.0)
    assert yolo_post.YoloHead(40).boxes == 8000 and yolo_post.YoloHead((1, 1024), anchors=K.ANCHORS8).boxes == 8192
    for bad in (dict(grid=13, classes=0), dict(grid=13, classes=129), dict(grid=13, anchors=()),
                dict(grid=13, anchors=(1.0,) * 34), dict(grid=13, anchors=(1.0, 2.0, 3.0)),
                dict(grid=(1, 8193), anchors=(1.0, 1.0)), dict(grid=41), dict(grid=0), dict(grid=(3, -1)),
                dict(grid=2.5), dict(grid=13, score_thr=-0.1), dict(grid=13, score_thr=float("nan")),
                dict(grid=13, iou_thr=float("nan")), dict(grid=13, cell=0.0), dict(grid=13, cell=float("inf")),
                dict(grid=13, anchors=(1.0, float("nan")))):
        with pytest.raises(ValueError):
            yolo_post.YoloHead(**bad)
    for hw in ((600, 608), (608, 0), (16, 32), (416.5, 416)):
        with pytest.raises(ValueError):
            yolo_post.YoloHead.for_input(*hw)


def test_head_shape_errors_and_labels():
    h = yolo_post.YoloHead(19)
    with pytest.raises(ValueError):
        yolo_post.detect_batch(np.zeros((2, 13, 13, 125), np.float32), head=h)
    with pytest.raises(ValueError):
        yolo_post.postprocessing(np.zeros((2, 19, 19, 125), np.float32), head=h)
    rows = [(14, 1, 2, 3, 4, 0.5), (0, 5, 6, 7, 8, 0.4)]
    assert yolo_post.label_boxes(rows, h) == yolo_post.label_boxes(rows)  # the 20 VOC names: the reference's colours
    assert yolo_post.label_boxes(rows)[0] == ("person", (1, 2), (3, 4), yolo_post.COLORS[14])
    named = yolo_post.YoloHead(4, classes=tuple(f"c{i}" for i in range(15)))
    assert yolo_post.label_boxes(rows, named) == [("c14", (1, 2), (3, 4), None), ("c0", (5, 6), (7, 8), None)]
    assert yolo_post.label_boxes(rows, yolo_post.YoloHead(4, classes=15))[0] == (14, (1, 2), (3, 4), None)


def _call_head(head_struct, n_images=1, max_det=4, ws_bytes=None, lib=None):
    """dnn_yolo_postprocess_head with host buffers where device pointers belong: a call that
    passes validation would touch the GPU, which these tests must not reach."""
    lib = lib or dnn_hip.mylib
    buf = np.zeros(1 << 16, np.uint8)
    p = buf.ctypes.data
    return lib.dnn_yolo_postprocess_head(ctypes.byref(head_struct), p, n_images, p, max_det, p, p,
                                         len(buf) if ws_bytes is None else ws_bytes, None)


def _voc(gh=13, gw=13):
    c = yolo_post.HeadStruct()
    assert dnn_hip.mylib.dnn_yolo_head_voc(gh, gw, ctypes.byref(c)) == 0
    return c


def test_c_head_voc_and_boxes():
    c = _voc(19, 17)
    assert (c.grid_h, c.grid_w, c.n_anchors, c.n_classes) == (19, 17, 5, 20)
    assert (c.cell, c.score_thr, c.iou_thr) == (32.0, np.float32(0.3), 0.3)
    assert list(c.anchors)[:10] == [np.float32(a) for a in yolo_post.ANCHORS] and not any(list(c.anchors)[10:])
    assert dnn_hip.mylib.dnn_yolo_head_boxes(ctypes.byref(c)) == 19 * 17 * 5
    assert ctypes.sizeof(c) == 160
    assert dnn_hip.mylib.dnn_yolo_head_voc(41, 40, ctypes.byref(c)) < 0  # 8200 boxes
    assert dnn_hip.mylib.dnn_yolo_head_voc(13, 13, None) < 0
    assert dnn_hip.mylib.dnn_yolo_head_boxes(None) < 0
    b = ctypes.c_ulonglong(1)
    assert dnn_hip.mylib.dnn_yolo_head_workspace(ctypes.byref(_voc()), 64, ctypes.byref(b)) == 0 and b.value == 0
    assert dnn_hip.mylib.dnn_yolo_head_workspace(ctypes.byref(_voc(40, 40)), 2, ctypes.byref(b)) == 0
    assert b.value == 2 * 8000 * 40
    assert dnn_hip.mylib.dnn_yolo_head_workspace(ctypes.byref(_voc()), -1, ctypes.byref(b)) < 0


@pytest.mark.parametrize("what", ["classes0", "anchors17", "boxes8193", "score_thr<0", "score_thr nan", "cell0",
                                  "short workspace", "no workspace", "unaligned workspace", "n_images<0",
                                  "max_det<0"])
def test_c_entry_rejects_before_any_gpu_call(what):
    c, kw = _voc(), {}
    if what == "classes0":
        c.n_classes = 0
    elif what == "anchors17":
        c.n_anchors = 17
    elif what == "boxes8193":
        c.grid_h, c.grid_w, c.n_anchors = 1, 8193, 1
    elif what == "score_thr<0":
        c.score_thr = -0.25
    elif what == "score_thr nan":
        c.score_thr = float("nan")
    elif what == "cell0":
        c.cell = 0.0
    elif what == "short workspace":
        c, kw = _voc(40, 40), dict(n_images=1, ws_bytes=8000 * 40 - 1)
    elif what == "no workspace":
        c, kw = _voc(40, 40), dict(n_images=1, ws_bytes=0)
    elif what == "n_images<0":
        kw = dict(n_images=-1)
    elif what == "max_det<0":
        kw = dict(max_det=-1)
    for lib in (dnn_hip.mylib, dnn_hip.load_library("libdnn_hip_avx.so")):
        yolo_post._bind(lib)
        if what == "unaligned workspace":
            c = _voc(40, 40)
            buf = np.zeros(8000 * 40 + 16, np.uint8)
            p = buf.ctypes.data
            rc = lib.dnn_yolo_postprocess_head(ctypes.byref(c), p, 1, p, 4, p, p + (12 - p % 8), 8000 * 40, None)
        else:
            rc = _call_head(c, lib=lib, **kw)
        assert rc == -2, what
        assert "dnn_yolo_postprocess_head" in dnn_hip.last_error(lib)
    if what in ("classes0", "anchors17", "boxes8193", "score_thr<0", "score_thr nan", "cell0"):
        z = np.zeros(64, np.uint8).ctypes.data
        assert dnn_hip.mylib.dnn_yolo_postprocess_head_host(ctypes.byref(c), z, 1, z, 1, z) == -2
        assert dnn_hip.mylib.dnn_yolo_head_boxes(ctypes.byref(c)) == -2


def test_weights_validate_n_out():
    import yolo_weights as YW
    ws = synth.yolo_zero_weights(channels=synth.CHANNELS[:-1] + (36,))
    with pytest.raises(YW.WeightFileError):
        YW.validate(ws)
    assert YW.validate(ws, n_out=36)[-1]["kernel"].shape == (1, 1, 1024, 36)
    with pytest.raises(YW.WeightFileError):
        YW.validate(synth.yolo_zero_weights(), n_out=36)
    assert len(YW.validate(synth.yolo_zero_weights())) == 9


def test_front_end_rejects_input_that_is_no_multiple_of_32():
    import yolov2tiny
    for shape in ([1, 400, 416, 3], [1, 416, 100, 3], [416, 416, 3]):
        with pytest.raises(ValueError):
            yolov2tiny.YOLO_V2_TINY(shape, synth.yolo_zero_weights(), False)
    with pytest.raises(ValueError):  # a head whose width the weights do not have
        yolov2tiny.YOLO_V2_TINY([1, 64, 64, 3], synth.yolo_zero_weights(), False,
                                head=yolo_post.YoloHead(2, classes=3))
    with pytest.raises(ValueError):  # a width that is not 5 anchors x (5 + classes)
        yolov2tiny.YOLO_V2_TINY([1, 64, 64, 3], synth.yolo_zero_weights(channels=synth.CHANNELS[:-1] + (36,)), False)


def test_front_end_head_follows_in_shape_and_last_layer_width():
    import yolov2tiny
    assert yolov2tiny._head_for([1, 608, 416, 3], None).pred_shape == (19, 13, 125)
    h = yolov2tiny._head_for([1, 64, 96, 3], None, 425)
    assert (h.pred_shape, h.n_classes, h.names, h.anchors) == ((2, 3, 425), 80, None, yolo_post.ANCHORS)
    proto = yolo_post.YoloHead(7, anchors=(1, 2, 3, 4), classes=("a", "b", "c"), score_thr=0.5, iou_thr=0.45)
    h = yolov2tiny._head_for([1, 320, 64, 3], proto)
    assert (h.pred_shape, h.names, h.anchors, h.score_thr, h.iou_thr) == ((10, 2, 16), ("a", "b", "c"),
                                                                          (1.0, 2.0, 3.0, 4.0), 0.5, 0.45)
