"""Host-only checks of the DFL head decode: DflHead's refusals and shapes, dnn_yolo_dfl_boxes / _workspace, and
the -2 of the entries with the field named, before anything is launched."""
import ctypes

import pytest

import dnn_hip
import yolo_post

lib = dnn_hip.mylib


def _dfl(scales=((80, 80, 8.0), (40, 40, 16.0), (20, 20, 32.0)), classes=80, reg_max=16, score_thr=0.25, n_scales=None):
    d = yolo_post.DflStruct(len(scales) if n_scales is None else n_scales, classes, reg_max, score_thr, 0.45)
    for k, s in enumerate(scales[:4]):
        d.scale[k] = yolo_post.DflScaleStruct(*s)
    return d


def test_dflhead_shapes_and_refusals():
    h = yolo_post.DflHead.for_input(640, 640)
    assert h.boxes == 8400 and h.scale_boxes == [6400, 1600, 400] and h.max_det == 8400
    assert h.pred_shapes == [(80, 80, 144), (40, 40, 144), (20, 20, 144)] and h.names is None
    assert h._entry("host") == ("dnn_yolo_postprocess_dfl_host", (1, 0))
    assert h._entry("device") == ("dnn_yolo_postprocess_dfl", (1, 0))
    assert h.workspace_bytes(2) == 2 * (8400 * 40 + 16384 * 8 + 64)
    m = yolo_post.DflHead([(3, 5, 16)], ("a", "b", "c"), reg_max=5, nms="per_class", labels="multi")
    assert m.pred_shapes == [(3, 5, 23)] and m.max_det == 45 and m.names == ("a", "b", "c")
    assert yolo_post.label_boxes([(1, 2, 3, 4, 5, 0.5)], m) == [("b", (2, 3), (4, 5), None)]
    for kw, word in ((dict(reg_max=1), "reg_max"), (dict(reg_max=17), "reg_max"), (dict(classes=129), "classes"),
                     (dict(nms="any", labels="multi"), 'needs nms "per_class"'), (dict(nms="x"), "nms"),
                     (dict(labels=1), "labels"), (dict(score_thr=-0.1), "score_thr"), (dict(strides=(8, 24)), "multiples"),
                     (dict(strides=(8, 16, 32, 64, 128)), "scales")):
        with pytest.raises(ValueError, match=word):
            yolo_post.DflHead.for_input(640, 640, **kw)
    for scales, word in (([], "scales"), ([(2, 2)], "stride"), ([(0, 2, 8)], "cells"), ([(2, 2, 0.0)], "stride"),
                         ([(256, 256, 8), (1, 1, 16)], "65537 points")):
        with pytest.raises(ValueError, match=word):
            yolo_post.DflHead(scales, 80)


def test_boxes_workspace_and_refusals_name_the_field():
    assert lib.dnn_yolo_dfl_boxes(ctypes.byref(_dfl())) == 8400
    assert lib.dnn_yolo_dfl_boxes(ctypes.byref(_dfl(((256, 256, 8.0),), reg_max=2, classes=128))) == 65536
    b = ctypes.c_ulonglong()
    assert lib.dnn_yolo_dfl_workspace(ctypes.byref(_dfl()), 3, ctypes.byref(b)) == 0
    assert b.value == 3 * (8400 * 40 + 16384 * 8 + 64)
    ptrs = (ctypes.c_void_p * 3)(16, 16, 16)  # never read: every call below is refused on the host
    for bad, word in ((_dfl(reg_max=1), "reg_max"), (_dfl(reg_max=17), "reg_max"), (_dfl(n_scales=0), "scales"),
                      (_dfl(n_scales=5), "scales"), (_dfl(classes=0), "n_classes"), (_dfl(classes=129), "n_classes"),
                      (_dfl(((80, 80, 0.0),)), "stride"), (_dfl(((80, 0, 8.0),)), "grid"),
                      (_dfl(score_thr=float("nan")), "score_thr"), (_dfl(((256, 256, 8.0), (1, 1, 16.0))), "65537 points")):
        assert lib.dnn_yolo_dfl_boxes(ctypes.byref(bad)) == -2
        assert word in dnn_hip.last_error(), (word, dnn_hip.last_error())
        assert lib.dnn_yolo_dfl_workspace(ctypes.byref(bad), 1, ctypes.byref(b)) == -2
        assert lib.dnn_yolo_postprocess_dfl(ctypes.byref(bad), ptrs, 1, 8, 4, 8, 8, 1 << 40, 1, 0, None) == -2
        assert lib.dnn_yolo_postprocess_dfl_host(ctypes.byref(bad), ptrs, 1, 8, 4, 8, 1, 0) == -2
    assert lib.dnn_yolo_dfl_boxes(None) == -2
    d, need = _dfl(), 8400 * 40 + 16384 * 8 + 64
    for nms, labels, word in ((0, 1, "labels_mode"), (2, 0, "nms_mode"), (1, 2, "labels_mode"), (-1, 0, "nms_mode")):
        assert lib.dnn_yolo_postprocess_dfl(ctypes.byref(d), ptrs, 1, 8, 4, 8, 8, need, nms, labels, None) == -2
        assert word in dnn_hip.last_error(), (word, dnn_hip.last_error())
        assert lib.dnn_yolo_postprocess_dfl_host(ctypes.byref(d), ptrs, 1, 8, 4, 8, nms, labels) == -2
    assert lib.dnn_yolo_postprocess_dfl(ctypes.byref(d), ptrs, 1, 8, 4, 8, 8, need - 1, 1, 1, None) == -2
    assert "workspace" in dnn_hip.last_error()
    assert lib.dnn_yolo_postprocess_dfl(ctypes.byref(d), ptrs, 1, 8, 4, 8, 12, need, 1, 1, None) == -2
    assert lib.dnn_yolo_postprocess_dfl(ctypes.byref(d), ptrs, 0, None, 4, None, None, 0, 1, 1, None) == 0  # no images
