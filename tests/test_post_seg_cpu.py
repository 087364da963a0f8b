"""Host-only checks of the instance masks (dnn_yolo_seg, csrc/postprocess_seg.hip): the entries are declared,
dnn_yolo_seg_mask_words / dnn_yolo_dfl_seg_workspace, every argument error with its field named before any
device call, DflHead(mask_dim=None) unchanged, and the oracle's crop rule on hand-computed cases."""
import ctypes
import os

import numpy as np
import pytest

import dnn_hip
import post_seg_oracle as SO
import yolo_post

lib = dnn_hip.mylib
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dnn_hip_post.h")
DFL_WS = 8400 * 40 + 16384 * 8 + 64  # dnn_yolo_dfl_workspace of one 640 x 640 image


def _seg(n_coef=32, mask=(160, 160), net=(640, 640), max_masks=100):
    return yolo_post.SegStruct(n_coef, mask[0], mask[1], net[0], net[1], max_masks)


def test_entries_are_declared():
    text = open(HEADER).read()
    for name in ("dnn_yolo_seg_mask_words", "dnn_yolo_dfl_seg_workspace", "dnn_yolo_postprocess_dfl_seg",
                 "dnn_yolo_postprocess_dfl_seg_host"):
        assert f"int {name}(" in text and hasattr(lib, name), name
    assert "typedef struct dnn_yolo_seg {" in text and ctypes.sizeof(yolo_post.SegStruct) == 24


def test_mask_words_and_workspace():
    head = yolo_post.DflHead.for_input(640, 640, mask_dim=32)
    assert lib.dnn_yolo_seg_mask_words(ctypes.byref(_seg())) == 160 * 5
    assert lib.dnn_yolo_seg_mask_words(ctypes.byref(_seg(mask=(5, 33)))) == 5 * 2
    assert lib.dnn_yolo_seg_mask_words(ctypes.byref(_seg(mask=(1024, 1024)))) == 1024 * 32
    b = ctypes.c_ulonglong()
    assert lib.dnn_yolo_dfl_seg_workspace(ctypes.byref(head.c), ctypes.byref(_seg()), 3, 300, ctypes.byref(b)) == 0
    # the decode's, then points [3][300], coefficient rows [3][100][32] and rectangles [3][100], 16-byte aligned
    assert 3 * DFL_WS % 16 == 0 and b.value == 3 * DFL_WS + 3 * 300 * 4 + 3 * 100 * 32 * 4 + 3 * 100 * 16
    spec = head.seg((160, 160), (640, 640), max_masks=100)
    assert spec.workspace_bytes(head, 3, 300) == b.value and spec.w32 == 5 and spec.proto_shape == (160, 160, 32)
    assert head.coef_shapes == [(80, 80, 32), (40, 40, 32), (20, 20, 32)]
    assert lib.dnn_yolo_dfl_seg_workspace(ctypes.byref(head.c), ctypes.byref(_seg()), 1, 99, ctypes.byref(b)) != 0
    assert "max_masks" in dnn_hip.last_error()


@pytest.mark.parametrize("kw, word", [
    (dict(seg=_seg(n_coef=24)), "n_coef"), (dict(seg=_seg(n_coef=80)), "n_coef"),
    (dict(seg=_seg(mask=(0, 160))), "mask_h"), (dict(seg=_seg(mask=(160, 1025))), "mask_w"),
    (dict(seg=_seg(net=(0, 640))), "net_h"), (dict(seg=_seg(net=(640, -1))), "net_w"),
    (dict(seg=_seg(max_masks=0)), "max_masks"), (dict(seg=_seg(max_masks=301)), "max_masks"),
    (dict(coef=None), "coef"), (dict(coef=(32, 0, 32)), "coef[1]"), (dict(coef=(32, 32, 40)), "coef[2]"),
    (dict(proto=0), "proto"), (dict(proto=24), "proto"), (dict(masks=0), "masks"),
    (dict(ws=0), "workspace"), (dict(ws=24), "workspace"), (dict(ws_bytes=-1), "workspace"),
    (dict(nms=0, labels=1), "labels_mode"), (dict(reg_max=17), "reg_max"),
])
def test_argument_errors_name_the_field(kw, word):
    """Refused on the host: the pointers (small integers) are never read, and no device is needed."""
    head = yolo_post.DflHead.for_input(640, 640, mask_dim=32)
    dfl, seg = yolo_post.DflStruct.from_buffer_copy(head.c), kw.get("seg", _seg())
    dfl.reg_max = kw.get("reg_max", 16)
    pred = (ctypes.c_void_p * 3)(32, 32, 32)
    coef = None if "coef" in kw and kw["coef"] is None else (ctypes.c_void_p * 3)(*kw.get("coef", (32, 32, 32)))
    need = ctypes.c_ulonglong()
    assert lib.dnn_yolo_dfl_seg_workspace(ctypes.byref(head.c), ctypes.byref(_seg()), 1, 300, ctypes.byref(need)) == 0
    modes = (kw.get("nms", 1), kw.get("labels", 0))
    rc = lib.dnn_yolo_postprocess_dfl_seg(ctypes.byref(dfl), ctypes.byref(seg), pred, coef, kw.get("proto", 32), 1, 32,
                                          300, 32, kw.get("masks", 32), kw.get("ws", 32),
                                          need.value + kw.get("ws_bytes", 0), *modes, None)
    assert rc != 0 and word in dnn_hip.last_error(), (rc, dnn_hip.last_error())
    if not {"ws", "ws_bytes"} & set(kw) and kw.get("proto") != 24 and kw.get("coef") != (32, 32, 40):
        rc = lib.dnn_yolo_postprocess_dfl_seg_host(ctypes.byref(dfl), ctypes.byref(seg), pred, coef,
                                                   kw.get("proto", 32), 1, 32, 300, 32, kw.get("masks", 32), *modes)
        assert rc != 0 and word in dnn_hip.last_error(), (rc, dnn_hip.last_error())


def test_head_without_masks_is_unchanged_and_python_refusals():
    h = yolo_post.DflHead.for_input(640, 640)
    assert h.mask_dim is None and not hasattr(h, "coef_shapes")
    assert repr(h) == ("DflHead(80x80/8, 40x40/16, 20x20/32; 80 classes, reg_max 16, score > 0.25, IoU > 0.45, "
                       "NMS per_class, labels argmax)")
    assert h._entry("device") == ("dnn_yolo_postprocess_dfl", (1, 0)) and h.workspace_bytes(1) == DFL_WS
    with pytest.raises(ValueError, match="mask_dim"):
        h.seg((160, 160), (640, 640))
    with pytest.raises(ValueError, match="mask_dim"):
        yolo_post.DflHead.for_input(640, 640, mask_dim=20)
    m = yolo_post.DflHead.for_input(640, 640, mask_dim=32)
    assert repr(m).endswith("labels argmax, mask_dim 32)")
    for args, word in ((((0, 160), (640, 640)), "mask_h"), (((160, 2000), (640, 640)), "mask_w"),
                       (((160, 160), (640, 0)), "net_w"), (((160, 160), (640, 640), 0), "max_masks")):
        with pytest.raises(ValueError, match=word):
            m.seg(*args)


@pytest.mark.parametrize("corners, mask_hw, net_hw, xs, ys", [
    ((0, 0, 32, 32), (8, 8), (32, 32), range(0, 8), range(0, 8)),       # the whole frame
    ((24, -5, 40, 8), (8, 8), (32, 32), range(6, 8), range(0, 2)),      # over the right and top edges: clamped
    ((8, 8, 8, 24), (8, 8), (32, 32), range(0), range(2, 6)),           # left == right: empty
    ((40, 4, 50, 12), (8, 8), (32, 32), range(0), range(1, 3)),         # wholly outside
    ((-9, -9, -1, -1), (8, 8), (32, 32), range(0), range(0)),
    # net_w = 30 is no multiple of mask_w = 8: x * 30 >= 56 from x = 2, x * 30 < 160 up to x = 5
    ((7, 3, 20, 30), (5, 8), (30, 30), range(2, 6), range(1, 5)),       # y * 30 >= 15 from 1, y * 30 < 150 up to 4
    ((1, 1, 2, 2), (5, 33), (32, 32), range(2, 3), range(0)),           # 33 <= 32 x < 66: x = 2; 5 <= 32 y < 10: none
])
def test_oracle_crop_rule(corners, mask_hw, net_hw, xs, ys):
    want = np.zeros(mask_hw, bool)
    if len(xs) and len(ys):
        want[ys.start:ys.stop, xs.start:xs.stop] = True
    assert np.array_equal(SO.crop(corners, mask_hw, net_hw), want)
