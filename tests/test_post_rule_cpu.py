"""CPU: the host side of new_coords / DIoU NMS: with the neutral rule tests/post_rule_oracle.py is
post_xy_oracle; the importer's acceptance and refusals; MultiHead's validation; the four exports."""
import ctypes
import os

import pytest

import darknet_import as D
import dnn_hip
import post_rule_oracle as RO
import post_xy_cases as XK
import post_xy_oracle as XO
import v4tiny_cases as VK
import yolo_post
from conftest import PKG


@pytest.mark.parametrize("mode", XO.MODES)
@pytest.mark.parametrize("name", sorted(XK.HEADS))
def test_the_neutral_rule_is_the_xy_oracle(name, mode):
    multi, preds = XK.multi_of(name), XK.inputs(name)
    got = tuple(RO.detect_or_code([p[i] for p in preds], multi, XK.xy_of(name), mode) for i in range(XK.IMAGES))
    assert got == XK.refs(name, mode) and any(not isinstance(g, int) and g for g in got)


def _scaled():
    return D.cfg_text("yolov4", width=64, height=64, width_div=8, classes=3, scaled_head=True)


def _head(cfg, **kw):
    secs = D.parse_cfg(cfg, D.ACTIVATIONS)
    _, _, yolos = D.build_graph(dnn_hip.DnnGraphBuilder, secs, VK.random_layers(secs), [1, 64, 64, 3])
    return D.multi_head(yolos, 64, 64, **kw)


def test_the_scaled_head_imports_with_its_rule():
    for wide in (False, True):
        head = _head(_scaled(), wide=wide)
        assert type(head) is (yolo_post.WideHead if wide else yolo_post.MultiHead)
        assert (head.new_coords, head.nms_kind, head.beta_nms, head.scale_x_y) == (True, "diou", 0.6, (2.0, 2.0, 2.0))
        assert head._entry("device")[0].endswith("_rule") and "DIoU beta 0.6" in repr(head)
    assert _head(_scaled().replace("beta_nms=0.6", "beta_nms=0.8")).beta_nms == 0.8
    plain = _head(D.cfg_text("yolov4", width=64, height=64, width_div=8, classes=3).replace("beta_nms=0.6", "beta_nms=x"))
    assert plain.rule is None and plain._entry("device")[0].endswith("_xy")  # a greedy-NMS cfg: as before, beta_nms unread
    cfg = _scaled().replace("activation=logistic", "activation=linear", 1)  # Darknet would read raw values there
    with pytest.raises(D.DarknetError, match="new_coords = 1 after a .convolutional. with activation = linear"):
        D.layer_shapes(D.parse_cfg(cfg, D.ACTIVATIONS), [1, 64, 64, 3])


@pytest.mark.parametrize("changes", [(("new_coords=1", "new_coords=0"), ("nms_kind=diounms", "nms_kind=greedynms")),
                                     (("nms_kind=diounms", "nms_kind=greedynms"),), (("beta_nms=0.6", "beta_nms=0.7"),)])
def test_the_yolo_sections_must_agree(changes):
    cfg = _scaled()
    for old, new in changes:  # in the first [yolo] section only
        cfg = cfg.replace(old, new, 1)
    with pytest.raises(D.DarknetError, match="must agree"):
        _head(cfg)


def test_multi_head_validates_the_rule_and_the_libraries_export_the_entries():
    scales = XK.multi_of("two_scales").scales
    plain = yolo_post.MultiHead(scales, "logistic", "per_class", "multi")
    assert plain.rule is None and plain._entry("device")[0] == "dnn_yolo_postprocess_multi_labels"
    for kw, word in ((dict(nms="any", nms_kind="diou"), "per_class"), (dict(class_mode="softmax", new_coords=True), "logistic"),
                     (dict(nms="per_class", nms_kind="diou", beta_nms=0.0), "beta_nms"), (dict(nms_kind="giou"), "nms_kind")):
        with pytest.raises(ValueError, match=word):
            yolo_post.MultiHead(scales, **kw)
    iou = yolo_post.WideHead(scales, "logistic", "any", new_coords=True)  # new_coords alone: any NMS rule
    assert (iou.rule.new_coords, iou.rule.nms_kind) == (1, 0) and iou._entry("host")[0] == "dnn_yolo_postprocess_wide_rule_host"
    for lib in ("libdnn_hip.so", "libdnn_hip_avx.so"):
        so = ctypes.CDLL(os.path.join(PKG, lib))
        assert all(hasattr(so, f"dnn_yolo_postprocess_{k}_rule{f}") for k in ("multi", "wide") for f in ("", "_host"))
