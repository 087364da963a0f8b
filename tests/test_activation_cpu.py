"""CPU: the importer's side of mish / swish / logistic and the full YOLOv4 definition: what it accepts and
refuses, the cfg's sections, its lowering within the plan's four slots, and the weight file's size."""
import collections

import numpy as np
import pytest

import darknet_import as D
import dnn_hip
import v4tiny_cases as VK

NET = "[net]\nwidth=32\nheight=32\nchannels=3\n"
CONV = "[convolutional]\nbatch_normalize=1\nfilters=8\nsize=3\npad=1\nactivation={}\n"


def _lowering(secs, layers, size):
    g, _, _ = D.build_graph(dnn_hip.DnnGraphBuilder, secs, layers, [1, size, size, 3])
    entries = dnn_hip.lower_graph(g)
    return entries, dnn_hip.Plan.lowering(1, (size, size, 3), entries)


@pytest.mark.parametrize("act", ("mish", "swish", "logistic"))
def test_the_importer_accepts_the_activation_on_convs_and_shortcuts(act):
    text = NET + CONV.format(act) * 2 + f"[shortcut]\nfrom=-2\nactivation={act}\n"
    with pytest.raises(D.DarknetError, match=f"activation '{act}'"):
        D.parse_cfg(text)  # (on its own the parser lets through what every reader of its sections computes)
    secs = D.parse_cfg(text, D.ACTIVATIONS)
    assert D.conv_params(secs[1])[5] == act and D.layer_shapes(secs)[-1] == (32, 32, 8)
    text = _lowering(secs, VK.random_layers(secs), 32)[1]
    assert text.count(f"act={act}") == 3 and "activate" not in text, text  # two conv epilogues and the shortcut's


@pytest.mark.parametrize("section", (CONV.format("relu"), "[shortcut]\nfrom=-1\nactivation=elu\n"))
def test_the_importer_still_refuses_unknown_activations_by_name(section):
    with pytest.raises(D.DarknetError, match="activation '(relu|elu)'"):
        D.layer_shapes(D.parse_cfg(NET + CONV.format("mish") + section, D.ACTIVATIONS))


def test_full_yolov4_sections_weight_file_and_slots():
    secs = D.parse_cfg(D.cfg_text("yolov4", width=608, height=608), D.ACTIVATIONS)
    assert "yolov4" in D.MODELS and collections.Counter(s["type"] for s in secs[1:]) == {
        "convolutional": 110, "shortcut": 23, "route": 21, "maxpool": 3, "upsample": 2, "yolo": 3}
    assert collections.Counter(s.get("activation") for s in secs[1:]) == {
        "mish": 72, "leaky": 35, "linear": 3 + 23, None: 21 + 3 + 2 + 3}
    assert [(s["scale_x_y"], s["nms_kind"]) for s in secs if s["type"] == "yolo"] == [
        ("1.2", "greedynms"), ("1.1", "greedynms"), ("1.05", "greedynms")]
    shapes = D.weight_shapes(secs)
    # 64,363,101 parameters (biases, scales, weights); the file adds each BatchNorm's rolling mean and variance
    assert sum(n * ((2 if bn else 1) + c * size * size) for _, n, c, size, bn in shapes) == 64_363_101
    floats = sum(n * ((4 if bn else 1) + c * size * size) for _, n, c, size, bn in shapes)
    assert 20 + 4 * floats == 257_717_640  # yolov4.weights: the 20-byte header, then the floats
    # full width lowers within the plan's four slots, every mish a conv's epilogue (shapes only: zero weights)
    layers = [dict({"biases": np.zeros(n, np.float32), "weights": np.zeros((n, c, size, size), np.float32)},
                   **({k: np.ones(n, np.float32) for k in ("scales", "rolling_mean", "rolling_variance")} if bn else {}))
              for _, n, c, size, bn in shapes]
    entries, text = _lowering(secs, layers, 608)
    most, live = VK.replay_slots(entries)
    assert most == dnn_hip.MAX_SLOTS == 4 and not live
    assert text.count("act=mish") == 72 and "activate" not in text and text.count("\nspp ") == 1
