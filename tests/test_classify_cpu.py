"""Host side of the classifier import (no GPU): the five new cfg sections, their refusals, the connected
layer's place in a weight file, the classifier definitions and the plan entries they lower to."""
import numpy as np
import pytest

import darknet_cases as DC
import darknet_import as D
import dnn_hip

HEAD = "[net]\nwidth=8\nheight=8\nchannels=3\n[convolutional]\nfilters=6\nsize=3\nstride=2\npad=1\nactivation=leaky\n"
TAIL = HEAD + ("[avgpool]\n[dropout]\nprobability=.5\n[connected]\noutput=5\nbatch_normalize=1\nactivation=leaky\n"
               "[softmax]\ngroups=1\n[cost]\ntype=sse\n")


def test_new_sections_parse_and_shape():
    secs = D.parse_cfg(TAIL)
    assert [s["type"] for s in secs[1:]] == ["convolutional", "avgpool", "dropout", "connected", "softmax", "cost"]
    assert secs[-1]["type_"] == "sse"
    assert D.layer_shapes(secs) == [(4, 4, 6), (1, 1, 6), (1, 1, 6), (1, 1, 5), (1, 1, 5), (1, 1, 5)]
    assert D.conv_shapes(secs) == [(6, 3, 3, False)]
    assert D.weight_shapes(secs) == [("convolutional", 6, 3, 3, False), ("connected", 5, 6, 0, True)]


@pytest.mark.parametrize("tail, match", [
    ("[avgpool]\n[softmax]\ngroups=2\n", "groups = 2"),
    ("[avgpool]\n[softmax]\ntemperature=2\n", "temperature"),
    ("[avgpool]\n[softmax]\ntree=data/9k.tree\n", "tree"),
    ("[softmax]\n", "4 x 4"),
    ("[connected]\noutput=5\nactivation=linear\n", "4 x 4"),
    ("[avgpool]\n[connected]\noutput=5\nactivation=relu\n", "relu"),
    ("[avgpool]\n[connected]\nactivation=linear\n", "`output` is missing"),
    ("[shortcut]\nfrom=-1\nactivation=leaky\n", "leaky"),
    ("[reorg]\nstride=2\n", "reorg"),
])
def test_refusals(tail, match):
    with pytest.raises(D.DarknetError, match=match):
        D.layer_shapes(D.parse_cfg(HEAD + tail))


def test_dropout_counts_as_a_layer_for_route():
    cfg = HEAD + "[convolutional]\nfilters=4\nsize=1\nactivation=linear\n[dropout]\n[route]\nlayers=-2\n"
    secs = D.parse_cfg(cfg)
    assert D.layer_shapes(secs)[-1] == (4, 4, 4)  # -2 is the second conv: the dropout is layer 2 (else: 6 channels)
    g, outs, yolos = D.build_graph(dnn_hip.DnnGraphBuilder, secs, DC.darknet_layers(secs), [1, 8, 8, 3])
    assert yolos == [] and outs == [g.out_node] and g.out_node.result.shape == (1, 4, 4, 4)


def test_connected_weights_come_before_its_batchnorm_in_the_file(tmp_path):
    secs = D.parse_cfg(TAIL)
    fc = {"biases": np.full(5, 1, np.float32), "weights": np.arange(30, dtype=np.float32).reshape(5, 6) + 100,
          "scales": np.full(5, 2, np.float32), "rolling_mean": np.full(5, 3, np.float32),
          "rolling_variance": np.full(5, 4, np.float32)}
    layers = [DC.darknet_layers(secs)[0], fc]
    path = str(tmp_path / "fc.weights")
    D.save_weights(path, layers)
    back = D.load_weights(path, secs)
    assert all(np.array_equal(a[k], b[k]) for a, b in zip(layers, back) for k in a) and back[1]["weights"].shape == (5, 6)
    raw = np.fromfile(path, "<f4")[5 + 6 + 6 * 27:]  # after the header (20 bytes) and the conv
    assert raw.tolist() == [1] * 5 + list(range(100, 130)) + [2] * 5 + [3] * 5 + [4] * 5
    assert D.kernel_hwio(fc).shape == (1, 1, 6, 5) and D.kernel_hwio(fc)[0, 0, 2, 3] == fc["weights"][3, 2]
    with pytest.raises(D.DarknetError, match="connected layer 1"):
        D.check_layers(secs, [layers[0], dict(fc, weights=fc["weights"].T)])


@pytest.mark.parametrize("model, convs, size", [("darknet19", 19, 224), ("darknet53", 53, 256)])
def test_classifier_definitions_lower_to_one_plan(model, convs, size):
    assert model in D.MODELS
    full = D.parse_cfg(D.cfg_text(model))
    assert len(D.conv_shapes(full)) == convs and D.conv_shapes(full)[-1][0] == 1000
    assert D.net_shape(full) == (size, size, 3) and D.layer_shapes(full)[-1] == (1, 1, 1000)
    secs = D.parse_cfg(D.cfg_text(model, classes=10, width=64, height=64, width_div=8))
    g, outs, yolos = D.build_graph(dnn_hip.DnnGraphBuilder, secs, DC.darknet_layers(secs), [2, 64, 64, 3])
    assert yolos == [] and isinstance(g.out_node, dnn_hip.Softmax)
    entries = dnn_hip.lower_graph(g)
    kinds = [type(e).__name__ for e in entries if type(e).__name__ in ("AvgPoolEntry", "SoftmaxEntry")]
    assert kinds == ["AvgPoolEntry", "SoftmaxEntry"] and isinstance(entries[-1], dnn_hip.SoftmaxEntry)
    lines = dnn_hip.Plan.lowering(2, (64, 64, 3), entries).splitlines()
    assert sum(l.startswith("conv ") for l in lines) == convs
    pooled = "avgpool 2x2x10 -> 1x1x10" if model == "darknet19" else "avgpool 2x2x128 -> 1x1x128"
    assert pooled in lines and lines[-1] == "softmax 1x1x10"


def test_plan_entries_refuse_what_the_kernels_cannot_run():
    with pytest.raises(dnn_hip.DnnHipError, match="1x1xclasses"):
        dnn_hip.Plan.lowering(1, (2, 2, 10), [dnn_hip.SoftmaxEntry()])
    with pytest.raises(dnn_hip.DnnHipError, match="fp32 plans only"):
        dnn_hip.Plan.lowering(1, (2, 2, 16), [dnn_hip.AvgPoolEntry()], precision="fp16")
    assert dnn_hip.Plan.lowering(3, (7, 5, 12), [dnn_hip.AvgPoolEntry(), dnn_hip.SoftmaxEntry()]) == (
        "avgpool 7x5x12 -> 1x1x12\nsoftmax 1x1x12\n")
