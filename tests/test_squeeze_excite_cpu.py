"""CPU: the importer's squeeze-and-excitation pattern ([avgpool], two 1x1 convs, [scale_channels] -> one SqueezeExcite
node), its refusals, cfg_text("efficientnet_b0") and the node-by-node numpy forward."""
import numpy as np
import pytest

import darknet_import as D
import dnn_hip
import se_oracle as SO

HEAD = "[net]\nwidth=6\nheight=5\nchannels=3\n[convolutional]\nfilters=8\nsize=3\nstride=1\npad=1\nactivation=linear\n"
FC1 = "[convolutional]\nfilters=2\nsize=1\nstride=1\nactivation=swish\n"
FC2 = "[convolutional]\nbatch_normalize=1\nfilters=8\nsize=1\nstride=1\nactivation=logistic\n"
SE = "[avgpool]\n" + FC1 + FC2 + "[scale_channels]\nfrom=-4\nactivation=linear\n"


def _sections(text):
    return D.parse_cfg(text, D.ACTIVATIONS, D.SECTION_TYPES)


def test_the_four_sections_become_one_node_with_the_files_weights(tmp_path):
    secs = _sections(HEAD + SE + "[shortcut]\nfrom=-5\nactivation=linear\n")
    assert D.layer_shapes(secs) == [(5, 6, 8), (1, 1, 8), (1, 1, 2), (1, 1, 8), (5, 6, 8), (5, 6, 8)]
    # a hand-made file: header (0.2.0, 8-byte seen), then per conv biases[, scales, mean, variance], weights
    stem, fc1w, fc2w = np.arange(8 * 27, dtype="<f4") / 64, np.arange(16, dtype="<f4") + 100, np.arange(16, dtype="<f4") + 200
    one, zero = np.ones(8, "<f4"), np.zeros(8, "<f4")
    blob = [np.array([0, 2, 0], "<i4"), np.array([0], "<i8"), zero, stem, np.array([7, 9], "<f4"), fc1w,
            zero + 3, 2 * one, zero, one, fc2w]
    path = tmp_path / "se.weights"
    path.write_bytes(b"".join(a.tobytes() for a in blob))
    g, outs, _ = D.build_graph(dnn_hip.DnnGraphBuilder, secs, D.load_weights(str(path), secs), [1, 5, 6, 3])
    kinds = [type(e).__name__ for e in dnn_hip.lower_graph(g)]
    assert kinds == ["PaddedConvEntry", "StashEntry", "SqueezeExciteEntry", "ShortcutEntry", "ReleaseEntry"]
    node = [n for n in g.G.nodes if isinstance(n, dnn_hip.SqueezeExcite)]
    assert len(node) == 1 and (node[0].act1, node[0].act2) == ("swish", "logistic")
    # Darknet's [n][c][1][1] as [c][n]; the BatchNorm's scale 2 / (sqrt(1) + 1e-6) folded into the second matrix
    assert np.array_equal(node[0].w1, fc1w.reshape(2, 8).T) and node[0].b1.tolist() == [7, 9]
    assert np.allclose(node[0].w2, fc2w.reshape(8, 2).T * (2 / (1 + 1e-6)), rtol=2e-7, atol=0)
    assert np.allclose(node[0].b2, 3)


REFUSED = {
    "scale_wh": HEAD + SE.replace("from=-4", "from=-4\nscale_wh=1"),
    "activation": HEAD + SE.replace("activation=linear", "activation=swish"),
    "from elsewhere": HEAD + HEAD.split("\n", 4)[4] + SE.replace("from=-4", "from=-5"),
    "one conv": HEAD + "[avgpool]\n" + FC2 + "[scale_channels]\nfrom=-3\nactivation=linear\n",
    "three convs": HEAD + "[avgpool]\n" + FC1 + FC1 + FC2 + "[scale_channels]\nfrom=-5\nactivation=linear\n",
    "a 3x3 conv": HEAD + SE.replace("filters=2\nsize=1", "filters=2\nsize=3\npad=1"),
    "sam": HEAD + "[sam]\nfrom=-1\n",
    "inner layer read": HEAD + SE + "[route]\nlayers=-2\n",
}


@pytest.mark.parametrize("what", list(REFUSED))
def test_other_forms_are_refused_with_the_line(what):
    with pytest.raises(D.DarknetError, match="line \\d+"):
        secs = _sections(REFUSED[what])
        layers = [{"biases": np.zeros(n, np.float32), "weights": np.zeros((n, c, s, s), np.float32),
                   **({k: np.ones(n, np.float32) for k in ("scales", "rolling_mean", "rolling_variance")} if bn else {})}
                  for _, n, c, s, bn in D.weight_shapes(secs)]
        D.build_graph(dnn_hip.DnnGraphBuilder, secs, layers, [1, 5, 6, 3])


def test_efficientnet_b0_parses_and_lowers_within_the_slots():
    secs = _sections(D.cfg_text("efficientnet_b0"))
    assert D.net_shape(secs) == (224, 224, 3) and D.layer_shapes(secs)[-1] == (1, 1, 1000)
    shapes = D.weight_shapes(secs)
    # the paper's count: conv weights, a scale and a bias per BatchNorm channel, a bias elsewhere
    assert sum(n * c * s * s + (2 * n if bn else n) for _, n, c, s, bn in shapes) == 5288548
    layers = [{"biases": np.zeros(n, np.float32), "weights": np.zeros((n, c, s, s), np.float32),
               **({k: np.ones(n, np.float32) for k in ("scales", "rolling_mean", "rolling_variance")} if bn else {})}
              for _, n, c, s, bn in shapes]
    g, _, yolos = D.build_graph(dnn_hip.DnnGraphBuilder, secs, layers, [1, 224, 224, 3])
    entries = dnn_hip.lower_graph(g)
    assert yolos == [] and sum(isinstance(e, dnn_hip.SqueezeExciteEntry) for e in entries) == 16
    live = most = 0
    for e in entries:
        live += isinstance(e, dnn_hip.StashEntry) - isinstance(e, dnn_hip.ReleaseEntry)
        most = max(most, live)
    assert 1 <= most <= dnn_hip.MAX_SLOTS
    text = dnn_hip.Plan.lowering(1, (224, 224, 3), entries)
    assert text.count("squeeze_excite ") == 16 and "activate" not in text
    assert "squeeze_excite 7x7x1152 cr=48 act=swish,logistic" in text


def test_the_debug_paths_numpy_forward_is_the_oracles():
    x, w1, b1, w2, b2 = SO.tensors("scalar_odd")
    g = dnn_hip.DnnGraphBuilder()
    t = g.create_squeeze_excite(g.create_input(list(x.shape)), w1, b1, "mish", w2, b2, "logistic")
    g.set_out_node(t)
    t.in_node.set_input(x)
    t.run()
    want = SO.forward64(x, w1, b1, "mish", w2, b2, "logistic")
    assert np.abs(t.result - want).max() <= 1e-5 * np.abs(want).max()
    with pytest.raises(ValueError):
        g.create_squeeze_excite(t, w1[:, :0], b1[:0], "swish", w2[:0], b2, "logistic")  # cr = 0
