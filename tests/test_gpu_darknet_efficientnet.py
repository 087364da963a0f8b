"""GPU: a narrow EfficientNet-B0 (cfg_text's construction at a quarter of the widths, 64 x 64, batch 2) from seeded
weights through a .weights file and DarknetModel, against the float64 Darknet forward (tests/darknet_se_oracle.py)."""
import numpy as np
import pytest

import darknet_import as D
import darknet_se_oracle as SE

pytestmark = pytest.mark.gpu

NET_TOL = 1e-4  # normwise, end to end: the suite's bar for imported models (tests/test_gpu_darknet.py)


def test_narrow_efficientnet_b0_matches_the_float64_forward_and_its_top5(tmp_path):
    cfg = D.cfg_text("efficientnet_b0", classes=10, width=64, height=64, width_div=4)
    secs = D.parse_cfg(cfg, D.ACTIVATIONS, D.SECTION_TYPES)
    path = str(tmp_path / "b0.weights")
    layers = SE.seeded_layers(D.weight_shapes(secs), seed=21)
    layers[-1]["weights"] *= np.float32(0.1)  # logits of a few units: a softmax that is not saturated, a top 5 with gaps
    D.save_weights(path, layers)
    x = np.random.default_rng(22).uniform(0, 1, (2, 64, 64, 3)).astype(np.float32)
    want = SE.forward(secs, D.load_weights(path, secs), x)
    assert want.shape == (2, 1, 1, 10)
    p = want.reshape(2, 10).astype(np.float64)
    order = np.argsort(-p, kind="stable", axis=1)
    ranked = np.take_along_axis(p, order, 1)
    assert (ranked[:, :5] - ranked[:, 1:6] > NET_TOL * p.max()).all(), ranked  # the fixture: a top 5 that the bar decides
    m = D.DarknetModel(cfg, path, in_shape=[2, 64, 64, 3])
    got = m.inference(x)
    text = m.sess.plan().describe()
    assert text.count("squeeze_excite ") == 16 and "activate" not in text and "k5x5" in text
    err = np.abs(got.astype(np.float64) - want).max() / np.abs(want).max()
    print("narrow efficientnet_b0: normwise err", err)
    assert got.shape == want.shape and err <= NET_TOL
    index, prob = m.classify(x, k=5)
    assert index.tolist() == order[:, :5].tolist()
    assert np.array_equal(prob, np.take_along_axis(got.reshape(2, 10), index, 1))
