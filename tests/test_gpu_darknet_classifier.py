"""Imported Darknet classifiers on the GPU: narrow Darknet-19 and Darknet-53 and a net that ends in a
[connected] layer, from seeded weights through save_weights -> DarknetModel, against the float64 Darknet
forward (tests/darknet_oracle.py's convs, pools and sums; the three new layers restated here)."""
import numpy as np
import pytest

import darknet_cases as DC
import darknet_import as D
import darknet_oracle as DO

pytestmark = pytest.mark.gpu

NET_TOL = 1e-4  # normwise, end to end: the suite's bar for imported models (tests/test_gpu_darknet.py)
f8 = np.float64
FC_CFG = """[net]
width=24
height=24
channels=3
[convolutional]
batch_normalize=1
filters=16
size=3
stride=2
pad=1
activation=leaky
[avgpool]
[dropout]
probability=.5
[connected]
output=10
batch_normalize=1
activation=leaky
[softmax]
groups=1
"""
CFGS = {"darknet19": lambda: D.cfg_text("darknet19", classes=10, width=64, height=64, width_div=8),
        "darknet53": lambda: D.cfg_text("darknet53", classes=10, width=64, height=64, width_div=8),
        "connected": lambda: FC_CFG}


def layers_for(secs):
    """darknet_cases' conv weights, and seeded [outputs][inputs] weights where a [connected] stands."""
    convs = iter(DC.darknet_layers(secs))
    rng = np.random.default_rng(5)
    out = []
    for kind, n, c, _, _ in D.weight_shapes(secs):
        if kind == "convolutional":
            out.append(next(convs))
        else:
            out.append({"biases": rng.standard_normal(n).astype(np.float32),
                        "weights": rng.standard_normal((n, c)).astype(np.float32),
                        "scales": rng.uniform(0.5, 1.5, n).astype(np.float32) * np.float32(-1) ** np.arange(n),
                        "rolling_mean": rng.standard_normal(n).astype(np.float32),
                        "rolling_variance": rng.uniform(0.5, 1.5, n).astype(np.float32)})
    return out


def oracle(secs, layers, x):
    """The Darknet forward in float64 per layer, every layer's output rounded once to fp32."""
    outs, weights = [], iter(layers)
    cur = np.asarray(x, np.float32)
    for at, sec in enumerate(secs[1:]):
        kind = sec["type"]
        if kind == "convolutional":
            cur = DO.conv_layer(cur, sec, next(weights))
        elif kind == "maxpool":
            cur = DO.maxpool_layer(cur, sec)
        elif kind == "shortcut":
            cur = (cur.astype(f8) + outs[at + int(sec["from"])].astype(f8)).astype(np.float32)
        elif kind == "avgpool":
            cur = cur.astype(f8).mean((1, 2), keepdims=True).astype(np.float32)
        elif kind == "connected":  # biases, then weights [outputs][inputs]: y[o] = sum_i w[o][i] x[i]
            layer = next(weights)
            v = np.einsum("nhwi,oi->nhwo", cur.astype(f8), np.asarray(layer["weights"], f8))
            cur = DO.affine_leaky(v, *DO.fold(layer), sec["activation"] == "leaky")
        elif kind == "softmax":
            e = np.exp(cur.astype(f8) - cur.astype(f8).max(3, keepdims=True))
            cur = (e / e.sum(3, keepdims=True)).astype(np.float32)
        else:
            assert kind in ("dropout", "cost"), kind
        outs.append(cur)
    return cur


@pytest.mark.parametrize("name", sorted(CFGS))
def test_classifier_matches_the_float64_forward_and_its_top3(name, tmp_path):
    cfg = CFGS[name]()
    secs = D.parse_cfg(cfg)
    path = str(tmp_path / "net.weights")
    D.save_weights(path, layers_for(secs))
    h, w, c = D.net_shape(secs)
    x = np.random.default_rng(11).uniform(0, 1, (2, h, w, c)).astype(np.float32)
    want = oracle(secs, D.load_weights(path, secs), x)
    assert want.shape == (2, 1, 1, 10)
    p = want.reshape(2, 10).astype(f8)
    order = np.argsort(-p, kind="stable", axis=1)
    ranked = np.take_along_axis(p, order, 1)
    tol = NET_TOL * np.abs(want).max()
    assert (ranked[:, 2] - ranked[:, 3] > tol).all() and (ranked[:, :2] - ranked[:, 1:3] > tol).all(), ranked
    m = D.DarknetModel(cfg, path, in_shape=[2, h, w, c])
    assert m.head is None
    got = m.inference(x)
    err = np.abs(got.astype(f8) - want).max() / np.abs(want).max()
    print(name, "normwise err", err)
    assert got.shape == want.shape and err < NET_TOL
    index, prob = m.classify(x, k=3)
    assert index.tolist() == order[:, :3].tolist()
    assert np.array_equal(prob, np.take_along_axis(got.reshape(2, 10), index, 1))
    with pytest.raises(ValueError, match="no \\[yolo\\]"):
        m.detect(x)
