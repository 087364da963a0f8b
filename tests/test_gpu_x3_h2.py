"""The wide x3 conv on two fp16 pieces per operand ("h2", gemm_x3_h2.h: three MFMA products per fp32
product) against the float64 oracle, on chains that cover its three producers (the whole-image
kernel, the wide x3 kernel, itself), its three outputs (fp32, h2 planes, the bf16 planes of a 1x1
head) and its range contract.

Bars.  A chain of n convs is held to n * LAYER_TOL normwise (test_gpu_parity holds one layer to
LAYER_TOL and a chain of two to 2 * LAYER_TOL: the layers' errors add, the He-scaled weights pass
them on with gain about 1), and to 1.25x the error of the same chain on the fp32 MFMA (DNN_HIP_X3=0),
the project's bar for the x3 arithmetic.  The DNN_HIP_X3_H2=0 arm (three bf16 pieces) meets the
same oracle bar, so the two arms are within twice that bar of each other."""
import functools

import numpy as np
import pytest

import dnn_hip
import ref_numpy as R

pytestmark = pytest.mark.gpu

LAYER_TOL = 2e-6  # (test_gpu_parity.LAYER_TOL)
S1 = ([1, 2, 2, 1], [1, 1, 1, 1], "SAME")  # the 2x2 / stride-1 SAME pool

# name: (input shape, [(od, pool after)...] 3x3 convs behind a leading 2x2/s1 pool, 1x1 head or
# None, the conv layers that must run on two fp16 pieces)
CASES = {
    # conv 64->256 + pool on the whole-image kernel -> h2 (fp32 out); 507 rows: two full tiles
    # that cross images and a partial one
    "a": ((3, 13, 13, 64), [(256, True), (256, False)], None, [1]),
    # ragged frame; wide x3 -> h2 (h2 planes out) -> h2 (bf16 planes out) -> 1x1 with a ragged N panel
    "b": ((2, 9, 11, 32), [(256, False), (256, False), (256, False)], 200, [1, 2]),
    # four N panels, then K = 9216
    "c": ((5, 13, 13, 128), [(256, False), (1024, False), (256, False)], None, [1, 2]),
}


@functools.lru_cache(maxsize=None)
def _case(name):
    """(x, layers) of a case: layers = [(kernel, bias, (mean, var, gamma)) ...], the 1x1 head last
    with bn None.  Arrays are shared between tests: nobody writes them."""
    shape, convs, head, _ = CASES[name]
    rng = np.random.default_rng(100 + ord(name))
    x = rng.standard_normal(shape).astype(np.float32)
    layers, c = [], shape[3]
    for od, _ in convs:
        k = (rng.standard_normal((3, 3, c, od)) * np.sqrt(2.0 / (9 * c))).astype(np.float32)
        b = rng.standard_normal(od).astype(np.float32) * np.float32(0.1)
        bn = (rng.standard_normal(od).astype(np.float32) * np.float32(0.1), rng.uniform(0.5, 1.5, od).astype(np.float32),
              rng.uniform(0.5, 1.5, od).astype(np.float32))
        layers.append((k, b, bn))
        c = od
    if head:
        k = (rng.standard_normal((1, 1, c, head)) * np.sqrt(1.0 / c)).astype(np.float32)
        layers.append((k, rng.standard_normal(head).astype(np.float32) * np.float32(0.1), None))
    return x, layers


def _graph(name, shape, layers):
    pools = [p for _, p in CASES[name][1]]
    g = dnn_hip.DnnGraphBuilder()
    y = g.create_input(list(shape))
    y = g.create_max_pool2d(y, *S1)
    for i, (k, b, bn) in enumerate(layers):
        y = g.create_conv2d(y, k, [1, 1, 1, 1], "SAME")
        y = g.create_bias_add(y, b)
        if bn is not None:
            y = g.create_batch_norm(y, *bn, 1e-5)
            y = g.create_leaky_relu(y)
            if pools[i]:
                y = g.create_max_pool2d(y, *S1)
    g.set_out_node(y)
    return g


def _oracle(name, x, layers, upto=None):
    """The chain in float64 accumulation (oracle/ref_numpy.py); `upto`: after that many layers."""
    pools = [p for _, p in CASES[name][1]]
    y = R.max_pool2d(x, *S1)
    for i, (k, b, bn) in enumerate(layers[:upto]):
        y = R.bias_add(R.conv2d(y, k), b)
        if bn is not None:
            y = R.leaky_relu(R.batch_norm(y, *bn, 1e-5))
            if pools[i]:
                y = R.max_pool2d(y, *S1)
    return y


@functools.lru_cache(maxsize=None)
def _ref(name):
    x, layers = _case(name)
    return _oracle(name, x, layers)


def _h2_layers(plan):
    """Indices of the plan's conv layers on two fp16 pieces (dnn_plan_describe_pieces)."""
    return [i for i, ln in enumerate(plan.pieces()) if ln.endswith("pieces=h2")]


def _check_chain(monkeypatch, name, x, layers, ref):
    """The chain's checks (module docstring); returns the h2 arm's output."""
    n = len(layers)
    monkeypatch.delenv("DNN_HIP_X3", raising=False)
    monkeypatch.delenv("DNN_HIP_X3_H2", raising=False)
    eng = dnn_hip.DnnInferenceEngine(_graph(name, x.shape, layers), False)
    desc = eng.plan().describe()
    assert _h2_layers(eng.plan()) == CASES[name][3], eng.plan().pieces()
    y = eng.run(x)
    assert eng.plan().range_events() == 0
    assert np.array_equal(eng.run(x), y)  # run to run
    y0 = dnn_hip.DnnInferenceEngine(_graph(name, (1,) + x.shape[1:], layers), False).run(x[:1])
    assert np.array_equal(y0, y[:1])  # a batch-1 plan: row 0 bit for bit
    err = R.normwise_err(y, ref)
    monkeypatch.setenv("DNN_HIP_X3_H2", "0")
    e3 = dnn_hip.DnnInferenceEngine(_graph(name, x.shape, layers), False)
    assert _h2_layers(e3.plan()) == [] and desc == e3.plan().describe()
    y3 = e3.run(x)
    err3, d3 = R.normwise_err(y3, ref), R.normwise_err(y3, y)
    monkeypatch.delenv("DNN_HIP_X3_H2")
    monkeypatch.setenv("DNN_HIP_X3", "0")
    e32 = dnn_hip.DnnInferenceEngine(_graph(name, x.shape, layers), False)
    assert "patch_x3" not in e32.plan().describe()
    err32 = R.normwise_err(e32.run(x), ref)
    print("h2 case %s: normwise err h2 %.3e, three bf16 pieces %.3e, fp32 MFMA %.3e; h2 vs three pieces %.3e"
          % (name, err, err3, err32, d3))
    assert err < n * LAYER_TOL and err3 < n * LAYER_TOL and err32 < n * LAYER_TOL, (err, err3, err32)
    assert err <= 1.25 * err32, (err, err32)
    assert d3 < 2 * n * LAYER_TOL, d3
    return y


@pytest.mark.parametrize("name", sorted(CASES))
def test_h2_chain_vs_oracle(monkeypatch, name):
    x, layers = _case(name)
    _check_chain(monkeypatch, name, x, layers, _ref(name))


def _scaled(layers, s):
    """Case a with the producer's BatchNorm gamma scaled by `s` (a power of two: the values entering
    the h2 layer scale exactly) and the h2 layer's bias and BatchNorm mean scaled alike, so that its
    output scales too and the normwise error keeps its meaning at every magnitude."""
    (k1, b1, (m1, v1, g1)), (k2, b2, (m2, v2, g2)) = layers
    s = np.float32(s)
    return [(k1, b1, (m1, v1, g1 * s)), (k2, b2 * s, (m2 * s, v2, g2))]


@pytest.mark.parametrize("target", [2.0 ** -13, 2.0 ** 10])
def test_h2_magnitudes(monkeypatch, target):
    """Values entering the h2 layer with median magnitude about 2^-13 (most top pieces subnormal
    halves: what a subnormal flush in the MFMA would fail) and about 2^10: the same bars."""
    x, layers = _case("a")
    mid = _oracle("a", x, layers, upto=1)
    s = 2.0 ** np.round(np.log2(target / np.median(np.abs(mid))))
    sl = _scaled(layers, s)
    med = np.median(np.abs(_oracle("a", x, sl, upto=1)))
    assert target / 1.5 < med < target * 1.5, med
    _check_chain(monkeypatch, "a", x, sl, _oracle("a", x, sl))


def test_h2_range_contract(monkeypatch):
    """A producer bias that lifts one channel to about 1e5, past fp16's range: the producer writes
    infinite pieces and raises the plan's range word, the h2 layer's output is non-finite, and the
    word is cleared by reading it.  On three bf16 pieces (DNN_HIP_X3_H2=0) the same chain is finite,
    within the bar, and raises nothing."""
    x, layers = _case("a")
    (k1, b1, (m1, v1, g1)), l2 = layers
    b1 = b1.copy()
    b1[5] = np.float32(1e5) * np.sqrt(v1[5] + np.float32(1e-5)) / g1[5]
    big = [(k1, b1, (m1, v1, g1)), l2]
    mid = _oracle("a", x, big, upto=1)
    assert 9e4 < mid[..., 5].min() and mid[..., 5].max() < 1.1e5 and np.abs(np.delete(mid, 5, axis=3)).max() < 100
    monkeypatch.delenv("DNN_HIP_X3", raising=False)
    monkeypatch.delenv("DNN_HIP_X3_H2", raising=False)
    eng = dnn_hip.DnnInferenceEngine(_graph("a", x.shape, big), False)
    assert _h2_layers(eng.plan()) == [1]
    y = eng.run(x)
    assert eng.plan().range_events() > 0
    assert not np.isfinite(y).all()
    assert eng.plan().range_events() == 0  # read and cleared
    monkeypatch.setenv("DNN_HIP_X3_H2", "0")
    e3 = dnn_hip.DnnInferenceEngine(_graph("a", x.shape, big), False)
    y3 = e3.run(x)
    assert e3.plan().range_events() == 0
    assert np.isfinite(y3).all()
    assert R.normwise_err(y3, _oracle("a", x, big)) < 2 * LAYER_TOL
