"""The two-piece fp16 form ("h2") of the wide x3 conv, host side only (no GPU): a numpy model of
the operand split (gemm_f32.h split2h) against its error bound, and which layers of a plan take
the form (dnn_plan_describe_pieces), leaving dnn_plan_describe's text, the kernel list and the plan's
memory as they were (recorded plans pin all three)."""
import numpy as np
import pytest

import dnn_hip
import synth
import yolo_graph


def split2h(a):
    """(g0, g1) of float32 `a` as the device forms them: g0 = rn16(a), g1 = rn16((a - g0) * 2048),
    both round-to-nearest-even; the residual and its scaling in float32 (exact)."""
    a = np.asarray(a, dtype=np.float32)
    g0 = a.astype(np.float16)
    r = (a - g0.astype(np.float32)) * np.float32(2048.0)
    return g0, r.astype(np.float16)


def _recon(a):
    g0, g1 = split2h(a)
    return g0.astype(np.float64) + g1.astype(np.float64) / 2048.0


def test_split2h_error_bound():
    """|g0 + g1 / 2048 - a| <= 2^-23 |a| for 2^-12 <= |a| < 65504, and <= 2^-36 below that (g0 a
    subnormal half or zero): random values per binade, the binade edges and their neighbours."""
    rng = np.random.default_rng(11)
    vals = []
    for e in range(-40, 16):  # |a| in [2^e, 2^(e+1)), up to 65504
        m = rng.uniform(1.0, 2.0, 4000)
        v = np.ldexp(m, e).astype(np.float32)
        edge = np.float32(2.0 ** e)
        vals += [v, np.array([edge, np.nextafter(edge, np.float32(0)), np.nextafter(edge, np.float32(np.inf))],
                             dtype=np.float32)]
    a = np.concatenate(vals)
    a = np.concatenate([a, -a, np.array([0.0, 65503.996, 2.0 ** -24, 2.0 ** -25, 1e-45], dtype=np.float32)])
    a = a[np.abs(a) < 65504]
    err = np.abs(_recon(a) - a.astype(np.float64))
    mag = np.abs(a.astype(np.float64))
    big = mag >= 2.0 ** -12
    assert big.sum() > 100000 and (~big).sum() > 100000
    assert np.all(err[big] <= 2.0 ** -23 * mag[big]), (err[big] / mag[big]).max()
    assert np.all(err[~big] <= 2.0 ** -36), err[~big].max()
    # the pieces of in-range values are finite; the top piece of anything from the fp16 rounding
    # threshold up is infinite (what h2_split_ok guards)
    g0, g1 = split2h(a)
    assert np.all(np.isfinite(g0)) and np.all(np.isfinite(g1))
    assert np.isinf(split2h(np.float32(65520.0))[0]) and np.isfinite(split2h(np.float32(65519.996))[0])


def _yolo_entries(batch):
    g, _ = yolo_graph.build_graph(dnn_hip.DnnGraphBuilder, synth.yolo_weights(), in_shape=(batch, 416, 416, 3))
    return dnn_hip.lower_graph(g)


def _h2(lines):
    """Indices of the conv layers on two fp16 pieces."""
    assert all(ln.startswith("conv%d pieces=" % i) for i, ln in enumerate(lines)), lines
    return [i for i, ln in enumerate(lines) if ln.endswith("pieces=h2")]


def test_yolo_batch_plan_takes_h2_on_conv6_conv7(monkeypatch):
    """The YOLOv2-tiny batch plan: conv6 (fed by conv5 + pool5's whole-image kernel) and conv7 (fed
    by conv6) on two fp16 pieces, conv1-conv5 and conv8 on three bf16 pieces, conv0 on neither;
    none with DNN_HIP_X3_H2=0, none in a latency plan; the choice does not depend on the batch.
    describe()'s text and memory() are the same with and without it: the planes of an h2 layer
    live in the first two thirds of the producer's 6-B-per-element region."""
    monkeypatch.delenv("DNN_HIP_X3_H2", raising=False)
    entries = _yolo_entries(64)
    pieces = dnn_hip.Plan.lowering_pieces(64, (416, 416, 3), entries)
    assert _h2(pieces) == [6, 7], pieces
    assert [ln.split("=")[1] for ln in pieces] == ["-"] + ["x3"] * 5 + ["h2"] * 2 + ["x3"]
    assert _h2(dnn_hip.Plan.lowering_pieces(1, (416, 416, 3), _yolo_entries(1))) == [6, 7]
    assert _h2(dnn_hip.Plan.lowering_pieces(1, (416, 416, 3), _yolo_entries(1), latency=True)) == []
    text, mem = dnn_hip.Plan.lowering(64, (416, 416, 3), entries), dnn_hip.Plan.memory(64, (416, 416, 3), entries)
    assert "pieces" not in text
    monkeypatch.setenv("DNN_HIP_X3_H2", "0")
    off = dnn_hip.Plan.lowering_pieces(64, (416, 416, 3), entries)
    assert _h2(off) == [] and [ln.split("=")[1] for ln in off] == ["-"] + ["x3"] * 8
    assert dnn_hip.Plan.lowering(64, (416, 416, 3), entries) == text
    assert dnn_hip.Plan.memory(64, (416, 416, 3), entries) == mem


def _chain(shape, convs, head=None):
    """pool (2x2 s1) -> 3x3 convs (C -> od each, bias + leaky) [-> 1x1 conv]: graph entries."""
    rng = np.random.default_rng(5)
    g = dnn_hip.DnnGraphBuilder()
    y = g.create_input(list(shape))
    y = g.create_max_pool2d(y, [1, 2, 2, 1], [1, 1, 1, 1], "SAME")
    c = shape[3]
    for od in convs:
        y = g.create_conv2d(y, (rng.standard_normal((3, 3, c, od)) * 0.05).astype(np.float32), [1, 1, 1, 1], "SAME")
        y = g.create_bias_add(y, np.zeros(od, np.float32))
        y = g.create_leaky_relu(y)
        c = od
    if head:
        y = g.create_conv2d(y, (rng.standard_normal((1, 1, c, head)) * 0.05).astype(np.float32), [1, 1, 1, 1], "SAME")
    g.set_out_node(y)
    return dnn_hip.lower_graph(g)


def test_h2_follows_the_layer_and_its_producer(monkeypatch):
    """A wide layer behind a separate pool stays on three bf16 pieces (the pool writes bf16 planes);
    behind the wide kernel it takes h2, as does the next one behind it, and the 1x1 head keeps its
    bf16 planes; an N = 512, K = 2304 layer (two K slices) and a layer with a fused pool do not."""
    monkeypatch.delenv("DNN_HIP_X3_H2", raising=False)
    shape = (2, 9, 11, 32)
    entries = _chain(shape, [256, 256, 256], head=200)
    assert _h2(dnn_hip.Plan.lowering_pieces(2, shape[1:], entries)) == [1, 2]
    assert "mode=x3_1x1" in dnn_hip.Plan.lowering(2, shape[1:], entries).splitlines()[-1]
    entries = _chain(shape, [256, 512])  # K = 2304, N = 512
    assert "splitK=2" in dnn_hip.Plan.lowering(2, shape[1:], entries).splitlines()[-1]
    assert _h2(dnn_hip.Plan.lowering_pieces(2, shape[1:], entries)) == []
    # conv -> conv + 2x2/s2 pool -> conv: the pooled form is not an h2 layer, and not a producer of its planes
    rng = np.random.default_rng(6)
    g = dnn_hip.DnnGraphBuilder()
    y = g.create_input([2, 26, 26, 32])
    y = g.create_max_pool2d(y, [1, 2, 2, 1], [1, 1, 1, 1], "SAME")
    for i in range(3):
        y = g.create_conv2d(y, (rng.standard_normal((3, 3, 32 if i == 0 else 256, 256)) * 0.05).astype(np.float32),
                            [1, 1, 1, 1], "SAME")
        y = g.create_bias_add(y, np.zeros(256, np.float32))
        y = g.create_leaky_relu(y)
        if i == 1:
            y = g.create_max_pool2d(y, [1, 2, 2, 1], [1, 2, 2, 1], "SAME")
    g.set_out_node(y)
    entries = dnn_hip.lower_graph(g)
    conv = [ln for ln in dnn_hip.Plan.lowering(2, (26, 26, 32), entries).splitlines() if ln.startswith("conv")]
    assert "+pool2x2s2" in conv[1] and all("mode=patch_x3" in ln for ln in conv), conv
    assert _h2(dnn_hip.Plan.lowering_pieces(2, (26, 26, 32), entries)) == []


def test_out_of_range_weights_keep_three_pieces(monkeypatch):
    """A layer whose weights do not all fit fp16's range (|w| < 65520, finite) stays on x3; its
    neighbours choose for themselves."""
    monkeypatch.delenv("DNN_HIP_X3_H2", raising=False)
    shape = (2, 9, 11, 32)
    for bad in (65520.0, -1e6, np.inf, np.nan):
        entries = _chain(shape, [256, 256, 256])
        convs = [e for e in entries if isinstance(e, dnn_hip.ConvEntry)]
        convs[1].conv.kernel[1, 1, 7, 9] = bad
        assert _h2(dnn_hip.Plan.lowering_pieces(2, shape[1:], entries)) == [2], bad
    entries = _chain(shape, [256, 256, 256])
    [e for e in entries if isinstance(e, dnn_hip.ConvEntry)][1].conv.kernel[1, 1, 7, 9] = 65519.0
    assert _h2(dnn_hip.Plan.lowering_pieces(2, shape[1:], entries)) == [1, 2]
