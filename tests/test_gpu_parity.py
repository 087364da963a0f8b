"""GPU parity: the HIP path through its C-ABI vs the oracle (ref_numpy / dnn_oracle.c) and the
golden vectors of the reference's own engine.  Bars: bit-exact for bias_add / batch_norm /
leaky_relu / max_pool2d / im2col (pure fp32 element-wise or copy work); for convolutions
(fp32 MFMA, a different summation order than OpenBLAS) max|d| <= 1e-4 * max|ref| per tensor
(normwise), checked here at a tighter 2e-6 against the float64 oracle per
layer and 1e-4 on the 9-layer net."""
import ctypes
import os

import numpy as np
import pytest

import dnn_hip
import ref_numpy as R
import synth
import yolo_graph
from oracle_c import OracleC

pytestmark = pytest.mark.gpu

NET_TOL = 1e-4
LAYER_TOL = 2e-6


class _Fake(object):
    def __init__(self, arr):
        self.result = arr


@pytest.fixture(scope="module")
def oc():
    return OracleC()


@pytest.fixture(scope="module")
def avx():
    return dnn_hip.load_library("libdnn_hip_avx.so")


def _p(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


# ------------------------------------------------------------------ per-op ABI (libdnn_hip.so)
@pytest.mark.parametrize("name", ["c3_same", "c3_same_c3", "c3_valid", "c1_same", "c2_same", "c3_wide"])
def test_conv2d_mul_vs_golden(golden_ops, name):
    x, k = golden_ops[f"conv_{name}_x"], golden_ops[f"conv_{name}_k"]
    pad = str(golden_ops[f"conv_{name}_pad"])
    node = dnn_hip.Conv2D("c", _Fake(x), k, [1, 1, 1, 1], pad)
    node.run()
    assert R.normwise_err(node.result, golden_ops[f"conv_{name}_y"]) < 1e-5
    assert R.normwise_err(node.result, R.conv2d(x, k, padding=pad)) < LAYER_TOL


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_elementwise_abi_bit_exact(golden_ops, name):
    g = golden_ops
    n = dnn_hip.BiasAdd("b", _Fake(g[f"bias_{name}_x"]), g[f"bias_{name}_b"]); n.run()
    assert np.array_equal(n.result, g[f"bias_{name}_y"])
    n = dnn_hip.BatchNorm("bn", _Fake(g[f"bn_{name}_x"]), g[f"bn_{name}_mean"], g[f"bn_{name}_var"],
                          g[f"bn_{name}_gamma"], 1e-5)
    var_before = n.variance.copy()
    n.run()
    assert np.array_equal(n.result, g[f"bn_{name}_y"])
    assert np.array_equal(n.variance, var_before)  # never mutated (dnn_openblas.c:48-50 does)
    n.run()
    assert np.array_equal(n.result, g[f"bn_{name}_y"])  # stable across runs
    n = dnn_hip.LeakyReLU("l", _Fake(g[f"leaky_{name}_x"])); n.run()
    assert np.array_equal(n.result, g[f"leaky_{name}_y"])


@pytest.mark.parametrize("name", ["k2s2_even", "k2s2_odd", "k2s1_same", "k3s2_valid", "k3s2_same"])
def test_max_pool_abi_bit_exact(golden_ops, name):
    g = golden_ops
    k, s = g[f"pool_{name}_k"], g[f"pool_{name}_s"]
    n = dnn_hip.MaxPool2D("p", _Fake(g[f"pool_{name}_x"]), [1, int(k[0]), int(k[1]), 1],
                          [1, int(s[0]), int(s[1]), 1], str(g[f"pool_{name}_pad"]))
    n.run()
    assert np.array_equal(n.result, g[f"pool_{name}_y"])


def test_conv2d_mul_batched_and_strided(oc):
    """Batch > 1 is strided by ih*iw*ic (the reference strides by oh*ow*od, dnn_openblas.c:170)."""
    rng = np.random.default_rng(11)
    for (B, H, W, C, od, s) in [(3, 11, 9, 7, 12, 1), (2, 12, 10, 8, 20, 2)]:
        x = rng.standard_normal((B, H, W, C)).astype(np.float32)
        k = rng.standard_normal((3, 3, C, od)).astype(np.float32)
        node = dnn_hip.Conv2D("c", _Fake(x), k, [1, s, s, 1], "SAME")
        node.run()
        ref = R.conv2d(x, k, strides=[1, s, s, 1], padding="SAME")
        assert R.normwise_err(node.result, ref) < LAYER_TOL
        xp, oh, ow = R.pad_nhwc(x, 3, 3, s, s, "SAME")
        kr = np.ascontiguousarray(k.transpose(2, 0, 1, 3).reshape(-1, od))
        assert R.normwise_err(node.result, oc.conv2d_mul(xp, kr, oh, ow, 3, 3, s, s)) < LAYER_TOL


@pytest.mark.parametrize("shape", [(9, 8, 6, 4, 3, 3, 3, 2, 2), (18, 18, 3, 16, 16, 3, 3, 1, 1),
                                   (7, 7, 33, 7, 7, 1, 1, 1, 1), (10, 12, 5, 4, 5, 3, 2, 2, 2)])
def test_im2col_abi_bit_exact(oc, shape):
    """(ic, kh, kw) column order of dnn_openblas.c:135-158, gathered on the device."""
    ih, iw, ic, oh, ow, kh, kw, sh, sw = shape
    lib = dnn_hip.mylib
    rng = np.random.default_rng(4)
    xp = rng.standard_normal((1, ih, iw, ic)).astype(np.float32)
    col = np.zeros((oh * ow, ic * kh * kw), np.float32)
    lib.im2col(_p(xp), _p(col), oh, ow, ih, iw, ic, kh, kw, sh, sw)
    assert dnn_hip.last_error() == ""
    ref = np.empty_like(col)
    oc.lib.oracle_im2col(xp.ctypes.data, ref.ctypes.data, oh, ow, ih, iw, ic, kh, kw, sh, sw)
    assert np.array_equal(col, ref)


@pytest.mark.parametrize("name", ["c3_same", "c3_valid", "c1_same", "c2_same", "c3_wide"])
def test_conv2d_cublas_abi_vs_golden(golden_ops, name):
    """conv2d_cublas with the argument layout of proj3/dnn_cublas.py:176-191 (np.pad'ed input,
    col scratch [batch, oh*ow, ic*kh*kw], kernel_r = kernel.transpose(2,0,1,3) as [K, od],
    result shape, padded input shape, window, strides) vs the reference's conv golden."""
    x, k = golden_ops[f"conv_{name}_x"], golden_ops[f"conv_{name}_k"]
    pad = str(golden_ops[f"conv_{name}_pad"])
    kh, kw, ic, od = k.shape
    xp, oh, ow = R.pad_nhwc(x, kh, kw, 1, 1, pad)
    xp = np.ascontiguousarray(xp, dtype=np.float32)
    kr = np.ascontiguousarray(k.transpose(2, 0, 1, 3).reshape(-1, od))
    col = np.zeros((x.shape[0], oh * ow, ic * kh * kw), np.float32)
    out = np.zeros((x.shape[0], oh, ow, od), np.float32)
    dnn_hip.mylib.conv2d_cublas(_p(xp), _p(col), _p(kr), _p(out), *map(ctypes.c_int, out.shape),
                                *map(ctypes.c_int, xp.shape[1:]), ctypes.c_int(kh), ctypes.c_int(kw),
                                ctypes.c_int(1), ctypes.c_int(1))
    assert dnn_hip.last_error() == ""
    assert R.normwise_err(out, golden_ops[f"conv_{name}_y"]) < 1e-5
    assert R.normwise_err(out, R.conv2d(x, k, padding=pad)) < LAYER_TOL


def test_legacy_error_is_raised():
    x = np.zeros((1, 4, 4, 3), np.float32)
    node = dnn_hip.Conv2D("c", _Fake(x), np.zeros((3, 3, 3, 4), np.float32), [1, 1, 1, 1], "VALID")
    node.result = np.zeros((1, 5, 5, 4), np.float32)  # inconsistent with the padded input
    with pytest.raises(dnn_hip.DnnHipError):
        node.run()


# ------------------------------------------------------------------ AVX / CUDA ABI (libdnn_hip_avx.so)
def test_avx_abi(avx, oc):
    rng = np.random.default_rng(21)
    B, H, W, C, od = 2, 9, 8, 12, 20
    x = rng.standard_normal((B, H, W, C)).astype(np.float32)
    k = rng.standard_normal((3, 3, C, od)).astype(np.float32)
    xp, oh, ow = R.pad_nhwc(x, 3, 3, 1, 1, "SAME")
    xp = np.ascontiguousarray(xp)
    args = np.array([oh, ow, od, xp.shape[1], xp.shape[2], C, 3, 3, 1, 1], np.int32)
    out = np.zeros((B, oh, ow, od), np.float32)
    avx.conv2d_pthread(_p(xp), _p(k), _p(out), B, args.ctypes.data_as(ctypes.POINTER(ctypes.c_int)))
    assert dnn_hip.last_error(avx) == ""
    ref = R.conv2d(x, k, padding="SAME")
    assert R.normwise_err(out, ref) < LAYER_TOL
    kr = np.ascontiguousarray(k.transpose(2, 0, 1, 3).reshape(-1, od))
    out2 = np.zeros_like(out)
    # the col scratch (B * oh * ow rows of 3*3*C, the reference's im2col buffer) apart from the result
    col = np.full((B * oh * ow, 9 * C), np.nan, np.float32)
    avx.conv2d_cuda_pthread(_p(xp), _p(col), _p(kr), _p(out2), B, args.ctypes.data_as(ctypes.POINTER(ctypes.c_int)))
    assert R.normwise_err(out2, ref) < LAYER_TOL

    y = ref
    b = rng.standard_normal(od).astype(np.float32)
    r = np.zeros_like(y)
    avx.bias_add_pthread(_p(y), _p(b), _p(r), *y.shape)
    assert np.array_equal(r, oc.bias_add(y, b))
    alpha = rng.uniform(0.5, 1.5, od).astype(np.float32)
    beta = rng.uniform(-0.1, 0.1, od).astype(np.float32)
    for fn in (avx.batch_norm, avx.batch_norm_cuda):
        r = np.zeros_like(y)
        fn(_p(y), _p(alpha), _p(beta), _p(r), *y.shape)
        assert np.array_equal(r, oc.batch_norm_ab(y, alpha, beta))
    r = np.zeros_like(y)
    avx.leaky_relu(_p(y), _p(r), *y.shape)
    assert np.array_equal(r, R.leaky_relu_avx(y))

    # max pool, with signed zeros so `>` (vector channels) and `>=` (tail) differ
    z = rng.choice(np.array([0.0, -0.0, 1.0, -1.0], np.float32), size=(B, 8, 8, od)).astype(np.float32)
    zp = np.ascontiguousarray(z)
    pargs = np.array([4, 4, od, 8, 8, od, 2, 2, 2, 2], np.int32)
    r = np.zeros((B, 4, 4, od), np.float32)
    avx.max_pool2d_pthread(_p(zp), _p(r), B, pargs.ctypes.data_as(ctypes.POINTER(ctypes.c_int)))
    gt = od - od % 8
    ref = oc.max_pool2d(z, [1, 2, 2, 1], [1, 2, 2, 1], "VALID", gt_below=gt)
    assert np.array_equal(r.view(np.int32), ref.view(np.int32))
    r2 = np.zeros_like(r)
    avx.max_pool2d_avx(_p(zp), _p(r2), B, 4, 4, od, 8, 8, od, 2, 2, 2, 2)
    assert np.array_equal(r2.view(np.int32), ref.view(np.int32))
    r3 = np.zeros_like(r)
    dnn_hip.mylib.max_pool2d(_p(zp), _p(r3), B, 4, 4, od, 8, 8, od, 2, 2, 2, 2)
    assert np.array_equal(r3.view(np.int32), oc.max_pool2d(z, [1, 2, 2, 1], [1, 2, 2, 1], "VALID").view(np.int32))


# ------------------------------------------------------------------ fused plan, single layers
def _chain(x_shape, k, strides=(1, 1, 1, 1), pad="SAME", bias=None, bn=None, leaky=False, pool=None):
    g = dnn_hip.DnnGraphBuilder()
    y = g.create_input(list(x_shape))
    y = g.create_conv2d(y, k, list(strides), pad)
    if bias is not None:
        y = g.create_bias_add(y, bias)
    if bn is not None:
        y = g.create_batch_norm(y, *bn, 1e-5)
    if leaky:
        y = g.create_leaky_relu(y)
    if pool is not None:
        y = g.create_max_pool2d(y, [1, pool[0], pool[0], 1], [1, pool[1], pool[1], 1], pool[2])
    g.set_out_node(y)
    return g


def _oracle_chain(x, k, strides=(1, 1, 1, 1), pad="SAME", bias=None, bn=None, leaky=False, pool=None):
    y = R.conv2d(x, k, strides=strides, padding=pad)
    if bias is not None:
        y = R.bias_add(y, bias)
    if bn is not None:
        y = R.batch_norm(y, *bn, 1e-5)
    if leaky:
        y = R.leaky_relu(y)
    if pool is not None:
        y = R.max_pool2d(y, [1, pool[0], pool[0], 1], [1, pool[1], pool[1], 1], pool[2])
    return y


FUSED_CASES = [
    # B, H, W, C, kh, od, stride, pad, pool  -> exercises every GEMM config and edge
    (2, 40, 38, 3, 3, 16, 1, "SAME", (2, 2, "SAME")),     # cfg 256x16 (K=27 -> 32), conv0-like
    (1, 30, 26, 16, 3, 32, 1, "SAME", (2, 2, "SAME")),    # cfg 256x32 (K=144)
    (2, 17, 15, 32, 3, 64, 1, "SAME", None),              # cfg 128x64
    (8, 20, 20, 64, 3, 128, 1, "SAME", (2, 1, "SAME")),   # M=3200, 25 128-tiles -> cfg 64x128
    (64, 13, 13, 96, 3, 1024, 1, "SAME", None),           # M=10816, N=1024 -> cfg 128x128 (conv7-like)
    (64, 13, 13, 256, 3, 1024, 1, "SAME", (2, 1, "SAME")),  # K=2304 -> split-K 3 on the 128x512 tile + reduce, s1 pool
    (3, 13, 13, 64, 1, 125, 1, "SAME", None),             # 1x1 direct path, ragged N=125
    (4, 13, 13, 1024, 1, 125, 1, "SAME", None),           # conv8: 1x1, K=1024, N=125 (32x128 tiles)
    (2, 9, 11, 5, 3, 48, 2, "SAME", None),                # stride 2, K=45 not a multiple of BK
    (1, 10, 9, 8, 3, 24, 1, "VALID", None),               # VALID
]


@pytest.mark.parametrize("case", FUSED_CASES)
def test_fused_conv_bn_leaky_pool(case):
    B, H, W, C, kh, od, s, pad, pool = case
    rng = np.random.default_rng(B * 1000 + C * 10 + od)
    x = rng.standard_normal((B, H, W, C)).astype(np.float32)
    k = (rng.standard_normal((kh, kh, C, od)) * np.sqrt(2.0 / (kh * kh * C))).astype(np.float32)
    bias = rng.standard_normal(od).astype(np.float32) * 0.1
    bn = (rng.standard_normal(od).astype(np.float32) * 0.1, rng.uniform(0.5, 1.5, od).astype(np.float32),
          rng.uniform(0.5, 1.5, od).astype(np.float32))
    kw = dict(strides=(1, s, s, 1), pad=pad, bias=bias, bn=bn, leaky=True, pool=pool)
    g = _chain(x.shape, k, **kw)
    assert dnn_hip.lower_graph(g) is not None
    y = dnn_hip.DnnInferenceEngine(g, False).run(x)
    ref = _oracle_chain(x, k, **kw)
    assert y.shape == ref.shape
    assert R.normwise_err(y, ref) < LAYER_TOL
    # conv-only variant (no epilogue ops)
    g2 = _chain(x.shape, k, strides=(1, s, s, 1), pad=pad)
    y2 = dnn_hip.DnnInferenceEngine(g2, False).run(x)
    assert R.normwise_err(y2, R.conv2d(x, k, strides=(1, s, s, 1), padding=pad)) < LAYER_TOL


IMPLICIT_CASES = [
    # B, H, W, C, od, pool   (C == 16 or C % 32 == 0 -> implicit GEMM; pool 2x2/s2 fused)
    (2, 26, 22, 16, 32, True),     # conv1-like, MFMA 16x16x4 family
    (3, 20, 18, 32, 64, True),     # conv2-like
    (2, 13, 13, 32, 64, True),     # odd 13x13 -> 7x7: SAME pool padding inside the fused epilogue
    (4, 16, 16, 64, 128, True),    # conv3-like
    (2, 13, 11, 128, 256, False),  # conv5-like, no pool
    (1, 9, 9, 16, 125, False),     # ragged N
    (64, 26, 26, 128, 256, True),  # conv4 at batch 64: K = 1152 -> 128x128 tile with the fused pool
]


@pytest.mark.parametrize("case", IMPLICIT_CASES)
def test_implicit_gemm_and_fused_pool_vs_explicit_bit_exact(monkeypatch, case):
    """The implicit GEMM gathers the same A operand the im2col writes and uses the same MFMA
    family and K permutation, so fused and explicit paths must agree bit for bit; both are
    checked against the oracle too."""
    B, H, W, C, od, pool = case
    rng = np.random.default_rng(C + od + H)
    x = rng.standard_normal((B, H, W, C)).astype(np.float32)
    k = (rng.standard_normal((3, 3, C, od)) * np.sqrt(2.0 / (9 * C))).astype(np.float32)
    bias = rng.standard_normal(od).astype(np.float32) * 0.1
    bn = (rng.standard_normal(od).astype(np.float32) * 0.1, rng.uniform(0.5, 1.5, od).astype(np.float32),
          rng.uniform(0.5, 1.5, od).astype(np.float32))
    kw = dict(bias=bias, bn=bn, leaky=True, pool=(2, 2, "SAME") if pool else None)
    outs = {}
    for fuse in ("1", "0"):
        monkeypatch.setenv("DNN_HIP_FUSE", fuse)
        eng = dnn_hip.DnnInferenceEngine(_chain(x.shape, k, **kw), False)
        outs[fuse] = eng.run(x)
        desc = eng.plan().describe()
        assert ("implicit" in desc or "patch" in desc) == (fuse == "1")
        assert ("+pool2x2s2" in desc) == (fuse == "1" and pool)
    assert np.array_equal(outs["1"], outs["0"])
    assert R.normwise_err(outs["1"], _oracle_chain(x, k, **kw)) < LAYER_TOL


@pytest.mark.parametrize("fuse", ["1", "0"])
def test_empty_batch(monkeypatch, fuse):
    """A batch of 0 frames runs (no launches) and returns an empty [0, oh, ow, od] array, as the
    reference's numpy engines do."""
    monkeypatch.setenv("DNN_HIP_FUSE", fuse)
    rng = np.random.default_rng(5)
    k = rng.standard_normal((3, 3, 16, 32)).astype(np.float32)
    x = np.zeros((0, 12, 10, 16), dtype=np.float32)
    bn = (np.zeros(32, np.float32), np.ones(32, np.float32), np.ones(32, np.float32))
    eng = dnn_hip.DnnInferenceEngine(_chain(x.shape, k, bias=np.zeros(32, np.float32), bn=bn, leaky=True,
                                            pool=(2, 2, "SAME")), False)
    out = eng.run(x)
    assert out.shape == (0, 6, 5, 32) and out.dtype == np.float32


PATCH_CASES = [
    # B, H, W, C, epilogue   (3x3 SAME, 32 outputs, 2x2/s2 pool -> patch kernel)
    (2, 26, 22, 16, "bn"),        # partial 16x16 tiles on both edges
    (1, 208, 208, 16, "bn"),      # YOLOv2-tiny conv1 at batch 1
    (3, 34, 18, 32, "bn"),        # C = 32 (two 16-channel groups per tap)
    (2, 16, 16, 16, "bn_neg"),    # negative gamma: min-pool before the epilogue
    (2, 18, 20, 16, "bias"),      # bias + leaky only
    (1, 12, 14, 16, "none"),      # bare conv + pool
]


@pytest.mark.parametrize("case", PATCH_CASES)
def test_patch_conv_pool_bit_exact(monkeypatch, case):
    """The patch kernel issues the implicit GEMM's exact MFMA sequence per accumulator and
    pools before the (monotone) epilogue: patch == implicit == explicit im2col+GEMM+pool, bit
    for bit (value equality), and within tolerance of the oracle."""
    B, H, W, C, ep = case
    od = 32
    rng = np.random.default_rng(H * W + C)
    x = rng.standard_normal((B, H, W, C)).astype(np.float32)
    k = (rng.standard_normal((3, 3, C, od)) * np.sqrt(2.0 / (9 * C))).astype(np.float32)
    bias = rng.standard_normal(od).astype(np.float32) * 0.1
    gamma = rng.uniform(0.5, 1.5, od).astype(np.float32)
    if ep == "bn_neg":
        gamma[::3] *= -1
    bn = (rng.standard_normal(od).astype(np.float32) * 0.1, rng.uniform(0.5, 1.5, od).astype(np.float32), gamma)
    kw = dict(pool=(2, 2, "SAME"))
    if ep in ("bn", "bn_neg"):
        kw.update(bias=bias, bn=bn, leaky=True)
    elif ep == "bias":
        kw.update(bias=bias, leaky=True)
    outs = {}
    for fuse, patch, mode in (("1", "1", "patch"), ("1", "0", "implicit"), ("0", "1", "gemm")):
        monkeypatch.setenv("DNN_HIP_FUSE", fuse)
        monkeypatch.setenv("DNN_HIP_PATCH", patch)
        eng = dnn_hip.DnnInferenceEngine(_chain(x.shape, k, **kw), False)
        outs[mode] = eng.run(x)
        assert f"mode={mode} " in eng.plan().describe()
    assert np.array_equal(outs["patch"], outs["implicit"])
    assert np.array_equal(outs["patch"], outs["gemm"])
    assert R.normwise_err(outs["patch"], _oracle_chain(x, k, **kw)) < LAYER_TOL


@pytest.mark.parametrize("hw", [(40, 38), (13, 13), (17, 22), (40, 36), (18, 52), (33, 20)])
def test_direct_conv0_pool_vs_oracle(monkeypatch, hw):
    """conv0's direct kernel (3 input channels, pool fused) vs the oracle and vs the explicit path;
    where W % 4 == 0 (16-B patch-row DMAs, D16) also equal bit for bit to the 4-B row DMAs
    (DNN_HIP_C0_D16=0): tiles past the right / bottom edge, frames narrower than two tiles."""
    H, W = hw
    rng = np.random.default_rng(H * W)
    x = rng.uniform(0, 1, (3, H, W, 3)).astype(np.float32)
    k = (rng.standard_normal((3, 3, 3, 16)) * 0.3).astype(np.float32)
    bias = rng.standard_normal(16).astype(np.float32) * 0.1
    bn = (rng.standard_normal(16).astype(np.float32) * 0.1, rng.uniform(0.5, 1.5, 16).astype(np.float32),
          rng.uniform(0.5, 1.5, 16).astype(np.float32))
    kw = dict(bias=bias, bn=bn, leaky=True, pool=(2, 2, "SAME"))
    eng = dnn_hip.DnnInferenceEngine(_chain(x.shape, k, **kw), False)
    y = eng.run(x)
    assert "mode=direct " in eng.plan().describe()
    ref = _oracle_chain(x, k, **kw)
    assert y.shape == ref.shape
    assert R.normwise_err(y, ref) < LAYER_TOL
    assert np.array_equal(eng.run(x), y)
    if W % 4 == 0:
        monkeypatch.setenv("DNN_HIP_C0_D16", "0")  # read when the plan is created: an engine of its own
        assert np.array_equal(dnn_hip.DnnInferenceEngine(_chain(x.shape, k, **kw), False).run(x), y)
        monkeypatch.delenv("DNN_HIP_C0_D16")
    monkeypatch.setenv("DNN_HIP_FUSE", "0")
    y0 = dnn_hip.DnnInferenceEngine(_chain(x.shape, k, **kw), False).run(x)
    assert R.normwise_err(y, y0) < LAYER_TOL


def test_fused_epilogue_is_reference_order():
    """With an exactly representable conv (integer data, small K) the fused epilogue must equal
    bias_add -> batch_norm -> leaky_relu applied separately, bit for bit."""
    rng = np.random.default_rng(8)
    x = rng.integers(-3, 4, size=(2, 12, 12, 8)).astype(np.float32)
    k = rng.integers(-2, 3, size=(3, 3, 8, 40)).astype(np.float32)
    bias = rng.standard_normal(40).astype(np.float32)
    bn = (rng.standard_normal(40).astype(np.float32), rng.uniform(0.5, 1.5, 40).astype(np.float32),
          rng.uniform(0.5, 1.5, 40).astype(np.float32))
    g = _chain(x.shape, k, bias=bias, bn=bn, leaky=True)
    y = dnn_hip.DnnInferenceEngine(g, False).run(x)
    assert np.array_equal(y, _oracle_chain(x, k, bias=bias, bn=bn, leaky=True))


# ------------------------------------------------------------------ whole YOLOv2-tiny net
@pytest.fixture(scope="module")
def yolo_b1(yolo_weights):
    g, _ = yolo_graph.build_graph(dnn_hip.DnnGraphBuilder, yolo_weights, in_shape=(1, 416, 416, 3))
    return dnn_hip.DnnInferenceEngine(g, False)


@pytest.mark.parametrize("frame", [0, 1, 2, 3])
def test_yolo_batch1_vs_reference_golden(yolo_b1, golden_frames, frame):
    y = yolo_b1.run(synth.frame(frame))
    assert y.shape == (1, 13, 13, 125)
    err = R.normwise_err(y, golden_frames[frame])
    assert err < NET_TOL, err


def test_yolo_repeat_runs_identical(yolo_b1):
    a = yolo_b1.run(synth.frame(0)).copy()
    b = yolo_b1.run(synth.frame(0))
    assert np.array_equal(a, b)  # no cross-run state (the reference drifts)


def test_yolo_node_by_node_debug_path(yolo_weights, golden_frames, tmp_path, monkeypatch):
    """debug=True runs the reference's per-node traversal through the per-op ABI and dumps
    every layer like proj3/dnn_openblas.py:47-50."""
    import os
    monkeypatch.chdir(tmp_path)
    g, nodes = yolo_graph.build_graph(dnn_hip.DnnGraphBuilder, yolo_weights, in_shape=(1, 416, 416, 3))
    y = dnn_hip.DnnInferenceEngine(g, True).run(synth.frame(0))
    assert R.normwise_err(y, golden_frames[0]) < NET_TOL
    files = sorted(os.listdir(tmp_path / "intermediate"))
    assert len(files) == 40 and "layer_1.npy" in files and "layer_40.npy" in files
    from conftest import GOLDEN
    st = np.load(os.path.join(GOLDEN, "nodes_frame0.npz"))
    for k, n in enumerate(nodes):
        r = np.asarray(n.result)
        idx = np.linspace(0, r.size - 1, 64).astype(np.int64)
        assert R.normwise_err(r.reshape(-1)[idx], st[f"sample_{k}"]) < NET_TOL, k


def test_yolo_batch64_golden_indices_and_batch_invariance(yolo_weights, golden_frames, yolo_b1):
    """Batch 64 with the 4 golden frames at 0/17/42/63: each row must match
    its golden, and every row must equal the batch-1 run of the same frame bit for bit
    (images are independent and the k-order of the MFMA reduction does not depend on M)."""
    slots = {0: 0, 17: 1, 42: 2, 63: 3}
    idx = [slots.get(i, 100 + i) for i in range(64)]
    x = synth.frames(idx)
    g, _ = yolo_graph.build_graph(dnn_hip.DnnGraphBuilder, yolo_weights, in_shape=(64, 416, 416, 3))
    eng = dnn_hip.DnnInferenceEngine(g, False)
    y = eng.run(x)
    assert y.shape == (64, 13, 13, 125)
    for pos, f in slots.items():
        assert R.normwise_err(y[pos], golden_frames[f][0]) < NET_TOL
    for pos in (0, 5, 17, 42, 63):
        assert np.array_equal(y[pos:pos + 1], yolo_b1.run(x[pos:pos + 1]))
    # ragged n < batch and n == 0 through the same plan
    plan = eng.plan()
    y5 = plan.run_host(x[:5])
    assert np.array_equal(y5, y[:5])
    # ... and on five OTHER frames: rows 0-4 of every activation now differ from what the
    # 64-frame run left there, rows 5-63 are stale; nothing stale may reach the output
    x5 = synth.frames([300, 301, 302, 303, 304])
    z5 = plan.run_host(x5)
    for i in range(5):
        assert np.array_equal(z5[i:i + 1], yolo_b1.run(x5[i:i + 1])), i
    assert not np.array_equal(z5, y5)
    assert plan.run_host(x[:0]).shape == (0, 13, 13, 125)


def test_clock_stamps_and_plan_clock_api(yolo_b1):
    """dnn_clock_stamp (csrc/clock.hip) and the plan's clock stamps around one kernel
    (dnn_plan_clock_begin / end): per-XCD shader clocks in a plausible range, stamps monotone,
    every XCD sampled by one workgroup per CU, stamping stopped after the requested runs, the
    forward's output unchanged by the stamp launches, and the API's error returns."""
    import torch
    plan = yolo_b1.plan()
    x = synth.frame(1)
    y0 = plan.run_host(x)
    dev = torch.device("cuda", 0)
    nwg = 256
    s = torch.cuda.Stream(dev)
    buf = torch.zeros((2, nwg, 4), dtype=torch.int64, device=dev)
    dnn_hip.clock_stamp(buf[0].data_ptr(), nwg, s.cuda_stream)
    t = torch.empty((1 << 24,), device=dev)
    with torch.cuda.stream(s):
        for _ in range(20):
            t.mul_(1.0001)
    dnn_hip.clock_stamp(buf[1].data_ptr(), nwg, s.cuda_stream)
    s.synchronize()
    a, b = buf[0].cpu().numpy(), buf[1].cpu().numpy()
    # s_memrealtime is one 100 MHz clock; s_memtime counts per XCD (workgroup w of the two launches
    # may sit on different XCDs), so the clock is taken per XCD, from the medians
    assert np.all(b[:, 1] > a[:, 1])
    for xcd in set(a[:, 2].tolist()) & set(b[:, 2].tolist()):
        assert np.median(b[b[:, 2] == xcd, 0]) > np.median(a[a[:, 2] == xcd, 0])
    c = dnn_hip.sclk_from_stamps(a, b)
    # (a region with idle gaps averages a low clock: s_memtime counts shader cycles, which slow
    # down while the GPU idles -- measured ~0.1 GHz over this mostly idle region)
    assert c is not None and 0.0 < c["min"] <= c["mean"] <= c["max"] < 3.0, c
    assert len(c["per_xcd"]) >= 1 and all(0 <= int(k) < 16 for k in c["per_xcd"])
    runs = 3
    kb = torch.zeros((runs + 2, 2, nwg, 4), dtype=torch.int64, device=dev)
    plan.clock_begin("conv7.gemm", kb.data_ptr(), runs, nwg)
    for _ in range(runs + 2):  # more runs than slots: stamping stops at `runs`
        y = plan.run_host(x)
    assert plan.clock_end() == runs
    assert np.array_equal(y, y0)
    k = kb.cpu().numpy()
    for i in range(runs):
        ci = dnn_hip.sclk_from_stamps(k[i, 0], k[i, 1])
        assert ci is not None and 0.3 < ci["mean"] < 3.0, ci
    assert not k[runs:].any()
    with pytest.raises(dnn_hip.DnnHipError):
        plan.clock_end()  # not active
    with pytest.raises(dnn_hip.DnnHipError):
        dnn_hip.clock_stamp(kb.data_ptr(), 0, s.cuda_stream)


def test_plan_timing_api(yolo_b1):
    plan = yolo_b1.plan()
    x = synth.frame(1)
    plan.timing_begin(3)
    for _ in range(3):
        plan.run_host(x)
    ms, cnt = plan.timing_end()
    ks = plan.kernels()
    # 9 plan kernels: conv0-8 (conv4's pool and pool5 fused: conv5 on whole-image tiles)
    assert len(ms) == len(ks) == 9
    assert all(c == 3 for c in cnt)
    assert all(m > 0 for m in ms)
    # events around one kernel only (the bench's timed region): the others report no launches
    for only in ("conv7.gemm", "conv8.gemm", "conv0.direct"):
        plan.timing_begin(3, only=only)
        for _ in range(3):
            plan.run_host(x)
        ms1, cnt1 = plan.timing_end()
        names = [k["name"] for k in ks]
        assert [c for n, c in zip(names, cnt1) if n != only] == [0] * 8
        assert cnt1[names.index(only)] == 3 and ms1[names.index(only)] > 0


# ------------------------------------------------------------------ on-GPU postprocessing
def test_postprocess_gpu_vs_reference_golden(post_golden):
    """dnn_yolo_postprocess == the reference's postprocessing() on every fixture case
    (yolov2tiny.py:94-234), one batched launch."""
    import yolo_post
    names = list(post_golden)
    preds = np.stack([post_golden[n][0] for n in names])
    rows = yolo_post.detect_batch(preds, raise_errors=False)
    for name, r in zip(names, rows):
        if isinstance(post_golden[name][1], dict):  # the reference raises ZeroDivisionError
            assert r == -2, name
            continue
        got = [[b[0], list(b[1]), list(b[2])] for b in yolo_post.label_boxes(r)]
        assert got == post_golden[name][1], name
    # the single-image drop-in returns the reference's tuples, colors included
    lb = yolo_post.postprocessing(post_golden["net_frame0"][0].reshape(1, 13, 13, 125))
    assert [list(t[:1]) + [list(t[1]), list(t[2])] for t in lb] == post_golden["net_frame0"][1]
    assert all(t[3] == yolo_post.COLORS[yolo_post.CLASSES.index(t[0])] for t in lb)


def test_postprocess_gpu_vs_oracle_random_batch():
    """64 seeded synthetic images in one launch vs oracle/post_numpy.py: identical boxes,
    classes and order; scores equal up to the last bits of exp/pow."""
    import post_numpy as PN
    import yolo_post
    rng = np.random.default_rng(77)
    preds = np.stack([PN.synthetic_predictions(rng, tw_scale=(1.0 if i % 4 else 6.0)) for i in range(64)])
    rows = yolo_post.detect_batch(preds, raise_errors=False)
    n_total = n_err = 0
    for p, r in zip(preds, rows):
        try:
            ref = PN.detect(p)
        except ZeroDivisionError:  # the reference raises on this image: so must we
            assert r == -2
            n_err += 1
            continue
        assert [x[:5] for x in r] == [x[:5] for x in ref]
        np.testing.assert_allclose([x[5] for x in r], [x[5] for x in ref], rtol=1e-6)
        n_total += len(r)
    assert n_total > 1000 and n_err < 16


def test_postprocess_gpu_error_cases():
    """Non-finite corners raise like the reference's int(); empty input and no detections."""
    import yolo_post
    p = np.zeros((2, 13, 13, 125), np.float32)
    p.reshape(2, 845, 25)[1, 17, 2] = 100.0  # exp(100) = inf in fp32 -> int(inf) raises in the reference
    with pytest.raises(dnn_hip.DnnHipError):
        yolo_post.detect_batch(p)
    assert yolo_post.detect_batch(p[:1]) == [[]]  # all-zero logits: score 0.5 * 0.05 < 0.3
    assert yolo_post.detect_batch(np.zeros((0, 13, 13, 125), np.float32)) == []


def test_postprocess_device_buffers_match_host_api(post_golden):
    import torch
    import yolo_post
    names = list(post_golden)
    preds = np.stack([post_golden[n][0] for n in names])
    dev = torch.device("cuda", 0)
    buf = yolo_post.DetectionBuffers(len(names), dev)
    t = torch.from_numpy(preds).to(dev)
    buf.run(t.data_ptr(), len(names), torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    rows = yolo_post.DetectionBuffers.to_rows(buf.dets.cpu().numpy(), buf.counts.cpu().numpy(), raise_errors=False)
    assert rows == yolo_post.detect_batch(preds, raise_errors=False)
    # device-side packing + the (single-rank) detection gather round-trip
    import dist as D
    packed, total, counts = buf.pack(len(names), torch.cuda.current_stream(dev).cuda_stream)
    d, c = D.gather_detections(packed, total, counts, len(names))
    assert D.unpack_detections(d, c) == rows
    assert len(d) == sum(len(r) for r in rows if not isinstance(r, int))


def test_plan_graph_replay_matches_eager(yolo_b1):
    """dnn_plan_run_graph (captured HIP graph) == dnn_plan_run, re-captures on new buffers."""
    import torch
    plan = yolo_b1.plan()
    dev = torch.device("cuda", 0)
    s = torch.cuda.Stream(dev)
    x = torch.from_numpy(synth.frame(2)).to(dev)
    y_e = torch.empty((1, 13, 13, 125), device=dev)
    y_g = torch.empty_like(y_e)
    plan.run_device(1, x.data_ptr(), y_e.data_ptr(), s.cuda_stream)
    for _ in range(3):
        plan.run_graph(1, x.data_ptr(), y_g.data_ptr(), s.cuda_stream)
    s.synchronize()
    assert torch.equal(y_e, y_g)
    x2 = torch.from_numpy(synth.frame(3)).to(dev)
    y2 = torch.empty_like(y_e)
    plan.run_graph(1, x2.data_ptr(), y2.data_ptr(), s.cuda_stream)
    plan.run_device(1, x2.data_ptr(), y_e.data_ptr(), s.cuda_stream)
    s.synchronize()
    assert torch.equal(y_e, y2)
    with pytest.raises(dnn_hip.DnnHipError):
        plan.run_graph(1, x.data_ptr(), y_g.data_ptr(), 0)  # the NULL stream cannot be captured


def test_yolov2tiny_front_end_from_pickle(tmp_path, yolo_weights, golden_frames, post_golden):
    """The reference's model API (YOLO_V2_TINY(in_shape, weight_pickle, debug).inference +
    postprocessing) on our engine, weights read from a pickle by the safe loader."""
    import yolo_weights as YW
    import yolov2tiny
    p = tmp_path / "y2t_weights.pickle"
    YW.save_y2t_weights(yolo_weights, p)
    y2t = yolov2tiny.YOLO_V2_TINY([1, 416, 416, 3], str(p), False)
    out = y2t.inference(synth.frame(0))
    assert R.normwise_err(out, golden_frames[0]) < NET_TOL
    boxes = yolov2tiny.postprocessing(np.squeeze(out))
    import post_numpy as PN
    assert boxes == PN.postprocessing(np.squeeze(out))  # same tensor: exact
    # vs the reference's detections on ITS output (1e-6-level differences in the raw tensor
    # can move a truncated corner of a huge box by one pixel)
    gold = post_golden["net_frame0"][1]
    assert [b[0] for b in boxes] == [g[0] for g in gold]


# ------------------------------------------------------------------ fused split-K combine
SPLITK_CASES = [
    # B, H, W, C, od, pool: K = 9*C >= 2048 and od >= 512 -> split-K 3 (128x512 / 128x256 tiles)
    (64, 13, 13, 256, 512, (2, 1, "SAME")),  # conv5: 85 x 1 tiles, then the stride-1 pool
    (64, 13, 13, 512, 1024, None),           # conv6: 85 x 2 tiles
    (5, 13, 13, 512, 1024, None),            # ragged M = 845 (not a multiple of 128), few tiles
    (3, 9, 7, 256, 768, None),               # N = 768 -> 128x256 tiles, M = 189
]


@pytest.mark.parametrize("case", SPLITK_CASES)
def test_splitk_combine_in_gemm_equals_reduce_kernel(monkeypatch, case):
    """The last-arriving split of each tile sums the partials in split order inside the GEMM
    (agent-scope ticket, sc1 partials, gemm_f32.h splitk_combine): bit-identical to the
    separate ordered reduce kernel (DNN_HIP_SPLITK_FUSED=0), within the layer tolerance of
    the float64 oracle, and the same again on repeated runs and HIP-graph replays (the
    tickets re-arm themselves)."""
    B, H, W, C, od, pool = case
    rng = np.random.default_rng(B + C + od)
    x = rng.standard_normal((B, H, W, C)).astype(np.float32)
    k = (rng.standard_normal((3, 3, C, od)) * np.sqrt(2.0 / (9 * C))).astype(np.float32)
    bias = rng.standard_normal(od).astype(np.float32) * 0.1
    gam = rng.uniform(0.5, 1.5, od).astype(np.float32)
    gam[::7] *= -1  # negative gamma: the epilogue's decreasing branch
    bn = (rng.standard_normal(od).astype(np.float32) * 0.1, rng.uniform(0.5, 1.5, od).astype(np.float32), gam)
    kw = dict(bias=bias, bn=bn, leaky=True, pool=pool)
    monkeypatch.setenv("DNN_HIP_SPLITK_FUSED", "0")
    e_red = dnn_hip.DnnInferenceEngine(_chain(x.shape, k, **kw), False)
    y_red = e_red.run(x)
    assert "combine" not in e_red.plan().describe()
    monkeypatch.setenv("DNN_HIP_SPLITK_FUSED", "1")
    e_fus = dnn_hip.DnnInferenceEngine(_chain(x.shape, k, **kw), False)
    assert "splitK=3 combine" in e_fus.plan().describe()
    y1 = e_fus.run(x)
    y2 = e_fus.run(x)
    assert np.array_equal(y1, y_red) and np.array_equal(y2, y_red)
    assert R.normwise_err(y1, _oracle_chain(x, k, **kw)) < LAYER_TOL
    # device-resident runs and graph replays, with another layer's launch in between
    import torch
    plan = e_fus.plan()
    xd = torch.from_numpy(x).cuda()
    yd = torch.empty((B,) + plan.out_shape, device="cuda")
    st = torch.cuda.Stream()
    for it in range(3):
        plan.run_graph(B, xd.data_ptr(), yd.data_ptr(), st.cuda_stream)
        e_red.plan().run_host(x[:1])  # interleave other work
    st.synchronize()
    assert np.array_equal(yd.cpu().numpy(), y_red)


# ------------------------------------------------------------------ buffer-descriptor DMA
BUF_CASES = [
    # B, H, W, C, od, pool, precision: implicit GEMMs whose A/B DMAs go through buffer
    # descriptors (padding taps = out-of-range offsets, zero-filled by the hardware)
    (3, 20, 18, 32, 64, (2, 2, "SAME"), "fp32"),    # conv2-like, 256x64 / small-M tiles, edges
    (2, 13, 13, 128, 256, (2, 2, "SAME"), "fp32"),  # odd 13x13 -> 7x7 pool padding
    (64, 13, 13, 512, 1024, None, "fp32"),           # conv6: split-K 3 + combine
    (3, 20, 18, 32, 64, (2, 2, "SAME"), "fp16"),    # fp16 C = 32: two taps per K-step
    (2, 16, 16, 64, 128, None, "fp16"),              # fp16 C = 64: one tap per K-step
    (64, 13, 13, 256, 512, (2, 1, "SAME"), "fp16"),  # fp16 conv5: split-K 3 + combine, s1 pool
]


@pytest.mark.parametrize("case", BUF_CASES)
def test_buffer_dma_equals_flat_dma(monkeypatch, case):
    """Buffer-descriptor LDS-DMA (32-bit voffsets, OOB padding taps) gives the same bits as the
    flat-address DMA with the zero page (DNN_HIP_GEMM_BUF=0), fp32 and fp16, with and without
    the in-GEMM split-K combine."""
    B, H, W, C, od, pool, prec = case
    rng = np.random.default_rng(B * 3 + C + od)
    x = rng.standard_normal((B, H, W, C)).astype(np.float32)
    k = (rng.standard_normal((3, 3, C, od)) * np.sqrt(2.0 / (9 * C))).astype(np.float32)
    bias = rng.standard_normal(od).astype(np.float32) * 0.1
    bn = (rng.standard_normal(od).astype(np.float32) * 0.1, rng.uniform(0.5, 1.5, od).astype(np.float32),
          rng.uniform(0.5, 1.5, od).astype(np.float32))
    kw = dict(bias=bias, bn=bn, leaky=True, pool=pool)
    monkeypatch.setenv("DNN_HIP_GEMM_BUF", "0")
    y_flat = dnn_hip.DnnInferenceEngine(_chain(x.shape, k, **kw), False, precision=prec).run(x)
    monkeypatch.delenv("DNN_HIP_GEMM_BUF")
    y_buf = dnn_hip.DnnInferenceEngine(_chain(x.shape, k, **kw), False, precision=prec).run(x)
    assert np.array_equal(y_buf, y_flat)
    if prec == "fp16":  # fused combine == the fp16 reduce kernel
        monkeypatch.setenv("DNN_HIP_SPLITK_FUSED", "0")
        y_red = dnn_hip.DnnInferenceEngine(_chain(x.shape, k, **kw), False, precision=prec).run(x)
        assert np.array_equal(y_buf, y_red)
    ref = _oracle_chain(x, k, **kw)
    assert R.normwise_err(y_buf, ref) < (LAYER_TOL if prec == "fp32" else 5e-3)


# ------------------------------------------------------------------ fp16 path (BASELINE config 5)
FP16_LAYER_TOL = 5e-3   # normwise vs the fp32 oracle: fp16 inputs/weights/outputs (2^-11 each), fp32 accumulate
FP16_NET_TOL = 2e-2     # whole net vs the fp32 reference goldens (SURVEY.md §8d suggested bound)

FP16_CASES = [
    # B, H, W, C, kh, od, pool (2x2 s2 | s1 | None)
    (2, 26, 22, 16, 3, 32, "s2"),     # conv1-like: 4 taps per 64-half K-step
    (3, 20, 18, 32, 3, 64, "s2"),     # conv2-like
    (2, 13, 13, 32, 3, 64, "s2"),     # odd 13x13 -> 7x7 pool padding
    (4, 16, 16, 64, 3, 128, None),    # conv3-like, no pool
    (64, 13, 13, 256, 3, 512, "s1"),  # conv5-like: split-K 3 + reduce, then the stride-1 pool
    (3, 13, 13, 64, 1, 125, None),    # 1x1 dense, ragged N
    (2, 40, 38, 3, 3, 16, "s2"),      # conv0-like: direct kernel, fp32 frames -> fp16 activations
]


@pytest.mark.parametrize("case", FP16_CASES)
def test_fp16_layers_vs_oracle(case):
    B, H, W, C, kh, od, pool = case
    rng = np.random.default_rng(B * 7 + C + od)
    x = rng.standard_normal((B, H, W, C)).astype(np.float32)
    k = (rng.standard_normal((kh, kh, C, od)) * np.sqrt(2.0 / (kh * kh * C))).astype(np.float32)
    bias = rng.standard_normal(od).astype(np.float32) * 0.1
    bn = (rng.standard_normal(od).astype(np.float32) * 0.1, rng.uniform(0.5, 1.5, od).astype(np.float32),
          rng.uniform(0.5, 1.5, od).astype(np.float32))
    pl = {"s2": (2, 2, "SAME"), "s1": (2, 1, "SAME"), None: None}[pool]
    kw = dict(bias=bias, bn=bn, leaky=True, pool=pl)
    eng = dnn_hip.DnnInferenceEngine(_chain(x.shape, k, **kw), False, precision="fp16")
    y = eng.run(x)
    assert " fp16" in eng.plan().describe()
    ref = _oracle_chain(x, k, **kw)
    assert y.shape == ref.shape and y.dtype == np.float32
    assert R.normwise_err(y, ref) < FP16_LAYER_TOL


def test_fp16_yolo_vs_reference_golden_and_batch_invariance(yolo_weights, golden_frames):
    """Whole YOLOv2-tiny in fp16 vs the fp32 reference goldens, and batch-64 rows == batch-1
    runs bit for bit (the fp16 plan's summation order also depends on (N, K) only)."""
    g1, _ = yolo_graph.build_graph(dnn_hip.DnnGraphBuilder, yolo_weights, in_shape=(1, 416, 416, 3))
    e1 = dnn_hip.DnnInferenceEngine(g1, False, precision="fp16")
    errs = []
    for f in range(4):
        y = e1.run(synth.frame(f))
        errs.append(R.normwise_err(y, golden_frames[f]))
    assert max(errs) < FP16_NET_TOL, errs
    idx = [0, 1, 2, 3] + [100 + i for i in range(60)]
    x = synth.frames(idx)
    g64, _ = yolo_graph.build_graph(dnn_hip.DnnGraphBuilder, yolo_weights, in_shape=(64, 416, 416, 3))
    e64 = dnn_hip.DnnInferenceEngine(g64, False, precision="fp16")
    y64 = e64.run(x)
    # two batch-64 runs of the same frames are equal (round 5 found a since-removed fp16 tile-kernel
    # form whose batch-64 outputs differed run to run: DESIGN.md §2 "fp16 tile-kernel race")
    assert np.array_equal(e64.run(x), y64)
    for pos in (0, 3, 17, 63):
        assert np.array_equal(y64[pos:pos + 1], e1.run(x[pos:pos + 1]))


F16_HEAD_CASES = [
    # B, H, W, C, od (the 1x1 head's width): conv3x3 C -> 128 (+ BN, leaky) -> conv1x1 128 -> od (+ bias)
    (3, 13, 13, 64, 125),  # YOLO's conv8 width: Npad 128, the fp32-output launcher
    (2, 13, 13, 64, 64),   # Npad 64 < the launcher's 128-column tiles: the general path + conversion
    (2, 9, 11, 32, 30),    # Npad 32
]


@pytest.mark.parametrize("case", F16_HEAD_CASES)
def test_fp16_direct_output_head(monkeypatch, case):
    """The fp16 plan's last dense layer storing its fp32 epilogue values as the plan output
    (launch_gemm16_f32out, default) vs DNN_HIP_F16_DIRECT_OUT=0 (fp16 output + a conversion
    kernel): both within the fp16 tolerance of the fp32 oracle, equal within the fp16 rounding of
    the output, the conversion kernel absent exactly when the launcher runs, and only for heads
    whose Npad covers its 128-column tiles (narrower heads read past their weights)."""
    B, H, W, C, od = case
    rng = np.random.default_rng(B + C + od)
    x = rng.standard_normal((B, H, W, C)).astype(np.float32)
    k1 = (rng.standard_normal((3, 3, C, 128)) * np.sqrt(2.0 / (9 * C))).astype(np.float32)
    k2 = (rng.standard_normal((1, 1, 128, od)) * np.sqrt(2.0 / 128)).astype(np.float32)
    b1, b2 = rng.standard_normal(128).astype(np.float32) * 0.1, rng.standard_normal(od).astype(np.float32) * 0.1
    bn1 = (rng.standard_normal(128).astype(np.float32) * 0.1, rng.uniform(0.5, 1.5, 128).astype(np.float32),
           rng.uniform(0.5, 1.5, 128).astype(np.float32))

    def graph(shape):
        g = dnn_hip.DnnGraphBuilder()
        y = g.create_input(list(shape))
        y = g.create_conv2d(y, k1, [1, 1, 1, 1], "SAME")
        y = g.create_bias_add(y, b1)
        y = g.create_batch_norm(y, *bn1, 1e-5)
        y = g.create_leaky_relu(y)
        y = g.create_conv2d(y, k2, [1, 1, 1, 1], "SAME")
        y = g.create_bias_add(y, b2)
        g.set_out_node(y)
        return g

    ref = R.bias_add(R.conv2d(R.leaky_relu(R.batch_norm(R.bias_add(R.conv2d(x, k1), b1), *bn1, 1e-5)), k2), b2)
    outs = {}
    for arm in ("1", "0"):
        if arm == "1":
            monkeypatch.delenv("DNN_HIP_F16_DIRECT_OUT", raising=False)
        else:
            monkeypatch.setenv("DNN_HIP_F16_DIRECT_OUT", "0")
        eng = dnn_hip.DnnInferenceEngine(graph(x.shape), False, precision="fp16")
        names = [kk["name"] for kk in eng.plan().kernels()]
        direct = arm == "1" and od > 64
        assert ("output.cvt" in names) == (not direct), (arm, names)
        y = eng.run(x)
        assert np.array_equal(eng.run(x), y)
        err = R.normwise_err(y, ref)
        print("fp16 head", case, arm, "err %.3g" % err)
        assert err < FP16_LAYER_TOL, (arm, err)
        outs[arm] = y
    d = np.abs(outs["1"].astype(np.float64) - outs["0"])
    assert np.all(d <= np.abs(outs["1"]) * 2.0 ** -11 + 2.0 ** -24), float(d.max())


def test_fp16_detections_vs_fp32_within_decision_margins(yolo_weights, golden_frames):
    """BASELINE config 5 at the detection level.  Post-NMS detections of the
    fp16 plan vs the fp32 reference goldens on the 4 golden frames:
      * after dropping from BOTH tensors every box whose class, 0.3-threshold decision or integer
        corners could change within 1.5x the observed per-element fp16 deviation (and near-tied
        overlapping candidates, whose NMS order could flip; oracle/post_margin.py), the
        detection lists are identical (as multisets);
      * of the raw detections, >= 90 % in each direction have a same-class partner with
        IoU >= 0.9 (printed: the measured agreement)."""
    import post_margin as PM
    import post_numpy as PN
    g1, _ = yolo_graph.build_graph(dnn_hip.DnnGraphBuilder, yolo_weights, in_shape=(1, 416, 416, 3))
    e1 = dnn_hip.DnnInferenceEngine(g1, False, precision="fp16")
    stable, rates = 0, []
    for f in range(4):
        p32 = np.asarray(golden_frames[f], np.float32).reshape(13, 13, 5, 25)
        p16 = e1.run(synth.frame(f)).reshape(13, 13, 5, 25)
        margin = 1.5 * np.abs(p16.astype(np.float64) - p32) + 1e-6
        q32, q16, n = PM.drop_unstable(p32, p16, margin)
        stable += n
        d32, d16 = sorted(x[:5] for x in PN.detect(q32)), sorted(x[:5] for x in PN.detect(q16))
        assert d32 == d16, (f, d32, d16)
        r32, r16 = PN.detect(p32), PN.detect(p16)
        rates.append((PM.match_rate(r32, r16), PM.match_rate(r16, r32), len(r32), len(r16)))
    print(f"fp16 detections: {stable} decision-stable candidates over 4 frames; agreement "
          f"(fp32->fp16, fp16->fp32, n32, n16) per frame: {rates}")
    assert stable >= 20  # measured 41 (MI355X): the identity is not vacuous
    assert min(min(r[0], r[1]) for r in rates) >= 0.9, rates  # measured 0.96-1.0


# ------------------------------------------------------------------ frame ingest (§8f row 3)
@pytest.mark.parametrize("hw", [(416, 416), (480, 640), (240, 320), (417, 203)])
def test_preprocess_frames_vs_restatement(hw):
    """dnn_preprocess_frames == __init__.py:8-12 restated (oracle/ingest_numpy.py): exact for
    the identity size (the reference's own arithmetic), exact vs the restated fixed-point
    INTER_LINEAR for real resizes (parity with cv2 itself unpinned: cv2 is absent)."""
    import ingest
    import ingest_numpy as IN
    rng = np.random.default_rng(hw[0] + hw[1])
    im = rng.integers(0, 256, size=hw + (3,), dtype=np.uint8)
    got = ingest.resize_input_gpu(im)
    assert got.shape == (416, 416, 3) and got.dtype == np.float32
    assert np.array_equal(got, IN.resize_input(im))
    if hw == (416, 416):  # the reference's formula with cv2.resize the identity
        assert np.array_equal(got, np.asarray((im / 255.)[:, :, ::-1], dtype=np.float32))


def test_frame_ingest_pipeline_double_buffer(yolo_b1):
    """FrameIngest: two slots, uploads overlapped with compute, results per batch unchanged."""
    import torch
    import ingest
    import ingest_numpy as IN
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(3)
    batches = [rng.integers(0, 256, size=(3, 240, 320, 3), dtype=np.uint8) for _ in range(4)]
    fi = ingest.FrameIngest(3, 240, 320, dev)
    outs = []
    for b in batches:
        x = fi.submit(b)
        outs.append(x.clone())  # the "forward" consuming the batch on the compute stream
        fi.release()
    torch.cuda.synchronize()
    for b, o in zip(batches, outs):
        ref = np.stack([IN.resize_input(f) for f in b])
        assert np.array_equal(o.cpu().numpy(), ref)


def test_frame_ingest_rejected_submit_keeps_slot():
    """submit_host with n outside [0, batch] raises before the slot flips, so the
    next valid call still uploads the buffer next_host_buffer() handed out."""
    import ingest
    import ingest_numpy as IN
    rng = np.random.default_rng(5)
    fi = ingest.FrameIngest(2, 60, 80, __import__("torch").device("cuda", 0))
    frames = rng.integers(0, 256, size=(2, 60, 80, 3), dtype=np.uint8)
    fi.next_host_buffer()[:2].numpy()[...] = frames
    slot = fi.slot
    with pytest.raises(ValueError):
        fi.submit_host(3)
    assert fi.slot == slot
    x = fi.submit_host(2)
    __import__("torch").cuda.synchronize()
    assert np.array_equal(x.cpu().numpy(), np.stack([IN.resize_input(f) for f in frames]))


def test_frame_ingest_reuse_ordered_without_release():
    """slot reuse must be ordered without release().  Six batches through two
    slots; a frame decoder rewrites the pinned buffer as soon as next_host_buffer() returns,
    and each batch is read by a slow "forward" on the compute stream (a matmul chain first,
    so the copy stream runs ahead of the compute stream) with no release() call.  A second
    pass reads each batch on a side stream and records that with release(side).  Every batch
    must equal the restated preprocess of its own frames."""
    import torch
    import ingest
    import ingest_numpy as IN
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(31)
    batches = [rng.integers(0, 256, size=(4, 120, 160, 3), dtype=np.uint8) for _ in range(6)]
    busy = torch.randn(2048, 2048, device=dev)
    for use_side in (False, True):
        fi = ingest.FrameIngest(4, 120, 160, dev)
        side = torch.cuda.Stream(dev)
        outs = []
        for b in batches:
            fi.next_host_buffer()[:len(b)].numpy()[...] = b  # the decoder writes in place
            x = fi.submit_host(len(b))
            reader = side if use_side else fi.compute
            reader.wait_stream(fi.compute)
            with torch.cuda.stream(reader):
                y = busy
                for _ in range(8):
                    y = y @ busy  # keeps the reader late
                outs.append(x.clone())
            if use_side:
                fi.release(side)
        torch.cuda.synchronize()
        for b, o in zip(batches, outs):
            ref = np.stack([IN.resize_input(f) for f in b])
            assert np.array_equal(o.cpu().numpy(), ref)


# ------------------------------------------------------------------ latency plans (config 2)
LAT_CASES = [
    # B, H, W, C, od, kernel, pool, forced split (DNN_HIP_SPLIT) or None
    (1, 26, 26, 128, 256, 3, (2, 2, "SAME"), None),   # conv4 at batch 1: split + pool in the combine
    (1, 13, 13, 128, 256, 3, (2, 2, "SAME"), None),   # odd 13x13 -> 7x7 pool (ragged windows)
    (1, 13, 13, 1024, 1024, 3, None, None),           # conv7 at batch 1
    (1, 13, 13, 1024, 125, 1, None, None),            # conv8: 1x1, N = 125 (not a multiple of 4)
    (1, 13, 13, 512, 512, 3, None, 16),               # 16 splits (the most the combine takes)
    (2, 9, 11, 256, 384, 3, (2, 2, "VALID"), 9),      # M = 2*4*4*5 pooled rows, 9 splits
]


@pytest.mark.parametrize("case", LAT_CASES)
def test_latency_split_combine_vs_oracle(monkeypatch, case):
    """Latency plans split K by M (2..16 splits, the last split sums the partials in split
    order inside the GEMM, gemm_f32.h splitk_sum, then its normal or pool-fused store): within
    the layer tolerance of the float64 oracle, identical across runs and HIP-graph replays."""
    B, H, W, C, od, kk, pool, force = case
    if force:
        monkeypatch.setenv("DNN_HIP_SPLIT", f"{kk * kk * C}:{force}")
    rng = np.random.default_rng(B + C + od + kk)
    x = rng.standard_normal((B, H, W, C)).astype(np.float32)
    k = (rng.standard_normal((kk, kk, C, od)) * np.sqrt(2.0 / (kk * kk * C))).astype(np.float32)
    bias = rng.standard_normal(od).astype(np.float32) * 0.1
    gam = rng.uniform(0.5, 1.5, od).astype(np.float32)
    gam[::5] *= -1
    bn = (rng.standard_normal(od).astype(np.float32) * 0.1, rng.uniform(0.5, 1.5, od).astype(np.float32), gam)
    kw = dict(bias=bias, bn=bn, leaky=True, pool=pool)
    eng = dnn_hip.DnnInferenceEngine(_chain(x.shape, k, **kw), False, latency=True)
    desc = eng.plan().describe()
    want = f" splitK={force} combine" if force else " combine"
    assert want in desc and " latency" in desc, desc
    y1 = eng.run(x)
    y2 = eng.run(x)
    assert np.array_equal(y1, y2)
    assert R.normwise_err(y1, _oracle_chain(x, k, **kw)) < LAYER_TOL
    import torch
    plan = eng.plan()
    xd = torch.from_numpy(x).cuda()
    yd = torch.empty((B,) + plan.out_shape, device="cuda")
    st = torch.cuda.Stream()
    for _ in range(3):
        plan.run_graph(B, xd.data_ptr(), yd.data_ptr(), st.cuda_stream)
    st.synchronize()
    assert np.array_equal(yd.cpu().numpy(), y1)


@pytest.mark.parametrize("frame", [0, 1, 2, 3])
def test_yolo_latency_plan_vs_reference_golden(yolo_weights, golden_frames, frame, latency_b1_engine=[]):
    """BASELINE config 2 in latency mode: conv1 on the 16-channel x3 kernel's 4 x 26 tiles, conv2
    on the x3 tile kernel's 2 x 26 tiles, conv3 / conv4 / conv5 on the x3 kernel with
    the K split inside the workgroup (pool5 fused into conv5), conv6 / conv7 on the small-M x3
    kernel, conv8 on the 1x1 form of the K-split kernel; within the net tolerance of the reference goldens
    (not bit-equal to the batch plan's rows)."""
    if not latency_b1_engine:
        g, _ = yolo_graph.build_graph(dnn_hip.DnnGraphBuilder, yolo_weights, in_shape=(1, 416, 416, 3))
        latency_b1_engine.append(dnn_hip.DnnInferenceEngine(g, False, latency=True))
    eng = latency_b1_engine[0]
    desc = eng.plan().describe()
    conv = [ln for ln in desc.splitlines() if ln.startswith("conv")]
    assert "mode=x3_ktile" in conv[4] and "mode=x3_ktile" in conv[5] and "+pool2x2s1" in conv[5], desc
    assert "mode=x3_ktile" in conv[8], desc  # conv8: the 1x1 K-split x3 kernel
    assert "mode=x3_lat" in conv[6] and "mode=x3_lat" in conv[7], desc  # conv6 / conv7: small-M x3
    assert all("mode=patch_x3" in conv[i] for i in (1, 2)) and "mode=x3_ktile" in conv[3], desc  # conv1-conv3: x3
    y = eng.run(synth.frame(frame))
    assert R.normwise_err(y, golden_frames[frame]) < NET_TOL


X3_KTILE_CASES = [
    # B, pool5: pool 2x2 s1 -> conv3x3 128->256 + pool 2x2 s2 (26x26: the pooled 26-wide shape, 4 K
    # groups of one chunk) -> conv3x3 256->512 (13x13: the 13-wide shape, 4 groups of two chunks)
    # [-> pool 2x2 s1 SAME, fused into it], in a latency plan (YOLO's conv4 / conv5 / pool5)
    (1, True), (2, True), (2, False),
]


@pytest.mark.parametrize("case", X3_KTILE_CASES)
def test_x3_ktile_kernel_vs_oracle(monkeypatch, case):
    """conv3x3_x3_ktile_kernel (latency plans' conv4 / conv5): the K split over 4 wave groups
    inside the workgroup, the groups' folded sums added in group order, then the fused pool
    (2x2/s2, or 2x2/s1 SAME with the row below each tile computed too) and epilogue.  Each chain
    within the fp32 tolerance of the float64 oracle and within 1.25x of the fp32 MFMA latency
    plan's error (DNN_HIP_X3=0); repeat runs and graph replays identical; a two-frame run's rows
    equal to one-frame runs (the tiling has no cross-frame state)."""
    B, pool5 = case
    rng = np.random.default_rng(11 + B)
    x = rng.standard_normal((B, 26, 26, 128)).astype(np.float32)

    def layer(c, od):
        k = (rng.standard_normal((3, 3, c, od)) * np.sqrt(2.0 / (9 * c))).astype(np.float32)
        b = rng.standard_normal(od).astype(np.float32) * 0.1
        gam = rng.uniform(0.5, 1.5, od).astype(np.float32)
        gam[::5] *= -1
        return k, b, (rng.standard_normal(od).astype(np.float32) * 0.1, rng.uniform(0.5, 1.5, od).astype(np.float32),
                      gam)

    L = [layer(128, 256), layer(256, 512)]

    def graph(shape):
        g = dnn_hip.DnnGraphBuilder()
        y = g.create_input(list(shape))
        y = g.create_max_pool2d(y, [1, 2, 2, 1], [1, 1, 1, 1], "SAME")
        for j, (k, b, n) in enumerate(L):
            y = g.create_conv2d(y, k, [1, 1, 1, 1], "SAME")
            y = g.create_bias_add(y, b)
            y = g.create_batch_norm(y, *n, 1e-5)
            y = g.create_leaky_relu(y)
            if j == 0 or pool5:
                y = g.create_max_pool2d(y, [1, 2, 2, 1], [1, 2, 2, 1] if j == 0 else [1, 1, 1, 1], "SAME")
        g.set_out_node(y)
        return g

    ref = R.max_pool2d(x, [1, 2, 2, 1], [1, 1, 1, 1], "SAME")
    for j, (k, b, n) in enumerate(L):
        ref = R.leaky_relu(R.batch_norm(R.bias_add(R.conv2d(ref, k), b), *n, 1e-5))
        if j == 0 or pool5:
            ref = R.max_pool2d(ref, [1, 2, 2, 1], [1, 2, 2, 1] if j == 0 else [1, 1, 1, 1], "SAME")
    errs = {}
    for x3 in ("1", "0"):
        monkeypatch.setenv("DNN_HIP_X3", x3)
        eng = dnn_hip.DnnInferenceEngine(graph(x.shape), False, latency=True)
        desc = eng.plan().describe()
        conv = [ln for ln in desc.splitlines() if ln.startswith("conv")]
        if x3 == "1":
            assert "mode=x3_ktile" in conv[0] and "+pool2x2s2" in conv[0] and "mode=x3_ktile" in conv[1], desc
            assert ("+pool2x2s1" in conv[1]) == pool5 and desc.count("pool ") == 1, desc
        y = eng.run(x)
        errs[x3] = R.normwise_err(y, ref)
        if x3 == "1":
            assert np.array_equal(eng.run(x), y)
            import torch
            p = eng.plan()
            xd = torch.from_numpy(x).cuda()
            yd = torch.empty((B,) + p.out_shape, device="cuda")
            st = torch.cuda.Stream()
            for _ in range(2):
                p.run_graph(B, xd.data_ptr(), yd.data_ptr(), st.cuda_stream)
            st.synchronize()
            assert np.array_equal(yd.cpu().numpy(), y)
            if B > 1:
                one = dnn_hip.DnnInferenceEngine(graph((1,) + x.shape[1:]), False, latency=True)
                for f in range(B):
                    assert np.array_equal(one.run(x[f:f + 1]), y[f:f + 1]), f
    print("ktile chain errs", errs)
    assert errs["1"] < 3 * LAYER_TOL and errs["0"] < 3 * LAYER_TOL, errs
    assert errs["1"] <= 1.25 * errs["0"], errs


@pytest.mark.parametrize("B", [1, 3])
def test_x3_ktile_conv3_shape_vs_oracle(B):
    """The K-split x3 kernel's conv3 shape (latency plans: 52x52x64 -> 128 + 2x2/s2 pool, two
    26-wide tile columns, 2 K groups of 2 x 2 row blocks): within the fp32 tolerance of the
    float64 oracle, repeat runs identical, a 3-frame run's rows equal to one-frame runs."""
    rng = np.random.default_rng(5 + B)
    x = rng.standard_normal((B, 52, 52, 64)).astype(np.float32)
    k = (rng.standard_normal((3, 3, 64, 128)) * np.sqrt(2.0 / 576)).astype(np.float32)
    b = rng.standard_normal(128).astype(np.float32) * 0.1
    gam = rng.uniform(0.5, 1.5, 128).astype(np.float32)
    gam[::5] *= -1
    n = (rng.standard_normal(128).astype(np.float32) * 0.1, rng.uniform(0.5, 1.5, 128).astype(np.float32), gam)

    def graph(shape):
        g = dnn_hip.DnnGraphBuilder()
        y = g.create_input(list(shape))
        y = g.create_max_pool2d(y, [1, 2, 2, 1], [1, 1, 1, 1], "SAME")
        y = g.create_conv2d(y, k, [1, 1, 1, 1], "SAME")
        y = g.create_bias_add(y, b)
        y = g.create_batch_norm(y, *n, 1e-5)
        y = g.create_leaky_relu(y)
        y = g.create_max_pool2d(y, [1, 2, 2, 1], [1, 2, 2, 1], "SAME")
        g.set_out_node(y)
        return g

    ref = R.max_pool2d(x, [1, 2, 2, 1], [1, 1, 1, 1], "SAME")
    ref = R.leaky_relu(R.batch_norm(R.bias_add(R.conv2d(ref, k), b), *n, 1e-5))
    ref = R.max_pool2d(ref, [1, 2, 2, 1], [1, 2, 2, 1], "SAME")
    eng = dnn_hip.DnnInferenceEngine(graph(x.shape), False, latency=True)
    conv = [ln for ln in eng.plan().describe().splitlines() if ln.startswith("conv")]
    assert "mode=x3_ktile" in conv[0] and "+pool2x2s2" in conv[0], conv
    y = eng.run(x)
    assert np.array_equal(eng.run(x), y)
    assert R.normwise_err(y, ref) < LAYER_TOL
    if B > 1:
        one = dnn_hip.DnnInferenceEngine(graph((1,) + x.shape[1:]), False, latency=True)
        for f in range(B):
            assert np.array_equal(one.run(x[f:f + 1]), y[f:f + 1]), f


KTILE_SHAPE_CASES = [
    # B, H, W, C, OC, pool (0 none, 1 2x2/s2, 2 2x2/s1 SAME fused): frames the K-split kernel's
    # shape table (kernels_x3.hip x3_ktile_shape) accepts beyond YOLO's -- partial 13- / 14- / 26-wide
    # tiles, odd frames under the stride-1 pool, output widths 64 and 192
    (2, 9, 11, 256, 192, 2),
    (1, 13, 13, 256, 64, 0),
    (2, 18, 18, 128, 64, 1),
    (1, 20, 24, 128, 128, 0),
    (2, 30, 38, 64, 128, 1),
]


@pytest.mark.parametrize("case", KTILE_SHAPE_CASES)
def test_x3_ktile_shapes_vs_oracle(case):
    """conv3x3_x3_ktile_kernel on every shape class it accepts at non-YOLO frame sizes: within the
    fp32 tolerance of the float64 oracle, repeat runs identical, multi-frame rows equal to one-frame
    runs."""
    B, H, W, C, OC, pool = case
    rng = np.random.default_rng(H * 100 + W + C + OC)
    x = rng.standard_normal((B, H, W, C)).astype(np.float32)
    k = (rng.standard_normal((3, 3, C, OC)) * np.sqrt(2.0 / (9 * C))).astype(np.float32)
    b = rng.standard_normal(OC).astype(np.float32) * 0.1
    gam = rng.uniform(0.5, 1.5, OC).astype(np.float32)
    gam[::5] *= -1
    n = (rng.standard_normal(OC).astype(np.float32) * 0.1, rng.uniform(0.5, 1.5, OC).astype(np.float32), gam)
    pstride = [1, 2, 2, 1] if pool == 1 else [1, 1, 1, 1]

    def graph(shape):
        g = dnn_hip.DnnGraphBuilder()
        y = g.create_input(list(shape))
        y = g.create_max_pool2d(y, [1, 2, 2, 1], [1, 1, 1, 1], "SAME")  # an x3 producer (split planes)
        y = g.create_conv2d(y, k, [1, 1, 1, 1], "SAME")
        y = g.create_bias_add(y, b)
        y = g.create_batch_norm(y, *n, 1e-5)
        y = g.create_leaky_relu(y)
        if pool:
            y = g.create_max_pool2d(y, [1, 2, 2, 1], pstride, "SAME")
        g.set_out_node(y)
        return g

    ref = R.max_pool2d(x, [1, 2, 2, 1], [1, 1, 1, 1], "SAME")
    ref = R.leaky_relu(R.batch_norm(R.bias_add(R.conv2d(ref, k), b), *n, 1e-5))
    if pool:
        ref = R.max_pool2d(ref, [1, 2, 2, 1], pstride, "SAME")
    eng = dnn_hip.DnnInferenceEngine(graph(x.shape), False, latency=True)
    desc = eng.plan().describe()
    conv = [ln for ln in desc.splitlines() if ln.startswith("conv")]
    assert "mode=x3_ktile" in conv[0], desc
    if pool:
        assert ("+pool2x2s2" if pool == 1 else "+pool2x2s1") in conv[0], desc
    y = eng.run(x)
    assert y.shape == ref.shape
    assert np.array_equal(eng.run(x), y)
    err = R.normwise_err(y, ref)
    print("ktile shape", case, "err %.3g" % err)
    assert err < LAYER_TOL, err
    if B > 1:
        one = dnn_hip.DnnInferenceEngine(graph((1,) + x.shape[1:]), False, latency=True)
        for f in range(B):
            assert np.array_equal(one.run(x[f:f + 1]), y[f:f + 1]), f


X3_LAT_CASES = [
    # B, H, W, C, od1, od2, forced chunks per workgroup (DNN_HIP_X3L_CPW) or None, 1x1 outputs
    # or None: pool (2x2 s1) -> conv3x3 C->od1 -> conv3x3 od1->od2 [-> conv1x1 + bias] in a
    # latency plan, both 3x3 convs on the small-M x3 kernel (any workgroup count here)
    (1, 13, 13, 512, 1024, 1024, None, 125),  # conv6 / conv7 / conv8 at batch 1
    (2, 13, 13, 512, 320, 256, None, None),   # two frames: two 176-row tiles, the second straddling
    (1, 9, 11, 64, 192, 320, None, 40),       # non-square frame, N = 192 / 320, 2 and 6 chunks, small head
    (1, 13, 13, 128, 192, 256, 2, None),      # two chunks per workgroup forced (4 -> 2 slices; 6 -> 3)
]


@pytest.mark.parametrize("case", X3_LAT_CASES)
def test_x3_latency_kernel_vs_oracle(monkeypatch, case):
    """conv3x3_x3_lat_kernel (latency plans): 64-column workgroups over one or two 32-channel
    chunks, raw slice partials summed in slice order by the combine kernel with the epilogue
    (then YOLO's conv8-like 1x1 head on the fp32 MFMA).  Each layer within the fp32 LAYER_TOL
    of the float64 oracle and within 1.25x of the fp32 MFMA latency plan's error
    (DNN_HIP_X3=0), repeat runs and HIP-graph replays identical."""
    B, H, W, C, od1, od2, cpw, head = case
    monkeypatch.setenv("DNN_HIP_X3_LAT_MINWG", "1")
    if cpw:
        monkeypatch.setenv("DNN_HIP_X3L_CPW", str(cpw))
    rng = np.random.default_rng(B + C + od1 + od2)
    x = rng.standard_normal((B, H, W, C)).astype(np.float32)

    def layer(c, od, kk=3, bn=True):
        k = (rng.standard_normal((kk, kk, c, od)) * np.sqrt(2.0 / (kk * kk * c))).astype(np.float32)
        b = rng.standard_normal(od).astype(np.float32) * 0.1
        if not bn:
            return k, b, None
        gam = rng.uniform(0.5, 1.5, od).astype(np.float32)
        gam[::5] *= -1
        return k, b, (rng.standard_normal(od).astype(np.float32) * 0.1, rng.uniform(0.5, 1.5, od).astype(np.float32), gam)

    L = [layer(C, od1), layer(od1, od2)] + ([layer(od2, head, 1, False)] if head else [])

    def graph(layers):
        g = dnn_hip.DnnGraphBuilder()
        y = g.create_input(list(x.shape))
        y = g.create_max_pool2d(y, [1, 2, 2, 1], [1, 1, 1, 1], "SAME")
        for k, b, n in layers:
            y = g.create_conv2d(y, k, [1, 1, 1, 1], "SAME")
            y = g.create_bias_add(y, b)
            if n is not None:  # (the 1x1 head: bias only, as YOLO's conv8)
                y = g.create_batch_norm(y, *n, 1e-5)
                y = g.create_leaky_relu(y)
        g.set_out_node(y)
        return g

    ref = [R.max_pool2d(x, [1, 2, 2, 1], [1, 1, 1, 1], "SAME")]
    for k, b, n in L:
        y = R.bias_add(R.conv2d(ref[-1], k), b)
        ref.append(y if n is None else R.leaky_relu(R.batch_norm(y, *n, 1e-5)))
    errs = {}
    for x3 in ("1", "0"):
        monkeypatch.setenv("DNN_HIP_X3", x3)
        e1 = dnn_hip.DnnInferenceEngine(graph(L[:1]), False, latency=True)
        e2 = dnn_hip.DnnInferenceEngine(graph(L), False, latency=True)
        desc = e2.plan().describe()
        assert desc.count("mode=x3_lat") == (2 if x3 == "1" else 0), desc
        y1, y2 = e1.run(x), e2.run(x)
        errs[x3] = (R.normwise_err(y1, ref[1]), R.normwise_err(y2, ref[-1]))
        print("x3=%s layer/chain normwise err %.3e %.3e" % (x3, errs[x3][0], errs[x3][1]))
        if x3 == "1":
            assert " x3-combine latency" in desc, desc
            assert np.array_equal(e2.run(x), y2)
            import torch
            plan = e2.plan()
            xd = torch.from_numpy(x).cuda()
            yd = torch.empty((B,) + plan.out_shape, device="cuda")
            st = torch.cuda.Stream()
            for _ in range(3):
                plan.run_graph(B, xd.data_ptr(), yd.data_ptr(), st.cuda_stream)
            st.synchronize()
            assert np.array_equal(yd.cpu().numpy(), y2)
    nl = len(L)
    for x3 in ("0", "1"):
        assert errs[x3][0] < LAYER_TOL and errs[x3][1] < nl * LAYER_TOL, (x3, errs)
    assert errs["1"][0] <= 1.25 * errs["0"][0] and errs["1"][1] <= 1.25 * errs["0"][1], errs


IM2COL_ROW_CASES = [
    # B, H, W, C, kh, stride, pad: C % 4 != 0 -> the row-staged explicit im2col
    (2, 40, 38, 3, 3, 1, "SAME"),   # conv0-like
    (3, 9, 11, 5, 3, 2, "SAME"),    # stride 2, C = 5: Kpad / 4 = 12 does not divide 256 -> gather path
    (2, 9, 11, 3, 3, 2, "SAME"),    # stride 2 through the row-staged kernel
    (1, 10, 9, 3, 3, 1, "VALID"),
    (2, 7, 6, 6, 1, 1, "SAME"),     # 1x1 on C = 6 (explicit path: C % 32 != 0)
]


@pytest.mark.parametrize("case", IM2COL_ROW_CASES)
def test_im2col_rows_equals_gather_path(monkeypatch, case):
    """The unfused plan's explicit im2col for C % 4 != 0 stages the kh input rows of an output
    row in LDS and writes coalesced float4s (im2col_rows_kernel); its col buffer, hence the
    plan's output, is bit-identical to the per-element gather kernel (DNN_HIP_IM2COL_ROWS=0)."""
    B, H, W, C, kh, s, pad = case
    rng = np.random.default_rng(H * W + C)
    x = rng.standard_normal((B, H, W, C)).astype(np.float32)
    k = (rng.standard_normal((kh, kh, C, 16)) * 0.3).astype(np.float32)
    kw = dict(strides=(1, s, s, 1), pad=pad, bias=rng.standard_normal(16).astype(np.float32), leaky=True)
    monkeypatch.setenv("DNN_HIP_FUSE", "0")
    outs = []
    for rows in ("1", "0"):
        monkeypatch.setenv("DNN_HIP_IM2COL_ROWS", rows)
        outs.append(dnn_hip.DnnInferenceEngine(_chain(x.shape, k, **kw), False).run(x))
    assert np.array_equal(outs[0], outs[1])
    assert R.normwise_err(outs[0], _oracle_chain(x, k, **kw)) < LAYER_TOL


PERSIST_CASES = [
    # B, H, W, C, od, pool: unsplit implicit layers on the configs the persistent kernel covers
    (16, 104, 104, 32, 64, True),   # conv2 at batch 16: 256x64 tiles, 676 tiles > one round
    (16, 52, 52, 64, 128, True),    # conv3: 64x128
    (64, 26, 26, 128, 256, True),   # conv4 at batch 64: 64x128 forced (DNN_HIP_CFG), two N tiles
    (9, 27, 25, 64, 128, True),     # odd 27x25 -> 14x13 pool windows (ragged), partial last tile
    (12, 30, 30, 32, 128, False),   # no pool (MODE 1)
]


@pytest.mark.parametrize("case", PERSIST_CASES)
def test_persistent_gemm_equals_tile_kernel(monkeypatch, case):
    """The persistent implicit GEMM (gemm_persist.h: one workgroup walks many tiles, the LDS-DMA
    ring runs across tile boundaries, counted waits include the epilogue's fixed store count)
    gives the same bits as one tile per workgroup (DNN_HIP_PERSIST=0), and matches the oracle."""
    B, H, W, C, od, pool = case
    rng = np.random.default_rng(B + H + C + od)
    x = rng.standard_normal((B, H, W, C)).astype(np.float32)
    k = (rng.standard_normal((3, 3, C, od)) * np.sqrt(2.0 / (9 * C))).astype(np.float32)
    gam = rng.uniform(0.5, 1.5, od).astype(np.float32)
    gam[::3] *= -1
    kw = dict(bias=rng.standard_normal(od).astype(np.float32) * 0.1,
              bn=(rng.standard_normal(od).astype(np.float32) * 0.1, rng.uniform(0.5, 1.5, od).astype(np.float32), gam),
              leaky=True, pool=(2, 2, "SAME") if pool else None)
    outs = {}
    if C == 128:
        monkeypatch.setenv("DNN_HIP_CFG", "1152:4")  # 64x128: 1352 tiles, per-N-tile epilogue params
    for on in ("1", "0"):
        monkeypatch.setenv("DNN_HIP_PERSIST", "2" if on == "1" else "0")  # 2: every covered config
        eng = dnn_hip.DnnInferenceEngine(_chain(x.shape, k, **kw), False)
        outs[on] = eng.run(x)
        outs[on + "b"] = eng.run(x)
    assert np.array_equal(outs["1"], outs["0"]) and np.array_equal(outs["1b"], outs["1"])
    idx = np.arange(0, B, max(1, B // 3))
    assert R.normwise_err(outs["1"][idx], _oracle_chain(x[idx], k, **kw)) < LAYER_TOL


@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_shape_only_plan_with_copied_arena(yolo_weights, precision):
    """A rank that lays the plan out without weights (upload=False: the bench's non-root ranks,
    whose packed arena arrives by broadcast) must run the same epilogue as the uploading rank:
    with rank 0's arena copied in, its outputs equal rank 0's bit for bit."""
    import torch
    g, _ = yolo_graph.build_graph(dnn_hip.DnnGraphBuilder, yolo_weights, in_shape=(2, 416, 416, 3))
    entries = dnn_hip.lower_graph(g)
    wb, sb = dnn_hip.Plan.memory(2, (416, 416, 3), entries, precision=precision)
    bufs = [(torch.empty(wb, dtype=torch.uint8, device="cuda"), torch.empty(sb, dtype=torch.uint8, device="cuda"))
            for _ in range(2)]
    plans = [dnn_hip.Plan(2, (416, 416, 3), entries, device=0, weights_ptr=w.data_ptr(), workspace_ptr=s.data_ptr(),
                          upload=(k == 0), precision=precision) for k, (w, s) in enumerate(bufs)]
    bufs[1][0].copy_(bufs[0][0])
    x = torch.from_numpy(synth.frames([0, 1])).cuda()
    ys = [torch.empty((2, 13, 13, 125), device="cuda") for _ in range(2)]
    for p, y in zip(plans, ys):
        p.run_device(2, x.data_ptr(), y.data_ptr())
    torch.cuda.synchronize()
    assert torch.equal(ys[0], ys[1])
    assert R.normwise_err(ys[0][:1].cpu().numpy(), golden_frames_0()) < (NET_TOL if precision == "fp32" else 2e-2)
    for p in plans:
        p.close()


def golden_frames_0():
    import os
    from conftest import GOLDEN
    return np.load(os.path.join(GOLDEN, "net_frame0.npy"))


PATCH16_CASES = [
    # B, H, W, C, od1, od2: pool (2x2 s1) -> conv3x3 C->od1 -> conv3x3 od1->od2, both on the fp16
    # patch kernel (zero-bordered activations written by the pool and by the first conv)
    (64, 13, 13, 256, 512, 512),   # conv6-like at batch 64 (57 tiles of 192 rows)
    (3, 13, 13, 128, 256, 256),    # few rows: one partial tile per N panel
    (2, 9, 11, 64, 256, 512),      # non-square frame, 2 x 99 rows
]


@pytest.mark.parametrize("case", PATCH16_CASES)
def test_fp16_patch_conv_vs_oracle(monkeypatch, case):
    """conv3x3_f16_acc_kernel (input LDS-DMA'd once per 64-channel chunk for all 9 taps into
    row-skewed 160-B rows, weights straight to registers): whole chain within the fp16 layer
    tolerance of the fp32 oracle, both convs on mode patch16, and batch rows independent of the
    batch (row 0 alone == row 0 of the batch, bit for bit)."""
    B, H, W, C, od1, od2 = case
    rng = np.random.default_rng(B + C + od1)
    x = rng.standard_normal((B, H, W, C)).astype(np.float32)
    k1 = (rng.standard_normal((3, 3, C, od1)) * np.sqrt(2.0 / (9 * C))).astype(np.float32)
    k2 = (rng.standard_normal((3, 3, od1, od2)) * np.sqrt(2.0 / (9 * od1))).astype(np.float32)
    bn = lambda n: (rng.standard_normal(n).astype(np.float32) * 0.1, rng.uniform(0.5, 1.5, n).astype(np.float32),
                    rng.uniform(0.5, 1.5, n).astype(np.float32))
    b1, bn1 = rng.standard_normal(od1).astype(np.float32) * 0.1, bn(od1)
    b2, bn2 = rng.standard_normal(od2).astype(np.float32) * 0.1, bn(od2)

    def graph(shape):
        g = dnn_hip.DnnGraphBuilder()
        y = g.create_input(list(shape))
        y = g.create_max_pool2d(y, [1, 2, 2, 1], [1, 1, 1, 1], "SAME")
        for k, b, n in ((k1, b1, bn1), (k2, b2, bn2)):
            y = g.create_conv2d(y, k, [1, 1, 1, 1], "SAME")
            y = g.create_bias_add(y, b)
            y = g.create_batch_norm(y, *n, 1e-5)
            y = g.create_leaky_relu(y)
        g.set_out_node(y)
        return g

    monkeypatch.setenv("DNN_HIP_PATCH16", "1")
    eng = dnn_hip.DnnInferenceEngine(graph(x.shape), False, precision="fp16")
    assert eng.plan().describe().count("mode=patch16") == 2
    y = eng.run(x)
    assert np.array_equal(eng.run(x), y)  # run to run
    ref = R.max_pool2d(x, [1, 2, 2, 1], [1, 1, 1, 1], "SAME")
    for k, b, n in ((k1, b1, bn1), (k2, b2, bn2)):
        ref = R.leaky_relu(R.batch_norm(R.bias_add(R.conv2d(ref, k), b), *n, 1e-5))
    err = R.normwise_err(y, ref)
    print("fp16 patch", case, "err %.3g" % err)
    assert err < 2 * FP16_LAYER_TOL
    y0 = dnn_hip.DnnInferenceEngine(graph((1,) + x.shape[1:]), False, precision="fp16").run(x[:1])
    assert np.array_equal(y0, y[:1])
    assert np.array_equal(eng.run(x), y)


TILE16_CASES = [
    # B, H, W, C, od1, od2, tile16 layers: pool (2x2 s1) -> conv3x3 C->od1 + pool 2x2/s2 ->
    # conv3x3 od1->od2 + pool 2x2/s2, on the fp16 tile kernel where the frame allows it
    (4, 104, 104, 32, 64, 128, 2),   # conv2 -> conv3 shapes (8x52 then 4x52 tiles, zero-bordered hand-off)
    (3, 52, 52, 64, 128, 256, 2),    # conv3 -> conv4 shapes (4x52 then 8x26 tiles, 2 column groups)
    (2, 26, 26, 128, 256, 64, 1),    # conv4 shape (over patch16); its 13x13 pooled output feeds the implicit GEMM
    (2, 20, 36, 32, 64, 64, 2),      # ragged frames: edge tiles past the frame
    (2, 20, 18, 32, 64, 64, 1),      # ... then a 10x9 frame (odd: the implicit GEMM)
]


@pytest.mark.parametrize("case", TILE16_CASES)
def test_fp16_tile_conv_pool_vs_oracle(monkeypatch, case):
    """conv3x3_f16_tile_kernel (2-D tiles, 32-channel patches LDS-DMA'd as skewed 64-B rows,
    64-column waves, 2x2/s2 pool fused, persistent workgroups streaming (tile, chunk) pairs):
    whole chain within the fp16 layer tolerance of the fp32 oracle; batch rows independent of the
    batch (row 0 alone == row 0 of the batch, bit for bit); one tile per workgroup and one
    persistent workgroup per CU give the same bits as the default two."""
    B, H, W, C, od1, od2, ntile = case
    rng = np.random.default_rng(B + C + od1 + H)
    x = rng.standard_normal((B, H, W, C)).astype(np.float32)
    k1 = (rng.standard_normal((3, 3, C, od1)) * np.sqrt(2.0 / (9 * C))).astype(np.float32)
    k2 = (rng.standard_normal((3, 3, od1, od2)) * np.sqrt(2.0 / (9 * od1))).astype(np.float32)
    bn = lambda n: (rng.standard_normal(n).astype(np.float32) * 0.1, rng.uniform(0.5, 1.5, n).astype(np.float32),
                    rng.uniform(0.5, 1.5, n).astype(np.float32))
    b1, bn1 = rng.standard_normal(od1).astype(np.float32) * 0.1, bn(od1)
    b2, bn2 = rng.standard_normal(od2).astype(np.float32) * 0.1, bn(od2)

    def graph(shape):
        g = dnn_hip.DnnGraphBuilder()
        y = g.create_input(list(shape))
        y = g.create_max_pool2d(y, [1, 2, 2, 1], [1, 1, 1, 1], "SAME")
        for k, b, n in ((k1, b1, bn1), (k2, b2, bn2)):
            y = g.create_conv2d(y, k, [1, 1, 1, 1], "SAME")
            y = g.create_bias_add(y, b)
            y = g.create_batch_norm(y, *n, 1e-5)
            y = g.create_leaky_relu(y)
            y = g.create_max_pool2d(y, [1, 2, 2, 1], [1, 2, 2, 1], "SAME")
        g.set_out_node(y)
        return g

    monkeypatch.delenv("DNN_HIP_TILE16_WGS", raising=False)
    eng = dnn_hip.DnnInferenceEngine(graph(x.shape), False, precision="fp16")
    assert eng.plan().describe().count("mode=tile16") == ntile, eng.plan().describe()
    y = eng.run(x)
    assert np.array_equal(eng.run(x), y)  # run to run
    ref = R.max_pool2d(x, [1, 2, 2, 1], [1, 1, 1, 1], "SAME")
    for k, b, n in ((k1, b1, bn1), (k2, b2, bn2)):
        ref = R.leaky_relu(R.batch_norm(R.bias_add(R.conv2d(ref, k), b), *n, 1e-5))
        ref = R.max_pool2d(ref, [1, 2, 2, 1], [1, 2, 2, 1], "SAME")
    err = R.normwise_err(y, ref)
    print("fp16 tile", case, "err %.3g" % err)
    assert err < 2 * FP16_LAYER_TOL
    y0 = dnn_hip.DnnInferenceEngine(graph((1,) + x.shape[1:]), False, precision="fp16").run(x[:1])
    assert np.array_equal(y0, y[:1])
    for wgs in ("0", "1"):  # read when the plan is created: one engine per arm
        monkeypatch.setenv("DNN_HIP_TILE16_WGS", wgs)
        assert np.array_equal(dnn_hip.DnnInferenceEngine(graph(x.shape), False, precision="fp16").run(x), y), wgs


IMG16_CASES = [
    # B, C, od1, od2: 13x13 frames: pool (2x2 s1) -> conv3x3 C->od1 + pool 2x2/s1 SAME (the tile
    # kernel's whole-frame form) -> conv3x3 od1->od2 (patch16: the zero-bordered hand-off)
    (64, 256, 512, 256),   # conv5 + pool5 -> conv6 shapes at batch 64 (8 column groups)
    (3, 64, 192, 256),     # 3 column groups, few frames
    (1, 32, 64, 64),       # one frame; od2 = 64: the implicit GEMM reads a plain output
    (64, 256, 512, 1024),  # a 1024-wide consumer at batch 64 (the shape of round 5's run-to-run finding)
]


@pytest.mark.parametrize("case", IMG16_CASES)
def test_fp16_img_conv_pool1_vs_oracle(monkeypatch, case):
    """conv3x3_f16_tile_kernel MODE 1 (whole 13x13 frame per tile, raster rows in skewed 96-B
    LDS rows, epilogue staged in fp16 for the frame, the 2x2/s1 SAME pool taken from the stage):
    chain within the fp16 tolerance of the fp32 oracle; batch rows independent of the batch;
    the same bits with one frame per workgroup (DNN_HIP_TILE16_WGS=0)."""
    B, C, od1, od2 = case
    H = W = 13
    rng = np.random.default_rng(B + C + od1)
    x = rng.standard_normal((B, H, W, C)).astype(np.float32)
    k1 = (rng.standard_normal((3, 3, C, od1)) * np.sqrt(2.0 / (9 * C))).astype(np.float32)
    k2 = (rng.standard_normal((3, 3, od1, od2)) * np.sqrt(2.0 / (9 * od1))).astype(np.float32)
    bn = lambda n: (rng.standard_normal(n).astype(np.float32) * 0.1, rng.uniform(0.5, 1.5, n).astype(np.float32),
                    rng.uniform(0.5, 1.5, n).astype(np.float32))
    b1, bn1 = rng.standard_normal(od1).astype(np.float32) * 0.1, bn(od1)
    b2, bn2 = rng.standard_normal(od2).astype(np.float32) * 0.1, bn(od2)

    def graph(shape):
        g = dnn_hip.DnnGraphBuilder()
        y = g.create_input(list(shape))
        y = g.create_max_pool2d(y, [1, 2, 2, 1], [1, 1, 1, 1], "SAME")
        for i, (k, b, n) in enumerate(((k1, b1, bn1), (k2, b2, bn2))):
            y = g.create_conv2d(y, k, [1, 1, 1, 1], "SAME")
            y = g.create_bias_add(y, b)
            y = g.create_batch_norm(y, *n, 1e-5)
            y = g.create_leaky_relu(y)
            if i == 0:
                y = g.create_max_pool2d(y, [1, 2, 2, 1], [1, 1, 1, 1], "SAME")
        g.set_out_node(y)
        return g

    monkeypatch.delenv("DNN_HIP_TILE16_WGS", raising=False)
    eng = dnn_hip.DnnInferenceEngine(graph(x.shape), False, precision="fp16")
    d = eng.plan().describe()
    assert d.count("mode=tile16") == 1 and "+pool2x2s1" in d, d
    assert ("mode=patch16" in d) == (od2 % 256 == 0), d
    y = eng.run(x)
    assert np.array_equal(eng.run(x), y)  # run to run
    ref = R.max_pool2d(x, [1, 2, 2, 1], [1, 1, 1, 1], "SAME")
    for i, (k, b, n) in enumerate(((k1, b1, bn1), (k2, b2, bn2))):
        ref = R.leaky_relu(R.batch_norm(R.bias_add(R.conv2d(ref, k), b), *n, 1e-5))
        if i == 0:
            ref = R.max_pool2d(ref, [1, 2, 2, 1], [1, 1, 1, 1], "SAME")
    err = R.normwise_err(y, ref)
    print("fp16 img", case, "err %.3g" % err)
    assert err < 2 * FP16_LAYER_TOL
    y0 = dnn_hip.DnnInferenceEngine(graph((1,) + x.shape[1:]), False, precision="fp16").run(x[:1])
    assert np.array_equal(y0, y[:1])
    monkeypatch.setenv("DNN_HIP_TILE16_WGS", "0")  # read when the plan is created: an engine of its own
    assert np.array_equal(dnn_hip.DnnInferenceEngine(graph(x.shape), False, precision="fp16").run(x), y)


X3_CASES = [
    # B, H, W, C, od1, od2: pool (2x2 s1) -> conv3x3 C->od1 -> conv3x3 od1->od2, both on the fp32
    # x3 conv (exact 3-way bf16 splits; split planes written by the pool and by the first conv)
    (64, 13, 13, 512, 1024, 256),  # conv6-like at batch 64 (62 tiles of 176 rows), K = 4608 / 9216
    (3, 13, 13, 128, 256, 256),    # few rows: one partial tile per N panel
    (2, 9, 11, 32, 256, 512),      # non-square frame, one 32-channel chunk
]


@pytest.mark.parametrize("case", X3_CASES)
def test_x3_conv_vs_oracle(monkeypatch, case):
    """conv3x3_x3_patch_kernel: fp32 operands split exactly into three bf16 pieces, six bf16 MFMA
    products into an fp32 accumulator.  Each layer within the fp32 LAYER_TOL of the float64
    oracle (the x3 chain and the fp32-MFMA chain, DNN_HIP_X3=0, are held to the same bar, and the
    x3 error is at most 1.25x the fp32 path's), both convs on mode patch_x3, batch rows
    independent of the batch (bit for bit), repeat runs identical."""
    B, H, W, C, od1, od2 = case
    rng = np.random.default_rng(B + C + od1 + 7)
    x = rng.standard_normal((B, H, W, C)).astype(np.float32)
    k1 = (rng.standard_normal((3, 3, C, od1)) * np.sqrt(2.0 / (9 * C))).astype(np.float32)
    k2 = (rng.standard_normal((3, 3, od1, od2)) * np.sqrt(2.0 / (9 * od1))).astype(np.float32)
    bn = lambda n: (rng.standard_normal(n).astype(np.float32) * 0.1, rng.uniform(0.5, 1.5, n).astype(np.float32),
                    rng.uniform(0.5, 1.5, n).astype(np.float32))
    b1, bn1 = rng.standard_normal(od1).astype(np.float32) * 0.1, bn(od1)
    b2, bn2 = rng.standard_normal(od2).astype(np.float32) * 0.1, bn(od2)

    def graph(shape, layers):
        g = dnn_hip.DnnGraphBuilder()
        y = g.create_input(list(shape))
        y = g.create_max_pool2d(y, [1, 2, 2, 1], [1, 1, 1, 1], "SAME")
        for k, b, n in layers:
            y = g.create_conv2d(y, k, [1, 1, 1, 1], "SAME")
            y = g.create_bias_add(y, b)
            y = g.create_batch_norm(y, *n, 1e-5)
            y = g.create_leaky_relu(y)
        g.set_out_node(y)
        return g

    L = [(k1, b1, bn1), (k2, b2, bn2)]
    pooled = R.max_pool2d(x, [1, 2, 2, 1], [1, 1, 1, 1], "SAME")
    ref1 = R.leaky_relu(R.batch_norm(R.bias_add(R.conv2d(pooled, k1), b1), *bn1, 1e-5))
    ref2 = R.leaky_relu(R.batch_norm(R.bias_add(R.conv2d(ref1, k2), b2), *bn2, 1e-5))
    errs = {}
    for x3 in ("1", "0"):
        monkeypatch.setenv("DNN_HIP_X3", x3)
        e1 = dnn_hip.DnnInferenceEngine(graph(x.shape, L[:1]), False)
        e2 = dnn_hip.DnnInferenceEngine(graph(x.shape, L), False)
        assert e2.plan().describe().count("mode=patch_x3") == (2 if x3 == "1" else 0)
        y1, y2 = e1.run(x), e2.run(x)
        errs[x3] = (R.normwise_err(y1, ref1), R.normwise_err(y2, ref2))
        print("x3=%s layer/chain normwise err %.3e %.3e" % (x3, errs[x3][0], errs[x3][1]))
        if x3 == "1":
            y0 = dnn_hip.DnnInferenceEngine(graph((1,) + x.shape[1:], L), False).run(x[:1])
            assert np.array_equal(y0, y2[:1])
            assert np.array_equal(e2.run(x), y2)
    for x3 in ("0", "1"):
        assert errs[x3][0] < LAYER_TOL and errs[x3][1] < 2 * LAYER_TOL, (x3, errs)
    # measured: the x3 layer error is 0.4-0.95x the fp32 path's (its accumulator sees two
    # roundings per 32-channel step, the fp32 MFMA chain one per 2 channels)
    assert errs["1"][0] <= 1.25 * errs["0"][0] and errs["1"][1] <= 1.25 * errs["0"][1], errs


X3_1X1_CASES = [
    # B, H, W, C, od1, N: pool (2x2 s1) -> conv3x3 C->od1 (x3, writing split planes) -> conv1x1
    # od1->N + bias (the 1x1 x3 conv: YOLOv2-tiny's conv8 is 1024->125 on 13x13)
    (64, 13, 13, 256, 1024, 125),  # conv8's shape at batch 64 (338 row tiles, ragged N panel)
    (3, 9, 11, 64, 256, 200),      # non-square frame, two N panels (the second ragged), few rows
]


@pytest.mark.parametrize("case", X3_1X1_CASES)
def test_x3_1x1_conv_vs_oracle(monkeypatch, case):
    """conv1x1_x3_kernel (MODE_X3_1X1): the 1x1 conv after an x3 conv reads that producer's
    split planes and runs the x3 arithmetic (two accumulators, six bf16 products per step).
    Within the fp32 LAYER_TOL of the float64 oracle and at most 1.25x the fp32-MFMA plan's error
    (DNN_HIP_X3=0: the same layers on the fp32 MFMA), batch rows bit-equal to batch-1 runs,
    repeat runs identical, and the mode as planned (DNN_HIP_X3_1X1=0 keeps the fp32 GEMM)."""
    B, H, W, C, od1, N = case
    rng = np.random.default_rng(B + C + N)
    x = rng.standard_normal((B, H, W, C)).astype(np.float32)
    k1 = (rng.standard_normal((3, 3, C, od1)) * np.sqrt(2.0 / (9 * C))).astype(np.float32)
    k2 = (rng.standard_normal((1, 1, od1, N)) * np.sqrt(2.0 / od1)).astype(np.float32)
    b1 = rng.standard_normal(od1).astype(np.float32) * 0.1
    bn1 = (rng.standard_normal(od1).astype(np.float32) * 0.1, rng.uniform(0.5, 1.5, od1).astype(np.float32),
           rng.uniform(0.5, 1.5, od1).astype(np.float32))
    b2 = rng.standard_normal(N).astype(np.float32) * 0.1

    def graph(shape):
        g = dnn_hip.DnnGraphBuilder()
        y = g.create_input(list(shape))
        y = g.create_max_pool2d(y, [1, 2, 2, 1], [1, 1, 1, 1], "SAME")
        y = g.create_conv2d(y, k1, [1, 1, 1, 1], "SAME")
        y = g.create_bias_add(y, b1)
        y = g.create_batch_norm(y, *bn1, 1e-5)
        y = g.create_leaky_relu(y)
        y = g.create_conv2d(y, k2, [1, 1, 1, 1], "SAME")
        y = g.create_bias_add(y, b2)
        g.set_out_node(y)
        return g

    pooled = R.max_pool2d(x, [1, 2, 2, 1], [1, 1, 1, 1], "SAME")
    ref1 = R.leaky_relu(R.batch_norm(R.bias_add(R.conv2d(pooled, k1), b1), *bn1, 1e-5))
    ref = R.bias_add(R.conv2d(ref1, k2), b2)
    errs = {}
    for x3, x1 in (("1", "1"), ("0", "1"), ("1", "0")):
        monkeypatch.setenv("DNN_HIP_X3", x3)
        monkeypatch.setenv("DNN_HIP_X3_1X1", x1)
        eng = dnn_hip.DnnInferenceEngine(graph(x.shape), False)
        desc = eng.plan().describe()
        assert desc.count("mode=x3_1x1") == (1 if x3 == "1" and x1 == "1" else 0), desc
        y = eng.run(x)
        errs[x3 + x1] = R.normwise_err(y, ref)
        print("x3=%s 1x1=%s normwise err %.3e" % (x3, x1, errs[x3 + x1]))
        if x3 == "1" and x1 == "1":
            y0 = dnn_hip.DnnInferenceEngine(graph((1,) + x.shape[1:]), False).run(x[:1])
            assert np.array_equal(y0, y[:1])
            assert np.array_equal(eng.run(x), y)
    for k, e in errs.items():
        assert e < 2 * LAYER_TOL, (k, errs)
    assert errs["11"] <= 1.25 * errs["01"], errs


X3_IMG_CASES = [
    # B, last: pool 2x2 s1 -> conv3x3 256->512 + pool 2x2 s1 SAME (whole-image x3 tiles, 13x13) ->
    # conv3x3 512->256 (x3 consumer of its split planes), or with the pool-fused conv the last layer
    # (fp32 output)
    (5, False), (3, True), (1, False),
]


@pytest.mark.parametrize("case", X3_IMG_CASES)
def test_x3_img_conv_pool_vs_oracle(monkeypatch, case):
    """conv3x3_x3_img_kernel (batch plans' conv5 + pool5: one 13x13 image x 128 columns per
    workgroup over all of K, the stride-1 pool on the image's raw sums in LDS before the epilogue,
    split planes or fp32 out): mode as planned, within the fp32 tolerance of the float64 oracle and
    within 1.25x of the fp32-MFMA plan's error (DNN_HIP_X3=0), negative-gamma channels (the window's
    minimum), batch rows bit-equal to one-frame runs, repeat runs identical; the K-slice form
    (DNN_HIP_X3_IMG=0) within the same tolerance."""
    B, last = case
    rng = np.random.default_rng(B * 13 + int(last))
    x = rng.standard_normal((B, 13, 13, 256)).astype(np.float32)

    def layer(c, od):
        k = (rng.standard_normal((3, 3, c, od)) * np.sqrt(2.0 / (9 * c))).astype(np.float32)
        b = rng.standard_normal(od).astype(np.float32) * 0.1
        gam = rng.uniform(0.5, 1.5, od).astype(np.float32)
        gam[::5] *= -1
        return k, b, (rng.standard_normal(od).astype(np.float32) * 0.1, rng.uniform(0.5, 1.5, od).astype(np.float32),
                      gam)

    L = [layer(256, 512)] + ([] if last else [layer(512, 256)])

    def graph(shape):
        g = dnn_hip.DnnGraphBuilder()
        y = g.create_input(list(shape))
        y = g.create_max_pool2d(y, [1, 2, 2, 1], [1, 1, 1, 1], "SAME")  # (an x3 producer)
        for j, (k, b, n) in enumerate(L):
            y = g.create_conv2d(y, k, [1, 1, 1, 1], "SAME")
            y = g.create_bias_add(y, b)
            y = g.create_batch_norm(y, *n, 1e-5)
            y = g.create_leaky_relu(y)
            if j == 0:
                y = g.create_max_pool2d(y, [1, 2, 2, 1], [1, 1, 1, 1], "SAME")
        g.set_out_node(y)
        return g

    ref = R.max_pool2d(x, [1, 2, 2, 1], [1, 1, 1, 1], "SAME")
    for j, (k, b, n) in enumerate(L):
        ref = R.leaky_relu(R.batch_norm(R.bias_add(R.conv2d(ref, k), b), *n, 1e-5))
        if j == 0:
            ref = R.max_pool2d(ref, [1, 2, 2, 1], [1, 1, 1, 1], "SAME")
    errs = {}
    for arm in ("img", "slices", "fp32"):
        monkeypatch.setenv("DNN_HIP_X3", "0" if arm == "fp32" else "1")
        monkeypatch.setenv("DNN_HIP_X3_IMG", "0" if arm == "slices" else "1")
        eng = dnn_hip.DnnInferenceEngine(graph(x.shape), False)
        conv = [ln for ln in eng.plan().describe().splitlines() if ln.startswith("conv")]
        if arm == "img":
            assert "mode=x3_img" in conv[0] and "+pool2x2s1" in conv[0], conv
        y = eng.run(x)
        errs[arm] = R.normwise_err(y, ref)
        if arm == "img":
            assert np.array_equal(eng.run(x), y)
            for f in range(B):
                one = dnn_hip.DnnInferenceEngine(graph((1,) + x.shape[1:]), False).run(x[f:f + 1])
                assert np.array_equal(one, y[f:f + 1]), f
    print("x3 img errs", errs)
    assert all(e < 3 * LAYER_TOL for e in errs.values()), errs
    assert errs["img"] <= 1.25 * errs["fp32"], errs


X3_CHAIN_CASES = [
    # B, H, W, C0: conv3x3 C0->128 + pool 2x2 s2 (fp32 implicit GEMM writing the x3 split planes)
    # -> conv3x3 128->512 (x3, 2 K slices) -> then "pool" (2x2 s1: pool5's combine) or "conv"
    # (a standalone combine kernel) -> conv3x3 ->256 (x3)
    (8, 26, 26, 64, "pool"),
    (3, 26, 26, 32, "conv"),
]


@pytest.mark.parametrize("case", X3_CHAIN_CASES)
def test_x3_split_combine_and_producer_vs_oracle(monkeypatch, case):
    """The x3 conv's K slices (conv5's rule: N = 512 -> 2 slices of raw partials) combined in
    split order by the next pool (sum, epilogue, pool in the reference's order) or by a
    standalone combine kernel, and a pool-fused fp32 implicit GEMM storing its epilogue as
    x3 split planes (EPI_OUT_X3).  Every layer mode as planned, the chain within the fp32
    tolerance of the float64 oracle and within 1.25x of the fp32-MFMA plan's error
    (DNN_HIP_X3=0), batch rows bit-equal to batch-1 runs; negative-gamma channels throughout."""
    B, H, W, C0, mid = case
    monkeypatch.setenv("DNN_HIP_X3_IMG", "0")  # (the K-slice form; whole-image tiles: test_x3_img_*)
    rng = np.random.default_rng(B * 7 + C0)
    x = rng.standard_normal((B, H, W, C0)).astype(np.float32)

    def layer(c, od):
        k = (rng.standard_normal((3, 3, c, od)) * np.sqrt(2.0 / (9 * c))).astype(np.float32)
        b = rng.standard_normal(od).astype(np.float32) * 0.1
        # every 5th channel with a negative gamma: a decreasing epilogue, so the pools before the
        # epilogue (conv0's EPI_OUT_X3 store, pool5's combine) must take the window's minimum
        gam = rng.uniform(0.5, 1.5, od).astype(np.float32)
        gam[::5] *= -1
        n = (rng.standard_normal(od).astype(np.float32) * 0.1, rng.uniform(0.5, 1.5, od).astype(np.float32), gam)
        return k, b, n

    L0, L1, L2 = layer(C0, 128), layer(128, 512), layer(512, 256)

    def graph(shape):
        g = dnn_hip.DnnGraphBuilder()
        y = g.create_input(list(shape))
        for idx, (k, b, n) in enumerate((L0, L1, L2)):
            y = g.create_conv2d(y, k, [1, 1, 1, 1], "SAME")
            y = g.create_bias_add(y, b)
            y = g.create_batch_norm(y, *n, 1e-5)
            y = g.create_leaky_relu(y)
            if idx == 0:
                y = g.create_max_pool2d(y, [1, 2, 2, 1], [1, 2, 2, 1], "SAME")
            if idx == 1 and mid == "pool":
                y = g.create_max_pool2d(y, [1, 2, 2, 1], [1, 1, 1, 1], "SAME")
        g.set_out_node(y)
        return g

    ref = x
    for idx, (k, b, n) in enumerate((L0, L1, L2)):
        ref = R.leaky_relu(R.batch_norm(R.bias_add(R.conv2d(ref, k), b), *n, 1e-5))
        if idx == 0:
            ref = R.max_pool2d(ref, [1, 2, 2, 1], [1, 2, 2, 1], "SAME")
        if idx == 1 and mid == "pool":
            ref = R.max_pool2d(ref, [1, 2, 2, 1], [1, 1, 1, 1], "SAME")
    errs = {}
    for x3 in ("1", "0"):
        monkeypatch.setenv("DNN_HIP_X3", x3)
        eng = dnn_hip.DnnInferenceEngine(graph(x.shape), False)
        desc = eng.plan().describe()
        if x3 == "1":
            conv = [ln for ln in desc.splitlines() if ln.startswith("conv")]
            assert "mode=implicit" in conv[0] and "+pool2x2s2" in conv[0]
            assert "mode=patch_x3" in conv[1] and "splitK=2 x3-combine" in conv[1] and "mode=patch_x3" in conv[2]
            names = [k["name"] for k in eng.plan().kernels()]
            assert ("conv1.combine" in names) == (mid == "conv")
        y = eng.run(x)
        errs[x3] = R.normwise_err(y, ref)
        print("x3=%s chain normwise err %.3e" % (x3, errs[x3]))
        if x3 == "1":
            y0 = dnn_hip.DnnInferenceEngine(graph((1,) + x.shape[1:]), False).run(x[:1])
            assert np.array_equal(y0, y[:1])
    assert errs["1"] < 3 * LAYER_TOL and errs["0"] < 3 * LAYER_TOL, errs
    assert errs["1"] <= 1.25 * errs["0"], errs


X3_POOL_CASES = [
    # B, H, W, C: pool (2x2 s1) -> conv3x3 C->256 + pool 2x2 s2 fused into the x3 conv (rows
    # pool-window-major) -> conv3x3 256->512 + pool 2x2 s1 (13x13: whole-image x3 tiles with the
    # pool fused; else x3 in 2 K slices + the pool's combine)
    (8, 26, 26, 128),   # conv4-like
    (3, 13, 13, 64),    # odd: ragged windows (cells past the edge repeat cell (0, 0))
]


@pytest.mark.parametrize("case", X3_POOL_CASES)
def test_x3_pool_fused_vs_oracle(monkeypatch, case):
    """x3 conv with its 2x2/s2 pool fused (pooled before the epilogue, written as the next x3
    layer's split planes): modes as planned, chain within the fp32 tolerance of the float64
    oracle and within 1.25x of the fp32-MFMA plan's error, negative-gamma channels, batch rows
    bit-equal to batch-1 runs."""
    B, H, W, C = case
    rng = np.random.default_rng(B * 13 + C)
    x = rng.standard_normal((B, H, W, C)).astype(np.float32)

    def layer(c, od):
        k = (rng.standard_normal((3, 3, c, od)) * np.sqrt(2.0 / (9 * c))).astype(np.float32)
        b = rng.standard_normal(od).astype(np.float32) * 0.1
        gam = rng.uniform(0.5, 1.5, od).astype(np.float32)
        gam[::5] *= -1
        return k, b, (rng.standard_normal(od).astype(np.float32) * 0.1, rng.uniform(0.5, 1.5, od).astype(np.float32),
                      gam)

    L1, L2 = layer(C, 256), layer(256, 512)

    def graph(shape):
        g = dnn_hip.DnnGraphBuilder()
        y = g.create_input(list(shape))
        y = g.create_max_pool2d(y, [1, 2, 2, 1], [1, 1, 1, 1], "SAME")
        for idx, (k, b, n) in enumerate((L1, L2)):
            y = g.create_conv2d(y, k, [1, 1, 1, 1], "SAME")
            y = g.create_bias_add(y, b)
            y = g.create_batch_norm(y, *n, 1e-5)
            y = g.create_leaky_relu(y)
            y = g.create_max_pool2d(y, [1, 2, 2, 1], [1, 2, 2, 1] if idx == 0 else [1, 1, 1, 1], "SAME")
        g.set_out_node(y)
        return g

    ref = R.max_pool2d(x, [1, 2, 2, 1], [1, 1, 1, 1], "SAME")
    for idx, (k, b, n) in enumerate((L1, L2)):
        ref = R.leaky_relu(R.batch_norm(R.bias_add(R.conv2d(ref, k), b), *n, 1e-5))
        ref = R.max_pool2d(ref, [1, 2, 2, 1], [1, 2, 2, 1] if idx == 0 else [1, 1, 1, 1], "SAME")
    errs = {}
    for x3 in ("1", "0"):
        monkeypatch.setenv("DNN_HIP_X3", x3)
        eng = dnn_hip.DnnInferenceEngine(graph(x.shape), False)
        if x3 == "1":
            conv = [ln for ln in eng.plan().describe().splitlines() if ln.startswith("conv")]
            assert "mode=patch_x3" in conv[0] and "+pool2x2s2" in conv[0], conv
            if H // 2 == 13:  # 13x13 frames: whole-image tiles with the stride-1 pool fused
                assert "mode=x3_img" in conv[1] and "+pool2x2s1" in conv[1], conv
            else:
                assert "mode=patch_x3" in conv[1] and "splitK=2 x3-combine" in conv[1], conv
        y = eng.run(x)
        errs[x3] = R.normwise_err(y, ref)
        print("x3=%s pool-fused chain normwise err %.3e" % (x3, errs[x3]))
        if x3 == "1":
            y0 = dnn_hip.DnnInferenceEngine(graph((1,) + x.shape[1:]), False).run(x[:1])
            assert np.array_equal(y0, y[:1])
    assert errs["1"] < 3 * LAYER_TOL and errs["0"] < 3 * LAYER_TOL, errs
    assert errs["1"] <= 1.25 * errs["0"], errs


X3_TILE_CASES = [
    # B, H, W, form.  "pool": conv3x3 16->32 + pool 2x2 s2 (pool-fused patch conv, conv1-like,
    # writing split planes) -> 32->64 + pool (tile kernel, 4 waves) -> 64->128 + pool (tile kernel,
    # 8 waves; fused when the frame is even) -> 128->256 (row-run x3 kernel).  "raster": pool 2x2 s1
    # -> 32->64 -> 64->128, no pools (raster tile rows; ragged tiles in both directions)
    (3, 104, 104, "pool"),  # conv2/conv3-like frames: 52 / 26 wide, whole 8 x 26 / 4 x 26 tiles
    (2, 60, 60, "pool"),    # 30 wide: one partial tile per row band; 15x15 after: separate pool
    (2, 27, 61, "raster"),
    (2, 104, 104, "c16"),      # conv1-like: 16-channel x3 conv (fp32 input split while staged) + pool
    (2, 37, 45, "c16raster"),  # ... without a pool: raster rows, ragged tiles
]


@pytest.mark.parametrize("case", X3_TILE_CASES)
def test_x3_tile_kernel_vs_oracle(monkeypatch, case):
    """conv3x3_x3_tile2_kernel (N = 64 / 128 on 2-D 8 x 26 / 4 x 26 output tiles),
    conv3x3_x3_c16_kernel (16 input channels, two taps per 32-wide K step) and the patch conv's
    split-plane epilogue: modes as planned, the chain within the fp32 tolerance of the float64
    oracle and within 1.25x of the fp32-MFMA plan's error (DNN_HIP_X3=0), negative-gamma
    channels, batch rows bit-equal to batch-1 runs, repeat runs identical."""
    B, H, W, form = case
    rng = np.random.default_rng(B * 31 + H + W)

    def layer(c, od):
        k = (rng.standard_normal((3, 3, c, od)) * np.sqrt(2.0 / (9 * c))).astype(np.float32)
        b = rng.standard_normal(od).astype(np.float32) * 0.1
        gam = rng.uniform(0.5, 1.5, od).astype(np.float32)
        gam[::5] *= -1
        return k, b, (rng.standard_normal(od).astype(np.float32) * 0.1, rng.uniform(0.5, 1.5, od).astype(np.float32),
                      gam)

    if form == "pool":
        x = rng.standard_normal((B, H, W, 16)).astype(np.float32)
        layers = [(layer(16, 32), True), (layer(32, 64), True), (layer(64, 128), True), (layer(128, 256), False)]
    elif form == "c16":
        x = rng.standard_normal((B, H, W, 16)).astype(np.float32)
        layers = [(layer(16, 32), True), (layer(32, 64), True), (layer(64, 128), False)]
    elif form == "c16raster":
        x = rng.standard_normal((B, H, W, 16)).astype(np.float32)
        layers = [(layer(16, 32), False), (layer(32, 64), False)]
    else:
        x = rng.standard_normal((B, H, W, 32)).astype(np.float32)
        layers = [(layer(32, 64), False), (layer(64, 128), False)]

    def graph(shape):
        g = dnn_hip.DnnGraphBuilder()
        y = g.create_input(list(shape))
        if form != "pool":  # (a producer before the first conv: conv1 is never a plan's first layer)
            y = g.create_max_pool2d(y, [1, 2, 2, 1], [1, 1, 1, 1], "SAME")
        for (k, b, n), pool in layers:
            y = g.create_conv2d(y, k, [1, 1, 1, 1], "SAME")
            y = g.create_bias_add(y, b)
            y = g.create_batch_norm(y, *n, 1e-5)
            y = g.create_leaky_relu(y)
            if pool:
                y = g.create_max_pool2d(y, [1, 2, 2, 1], [1, 2, 2, 1], "SAME")
        g.set_out_node(y)
        return g

    ref = R.max_pool2d(x, [1, 2, 2, 1], [1, 1, 1, 1], "SAME") if form != "pool" else x
    for (k, b, n), pool in layers:
        ref = R.leaky_relu(R.batch_norm(R.bias_add(R.conv2d(ref, k), b), *n, 1e-5))
        if pool:
            ref = R.max_pool2d(ref, [1, 2, 2, 1], [1, 2, 2, 1], "SAME")
    errs = {}
    for x3 in ("1", "0"):
        monkeypatch.setenv("DNN_HIP_X3", x3)
        eng = dnn_hip.DnnInferenceEngine(graph(x.shape), False)
        if x3 == "1":
            conv = [ln for ln in eng.plan().describe().splitlines() if ln.startswith("conv")]
            if form == "pool":
                assert "mode=patch" in conv[0] and "+pool2x2s2" in conv[0], conv
                assert all("mode=patch_x3" in c for c in conv[1:]), conv
                assert "+pool2x2s2" in conv[1] and ("+pool2x2s2" in conv[2]) == (H % 8 == 0), conv
            else:
                assert all("mode=patch_x3" in c for c in conv), conv
                if form == "c16":
                    assert "+pool2x2s2" in conv[0] and "+pool2x2s2" in conv[1], conv
        y = eng.run(x)
        errs[x3] = R.normwise_err(y, ref)
        print("x3=%s tile chain normwise err %.3e" % (x3, errs[x3]))
        if x3 == "1":
            y0 = dnn_hip.DnnInferenceEngine(graph((1,) + x.shape[1:]), False).run(x[:1])
            assert np.array_equal(y0, y[:1])
            assert np.array_equal(eng.run(x), y)
            if form == "c16":  # latency plans: the 16-channel kernel's 4 x 26 tiles
                el = dnn_hip.DnnInferenceEngine(graph(x.shape), False, latency=True)
                lconv = [ln for ln in el.plan().describe().splitlines() if ln.startswith("conv")]
                assert "mode=patch_x3" in lconv[0] and "latency" in lconv[0], lconv
                yl = el.run(x)
                assert np.array_equal(el.run(x), yl)
                errs["lat"] = R.normwise_err(yl, ref)
    assert errs["1"] < 3 * LAYER_TOL and errs["0"] < 3 * LAYER_TOL, errs
    assert errs["1"] <= 1.25 * errs["0"] and errs.get("lat", 0.0) <= 1.25 * errs["0"], errs


def test_x3_c16_pooled_plain_output_vs_oracle(monkeypatch):
    """A pooled 16-channel x3 conv whose output is the plan's plain fp32 output (nothing after its
    pool: the unstaged pooled epilogue with out_mode 0), tiles ragged in both directions against
    16 x 26: the persistent kernel (batch plan), the one-tile kernel (DNN_HIP_X3_C16P=0) and the
    latency plan's 4 x 26 tiles.  Each arm within the fp32 tolerance of the float64 oracle and
    within 1.25x of the fp32-MFMA plan's error (DNN_HIP_X3=0), negative-gamma channels, repeat runs
    identical.  (The arms are not bit-equal to each other: the K = 16 step sums differently.)"""
    B, H, W = 2, 36, 44
    rng = np.random.default_rng(B * 31 + H + W)
    x = rng.standard_normal((B, H, W, 16)).astype(np.float32)
    k = (rng.standard_normal((3, 3, 16, 32)) * np.sqrt(2.0 / (9 * 16))).astype(np.float32)
    b = rng.standard_normal(32).astype(np.float32) * 0.1
    gam = rng.uniform(0.5, 1.5, 32).astype(np.float32)
    gam[::5] *= -1
    n = (rng.standard_normal(32).astype(np.float32) * 0.1, rng.uniform(0.5, 1.5, 32).astype(np.float32), gam)

    def graph():
        g = dnn_hip.DnnGraphBuilder()
        y = g.create_input([B, H, W, 16])
        y = g.create_max_pool2d(y, [1, 2, 2, 1], [1, 1, 1, 1], "SAME")  # (conv1 is never a plan's first layer)
        y = g.create_conv2d(y, k, [1, 1, 1, 1], "SAME")
        y = g.create_bias_add(y, b)
        y = g.create_batch_norm(y, *n, 1e-5)
        y = g.create_leaky_relu(y)
        y = g.create_max_pool2d(y, [1, 2, 2, 1], [1, 2, 2, 1], "SAME")
        g.set_out_node(y)
        return g

    ref = R.max_pool2d(x, [1, 2, 2, 1], [1, 1, 1, 1], "SAME")
    ref = R.leaky_relu(R.batch_norm(R.bias_add(R.conv2d(ref, k), b), *n, 1e-5))
    ref = R.max_pool2d(ref, [1, 2, 2, 1], [1, 2, 2, 1], "SAME")

    def run(latency):
        eng = dnn_hip.DnnInferenceEngine(graph(), False, latency=latency)
        conv = [ln for ln in eng.plan().describe().splitlines() if ln.startswith("conv")]
        y = eng.run(x)
        assert np.array_equal(eng.run(x), y)
        return conv, R.normwise_err(y, ref)

    monkeypatch.setenv("DNN_HIP_X3", "0")
    _, e0 = run(False)
    monkeypatch.setenv("DNN_HIP_X3", "1")
    errs = {}
    conv, errs["c16p"] = run(False)
    assert len(conv) == 1 and "mode=patch_x3" in conv[0] and "+pool2x2s2" in conv[0] and "latency" not in conv[0], conv
    monkeypatch.setenv("DNN_HIP_X3_C16P", "0")
    _, errs["c16"] = run(False)
    monkeypatch.delenv("DNN_HIP_X3_C16P")
    conv, errs["lat"] = run(True)
    assert "mode=patch_x3" in conv[0] and "+pool2x2s2" in conv[0] and "latency" in conv[0], conv
    print("c16 pooled plain output: normwise err", errs, "fp32 MFMA %.3e" % e0)
    assert e0 < 3 * LAYER_TOL, e0
    for arm, e in errs.items():
        assert e < 3 * LAYER_TOL and e <= 1.25 * e0, (arm, errs, e0)


def test_engine_keeps_the_kernel_it_was_built_with(monkeypatch):
    """A plan reads its switches once, at creation: on the graph and input of
    test_x3_c16_pooled_plain_output_vs_oracle, an engine built under the default environment (the
    persistent 16-channel kernel), one built under DNN_HIP_X3_C16P=0 (one tile per workgroup) and
    one built under DNN_HIP_X3=0 (the fp32 MFMA) all stay alive, and each gives byte-equal outputs
    with DNN_HIP_X3_C16P unset, 0 and 1 and with DNN_HIP_X3 unset and 0.
    Measured on an MI355X, this commit and its parent alike: the first two engines' outputs are
    byte-equal at this shape (0 of 25,344 elements differ at this seed and at seeds 0..47), so
    they cannot show which kernel ran; the third engine's output differs from the first's, which
    is what keeps the test from passing vacuously."""
    B, H, W = 2, 36, 44
    rng = np.random.default_rng(B * 31 + H + W)
    x = rng.standard_normal((B, H, W, 16)).astype(np.float32)
    k = (rng.standard_normal((3, 3, 16, 32)) * np.sqrt(2.0 / (9 * 16))).astype(np.float32)
    b = rng.standard_normal(32).astype(np.float32) * 0.1
    gam = rng.uniform(0.5, 1.5, 32).astype(np.float32)
    gam[::5] *= -1
    n = (rng.standard_normal(32).astype(np.float32) * 0.1, rng.uniform(0.5, 1.5, 32).astype(np.float32), gam)

    def engine(x3):
        g = dnn_hip.DnnGraphBuilder()
        y = g.create_input([B, H, W, 16])
        y = g.create_max_pool2d(y, [1, 2, 2, 1], [1, 1, 1, 1], "SAME")
        y = g.create_conv2d(y, k, [1, 1, 1, 1], "SAME")
        y = g.create_bias_add(y, b)
        y = g.create_batch_norm(y, *n, 1e-5)
        y = g.create_leaky_relu(y)
        y = g.create_max_pool2d(y, [1, 2, 2, 1], [1, 2, 2, 1], "SAME")
        g.set_out_node(y)
        eng = dnn_hip.DnnInferenceEngine(g, False)
        assert ("mode=patch_x3" in eng.plan().describe()) == x3  # (an engine builds its plan on first use: here)
        return eng

    monkeypatch.delenv("DNN_HIP_X3_C16P", raising=False)
    monkeypatch.delenv("DNN_HIP_X3", raising=False)
    eng_a = engine(True)
    monkeypatch.setenv("DNN_HIP_X3_C16P", "0")
    eng_b = engine(True)
    monkeypatch.delenv("DNN_HIP_X3_C16P")
    monkeypatch.setenv("DNN_HIP_X3", "0")
    eng_c = engine(False)
    monkeypatch.delenv("DNN_HIP_X3")
    engines = (eng_a, eng_b, eng_c)
    first = [e.run(x).tobytes() for e in engines]
    assert first[0] != first[2]
    for var, arms in (("DNN_HIP_X3_C16P", ("0", "1", None)), ("DNN_HIP_X3", ("0", None))):
        for arm in arms:
            if arm is None:
                monkeypatch.delenv(var)
            else:
                monkeypatch.setenv(var, arm)
            for e, y in zip(engines, first):
                assert e.run(x).tobytes() == y, (var, arm)


@pytest.mark.parametrize("B", [24, 21])
def test_x3_pingpong_equals_tile_kernel(monkeypatch, B):
    """conv3x3_x3_pp_kernel (N = 64 from one 32-channel chunk, pooled into split planes, batch
    grids of >= 4 tiles per CU: one workgroup per CU whose two wave teams alternate MFMA and store
    steps over the CU's tile range) against the tile kernel (DNN_HIP_X3_PP=0): bit-identical
    outputs, including uneven team tile counts (B = 24: 1,248 tiles over 256 workgroups, 4 or 5
    each; B = 21: 1,092); within the fp32 tolerance of the float64 oracle; repeat runs identical."""
    rng = np.random.default_rng(B)
    x = rng.standard_normal((B, 104, 104, 32)).astype(np.float32)
    k = (rng.standard_normal((3, 3, 32, 64)) * np.sqrt(2.0 / 288)).astype(np.float32)
    b = rng.standard_normal(64).astype(np.float32) * 0.1
    gam = rng.uniform(0.5, 1.5, 64).astype(np.float32)
    gam[::5] *= -1
    n = (rng.standard_normal(64).astype(np.float32) * 0.1, rng.uniform(0.5, 1.5, 64).astype(np.float32), gam)
    k2 = (rng.standard_normal((3, 3, 64, 128)) * np.sqrt(2.0 / 576)).astype(np.float32)  # (x3 consumer)

    def graph():
        g = dnn_hip.DnnGraphBuilder()
        y = g.create_input(list(x.shape))
        y = g.create_max_pool2d(y, [1, 2, 2, 1], [1, 1, 1, 1], "SAME")
        y = g.create_conv2d(y, k, [1, 1, 1, 1], "SAME")
        y = g.create_bias_add(y, b)
        y = g.create_batch_norm(y, *n, 1e-5)
        y = g.create_leaky_relu(y)
        y = g.create_max_pool2d(y, [1, 2, 2, 1], [1, 2, 2, 1], "SAME")
        y = g.create_conv2d(y, k2, [1, 1, 1, 1], "SAME")
        y = g.create_leaky_relu(y)
        g.set_out_node(y)
        return g

    outs = {}
    for pp in ("1", "0"):  # read when the plan is created: one engine per arm
        monkeypatch.setenv("DNN_HIP_X3_PP", pp)
        eng = dnn_hip.DnnInferenceEngine(graph(), False)
        conv = [ln for ln in eng.plan().describe().splitlines() if ln.startswith("conv")]
        assert "mode=patch_x3" in conv[0] and "+pool2x2s2" in conv[0] and "mode=patch_x3" in conv[1], conv
        outs[pp] = eng.run(x)
        assert np.array_equal(eng.run(x), outs[pp])
    assert np.array_equal(outs["1"], outs["0"])
    ref = R.max_pool2d(x, [1, 2, 2, 1], [1, 1, 1, 1], "SAME")
    ref = R.max_pool2d(R.leaky_relu(R.batch_norm(R.bias_add(R.conv2d(ref, k), b), *n, 1e-5)),
                       [1, 2, 2, 1], [1, 2, 2, 1], "SAME")
    ref = R.leaky_relu(R.conv2d(ref, k2))
    assert R.normwise_err(outs["1"], ref) < 3 * LAYER_TOL


@pytest.mark.parametrize("case", [(11, 208, 208), (9, 200, 210)])
def test_x3_c16_pingpong_equals_persistent(monkeypatch, case):
    """conv1's ping-pong kernel (conv3x3_x3_c16pp_kernel: one 512-thread workgroup per CU, two
    wave teams alternating MFMA and store steps; batch grids of >= 4 tiles per CU) equals the
    two-workgroup persistent kernel (DNN_HIP_X3_C16PP=0) bit for bit -- YOLO's 208 x 208 frames
    and ragged 200 x 210 ones (partial tiles on both edges), tile counts that leave the teams of a
    workgroup unequal work; repeat runs equal; batch rows equal batch-1 runs; within the fp32
    tolerance of the float64 oracle; negative-gamma channels."""
    B, H, W = case
    rng = np.random.default_rng(B * 31 + H + W)
    x = rng.standard_normal((B, H, W, 16)).astype(np.float32)

    def layer(c, od):
        k = (rng.standard_normal((3, 3, c, od)) * np.sqrt(2.0 / (9 * c))).astype(np.float32)
        b = rng.standard_normal(od).astype(np.float32) * 0.1
        gam = rng.uniform(0.5, 1.5, od).astype(np.float32)
        gam[::5] *= -1
        return k, b, (rng.standard_normal(od).astype(np.float32) * 0.1, rng.uniform(0.5, 1.5, od).astype(np.float32),
                      gam)

    layers = [(layer(16, 32), True), (layer(32, 64), False)]

    def graph(shape):
        g = dnn_hip.DnnGraphBuilder()
        y = g.create_input(list(shape))
        y = g.create_max_pool2d(y, [1, 2, 2, 1], [1, 1, 1, 1], "SAME")  # (an fp32 producer before conv1)
        for (k, b, n), pool in layers:
            y = g.create_conv2d(y, k, [1, 1, 1, 1], "SAME")
            y = g.create_bias_add(y, b)
            y = g.create_batch_norm(y, *n, 1e-5)
            y = g.create_leaky_relu(y)
            if pool:
                y = g.create_max_pool2d(y, [1, 2, 2, 1], [1, 2, 2, 1], "SAME")
        g.set_out_node(y)
        return g

    outs = {}
    for arm in ("1", "0"):
        monkeypatch.setenv("DNN_HIP_X3_C16PP", arm)
        eng = dnn_hip.DnnInferenceEngine(graph(x.shape), False)
        conv = [ln for ln in eng.plan().describe().splitlines() if ln.startswith("conv")]
        assert all("mode=patch_x3" in c for c in conv) and "+pool2x2s2" in conv[0], conv
        outs[arm] = eng.run(x)
        assert np.array_equal(eng.run(x), outs[arm]), arm
    assert np.array_equal(outs["1"], outs["0"])
    monkeypatch.delenv("DNN_HIP_X3_C16PP")
    one = dnn_hip.DnnInferenceEngine(graph((1,) + x.shape[1:]), False)
    assert np.array_equal(one.run(x[B - 1:B]), outs["1"][B - 1:B])
    ref = R.max_pool2d(x[[0, B - 1]], [1, 2, 2, 1], [1, 1, 1, 1], "SAME")
    for (k, b, n), pool in layers:
        ref = R.leaky_relu(R.batch_norm(R.bias_add(R.conv2d(ref, k), b), *n, 1e-5))
        if pool:
            ref = R.max_pool2d(ref, [1, 2, 2, 1], [1, 2, 2, 1], "SAME")
    assert R.normwise_err(outs["1"][[0, B - 1]], ref) < 3 * LAYER_TOL


def test_x3_tile_small_tiles_same_bits():
    """The narrow x3 tile kernel's two tile shapes (kernels_x3.hip: 8 x 26 / 4 x 26 tiles when a
    launch has at least two workgroups per CU, else 2 x 26 tiles of 2 x 2 waves -- the single-frame
    latency plans' conv2 / conv3): a 12-frame batch takes the batch tiles for both layers (624 /
    1,248 tiles at 104 x 104), each frame alone the small ones (52 / 104); the rows are
    bit-identical (the summation order depends on N and K only), within the fp32 tolerance of the
    float64 oracle."""
    rng = np.random.default_rng(77)
    B, H, W = 12, 104, 104
    x = rng.standard_normal((B, H, W, 32)).astype(np.float32)

    def layer(c, od):
        k = (rng.standard_normal((3, 3, c, od)) * np.sqrt(2.0 / (9 * c))).astype(np.float32)
        b = rng.standard_normal(od).astype(np.float32) * 0.1
        gam = rng.uniform(0.5, 1.5, od).astype(np.float32)
        gam[::5] *= -1
        return k, b, (rng.standard_normal(od).astype(np.float32) * 0.1, rng.uniform(0.5, 1.5, od).astype(np.float32),
                      gam)

    layers = [(layer(32, 64), False), (layer(64, 128), True)]

    def graph(shape):
        g = dnn_hip.DnnGraphBuilder()
        y = g.create_input(list(shape))
        y = g.create_max_pool2d(y, [1, 2, 2, 1], [1, 1, 1, 1], "SAME")
        for (k, b, n), pool in layers:
            y = g.create_conv2d(y, k, [1, 1, 1, 1], "SAME")
            y = g.create_bias_add(y, b)
            y = g.create_batch_norm(y, *n, 1e-5)
            y = g.create_leaky_relu(y)
            if pool:
                y = g.create_max_pool2d(y, [1, 2, 2, 1], [1, 2, 2, 1], "SAME")
        g.set_out_node(y)
        return g

    eng = dnn_hip.DnnInferenceEngine(graph(x.shape), False)
    conv = [ln for ln in eng.plan().describe().splitlines() if ln.startswith("conv")]
    assert all("mode=patch_x3" in c for c in conv) and "+pool2x2s2" in conv[1], conv
    y = eng.run(x)
    one = dnn_hip.DnnInferenceEngine(graph((1,) + x.shape[1:]), False)
    for f in (0, 5, B - 1):
        assert np.array_equal(one.run(x[f:f + 1]), y[f:f + 1]), f
    ref = R.max_pool2d(x[[0, B - 1]], [1, 2, 2, 1], [1, 1, 1, 1], "SAME")
    for (k, b, n), pool in layers:
        ref = R.leaky_relu(R.batch_norm(R.bias_add(R.conv2d(ref, k), b), *n, 1e-5))
        if pool:
            ref = R.max_pool2d(ref, [1, 2, 2, 1], [1, 2, 2, 1], "SAME")
    assert R.normwise_err(y[[0, B - 1]], ref) < 3 * LAYER_TOL


CHAIN01_CASES = [
    # B, H, W: conv 3->16 + pool 2x2 s2 (conv0's packed kernel) -> 16->32 + pool (the 16-channel
    # x3 kernel) -> 32->64 (tile kernel)
    (2, 96, 104),  # whole 16 x 26 tiles of the 16-channel kernel after the pool (48 x 52)
    (3, 60, 84),   # ragged tiles (30 x 42 after the pool)
]


@pytest.mark.parametrize("case", CHAIN01_CASES)
def test_conv0_conv1_chain(monkeypatch, case):
    """conv0's packed kernel (pool fused) -> conv1's 16-channel x3 kernel (splits conv0's fp32
    output while staging; pool fused) -> a 32-channel x3 tile conv: within the fp32 tolerance of
    the float64 oracle; batch rows bit-equal to batch-1 runs and repeat runs; negative-gamma
    channels; whole and ragged 16 x 26 tiles."""
    B, H, W = case
    rng = np.random.default_rng(B * 13 + H + W)
    x = rng.uniform(0.0, 1.0, (B, H, W, 3)).astype(np.float32)

    def layer(c, od):
        k = (rng.standard_normal((3, 3, c, od)) * np.sqrt(2.0 / (9 * c))).astype(np.float32)
        b = rng.standard_normal(od).astype(np.float32) * 0.1
        gam = rng.uniform(0.5, 1.5, od).astype(np.float32)
        gam[::5] *= -1
        return k, b, (rng.standard_normal(od).astype(np.float32) * 0.1, rng.uniform(0.5, 1.5, od).astype(np.float32),
                      gam)

    layers = [(layer(3, 16), True), (layer(16, 32), True), (layer(32, 64), False)]

    def graph(shape):
        g = dnn_hip.DnnGraphBuilder()
        y = g.create_input(list(shape))
        for (k, b, n), pool in layers:
            y = g.create_conv2d(y, k, [1, 1, 1, 1], "SAME")
            y = g.create_bias_add(y, b)
            y = g.create_batch_norm(y, *n, 1e-5)
            y = g.create_leaky_relu(y)
            if pool:
                y = g.create_max_pool2d(y, [1, 2, 2, 1], [1, 2, 2, 1], "SAME")
        g.set_out_node(y)
        return g

    ref = x
    for (k, b, n), pool in layers:
        ref = R.leaky_relu(R.batch_norm(R.bias_add(R.conv2d(ref, k), b), *n, 1e-5))
        if pool:
            ref = R.max_pool2d(ref, [1, 2, 2, 1], [1, 2, 2, 1], "SAME")
    outs = {}
    # conv1's kernel (DNN_HIP_X3_C16P, read when the plan is created): 0 one tile per workgroup, 1 (default)
    # persistent with the last K step on 16x16x16 (another MFMA for tap 8)
    for pv in ("0", "1"):
        monkeypatch.setenv("DNN_HIP_X3_C16P", pv)
        eng = dnn_hip.DnnInferenceEngine(graph(x.shape), False)
        conv = [ln for ln in eng.plan().describe().splitlines() if ln.startswith("conv")]
        assert "mode=direct" in conv[0] and "mode=patch_x3" in conv[1] and "mode=patch_x3" in conv[2], conv
        y = eng.run(x)
        y0 = dnn_hip.DnnInferenceEngine(graph((1,) + x.shape[1:]), False).run(x[:1])
        assert np.array_equal(y0, y[:1]), pv
        assert np.array_equal(eng.run(x), y), pv
        assert R.normwise_err(y, ref) < 3 * LAYER_TOL, pv
        outs[pv] = y
    assert R.normwise_err(outs["1"], ref) <= 1.25 * max(R.normwise_err(outs["0"], ref), 1e-7)


FRONT_CASES = [
    # B, H, W: conv0 (direct) -> conv1 (16-channel x3, split planes out) -> an x3 layer reading them
    (2, 96, 128),   # 6 x 8 tiles per frame: the frame patch's zero border on every side
    (5, 64, 32),    # narrow frames, several rounds of tiles per workgroup on small grids
    (1, 416, 416),  # YOLO's frame: 169 tiles, fewer than the CUs
]


@pytest.mark.parametrize("case", FRONT_CASES)
def test_front_conv0_conv1_chain(case):
    """YOLO's front (conv0_packed_pool -> conv3x3_x3_c16p) with a third x3 layer reading the split
    planes conv1 writes: batch rows equal batch-1 runs, repeat runs equal, within the layer
    tolerance of the float64 oracle, negative-gamma channels.  (Round 5's fused conv0 + conv1
    kernel, measured slower than these two, was removed in round 6.)"""
    B, H, W = case
    rng = np.random.default_rng(B * 7 + H + W)
    x = rng.uniform(0.0, 1.0, (B, H, W, 3)).astype(np.float32)
    x[0, 0, :5] = 0.0  # zero pixels at a frame corner, exact 1.0 inside
    x[-1, H // 2, W // 2] = 1.0

    def layer(c, od):
        k = (rng.standard_normal((3, 3, c, od)) * np.sqrt(2.0 / (9 * c))).astype(np.float32)
        b = rng.standard_normal(od).astype(np.float32) * 0.1
        gam = rng.uniform(0.5, 1.5, od).astype(np.float32)
        gam[::5] *= -1
        return k, b, (rng.standard_normal(od).astype(np.float32) * 0.1, rng.uniform(0.5, 1.5, od).astype(np.float32),
                      gam)

    layers = [(layer(3, 16), True), (layer(16, 32), True), (layer(32, 64), False)]

    def graph(shape):
        g = dnn_hip.DnnGraphBuilder()
        y = g.create_input(list(shape))
        for (k, b, n), pool in layers:
            y = g.create_conv2d(y, k, [1, 1, 1, 1], "SAME")
            y = g.create_bias_add(y, b)
            y = g.create_batch_norm(y, *n, 1e-5)
            y = g.create_leaky_relu(y)
            if pool:
                y = g.create_max_pool2d(y, [1, 2, 2, 1], [1, 2, 2, 1], "SAME")
        g.set_out_node(y)
        return g

    eng = dnn_hip.DnnInferenceEngine(graph(x.shape), False)
    conv = [ln for ln in eng.plan().describe().splitlines() if ln.startswith("conv")]
    assert "mode=direct" in conv[0] and "front01" not in eng.plan().describe(), conv
    y = eng.run(x)
    assert np.array_equal(eng.run(x), y)
    f = B - 1
    y1 = dnn_hip.DnnInferenceEngine(graph((1,) + x.shape[1:]), False).run(x[f:f + 1])
    assert np.array_equal(y1, y[f:f + 1])
    ref = x
    for (k, b, n), pool in layers:
        ref = R.leaky_relu(R.batch_norm(R.bias_add(R.conv2d(ref, k), b), *n, 1e-5))
        if pool:
            ref = R.max_pool2d(ref, [1, 2, 2, 1], [1, 2, 2, 1], "SAME")
    assert R.normwise_err(y, ref) < 3 * LAYER_TOL


@pytest.mark.parametrize("kind", ["huge", "tiny"])
def test_x3_split_total_over_finite_fp32(monkeypatch, kind):
    """split3 (gemm_f32.h) is total over finite fp32: an operand above the largest bf16
    (0x1.fep127 < |x| <= FLT_MAX, where round-to-nearest gives inf and the remainder a NaN)
    takes the truncated top piece and stays exact; operands below 2^-100 lose at most 2^-124
    absolute.  A pool -> conv3x3 (x3 patch kernel, C = 64 -> 256) on inputs holding such values
    among normal ones: finite everywhere, within the layer tolerance of the float64 oracle and
    of the fp32-MFMA path's error (DNN_HIP_X3=0) on the same input."""
    rng = np.random.default_rng(11 if kind == "huge" else 12)
    B, H, W, C, N = 2, 13, 13, 64, 256
    x = rng.standard_normal((B, H, W, C)).astype(np.float32)
    fmax = np.finfo(np.float32).max
    if kind == "huge":
        # FLT_MAX, values between the largest bf16 and FLT_MAX, and their negatives, spread over
        # pixels and channels; weights small enough that every sum stays finite
        vals = np.array([fmax, 3.3999e38, 3.3962e38, -fmax, -3.398e38, 3.3895e38], np.float32)
        idx = rng.choice(B * H * W * C, size=120, replace=False)
        x.reshape(-1)[idx] = vals[np.arange(idx.size) % vals.size]
        scale = 1e-8
    else:
        # a quarter of the elements below 2^-100 (down into fp32 denormals)
        tiny = (rng.standard_normal(x.size // 4) * 10.0 ** rng.uniform(-44, -31, x.size // 4)).astype(np.float32)
        x.reshape(-1)[rng.choice(x.size, size=tiny.size, replace=False)] = tiny
        scale = 1.0
    k = (rng.standard_normal((3, 3, C, N)) * np.sqrt(2.0 / (9 * C)) * scale).astype(np.float32)

    def graph():
        g = dnn_hip.DnnGraphBuilder()
        y = g.create_input(list(x.shape))
        y = g.create_max_pool2d(y, [1, 2, 2, 1], [1, 1, 1, 1], "SAME")
        y = g.create_conv2d(y, k, [1, 1, 1, 1], "SAME")
        g.set_out_node(y)
        return g

    ref = R.conv2d(R.max_pool2d(x, [1, 2, 2, 1], [1, 1, 1, 1], "SAME"), k)
    assert np.isfinite(ref).all()
    errs = {}
    for x3 in ("1", "0"):
        monkeypatch.setenv("DNN_HIP_X3", x3)
        eng = dnn_hip.DnnInferenceEngine(graph(), False)
        assert eng.plan().describe().count("mode=patch_x3") == (1 if x3 == "1" else 0)
        y = eng.run(x)
        assert np.isfinite(y).all(), (x3, int((~np.isfinite(y)).sum()))
        errs[x3] = R.normwise_err(y, ref)
        print("%s x3=%s normwise err %.3e" % (kind, x3, errs[x3]))
    assert errs["1"] < LAYER_TOL and errs["0"] < LAYER_TOL, errs
    assert errs["1"] <= max(1.25 * errs["0"], 2e-7), errs
