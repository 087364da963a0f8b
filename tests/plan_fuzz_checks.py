"""Comparison helpers of tests/test_gpu_plan_fuzz.py: plain functions on numpy arrays, so that
tests/test_plan_fuzz_cases.py can show without a GPU that each of them fails on a tampered
buffer.  Every helper raises AssertionError naming what differed and where."""
import numpy as np

import ref_numpy as R

LAYER_TOL = 2e-6       # fp32 and latency plans, per layer (the suite's existing bar)
FP16_LAYER_TOL = 5e-3  # fp16 plans, per layer (the suite's existing bar)
GUARD_BYTES = 4096     # on each side of the weight arena and the workspace (keeps 256-B alignment)
GUARD_FLOATS = 1024    # on each side of the input and output tensors
POISON = 0xFF          # 0xFFFF.. is a NaN as fp32, fp16 and bf16
CANARY = 0x7FC0BEEF    # a quiet fp32 NaN with a fixed payload; compared as int32


def _i32(a):
    a = np.ascontiguousarray(a)
    assert a.dtype.itemsize == 4, a.dtype
    return a.view(np.int32)


def check_bits(got, want, what):
    """got == want bit for bit (NaNs and signed zeros included)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, f"{what}: shape {got.shape} != {want.shape}"
    bad = np.flatnonzero(_i32(got).reshape(-1) != _i32(want).reshape(-1))
    assert bad.size == 0, (f"{what}: {bad.size} of {got.size} words differ, first at flat index {int(bad[0])}: "
                           f"{got.reshape(-1)[bad[0]]!r} != {want.reshape(-1)[bad[0]]!r}")


def check_finite(got, what):
    bad = np.flatnonzero(~np.isfinite(np.asarray(got)).reshape(-1))
    assert bad.size == 0, f"{what}: {bad.size} non-finite values, first at flat index {int(bad[0])}"


def check_canary(flat, n, row_floats, batch, what):
    """`flat` is the whole output tensor: GUARD_FLOATS, batch rows of row_floats, GUARD_FLOATS.
    After a run of n frames both guards and the rows >= n must still hold CANARY exactly."""
    w = _i32(flat).reshape(-1)
    assert w.size == 2 * GUARD_FLOATS + batch * row_floats, (w.size, batch, row_floats)
    keep = np.ones(w.size, dtype=bool)
    keep[GUARD_FLOATS:GUARD_FLOATS + n * row_floats] = False
    bad = np.flatnonzero(keep & (w != np.int32(CANARY)))
    if bad.size:
        i = int(bad[0])
        where = ("front guard" if i < GUARD_FLOATS else "back guard" if i >= GUARD_FLOATS + batch * row_floats
                 else f"row {(i - GUARD_FLOATS) // row_floats} (>= n = {n})")
        raise AssertionError(f"{what}: {bad.size} canary words overwritten, first at word {i} ({where}): "
                             f"{int(w[i]) & 0xFFFFFFFF:#010x}")


def check_guard(buf_u8, what):
    """`buf_u8` is a whole uint8 buffer: its first and last GUARD_BYTES must still be POISON."""
    b = np.asarray(buf_u8)
    assert b.dtype == np.uint8 and b.size >= 2 * GUARD_BYTES, (b.dtype, b.size)
    for name, g, base in (("front", b[:GUARD_BYTES], 0), ("back", b[-GUARD_BYTES:], b.size - GUARD_BYTES)):
        bad = np.flatnonzero(g != POISON)
        assert bad.size == 0, (f"{what}: {bad.size} bytes of the {name} guard overwritten, first at byte "
                               f"{base + int(bad[0])}: {int(g[bad[0]]):#04x}")


def check_layer_err(got, want, tol, what):
    """Teacher-forced per-layer accuracy: max|got - want| / max|want| < tol, and got finite."""
    check_finite(got, what)
    assert np.asarray(got).shape == np.asarray(want).shape, f"{what}: shape {got.shape} != {want.shape}"
    err = R.normwise_err(got, want)
    assert err < tol, f"{what}: normwise error {err:.3e} >= {tol:.1e}"
    return err


def oracle_block(x, block, w):
    """One block in float64 accumulation: [2x2/s1 pool] conv [bias] [bn] [leaky] [2x2 pool]."""
    kern, bias, bn, leaky = w
    y = np.asarray(x, np.float32)
    if block["pre_pool"]:
        y = R.max_pool2d(y, [1, 2, 2, 1], [1, 1, 1, 1], "SAME")
    y = R.conv2d(y, kern, strides=(1, 1, 1, 1), padding="SAME")
    if bias is not None:
        y = R.bias_add(y, bias)
    if bn is not None:
        y = R.batch_norm(y, *bn, 1e-5)
    if leaky:
        y = R.leaky_relu(y)
    if block["pool"]:
        s = 2 if block["pool"] == "s2" else 1
        y = R.max_pool2d(y, [1, 2, 2, 1], [1, s, s, 1], "SAME")
    return y
