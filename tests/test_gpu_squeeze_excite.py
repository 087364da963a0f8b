"""GPU: the squeeze-and-excitation kernels (csrc/squeeze_excite.hip) against the float64 formulas (tests/se_oracle.py):
the host entry and the plan entry on guarded buffers, batch rows bit for bit, and the refused widths."""
import ctypes

import numpy as np
import pytest

import dnn_hip
import plan_fuzz_checks as K
import ref_numpy as R
import residual_cases as RS
import se_oracle as SO

pytestmark = pytest.mark.gpu

# Normwise against float64.  The project's bar for forwards is 1e-4; the measured worst case of these cases is 2.1e-7
# (squeeze-and-excitation), so the bar here is ten times that: a few fp32 roundings per output.
TOL = 2e-6
ACTS = [(name, "swish", "logistic") for name in SO.CASES] + [
    ("scalar_odd", "leaky", "logistic"), ("scalar_odd", "linear", "linear"), ("scalar_odd", "mish", "swish")]


def _entry(x, w1, b1, act1, w2, b2, act2):
    g = dnn_hip.DnnGraphBuilder()
    return dnn_hip.SqueezeExciteEntry(g.create_squeeze_excite(g.create_input(list(x.shape)), w1, b1, act1, w2, b2, act2))


@pytest.mark.parametrize("name,act1,act2", ACTS)
def test_squeeze_excite_against_float64(name, act1, act2):
    x, w1, b1, w2, b2 = SO.tensors(name)
    want = SO.forward64(x, w1, b1, act1, w2, b2, act2)
    if act2 == "logistic":  # the fixture's promise: gates spread over (0, 1)
        g = SO.gate64(x, w1, b1, act1, w2, b2, act2)
        assert g.min() < 0.35 and g.max() > 0.65 and 0.2 < np.median(g) < 0.8
    out = np.full(x.shape, np.nan, np.float32)
    v, A = dnn_hip._vp, dnn_hip.SE_ACTIVATIONS
    rc = dnn_hip.mylib.dnn_squeeze_excite_host(v(x), v(w1), v(b1), A[act1], v(w2), v(b2), A[act2], v(out), *x.shape,
                                               w1.shape[1])
    assert rc == 0, dnn_hip.last_error()
    err = R.normwise_err(out, want)
    print(f"{name} {act1},{act2}: dnn_squeeze_excite_host normwise error {err:.3e}")
    assert err <= TOL
    gp = RS.GuardedPlan(x.shape[0], x.shape[1:], [_entry(x, w1, b1, act1, w2, b2, act2)])
    try:
        y = gp.run(x, name)
        assert [q["name"] for q in gp.plan.kernels()] == ["se0.squeeze", "se0.excite"]
        assert f"squeeze_excite {x.shape[1]}x{x.shape[2]}x{x.shape[3]} cr={w1.shape[1]}" in gp.plan.describe()
    finally:
        gp.close()
    K.check_bits(y, out, f"{name}: the plan's rows are the host entry's")


@pytest.mark.parametrize("name", ["scalar_odd", "two_ranges_ragged"])
def test_batch_rows_equal_batch_one_runs_bit_for_bit(name):
    x, w1, b1, w2, b2 = SO.tensors(name)
    entries = [_entry(x, w1, b1, "swish", w2, b2, "logistic")]
    whole, one = RS.GuardedPlan(x.shape[0], x.shape[1:], entries), RS.GuardedPlan(1, x.shape[1:], entries)
    try:
        y = whole.run(x, name)
        for i in range(x.shape[0]):
            K.check_bits(one.run(x[i:i + 1], name), y[i:i + 1], f"{name}: image {i} alone against its row of the batch")
    finally:
        whole.close()
        one.close()


@pytest.mark.parametrize("c,cr,word", [(4097, 4, "DNN_SE_MAX_C"), (8, 0, "DNN_SE_MAX_CR")])
def test_widths_outside_the_limits_are_refused(c, cr, word):
    lib, h = dnn_hip.mylib, ctypes.c_void_p()
    assert lib.dnn_plan_create(1, 2, 2, c, ctypes.byref(h)) == 0
    try:
        assert lib.dnn_plan_add_squeeze_excite(h, cr, None, None, 4, None, None, 3) != 0
        assert "dnn_plan_add_squeeze_excite" in dnn_hip.last_error() and word in dnn_hip.last_error()
        assert lib.dnn_plan_num_kernels(h) == 0
    finally:
        lib.dnn_plan_destroy(h)
    x, w = np.zeros((1, 2, 2, c), np.float32), np.zeros((c, max(cr, 1)), np.float32)
    v = dnn_hip._vp
    assert lib.dnn_squeeze_excite_host(v(x), v(w), None, 4, v(w), None, 3, v(np.zeros_like(x)), 1, 2, 2, c, cr) != 0
    assert "dnn_squeeze_excite_host" in dnn_hip.last_error() and word in dnn_hip.last_error()
