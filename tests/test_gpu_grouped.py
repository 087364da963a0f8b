"""GPU: the grouped-conv kernels (csrc/conv_grouped.hip) against torch's float64 conv2d(groups=g): the host
entry, plans on guarded buffers (batch and latency mode, into a tap's region, rows bit-equal across batch
sizes), Conv2DPadded.run(), a finalized plan's refusal, and a narrow grouped Darknet cfg end to end."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import darknet_cases as DC
import darknet_import as D
import dnn_hip
import plan_fuzz_checks as K
import ref_numpy as R
import residual_cases as RS
from test_grouped_cpu import conv_section as _conv

pytestmark = pytest.mark.gpu

TOL = 1e-4  # the project's normwise bar against float64
B = 3

# name: (h, w, c, od, groups, k, stride, pad, affine, leaky)
CASES = {
    "one_full_tile": (5, 6, 64, 64, 16, 3, 1, 1, True, 2),
    "channel_tail_dead_blocks": (5, 6, 8, 8, 2, 3, 1, 1, False, 0),
    "tile_spans_groups_unevenly": (5, 6, 48, 96, 12, 3, 1, 1, True, 1),   # cg 4, og 8: tiles of 8 and 4 groups
    "register_budget_edge": (5, 6, 32, 32, 2, 3, 1, 1, True, 2),           # cg 16: 144 resident floats
    "two_k_chunks": (5, 6, 64, 64, 2, 3, 1, 1, True, 2),                   # cg 32: chunks of 5 and 4 taps
    "stride2_quad_tail_across_images": (13, 13, 16, 16, 4, 3, 2, 1, True, 2),  # 49 pixels an image
    "one_by_one": (5, 6, 32, 32, 4, 1, 1, 0, True, 0),                     # cg 8
    "streamed_5x5_cg12": (7, 5, 24, 8, 2, 5, 1, 2, True, 2),               # off the resident forms
    "depthwise_s1": (7, 5, 8, 8, 8, 3, 1, 1, True, 2),                     # from here on the direct kernels
    "depthwise_s2": (7, 5, 8, 8, 8, 3, 2, 1, True, 2),
    "depthwise_two_strips": (19, 5, 8, 8, 8, 3, 1, 1, False, 0),           # strips of 8 rows: 8, 8, 3
    "depthwise_5x5": (7, 5, 8, 8, 8, 5, 1, 2, True, 1),
    "scalar_depthwise_c6": (7, 5, 6, 6, 6, 3, 1, 1, True, 2),
    "scalar_multiplier_cg2_og3": (7, 5, 4, 6, 2, 3, 1, 1, True, 2),
}


def _tensors(name):
    h, w, c, od, g, k = CASES[name][:6]
    rng = np.random.default_rng(7100 + list(CASES).index(name))
    x = rng.standard_normal((B, h, w, c)).astype(np.float32)
    kern = (rng.standard_normal((k, k, c // g, od)) / np.sqrt(k * k * c // g)).astype(np.float32)
    scale = rng.uniform(0.5, 1.5, od).astype(np.float32) * np.where(np.arange(od) % 3, 1, -1).astype(np.float32)
    shift = rng.standard_normal(od).astype(np.float32)
    return x, kern, scale, shift


def _ref(x, kern, stride, pad, groups, scale, shift, leaky):
    """float64: conv2d(groups) on NCHW / OIHW, then the affine and leaky steps, back to NHWC."""
    v = F.conv2d(torch.from_numpy(x).double().permute(0, 3, 1, 2), torch.from_numpy(kern).double().permute(3, 2, 0, 1),
                 stride=stride, padding=pad, groups=groups).permute(0, 2, 3, 1).numpy()
    if scale is not None:
        v = v * scale.astype(np.float64) + shift.astype(np.float64)
    return np.where(v > 0, v, v * float(np.float32(0.1)) if leaky == 2 else v * 0.1) if leaky else v


def _entry(x, kern, stride, pad, groups, scale, shift, leaky):
    g = dnn_hip.DnnGraphBuilder()
    t = g.create_conv2d_padded(g.create_input(list(x.shape)), kern, [1, stride, stride, 1], (pad, pad), groups=groups)
    e = dnn_hip.GroupedConvEntry(t, (pad, pad))
    if scale is not None:
        e.affine = g.create_scale_shift(t, scale, shift)
    e.leaky = leaky
    return e


@pytest.mark.parametrize("name", list(CASES))
def test_grouped_conv_against_float64(name):
    h, w, c, od, groups, k, stride, pad, affine, leaky = CASES[name]
    x, kern, scale, shift = _tensors(name)
    if not affine:
        scale = shift = None
    want = _ref(x, kern, stride, pad, groups, scale, shift, leaky)
    mode = "grouped_mfma" if (c // groups) % 4 == 0 and (od // groups) % 4 == 0 else "grouped_direct"
    # the host entry
    out = np.full(want.shape, np.nan, np.float32)
    rc = dnn_hip.mylib.dnn_conv_grouped_host(dnn_hip._vp(x), dnn_hip._vp(kern), dnn_hip._vp(scale), dnn_hip._vp(shift),
                                             dnn_hip._vp(out), *x.shape, k, k, od, stride, stride, pad, pad, groups, leaky)
    assert rc == 0, dnn_hip.last_error()
    err = R.normwise_err(out, want)
    print(f"{name}: dnn_conv_grouped_host normwise error {err:.3e}")
    assert err < TOL
    # in plans: the grouped conv writes a tap's region, a whole-tensor slice copies it to the output
    entries = [_entry(x, kern, stride, pad, groups, scale, shift, leaky), dnn_hip.TapEntry(0), dnn_hip.SliceEntry(0, od)]
    rows = {}
    for batch, latency in ((B, False), (1, False), (1, True)):
        gp = RS.GuardedPlan(batch, (h, w, c), entries, latency=latency)
        try:
            y = gp.run(x[:batch], f"{name} batch {batch} latency {latency}")
            assert [q["name"] for q in gp.plan.kernels()] == ["gconv0", "slice0"]
            assert f"mode={mode}" in gp.plan.describe() and f"groups={groups}" in gp.plan.describe()
        finally:
            gp.close()
        assert R.normwise_err(y, want[:batch]) < TOL
        rows[batch, latency] = y
    K.check_bits(rows[B, False], out, f"{name}: the plan's rows are the host entry's")
    K.check_bits(rows[1, False], rows[B, False][:1], f"{name}: batch 1 against batch {B}")
    K.check_bits(rows[1, True], rows[1, False], f"{name}: latency against batch mode")
    # the node (no epilogue): Conv2DPadded.run() -> dnn_conv_grouped_host
    node = entries[0].conv
    node.in_node.set_input(x)
    node.run()
    assert R.normwise_err(node.result, _ref(x, kern, stride, pad, groups, None, None, 0)) < TOL


def test_a_finalized_plan_refuses_the_entry_and_stays_as_it_is():
    x, kern, scale, shift = _tensors("one_full_tile")
    plan = dnn_hip.Plan(B, x.shape[1:], [_entry(x, kern, 1, 1, 16, scale, shift, 2)], device=0)
    try:
        before, steps, y = plan.describe(), plan.kernels(), plan.run_host(x)
        assert dnn_hip.mylib.dnn_plan_add_conv_grouped(plan.h, 3, 3, 64, 1, 1, 1, 1, 16, None, None, None, 2) != 0
        err = dnn_hip.last_error()
        assert "dnn_plan_add_conv_grouped" in err and "finalized" in err
        assert plan.describe() == before and plan.kernels() == steps and plan.out_shape == (5, 6, 64)
        K.check_bits(plan.run_host(x), y, "output after the refused entry")
        assert R.normwise_err(y, _ref(x, kern, 1, 1, 16, scale, shift, 2)) < TOL
    finally:
        plan.close()


def test_host_entry_refuses_bad_arguments():
    x, kern = np.zeros((1, 4, 4, 8), np.float32), np.zeros((3, 3, 4, 8), np.float32)
    ptrs = (dnn_hip._vp(x), dnn_hip._vp(kern), None, None, dnn_hip._vp(np.zeros_like(x)))
    for n, hw, groups, pad, word in ((1, 4, 1, 1, "padded"), (1, 4, 3, 1, "divide"), (1, 4, 2, 3, "pads"), (64, 2048, 2, 1, "2 GiB")):
        assert dnn_hip.mylib.dnn_conv_grouped_host(*ptrs, n, hw, hw, 8, 3, 3, 8, 1, 1, pad, pad, groups, 0) != 0
        assert "dnn_conv_grouped_host" in dnn_hip.last_error() and word in dnn_hip.last_error()


# a stem and a stride-2 grouped 3x3, a ResNeXt block (1x1, grouped 3x3, 1x1, shortcut), a depthwise +
# pointwise pair, one head
CFG = ("[net]\nwidth=32\nheight=32\nchannels=3\n" + _conv(16, 3) + _conv(32, 3, 2, groups=4) +
       _conv(16, 1) + _conv(16, 3, groups=4) + _conv(32, 1) + "[shortcut]\nfrom=-4\nactivation=linear\n" +
       _conv(32, 3, 2, groups=32) + _conv(48, 1) + _conv(24, 1, act="linear") +
       "[yolo]\nmask=0,1,2\nanchors=4,5,8,10,13,16\nclasses=3\n")


def test_darknet_model_with_grouped_and_depthwise_convs():
    secs = D.parse_cfg(CFG)
    layers = DC.darknet_layers(secs)
    m = D.DarknetModel(CFG, layers, in_shape=[2, 32, 32, 3])
    x = np.random.default_rng(7200).uniform(0, 1, (2, 32, 32, 3)).astype(np.float32)
    out = m.inference(x)[0].copy()
    text = m.sess.plan().describe()
    assert m.sess._plan is not None and [l.rsplit("groups=", 1)[1] for l in text.splitlines() if "groups=" in l] == ["4", "4", "32"]
    v, acts, convs = x.astype(np.float64), [], iter(layers)
    for sec in secs[1:-1]:
        if sec["type"] == "shortcut":
            v = v + acts[int(sec["from"])]
        else:
            _, size, stride, pad, _, act = D.conv_params(sec)
            layer = next(convs)
            scale, shift = D.fold_batchnorm(layer)
            v = _ref(v, D.kernel_hwio(layer), stride, pad, int(sec["groups"]), scale, shift, 2 if act == "leaky" else 0)
        acts.append(v)
    assert out.shape == v.shape == (2, 8, 8, 24) and 0.01 < float(np.abs(v).mean()) < 100
    err = R.normwise_err(out, v)
    print(f"narrow grouped Darknet model: normwise error {err:.3e}")
    assert err < TOL
