"""CPU: the grouped-conv plan entry (dnn_plan_add_conv_grouped) without a device: exported symbols,
refusals that leave the plan unchanged, its describe / kernel_info lines, and Darknet's groups= in the
importer (shapes, weight counts, the .weights round trip)."""
import ctypes
import os

import numpy as np
import pytest

import darknet_cases as DC
import darknet_import as D
import dnn_hip

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = dnn_hip.mylib


def conv_section(filters, size, stride=1, groups=1, act="leaky"):
    bn = "batch_normalize=1\n" if act == "leaky" else ""
    return f"[convolutional]\n{bn}filters={filters}\nsize={size}\nstride={stride}\npad=1\ngroups={groups}\nactivation={act}\n"


CFG = ("[net]\nwidth=16\nheight=16\nchannels=3\n" + conv_section(16, 3) + conv_section(32, 3, 2, groups=4) +
       conv_section(24, 1, act="linear") + "[yolo]\nmask=0,1,2\nanchors=1,2,3,4,5,6\nclasses=3\n")


def _plan(shape=(8, 8, 16), precision="fp32"):
    h = ctypes.c_void_p()
    assert LIB.dnn_plan_create(2, *shape, ctypes.byref(h)) == 0
    assert LIB.dnn_plan_set_precision(h, dnn_hip.PRECISIONS[precision]) == 0
    return h


def _describe(h):
    buf = ctypes.create_string_buffer(4096)
    assert LIB.dnn_plan_describe(h, buf, 4096) == 0
    return buf.value.decode()


def _add(h, od=32, groups=4, k=3, pad=1, stride=1):
    return LIB.dnn_plan_add_conv_grouped(h, k, k, od, stride, stride, pad, pad, groups, None, None, None, 2)


def test_both_libraries_export_the_symbols_and_the_header_declares_them():
    plan_h = open(os.path.join(REPO, "include", "dnn_hip_plan.h")).read()
    for name in ("libdnn_hip.so", "libdnn_hip_avx.so"):
        lib = dnn_hip.load_library(name)
        for sym in ("dnn_plan_add_conv_grouped", "dnn_conv_grouped_host"):
            assert hasattr(lib, sym), f"{name} does not export {sym}"
            assert f"int {sym}(" in plan_h


@pytest.mark.parametrize("kw,word", [(dict(groups=1), "dnn_plan_add_conv_padded"), (dict(groups=0), "groups"),
                                     (dict(groups=3), "divide"), (dict(od=30), "divide"), (dict(pad=3), "pads"),
                                     (dict(pad=-1), "pads"), (dict(precision="fp16"), "fp16")])
def test_refusals_leave_the_plan_unchanged(kw, word):
    h = _plan(precision=kw.pop("precision", "fp32"))
    try:
        ok = _add(h) == 0  # (an fp16 plan stays empty)
        before, nk = _describe(h), LIB.dnn_plan_num_kernels(h)
        assert ok == (word != "fp16") and (before != "") == ok
        assert _add(h, **kw) != 0
        err = dnn_hip.last_error()
        assert "dnn_plan_add_conv_grouped" in err and word in err
        assert _describe(h) == before and LIB.dnn_plan_num_kernels(h) == nk
    finally:
        LIB.dnn_plan_destroy(h)


def test_describe_and_kernel_info():
    h = _plan()
    try:
        assert _add(h, od=32, groups=4, stride=2) == 0 and _add(h, od=32, groups=32) == 0
        assert LIB.dnn_plan_add_max_pool(h, 2, 2, 2, 2, 1) == 0  # no pool folds into a grouped conv
        lines = _describe(h).splitlines()
        assert lines[0] == "conv 8x8x16 -> 4x4x32 k3x3 s2 mode=grouped_mfma K=36 pad=1,1 groups=4"
        assert lines[1] == "conv 4x4x32 -> 4x4x32 k3x3 s1 mode=grouped_direct K=9 pad=1,1 groups=32"
        assert lines[2].startswith("pool 4x4x32 -> 2x2x32")
        name, fl, by, M = ctypes.create_string_buffer(64), ctypes.c_double(), ctypes.c_double(), 2 * 4 * 4
        for k, cg, in_floats in ((0, 4, 2 * 8 * 8 * 16), (1, 1, M * 32)):
            assert LIB.dnn_plan_kernel_info(h, k, name, 64, ctypes.byref(fl), ctypes.byref(by)) == 0
            assert (name.value, fl.value) == (b"gconv%d" % k, 2.0 * M * 32 * 9 * cg)
            assert by.value == 4.0 * (in_floats + 9 * cg * 32 + M * 32)
    finally:
        LIB.dnn_plan_destroy(h)


def test_node_and_lowering():
    g = dnn_hip.DnnGraphBuilder()
    x = g.create_input([2, 8, 8, 16])
    w = np.zeros((3, 3, 4, 32), np.float32)
    with pytest.raises(ValueError):
        g.create_conv2d_padded(x, w, [1, 1, 1, 1], (1, 1), groups=2)  # the kernel's I is not C / groups
    t = g.create_conv2d_padded(x, w, [1, 2, 2, 1], (1, 1), groups=4)
    t = g.create_scale_shift(t, np.ones(32, np.float32), np.zeros(32, np.float32))
    g.set_out_node(g.create_leaky_relu_f32(t))
    entries = dnn_hip.lower_graph(g)
    assert [type(e).__name__ for e in entries] == ["GroupedConvEntry"] and entries[0].groups == 4
    assert dnn_hip.Plan.lowering(2, (8, 8, 16), entries).strip().endswith("pad=1,1 affine groups=4")


def test_importer_shapes_weights_and_round_trip(tmp_path):
    secs = D.parse_cfg(CFG)
    assert D.layer_shapes(secs)[:3] == [(16, 16, 16), (8, 8, 32), (8, 8, 24)]
    assert D.conv_shapes(secs) == [(16, 3, 3, True), (32, 4, 3, True), (24, 32, 1, False)]
    layers = DC.darknet_layers(secs)
    assert layers[1]["weights"].shape == (32, 4, 3, 3) and D.kernel_hwio(layers[1]).shape == (3, 3, 4, 32)
    path = str(tmp_path / "g.weights")
    D.save_weights(path, layers)
    back = D.load_weights(path, secs)
    for a, b in zip(layers, back):
        assert sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k]) for k in a)
    # the cfg without groups= holds 4 x the grouped conv's weights: neither file reads against the other cfg
    dense = D.parse_cfg(CFG.replace("groups=4\n", "groups=1\n"))
    with pytest.raises(D.DarknetError, match="ends inside the weights of convolutional layer 1"):
        D.load_weights(path, dense)
    D.save_weights(path, DC.darknet_layers(dense))
    with pytest.raises(D.DarknetError, match="does not match"):
        D.load_weights(path, secs)
    with pytest.raises(D.DarknetError, match="grouped"):
        D.layer_shapes(D.parse_cfg(CFG.replace("filters=32", "filters=30")))
