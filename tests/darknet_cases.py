"""Shared cases of tests/test_darknet_import_cpu.py and tests/test_gpu_darknet.py: synthetic Darknet
weights for a cfg, the narrow models the existing model tests use, and small graphs on the padded
conv entry."""
import re

import numpy as np

import darknet_import as D
import dnn_hip
import synth

# (model, width_div, input size): the widths and sizes of tests/test_gpu_multi_out.py's narrow
# YOLOv3, tests/test_gpu_spp.py's narrow YOLOv3-SPP and the narrow YOLOv3-tiny of the decode tests
NARROW = {"yolov3": (8, 64), "yolov3-spp": (8, 96), "yolov3-tiny": (4, 64)}
CLASSES = 3  # 3 x (5 + 3) = 24 head outputs, as those tests
HEAD_GAIN = 0.25  # darknet_layers: the scale of a linear head conv's weights and biases


def narrow_cfg(model, size=None):
    div, s = NARROW[model]
    s = size or s
    return D.cfg_text(model, classes=CLASSES, width=s, height=s, width_div=div)


def darknet_layers(sections, seed=0):
    """Synthetic weights in load_weights' format for every conv of `sections`, from synth's
    counter-based generators (conv k draws from streams 10 k + j): beta = 3 x the biases draw
    (non-trivial; a linear head's weights and biases are HEAD_GAIN x the draws), gamma with every third channel negative and one exactly zero (mixed sign),
    var in [0.5, 1.5).  The gamma of a conv that a [shortcut] follows is scaled by synth's
    residual gain, so 23 residual sums keep the activations O(1)."""
    layers = []
    convs = [i for i, s in enumerate(sections[1:]) if s["type"] == "convolutional"]
    for k, (at, (n, c, size, bn)) in enumerate(zip(convs, D.conv_shapes(sections))):
        w = synth.layer_weights(k, c, n, k=size, seed=seed, bn=bn)
        # (a linear head: small outputs, so that the decode's exp() gives boxes of about an anchor's size)
        gain = np.float32(3) if bn else np.float32(HEAD_GAIN)
        layer = {"biases": (w["biases"] * gain).astype(np.float32),
                 "weights": np.ascontiguousarray(w["kernel"].transpose(3, 2, 0, 1) * (np.float32(1) if bn else gain))}
        if bn:
            gamma = w["gamma"].copy()
            gamma[::3] *= np.float32(-1)
            if n > 4:
                gamma[4] = 0
            nxt = sections[at + 2] if at + 2 < len(sections) else None
            if nxt is not None and nxt["type"] == "shortcut":
                gamma *= np.float32(synth.DARKNET53_RESIDUAL_GAIN)
            layer["scales"] = gamma.astype(np.float32)
            layer["rolling_mean"] = w["moving_mean"]
            layer["rolling_variance"] = w["moving_variance"]
        layers.append(layer)
    return layers


def conv_lines(text):
    """dnn_plan_describe's lines with the padded entry's suffixes taken off: what is left is the
    entry kind, the shapes and the execution mode."""
    return [re.sub(r" pad=\d+,\d+( affine)?$", "", l) for l in text.splitlines()]


def padded_graph(B, in_shape, kernels, strides, pads, scales=None, shifts=None, leaky=None, pool=None):
    """A chain of padded convs: kernels[i] HWIO, strides[i], pads[i] = (ph, pw); scales[i] /
    shifts[i] None: no ScaleShift; leaky[i]: 0 none, 1 LeakyReLU, 2 LeakyReLUF32; pool[i]: None or
    the stride of a 2x2 SAME max pool after layer i."""
    g = dnn_hip.DnnGraphBuilder()
    t = g.create_input([B] + list(in_shape))
    for i, k in enumerate(kernels):
        t = g.create_conv2d_padded(t, k, [1, strides[i], strides[i], 1], pads[i])
        if scales is not None and scales[i] is not None:
            t = g.create_scale_shift(t, scales[i], shifts[i])
        lk = leaky[i] if leaky is not None else 0
        if lk:
            t = g.create_leaky_relu(t) if lk == 1 else g.create_leaky_relu_f32(t)
        if pool is not None and pool[i]:
            t = g.create_max_pool2d(t, [1, 2, 2, 1], [1, pool[i], pool[i], 1], "SAME")
    g.set_out_node(t)
    return g


# ------------------------------------------------------------------------------ execution modes
# One chain per fp32 execution mode a conv entry can take, at the smallest shapes of
# tests/geometry_cases.py and tests/test_gpu_parity.py that select it.  ops: ("pool", stride) a
# 2x2 SAME max pool, ("conv", k, oc) a k x k stride-1 conv padded k // 2 (= SAME's pads);
# `lines`: per conv line of dnn_plan_describe the tokens it must contain; `env` is set while the
# plan is built (the switches are read at plan time).
def _chain(B, shape, ops, lines, latency=False, env=None):
    return {"B": B, "shape": tuple(shape), "ops": ops, "lines": lines, "latency": latency, "env": env or {}}


P1, P2 = ("pool", 1), ("pool", 2)
MODE_CHAINS = {
    "gemm": _chain(2, (9, 11, 5), [("conv", 5, 24)], [["mode=gemm"]]),
    "direct_a": _chain(3, (13, 13, 64), [("conv", 1, 125)], [["mode=direct_a"]]),
    "implicit": _chain(2, (17, 15, 32), [("conv", 3, 64)], [["mode=implicit"]]),
    "implicit_c16": _chain(1, (9, 9, 16), [("conv", 3, 125)], [["mode=implicit"]]),
    "implicit_pool": _chain(3, (20, 18, 32), [("conv", 3, 64), P2], [["mode=implicit", "+pool2x2s2"]]),
    "implicit_pool_tile": _chain(2, (13, 13, 32), [("conv", 3, 64), P2], [["mode=implicit", "+pool2x2s2"]],
                                 env={"DNN_HIP_PERSIST": "0"}),
    "implicit_pool_out_x3": _chain(3, (26, 26, 32), [("conv", 3, 128), P2, ("conv", 3, 512), ("conv", 3, 256)],
                                   [["mode=implicit", "+pool2x2s2"], ["mode=patch_x3", "splitK=2 x3-combine"],
                                    ["mode=patch_x3"]]),
    "splitk_combine": _chain(3, (9, 7, 256), [("conv", 3, 768)], [["mode=implicit", "splitK=3 combine"]]),
    "splitk_reduce": _chain(3, (9, 7, 256), [("conv", 3, 768)], [["mode=implicit", "splitK=3"]],
                            env={"DNN_HIP_SPLITK_FUSED": "0"}),
    "patch": _chain(2, (26, 22, 16), [("conv", 3, 32), P2], [["mode=patch", "+pool2x2s2"]]),
    "patch_out_x3": _chain(2, (26, 22, 16), [("conv", 3, 32), P2, ("conv", 3, 64)],
                           [["mode=patch ", "+pool2x2s2"], ["mode=patch_x3"]]),
    "direct_c3": _chain(2, (40, 38, 3), [("conv", 3, 16), P2], [["mode=direct", "+pool2x2s2"]]),
    "direct_c4": _chain(2, (17, 22, 4), [("conv", 3, 16), P2], [["mode=direct", "+pool2x2s2"]]),
    "conv0_conv1_x3_c16": _chain(2, (36, 44, 3), [("conv", 3, 16), P2, ("conv", 3, 32), P2, ("conv", 3, 64)],
                                 [["mode=direct"], ["mode=patch_x3", "+pool2x2s2"], ["mode=patch_x3"]]),
    "x3_c16_raster": _chain(2, (36, 44, 3), [("conv", 3, 16), P2, ("conv", 3, 32)],
                            [["mode=direct"], ["mode=patch_x3"]]),
    "lat_x3_c16": _chain(1, (36, 44, 3), [("conv", 3, 16), P2, ("conv", 3, 32), P2, ("conv", 3, 64)],
                         [["mode=direct"], ["mode=patch_x3", "+pool2x2s2"], ["mode="]], latency=True),
    "x3_wide": _chain(2, (9, 11, 32), [P1, ("conv", 3, 256), ("conv", 3, 512)],
                      [["mode=patch_x3"], ["mode=patch_x3"]]),
    "x3_tile_raster": _chain(2, (27, 61, 32), [P1, ("conv", 3, 64), ("conv", 3, 128)],
                             [["mode=patch_x3"], ["mode=patch_x3"]]),
    "x3_tile_pool": _chain(2, (24, 52, 32), [P1, ("conv", 3, 64), P2, ("conv", 3, 128), P2, ("conv", 3, 256)],
                           [["mode=patch_x3", "+pool2x2s2"], ["mode=patch_x3", "+pool2x2s2"], ["mode=patch_x3"]]),
    "x3_pool_img": _chain(3, (13, 13, 64), [P1, ("conv", 3, 256), P2, ("conv", 3, 512), P1],
                          [["mode=patch_x3", "+pool2x2s2"], ["mode="]]),
    "x3_img": _chain(3, (13, 13, 256), [P1, ("conv", 3, 512), P1, ("conv", 3, 256)],
                     [["mode=x3_img", "+pool2x2s1"], ["mode=patch_x3"]]),
    "x3_1x1": _chain(3, (9, 11, 64), [P1, ("conv", 3, 256), ("conv", 1, 200)], [["mode=patch_x3"], ["mode=x3_1x1"]]),
    "lat_split_pool": _chain(1, (13, 13, 128), [("conv", 3, 256), P2], [["mode=implicit", "+pool2x2s2", "splitK="]],
                             latency=True),
    "lat_x3_ktile": _chain(2, (18, 18, 128), [P1, ("conv", 3, 64), P2], [["mode=x3_ktile", "+pool2x2s2"]],
                           latency=True),
    "lat_x3_ktile_pool1": _chain(2, (9, 11, 256), [P1, ("conv", 3, 192), P1], [["mode=x3_ktile", "+pool2x2s1"]],
                                 latency=True),
    "lat_x3_lat_head": _chain(1, (9, 11, 64), [P1, ("conv", 3, 192), ("conv", 3, 256), ("conv", 1, 40)],
                              [["mode=x3_lat"], ["mode=x3_lat"], ["mode=x3_ktile", "k1x1"]], latency=True,
                              env={"DNN_HIP_X3_LAT_MINWG": "1"}),
}


def chain_graph(c, ws, padded, leaky):
    """The chain as a graph: padded False -> create_conv2d SAME + BiasAdd(shift) (+ LeakyReLU), the
    entry dnn_plan_add_conv has had all along; True -> create_conv2d_padded + ScaleShift (+ leaky).
    ws: per conv (kernel, scale, shift); leaky 0 none, 1 LeakyReLU, 2 LeakyReLUF32."""
    g = dnn_hip.DnnGraphBuilder()
    t = g.create_input([c["B"]] + list(c["shape"]))
    ws = iter(ws)
    for op in c["ops"]:
        if op[0] == "pool":
            t = g.create_max_pool2d(t, [1, 2, 2, 1], [1, op[1], op[1], 1], "SAME")
            continue
        kern, scale, shift = next(ws)
        if padded:
            t = g.create_conv2d_padded(t, kern, [1, 1, 1, 1], (op[1] // 2, op[1] // 2))
            t = g.create_scale_shift(t, scale, shift)
        else:
            t = g.create_bias_add(g.create_conv2d(t, kern, [1, 1, 1, 1], "SAME"), shift)
        if leaky:  # (the BiasAdd form takes the leaky variant from the Plan: leaky_variant=leaky)
            t = g.create_leaky_relu(t) if leaky == 1 or not padded else g.create_leaky_relu_f32(t)
    g.set_out_node(t)
    return g


def chain_tensors(c, seed, unit_scale):
    """(x, ws): a standard-normal input and per conv a He-scaled kernel, a scale (ones with
    unit_scale; else magnitudes from 2^-6 to 2^6 with every third channel negative and channels 1
    and 5 exactly zero) and a nonzero shift."""
    rng = np.random.default_rng(71000 + seed)
    x = rng.standard_normal((c["B"],) + c["shape"]).astype(np.float32)
    ws, cin = [], c["shape"][2]
    for op in c["ops"]:
        if op[0] != "conv":
            continue
        _, k, oc = op
        kern = (rng.standard_normal((k, k, cin, oc)) * np.sqrt(2.0 / (k * k * cin))).astype(np.float32)
        shift = rng.uniform(0.25, 1.5, oc).astype(np.float32) * rng.choice(np.float32([-1, 1]), oc)
        if unit_scale:
            scale = np.ones(oc, np.float32)
        else:
            scale = np.exp2(rng.integers(-6, 7, oc)).astype(np.float32) * rng.uniform(1, 2, oc).astype(np.float32)
            scale[::3] *= np.float32(-1)
            scale[[1, 5]] = 0
        ws.append((kern, scale, shift.astype(np.float32)))
        cin = oc
    return x, ws


def chain_oracle(c, x, ws, leaky):
    """The chain in float64 per layer (tests/darknet_oracle.py), every layer's output fp32."""
    import darknet_oracle as DO
    import ref_numpy as R
    y = np.asarray(x, np.float32)
    ws = iter(ws)
    for op in c["ops"]:
        if op[0] == "pool":
            y = R.max_pool2d(y, [1, 2, 2, 1], [1, op[1], op[1], 1], "SAME")
            continue
        kern, scale, shift = next(ws)
        y = DO.affine_leaky(DO.conv_padded(y, kern, 1, op[1] // 2, op[1] // 2), scale, shift, leaky == 2)
        assert leaky in (0, 2)
    return y


def check_chain_lines(c, text):
    convs = [l for l in text.splitlines() if l.startswith("conv ")]
    assert len(convs) == len(c["lines"]), text
    for line, tokens in zip(convs, c["lines"]):
        for t in tokens:
            assert t in line, (t, line)
    return convs
