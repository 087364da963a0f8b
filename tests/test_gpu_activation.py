"""GPU: logistic, swish and mish against their float64 definitions (tests/act_oracle.py): the element-wise
kernel, the fused epilogues (bit-equal to it), the pool rule, and a narrow full YOLOv4 through the importer."""
import numpy as np
import pytest

import act_oracle as AO
import darknet_import as D
import dnn_hip
import post_head_cases as HK
import post_multi_oracle as MO
import post_xy_oracle as XO
import ref_numpy as R
import v4tiny_cases as VK
from dnn_hip import ActivationEntry as Act, ReleaseEntry, RestoreEntry, ShortcutEntry, StashEntry

pytestmark = pytest.mark.gpu
F32 = np.float32
# twice the largest error measured on the MI355X over SWEEP, in fp32 ulps (activations); ceiling 16
MAX_ULP = {"logistic": 2 * 1.654, "swish": 2 * 2.177, "mish": 2 * 3.169}
# a dense sweep, +-0, expf's overflow and underflow edges, FLT_MAX, mish's two cut-offs and their fp32 neighbours
SWEEP = np.concatenate([np.linspace(-30, 30, 4002), [0.0, -0.0, 88, -88, 104, -104, 1e4, -1e4, np.finfo(F32).max],
                        [np.nextafter(F32(c), F32(d)) for c in (-0.6, 9.02) for d in (-99, c, 99)]]).astype(F32)


@pytest.mark.parametrize("kind", sorted(MAX_ULP))
def test_activate_host_against_the_float64_definition(kind):
    out = np.empty_like(SWEEP)  # (4017 values, not a multiple of 4: the scalar tail runs)
    assert dnn_hip.mylib.dnn_activate_host(dnn_hip._vp(SWEEP), dnn_hip._vp(out), SWEEP.size, dnn_hip.ACTIVATIONS[kind]) == 0
    err = AO.ulp_err(out, AO.act64(kind, SWEEP))
    print(f"{kind}: max error {err.max():.3f} ulp at v = {SWEEP[err.argmax()]!r}")
    assert np.isfinite(out).all() and err.max() <= MAX_ULP[kind]


def _conv(shape, k, od, pad=1, groups=1, shift=0.0):  # a padded-conv entry with an affine epilogue, seeded by its shape
    rng = np.random.default_rng(k * 1000 + od + shape[3])
    g, cg = dnn_hip.DnnGraphBuilder(), shape[3] // groups
    kernel = (rng.standard_normal((k, k, cg, od)) / np.sqrt(k * k * cg)).astype(F32)
    c = g.create_conv2d_padded(g.create_input(list(shape)), kernel, [1, 1, 1, 1], (pad, pad), groups=groups)
    e = (dnn_hip.GroupedConvEntry if groups > 1 else dnn_hip.PaddedConvEntry)(c, c.pads)
    scale = rng.uniform(0.5, 1.5, od) * np.where(np.arange(od) % 3, 1, -1)
    e.affine = g.create_scale_shift(c, scale, rng.standard_normal(od) * 0.3 + shift)
    return e


def _pool(shape, k, s):
    g = dnn_hip.DnnGraphBuilder()
    return dnn_hip.PoolEntry(g.create_max_pool2d(g.create_input(list(shape)), [1, k, k, 1], [1, s, s, 1], "SAME"))


def _run(shape, entries, x=None):
    x = np.random.default_rng(7).standard_normal(shape).astype(F32) if x is None else x
    plan = dnn_hip.Plan(shape[0], shape[1:], entries)
    return plan.run_host(x), plan.describe(), [k["name"] for k in plan.kernels()]


PATHS = {  # name: (input shape, entries before the activation, what the fused lowering must show)
    "gemm": ((2, 9, 11, 3), lambda s: [_conv(s, 3, 8)], "mode=gemm"),
    "implicit": ((2, 9, 11, 32), lambda s: [_conv(s, 3, 40)], "mode=implicit"),
    "x3": ((2, 8, 8, 32), lambda s: [_pool(s, 1, 1), _conv(s, 3, 64)], "mode=patch_x3"),
    "splitk": ((2, 5, 4, 256), lambda s: [_conv(s, 3, 512)], "splitK=3 combine"),
    "grouped": ((2, 9, 11, 16), lambda s: [_conv(s, 3, 16, groups=2)], "mode=grouped_mfma"),
    "shortcut": ((2, 9, 11, 32), lambda s: [StashEntry(0), _conv(s, 1, 32, pad=0), ShortcutEntry(0), ReleaseEntry(0)],
                 "shortcut 9x11x32 slot=0"),
}


@pytest.mark.parametrize("kind", ("mish", "logistic"))
@pytest.mark.parametrize("path", sorted(PATHS))
def test_fused_epilogue_equals_the_standalone_kernel_bit_for_bit(path, kind):
    shape, before, shows = PATHS[path]
    fused, text, names = _run(shape, before(shape) + [Act(kind)])
    line = [l for l in text.splitlines() if shows in l]
    assert line and line[0].endswith("act=" + kind) and not any(n.startswith("activate") for n in names), text
    plain, text, names = _run(shape, before(shape) + [StashEntry(0), RestoreEntry(0), Act(kind)])
    assert text.splitlines()[-1].startswith("activate") and names[-1] == "activate0", text
    assert np.array_equal(fused.view(np.uint32), plain.view(np.uint32))
    assert AO.ulp_err(fused, AO.act64(kind, _run(shape, before(shape))[0])).max() <= MAX_ULP[kind]


def test_an_x3_conv_with_mish_writes_the_same_split_planes():
    # the epilogue's split planes feeding a second x3 conv == that conv on the fp32 result split by the pool kernel
    shape, first = PATHS["x3"][:2]
    y1 = _run(shape, first(shape) + [Act("mish")])[0]
    chained, text, _ = _run(shape, first(shape) + [Act("mish"), _conv(y1.shape, 3, 128)])
    assert text.count("mode=patch_x3") == 2, text
    apart = _run(y1.shape, [_pool(y1.shape, 1, 1), _conv(y1.shape, 3, 128)], y1)[0]
    assert np.array_equal(chained.view(np.uint32), apart.view(np.uint32))


@pytest.mark.parametrize("kind", ("mish", "logistic"))
@pytest.mark.parametrize("cin,od", ((3, 16), (16, 32)))  # the direct conv0 kernel's shape, the patch conv1 kernel's
def test_a_pool_behind_a_conv_with_mish_is_its_own_kernel(cin, od, kind):
    shape = (2, 10, 12, cin)
    conv = _conv(shape, 3, od, shift=-1.19)  # pre-activation values on both sides of mish's minimum
    x = np.random.default_rng(7).standard_normal(shape).astype(F32)
    z = R.conv2d(np.pad(x, [(0, 0), (1, 1), (1, 1), (0, 0)]), conv.conv.kernel, padding="VALID", acc=np.float64)
    z = np.asarray(z, np.float64) * conv.affine.scale + conv.affine.shift
    pool = lambda t: t.reshape(2, 5, 2, 6, 2, od).max(axis=(2, 4))  # noqa: E731
    want = pool(AO.act64(kind, z))
    assert (np.abs(want - AO.act64(kind, pool(z))) > 1e-3).any() == (kind == "mish")  # pooling first is wrong for mish only
    got, text, names = _run(shape, [conv, Act(kind), _pool((2, 10, 12, od), 2, 2)], x)
    assert kind != "mish" or ("+pool" not in text and "pool0" in names), text
    assert R.normwise_err(got, want) < 1e-4, R.normwise_err(got, want)


def test_imported_narrow_yolov4_against_the_oracle_and_the_decode(tmp_path):
    cfg = D.cfg_text("yolov4", width=64, height=64, width_div=8, classes=3)
    secs = D.parse_cfg(cfg, D.ACTIVATIONS)
    layers = VK.random_layers(secs)
    for layer in layers:  # gamma x 0.7: the signal neither grows nor dies over 110 random layers (heads' mean |v| 0.3)
        if "scales" in layer:
            layer["scales"] = layer["scales"] * F32(0.7)
    x = np.random.default_rng(5).uniform(0, 1, (2, 64, 64, 3)).astype(F32)
    want = AO.forward(secs, layers, x)
    D.save_weights(tmp_path / "v4.weights", layers)
    m = D.DarknetModel(cfg, str(tmp_path / "v4.weights"), in_shape=[2, 64, 64, 3], score_thr=0.3)
    outs = [o.copy() for o in m.inference(x)]
    assert m.sess._plan is not None and m.sess.plan().describe().count("act=mish") == 72
    assert [o.shape for o in outs] == [w.shape for w in want] == [(2, 8, 8, 24), (2, 4, 4, 24), (2, 2, 2, 24)]
    for o, w in zip(outs, want):
        print(f"imported narrow YOLOv4 {o.shape}: normwise error {R.normwise_err(o, w):.3e}, mean |v| {np.abs(w).mean():.3f}")
        assert np.isfinite(o).all() and R.normwise_err(o, w) < 1e-4
    multi = MO.Multi(tuple(m.head.scales), "logistic")
    rows = m.detect(x, raise_errors=False)
    assert all(not isinstance(r, int) and len(r) > 0 for r in rows), rows
    for i in range(2):
        HK.same_rows(rows[i], XO.detect_or_code([o[i] for o in outs], multi, m.head.scale_x_y, "multi"), f"image {i}")
