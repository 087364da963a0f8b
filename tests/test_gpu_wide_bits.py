"""The wide 3x3 conv kernels bit for bit: conv3x3_f16_acc_kernel (fp16 plans), conv3x3_x3_h2_kernel
(fp32 on two fp16 pieces) and conv3x3_x3_acc2_kernel (fp32 on three bf16 pieces: DNN_HIP_X3_H2=0,
its pooled tail, its split-K form).  Each case is a small chain whose plan must put its convs on the
intended kernel and whose output must have the SHA-256 recorded in golden/wide_conv_bits.json.

The digests pin the arithmetic (products, their order, the epilogue) across changes that are meant
to leave it alone; they were recorded with the library of the commit before the three kernels took
their shared phases from conv_wide_dev.h.  A change that alters the arithmetic on purpose records
them again with the library it trusts, as a plain script (no pytest: conftest.py insists on a
library built from this tree):

    DNN_HIP_LIB=/path/to/trusted/libdnn_hip.so python tests/test_gpu_wide_bits.py --record [--out FILE]

Shapes: the smallest that still cross an image boundary inside a 176-row tile, leave a partial tile,
wrap the skewed LDS rows inside a 16-row fragment (11- and 15-wide padded rows) and use more than
one N panel.  The "lin" chains have convs with a bias only, so the kernels' forms with run-time
epilogue flags run too."""
import functools
import hashlib
import json
import os
import sys

if __name__ == "__main__":  # the recorder: the paths conftest.py would set
    _R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [os.path.join(_R, "tests"), os.path.join(_R, "dnn-inference-engine_amd"), os.path.join(_R, "oracle")]

import numpy as np
import pytest

import dnn_hip
import test_gpu_x3_h2 as H2
from test_gpu_parity import PATCH16_CASES, X3_CASES, X3_CHAIN_CASES, X3_POOL_CASES

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wide_conv_bits.json")
S1 = ([1, 2, 2, 1], [1, 1, 1, 1], "SAME")
S2 = ([1, 2, 2, 1], [1, 2, 2, 1], "SAME")
H2OFF = {"DNN_HIP_X3_H2": "0"}


def _two(case):
    """test_gpu_parity's (B, H, W, C, od1, od2) chains: pool s1 -> two 3x3 convs with BatchNorm."""
    B, H, W, C, od1, od2 = case
    return (B, H, W, C), True, [(od1, "bn", None), (od2, "bn", None)]


# name: (precision, environment, (input shape, leading 2x2/s1 pool, [(od, "bn" | "bias", pool after)]),
#        kernel the plan must choose: ("patch16", convs) | ("h2", layers on h2) | ("x3", convs, text per conv))
CASES = {
    "f16_3x13x13": ("fp16", {}, _two(PATCH16_CASES[1]), ("patch16", 2)),
    "f16_2x9x11": ("fp16", {}, _two(PATCH16_CASES[2]), ("patch16", 2)),
    "f16_lin": ("fp16", {}, ((2, 9, 11, 64), True, [(256, "bias", None), (256, "bias", None)]), ("patch16", 2)),
    "h2_a": ("fp32", {}, "a", ("h2", H2.CASES["a"][3])),
    "h2_b": ("fp32", {}, "b", ("h2", H2.CASES["b"][3])),
    "h2_c": ("fp32", {}, "c", ("h2", H2.CASES["c"][3])),
    "h2_lin": ("fp32", {}, ((2, 9, 11, 32), True, [(256, "bn", None), (256, "bias", None)]), ("h2", [1])),
    "x3_3x13x13": ("fp32", H2OFF, _two(X3_CASES[1]), ("x3", 2, {})),
    "x3_2x9x11": ("fp32", H2OFF, _two(X3_CASES[2]), ("x3", 2, {})),
    # test_x3_pool_fused_vs_oracle's smallest: the pooled tail (ragged windows), then two K slices
    "x3_pool": ("fp32", H2OFF, (X3_POOL_CASES[1], True, [(256, "bn", S2), (512, "bn", S1)]),
                ("x3", 2, {0: "+pool2x2s2", 1: "splitK=2 x3-combine"})),
    # test_x3_split_combine_and_producer_vs_oracle's smallest: raw partials and a combine kernel
    "x3_split": ("fp32", dict(H2OFF, DNN_HIP_X3_IMG="0"),
                 (X3_CHAIN_CASES[1][:4], False, [(128, "bn", S2), (512, "bn", None), (256, "bn", None)]),
                 ("x3", 2, {1: "splitK=2 x3-combine"})),
    "x3_lin": ("fp32", H2OFF, ((2, 9, 11, 32), True, [(256, "bias", None), (256, "bias", None)]), ("x3", 2, {})),
    "x3_pool_lin": ("fp32", H2OFF, ((3, 13, 13, 64), True, [(256, "bias", S2), (256, "bias", None)]),
                    ("x3", 2, {0: "+pool2x2s2"})),
}


@functools.lru_cache(maxsize=None)
def _chain(name):
    """(x, graph builder) of a case; every fifth BatchNorm gamma negative (a decreasing epilogue:
    the fused pools take the window's minimum there)."""
    chain = CASES[name][2]
    if isinstance(chain, str):  # test_gpu_x3_h2's case
        x, layers = H2._case(chain)
        return x, lambda: H2._graph(chain, x.shape, layers)
    shape, lead, convs = chain
    rng = np.random.default_rng(int.from_bytes(hashlib.sha256(name.encode()).digest()[:4], "little"))
    x = rng.standard_normal(shape).astype(np.float32)
    layers, c = [], shape[3]
    for od, epi, pool in convs:
        k = (rng.standard_normal((3, 3, c, od)) * np.sqrt(2.0 / (9 * c))).astype(np.float32)
        b = rng.standard_normal(od).astype(np.float32) * np.float32(0.1)
        gam = rng.uniform(0.5, 1.5, od).astype(np.float32)
        gam[::5] *= -1
        bn = (rng.standard_normal(od).astype(np.float32) * np.float32(0.1), rng.uniform(0.5, 1.5, od).astype(np.float32), gam)
        layers.append((k, b, bn if epi == "bn" else None, pool))
        c = od

    def graph():
        g = dnn_hip.DnnGraphBuilder()
        y = g.create_input(list(shape))
        if lead:
            y = g.create_max_pool2d(y, *S1)
        for k, b, bn, pool in layers:
            y = g.create_conv2d(y, k, [1, 1, 1, 1], "SAME")
            y = g.create_bias_add(y, b)
            if bn is not None:
                y = g.create_batch_norm(y, *bn, 1e-5)
                y = g.create_leaky_relu(y)
            if pool is not None:
                y = g.create_max_pool2d(y, *pool)
        g.set_out_node(y)
        return g

    return x, graph


def _routing(name, plan):
    """None if the plan runs the case's convs on the intended kernel, else what it chose."""
    want = CASES[name][3]
    desc, pieces = plan.describe(), plan.pieces()
    conv = [ln for ln in desc.splitlines() if ln.startswith("conv")]
    h2 = [i for i, ln in enumerate(pieces) if ln.endswith("pieces=h2")]
    if want[0] == "patch16":
        ok = desc.count("mode=patch16") == want[1]
    elif want[0] == "h2":
        ok = h2 == want[1]
    else:
        # mode=patch_x3 is also the x3 tile kernels' (N = 64, N % 128 == 0): only N % 256 == 0 on more
        # than 16 channels is the wide kernel (kernels_x3.hip, x3_kind 0)
        shape, _, convs = CASES[name][2]
        chans = [shape[3]] + [od for od, _, _ in convs]
        wide = [chans[i] > 16 and chans[i + 1] % 256 == 0 for i in range(len(convs))][-want[1]:]
        ok = (all(wide) and h2 == [] and desc.count("mode=patch_x3") == want[1]
              and all("mode=patch_x3" in ln for ln in conv[-want[1]:]) and all(t in conv[i] for i, t in want[2].items()))
    return None if ok else "%s\n%s" % (desc, pieces)


def _run(name, setenv):
    """(routing complaint or None, digest record) of a case under its environment."""
    precision, env, _, _ = CASES[name]
    for k in ("DNN_HIP_X3", "DNN_HIP_X3_H2", "DNN_HIP_X3_IMG", "DNN_HIP_PATCH16"):
        setenv(k, env.get(k))
    x, graph = _chain(name)
    kw = {"precision": precision} if precision != "fp32" else {}
    eng = dnn_hip.DnnInferenceEngine(graph(), False, **kw)
    y = np.ascontiguousarray(eng.run(x))
    return _routing(name, eng.plan()), {"shape": list(y.shape), "dtype": str(y.dtype),
                                        "sha256": hashlib.sha256(y.tobytes()).hexdigest()}


@functools.lru_cache(maxsize=None)
def _golden():
    with open(GOLDEN) as f:
        return json.load(f)["cases"]


@pytest.mark.parametrize("name", sorted(CASES))
def test_wide_conv_bits(monkeypatch, name):
    def setenv(k, v):
        monkeypatch.delenv(k, raising=False) if v is None else monkeypatch.setenv(k, v)

    bad, rec = _run(name, setenv)
    assert bad is None, bad
    assert rec == _golden()[name], (name, rec, _golden()[name])


def record(out):
    """Write the digests of every case, computed with the library DNN_HIP_LIB names."""
    def setenv(k, v):
        os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)

    cases, bad = {}, []
    for name in sorted(CASES):
        why, cases[name] = _run(name, setenv)
        print(name, cases[name]["shape"], cases[name]["sha256"][:16], "ok" if why is None else "NOT ON ITS KERNEL\n" + why,
              flush=True)
        if why is not None:
            bad.append(name)
    import ctypes
    lib = dnn_hip.load_library()
    lib.dnn_build_id.restype = ctypes.c_char_p
    with open(out, "w") as f:
        json.dump({"recorded_with_build_id": lib.dnn_build_id().decode(), "cases": cases}, f, indent=1, sort_keys=True)
        f.write("\n")
    if bad:
        sys.exit("not on the intended kernel: %s" % bad)


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--record", action="store_true", required=True)
    ap.add_argument("--out", default=GOLDEN)
    record(ap.parse_args().out)
