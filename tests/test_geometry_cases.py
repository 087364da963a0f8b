"""CPU-only checks behind tests/test_gpu_geometry.py: the float64 oracle against torch's float64
conv and pool at every geometry the cases use (and against the C restatement at the named
ones), what the cases reach in the chooser (every case lowered through the C ABI with
kernel = NULL), the preconditions of the exact-integer tensors, and that the comparison helpers
fail on an output computed the way the buffer-addressed input fetch computed it for a top pad of
2 (image 0's first output row with every tap read as zero)."""
import collections
import math

import numpy as np
import pytest
import torch

import geometry_cases as G
import plan_fuzz_checks as K
import ref_numpy as R

F32_LOWEST = -3.4028234663852886e38  # -FLT_MAX


def _all_cases():
    """(label, kind, B, shape, blocks): every named case in each of its kinds, every seed."""
    out = []
    for c in G.NAMED:
        for kind in G.named_kinds(c):
            out.append((c["name"], kind, c["B"], c["shape"], c["blocks"]))
    for seed in range(G.NSEEDS):
        out.append((f"seed {seed}",) + G.geometry_case(seed))
    return out


def _geometries():
    """Every distinct (type, H, W, kh, kw, sh, sw, padding) of the named and seeded cases."""
    seen = {}
    for label, _, _, shape, blocks in _all_cases():
        for o in G.ops(shape, blocks):
            key = (o["type"], o["H"], o["W"], o["kh"], o["kw"], o["sh"], o["sw"], o["padding"])
            seen.setdefault(key, label)
    return sorted(seen.items())


def _same_pads(size, k, s, padding):
    """TensorFlow's SAME / VALID, restated here (not taken from the oracle): (out, front, back)."""
    if padding == "VALID":
        return (size - k) // s + 1, 0, 0
    out = -(-size // s)
    total = max((out - 1) * s + k - size, 0)
    return out, total // 2, total - total // 2


# ------------------------------------------------------------------------------ 1. the oracle
def test_cases_are_valid_and_deterministic():
    kinds = collections.Counter()
    for seed in range(G.NSEEDS):
        kind, B, shape, blocks = G.geometry_case(seed)
        assert (kind, B, shape, blocks) == G.geometry_case(seed)
        kinds[kind] += 1
        assert kind == G.KINDS[seed % 3] and B in G.BATCHES and 1 <= len(blocks) <= 3
        assert 5 <= shape[0] <= 24 and 5 <= shape[1] <= 24
        assert G.conv_flops(B, shape, blocks) <= G.MAX_FLOPS
        assert all(o["oh"] > 0 and o["ow"] > 0 for o in G.ops(shape, blocks))  # (ops() checks the channel chain)
        assert kind != "fp16" or G.fp16_ok(blocks)
        for b in blocks:
            assert b["conv"][:2] in G.KERNELS and b["conv"][2] in G.STRIDES and b["conv"][3] in G.STRIDES
            assert b["pool"] in G.POOLS and b["epi"] in G.EPIS and b["oc"] in G.OUT_CHANNELS
    assert set(kinds.values()) == {G.NSEEDS // 3}
    assert len(set(G.NAMES)) == len(G.NAMES)
    drawn = [b["conv"] for s in range(G.NSEEDS) for b in G.geometry_case(s)[3]]
    assert {g[:2] for g in drawn} == set(G.KERNELS)
    assert any(g[2] != g[3] for g in drawn) and {g[4] for g in drawn} == {"SAME", "VALID"}


def test_oracle_conv_and_pool_equal_torch_float64():
    """ref_numpy.conv2d / max_pool2d against torch.nn.functional in float64 on an input padded
    here with the asymmetric SAME pads (zeros for conv, -FLT_MAX for pool): equal shapes, conv to
    1e-12 relative (its float64 stage, and its fp32 result against torch's rounded to fp32), pool
    bit for bit."""
    rng = np.random.default_rng(5)
    geoms = _geometries()
    assert len(geoms) > 100
    worst = 0.0
    for (typ, H, W, kh, kw, sh, sw, padding), label in geoms:
        what = f"{label}: {typ} {H}x{W} k{kh}x{kw} s{sh}x{sw} {padding}"
        oh, pt, pb = _same_pads(H, kh, sh, padding)
        ow, pl, pr = _same_pads(W, kw, sw, padding)
        C = 3
        x = rng.standard_normal((2, H, W, C)).astype(np.float32)
        fill = 0.0 if typ == "conv" else F32_LOWEST
        xp = np.full((2, H + pt + pb, W + pl + pr, C), fill, np.float64)
        xp[:, pt:pt + H, pl:pl + W] = x
        tx = torch.from_numpy(np.ascontiguousarray(xp.transpose(0, 3, 1, 2)))
        if typ == "conv":
            k = rng.standard_normal((kh, kw, C, 4)).astype(np.float32)
            tk = torch.from_numpy(np.ascontiguousarray(k.transpose(3, 2, 0, 1)).astype(np.float64))
            want = torch.nn.functional.conv2d(tx, tk, stride=(sh, sw)).numpy().transpose(0, 2, 3, 1)
            got = R.conv2d(x, k, strides=(1, sh, sw, 1), padding=padding)
            assert got.shape == want.shape == (2, oh, ow, 4), (what, got.shape, want.shape)
            # conv2d's float64 stage, before its rounding to fp32
            p, oh2, ow2 = R.pad_nhwc(x, kh, kw, sh, sw, padding)
            g64 = (R.im2col(p, kh, kw, sh, sw, oh2, ow2, order="kkc").astype(np.float64) @
                   k.reshape(-1, 4).astype(np.float64)).reshape(2, oh2, ow2, 4)
            scale = np.abs(want).max()
            assert scale > 0, what
            e64 = np.abs(g64 - want).max() / scale
            e32 = np.abs(got.astype(np.float64) - want.astype(np.float32).astype(np.float64)).max() / scale
            worst = max(worst, e64, e32)
            assert e64 <= 1e-12 and e32 <= 1e-12, (what, e64, e32)
        else:
            want = torch.nn.functional.max_pool2d(tx, (kh, kw), stride=(sh, sw)).numpy().transpose(0, 2, 3, 1)
            got = R.max_pool2d(x, [1, kh, kw, 1], [1, sh, sw, 1], padding)
            assert got.shape == want.shape == (2, oh, ow, C), (what, got.shape, want.shape)
            K.check_bits(got, want.astype(np.float32), what)
    print(f"{len(geoms)} geometries, worst conv difference {worst:.2e} relative")


def test_oracle_equals_the_c_restatement_at_the_named_geometries():
    """ref_numpy against oracle/dnn_oracle.c (its conv2d_mul on a host-padded input and its
    max_pool2d) with test_oracle_golden.py's bars: 1e-6 normwise for conv, equal for pool."""
    from oracle_c import OracleC
    oc = OracleC()
    rng = np.random.default_rng(6)
    done = set()
    for c in G.NAMED:
        for o in G.ops(c["shape"], c["blocks"]):
            key = tuple(o[k] for k in ("type", "H", "W", "C", "oc", "kh", "kw", "sh", "sw", "padding"))
            if key in done:
                continue
            done.add(key)
            C = min(o["C"], 8)  # (geometry, not width, is what differs from the golden cases)
            x = rng.standard_normal((2, o["H"], o["W"], C)).astype(np.float32)
            if o["type"] == "conv":
                k = rng.standard_normal((o["kh"], o["kw"], C, 5)).astype(np.float32)
                ref = R.conv2d(x, k, strides=(1, o["sh"], o["sw"], 1), padding=o["padding"])
                xp, oh, ow = R.pad_nhwc(x, o["kh"], o["kw"], o["sh"], o["sw"], o["padding"])
                kr = np.ascontiguousarray(k.transpose(2, 0, 1, 3).reshape(-1, 5))
                yc = oc.conv2d_mul(xp, kr, oh, ow, o["kh"], o["kw"], o["sh"], o["sw"])
                assert yc.shape == ref.shape and R.normwise_err(yc, ref) < 1e-6, (c["name"], o)
                yd = oc.conv2d_direct(xp, k, oh, ow, o["sh"], o["sw"], nthreads=2)
                assert R.normwise_err(yd, ref) < 1e-6, (c["name"], o)
            else:
                args = ([1, o["kh"], o["kw"], 1], [1, o["sh"], o["sw"], 1], o["padding"])
                assert np.array_equal(oc.max_pool2d(x, *args), R.max_pool2d(x, *args)), (c["name"], o)


# ------------------------------------------------------------------------------ 2. coverage
def test_named_cases_reach_their_paths():
    """The fp32 batch plan of every named case holds the layer its table row names."""
    for c in G.NAMED:
        lines, names = G.lower_host("fp32", c["B"], c["shape"], c["blocks"])
        recs = G.annotate(lines, c["shape"], c["blocks"])
        for layer, tokens in c["paths"]:
            have = recs[layer]["line"].split()
            for t in tokens:
                assert any(h == t or (t.endswith("=") and h.startswith(t)) for h in have), (c["name"], t, lines)
        convs = [r for r in recs if r["type"] == "conv"]
        if c["pad2"]:
            assert any(r["mode"] == "implicit" and r["op"]["C"] % 32 == 0 and max(r["op"]["pt"], r["op"]["pl"]) >= 2
                       for r in convs), (c["name"], lines)
    by = {c["name"]: c for c in G.NAMED}

    def first_op(name):
        return G.ops(by[name]["shape"], by[name]["blocks"])[0]

    assert (first_op("down_even")["pt"], first_op("down_even")["pl"]) == (0, 0)
    assert (first_op("down_odd")["pt"], first_op("down_odd")["pl"]) == (1, 1)
    assert (first_op("wide5")["pt"], first_op("wide5")["pl"]) == (2, 2)
    assert (first_op("wide5_s2")["pt"], first_op("wide5_s2")["pl"]) == (1, 1)
    assert (first_op("wide5_s2_odd")["pt"], first_op("wide5_s2_odd")["pl"]) == (2, 2)
    assert (first_op("row_1x5")["pt"], first_op("row_1x5")["pl"]) == (0, 2)
    assert (first_op("col_5x1")["pt"], first_op("col_5x1")["pl"]) == (2, 0)
    assert first_op("rect_stride")["sh"] == 2 and first_op("rect_stride")["sw"] == 1
    lines, names = G.lower_host("fp32", by["down_block"]["B"], by["down_block"]["shape"], by["down_block"]["blocks"])
    assert [ln.split()[0] for ln in lines] == ["conv", "stash", "conv", "conv", "shortcut", "release"], lines
    _, names = G.lower_host("fp32", by["stem7"]["B"], by["stem7"]["shape"], by["stem7"]["blocks"])
    assert names == ["conv0.im2col", "conv0.gemm", "pool0"], names
    # the 1x1 stride-2 projection is not the 1x1-on-the-input shortcut
    assert "mode=direct_a" not in " ".join(G.lower_host("fp32", 2, by["proj_1x1_s2"]["shape"],
                                                        by["proj_1x1_s2"]["blocks"])[0])


def test_geometry_cases_cover_the_chooser():
    """Every case lowers (return code 0 from every dnn_plan_add_*), no fp16 plan holds a conv the
    fp16 path rejects, and each row of the coverage table is reached by at least two cases."""
    hits = collections.defaultdict(list)
    rows_total = rows_same = 0
    for label, kind, B, shape, blocks in _all_cases():
        lines, names = G.lower_host(kind, B, shape, blocks)
        if kind == "fp16":
            assert not any("mode=gemm" in ln for ln in lines), (label, lines)
        for row in G.coverage_rows(kind, G.annotate(lines, shape, blocks)):
            hits[row].append(f"{label} ({kind})")
        if kind != "latency" and B > 1:
            one, _ = G.lower_host(kind, 1, shape, blocks)
            rows_total += 1
            rows_same += [G.layer_config(ln) for ln in one] == [G.layer_config(ln) for ln in lines]
    for row in G.ROWS:
        print(f"{row}: {len(hits[row])}: {hits[row][:8]}")
    print(f"batch-row check applies to {rows_same} of {rows_total} non-latency cases with B > 1")
    for row in G.ROWS:
        assert len(hits[row]) >= 2, (row, hits[row])
    assert 2 * rows_same >= rows_total > 0


# ------------------------------------------------------------------------------ 3. exact tensors
@pytest.mark.parametrize("name", G.NAMES)
def test_exact_case_preconditions(name):
    c = G.named(name)
    X, X2, ws = G.exact_tensors(G.NAMES.index(name), c["B"], c["shape"], c["blocks"])
    for x in (X, X2):
        assert np.array_equal(x, np.rint(x)) and np.abs(x).max() == 4
        assert np.all(x[:, :2] != 0) and np.all(x[:, :, :2] != 0)  # a tap read as zero changes the sum
    for w in ws:
        if w is not None:
            assert np.array_equal(w[0], np.rint(w[0])) and np.abs(w[0]).max() == 2 and w[2] is None and not w[3]
            assert w[1] is None or np.array_equal(w[1], np.rint(w[1]))
    for j, y in enumerate(G.oracle_chain(X, c["blocks"], ws)):
        assert np.array_equal(y, np.rint(y)), (name, j)
        # (a block that is only a pool passes its input's integers on: nothing to accumulate)
        low = 4 if c["blocks"][j]["conv"] is not None else 3
        assert low < np.abs(y).max() < 2 ** 20, (name, j, np.abs(y).max())
    # the bound on any partial sum of any conv: sum |x| |w| over the window, in float64
    a = X
    for b, w, y in zip(c["blocks"], ws, G.oracle_chain(X, c["blocks"], ws)):
        if w is not None:
            if b["pre_pool"] is not None:
                g = b["pre_pool"]
                a = R.max_pool2d(a, [1, g[0], g[1], 1], [1, g[2], g[3], 1], g[4])
            mag = R.conv2d(np.abs(a), np.abs(w[0]), strides=(1, b["conv"][2], b["conv"][3], 1), padding=b["conv"][4])
            assert mag.max() + 3 < 2 ** 24, (name, mag.max())
        a = y


# ------------------------------------------------------------------------------ 4. the helpers have teeth
@pytest.mark.parametrize("name", [c["name"] for c in G.NAMED if c["pad2"]])
@pytest.mark.parametrize("tensors", ["exact", "random"])
def test_helpers_catch_in_frame_taps_read_as_zero(name, tensors):
    """What a conv whose input fetch takes the in-frame taps of image 0, output row 0 for padding
    would give (that row recomputed with every tap zero) fails the bit comparison and the per-layer bar
    of either precision."""
    c = G.named(name)
    make = G.exact_tensors if tensors == "exact" else G.case_tensors
    X, _, ws = make(G.NAMES.index(name), c["B"], c["shape"], c["blocks"])
    good = G.oracle_block(X, c["blocks"][0], ws[0])
    bad = G.oracle_block(X, c["blocks"][0], ws[0], tamper=True)
    assert good.shape == bad.shape and np.array_equal(good[1:], bad[1:]) and np.array_equal(good[0, 1:], bad[0, 1:])
    K.check_bits(good, good.copy(), name)
    K.check_layer_err(good, good.astype(np.float64), K.LAYER_TOL, name)
    with pytest.raises(AssertionError, match="words differ, first at flat index"):
        K.check_bits(bad, good, name)
    for tol in (K.LAYER_TOL, K.FP16_LAYER_TOL):
        with pytest.raises(AssertionError, match="normwise error"):
            K.check_layer_err(bad, good, tol, name)


def test_oracle_block_matches_the_graph_oracle():
    """oracle_chain (block by block) equals residual_cases.oracle_graph on the builder graph, the
    Add of down_block included."""
    import residual_cases as RS
    for name in ("down_block", "stem7", "pool_c6", "pool2_valid_odd"):
        c = G.named(name)
        X, _, ws = G.case_tensors(G.NAMES.index(name), c["B"], c["shape"], c["blocks"])
        want = RS.oracle_graph(G.graph(c["B"], c["shape"], c["blocks"], ws), X)
        got = G.oracle_chain(X, c["blocks"], ws)[-1]
        assert got.shape == (c["B"],) + G.out_shape(c["shape"], c["blocks"])
        K.check_bits(got, want, name)
    assert math.isclose(G.conv_flops(1, (13, 13, 256), G.named("x3_split_pool3_s1")["blocks"]), 2 * 169 * 2304 * 512)
