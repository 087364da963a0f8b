"""CPU-only checks behind tests/test_gpu_plan_fuzz.py: what the generated plan cases cover
(every seed lowered through the C ABI with kernel = NULL), and that the comparison helpers of
the guarded runner fail on tampered buffers."""
import collections

import numpy as np
import pytest

import plan_fuzz_cases as F
import plan_fuzz_checks as K

REQUIRED = {
    "fp32": ["direct+p2", "gemm", "implicit", "implicit+p2", "implicit+split", "direct_a", "patch_x3",
             "patch_x3+p2", "patch_x3+split", "x3_img+p1", "x3_1x1", "pool_s1", "pool_s2"],
    "latency": ["patch_x3", "x3_ktile", ("x3_ktile+p1", "x3_ktile+p2"), "x3_lat+split", "implicit+p2+split",
                "direct_a+split"],
    "fp16": ["direct+p2", "patch+p2", "implicit", "implicit+p2", "implicit+split", "patch16", "tile16+p2",
             "tile16+p1", "direct_a"],
}


def test_cases_are_valid_and_deterministic():
    for seed in range(F.NSEEDS):
        kind, B, shape, layers = F.chain_case(seed)
        assert (kind, B, shape, layers) == F.chain_case(seed)
        assert kind == F.KINDS[seed % 3] and B in F.BATCHES
        h, w, c = shape
        assert 7 <= h <= 72 and 7 <= w <= 72
        assert F.conv_flops(B, shape, layers) <= F.MAX_FLOPS
        assert c == layers[0]["cin"] and all(a["oc"] == b["cin"] for a, b in zip(layers, layers[1:]))
        assert not any(b["pre_pool"] for b in layers[1:])
        for i, b in enumerate(layers):
            assert b["k"] == 3 or (b["k"] == 1 and i == len(layers) - 1 and i > 0)
            assert b["epi"] in F.EPIS and b["pool"] in (None, "s1", "s2")
            assert b["oc"] in F.WIDTHS or (i == len(layers) - 1 and b["oc"] in F.RAGGED)
            if b["cin"] == 3:
                assert i == 0 and b["oc"] == 16 and b["pool"] == "s2" and not b["pre_pool"]
            else:
                assert b["cin"] in F.WIDTHS
            if kind == "fp16" and b["pool"]:
                assert b["oc"] % 8 == 0
    kinds = collections.Counter(F.chain_case(s)[0] for s in range(F.NSEEDS))
    assert set(kinds.values()) == {F.NSEEDS // 3}


def test_plan_fuzz_cases_cover_the_chooser():
    """Every predecessor-dependent kernel choice of dnn_plan_add_conv / dnn_plan_add_max_pool
    is reached by at least two seeds of its plan kind (tags: plan_fuzz_cases.line_tag)."""
    seeds = {k: collections.defaultdict(set) for k in F.KINDS}
    preds = collections.defaultdict(set)
    pairs = set()
    split_follow = {"pool": set(), "conv": set()}
    cvt = {True: set(), False: set()}
    rows_total, rows_same = 0, 0
    for seed in range(F.NSEEDS):
        kind, B, shape, layers = F.chain_case(seed)
        lines, names = F.lower_host(kind, B, shape, layers)  # asserts dnn_plan_add_* == 0
        if kind == "fp16":
            assert not any("mode=gemm" in ln for ln in lines), (seed, lines)
            cvt["output.cvt" in names].add(seed)
        tags = [F.line_tag(ln) for ln in lines]
        for i, t in enumerate(tags):
            seeds[kind][t].add(seed)
            prev = tags[i - 1] if i else "input"
            pairs.add((kind, prev, t))
            preds[t.split("+")[0]].add(prev)
            if kind == "fp32" and t == "patch_x3+split" and i + 1 < len(tags):
                if tags[i + 1].startswith("pool"):
                    split_follow["pool"].add(seed)
                elif any(n.endswith(".combine") for n in names):
                    split_follow["conv"].add(seed)
        if kind != "latency" and B > 1:  # batch-row check of the GPU test: same mode / cfg / split at B = 1
            one, _ = F.lower_host(kind, 1, shape, layers)
            rows_total += 1
            rows_same += [F.layer_config(ln) for ln in one] == [F.layer_config(ln) for ln in lines]
    for kind in F.KINDS:
        print(kind, {t: len(s) for t, s in sorted(seeds[kind].items())})
    print("distinct predecessor -> layer pairs:", {k: sum(p[0] == k for p in pairs) for k in F.KINDS})
    print("patch_x3+split followed by a pool:", sorted(split_follow["pool"]), "by a conv (convN.combine):",
          sorted(split_follow["conv"]))
    print("fp16 plans with output.cvt:", len(cvt[True]), "without:", len(cvt[False]))
    print(f"batch-row check applies to {rows_same} of {rows_total} non-latency seeds with B > 1")
    for kind, want in REQUIRED.items():
        for t in want:
            alts = t if isinstance(t, tuple) else (t,)
            hit = set().union(*(seeds[kind][a] for a in alts))
            assert len(hit) >= 2, f"{kind}: tag {t} reached by seeds {sorted(hit)}"
    assert split_follow["pool"] and split_follow["conv"], split_follow
    assert cvt[True] and cvt[False]
    for mode in ("patch_x3", "x3_1x1", "patch16", "tile16"):
        assert len(preds[mode]) >= 2, (mode, preds[mode])
    assert 2 * rows_same >= rows_total > 0


# ------------------------------------------------------------ the helpers have teeth
def _output(batch=3, row=40, n=3, seed=0):
    rng = np.random.default_rng(seed)
    y = rng.standard_normal((batch, row)).astype(np.float32)
    flat = np.full(2 * K.GUARD_FLOATS + batch * row, K.CANARY, dtype=np.uint32).view(np.float32)
    flat[K.GUARD_FLOATS:K.GUARD_FLOATS + n * row] = y[:n].reshape(-1)
    return y, flat


def test_helpers_pass_on_untouched_buffers():
    y, flat = _output(n=2)
    K.check_canary(flat, 2, 40, 3, "out")
    K.check_bits(flat[K.GUARD_FLOATS:K.GUARD_FLOATS + 80].reshape(2, 40), y[:2], "y")
    K.check_layer_err(y, y.astype(np.float64), K.LAYER_TOL, "layer")
    K.check_guard(np.full(3 * K.GUARD_BYTES, K.POISON, np.uint8), "ws")
    nan = np.full(4, K.CANARY, np.uint32).view(np.float32)
    assert np.all(np.isnan(nan))
    K.check_bits(nan, nan.copy(), "canaries compare as bits")
    for dt in (np.float32, np.float16):
        assert np.all(np.isnan(np.full(8, K.POISON, np.uint8).view(dt)))
    assert np.all(np.isnan((np.full(2, 0xFFFF, np.uint32) << 16).view(np.float32)))  # bf16 0xFFFF


def test_helpers_catch_one_element_off_by_1e_5():
    y, _ = _output()
    bad = y.copy()
    i = np.unravel_index(np.argmax(np.abs(y)), y.shape)
    bad[i] *= np.float32(1 + 1e-5)
    assert bad[i] != y[i]
    with pytest.raises(AssertionError, match="words differ"):
        K.check_bits(bad, y, "y")
    with pytest.raises(AssertionError, match="normwise error"):
        K.check_layer_err(bad, y, K.LAYER_TOL, "layer")


@pytest.mark.parametrize("where", ["front", "row", "back"])
def test_helpers_catch_one_canary_word(where):
    _, flat = _output(n=2)
    w = flat.view(np.uint32)
    i = {"front": K.GUARD_FLOATS - 1, "row": K.GUARD_FLOATS + 2 * 40 + 7, "back": K.GUARD_FLOATS + 3 * 40}[where]
    w[i] ^= 1  # still a NaN: only the bit pattern tells
    with pytest.raises(AssertionError, match="canary words overwritten"):
        K.check_canary(flat, 2, 40, 3, "out")


@pytest.mark.parametrize("at", [0, K.GUARD_BYTES - 1, -K.GUARD_BYTES, -1])
def test_helpers_catch_one_guard_byte(at):
    buf = np.full(2 * K.GUARD_BYTES + 1000, K.POISON, np.uint8)
    buf[K.GUARD_BYTES:K.GUARD_BYTES + 1000] = 0  # the interior is the plan's to write
    K.check_guard(buf, "ws")
    buf[at] = 0xFE
    with pytest.raises(AssertionError, match="guard overwritten"):
        K.check_guard(buf, "ws")


def test_helpers_catch_one_nan():
    y, _ = _output()
    bad = y.copy()
    bad[1, 5] = np.nan
    with pytest.raises(AssertionError, match="non-finite"):
        K.check_finite(bad, "y")
    with pytest.raises(AssertionError, match="non-finite"):
        K.check_layer_err(bad, y, K.FP16_LAYER_TOL, "layer")
    with pytest.raises(AssertionError, match="words differ"):
        K.check_bits(bad, y, "y")


def test_oracle_block_matches_the_single_layer_oracle():
    kind, B, shape, layers = F.chain_case(11)
    X, _, ws = F.case_tensors(11, B, shape, layers)
    y = K.oracle_block(X, layers[0], ws[0])
    h, w = F.out_frame(shape[0], shape[1], layers[0]["pool"])
    assert y.shape == (B, h, w, layers[0]["oc"]) and y.dtype == np.float32
