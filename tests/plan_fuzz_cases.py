"""Seeded multi-layer plan cases for tests/test_gpu_plan_fuzz.py, and the host-only lowering
that tests/test_plan_fuzz_cases.py uses to check what the cases cover.

chain_case(seed) -> (kind, B, (H, W, C), layers).  `kind` is "fp32", "latency" or "fp16"
(seed % 3).  `layers` is a list of blocks, each a dict

    pre_pool  a 2x2/s1 SAME pool in front of the conv (first block only)
    k         3 or 1: a SAME stride-1 k x k conv `cin` -> `oc`
    epi       "bn", "bn_neg" (every other gamma negative), "bias" or "none"
    pool      None, "s2" or "s1": a 2x2 SAME pool behind the conv

The plan chooses a layer's kernel from its predecessor, its own pool and (latency plans) its
tile count, so the cases are chains: widths from WIDTHS, ragged head widths, odd and even
frames from 7 to 72, batches 1 / 2 / 3 / 5.  A third of the seeds are "ladders" (widths
doubling, every conv pooled, even conv frames, optional 1x1 x 125 head: the pattern the kernels
are specialised to), and part of the rest sits on a 13 x 13 frame behind a pool, where the
whole-image kernels (x3_img, the K-split x3 kernel with a stride-1 pool, the fp16 whole-frame
tile kernel) are chosen.  The conv work of a case is capped at MAX_FLOPS so that the float64
oracle takes about a second: B is reduced first, then the frame."""
import ctypes

import numpy as np

KINDS = ("fp32", "latency", "fp16")
NSEEDS = 96
WIDTHS = (16, 32, 64, 128, 256, 512, 1024)
RAGGED = (125, 30, 200)
BATCHES = (1, 2, 3, 5)
EPIS = ("bn", "bn_neg", "bias", "none")
MAX_FLOPS = 3e9


def _block(k, cin, oc, epi, pool, pre_pool=False):
    return {"pre_pool": bool(pre_pool), "k": int(k), "cin": int(cin), "oc": int(oc), "epi": str(epi),
            "pool": pool}


def _epi(rng):
    return str(rng.choice(EPIS, p=[0.5, 0.2, 0.2, 0.1]))


def out_frame(h, w, pool):
    return ((h + 1) // 2, (w + 1) // 2) if pool == "s2" else (h, w)


def conv_flops(B, shape, layers):
    """Sum of 2 M K N over the convs (M = B OH OW: SAME stride-1 convs keep the frame)."""
    h, w, _ = shape
    total = 0.0
    for b in layers:
        total += 2.0 * B * h * w * b["k"] * b["k"] * b["cin"] * b["oc"]
        h, w = out_frame(h, w, b["pool"])
    return total


def _ladder(rng):
    """Widths doubling, every conv pooled; frames such that every s2-pooled conv sees an even one."""
    n = int(rng.choice([2, 3]))
    pools = ["s2"] * n
    if rng.random() < 0.35:
        pools[-1] = "s1"
    ns2 = pools.count("s2")
    f_end = 13 if rng.random() < 0.5 else int(rng.integers(4, 72 // (1 << ns2) + 1))
    while f_end * (1 << ns2) > 72:
        f_end -= 1
    rgb = rng.random() < 0.3
    c = 3 if rgb else int(rng.choice(WIDTHS[:7 - n]))
    layers = []
    for i in range(n):
        oc = 16 if c == 3 else 2 * c
        layers.append(_block(3, c, oc, _epi(rng), "s2" if c == 3 else pools[i]))
        c = oc
    if rng.random() < 0.5:
        layers.append(_block(1, c, 125, str(rng.choice(["bias", "none"])), None))
    ns2 = sum(b["pool"] == "s2" for b in layers)
    f = f_end * (1 << ns2)
    return (f, f, layers[0]["cin"]), layers, ("ladder", f_end)


def _small13(rng):
    """13 x 13 frames behind a pool, 256 -> 512 (-> 1024 / a 1x1 head), stride-1 pools."""
    c = int(rng.choice([128, 256, 256, 256]))
    pool = [None, "s1", "s2"][int(rng.choice(3, p=[0.3, 0.45, 0.25]))]
    layers = [_block(3, c, 2 * c, _epi(rng), pool, pre_pool=True)]
    c *= 2
    r = rng.random()
    if r < (0.6 if pool is None else 0.4) and pool != "s2":
        layers.append(_block(3, c, min(2 * c, 1024), _epi(rng), None))
        c = min(2 * c, 1024)
    if rng.random() < 0.6 or (pool is None and len(layers) == 1):  # an unpooled conv gets a consumer
        oc = int(rng.choice(RAGGED + (128,)))
        layers.append(_block(1, c, oc, _epi(rng), None))
    return (13, 13, layers[0]["cin"]), layers, ("small13", 13)


def _free(rng):
    n = int(rng.choice([1, 2, 3], p=[0.2, 0.45, 0.35]))
    if rng.random() < 1.0 / 3:
        f = int(rng.choice([13, 26, 52]))
        h, w = f, f
    else:
        h, w = int(rng.integers(7, 71)), int(rng.integers(7, 71))
    layers = []
    if rng.random() < 0.25:
        layers.append(_block(3, 3, 16, _epi(rng), "s2"))
        c = 16
    else:
        c = int(rng.choice(WIDTHS[:6]))
    first = not layers
    while len(layers) < n:
        last = len(layers) == n - 1
        k = 1 if (last and layers and rng.random() < 0.35) else 3
        step = rng.random()
        i = WIDTHS.index(c)
        if step < 0.5:
            oc = WIDTHS[min(i + 1, 6)]
        elif step < 0.7:
            oc = c
        elif step < 0.85:
            oc = WIDTHS[max(i - 1, 0)]
        else:
            oc = int(rng.choice(WIDTHS))
        pool = [None, "s2", "s1"][int(rng.choice(3, p=[0.4, 0.45, 0.15]))]
        if last and rng.random() < 0.3:
            oc = int(rng.choice(RAGGED))
            pool = None  # (fp16 pools need C % 8 == 0)
        layers.append(_block(k, c, oc, _epi(rng), pool, pre_pool=first and not layers and rng.random() < 0.4))
        c = oc
    return (h, w, layers[0]["cin"]), layers, ("free", 0)


def chain_case(seed):
    rng = np.random.default_rng(52000 + int(seed))
    kind = KINDS[seed % 3]
    style = (seed // 3) % 3
    if style == 0:
        shape, layers, (sname, f_end) = _ladder(rng)
    elif rng.random() < 0.45:
        shape, layers, (sname, f_end) = _small13(rng)
    else:
        shape, layers, (sname, f_end) = _free(rng)
    B = int(rng.choice(BATCHES, p=[0.7, 0.1, 0.1, 0.1] if kind == "latency" else [0.25, 0.25, 0.25, 0.25]))
    h, w, c = shape
    while conv_flops(B, (h, w, c), layers) > MAX_FLOPS:
        if B > 1:
            B = BATCHES[BATCHES.index(B) - 1]
        elif sname == "ladder":
            ns2 = sum(b["pool"] == "s2" for b in layers)
            f_end -= 1
            h = w = f_end * (1 << ns2)
        else:
            assert h > 7 or w > 7, (seed, layers)
            h, w = max(7, h * 7 // 8), max(7, w * 7 // 8)
    return kind, B, (h, w, c), layers


def case_tensors(seed, B, shape, layers):
    """Two different seeded standard-normal inputs [B, H, W, C] and, per block, He-scaled
    weights: (kernel HWIO, bias or None, (mean, var, gamma) or None, leaky)."""
    rng = np.random.default_rng(91000 + int(seed))
    X = rng.standard_normal((B,) + tuple(shape)).astype(np.float32)
    X2 = rng.standard_normal((B,) + tuple(shape)).astype(np.float32)
    ws = []
    for b in layers:
        k, c, oc = b["k"], b["cin"], b["oc"]
        kern = (rng.standard_normal((k, k, c, oc)) * np.sqrt(2.0 / (k * k * c))).astype(np.float32)
        bias = (rng.standard_normal(oc) * 0.1).astype(np.float32) if b["epi"] != "none" else None
        bn = None
        if b["epi"].startswith("bn"):
            gamma = rng.uniform(0.5, 1.5, oc).astype(np.float32)
            if b["epi"] == "bn_neg":
                gamma[::2] *= -1.0  # non-increasing epilogue channels: min-pool before the epilogue
            bn = ((rng.standard_normal(oc) * 0.1).astype(np.float32), rng.uniform(0.5, 1.5, oc).astype(np.float32),
                  gamma)
        ws.append((kern, bias, bn, b["epi"] != "none"))
    return X, X2, ws


def lower_host(kind, B, shape, layers):
    """Lower a case through the C ABI with kernel = NULL (shapes only, no GPU):
    (describe() lines, kernel names).  Every dnn_plan_add_* must return 0."""
    import dnn_hip
    lib = dnn_hip.mylib
    h = ctypes.c_void_p()
    assert lib.dnn_plan_create(B, *shape, ctypes.byref(h)) == 0
    try:
        assert lib.dnn_plan_set_precision(h, 1 if kind == "fp16" else 0) == 0
        assert lib.dnn_plan_set_latency_mode(h, 1 if kind == "latency" else 0) == 0
        one = ctypes.c_void_p(1)  # presence flags only: nothing is read without a kernel
        for b in layers:
            if b["pre_pool"]:
                assert lib.dnn_plan_add_max_pool(h, 2, 2, 1, 1, 1) == 0, dnn_hip.last_error()
            bn = one if b["epi"].startswith("bn") else None
            rc = lib.dnn_plan_add_conv(h, b["k"], b["k"], b["oc"], 1, 1, 1, None, one if b["epi"] != "none" else None,
                                       bn, bn, bn, 1e-5, 0 if b["epi"] == "none" else 1)
            assert rc == 0, dnn_hip.last_error()
            if b["pool"]:
                s = 2 if b["pool"] == "s2" else 1
                assert lib.dnn_plan_add_max_pool(h, 2, 2, s, s, 1) == 0, dnn_hip.last_error()
        buf = ctypes.create_string_buffer(8192)
        assert lib.dnn_plan_describe(h, buf, 8192) == 0
        names = []
        for i in range(lib.dnn_plan_num_kernels(h)):
            nm = ctypes.create_string_buffer(64)
            assert lib.dnn_plan_kernel_info(h, i, nm, 64, None, None) == 0
            names.append(nm.value.decode())
        return buf.value.decode().splitlines(), names
    finally:
        lib.dnn_plan_destroy(h)


def line_tag(line):
    """describe() line -> tag: mode [+p2 | +p1] [+split] for a conv, pool_s1 / pool_s2 for a pool."""
    f = line.split()
    if f[0] == "pool":
        return "pool_" + [t for t in f if t in ("s1", "s2")][0]
    tag = [t for t in f if t.startswith("mode=")][0][5:]
    if "+pool2x2s2" in f:
        tag += "+p2"
    if "+pool2x2s1" in f:
        tag += "+p1"
    if any(t.startswith("splitK=") for t in f):
        tag += "+split"
    return tag


def layer_config(line):
    """What decides a conv's arithmetic: mode, tile config and K split (pool lines: the line)."""
    f = line.split()
    if f[0] == "pool":
        return ("pool",)
    return tuple(t for t in f if t.startswith(("mode=", "cfg=", "splitK=")))
