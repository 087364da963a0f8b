"""Conv and pool geometry through plans: the cases of tests/test_gpu_geometry.py and the host-only
pieces tests/test_geometry_cases.py checks them with.

The plan ABI takes any kh x kw, any stride_h x stride_w and SAME or VALID padding, and sends
almost all of it to kernels that are generic in geometry; plan_fuzz_cases only draws YOLOv2-tiny's
(3x3 / 1x1 stride-1 SAME convs, 2x2 SAME pools).  Here a block carries its full geometry:

    conv      (kh, kw, sh, sw, padding) or None (a block that is only its pool)
    cin, oc   channels in and out
    epi       "bn", "bn_neg" (every other gamma negative), "bias" or "none"
    pool      None or (kh, kw, sh, sw, padding): a pool behind the conv
    pre_pool  None or the same form: a pool in front of the conv
    add       None or the index of an earlier block whose output is added to this block's
              (dnn_hip.Add after the epilogue: stash / shortcut / release in the plan)

NAMED holds hand-written cases, each pinned to one dispatch path at the smallest shape that still
has every edge (a ragged last M tile, a ragged N, an image boundary inside a tile, B >= 2);
geometry_case(seed) draws NSEEDS more.  `paths` lists, per case, tokens that the describe() lines
of the layers under test must contain; lower_host gives those lines without a GPU."""
import ctypes

import numpy as np

import ref_numpy as R

KINDS = ("fp32", "latency", "fp16")
NSEEDS = 48
EPIS = ("bn", "bn_neg", "bias", "none")
MAX_FLOPS = 5e8
X3_MODES = ("patch_x3", "x3_lat", "x3_ktile", "x3_img")

KERNELS = ((1, 1), (3, 3), (5, 5), (1, 5), (5, 1), (2, 2), (3, 1), (7, 7))
STRIDES = (1, 2, 3)
POOLS = (None, (2, 2, 2, 2, "SAME"), (2, 2, 1, 1, "SAME"), (3, 3, 2, 2, "SAME"), (3, 3, 1, 1, "SAME"),
         (2, 2, 2, 2, "VALID"))
CHANNELS = (3, 5, 16, 32, 64, 96)
OUT_CHANNELS = (16, 24, 32, 64, 125, 128)
BATCHES = (1, 2, 3)


def block(conv, cin, oc, epi="bn", pool=None, pre_pool=None, add=None):
    geom = lambda g: None if g is None else (int(g[0]), int(g[1]), int(g[2]), int(g[3]), str(g[4]))
    assert (conv is None) == (oc is None)
    return {"conv": geom(conv), "cin": int(cin), "oc": int(cin if oc is None else oc), "epi": str(epi),
            "pool": geom(pool), "pre_pool": geom(pre_pool), "add": add}


def sq(k, s=1, padding="SAME"):
    return (k, k, s, s, padding)


# ------------------------------------------------------------------------------ shapes
def out_hw(h, w, geom):
    """Output frame and front pads of one conv or pool: (oh, ow, pt, pl)."""
    kh, kw, sh, sw, padding = geom
    oh, pt, _ = R.get_out_pads(h, kh, sh, padding)
    ow, pl, _ = R.get_out_pads(w, kw, sw, padding)
    return oh, ow, pt, pl


def ops(shape, blocks):
    """The convs and pools of a case in plan order: dicts with type "conv" / "pool", the block's
    index, the input H, W, C, the geometry, the output oh, ow, oc and the front pads pt, pl."""
    h, w, c = shape
    out = []
    for i, b in enumerate(blocks):
        assert c == b["cin"], (i, c, b)
        for typ, g in (("pool", b["pre_pool"]), ("conv", b["conv"]), ("pool", b["pool"])):
            if g is None:
                continue
            oh, ow, pt, pl = out_hw(h, w, g)
            oc = b["oc"] if typ == "conv" else c
            out.append({"type": typ, "block": i, "H": h, "W": w, "C": c, "kh": g[0], "kw": g[1], "sh": g[2],
                        "sw": g[3], "padding": g[4], "oh": oh, "ow": ow, "oc": oc, "pt": pt, "pl": pl})
            h, w, c = oh, ow, oc
    return out


def out_shape(shape, blocks):
    o = ops(shape, blocks)[-1]
    return o["oh"], o["ow"], o["oc"]


def conv_flops(B, shape, blocks):
    return sum(2.0 * B * o["oh"] * o["ow"] * o["kh"] * o["kw"] * o["C"] * o["oc"] for o in ops(shape, blocks)
               if o["type"] == "conv")


def fp16_ok(blocks):
    """The fp16 path takes convs with C % 8 == 0 and at most 30 taps, pools with C % 8 == 0, no slots."""
    for b in blocks:
        if b["add"] is not None or b["cin"] % 8:
            return False
        if b["conv"] is not None and b["conv"][0] * b["conv"][1] > 30:
            return False
        if b["pool"] is not None and b["oc"] % 8:
            return False
    return True


# ------------------------------------------------------------------------------ graph, oracle
def _pool_args(g):
    return [1, g[0], g[1], 1], [1, g[2], g[3], 1], g[4]


def graph(B, shape, blocks, ws):
    """The case as a builder graph (ws: per block (kernel HWIO, bias, (mean, var, gamma), leaky),
    None for a pool-only block)."""
    import dnn_hip
    g = dnn_hip.DnnGraphBuilder()
    y = g.create_input([B] + list(shape))
    outs = []
    for b, w in zip(blocks, ws):
        if b["pre_pool"] is not None:
            y = g.create_max_pool2d(y, *_pool_args(b["pre_pool"]))
        if b["conv"] is not None:
            kern, bias, bn, leaky = w
            y = g.create_conv2d(y, kern, [1, b["conv"][2], b["conv"][3], 1], b["conv"][4])
            if bias is not None:
                y = g.create_bias_add(y, bias)
            if bn is not None:
                y = g.create_batch_norm(y, *bn, 1e-5)
            if leaky:
                y = g.create_leaky_relu(y)
        if b["add"] is not None:
            y = g.create_add([outs[b["add"]], y])
        if b["pool"] is not None:
            y = g.create_max_pool2d(y, *_pool_args(b["pool"]))
        outs.append(y)
    g.set_out_node(y)
    return g


def oracle_block(x, b, w, skip=None, tamper=False):
    """One block with float64 accumulation: [pool] conv [bias] [bn] [leaky] [+ skip] [pool].
    tamper: row 0 of image 0 of the conv as if every tap had read zero (what an input fetch that
    takes in-frame taps for padding computes there)."""
    y = np.asarray(x, np.float32)
    if b["pre_pool"] is not None:
        y = R.max_pool2d(y, *_pool_args(b["pre_pool"]))
    if b["conv"] is not None:
        kern, bias, bn, leaky = w
        y = R.conv2d(y, kern, strides=(1, b["conv"][2], b["conv"][3], 1), padding=b["conv"][4])
        if tamper:
            y[0, 0] = 0.0
        if bias is not None:
            y = R.bias_add(y, bias)
        if bn is not None:
            y = R.batch_norm(y, *bn, 1e-5)
        if leaky:
            y = R.leaky_relu(y)
    if b["add"] is not None:
        y = (y + np.asarray(skip, np.float32)).astype(np.float32)
    if b["pool"] is not None:
        y = R.max_pool2d(y, *_pool_args(b["pool"]))
    return y


def oracle_chain(x, blocks, ws):
    """Every block's output, each from the oracle's own previous one."""
    outs = []
    for b, w in zip(blocks, ws):
        x = oracle_block(x, b, w, skip=None if b["add"] is None else outs[b["add"]])
        outs.append(x)
    return outs


# ------------------------------------------------------------------------------ tensors
def case_tensors(seed, B, shape, blocks):
    """Two seeded standard-normal inputs [B, H, W, C] and He-scaled weights per block."""
    rng = np.random.default_rng(93000 + int(seed))
    X = rng.standard_normal((B,) + tuple(shape)).astype(np.float32)
    X2 = rng.standard_normal((B,) + tuple(shape)).astype(np.float32)
    ws = []
    for b in blocks:
        if b["conv"] is None:
            ws.append(None)
            continue
        kh, kw = b["conv"][:2]
        c, oc = b["cin"], b["oc"]
        kern = (rng.standard_normal((kh, kw, c, oc)) * np.sqrt(2.0 / (kh * kw * c))).astype(np.float32)
        bias = (rng.standard_normal(oc) * 0.1).astype(np.float32) if b["epi"] != "none" else None
        bn = None
        if b["epi"].startswith("bn"):
            gamma = rng.uniform(0.5, 1.5, oc).astype(np.float32)
            if b["epi"] == "bn_neg":
                gamma[::2] *= -1.0
            bn = ((rng.standard_normal(oc) * 0.1).astype(np.float32), rng.uniform(0.5, 1.5, oc).astype(np.float32),
                  gamma)
        ws.append((kern, bias, bn, b["epi"] != "none"))
    return X, X2, ws


def exact_tensors(seed, B, shape, blocks):
    """Small integers: inputs in [-4, 4] (none zero in the two top rows and the two left columns),
    weights in [-2, 2], an integer bias where the block has an epilogue, no BatchNorm and no leaky.
    Every partial sum is an integer below 2^24, so the fp32 MFMA in any order, the three-piece bf16
    split and the float64 oracle give the same bits."""
    rng = np.random.default_rng(94000 + int(seed))
    xs = []
    for _ in range(2):
        x = rng.integers(-4, 5, (B,) + tuple(shape)).astype(np.float32)
        for edge in (x[:, :2], x[:, :, :2]):
            edge[edge == 0] = 1.0
        xs.append(x)
    ws = []
    for b in blocks:
        if b["conv"] is None:
            ws.append(None)
            continue
        kh, kw = b["conv"][:2]
        kern = rng.integers(-2, 3, (kh, kw, b["cin"], b["oc"])).astype(np.float32)
        bias = rng.integers(-3, 4, b["oc"]).astype(np.float32) if b["epi"] != "none" else None
        ws.append((kern, bias, None, False))
    return xs[0], xs[1], ws


def zero_tensors(blocks):
    """Weights of the right shapes and nothing else: for lowering only."""
    ws = []
    for b in blocks:
        if b["conv"] is None:
            ws.append(None)
            continue
        z = np.zeros(b["oc"], np.float32)
        ws.append((np.zeros(b["conv"][:2] + (b["cin"], b["oc"]), np.float32), z if b["epi"] != "none" else None,
                   (z, z, z) if b["epi"].startswith("bn") else None, b["epi"] != "none"))
    return ws


# ------------------------------------------------------------------------------ host-only lowering
def lower_host(kind, B, shape, blocks):
    """Lower a case through lower_graph and the C ABI with kernel = NULL (shapes only, no GPU):
    (describe() lines, kernel names).  Every dnn_plan_add_* must return 0."""
    import dnn_hip
    lib = dnn_hip.mylib
    entries = dnn_hip.lower_graph(graph(B, shape, blocks, zero_tensors(blocks)))
    assert entries is not None, blocks
    h = ctypes.c_void_p()
    assert lib.dnn_plan_create(B, *shape, ctypes.byref(h)) == 0
    try:
        assert lib.dnn_plan_set_precision(h, 1 if kind == "fp16" else 0) == 0
        assert lib.dnn_plan_set_latency_mode(h, 1 if kind == "latency" else 0) == 0
        one = ctypes.c_void_p(1)  # presence flags only: nothing is read without a kernel
        for e in entries:
            if dnn_hip._add_structural(lib, h, e):
                continue
            if isinstance(e, dnn_hip.ConvEntry):
                kh, kw, _, od = e.conv.kernel.shape
                bn = one if e.bn is not None else None
                rc = lib.dnn_plan_add_conv(h, kh, kw, od, int(e.conv.strides[1]), int(e.conv.strides[2]),
                                           dnn_hip._pad_code(e.conv.padding), None, one if e.bias is not None else None,
                                           bn, bn, bn, 1e-5, 1 if e.leaky else 0)
            else:
                p = e.pool
                rc = lib.dnn_plan_add_max_pool(h, int(p.ksize[1]), int(p.ksize[2]), int(p.strides[1]),
                                               int(p.strides[2]), dnn_hip._pad_code(p.padding))
            assert rc == 0, dnn_hip.last_error()
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


def layer_config(line):
    """What decides a conv's arithmetic: mode, tile config and K split (other lines: their kind)."""
    f = line.split()
    if f[0] != "conv":
        return (f[0],)
    return tuple(t for t in f if t.startswith(("mode=", "cfg=", "splitK=")))


def annotate(lines, shape, blocks):
    """describe() lines joined with the geometry they run: a list of records, one per conv or
    separate pool line, {"line", "type", "op" (ops() entry), "mode" (convs), "fused" (the ops()
    entry of a pool fused into the conv, or None), "split" (bool), "next" (the following record)}.
    describe() prints neither stride_w nor the pads; they come from the case."""
    todo = ops(shape, blocks)
    recs = []
    for ln in lines:
        f = ln.split()
        if f[0] not in ("conv", "pool"):
            continue
        op = todo.pop(0)
        assert op["type"] == f[0], (ln, op)
        assert f[1] == "%dx%dx%d" % (op["H"], op["W"], op["C"]), (ln, op)
        rec = {"line": ln, "type": f[0], "op": op, "mode": None, "fused": None, "split": False, "next": None}
        if f[0] == "conv":
            rec["mode"] = [t for t in f if t.startswith("mode=")][0][5:]
            rec["split"] = any(t.startswith("splitK=") for t in f)
            if "+pool2x2s2" in f or "+pool2x2s1" in f:
                rec["fused"] = todo.pop(0)
                assert rec["fused"]["type"] == "pool", ln
        if recs:
            recs[-1]["next"] = rec
        recs.append(rec)
    assert not todo, (lines, todo)
    return recs


def coverage_rows(kind, recs):
    """The rows of the coverage table (tests/test_geometry_cases.py) that these records reach."""
    rows = set()
    for r in recs:
        op = r["op"]
        strided = op["sh"] > 1 or op["sw"] > 1
        if r["type"] == "conv":
            if r["mode"] == "implicit" and strided:
                rows.add("fp16 implicit stride > 1" if kind == "fp16" else "implicit stride > 1")
            if r["mode"] == "implicit" and kind != "fp16" and (op["pt"] >= 2 or op["pl"] >= 2) and op["C"] % 32 == 0:
                rows.add("implicit pad >= 2, C % 32 == 0")
            if r["mode"] == "implicit" and kind != "fp16" and r["fused"] is not None and strided:
                rows.add("implicit + fused pool, stride > 1")
            if r["mode"] == "gemm" and strided:
                rows.add("explicit gemm stride > 1")
            nx = r["next"]
            if r["mode"] in X3_MODES and r["split"] and nx is not None and nx["type"] == "pool" and \
                    (nx["op"]["kh"], nx["op"]["kw"]) != (2, 2):
                rows.add("x3 split + pool not 2x2")
        else:
            if (op["kh"], op["kw"]) != (2, 2):
                rows.add("separate pool not 2x2")
            nx = r["next"]
            if nx is not None and nx["type"] == "conv" and nx["mode"] in X3_MODES and nx["op"]["C"] != 16:
                rows.add("pool feeding an x3 conv")
    return rows


ROWS = ("implicit stride > 1", "implicit pad >= 2, C % 32 == 0", "implicit + fused pool, stride > 1",
        "explicit gemm stride > 1", "separate pool not 2x2", "pool feeding an x3 conv", "x3 split + pool not 2x2",
        "fp16 implicit stride > 1")


# ------------------------------------------------------------------------------ named cases
def _case(name, B, shape, blocks, layer, path, pad2=False, more=()):
    """`path`: tokens that the fp32 batch plan's describe() line number `layer` (counting conv and
    pool lines) must contain, `more` further (layer, tokens) pairs; pad2: a front pad of 2 on a
    conv whose input fetch is buffer-addressed (C % 32 == 0)."""
    return {"name": name, "B": B, "shape": tuple(shape), "blocks": blocks,
            "paths": ((layer, tuple(path)),) + tuple((l, tuple(t)) for l, t in more), "pad2": pad2}


NAMED = [
    _case("down_even", 3, (12, 10, 32), [block(sq(3, 2), 32, 64)], 0, ["k3x3", "s2", "mode=implicit"]),
    _case("down_odd", 2, (11, 9, 64), [block(sq(3, 2), 64, 128)], 0, ["k3x3", "s2", "mode=implicit"]),
    _case("down_block", 3, (12, 10, 32),
          [block(sq(3, 2), 32, 64), block(sq(1), 64, 32), block(sq(3), 32, 64, add=0)], 0,
          ["k3x3", "s2", "mode=implicit"]),
    _case("down_pool", 2, (16, 16, 32), [block(sq(3, 2), 32, 64, pool=(2, 2, 2, 2, "SAME"))], 0,
          ["s2", "mode=implicit", "+pool2x2s2"]),
    _case("proj_1x1_s2", 2, (9, 12, 64), [block(sq(1, 2), 64, 128)], 0, ["k1x1", "s2", "mode=implicit"]),
    _case("valid_3x3", 2, (10, 9, 32), [block(sq(3, 1, "VALID"), 32, 48)], 0, ["k3x3", "s1", "mode=implicit"]),
    _case("rect_stride", 2, (9, 11, 32), [block((3, 3, 2, 1, "SAME"), 32, 64)], 0, ["k3x3", "s2", "mode=implicit"]),
    _case("wide5", 2, (9, 11, 32), [block(sq(5), 32, 64)], 0, ["k5x5", "s1", "mode=implicit"], pad2=True),
    _case("wide5_s2", 2, (12, 12, 64), [block(sq(5, 2), 64, 64)], 0, ["k5x5", "s2", "mode=implicit"]),
    _case("wide5_s2_odd", 2, (11, 11, 64), [block(sq(5, 2), 64, 64)], 0, ["k5x5", "s2", "mode=implicit"], pad2=True),
    _case("row_1x5", 2, (7, 13, 32), [block((1, 5, 1, 1, "SAME"), 32, 32)], 0, ["k1x5", "mode=implicit"], pad2=True),
    _case("col_5x1", 2, (7, 13, 32), [block((5, 1, 1, 1, "SAME"), 32, 32)], 0, ["k5x1", "mode=implicit"], pad2=True),
    _case("wide5_c16", 2, (9, 11, 16), [block(sq(5), 16, 32)], 0, ["k5x5", "mode=implicit"]),
    _case("stem7", 2, (20, 18, 3), [block(sq(7, 2), 3, 16, pool=(3, 3, 2, 2, "SAME"))], 0,
          ["k7x7", "s2", "mode=gemm"], more=[(1, ["pool", "k3x3", "s2"])]),
    _case("c5_5x5", 2, (9, 11, 5), [block(sq(5), 5, 24)], 0, ["k5x5", "mode=gemm"]),
    # a separate general-window pool writing the split planes of the x3 conv behind it
    _case("pool3_s2", 2, (13, 13, 32), [block(sq(3), 32, 64, pool=sq(3, 2)), block(sq(3), 64, 128)], 1,
          ["pool", "k3x3", "s2"], more=[(2, ["mode=patch_x3"])]),
    _case("pool3_s1", 2, (13, 13, 32), [block(sq(3), 32, 64, pool=sq(3, 1)), block(sq(3), 64, 128)], 1,
          ["pool", "k3x3", "s1"], more=[(2, ["mode=patch_x3"])]),
    # a 2x2/s2 VALID pool has front pads 0 on any frame, so the plan fuses it (no separate pool
    # kernel): the 13th conv row and column reach no window, and the epilogue writes split planes
    _case("pool2_valid_odd", 2, (13, 13, 32), [block(sq(3), 32, 64, pool=sq(2, 2, "VALID")), block(sq(3), 64, 128)],
          0, ["13x13x32", "6x6x64", "mode=implicit", "+pool2x2s2"], more=[(1, ["mode=patch_x3"])]),
    _case("pool_c6", 2, (7, 9, 6), [block(None, 6, None, pool=(2, 3, 1, 2, "SAME"))], 0, ["pool", "k2x3"]),
    # the K-split x3 conv whose partials the next pool combines at a general window (13 x 13 x 256
    # -> 512 is the smallest shape of the table at which the batch lowering splits: splitK=2)
    _case("x3_split_pool3", 2, (13, 13, 256),
          [block(sq(3), 256, 512, pool=sq(3, 2), pre_pool=sq(2, 1))], 1,
          ["mode=patch_x3", "splitK=", "x3-combine"], more=[(2, ["pool", "k3x3", "s2"])]),
    _case("x3_split_pool3_s1", 1, (13, 13, 256),
          [block(sq(3), 256, 512, "bn_neg", pool=sq(3, 1), pre_pool=sq(2, 1))], 1,
          ["mode=patch_x3", "splitK=", "x3-combine"], more=[(2, ["pool", "k3x3", "s1"])]),
]
NAMES = [c["name"] for c in NAMED]


def named(name):
    return NAMED[NAMES.index(name)]


def named_kinds(case):
    """The plan kinds a named case runs as: fp32 always, fp16 where the fp16 path takes its
    channels, latency where that lowering chooses differently from the batch one."""
    kinds = ["fp32"]
    args = (case["B"], case["shape"], case["blocks"])
    if [layer_config(ln) for ln in lower_host("latency", *args)[0]] != \
            [layer_config(ln) for ln in lower_host("fp32", *args)[0]]:
        kinds.append("latency")
    if fp16_ok(case["blocks"]):
        kinds.append("fp16")
    return kinds


# ------------------------------------------------------------------------------ seeded cases
def _draw_geom(rng, kernels):
    kh, kw = kernels[int(rng.integers(len(kernels)))]
    sh, sw = (int(rng.choice(STRIDES, p=[0.5, 0.3, 0.2])) for _ in range(2))  # (mostly 1: the frame survives 3 blocks)
    return (kh, kw, sh, sw, str(rng.choice(["SAME", "VALID"], p=[0.7, 0.3])))


def _nonempty(h, w, g):
    if g is None:
        return True
    oh, ow, _, _ = out_hw(h, w, g)
    return oh > 0 and ow > 0


def geometry_case(seed):
    """(kind, B, (H, W, C), blocks): 1-3 blocks with independently drawn kernels, strides h and w,
    padding and pools.  Draws whose output would be empty are redrawn; the conv work is capped at
    MAX_FLOPS (B first, then the frame) so that the oracle takes well under a second."""
    kind = KINDS[seed % 3]
    rng = np.random.default_rng(57000 + int(seed))
    f16 = kind == "fp16"
    kernels = [k for k in KERNELS if not (f16 and k[0] * k[1] > 30)]
    chans = [c for c in CHANNELS if not (f16 and c % 8)]
    n = int(rng.choice([1, 2, 3], p=[0.3, 0.4, 0.3]))
    B = int(rng.choice(BATCHES))
    H, W = int(rng.integers(5, 25)), int(rng.integers(5, 25))
    cin = int(rng.choice(chans))
    while True:
        h, w, c = H, W, cin
        blocks = []
        for i in range(n):
            last = i == n - 1
            for _ in range(64):
                pre = POOLS[int(rng.integers(1, len(POOLS)))] if i == 0 and rng.random() < 0.2 else None
                conv = _draw_geom(rng, kernels)
                pool = POOLS[int(rng.integers(len(POOLS)))]
                oc = int(rng.choice(OUT_CHANNELS))
                if f16 and (c % 8 or (pre is not None and c % 8)):
                    continue
                if f16 and oc % 8 and (pool is not None or not last):
                    continue
                hh, ww, ok = h, w, True
                for g in (pre, conv, pool):
                    if g is not None:
                        ok = ok and _nonempty(hh, ww, g)
                        if ok:
                            hh, ww, _, _ = out_hw(hh, ww, g)
                if ok:
                    break
            else:
                pre, conv, pool, oc = None, sq(1), None, 32
                hh, ww = h, w
            epi = str(rng.choice(EPIS, p=[0.5, 0.2, 0.2, 0.1]))
            blocks.append(block(conv, c, oc, epi, pool=pool, pre_pool=pre))
            h, w, c = hh, ww, oc
        if conv_flops(B, (H, W, cin), blocks) <= MAX_FLOPS:
            return kind, B, (H, W, cin), blocks
        if B > 1:
            B -= 1
        else:
            H, W = max(5, H * 3 // 4), max(5, W * 3 // 4)
