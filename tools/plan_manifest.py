#!/usr/bin/env python3
"""What the plan lowers every known case to, without a device: for each case and arm the weight
and workspace bytes, the kernel count and dnn_plan_describe's text followed by every kernel's name,
repr(flops) and repr(bytes), kept as one SHA-256 per case over all its arms.  Plans are declared (Plan._declared: shapes only, never
finalized), so this runs anywhere the library loads.

    tools/plan_manifest.py --write         rewrite tests/golden/plan_manifest.json
    tools/plan_manifest.py --check         compare with that file (tests/test_plan_manifest_cpu.py does the same)
    tools/plan_manifest.py --dump CASE     the full text of every arm of one case (diff two checkouts' dumps)
    tools/plan_manifest.py --list          case names

Cases: the six models as the CPU tests build them (narrow) and at full width on a 416 frame (the
narrow entries with their output channels scaled back up: declaring reads shapes only), every named
case of tests/geometry_cases.py, every seed of tests/plan_fuzz_cases.py, and the graphs of
route_cases, residual_cases, multi_out_cases and darknet_cases.  Arms: batch 1 / 2 / 64 x fp32 /
latency / fp16 x the default environment and each plan-time switch off on its own.  Where declaring
raises (fork entries in an fp16 plan, ...) the error text is the record.

A record that differs names the case; `--dump CASE` on the two checkouts shows the arm and the line."""
import argparse
import copy
import ctypes
import hashlib
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(REPO, "dnn-inference-engine_amd"), os.path.join(REPO, "oracle"), os.path.join(REPO, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402

import dnn_hip  # noqa: E402

MANIFEST = os.path.join(REPO, "tests", "golden", "plan_manifest.json")
BATCHES = (1, 2, 64)
KINDS = ("fp32", "latency", "fp16")
SWITCHES = ("DNN_HIP_FUSE", "DNN_HIP_PATCH", "DNN_HIP_SPLITK_FUSED", "DNN_HIP_F16_DIRECT_OUT")
ENVS = ("default",) + tuple(s + "=0" for s in SWITCHES)
ARMS = tuple(f"b{b}/{k}/{e}" for b in BATCHES for k in KINDS for e in ENVS)


# ------------------------------------------------------------------------------ cases
class _ShapeOnlyConv(object):
    """What Plan._declared reads of a conv node: the kernel's shape, the strides, the padding."""

    def __init__(self, conv, od):
        kh, kw, ic, _ = conv.kernel.shape
        self.kernel = np.broadcast_to(np.float32(0), (kh, kw, ic, od))
        self.strides, self.padding = conv.strides, getattr(conv, "padding", None)


def _widened(entries, div, n_out):
    """The entries of a model built `div` times narrower, at full width: every conv's output
    channels x div but the heads' (n_out).  Input channels follow from the plan."""
    out = []
    for e in entries:
        if isinstance(e, (dnn_hip.ConvEntry, dnn_hip.PaddedConvEntry)):
            od = e.conv.kernel.shape[3]
            e = copy.copy(e)
            e.conv = _ShapeOnlyConv(e.conv, od if od == n_out else od * div)
        out.append(e)
    return out


def _models():
    import darknet53
    import synth
    import yolo_graph
    import yolov2
    import yolov3
    import yolov3_spp
    import yolov3_tiny
    B = dnn_hip.DnnGraphBuilder
    out = []
    g = yolo_graph.build_graph(B, synth.yolo_zero_weights(), in_shape=(1, 416, 416, 3))[0]
    out.append(("model/yolov2tiny", (416, 416, 3), dnn_hip.lower_graph(g), {}))
    narrow = (
        ("yolov2", yolov2, synth.yolov2_weights, 8, 40, 64),
        ("darknet53", darknet53, synth.darknet53_weights, 8, 24, 64),
        ("yolov3", yolov3, synth.yolov3_weights, 8, 24, 64),
        ("yolov3-spp", yolov3_spp, synth.yolov3_spp_weights, 8, 24, 96),
        ("yolov3-tiny", yolov3_tiny, synth.yolov3_tiny_weights, 4, 24, 96),
    )
    for name, mod, make, div, n_out, size in narrow:
        g = mod.build_graph(B, mod.validate(make(width_div=div, n_out=n_out), n_out), in_shape=(1, size, size, 3))[0]
        es = dnn_hip.lower_graph(g)
        out.append((f"model/{name}", (size, size, 3), es, {}))
        out.append((f"model/{name}@416", (416, 416, 3), _widened(es, div, n_out), {}))
    return out


def _geometry():
    import geometry_cases as GC
    for c in GC.NAMED:
        g = GC.graph(1, c["shape"], c["blocks"], GC.zero_tensors(c["blocks"]))
        yield f"geometry/{c['name']}", c["shape"], dnn_hip.lower_graph(g), {}


def _fuzz():
    import geometry_cases as GC
    import plan_fuzz_cases as FC
    for seed in range(FC.NSEEDS):
        _, _, shape, layers = FC.chain_case(seed)
        blocks = [GC.block(GC.sq(b["k"]), b["cin"], b["oc"], b["epi"],
                           pool=None if b["pool"] is None else GC.sq(2, 2 if b["pool"] == "s2" else 1),
                           pre_pool=GC.sq(2, 1) if b["pre_pool"] else None) for b in layers]
        g = GC.graph(1, shape, blocks, GC.zero_tensors(blocks))
        yield f"fuzz/seed{seed}", shape, dnn_hip.lower_graph(g), {}


def _graphs():
    import multi_out_cases as MC
    import residual_cases as RS
    import route_cases as RC
    ew = RC.exact_weights
    yield "route/fork_join", RC.FORK_JOIN_IN, RC.fork_join_graph(1, RC.fork_join_weights("exact")), {}
    yield "route/fork_join_bn", RC.FORK_JOIN_IN, RC.fork_join_graph(1, RC.fork_join_weights("random")), {}
    yield "route/empty_branch", (8, 8, 32), RC.empty_branch_graph(1, ew(RC.EMPTY_BRANCH_LAYERS)), {}
    yield "route/two_joins", (8, 8, 32), RC.two_joins_graph(1, ew(RC.TWO_JOINS_LAYERS)), {}
    for n in (1, 2, 4):
        yield f"residual/blocks{n}", RS.IN_SHAPE, RS.blocks_graph(1, ew(RS.blocks_layers(n)), n), {}
    yield "residual/blocks2_act", RS.IN_SHAPE, RS.blocks_graph(1, ew(RS.blocks_layers(2)), 2, act_after_add=True), {}
    yield "residual/projection", RS.IN_SHAPE, RS.projection_graph(1, ew(RS.PROJECTION_LAYERS)), {}
    yield "residual/top_down", RS.IN_SHAPE, RS.top_down_graph(1, ew(RS.TOP_DOWN_LAYERS)), {}
    yield "multi_out/tap_chain", MC.IN_SHAPE, MC.tap_chain_graph(1, ew(MC.TAP_CHAIN_LAYERS)), {}
    yield "multi_out/branch", MC.IN_SHAPE, MC.branch_graph(1, ew(MC.BRANCH_LAYERS)), {}
    yield "multi_out/neck", MC.IN_SHAPE, MC.neck_graph(1, ew(MC.NECK_LAYERS)), {}
    yield "multi_out/churn", MC.IN_SHAPE, MC.churn_graph(1, ew(MC.churn_layers())), {}
    yield "multi_out/nested_skips3", MC.IN_SHAPE, MC.nested_skips_graph(1, ew(MC.NESTED_SKIPS_LAYERS), 3), {}


def _darknet():
    import darknet_cases as DC
    import darknet_import as D
    for name, c in DC.MODE_CHAINS.items():
        _, ws = DC.chain_tensors(c, 0, True)
        for padded in (False, True):
            g = DC.chain_graph(dict(c, B=1), ws, padded, 2 if padded else 1)
            yield f"darknet/{name}/{'padded' if padded else 'same'}", c["shape"], g, c["env"]
    for model, (_, size) in DC.NARROW.items():
        secs = D.parse_cfg(DC.narrow_cfg(model))
        g = D.build_graph(dnn_hip.DnnGraphBuilder, secs, DC.darknet_layers(secs), [1, size, size, 3])[0]
        yield f"darknet/{model}", (size, size, 3), g, {}


def cases():
    """[(name, per-image input shape, plan entries, environment of the case's own)]."""
    out = list(_models()) + list(_geometry()) + list(_fuzz())
    for name, shape, g, env in list(_graphs()) + list(_darknet()):
        out.append((name, tuple(shape), dnn_hip.lower_graph(g), env))
    for name, _, es, _ in out:
        assert es is not None, name
    assert len({c[0] for c in out}) == len(out)
    return out


# ------------------------------------------------------------------------------ one arm
class _Env(object):
    def __init__(self, env):
        self.env = env

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.env}
        os.environ.update(self.env)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def arm_text(batch, kind, env, shape, entries, case_env):
    """(weight bytes, workspace bytes, kernel count, text) or the error text of a failed declare."""
    lib = dnn_hip.mylib
    e = dict(case_env)
    if env != "default":
        k, v = env.split("=")
        e[k] = v
    with _Env({s: "1" for s in SWITCHES if s not in e}), _Env(e):
        try:
            h = dnn_hip.Plan._declared(batch, shape, entries, lib, "fp16" if kind == "fp16" else "fp32",
                                       kind == "latency")
        except dnn_hip.DnnHipError as err:
            return str(err)
        try:
            buf = ctypes.create_string_buffer(1 << 17)
            dnn_hip._check(lib.dnn_plan_describe(h, buf, 1 << 17), "dnn_plan_describe", lib)
            wb, sb = ctypes.c_size_t(), ctypes.c_size_t()
            dnn_hip._check(lib.dnn_plan_memory(h, ctypes.byref(wb), ctypes.byref(sb)), "dnn_plan_memory", lib)
            lines = [buf.value.decode()]
            nk = lib.dnn_plan_num_kernels(h)
            for i in range(nk):
                nm = ctypes.create_string_buffer(64)
                fl, by = ctypes.c_double(), ctypes.c_double()
                dnn_hip._check(lib.dnn_plan_kernel_info(h, i, nm, 64, ctypes.byref(fl), ctypes.byref(by)),
                               "dnn_plan_kernel_info", lib)
                lines.append(f"{nm.value.decode()} {fl.value!r} {by.value!r}\n")
            return wb.value, sb.value, nk, "".join(lines)
        finally:
            lib.dnn_plan_destroy(h)


def case_record(shape, entries, case_env):
    """What the fixture keeps of one case: [weight bytes, workspace bytes, kernels] of the batch-64
    fp32 plan in the default environment (for a reader; "error" if it does not declare), and one
    SHA-256 over every arm's dump (arm name, then the error text, or the three numbers and the
    text), in ARMS' order."""
    h, b64 = hashlib.sha256(), None
    for arm, (b, k, e) in zip(ARMS, ((b, k, e) for b in BATCHES for k in KINDS for e in ENVS)):
        r = arm_text(b, k, e, shape, entries, case_env)
        h.update(arm_dump(arm, r).encode())
        if (b, k, e) == (BATCHES[-1], "fp32", "default"):
            b64 = "error" if isinstance(r, str) else list(r[:3])
    return {"b64": b64, "sha256": h.hexdigest()}


def arm_dump(arm, r):
    return f"== {arm}\n" + (r + "\n" if isinstance(r, str) else "weights %d workspace %d kernels %d\n%s" % r)


def compute():
    """{case: record}."""
    return {name: case_record(shape, es, env) for name, shape, es, env in cases()}


def load(path=MANIFEST):
    with open(path) as f:
        m = json.load(f)
    assert tuple(m["arms"]) == ARMS, "the fixture's arms differ from this tool's"
    return m["cases"]


def write(path=MANIFEST):
    got = compute()
    with open(path, "w") as f:  # (one case per line: a later change to the fixture shows as the cases it touches)
        f.write('{"arms": %s,\n "cases": {\n' % json.dumps(list(ARMS)))
        f.write(",\n".join("  %s: %s" % (json.dumps(n), json.dumps(r)) for n, r in got.items()))
        f.write("\n }}\n")
    return len(got)


def differences(want, got):
    """["case: ..."] for every case whose record differs, and for cases only one side has."""
    bad = [f"{n}: only in the {'fixture' if n in want else 'tree'}" for n in sorted(set(want) ^ set(got))]
    return bad + [f"{n}: fixture {want[n]} tree {got[n]}" for n in sorted(set(want) & set(got)) if want[n] != got[n]]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--write", action="store_true")
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--list", action="store_true")
    ap.add_argument("--dump", metavar="CASE")
    a = ap.parse_args()
    if a.write:
        print("wrote %d cases" % write())
    elif a.check:
        bad = differences(load(), compute())
        print("\n".join(bad[:40]) or "manifest matches")
        sys.exit(1 if bad else 0)
    elif a.dump:
        name, shape, es, env = [c for c in cases() if c[0] == a.dump][0]
        for arm, (b, k, e) in zip(ARMS, ((b, k, e) for b in BATCHES for k in KINDS for e in ENVS)):
            print(arm_dump(arm, arm_text(b, k, e, shape, es, env)), end="")
    else:
        for c in cases():
            print(c[0])


if __name__ == "__main__":
    main()
