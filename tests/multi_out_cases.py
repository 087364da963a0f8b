"""TEST INFRASTRUCTURE ONLY — graphs with several outputs (taps) shared by
tests/test_multi_out_cpu.py and tests/test_gpu_multi_out.py, their float64 oracle, and helpers
that read a tap out of a residual_cases.GuardedPlan's poisoned workspace.  Every graph takes
[B, 8, 8, 32]; with route_cases.exact_weights and exact_input every product and sum is a small
integer, so plans are bit-equal to the oracle."""
import numpy as np

import dnn_hip
import plan_fuzz_checks as K
import residual_cases as RS
import route_cases as RC

IN_SHAPE = RS.IN_SHAPE


def entry_kinds(entries):
    """residual_cases.entry_kinds plus T tap."""
    names = {dnn_hip.ConvEntry: "C", dnn_hip.PoolEntry: "P", dnn_hip.StashEntry: "S", dnn_hip.RestoreEntry: "R",
             dnn_hip.RouteEntry: "J", dnn_hip.ShortcutEntry: "A", dnn_hip.ReleaseEntry: "X",
             dnn_hip.UpsampleEntry: "U", dnn_hip.TapEntry: "T"}
    return "".join(names[type(e)] for e in entries)


def numbers(entries):
    """(kind, slot or tap index) of every stash, restore, route, shortcut, release and tap."""
    out = []
    for e, k in zip(entries, entry_kinds(entries)):
        if k in "SRJAX":
            out.append((k, e.slot))
        elif k == "T":
            out.append((k, e.index))
    return out


def max_live_slots(entries):
    live, most = set(), 0
    for e, k in zip(entries, entry_kinds(entries)):
        if k == "S":
            assert e.slot not in live and e.slot == min(set(range(len(live) + 1)) - live)
            live.add(e.slot)
        elif k == "X":
            live.remove(e.slot)
        elif k in "RJA" and e.slot >= 0:
            assert e.slot in live
        most = max(most, len(live))
    return most


def _conv(g, x, w, stride=1):
    x = g.create_conv2d(x, w["kernel"], [1, stride, stride, 1], "SAME")
    return g.create_bias_add(x, w["biases"])


def _input(g, B):
    return g.create_input([B] + list(IN_SHAPE))


# (a) conv - tap - conv: an extra output on the main line
TAP_CHAIN_LAYERS = ((3, 32, 32), (1, 32, 8))


def tap_chain_graph(B, ws):
    g = dnn_hip.DnnGraphBuilder()
    x = _conv(g, _input(g, B), ws[0])
    g.add_out_node(x)
    g.set_out_node(_conv(g, x, ws[1]))
    return g


# (b) output branch: x -> conv -> tap and x -> conv -> primary
BRANCH_LAYERS = ((3, 32, 32), (3, 32, 16), (1, 32, 8))


def branch_graph(B, ws):
    g = dnn_hip.DnnGraphBuilder()
    x = _conv(g, _input(g, B), ws[0])
    g.add_out_node(_conv(g, x, ws[1]))
    g.set_out_node(_conv(g, x, ws[2]))
    return g


# (c) mini-neck: conv/s2 -> x; Add block; conv/s2; conv -> y; y -> conv -> tap 0;
#     y -> conv1x1 -> upsample 2 -> Concat([upsampled, x]) -> conv -> primary
NECK_LAYERS = ((3, 32, 32), (1, 32, 16), (3, 16, 32), (3, 32, 32), (3, 32, 32), (1, 32, 8), (1, 32, 16), (3, 48, 8))
NECK_KINDS = "CSSCCAXCCSCTRXCUJXC"
NECK_NUMBERS = [("S", 0), ("S", 1), ("A", 1), ("X", 1), ("S", 1), ("T", 0), ("R", 1), ("X", 1), ("J", 0), ("X", 0)]


def neck_graph(B, ws):
    g = dnn_hip.DnnGraphBuilder()
    x = _conv(g, _input(g, B), ws[0], stride=2)
    t = g.create_add([x, _conv(g, _conv(g, x, ws[1]), ws[2])])
    t = _conv(g, t, ws[3], stride=2)
    y = _conv(g, t, ws[4])
    g.add_out_node(_conv(g, y, ws[5]))
    u = g.create_upsample(_conv(g, y, ws[6]), 2)
    g.set_out_node(_conv(g, g.create_concat([u, x]), ws[7]))
    return g


# (d) a tap followed by four Add blocks: the stash / release churn beside a region held for good
def churn_layers(nblocks=4):
    return RS.blocks_layers(nblocks)


def churn_graph(B, ws, nblocks=4, tap=True):
    """residual_cases.blocks_graph with the first conv's output as an extra output."""
    g = RS.blocks_graph(B, ws, nblocks)
    if tap:
        first = [n for n in RC.topo_nodes(g) if isinstance(n, dnn_hip.BiasAdd)][0]
        g.add_out_node(first)
    return g


# unsupported: a long skip into an Add; a fifth live slot
def long_skip_add_graph(B, ws):
    """x -> Add block -> Add([., x]): x skips over a whole block into an Add."""
    g = dnn_hip.DnnGraphBuilder()
    x = _conv(g, _input(g, B), ws[0])
    t = _conv(g, x, ws[3])
    t = g.create_add([t, _conv(g, _conv(g, t, ws[1]), ws[2])])
    g.set_out_node(_conv(g, g.create_add([t, x]), ws[4]))
    return g


LONG_SKIP_ADD_LAYERS = ((3, 32, 32), (1, 32, 16), (3, 16, 32), (3, 32, 32), (1, 32, 8))


def nested_skips_graph(B, ws, depth):
    """`depth` long skips open at once (x_i = conv(x_{i-1}), each concatenated later, innermost
    first), then an Add block inside all of them: depth + 1 live slots."""
    g = dnn_hip.DnnGraphBuilder()
    t = _input(g, B)
    xs = []
    for _ in range(depth):
        t = _conv(g, t, ws[0])
        xs.append(t)
        t = _conv(g, t, ws[0])
    t = g.create_add([t, _conv(g, _conv(g, t, ws[1]), ws[2])])
    for x in reversed(xs):
        t = _conv(g, g.create_concat([t, x]), ws[3])
    g.set_out_node(t)
    return g


NESTED_SKIPS_LAYERS = ((3, 32, 32), (1, 32, 16), (3, 16, 32), (1, 64, 32))


# ------------------------------------------------------------------------------ oracle
class _View(object):
    """The graph seen from one of its outputs (route_cases.topo_nodes walks back from out_node)."""

    def __init__(self, g, node):
        self.g, self.out_node = g, node

    def predecessors(self, n):
        return self.g.predecessors(n)


class _Union(_View):
    """The graph seen from its primary output, which here also 'depends' on the extra outputs, so
    that one walk reaches every node (the oracle evaluates a node from its own inputs)."""

    def __init__(self, g):
        _View.__init__(self, g, g.out_node)

    def predecessors(self, n):
        return list(self.g.predecessors(n)) + (list(self.g.extra_out_nodes) if n is self.out_node else [])


def oracle_outputs(g, x, acc=np.float64):
    """[extra outputs in declaration order..., primary] from one residual_cases.oracle_graph pass."""
    val = RS.oracle_graph(_Union(g), x, acc=acc, keep=True)
    return [val[n] for n in list(g.extra_out_nodes) + [g.out_node]]


# ------------------------------------------------------------------------------ taps of a guarded plan
def tap_bytes(gp, k):
    """(the tap's whole region for the planned batch as a uint8 host array, its device address):
    asserts that it lies inside the caller's workspace, between the guards."""
    ptr, nbytes = gp.plan.tap_buffer(k)
    lo = gp.sbuf.data_ptr() + K.GUARD_BYTES
    hi = gp.sbuf.data_ptr() + gp.sbuf.numel() - K.GUARD_BYTES
    assert lo <= ptr and ptr + nbytes <= hi, f"tap {k} at {ptr:#x}+{nbytes} outside the workspace [{lo:#x}, {hi:#x})"
    h, w, c = gp.plan.tap_shapes[k]
    assert nbytes == gp.B * h * w * c * 4
    off = ptr - gp.sbuf.data_ptr()
    gp.torch.cuda.synchronize()
    return gp.sbuf[off:off + nbytes].cpu().numpy(), ptr


def read_tap(gp, k, n, fresh_tail=False):
    """The first n images of tap k after a run; with fresh_tail (a plan that never ran more than
    n images) also a check that the rest of its region still holds the workspace's poison."""
    raw, _ = tap_bytes(gp, k)
    h, w, c = gp.plan.tap_shapes[k]
    used = n * h * w * c * 4
    if fresh_tail:
        assert len(raw) > used and (raw[used:] == K.POISON).all(), \
            f"tap {k}: bytes past the first {n} images were written"
    return raw[:used].view(np.float32).reshape(n, h, w, c).copy()
