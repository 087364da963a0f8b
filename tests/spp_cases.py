"""Shared by tests/test_spp_cpu.py and tests/test_gpu_spp.py: the SPP oracle composed from
oracle/ref_numpy.py's max pool, tie-heavy inputs with both zeros, graphs with an Spp node, and the
graph oracle of residual_cases / multi_out_cases extended with that node."""
import numpy as np

import dnn_hip
import multi_out_cases as MC
import ref_numpy as R
import residual_cases as RS
import route_cases as RC

DARKNET_SIZES = (13, 9, 5)
# (sizes, x_first) every kernel shape is run with
SIZE_CASES = (((13, 9, 5), False), ((5, 9, 13), True), ((3,), False), ((5, 5), False))
# (n, h, w, c): one pixel; smaller than every halo; the two maps where SPP occurs; a channel count
# that is no multiple of 4 (the scalar path) above one slab; odd everything; two tiles each way with
# a ragged last tile in x (the kernel's tiles are at most 20 x 20); and, beyond the issue's list,
# ragged last tiles in both directions with three tiles in x
KERNEL_SHAPES = ((1, 1, 1, 1), (2, 2, 3, 5), (2, 13, 13, 8), (1, 19, 19, 12), (1, 7, 9, 67), (3, 5, 4, 3),
                 (1, 40, 37, 4), (1, 23, 41, 4))


def spp(x, sizes, x_first=False):
    """[MaxPool2D(k, stride 1, SAME)(x) for k in sizes] and x (last, or first) on channels."""
    x = np.asarray(x, np.float32)
    pools = [R.max_pool2d(x, [1, k, k, 1], [1, 1, 1, 1], "SAME") for k in sizes]
    return np.ascontiguousarray(np.concatenate(([x] + pools) if x_first else (pools + [x]), axis=3))


def tie_input(rng, shape):
    """Small integers in [-3, 3] with about a third of the entries replaced by +0.0 / -0.0 at
    random (ties between equal maxima, and between the two zeros), and the last image all
    negative (a maximum initialised to zero would show)."""
    x = rng.integers(-3, 4, shape).astype(np.float32)
    zero = rng.random(shape) < 1.0 / 3.0
    sign = rng.random(shape) < 0.5
    x = np.where(zero, np.where(sign, np.float32(-0.0), np.float32(0.0)), x).astype(np.float32)
    neg = -rng.integers(1, 4, shape[1:]).astype(np.float32)
    return np.concatenate([x, neg[None]], axis=0)


# ------------------------------------------------------------------------------ graphs
# Every graph takes [B, 8, 8, 32] (residual_cases.IN_SHAPE: a map smaller than the 13 window, so
# every window is clipped); with route_cases.exact_weights and exact_input all values are small
# integers and plans are bit-equal to the oracle.  (kernel size, input channels, output channels)
IN_SHAPE = RS.IN_SHAPE
CHAIN_LAYERS = ((3, 32, 32), (1, 128, 8))       # conv -> spp(13, 9, 5) -> conv
FIRST_LAYERS = ((1, 128, 8),)                   # spp -> conv
LAST_LAYERS = ((3, 32, 32),)                    # conv -> spp
TAP_LAYERS = ((3, 32, 32), (1, 96, 8))          # conv -> spp(5, 9) x first -> tap -> conv
RESTORE_LAYERS = ((3, 32, 32), (3, 32, 16), (1, 128, 8))  # conv -> x; x -> conv -> tap; x -> spp -> conv


def chain_graph(B, ws):
    g = dnn_hip.DnnGraphBuilder()
    x = MC._conv(g, MC._input(g, B), ws[0])
    g.set_out_node(MC._conv(g, g.create_spp(x, DARKNET_SIZES), ws[1]))
    return g


def first_graph(B, ws):
    g = dnn_hip.DnnGraphBuilder()
    g.set_out_node(MC._conv(g, g.create_spp(MC._input(g, B), DARKNET_SIZES), ws[0]))
    return g


def last_graph(B, ws):
    g = dnn_hip.DnnGraphBuilder()
    g.set_out_node(g.create_spp(MC._conv(g, MC._input(g, B), ws[0]), DARKNET_SIZES))
    return g


def tap_graph(B, ws):
    g = dnn_hip.DnnGraphBuilder()
    s = g.create_spp(MC._conv(g, MC._input(g, B), ws[0]), (5, 9), x_first=True)
    g.add_out_node(s)
    g.set_out_node(MC._conv(g, s, ws[1]))
    return g


def restore_graph(B, ws):
    """An output branch from x, then the SPP block on the restored x: it reads a slot region."""
    g = dnn_hip.DnnGraphBuilder()
    x = MC._conv(g, MC._input(g, B), ws[0])
    g.add_out_node(MC._conv(g, x, ws[1]))
    g.set_out_node(MC._conv(g, g.create_spp(x, DARKNET_SIZES), ws[2]))
    return g


PLAN_CASES = {
    # name: (layers, graph builder, entry kinds)
    "chain": (CHAIN_LAYERS, chain_graph, "CYC"),
    "first": (FIRST_LAYERS, first_graph, "YC"),
    "last": (LAST_LAYERS, last_graph, "CY"),
    "tap": (TAP_LAYERS, tap_graph, "CYTC"),
    "restore": (RESTORE_LAYERS, restore_graph, "CSCTRXYC"),
}


# ------------------------------------------------------------------------------ graph oracle
def oracle_graph(g, x, acc=np.float64, keep=False):
    """residual_cases.oracle_graph for graphs that may also hold Spp nodes."""
    val = {}
    for n in RC.topo_nodes(g):
        if isinstance(n, dnn_hip.Input):
            val[n] = np.asarray(x, np.float32)
        elif isinstance(n, dnn_hip.Conv2D):
            val[n] = R.conv2d(val[n.in_node], n.kernel, strides=tuple(n.strides), padding=n.padding, acc=acc)
        elif isinstance(n, dnn_hip.BiasAdd):
            val[n] = R.bias_add(val[n.in_node], n.biases)
        elif isinstance(n, dnn_hip.BatchNorm):
            val[n] = R.batch_norm(val[n.in_node], n.mean, n.variance, n.gamma, n.epsilon)
        elif isinstance(n, dnn_hip.LeakyReLU):
            val[n] = R.leaky_relu(val[n.in_node])
        elif isinstance(n, dnn_hip.MaxPool2D):
            val[n] = R.max_pool2d(val[n.in_node], n.ksize, n.strides, n.padding)
        elif isinstance(n, dnn_hip.SpaceToDepth):
            val[n] = RC.route(val[n.in_node], None, n.block)
        elif isinstance(n, dnn_hip.Concat):
            val[n] = RC.route(val[n.in_nodes[0]], val[n.in_nodes[1]], 1)
        elif isinstance(n, dnn_hip.Add):
            val[n] = RS.add(val[n.in_nodes[0]], val[n.in_nodes[1]])
        elif isinstance(n, dnn_hip.Upsample):
            val[n] = RS.upsample(val[n.in_node], n.factor)
        elif isinstance(n, dnn_hip.Spp):
            val[n] = spp(val[n.in_node], n.ksizes, n.x_first)
        else:
            raise TypeError(type(n).__name__)
    return val if keep else val[g.out_node]


def oracle_outputs(g, x, acc=np.float64):
    """multi_out_cases.oracle_outputs for graphs that may hold Spp nodes: [extra outputs in
    declaration order..., primary]."""
    val = oracle_graph(MC._Union(g), x, acc=acc, keep=True)
    return [val[n] for n in list(g.extra_out_nodes) + [g.out_node]]


def entry_kinds(entries):
    """multi_out_cases.entry_kinds plus Y spp."""
    names = {dnn_hip.ConvEntry: "C", dnn_hip.PoolEntry: "P", dnn_hip.StashEntry: "S", dnn_hip.RestoreEntry: "R",
             dnn_hip.RouteEntry: "J", dnn_hip.ShortcutEntry: "A", dnn_hip.ReleaseEntry: "X",
             dnn_hip.UpsampleEntry: "U", dnn_hip.TapEntry: "T", dnn_hip.SppEntry: "Y"}
    return "".join(names[type(e)] for e in entries)


def max_live_slots(entries):
    """multi_out_cases.max_live_slots on a plan that may hold spp entries (they name no slot)."""
    return MC.max_live_slots([e for e in entries if not isinstance(e, dnn_hip.SppEntry)])
