"""Shared by tests/test_route_cpu.py and tests/test_gpu_route.py: the numpy definition of the
route op, the fork/join graphs, their weights, and a float64 oracle that evaluates any builder
graph node by node with oracle/ref_numpy.py."""
import numpy as np

import dnn_hip
import ref_numpy as R
import synth


def route(a, b=None, block=1, b_first=False):
    """space_to_depth(a, block) in TensorFlow's NHWC order, concatenated on channels with b."""
    n, h, w, c = a.shape
    s = a.reshape(n, h // block, block, w // block, block, c).transpose(0, 1, 3, 2, 4, 5)
    s = s.reshape(n, h // block, w // block, block * block * c)
    if b is None:
        return np.ascontiguousarray(s)
    return np.concatenate([b, s] if b_first else [s, b], axis=3)


def route_loops(a, b, block, b_first):
    """The definition, literally (tiny inputs only)."""
    n, h, w, ca = a.shape
    cb = 0 if b is None else b.shape[3]
    out = np.zeros((n, h // block, w // block, block * block * ca + cb), a.dtype)
    a0 = cb if b_first else 0
    b0 = 0 if b_first else block * block * ca
    for i in range(n):
        for y in range(h // block):
            for x in range(w // block):
                for dy in range(block):
                    for dx in range(block):
                        for c in range(ca):
                            out[i, y, x, a0 + (dy * block + dx) * ca + c] = a[i, y * block + dy, x * block + dx, c]
                for c in range(cb):
                    out[i, y, x, b0 + c] = b[i, y, x, c]
    return out


# ------------------------------------------------------------------------------ weights
def exact_layer(rng, k, ic, od):
    """Weights in {-1, 0, 1} with at most 4 non-zeros per output channel and an integer bias: on
    integer inputs every sum is a small integer, exact in fp32 whatever the summation order
    and exact through the bf16 three-way split."""
    kern = np.zeros((k * k * ic, od), np.float32)
    for d in range(od):
        idx = rng.choice(k * k * ic, size=4, replace=False)
        kern[idx, d] = rng.choice(np.array([-1.0, 0.0, 1.0], np.float32), size=4)
    return {"kernel": kern.reshape(k, k, ic, od), "biases": rng.integers(-2, 3, od).astype(np.float32)}


def exact_input(rng, shape):
    return rng.integers(-3, 4, shape).astype(np.float32)


def random_layer(layer, k, ic, od, bn=True):
    """synth's generators: He-like kernel, bias, BatchNorm parameters."""
    return synth.layer_weights(layer, ic, od, k=k, seed=7, bn=bn)


# the fork/join plan of the issue: (kernel size, input channels, output channels) per conv
FORK_JOIN_IN = (16, 16, 32)
FORK_JOIN_LAYERS = ((3, 32, 64), (3, 64, 128), (1, 64, 32), (3, 256, 64), (1, 64, 30))


def fork_join_weights(kind, seed=0):
    rng = np.random.default_rng(seed)
    if kind == "exact":
        return [exact_layer(rng, *l) for l in FORK_JOIN_LAYERS]
    last = len(FORK_JOIN_LAYERS) - 1
    return [random_layer(i, *l, bn=i != last) for i, l in enumerate(FORK_JOIN_LAYERS)]


def _conv(g, x, w, act=True):
    x = g.create_conv2d(x, w["kernel"], [1, 1, 1, 1], "SAME")
    x = g.create_bias_add(x, w["biases"])
    if "gamma" in w:
        x = g.create_batch_norm(x, w["moving_mean"], w["moving_variance"], w["gamma"], 1e-5)
        if act:
            x = g.create_leaky_relu(x)
    return x


def fork_join_graph(B, ws, tail=2):
    """conv -> X; trunk: pool, conv; passthrough: 1x1 conv on X, SpaceToDepth(2);
    Concat([passthrough, trunk]); `tail` more convs (of ws[3:])."""
    g = dnn_hip.DnnGraphBuilder()
    x = g.create_input([B] + list(FORK_JOIN_IN))
    x = _conv(g, x, ws[0])
    t = g.create_max_pool2d(x, [1, 2, 2, 1], [1, 2, 2, 1], "SAME")
    t = _conv(g, t, ws[1])
    p = _conv(g, x, ws[2])
    p = g.create_space_to_depth(p, 2)
    y = g.create_concat([p, t])
    for w in ws[3:3 + tail]:
        y = _conv(g, y, w)
    g.set_out_node(y)
    return g


def empty_branch_graph(B, ws):
    """Concat([x, f(x)]) with x the first conv's output and f one 3x3 conv, then a 1x1 conv."""
    g = dnn_hip.DnnGraphBuilder()
    x = g.create_input([B, 8, 8, 32])
    x = _conv(g, x, ws[0])
    f = _conv(g, x, ws[1])
    y = g.create_concat([x, f])
    y = _conv(g, y, ws[2])
    g.set_out_node(y)
    return g


EMPTY_BRANCH_LAYERS = ((3, 32, 32), (3, 32, 64), (1, 96, 16))


def two_joins_graph(B, ws):
    """Two fork/joins in sequence: Concat([conv(x), pool-free conv(x)]) twice, the second with a
    SpaceToDepth on the branch given second."""
    g = dnn_hip.DnnGraphBuilder()
    x = g.create_input([B, 8, 8, 32])
    x = _conv(g, x, ws[0])
    a = _conv(g, x, ws[1])
    b = _conv(g, x, ws[2])
    x = g.create_concat([a, b])
    x = _conv(g, x, ws[3])
    t = g.create_max_pool2d(x, [1, 2, 2, 1], [1, 2, 2, 1], "SAME")
    t = _conv(g, t, ws[4])
    p = g.create_space_to_depth(_conv(g, x, ws[5]), 2)
    y = g.create_concat([t, p])
    y = _conv(g, y, ws[6])
    g.set_out_node(y)
    return g


TWO_JOINS_LAYERS = ((3, 32, 32), (3, 32, 32), (1, 32, 16), (3, 48, 32), (3, 32, 64), (1, 32, 8), (1, 96, 20))


def exact_weights(layers, seed=0):
    rng = np.random.default_rng(seed)
    return [exact_layer(rng, *l) for l in layers]


# ------------------------------------------------------------------------------ oracle
def topo_nodes(g):
    """The graph's nodes, every node after its inputs."""
    order, seen = [], set()

    def visit(n):
        if id(n) in seen:
            return
        seen.add(id(n))
        for p in g.predecessors(n):
            visit(p)
        order.append(n)

    visit(g.out_node)
    return order


def oracle_graph(g, x, acc=np.float64, keep=False):
    """Evaluate a builder graph with ref_numpy (conv sums in `acc`).  Returns the output, or
    with keep=True the dict node -> result."""
    val = {}
    for n in topo_nodes(g):
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
            val[n] = route(val[n.in_node], None, n.block)
        elif isinstance(n, dnn_hip.Concat):
            val[n] = route(val[n.in_nodes[0]], val[n.in_nodes[1]], 1)
        else:
            raise TypeError(type(n).__name__)
    return val if keep else val[g.out_node]


def entry_kinds(entries):
    """One letter per plan entry: C conv, P pool, S stash, R restore, J route."""
    names = {dnn_hip.ConvEntry: "C", dnn_hip.PoolEntry: "P", dnn_hip.StashEntry: "S", dnn_hip.RestoreEntry: "R",
             dnn_hip.RouteEntry: "J"}
    return "".join(names[type(e)] for e in entries)
