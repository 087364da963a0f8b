"""Shared by tests/test_residual_cpu.py and tests/test_gpu_residual.py: the numpy statements of
the element-wise add (with its activations) and the nearest-neighbour upsample, residual and
top-down graphs with their weights, an oracle that evaluates them node by node (route_cases'
one plus the two new nodes), and a plan on poisoned, guarded buffers."""
import numpy as np

import dnn_hip
import plan_fuzz_checks as K
import ref_numpy as R
import route_cases as RC


# ------------------------------------------------------------------------------ definitions
def leaky(t, variant):
    """The conv epilogue's activations on float32: 0 none, 1 t < 0 ? (float)(0.1 * (double)t) : t,
    2 max(t, 0.1f * t) as the compare-and-select `t > 0.1f*t ? t : 0.1f*t`."""
    t = np.asarray(t, np.float32)
    if variant == 0:
        return t
    if variant == 1:
        return np.where(t < 0, (0.1 * t.astype(np.float64)).astype(np.float32), t)
    s = (t * np.float32(0.1)).astype(np.float32)
    return np.where(t > s, t, s)


def add(a, b, variant=0):
    """act(a + b): one float32 add, rounded once."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        return leaky((a + b).astype(np.float32), variant)


def upsample(a, f):
    """out[n, h, w, c] = a[n, h // f, w // f, c]."""
    return np.ascontiguousarray(np.repeat(np.repeat(a, f, axis=1), f, axis=2))


def upsample_loops(a, f):
    """The definition, literally (tiny inputs only)."""
    n, h, w, c = a.shape
    out = np.zeros((n, h * f, w * f, c), a.dtype)
    for i in range(n):
        for y in range(h * f):
            for x in range(w * f):
                for k in range(c):
                    out[i, y, x, k] = a[i, y // f, x // f, k]
    return out


# ------------------------------------------------------------------------------ oracle
def oracle_graph(g, x, acc=np.float64, keep=False):
    """route_cases.oracle_graph for graphs that may also hold Add and Upsample nodes."""
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
            val[n] = add(val[n.in_nodes[0]], val[n.in_nodes[1]])
        elif isinstance(n, dnn_hip.Upsample):
            val[n] = upsample(val[n.in_node], n.factor)
        else:
            raise TypeError(type(n).__name__)
    return val if keep else val[g.out_node]


def entry_kinds(entries):
    """route_cases.entry_kinds plus A shortcut, X release, U upsample."""
    names = {dnn_hip.ConvEntry: "C", dnn_hip.PoolEntry: "P", dnn_hip.StashEntry: "S", dnn_hip.RestoreEntry: "R",
             dnn_hip.RouteEntry: "J", dnn_hip.ShortcutEntry: "A", dnn_hip.ReleaseEntry: "X",
             dnn_hip.UpsampleEntry: "U"}
    return "".join(names[type(e)] for e in entries)


# ------------------------------------------------------------------------------ graphs
# (kernel size, input channels, output channels) per conv; every graph takes [B, 8, 8, 32]
IN_SHAPE = (8, 8, 32)
BLOCK = ((1, 32, 16), (3, 16, 32))


def blocks_layers(nblocks):
    return ((3, 32, 32),) + BLOCK * nblocks + ((1, 32, 8),)


def blocks_graph(B, ws, nblocks, act_after_add=False):
    """conv -> x; nblocks times x = Add([x, conv3x3(conv1x1(x))]) [-> LeakyReLU]; a 1x1 conv."""
    g = dnn_hip.DnnGraphBuilder()
    x = RC._conv(g, g.create_input([B] + list(IN_SHAPE)), ws[0])
    for i in range(nblocks):
        f = RC._conv(g, RC._conv(g, x, ws[1 + 2 * i]), ws[2 + 2 * i])
        x = g.create_add([x, f])
        if act_after_add:
            x = g.create_leaky_relu(x)
    x = RC._conv(g, x, ws[1 + 2 * nblocks])
    g.set_out_node(x)
    return g


PROJECTION_LAYERS = ((3, 32, 32), (1, 32, 16), (3, 16, 64), (1, 32, 64), (1, 64, 8))


def projection_graph(B, ws):
    """conv -> x; Add([conv3x3(conv1x1(x)), proj1x1(x)]): a projection conv in the second branch."""
    g = dnn_hip.DnnGraphBuilder()
    x = RC._conv(g, g.create_input([B] + list(IN_SHAPE)), ws[0])
    f = RC._conv(g, RC._conv(g, x, ws[1]), ws[2])
    p = RC._conv(g, x, ws[3])
    y = RC._conv(g, g.create_add([f, p]), ws[4])
    g.set_out_node(y)
    return g


TOP_DOWN_LAYERS = ((3, 32, 32), (3, 32, 64), (1, 64, 16), (3, 48, 8))


def top_down_graph(B, ws):
    """conv -> x; Concat([Upsample(conv1x1(conv3x3(pool(x))), 2), x]); a 3x3 conv."""
    g = dnn_hip.DnnGraphBuilder()
    x = RC._conv(g, g.create_input([B] + list(IN_SHAPE)), ws[0])
    t = g.create_max_pool2d(x, [1, 2, 2, 1], [1, 2, 2, 1], "SAME")
    t = RC._conv(g, RC._conv(g, t, ws[1]), ws[2])
    t = g.create_upsample(t, 2)
    y = RC._conv(g, g.create_concat([t, x]), ws[3])
    g.set_out_node(y)
    return g


def conv_entries(ws):
    """One ConvEntry (conv + bias) per weight dict of RC.exact_weights, chained from IN_SHAPE: for
    plans assembled entry by entry.  Returns the list; entry i is the graph's i-th conv."""
    g = dnn_hip.DnnGraphBuilder()
    x = g.create_input([1] + list(IN_SHAPE))
    out = []
    for w in ws:
        c = g.create_conv2d(x, w["kernel"], [1, 1, 1, 1], "SAME")
        b = g.create_bias_add(c, w["biases"])
        e = dnn_hip.ConvEntry(c)
        e.bias = b
        e.nodes.append(b)
        out.append(e)
        x = b
    return out


def conv_ref(x, w):
    return R.bias_add(R.conv2d(x, w["kernel"], strides=(1, 1, 1, 1), padding="SAME"), w["biases"])


# ------------------------------------------------------------------------------ guarded plan
class GuardedPlan(object):
    """A plan from entries on caller-owned, poisoned, guarded buffers (as test_gpu_plan_fuzz.py):
    run() checks that nothing outside the n output rows was written, that the guards of the
    workspace and the weight arena are intact and that no poison survives in the output."""

    def __init__(self, B, shape, entries, **kw):
        import torch
        self.torch = torch
        wb, sb = dnn_hip.Plan.memory(B, shape, entries, **{k: v for k, v in kw.items() if k != "leaky_variant"})
        self.wbuf = torch.full((wb + 2 * K.GUARD_BYTES,), K.POISON, dtype=torch.uint8, device="cuda")
        self.sbuf = torch.full((sb + 2 * K.GUARD_BYTES,), K.POISON, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        self.plan = dnn_hip.Plan(B, shape, entries, device=0, weights_ptr=self.wbuf.data_ptr() + K.GUARD_BYTES,
                                 workspace_ptr=self.sbuf.data_ptr() + K.GUARD_BYTES, **kw)
        self.B, self.shape = B, tuple(shape)
        self.in_floats = int(np.prod(shape))
        self.row = int(np.prod(self.plan.out_shape))
        self.xin = torch.empty(2 * K.GUARD_FLOATS + B * self.in_floats, dtype=torch.float32, device="cuda")
        self.out = torch.empty(2 * K.GUARD_FLOATS + B * self.row, dtype=torch.int32, device="cuda")
        self.stream = torch.cuda.Stream()

    def run(self, x, what, how="run"):
        torch = self.torch
        n = x.shape[0]
        assert n <= self.B and tuple(x.shape[1:]) == self.shape
        self.xin.fill_(float("nan"))
        self.xin[K.GUARD_FLOATS:K.GUARD_FLOATS + n * self.in_floats] = torch.from_numpy(x.reshape(-1)).to("cuda")
        self.out.fill_(K.CANARY)
        torch.cuda.synchronize()
        pin, pout = self.xin.data_ptr() + 4 * K.GUARD_FLOATS, self.out.data_ptr() + 4 * K.GUARD_FLOATS
        if how == "graph":
            self.plan.run_graph(n, pin, pout, self.stream.cuda_stream)
        else:
            self.plan.run_device(n, pin, pout)
        torch.cuda.synchronize()
        flat = self.out.cpu().numpy()
        K.check_canary(flat, n, self.row, self.B, f"{what}: output")
        for name, buf in (("workspace", self.sbuf), ("weight arena", self.wbuf)):
            ends = torch.cat([buf[:K.GUARD_BYTES], buf[-K.GUARD_BYTES:]]).cpu().numpy()
            K.check_guard(ends, f"{what}: {name}")
        y = flat[K.GUARD_FLOATS:K.GUARD_FLOATS + n * self.row].view(np.float32)
        y = y.reshape((n,) + self.plan.out_shape).copy()
        K.check_finite(y, what)
        return y

    def close(self):
        self.plan.close()
