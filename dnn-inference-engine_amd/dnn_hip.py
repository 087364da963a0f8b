"""dnn_hip — MI355X (gfx950) drop-in for proj3's `dnn_openblas.py` / `dnn_cublas.py`.

Same public surface as the reference wrapper (proj3/dnn_openblas.py:23-300):
`DnnGraphBuilder` with `create_input / create_conv2d / create_bias_add /
create_batch_norm / create_leaky_relu / create_max_pool2d / set_out_node`, the node
classes `Conv2D, BiasAdd, MaxPool2D, BatchNorm, LeakyReLU, Input` with the same
constructor arguments and `ValueError` shape checks, `get_out_pads`, and
`DnnInferenceEngine(graph, debug).run(tin) -> np.ndarray`.  `yolov2tiny.py` switches
engines by its import line (proj3/yolov2tiny.py:5):

    from dnn_hip import DnnGraphBuilder, DnnInferenceEngine

Execution.  `run` lowers the node chain ONCE to a device-resident plan
(include/dnn_hip_plan.h): every Conv2D -> BiasAdd -> BatchNorm -> LeakyReLU run becomes
one im2col + fp32-MFMA GEMM with the element-wise ops in its epilogue, every MaxPool2D
one pool kernel; weights are uploaded once and activations stay in HBM.  Two node kinds the
reference lacks, `SpaceToDepth` and `Concat` (`create_space_to_depth`, `create_concat`), express
YOLOv2's passthrough: a fork joined by a Concat lowers to stash / restore / route plan entries
(the route kernel does the fold and the concat in one pass).  Two more, `Add` and `Upsample`
(`create_add`, `create_upsample`), express the residual block y = x + f(x) and the top-down
merge: a fork joined by an Add lowers to stash / shortcut / release entries (a release hands the
slot and its workspace region back, so any number of blocks fit in one plan).  A graph may have
extra outputs (`DnnGraphBuilder.add_out_node`, `DnnInferenceEngine.run_all`): each becomes a tap
entry of the plan, and a branch that ends in one, or a tensor concatenated many layers later, lowers
too (lower_graph; YOLOv3's three heads and two merges, yolov3.py).  `Spp` (`create_spp`) is
YOLOv3-SPP's pyramid pooling block, [maxpool13(x), maxpool9(x), maxpool5(x), x] on channels: one
node, one spp plan entry, one kernel (yolov3_spp.py).  `Conv2DPadded` (`create_conv2d_padded`) is
a conv with the same zero padding on both sides of each axis (Darknet's), `ScaleShift`
(`create_scale_shift`) a per-channel y = x * scale + shift (a BatchNorm folded on the host) and
`LeakyReLUF32` (`create_leaky_relu_f32`) the fp32 leaky max(x, 0.1f x); a conv followed by a
ScaleShift and either leaky lowers to one dnn_plan_add_conv_padded entry (darknet_import.py).  With
`debug=True` (or a graph the plan cannot express) it instead runs node by node through
the per-op C-ABI (`conv2d_mul`, `bias_add`, ... in libdnn_hip.so, include/dnn_hip.h),
exactly like the reference, and saves every layer to ./intermediate/layer_{k}.npy
(counter from 1, proj3/dnn_openblas.py:47-50; the reference saves unconditionally, the
AVX wrapper only in debug mode, proj3/dnn_avx.py:55-57 — we follow the latter).

Numerics are the reference's correct semantics: fp32 everywhere, the
conv accumulation order differs from OpenBLAS, so outputs match within the stated
normwise tolerance max|d| <= 1e-4 * max|ref|; the element-wise ops and max pool are
bit-exact.  There is no CPU fallback: a missing or broken HIP library raises.
"""
import ctypes
import math
import os

import numpy as np

try:  # the reference's graph container (proj3/dnn_openblas.py:1-4)
    import networkx as nx
except ImportError:  # pragma: no cover - networkx ships in the image
    nx = None

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_NAME = os.environ.get("DNN_HIP_LIB", "libdnn_hip.so")

c_float_pointer_type = ctypes.POINTER(ctypes.c_float)
c_int_pointer_type = ctypes.POINTER(ctypes.c_int)


class DnnHipError(RuntimeError):
    pass


def _bind_plan_api(lib):
    vp, i, f, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_size_t
    P = ctypes.POINTER
    sig = {
        "dnn_last_error": (ctypes.c_char_p, []),
        "dnn_plan_create": (i, [i, i, i, i, P(vp)]),
        "dnn_plan_destroy": (None, [vp]),
        "dnn_plan_add_conv": (i, [vp, i, i, i, i, i, i, vp, vp, vp, vp, vp, f, i]),
        "dnn_plan_add_conv_padded": (i, [vp, i, i, i, i, i, i, i, vp, vp, vp, i]),
        "dnn_scale_shift_host": (i, [vp, vp, vp, vp, i, i, i, i, i]),
        "dnn_plan_add_max_pool": (i, [vp, i, i, i, i, i]),
        "dnn_plan_add_stash": (i, [vp, P(i)]),
        "dnn_plan_add_restore": (i, [vp, i]),
        "dnn_plan_add_route": (i, [vp, i, i, i]),
        "dnn_route_host": (i, [vp, vp, vp, i, i, i, i, i, i, i]),
        "dnn_plan_add_shortcut": (i, [vp, i, i]),
        "dnn_plan_add_upsample": (i, [vp, i]),
        "dnn_plan_add_release": (i, [vp, i]),
        "dnn_plan_add_tap": (i, [vp, P(i)]),
        "dnn_plan_num_taps": (i, [vp]),
        "dnn_plan_tap_shape": (i, [vp, i, P(i), P(i), P(i)]),
        "dnn_plan_tap_buffer": (i, [vp, i, P(vp), P(sz)]),
        "dnn_plan_tap_read_host": (i, [vp, i, i, vp]),
        "dnn_shortcut_host": (i, [vp, vp, vp, i, i, i, i, i]),
        "dnn_upsample_host": (i, [vp, vp, i, i, i, i, i]),
        "dnn_plan_add_spp": (i, [vp, i, P(i), i]),
        "dnn_plan_add_slice": (i, [vp, i, i]),
        "dnn_slice_host": (i, [vp, vp, i, i, i, i, i, i]),
        "dnn_spp_host": (i, [vp, vp, i, i, i, i, i, P(i), i]),
        "dnn_plan_output_shape": (i, [vp, P(i), P(i), P(i), P(i)]),
        "dnn_plan_describe": (i, [vp, ctypes.c_char_p, i]),
        "dnn_plan_memory": (i, [vp, P(sz), P(sz)]),
        "dnn_plan_finalize": (i, [vp, i, vp, vp]),
        "dnn_plan_weight_buffer": (i, [vp, P(vp), P(sz)]),
        "dnn_plan_run": (i, [vp, i, vp, vp, vp]),
        "dnn_plan_run_host": (i, [vp, i, vp, vp]),
        "dnn_plan_run_graph": (i, [vp, i, vp, vp, vp]),
        "dnn_plan_set_precision": (i, [vp, i]),
        "dnn_plan_set_latency_mode": (i, [vp, i]),
        "dnn_plan_num_kernels": (i, [vp]),
        "dnn_plan_kernel_info": (i, [vp, i, ctypes.c_char_p, i, P(ctypes.c_double), P(ctypes.c_double)]),
        "dnn_plan_timing_begin": (i, [vp, i]),
        "dnn_plan_timing_begin_only": (i, [vp, i, i]),
        "dnn_plan_timing_end": (i, [vp, P(ctypes.c_double), P(ctypes.c_longlong)]),
        "dnn_clock_stamp": (i, [vp, vp, i]),
        "dnn_plan_clock_begin": (i, [vp, i, vp, i, i]),
        "dnn_plan_clock_end": (i, [vp, P(i)]),
        "dnn_plan_set_mark": (i, [vp, i]),
        "dnn_plan_wait_mark": (i, [vp, vp]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if hasattr(lib, "dnn_plan_range_events"):  # (tools/lib_ab.py also loads libraries from before it)
        lib.dnn_plan_range_events.restype = i
        lib.dnn_plan_range_events.argtypes = [vp, P(ctypes.c_uint)]
        lib.dnn_plan_describe_pieces.restype = i
        lib.dnn_plan_describe_pieces.argtypes = [vp, ctypes.c_char_p, i]
    return lib


def _one_hip_runtime():
    """PyTorch-ROCm bundles its own libamdhip64.so (SONAME libamdhip64.so.7).  If torch is
    importable, import it BEFORE our library so that our NEEDED libamdhip64.so.7 resolves to
    that already-loaded runtime by SONAME: one HIP runtime per process, and device pointers
    and streams from torch are valid here.  Without torch the system ROCm runtime is used."""
    if os.environ.get("DNN_HIP_NO_TORCH") == "1":
        return
    try:
        import torch  # noqa: F401
    except ImportError:
        pass


def load_library(name=LIB_NAME):
    """Load one of the in-tree C-ABI libraries (built by csrc/Makefile).  Fails loudly:
    there is no CPU fallback for the product path."""
    _one_hip_runtime()
    path = name if os.path.isabs(name) else os.path.join(_HERE, name)
    if not os.path.exists(path):
        raise DnnHipError(f"{path} not found: build it with `make -C {os.path.join(_HERE, 'csrc')}` "
                          "(or __graft_entry__.build())")
    return _bind_plan_api(ctypes.CDLL(path))


mylib = load_library()


def last_error(lib=None):
    msg = (lib or mylib).dnn_last_error()
    return msg.decode() if msg else ""


def _check(rc, what, lib=None):
    if rc != 0:
        raise DnnHipError(f"{what} failed ({rc}): {last_error(lib)}")


def _check_legacy(what):
    msg = last_error()
    if msg:
        raise DnnHipError(f"{what} failed: {msg}")


def _fp(a):
    return a.ctypes.data_as(c_float_pointer_type)


def _vp(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


PRECISIONS = {"fp32": 0, "fp16": 1}


def _precision(p):
    p = (os.environ.get("DNN_HIP_PRECISION", "fp32") if p is None else p).lower()
    if p not in PRECISIONS:
        raise ValueError(f"precision must be one of {sorted(PRECISIONS)}, got {p!r}")
    return p


class DnnInferenceEngine(object):
    """proj3/dnn_openblas.py:23-57.  `device` picks the GPU (default $DNN_HIP_DEVICE or 0);
    `precision` "fp32" (default, the reference's arithmetic) or "fp16" (fp16 MFMA conv path,
    BASELINE config 5; default from $DNN_HIP_PRECISION); `latency` True builds a latency plan
    (dnn_plan_set_latency_mode: K splits chosen for the graph's batch, for single-frame
    inference as proj3/__init__.py:24-26 runs it; fp32 only).  Unset, $DNN_HIP_LATENCY=1 turns
    it on for fp32 engines and is ignored by fp16 ones; latency=True with fp16 is an error."""

    def __init__(self, graph, debug, device=None, precision=None, latency=None):
        self.g = graph
        self.debug = debug
        self.precision = _precision(precision)
        if latency is None:  # the environment default applies where latency plans exist (fp32)
            latency = os.environ.get("DNN_HIP_LATENCY") == "1" and self.precision == "fp32"
        self.latency = bool(latency)
        self.device = int(os.environ.get("DNN_HIP_DEVICE", "0")) if device is None else device
        self.save_dir = os.path.join(os.getcwd(), "intermediate")
        self._plan = None
        self._chain = None

    # -- fused, device-resident path ------------------------------------------------
    def plan(self):
        """The lowered plan (built on first use; weights uploaded once)."""
        if self._plan is None:
            self._plan = Plan.from_graph(self.g, device=self.device, precision=self.precision,
                                         latency=self.latency)
        return self._plan

    def run(self, tin):
        self.g.in_node.set_input(tin)
        if not self.debug and lower_graph(self.g) is not None:
            x = np.ascontiguousarray(tin, dtype=np.float32)
            out = self.plan().run_host(x)
            self.g.out_node.result = out
            return out
        return self._run_nodes()

    def run_all(self, tin):
        """Every output of a graph with extra outputs (DnnGraphBuilder.add_out_node): the extra
        ones in declaration order, then the primary one.  Same two paths as run()."""
        self.g.in_node.set_input(tin)
        extras = list(self.g.extra_out_nodes)
        if not self.debug and lower_graph(self.g) is not None:
            x = np.ascontiguousarray(tin, dtype=np.float32)
            plan = self.plan()
            outs = plan.run_host_all(x)  # taps in plan order, then the primary output
            by_node = {id(e.node): t for e, t in zip(plan.tap_entries, outs[:-1])}
            for n in extras:
                n.result = by_node[id(n)]
            self.g.out_node.result = outs[-1]
            return [by_node[id(n)] for n in extras] + [outs[-1]]
        primary = self._run_nodes()
        return [n.result for n in extras] + [primary]

    # -- node-by-node path through the per-op ABI (the reference's traversal) --------
    def _run_nodes(self):
        out = {}
        currents = [self.g.in_node]
        done = set()
        counter = 0
        if self.debug:
            os.makedirs(self.save_dir, exist_ok=True)
        while len(currents) != 0:
            nexts = []
            for current in currents:
                if current in done:
                    continue
                if any(p not in done for p in self.g.predecessors(current)):
                    nexts.extend(p for p in self.g.predecessors(current) if p not in done)
                    continue
                current.run()
                if not isinstance(current, Input):
                    counter += 1
                    if self.debug:
                        np.save(os.path.join(self.save_dir, "layer_{}.npy".format(counter)), current.result)
                if self.g.is_out_node(current):
                    out = current.result
                done.add(current)
                nexts.extend(self.g.successors(current))
            currents = nexts
        return out


class _DiGraph(object):
    """Minimal stand-in for networkx.DiGraph when networkx is unavailable."""

    def __init__(self):
        self._succ, self._pred = {}, {}

    def add_node(self, n):
        self._succ.setdefault(n, [])
        self._pred.setdefault(n, [])

    def add_edge(self, a, b):
        self.add_node(a)
        self.add_node(b)
        self._succ[a].append(b)
        self._pred[b].append(a)

    def successors(self, n):
        return iter(self._succ.get(n, []))

    def predecessors(self, n):
        return iter(self._pred.get(n, []))


class DnnGraphBuilder(object):
    """proj3/dnn_openblas.py:59-114."""

    def __init__(self):
        self.G = nx.DiGraph() if nx is not None else _DiGraph()
        self.name_num = {"conv2d": 0, "bias_add": 0, "max_pool2d": 0, "batch_norm": 0, "leaky_relu": 0,
                         "input": 0, "space_to_depth": 0, "concat": 0, "add": 0, "upsample": 0, "spp": 0,
                         "channel_slice": 0,
                         "conv2d_padded": 0, "scale_shift": 0, "leaky_relu_f32": 0}
        self.in_node = None
        self.out_node = None
        self.extra_out_nodes = []

    def set_in_node(self, node):
        self.in_node = node

    def set_out_node(self, node):
        self.out_node = node

    def add_out_node(self, node):
        """Declare an extra output (not in the reference: its graphs have one).  Extra outputs
        are returned by DnnInferenceEngine.run_all in the order declared, before the primary
        output of set_out_node, which must be the last tensor the graph computes."""
        if any(n is node for n in self.extra_out_nodes):
            raise ValueError("node is already an extra output")
        self.extra_out_nodes.append(node)

    def is_out_node(self, node):
        return self.out_node is node

    def successors(self, node):
        return list(self.G.successors(node))

    def predecessors(self, node):
        return list(self.G.predecessors(node))

    def get_name(self, layer_name):
        name = layer_name + "_" + str(self.name_num[layer_name])
        self.name_num[layer_name] += 1
        return name

    def create_conv2d(self, in_node, kernel, strides, padding):
        out_node = Conv2D(self.get_name("conv2d"), in_node, kernel, strides, padding)
        self.G.add_edge(in_node, out_node)
        return out_node

    def create_bias_add(self, in_node, biases):
        out_node = BiasAdd(self.get_name("bias_add"), in_node, biases)
        self.G.add_edge(in_node, out_node)
        return out_node

    def create_max_pool2d(self, in_node, ksize, strides, padding):
        out_node = MaxPool2D(self.get_name("max_pool2d"), in_node, ksize, strides, padding)
        self.G.add_edge(in_node, out_node)
        return out_node

    def create_batch_norm(self, in_node, mean, variance, gamma, epsilon):
        out_node = BatchNorm(self.get_name("batch_norm"), in_node, mean, variance, gamma, epsilon)
        self.G.add_edge(in_node, out_node)
        return out_node

    def create_leaky_relu(self, in_node):
        out_node = LeakyReLU(self.get_name("leaky_relu"), in_node)
        self.G.add_edge(in_node, out_node)
        return out_node

    def create_space_to_depth(self, in_node, block):
        out_node = SpaceToDepth(self.get_name("space_to_depth"), in_node, block)
        self.G.add_edge(in_node, out_node)
        return out_node

    def create_concat(self, in_nodes):
        out_node = Concat(self.get_name("concat"), in_nodes)
        for in_node in out_node.in_nodes:
            self.G.add_edge(in_node, out_node)
        return out_node

    def create_add(self, in_nodes):
        out_node = Add(self.get_name("add"), in_nodes)
        for in_node in out_node.in_nodes:
            self.G.add_edge(in_node, out_node)
        return out_node

    def create_upsample(self, in_node, factor):
        out_node = Upsample(self.get_name("upsample"), in_node, factor)
        self.G.add_edge(in_node, out_node)
        return out_node

    def create_channel_slice(self, in_node, first, channels):
        out_node = ChannelSlice(self.get_name("channel_slice"), in_node, first, channels)
        self.G.add_edge(in_node, out_node)
        return out_node

    def create_spp(self, in_node, ksizes, x_first=False):
        out_node = Spp(self.get_name("spp"), in_node, ksizes, x_first)
        self.G.add_edge(in_node, out_node)
        return out_node

    def create_conv2d_padded(self, in_node, kernel, strides, pads):
        """A conv with explicit zero padding: `pads` = (pad_h, pad_w), each applied on both sides
        (Darknet's rule; create_conv2d's SAME is TensorFlow's)."""
        out_node = Conv2DPadded(self.get_name("conv2d_padded"), in_node, kernel, strides, pads)
        self.G.add_edge(in_node, out_node)
        return out_node

    def create_scale_shift(self, in_node, scale, shift):
        out_node = ScaleShift(self.get_name("scale_shift"), in_node, scale, shift)
        self.G.add_edge(in_node, out_node)
        return out_node

    def create_leaky_relu_f32(self, in_node):
        """The fp32 leaky max(x, 0.1f * x) (dnn_avx.c's; the plan's leaky 2), which is Darknet's
        x > 0 ? x : .1f * x for every non-NaN x.  create_leaky_relu rounds 0.1 * x in double."""
        out_node = LeakyReLUF32(self.get_name("leaky_relu_f32"), in_node)
        self.G.add_edge(in_node, out_node)
        return out_node

    def create_input(self, in_shape):
        out_node = Input(self.get_name("input"), in_shape)
        self.G.add_node(out_node)
        self.set_in_node(out_node)  # Assume there's only one input
        return out_node


class DnnNode(object):
    def __init__(self):
        pass

    def run(self):
        self.result = None


def get_out_pads(in_size, filter_size, stride_size, padding):
    """TF SAME/VALID output size and pads (proj3/dnn_openblas.py:127-142)."""
    assert padding == 'SAME' or padding == 'VALID'
    if padding == 'SAME':
        out_size = math.ceil(float(in_size) / float(stride_size))
        pad_size = max((out_size - 1) * stride_size + filter_size - in_size, 0)
        pad_front = pad_size // 2
        pad_back = pad_size - pad_front
    else:
        out_size = math.ceil(float(in_size - filter_size + 1) / float(stride_size))
        pad_front = 0
        pad_back = 0
    return out_size, pad_front, pad_back


class Conv2D(DnnNode):
    """proj3/dnn_openblas.py:144-188; run() -> conv2d_mul on the device."""

    def __init__(self, name, in_node, kernel, strides, padding):
        batch, np_ih, np_iw, ic = in_node.result.shape
        kh, kw, kernel_ic, od = kernel.shape
        if kernel_ic != ic:
            raise ValueError
        if not (padding == 'SAME' or padding == 'VALID'):
            raise ValueError
        oh, self.pad_top, self.pad_bottom = get_out_pads(np_ih, kh, strides[1], padding)
        ow, self.pad_left, self.pad_right = get_out_pads(np_iw, kw, strides[2], padding)
        self.in_node = in_node
        self.kernel = np.ascontiguousarray(kernel).astype(np.float32)
        self.strides = strides
        self.padding = padding
        self.result = np.zeros((batch, oh, ow, od), dtype='float32')
        # K order (ic, kh, kw), the layout conv2d_mul expects (dnn_openblas.py:166-167)
        self.kernel_r = np.ascontiguousarray(self.kernel.transpose(2, 0, 1, 3).reshape(-1, od))
        # the host im2col scratch of the reference is not needed: the device has its own
        self.col = np.zeros((0,), dtype=np.float32)
        self.name = name

    def run(self):
        in_layer = np.ascontiguousarray(np.pad(
            self.in_node.result,
            [(0, 0), (self.pad_top, self.pad_bottom), (self.pad_left, self.pad_right), (0, 0)],
            'constant'), dtype=np.float32)
        mylib.conv2d_mul(
            _fp(in_layer), _fp(self.col), _fp(self.kernel_r), _fp(self.result),
            *map(ctypes.c_int, self.result.shape),
            *map(ctypes.c_int, in_layer.shape[1:]),
            *map(ctypes.c_int, self.kernel.shape[:2]),
            *map(ctypes.c_int, self.strides[1:3]))
        _check_legacy(self.name)


class BiasAdd(DnnNode):
    """proj3/dnn_openblas.py:190-209; run() -> bias_add."""

    def __init__(self, name, in_node, biases):
        if not (biases.ndim == 1 and in_node.result.shape[-1] == biases.shape[0]):
            raise ValueError
        self.in_node = in_node
        self.biases = np.ascontiguousarray(biases, dtype=np.float32)
        self.result = np.zeros(in_node.result.shape, dtype='float32')
        self.name = name

    def run(self):
        x = np.ascontiguousarray(self.in_node.result, dtype=np.float32)
        mylib.bias_add(_fp(x), _fp(self.biases), _fp(self.result), *map(ctypes.c_int, self.result.shape))
        _check_legacy(self.name)


class MaxPool2D(DnnNode):
    """proj3/dnn_openblas.py:211-242; run() -> max_pool2d on a -FLT_MAX padded input."""

    def __init__(self, name, in_node, ksize, strides, padding):
        if not (padding == 'SAME' or padding == 'VALID'):
            raise ValueError
        batch, in_height, in_width, in_channels = in_node.result.shape
        out_height, self.pad_top, self.pad_bottom = get_out_pads(in_height, ksize[1], strides[1], padding)
        out_width, self.pad_left, self.pad_right = get_out_pads(in_width, ksize[2], strides[2], padding)
        self.in_node = in_node
        self.ksize = ksize
        self.strides = strides
        self.padding = padding
        self.result = np.zeros((batch, out_height, out_width, in_channels), dtype='float32')
        self.name = name

    def run(self):
        in_layer = np.ascontiguousarray(np.pad(
            self.in_node.result,
            [(0, 0), (self.pad_top, self.pad_bottom), (self.pad_left, self.pad_right), (0, 0)],
            'constant', constant_values=np.finfo('float32').min), dtype=np.float32)
        mylib.max_pool2d(_fp(in_layer), _fp(self.result),
                         *map(ctypes.c_int, self.result.shape),
                         *map(ctypes.c_int, in_layer.shape[1:]),
                         *map(ctypes.c_int, self.ksize[1:3]),
                         *map(ctypes.c_int, self.strides[1:3]))
        _check_legacy(self.name)


class BatchNorm(DnnNode):
    """proj3/dnn_openblas.py:244-270; run() -> batch_norm (variance is never mutated)."""

    def __init__(self, name, in_node, mean, variance, gamma, epsilon):
        if not all(arg.ndim == 1 and in_node.result.shape[-1] == arg.shape[0] for arg in [mean, variance, gamma]):
            raise ValueError
        self.in_node = in_node
        self.mean = np.ascontiguousarray(mean, dtype=np.float32)
        self.variance = np.ascontiguousarray(variance, dtype=np.float32)
        self.gamma = np.ascontiguousarray(gamma, dtype=np.float32)
        self.epsilon = epsilon
        self.result = np.zeros(in_node.result.shape, dtype='float32')
        self.name = name

    def run(self):
        x = np.ascontiguousarray(self.in_node.result, dtype=np.float32)
        mylib.batch_norm(_fp(x), _fp(self.mean), _fp(self.variance), _fp(self.gamma),
                         ctypes.c_float(self.epsilon), _fp(self.result), *map(ctypes.c_int, self.result.shape))
        _check_legacy(self.name)


class LeakyReLU(DnnNode):
    """proj3/dnn_openblas.py:272-284; run() -> leaky_relu."""

    def __init__(self, name, in_node):
        self.in_node = in_node
        self.result = np.zeros(in_node.result.shape, dtype='float32')
        self.name = name

    def run(self):
        x = np.ascontiguousarray(self.in_node.result, dtype=np.float32)
        mylib.leaky_relu(_fp(x), _fp(self.result), *map(ctypes.c_int, self.result.shape))
        _check_legacy(self.name)


class Conv2DPadded(DnnNode):
    """Not in the reference (Darknet's convs need it): Conv2D with `pads` = (pad_h, pad_w) zeros on
    BOTH sides of each axis, out = (in + 2 * pad - k) // stride + 1, 0 <= pad < k.  run() ->
    conv2d_mul on the np.pad'ed input, like Conv2D."""

    def __init__(self, name, in_node, kernel, strides, pads):
        batch, ih, iw, ic = in_node.result.shape
        kh, kw, kernel_ic, od = kernel.shape
        if kernel_ic != ic:
            raise ValueError
        try:
            ph, pw = (int(v) for v in pads)
        except (TypeError, ValueError):
            raise ValueError
        if (ph, pw) != tuple(pads) or not (0 <= ph < kh and 0 <= pw < kw):
            raise ValueError
        if len(strides) != 4 or strides[1] < 1 or strides[2] < 1:
            raise ValueError
        if ih + 2 * ph < kh or iw + 2 * pw < kw:
            raise ValueError
        oh = (ih + 2 * ph - kh) // strides[1] + 1
        ow = (iw + 2 * pw - kw) // strides[2] + 1
        self.in_node = in_node
        self.kernel = np.ascontiguousarray(kernel).astype(np.float32)
        self.strides = strides
        self.pads = (ph, pw)
        self.result = np.zeros((batch, oh, ow, od), dtype='float32')
        self.kernel_r = np.ascontiguousarray(self.kernel.transpose(2, 0, 1, 3).reshape(-1, od))
        self.col = np.zeros((0,), dtype=np.float32)
        self.name = name

    def run(self):
        ph, pw = self.pads
        in_layer = np.ascontiguousarray(np.pad(self.in_node.result, [(0, 0), (ph, ph), (pw, pw), (0, 0)], 'constant'),
                                        dtype=np.float32)
        mylib.conv2d_mul(
            _fp(in_layer), _fp(self.col), _fp(self.kernel_r), _fp(self.result),
            *map(ctypes.c_int, self.result.shape),
            *map(ctypes.c_int, in_layer.shape[1:]),
            *map(ctypes.c_int, self.kernel.shape[:2]),
            *map(ctypes.c_int, self.strides[1:3]))
        _check_legacy(self.name)


def _scale_shift_host(name, x, scale, shift, out, leaky):
    x = np.ascontiguousarray(x, dtype=np.float32)
    rc = mylib.dnn_scale_shift_host(_vp(x), _vp(scale), _vp(shift), _vp(out), *map(int, x.shape), int(leaky))
    _check(rc, name)


class ScaleShift(DnnNode):
    """Not in the reference (a BatchNorm folded on the host needs it): y = x * scale[c] +
    shift[c], one fp32 multiply and one fp32 add per element.  In a plan it exists only as the
    epilogue of the conv before it.  run() -> dnn_scale_shift_host."""

    def __init__(self, name, in_node, scale, shift):
        scale, shift = np.asarray(scale), np.asarray(shift)
        if len(in_node.result.shape) != 4:
            raise ValueError
        if not all(a.ndim == 1 and a.shape[0] == in_node.result.shape[-1] for a in (scale, shift)):
            raise ValueError
        self.in_node = in_node
        self.scale = np.ascontiguousarray(scale, dtype=np.float32)
        self.shift = np.ascontiguousarray(shift, dtype=np.float32)
        self.result = np.zeros(in_node.result.shape, dtype='float32')
        self.name = name

    def run(self):
        _scale_shift_host(self.name, self.in_node.result, self.scale, self.shift, self.result, 0)


class LeakyReLUF32(DnnNode):
    """Not in the reference's OpenBLAS engine: the fp32 leaky max(x, 0.1f * x) (dnn_avx.c's form,
    the plan's leaky 2; Darknet's for every non-NaN x).  run() -> dnn_scale_shift_host."""

    def __init__(self, name, in_node):
        self.in_node = in_node
        self.result = np.zeros(in_node.result.shape, dtype='float32')
        self.name = name

    def run(self):
        _scale_shift_host(self.name, self.in_node.result, None, None, self.result, 2)


MAX_ROUTE_BLOCK = 8  # dnn_plan_add_route / dnn_route_host: block in 1..8
MAX_SLOTS = 4        # dnn_plan_add_stash: slots per plan
MAX_TAPS = 4         # DNN_PLAN_MAX_TAPS: extra outputs per plan


def _route_host(name, a, b, out, block, b_first=False):
    """out = route(a, b, block) through dnn_route_host (include/dnn_hip_plan.h)."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    b = None if b is None else np.ascontiguousarray(b, dtype=np.float32)
    n, h, w, ca = a.shape
    rc = mylib.dnn_route_host(_vp(a), _vp(b), _vp(out), n, h, w, ca, int(block), 0 if b is None else b.shape[3],
                              1 if b_first else 0)
    _check(rc, name)


class SpaceToDepth(DnnNode):
    """Not in the reference (YOLOv2's passthrough needs it): [n, H, W, C] ->
    [n, H/block, W/block, block*block*C] in TensorFlow's space_to_depth channel order,
    out[n, h, w, (dy*block + dx)*C + c] = in[n, h*block + dy, w*block + dx, c] (not Darknet's
    reorg order).  run() -> dnn_route_host."""

    def __init__(self, name, in_node, block):
        if len(in_node.result.shape) != 4 or int(block) != block or not 1 <= block <= MAX_ROUTE_BLOCK:
            raise ValueError
        batch, h, w, c = in_node.result.shape
        if h % block or w % block:
            raise ValueError
        self.in_node = in_node
        self.block = int(block)
        self.result = np.zeros((batch, h // self.block, w // self.block, self.block * self.block * c), dtype='float32')
        self.name = name

    def run(self):
        _route_host(self.name, self.in_node.result, None, self.result, self.block)


class Concat(DnnNode):
    """Not in the reference: channel concat of exactly two NHWC tensors of the same batch and
    spatial size, in the order given.  run() -> dnn_route_host with block 1."""

    def __init__(self, name, in_nodes):
        in_nodes = list(in_nodes)
        if len(in_nodes) != 2 or any(len(n.result.shape) != 4 for n in in_nodes):
            raise ValueError
        sa, sb = in_nodes[0].result.shape, in_nodes[1].result.shape
        if tuple(sa[:3]) != tuple(sb[:3]):
            raise ValueError
        self.in_nodes = in_nodes
        self.result = np.zeros(tuple(sa[:3]) + (sa[3] + sb[3],), dtype='float32')
        self.name = name

    def run(self):
        _route_host(self.name, self.in_nodes[0].result, self.in_nodes[1].result, self.result, 1)


MAX_UPSAMPLE_FACTOR = 8  # dnn_plan_add_upsample / dnn_upsample_host: factor in 1..8


class Add(DnnNode):
    """Not in the reference (the residual block y = x + f(x) needs it): the element-wise sum of
    exactly two NHWC tensors of identical shape, one fp32 add per element.  run() ->
    dnn_shortcut_host."""

    def __init__(self, name, in_nodes):
        in_nodes = list(in_nodes)
        if len(in_nodes) != 2 or any(len(n.result.shape) != 4 for n in in_nodes):
            raise ValueError
        if tuple(in_nodes[0].result.shape) != tuple(in_nodes[1].result.shape):
            raise ValueError
        self.in_nodes = in_nodes
        self.result = np.zeros(tuple(in_nodes[0].result.shape), dtype='float32')
        self.name = name

    def run(self):
        a = np.ascontiguousarray(self.in_nodes[0].result, dtype=np.float32)
        b = np.ascontiguousarray(self.in_nodes[1].result, dtype=np.float32)
        rc = mylib.dnn_shortcut_host(_vp(a), _vp(b), _vp(self.result), *map(int, a.shape), 0)
        _check(rc, self.name)


class Upsample(DnnNode):
    """Not in the reference (a top-down merge needs it): nearest-neighbour upsample,
    [n, H, W, C] -> [n, H*factor, W*factor, C], out[n, h, w, c] = in[n, h // factor, w // factor, c].
    run() -> dnn_upsample_host."""

    def __init__(self, name, in_node, factor):
        if len(in_node.result.shape) != 4 or int(factor) != factor or not 1 <= factor <= MAX_UPSAMPLE_FACTOR:
            raise ValueError
        batch, h, w, c = in_node.result.shape
        self.in_node = in_node
        self.factor = int(factor)
        self.result = np.zeros((batch, h * self.factor, w * self.factor, c), dtype='float32')
        self.name = name

    def run(self):
        a = np.ascontiguousarray(self.in_node.result, dtype=np.float32)
        rc = mylib.dnn_upsample_host(_vp(a), _vp(self.result), *map(int, a.shape), self.factor)
        _check(rc, self.name)


class ChannelSlice(DnnNode):
    """Not in the reference (a CSP block's split needs it; Darknet's [route] with groups / group_id):
    a channel range, [n, H, W, C] -> [n, H, W, channels], out[..., k] = in[..., first + k] with
    0 <= first, channels >= 1 and first + channels <= C.  run() -> dnn_slice_host."""

    def __init__(self, name, in_node, first, channels):
        if len(in_node.result.shape) != 4:
            raise ValueError
        for v in (first, channels):
            if isinstance(v, bool) or int(v) != v:
                raise ValueError
        batch, h, w, c = in_node.result.shape
        if first < 0 or channels < 1 or first + channels > c:
            raise ValueError
        self.in_node = in_node
        self.first, self.channels = int(first), int(channels)
        self.result = np.zeros((batch, h, w, self.channels), dtype='float32')
        self.name = name

    def run(self):
        a = np.ascontiguousarray(self.in_node.result, dtype=np.float32)
        rc = mylib.dnn_slice_host(_vp(a), _vp(self.result), *map(int, a.shape), self.first, self.channels)
        _check(rc, self.name)


MAX_SPP_SIZES = 3  # DNN_SPP_MAX_SIZES: pools per spp entry
MAX_SPP_K = 13     # DNN_SPP_MAX_K: the largest pool window (sizes are odd, 3..13)


def _spp_sizes(ksizes):
    """The window sizes of an Spp as a tuple of ints; ValueError unless 1..MAX_SPP_SIZES odd sizes
    in 3..MAX_SPP_K."""
    try:
        ks = list(ksizes)
    except TypeError:
        raise ValueError
    if not 1 <= len(ks) <= MAX_SPP_SIZES:
        raise ValueError
    for k in ks:
        if isinstance(k, bool) or int(k) != k or not 3 <= k <= MAX_SPP_K or int(k) % 2 == 0:
            raise ValueError
    return tuple(int(k) for k in ks)


class Spp(DnnNode):
    """Not in the reference (YOLOv3-SPP's neck needs it): spatial pyramid pooling,
    [n, H, W, C] -> [n, H, W, (len(ksizes) + 1) * C].  Channel block j is MaxPool2D(ksize
    ksizes[j], stride 1, SAME) of the input, bit for bit, in the order given; the input itself is
    the last block, or the first with x_first.  (13, 9, 5) is Darknet's order, (5, 9, 13) with
    x_first YOLOv5's.  run() -> dnn_spp_host."""

    def __init__(self, name, in_node, ksizes, x_first=False):
        if len(in_node.result.shape) != 4:
            raise ValueError
        self.ksizes = _spp_sizes(ksizes)
        batch, h, w, c = in_node.result.shape
        self.in_node = in_node
        self.x_first = bool(x_first)
        self.result = np.zeros((batch, h, w, (len(self.ksizes) + 1) * c), dtype='float32')
        self.name = name

    def run(self):
        a = np.ascontiguousarray(self.in_node.result, dtype=np.float32)
        sizes = (ctypes.c_int * len(self.ksizes))(*self.ksizes)
        rc = mylib.dnn_spp_host(_vp(a), _vp(self.result), *map(int, a.shape), len(self.ksizes), sizes,
                                1 if self.x_first else 0)
        _check(rc, self.name)


class Input(DnnNode):
    """proj3/dnn_openblas.py:287-300 (unchanged contract)."""

    def __init__(self, name, in_shape):
        self.name = name
        self.in_shape = in_shape
        self.result = np.ndarray(self.in_shape)

    def set_input(self, tensor):
        assert tuple(self.in_shape) == tuple(tensor.shape)
        self.result = tensor

    def run(self):
        pass


# ---------------------------------------------------------------------------------------
# Graph -> plan lowering
# ---------------------------------------------------------------------------------------
class ConvEntry(object):
    """One fused plan conv: Conv2D [-> BiasAdd] [-> BatchNorm] [-> LeakyReLU]."""

    def __init__(self, conv):
        self.conv, self.bias, self.bn, self.leaky = conv, None, None, False
        self.nodes = [conv]


class PaddedConvEntry(object):
    """dnn_plan_add_conv_padded: Conv2DPadded (or a Conv2D whose pads are the same on both sides)
    [-> ScaleShift] [-> LeakyReLU | LeakyReLUF32]; `pads` = (pad_h, pad_w), `affine` the ScaleShift
    node or None, `leaky` 0, or 2 for LeakyReLUF32, or None for a LeakyReLU (the plan's
    leaky_variant)."""

    def __init__(self, conv, pads):
        self.conv, self.pads, self.affine, self.leaky = conv, tuple(pads), None, 0
        self.nodes = [conv]


class PoolEntry(object):
    def __init__(self, pool):
        self.pool = pool
        self.nodes = [pool]


class StashEntry(object):
    """dnn_plan_add_stash: the current tensor becomes slot `slot` (no kernel)."""

    def __init__(self, slot):
        self.slot = slot
        self.nodes = []


class RestoreEntry(object):
    """dnn_plan_add_restore: slot `slot` becomes the current tensor (no kernel)."""

    def __init__(self, slot):
        self.slot = slot
        self.nodes = []


class RouteEntry(object):
    """dnn_plan_add_route: space_to_depth(current, block) concatenated with slot `slot`'s tensor
    (-1: none), the slot's channels first with slot_first."""

    def __init__(self, block, slot=-1, slot_first=False, nodes=()):
        self.block, self.slot, self.slot_first = int(block), int(slot), bool(slot_first)
        self.nodes = list(nodes)


class ShortcutEntry(object):
    """dnn_plan_add_shortcut: current = act(current + slot `slot`'s tensor); `leaky` when a
    LeakyReLU directly after the Add is folded in."""

    def __init__(self, slot, leaky=False, nodes=()):
        self.slot, self.leaky = int(slot), bool(leaky)
        self.nodes = list(nodes)


class ReleaseEntry(object):
    """dnn_plan_add_release: slot `slot` stops being live; its number and region are reused."""

    def __init__(self, slot):
        self.slot = int(slot)
        self.nodes = []


class UpsampleEntry(object):
    """dnn_plan_add_upsample: nearest-neighbour upsample of the current tensor by `factor`."""

    def __init__(self, factor, nodes=()):
        self.factor = int(factor)
        self.nodes = list(nodes)


class SppEntry(object):
    """dnn_plan_add_spp: the stride-1 SAME max pools `ksizes` of the current tensor and the tensor
    itself (first with x_first, else last) as channel blocks of one output."""

    def __init__(self, ksizes, x_first=False, nodes=()):
        self.ksizes, self.x_first = _spp_sizes(ksizes), bool(x_first)
        self.nodes = list(nodes)


class SliceEntry(object):
    """dnn_plan_add_slice: channels [first, first + channels) of the current tensor."""

    def __init__(self, first, channels, nodes=()):
        self.first, self.channels = int(first), int(channels)
        self.nodes = list(nodes)


class TapEntry(object):
    """dnn_plan_add_tap: the current tensor becomes the plan's extra output `index` (no kernel);
    `node` is the graph node it is the result of (None in plans assembled by hand)."""

    def __init__(self, index, node=None):
        self.index = int(index)
        self.node = node
        self.nodes = []


def _is_output(g, node):
    return g.is_out_node(node) or any(n is node for n in getattr(g, "extra_out_nodes", ()))


def _free_slots(live, count):
    """The `count` lowest slot numbers not in `live` (dnn_plan_add_stash hands them out so)."""
    out, k = [], 0
    while len(out) < count:
        if k not in live:
            out.append(k)
        k += 1
    return out


def _lower_one(g, nxt):
    """The plan entry that starts at node `nxt`, and the last node it covers; None if `nxt` is
    not the start of one."""
    if isinstance(nxt, ScaleShift):
        raise DnnHipError(f"{nxt.name}: a ScaleShift exists in a plan only as the epilogue of the conv directly "
                          "before it (Conv2DPadded, or a Conv2D padded alike on both sides, with no BiasAdd / "
                          "BatchNorm and no other consumer in between); run the graph with debug=True otherwise")
    if isinstance(nxt, (Conv2D, Conv2DPadded)):
        nn = list(g.G.successors(nxt))
        follows = not _is_output(g, nxt) and len(nn) == 1 and isinstance(nn[0], (ScaleShift, LeakyReLUF32))
        if isinstance(nxt, Conv2DPadded):
            pads = nxt.pads
        elif follows and nxt.pad_top == nxt.pad_bottom and nxt.pad_left == nxt.pad_right:
            pads = (nxt.pad_top, nxt.pad_left)  # VALID, or a SAME that pads alike on both sides
        else:
            pads = None
        if pads is not None:
            e = PaddedConvEntry(nxt, pads)
            cur = nxt
            for kinds in ((ScaleShift,), (LeakyReLU, LeakyReLUF32)):
                nn = list(g.G.successors(cur))
                if _is_output(g, cur) or len(nn) != 1 or not isinstance(nn[0], kinds):
                    continue
                cur = nn[0]
                if isinstance(cur, ScaleShift):
                    e.affine = cur
                else:
                    e.leaky = 2 if isinstance(cur, LeakyReLUF32) else None
                e.nodes.append(cur)
            nn = list(g.G.successors(cur))
            if cur is nxt and not _is_output(g, cur) and len(nn) == 1 and isinstance(nn[0], (BiasAdd, BatchNorm)):
                return None  # BiasAdd / BatchNorm are dnn_plan_add_conv's epilogue: use ScaleShift
            return e, cur
        e = ConvEntry(nxt)
        cur = nxt
        for kind in (BiasAdd, BatchNorm, LeakyReLU):
            nn = list(g.G.successors(cur))
            if _is_output(g, cur) or len(nn) != 1 or not isinstance(nn[0], kind):
                continue
            cur = nn[0]
            if kind is BiasAdd:
                e.bias = cur
            elif kind is BatchNorm:
                e.bn = cur
            else:
                e.leaky = True
            e.nodes.append(cur)
        return e, cur
    if isinstance(nxt, MaxPool2D):
        return PoolEntry(nxt), nxt
    if isinstance(nxt, SpaceToDepth):
        return RouteEntry(nxt.block, nodes=[nxt]), nxt
    if isinstance(nxt, Upsample):
        return UpsampleEntry(nxt.factor, nodes=[nxt]), nxt
    if isinstance(nxt, ChannelSlice):
        return SliceEntry(nxt.first, nxt.channels, nodes=[nxt]), nxt
    if isinstance(nxt, Spp):
        return SppEntry(nxt.ksizes, nxt.x_first, nodes=[nxt]), nxt
    return None  # a standalone element-wise op: not expressible as a fused entry


def _lower_chain(g, chain):
    """The entries of a plain chain of nodes, or None."""
    es, i = [], 0
    while i < len(chain):
        r = _lower_one(g, chain[i])
        if r is None:
            return None
        es.append(r[0])
        i += len(r[0].nodes)
    return es


def _lower_fork(g, x, heads, live, nested=False):
    """Node `x` has the two successors `heads`: lower the two chains up to the Concat or Add that
    joins them.  Returns (entries, the last node covered, live slots afterwards), or None for
    anything but two plain chains (either may be empty) meeting in one Concat or one Add.  `live`
    is the set of slot numbers in use; new slots are the lowest free numbers.  An Add block releases
    every slot it opens, so any number of them fit in sequence.  A Concat fork keeps its slots to
    the end of the plan, unless it is `nested`: lowered inside a pending long skip (another slot is
    live then: a CSP block's inner fork), it gives them back with ReleaseEntry right after its
    RouteEntry."""
    chains, joins = [], []
    for cur in heads:
        chain = []
        while not (isinstance(cur, (Concat, Add)) and len(list(g.G.predecessors(cur))) == 2):
            succ = list(g.G.successors(cur))
            if len(list(g.G.predecessors(cur))) != 1 or len(succ) != 1 or _is_output(g, cur):
                return None  # a nested fork, a join of another kind, or an output inside a branch
            chain.append(cur)
            cur = succ[0]
        chains.append(chain)
        joins.append(cur)
    join = joins[0]
    if joins[1] is not join:
        return None
    tails = [c[-1] if c else x for c in chains]
    if tails[0] is join.in_nodes[1] and tails[1] is join.in_nodes[0]:
        chains.reverse()
    elif not (tails[0] is join.in_nodes[0] and tails[1] is join.in_nodes[1]):
        return None
    lowered = []  # the join's inputs in order
    for chain in chains:
        es = _lower_chain(g, chain)
        if es is None:
            return None
        lowered.append(es)
    if isinstance(join, Add):
        return _emit_add_block(g, join, lowered, live)

    def ends_in_s2d(es):
        return bool(es) and isinstance(es[-1], RouteEntry) and es[-1].slot < 0

    # the branch lowered last is the route's `a` (the other one waits in a slot): the non-empty
    # one, then the one that ends in a SpaceToDepth (it fuses into the route), then the second
    if not lowered[0]:
        last = 1
    elif not lowered[1]:
        last = 0
    else:
        last = 0 if ends_in_s2d(lowered[0]) and not ends_in_s2d(lowered[1]) else 1
    first = 1 - last
    x_slot, b_new = _free_slots(live, 2)
    entries = [StashEntry(x_slot)]
    used = {x_slot}
    b_slot = x_slot
    if lowered[first]:
        b_slot = b_new
        used.add(b_slot)
        entries += lowered[first] + [StashEntry(b_slot), RestoreEntry(x_slot)]
    if max(used) >= MAX_SLOTS:
        return None
    tail = list(lowered[last])
    block, nodes = 1, [join]
    if ends_in_s2d(tail):
        s2d = tail.pop()
        block, nodes = s2d.block, s2d.nodes + [join]
    entries += tail + [RouteEntry(block, b_slot, slot_first=(first == 0), nodes=nodes)]
    if nested:  # the route has read both, and nothing later names them
        return entries + [ReleaseEntry(s) for s in sorted(used)], join, live
    return entries, join, live | used


def _emit_add_block(g, join, lowered, live):
    """The entries of a fork joined by the Add `join` (its inputs' chains lowered in `lowered`):
    Stash(x), f..., Shortcut(x), Release(x) with one empty branch, else Stash(x), first..., Stash(a),
    Restore(x), second..., Shortcut(a), Release(x), Release(a).  The slots are the lowest free
    numbers and are all released, so at most two are live on top of the ones already in use."""
    last_node, leaky = join, False
    succ = list(g.G.successors(join))
    if not _is_output(g, join) and len(succ) == 1 and isinstance(succ[0], LeakyReLU) \
            and len(list(g.G.predecessors(succ[0]))) == 1:
        last_node, leaky = succ[0], True  # a single LeakyReLU directly after the Add: the shortcut's activation
    nodes = [join] + ([last_node] if leaky else [])
    x_slot, a_slot = _free_slots(live, 2)
    if not lowered[0] or not lowered[1]:
        if x_slot + 1 > MAX_SLOTS or not (lowered[0] or lowered[1]):
            return None
        entries = [StashEntry(x_slot)] + (lowered[0] or lowered[1])
        entries += [ShortcutEntry(x_slot, leaky, nodes), ReleaseEntry(x_slot)]
        return entries, last_node, live
    if a_slot + 1 > MAX_SLOTS:
        return None
    entries = [StashEntry(x_slot)] + lowered[0] + [StashEntry(a_slot), RestoreEntry(x_slot)] + lowered[1]
    entries += [ShortcutEntry(a_slot, leaky, nodes), ReleaseEntry(x_slot), ReleaseEntry(a_slot)]
    return entries, last_node, live


def _output_branch(g, head):
    """The nodes of a plain chain from `head` to an extra output without successors, or None."""
    chain, cur = [], head
    while True:
        if len(list(g.G.predecessors(cur))) != 1:
            return None
        chain.append(cur)
        succ = list(g.G.successors(cur))
        if not succ:
            return chain if _is_output(g, cur) and not g.is_out_node(cur) else None
        if len(succ) != 1 or _is_output(g, cur):
            return None
        cur = succ[0]


def lower_graph(g):
    """Lower a builder graph to fused plan entries, or None if the plan cannot express it (then
    the node-by-node path runs).  Expressible: a chain of Conv2D (with its BiasAdd / BatchNorm /
    LeakyReLU), MaxPool2D, SpaceToDepth, Upsample, ChannelSlice and Spp, and forks of two such chains (either may be
    empty) joined by one Concat or one Add (with a LeakyReLU directly after it), any number of
    them in sequence within the plan's slots (an Add block gives its slots back, and so does a
    Concat fork lowered inside a pending long skip); forks nested in a fork's branch are not.
    Graphs with extra outputs (add_out_node) add patterns at a node x with two successors:

      output branch  one successor starts a plain chain that ends in an extra output without
                     successors: Stash(x), the chain, Tap, Restore(x), Release(x), and the
                     lowering goes on from x's other successor;
      long skip      one successor is a Concat that takes x directly and whose other input the
                     main line produces later, whatever complete blocks lie in between:
                     Stash(x), the main line, Route(1, slot, slot_first = x is the Concat's first
                     input), Release(slot).  A long skip into an Add is not expressible.  A
                     Concat-joined fork may lie inside a long skip (a CSP block: the skip is
                     concat[A, D], the fork concat[C, B] inside it); it releases its slots after
                     its Route, so a sequence of such blocks stays within the plan's slots;
      arrival plus   x has two successors, the pending Concat of a long skip that the main line
      a new skip     arrives at with x, and a Concat of a NEW long skip from x (YOLOv4-tiny's layer
                     23: the end of the third CSP block and the lateral of the top-down merge):
                     Stash(x), then the pending Route(1, slot, ...) and Release(slot); the new skip
                     is resolved where the main line reaches its Concat.

    An extra output on the main line is a Tap after the entry that computes it.  Slots are the
    lowest free numbers; more than MAX_SLOTS live at once gives None.

    A Conv2DPadded [-> ScaleShift] [-> LeakyReLU | LeakyReLUF32] is one PaddedConvEntry
    (dnn_plan_add_conv_padded), and so is a Conv2D directly followed by a ScaleShift or a
    LeakyReLUF32 when its SAME / VALID pads are the same on both sides.  A ScaleShift anywhere else
    has no plan form: DnnHipError (the node-by-node path, debug=True, runs any graph)."""
    if g.in_node is None or g.out_node is None:
        return None
    extras = list(getattr(g, "extra_out_nodes", ()))
    if any(g.is_out_node(n) for n in extras) or len(extras) > MAX_TAPS:
        return None
    entries = []
    live = set()      # slot numbers in use
    pending = {}      # Concat of a long skip -> (slot, x)
    handled = set()   # (x, successor) edges already dealt with: output-branch heads, long-skip Concats
    tapped = []

    def tap(node):
        if any(n is node for n in extras):
            entries.append(TapEntry(len(tapped), node))
            tapped.append(node)

    def long_skip(succ):
        """Stash `node` for the one Concat among `succ` that takes it directly; False if there is
        not exactly one, or no slot."""
        skips = [h for h in succ if isinstance(h, Concat) and len(list(g.G.predecessors(h))) == 2
                 and (h.in_nodes[0] is node) != (h.in_nodes[1] is node)]
        slot = _free_slots(live, 1)[0]
        if len(skips) != 1 or slot >= MAX_SLOTS:
            return False
        entries.append(StashEntry(slot))
        live.add(slot)
        pending[skips[0]] = (slot, node)
        handled.add((node, skips[0]))
        return True

    node = g.in_node
    while not g.is_out_node(node):
        succ = [s for s in g.G.successors(node) if (node, s) not in handled]
        arriving = [s for s in succ if s in pending]
        if len(succ) == 2 and len(arriving) == 1:  # arrival plus a new long skip from this node
            if not long_skip([s for s in succ if s is not arriving[0]]):
                return None
            continue  # (the new skip's edge is handled: the arrival is the one successor left)
        if len(succ) == 1:
            nxt = succ[0]
            if nxt in pending:  # the main line arrives at a long skip's Concat
                slot, x = pending.pop(nxt)
                other = nxt.in_nodes[1] if nxt.in_nodes[0] is x else nxt.in_nodes[0]
                if other is not node or len(list(g.G.predecessors(nxt))) != 2:
                    return None
                entries += [RouteEntry(1, slot, slot_first=nxt.in_nodes[0] is x, nodes=[nxt]), ReleaseEntry(slot)]
                live.discard(slot)
                node = nxt
                tap(node)
                continue
            if len(list(g.G.predecessors(nxt))) != 1:
                return None
            r = _lower_one(g, nxt)
            if r is None:
                return None
            entries.append(r[0])
            node = r[1]
            tap(node)
        elif len(succ) == 2:
            r = _lower_fork(g, node, succ, live, nested=bool(pending))
            if r is not None:
                entries += r[0]
                node, live = r[1], set(r[2])
                tap(node)
                continue
            slot = _free_slots(live, 1)[0]
            if slot >= MAX_SLOTS:
                return None
            branches = [(h, _output_branch(g, h)) for h in succ]
            branches = [(h, c) for h, c in branches if c is not None]
            if branches:
                head, chain = branches[0]
                es = _lower_chain(g, chain)
                if es is None:
                    return None
                entries += [StashEntry(slot)] + es
                tap(chain[-1])
                entries += [RestoreEntry(slot), ReleaseEntry(slot)]
                handled.add((node, head))
                continue
            if not long_skip(succ):
                return None
        elif len(succ) == 3:  # a long skip from a node that also opens a fork (a residual block's input)
            if not long_skip(succ):
                return None
        else:
            return None
    if not entries or pending or len(tapped) != len(extras) or isinstance(entries[-1], TapEntry):
        return None
    return entries


def clock_stamp(dev_ptr, nwg, stream_ptr, lib=None):
    """Launch the clock-stamp kernel (dnn_clock_stamp): nwg workgroups, 4 uint64 each at dev_ptr."""
    lib = lib or mylib
    _check(lib.dnn_clock_stamp(ctypes.c_void_p(stream_ptr), ctypes.c_void_p(dev_ptr), int(nwg)), "clock_stamp", lib)


def sclk_from_stamps(start, end):
    """Mean shader clock per XCD between two stamp launches (arrays [nwg][4] of uint64:
    s_memtime, s_memrealtime (100 MHz), XCC_ID, HW_ID): per XCD the median of each counter over
    its workgroups, then d(memtime) / d(memrealtime) x 100 MHz.  Returns {"mean", "min", "max",
    "per_xcd": {xcd: GHz}, "window_us"} (GHz, the mean over XCDs)."""
    import numpy as np
    a, b = np.asarray(start, dtype=np.uint64), np.asarray(end, dtype=np.uint64)
    per = {}
    win = []
    for x in sorted(set(int(v) for v in a[:, 2]) & set(int(v) for v in b[:, 2])):
        sa, sb = a[a[:, 2] == x], b[b[:, 2] == x]
        dt = float(np.median(sb[:, 0].astype(np.float64))) - float(np.median(sa[:, 0].astype(np.float64)))
        dr = float(np.median(sb[:, 1].astype(np.float64))) - float(np.median(sa[:, 1].astype(np.float64)))
        if dr > 0 and dt > 0:
            per[x] = dt / dr * 0.1  # memrealtime ticks at 100 MHz: GHz = (dt / dr) x 0.1
            win.append(dr * 0.01)   # microseconds
    if not per:
        return None
    v = list(per.values())
    return {"mean": sum(v) / len(v), "min": min(v), "max": max(v), "per_xcd": per,
            "window_us": sum(win) / len(win)}


def _pad_code(padding):
    return 1 if padding == 'SAME' else 0


def _add_structural(lib, h, e, leaky_variant=1):
    """Emit a StashEntry / RestoreEntry / RouteEntry / ShortcutEntry / ReleaseEntry /
    UpsampleEntry / SppEntry / SliceEntry / TapEntry; False if `e` is none of them."""
    if isinstance(e, StashEntry):
        slot = ctypes.c_int(-1)
        _check(lib.dnn_plan_add_stash(h, ctypes.byref(slot)), "dnn_plan_add_stash", lib)
        if slot.value != e.slot:
            raise DnnHipError(f"dnn_plan_add_stash gave slot {slot.value}, the lowering expected {e.slot}")
    elif isinstance(e, RestoreEntry):
        _check(lib.dnn_plan_add_restore(h, e.slot), "dnn_plan_add_restore", lib)
    elif isinstance(e, RouteEntry):
        _check(lib.dnn_plan_add_route(h, e.block, e.slot, 1 if e.slot_first else 0), "dnn_plan_add_route", lib)
    elif isinstance(e, ShortcutEntry):
        _check(lib.dnn_plan_add_shortcut(h, e.slot, leaky_variant if e.leaky else 0), "dnn_plan_add_shortcut", lib)
    elif isinstance(e, ReleaseEntry):
        _check(lib.dnn_plan_add_release(h, e.slot), "dnn_plan_add_release", lib)
    elif isinstance(e, UpsampleEntry):
        _check(lib.dnn_plan_add_upsample(h, e.factor), "dnn_plan_add_upsample", lib)
    elif isinstance(e, SppEntry):
        sizes = (ctypes.c_int * len(e.ksizes))(*e.ksizes)
        _check(lib.dnn_plan_add_spp(h, len(e.ksizes), sizes, 1 if e.x_first else 0), "dnn_plan_add_spp", lib)
    elif isinstance(e, SliceEntry):
        _check(lib.dnn_plan_add_slice(h, e.first, e.channels), "dnn_plan_add_slice", lib)
    elif isinstance(e, TapEntry):
        index = ctypes.c_int(-1)
        _check(lib.dnn_plan_add_tap(h, ctypes.byref(index)), "dnn_plan_add_tap", lib)
        if index.value != e.index:
            raise DnnHipError(f"dnn_plan_add_tap gave index {index.value}, the lowering expected {e.index}")
    else:
        return False
    return True


class Plan(object):
    """Owner of a dnn_plan handle (include/dnn_hip_plan.h)."""

    def __init__(self, batch, in_shape, entries, device=0, weights_ptr=None, workspace_ptr=None, upload=True,
                 leaky_variant=1, lib=None, precision="fp32", latency=False):
        self.lib = lib or mylib
        self.batch = int(batch)
        self.in_shape = tuple(int(v) for v in in_shape)
        self.precision = _precision(precision)
        h = ctypes.c_void_p()
        _check(self.lib.dnn_plan_create(self.batch, *self.in_shape, ctypes.byref(h)), "dnn_plan_create", self.lib)
        self.h = h
        _check(self.lib.dnn_plan_set_precision(self.h, PRECISIONS[self.precision]), "dnn_plan_set_precision",
               self.lib)
        self.latency = bool(latency)
        if self.latency:
            _check(self.lib.dnn_plan_set_latency_mode(self.h, 1), "dnn_plan_set_latency_mode", self.lib)
        self.entries = entries
        for e in entries:
            if _add_structural(self.lib, self.h, e, leaky_variant):
                continue
            if isinstance(e, PaddedConvEntry):
                c = e.conv
                kh, kw, _, od = c.kernel.shape
                scale = e.affine.scale if e.affine is not None else None
                shift = e.affine.shift if e.affine is not None else None
                keep = (c.kernel, scale, shift)  # noqa: F841 (alive across the call)
                rc = self.lib.dnn_plan_add_conv_padded(
                    self.h, kh, kw, od, int(c.strides[1]), int(c.strides[2]), e.pads[0], e.pads[1],
                    _vp(c.kernel) if upload else None, _vp(scale), _vp(shift),
                    leaky_variant if e.leaky is None else e.leaky)
                _check(rc, "dnn_plan_add_conv_padded", self.lib)
            elif isinstance(e, ConvEntry):
                c = e.conv
                kh, kw, _, od = c.kernel.shape
                bias = e.bias.biases if e.bias is not None else None
                if e.bn is not None:
                    mean, var, gamma, eps = e.bn.mean, e.bn.variance, e.bn.gamma, float(e.bn.epsilon)
                else:
                    mean = var = gamma = None
                    eps = 0.0
                keep = (c.kernel, bias, mean, var, gamma)  # noqa: F841 (alive across the call)
                rc = self.lib.dnn_plan_add_conv(
                    self.h, kh, kw, od, int(c.strides[1]), int(c.strides[2]), _pad_code(c.padding),
                    # without upload only the kernel is withheld: the epilogue pointers still
                    # declare which of bias / BN the layer has (the values arrive with the arena)
                    _vp(c.kernel) if upload else None, _vp(bias), _vp(mean), _vp(var), _vp(gamma), eps,
                    leaky_variant if e.leaky else 0)
                _check(rc, "dnn_plan_add_conv", self.lib)
            else:
                p = e.pool
                _check(self.lib.dnn_plan_add_max_pool(self.h, int(p.ksize[1]), int(p.ksize[2]), int(p.strides[1]),
                                                      int(p.strides[2]), _pad_code(p.padding)),
                       "dnn_plan_add_max_pool", self.lib)
        b, oh, ow, oc = (ctypes.c_int() for _ in range(4))
        _check(self.lib.dnn_plan_output_shape(self.h, ctypes.byref(b), ctypes.byref(oh), ctypes.byref(ow),
                                              ctypes.byref(oc)), "dnn_plan_output_shape", self.lib)
        self.out_shape = (oh.value, ow.value, oc.value)
        self.tap_entries = [e for e in entries if isinstance(e, TapEntry)]
        self.tap_shapes = []  # per tap (h, w, c), in tap order
        for k in range(self.lib.dnn_plan_num_taps(self.h)):
            th, tw, tc = (ctypes.c_int() for _ in range(3))
            _check(self.lib.dnn_plan_tap_shape(self.h, k, ctypes.byref(th), ctypes.byref(tw), ctypes.byref(tc)),
                   "dnn_plan_tap_shape", self.lib)
            self.tap_shapes.append((th.value, tw.value, tc.value))
        self.device = device
        _check(self.lib.dnn_plan_finalize(self.h, device, weights_ptr, workspace_ptr), "dnn_plan_finalize",
               self.lib)

    @classmethod
    def from_graph(cls, g, device=0, **kw):
        entries = lower_graph(g)
        if entries is None:
            raise DnnHipError("graph is not a conv/pool chain (with Concat- or Add-joined forks) the fused plan can express")
        return cls(g.in_node.in_shape[0], tuple(g.in_node.in_shape[1:]), entries, device=device, **kw)

    @staticmethod
    def _declared(batch, in_shape, entries, lib, precision, latency, kernels=False):
        """A plan handle with the entries' shapes declared (no weights, not finalized: no device).
        `kernels`: the conv kernels are passed too (the pieces choice checks their range)."""
        h = ctypes.c_void_p()
        _check(lib.dnn_plan_create(int(batch), *in_shape, ctypes.byref(h)), "dnn_plan_create", lib)
        try:
            _check(lib.dnn_plan_set_precision(h, PRECISIONS[_precision(precision)]), "dnn_plan_set_precision", lib)
            if latency:
                _check(lib.dnn_plan_set_latency_mode(h, 1), "dnn_plan_set_latency_mode", lib)
            for e in entries:
                if _add_structural(lib, h, e):
                    continue
                if isinstance(e, PaddedConvEntry):
                    kh, kw, _, od = e.conv.kernel.shape
                    sc = _vp(e.affine.scale) if e.affine is not None else None  # (only says: affine or not)
                    _check(lib.dnn_plan_add_conv_padded(h, kh, kw, od, int(e.conv.strides[1]), int(e.conv.strides[2]),
                                                        e.pads[0], e.pads[1], None, sc, sc,
                                                        1 if e.leaky is None else e.leaky),
                           "dnn_plan_add_conv_padded", lib)
                elif isinstance(e, ConvEntry):
                    kh, kw, _, od = e.conv.kernel.shape
                    _check(lib.dnn_plan_add_conv(h, kh, kw, od, int(e.conv.strides[1]), int(e.conv.strides[2]),
                                                 _pad_code(e.conv.padding), _vp(e.conv.kernel) if kernels else None,
                                                 None, None, None, None, 0.0, 1 if e.leaky else 0),
                           "dnn_plan_add_conv", lib)
                else:
                    p = e.pool
                    _check(lib.dnn_plan_add_max_pool(h, int(p.ksize[1]), int(p.ksize[2]), int(p.strides[1]),
                                                     int(p.strides[2]), _pad_code(p.padding)),
                           "dnn_plan_add_max_pool", lib)
        except Exception:
            lib.dnn_plan_destroy(h)
            raise
        return h

    @staticmethod
    def memory(batch, in_shape, entries, lib=None, precision="fp32", latency=False):
        """(weight_bytes, workspace_bytes) a plan of this shape needs, without finalizing."""
        lib = lib or mylib
        h = Plan._declared(batch, in_shape, entries, lib, precision, latency)
        try:
            wb, sb = ctypes.c_size_t(), ctypes.c_size_t()
            _check(lib.dnn_plan_memory(h, ctypes.byref(wb), ctypes.byref(sb)), "dnn_plan_memory", lib)
            return wb.value, sb.value
        finally:
            lib.dnn_plan_destroy(h)

    @staticmethod
    def lowering(batch, in_shape, entries, lib=None, precision="fp32", latency=False):
        """dnn_plan_describe's text for a plan of this shape, without finalizing (needs no device)."""
        lib = lib or mylib
        h = Plan._declared(batch, in_shape, entries, lib, precision, latency)
        try:
            buf = ctypes.create_string_buffer(65536)
            _check(lib.dnn_plan_describe(h, buf, 65536), "dnn_plan_describe", lib)
            return buf.value.decode()
        finally:
            lib.dnn_plan_destroy(h)

    @staticmethod
    def lowering_pieces(batch, in_shape, entries, lib=None, precision="fp32", latency=False):
        """dnn_plan_describe_pieces' lines for a plan of this shape and these conv kernels,
        without finalizing (needs no device)."""
        lib = lib or mylib
        h = Plan._declared(batch, in_shape, entries, lib, precision, latency, kernels=True)
        try:
            buf = ctypes.create_string_buffer(65536)
            _check(lib.dnn_plan_describe_pieces(h, buf, 65536), "dnn_plan_describe_pieces", lib)
            return buf.value.decode().splitlines()
        finally:
            lib.dnn_plan_destroy(h)

    def pieces(self):
        """Per conv layer "convN pieces=h2|x3|-" (dnn_plan_describe_pieces)."""
        buf = ctypes.create_string_buffer(65536)
        _check(self.lib.dnn_plan_describe_pieces(self.h, buf, 65536), "dnn_plan_describe_pieces", self.lib)
        return buf.value.decode().splitlines()

    def describe(self):
        buf = ctypes.create_string_buffer(65536)
        _check(self.lib.dnn_plan_describe(self.h, buf, 65536), "dnn_plan_describe", self.lib)
        return buf.value.decode()

    def range_events(self):
        """Non-zero if a producer of an h2 layer's fp16 planes met a value outside fp16's range
        since the last call (dnn_plan_range_events: synchronises, reads and clears the word)."""
        ev = ctypes.c_uint()
        _check(self.lib.dnn_plan_range_events(self.h, ctypes.byref(ev)), "dnn_plan_range_events", self.lib)
        return ev.value

    def weight_buffer(self):
        p, n = ctypes.c_void_p(), ctypes.c_size_t()
        _check(self.lib.dnn_plan_weight_buffer(self.h, ctypes.byref(p), ctypes.byref(n)), "weight_buffer", self.lib)
        return p.value, n.value

    def run_host(self, x):
        x = np.ascontiguousarray(x, dtype=np.float32)
        n = x.shape[0]
        if tuple(x.shape[1:]) != self.in_shape or n > self.batch:
            raise ValueError(f"input {x.shape} does not fit plan [{self.batch}, {self.in_shape}]")
        out = np.empty((n,) + self.out_shape, dtype=np.float32)
        _check(self.lib.dnn_plan_run_host(self.h, n, _vp(x), _vp(out)), "dnn_plan_run_host", self.lib)
        return out

    def tap_buffer(self, k):
        """(device address, bytes for the planned batch) of tap `k` (dnn_plan_tap_buffer): after a
        run of n images the first n x h x w x c floats there are the tap's tensor."""
        p, n = ctypes.c_void_p(), ctypes.c_size_t()
        _check(self.lib.dnn_plan_tap_buffer(self.h, int(k), ctypes.byref(p), ctypes.byref(n)), "dnn_plan_tap_buffer",
               self.lib)
        return p.value, n.value

    def run_host_all(self, x):
        """run_host plus the taps: [tap 0, tap 1, ..., the plan's output] as host arrays."""
        out = self.run_host(x)
        n = out.shape[0]
        taps = []
        for k, shape in enumerate(self.tap_shapes):
            t = np.empty((n,) + shape, dtype=np.float32)
            _check(self.lib.dnn_plan_tap_read_host(self.h, k, n, _vp(t)), "dnn_plan_tap_read_host", self.lib)
            taps.append(t)
        return taps + [out]

    def run_device(self, n, in_ptr, out_ptr, stream_ptr=None):
        _check(self.lib.dnn_plan_run(self.h, int(n), ctypes.c_void_p(in_ptr), ctypes.c_void_p(out_ptr),
                                     ctypes.c_void_p(stream_ptr) if stream_ptr else None),
               "dnn_plan_run", self.lib)

    def run_graph(self, n, in_ptr, out_ptr, stream_ptr):
        """run_device through a captured HIP graph (dnn_plan_run_graph): one submission per
        forward after the first call for these (n, in, out)."""
        _check(self.lib.dnn_plan_run_graph(self.h, int(n), ctypes.c_void_p(in_ptr), ctypes.c_void_p(out_ptr),
                                           ctypes.c_void_p(stream_ptr)), "dnn_plan_run_graph", self.lib)

    def kernels(self):
        out = []
        for i in range(self.lib.dnn_plan_num_kernels(self.h)):
            name = ctypes.create_string_buffer(64)
            fl, by = ctypes.c_double(), ctypes.c_double()
            _check(self.lib.dnn_plan_kernel_info(self.h, i, name, 64, ctypes.byref(fl), ctypes.byref(by)),
                   "kernel_info", self.lib)
            out.append({"name": name.value.decode(), "flops": fl.value, "bytes": by.value})
        return out

    def timing_begin(self, max_runs, only=None):
        """Per-kernel HIP events over the next runs; `only` = a kernel name: events around that
        kernel alone (dnn_plan_timing_begin_only)."""
        if only is None:
            _check(self.lib.dnn_plan_timing_begin(self.h, int(max_runs)), "timing_begin", self.lib)
            return
        idx = [k["name"] for k in self.kernels()].index(only)
        _check(self.lib.dnn_plan_timing_begin_only(self.h, int(max_runs), idx), "timing_begin_only", self.lib)

    def timing_end(self):
        nk = self.lib.dnn_plan_num_kernels(self.h)
        ms = (ctypes.c_double * nk)()
        cnt = (ctypes.c_longlong * nk)()
        _check(self.lib.dnn_plan_timing_end(self.h, ms, cnt), "timing_end", self.lib)
        return list(ms), list(cnt)

    def clock_begin(self, kernel, dev_buf_ptr, max_runs, nwg):
        """Shader-clock stamps around `kernel` (a kernel name) in the next runs, into a device
        buffer of max_runs x 8 x nwg uint64 (dnn_plan_clock_begin; sclk_from_stamps reads them)."""
        idx = [k["name"] for k in self.kernels()].index(kernel)
        _check(self.lib.dnn_plan_clock_begin(self.h, idx, ctypes.c_void_p(dev_buf_ptr), int(max_runs), int(nwg)),
               "clock_begin", self.lib)

    def clock_end(self):
        runs = ctypes.c_int()
        _check(self.lib.dnn_plan_clock_end(self.h, ctypes.byref(runs)), "clock_end", self.lib)
        return runs.value

    def set_mark(self, kernel):
        """Record an event right before `kernel` (a kernel name; None: off) in every later run
        (dnn_plan_set_mark); wait_mark(stream) makes a stream wait for the latest run's mark."""
        idx = -1 if kernel is None else [k["name"] for k in self.kernels()].index(kernel)
        _check(self.lib.dnn_plan_set_mark(self.h, idx), "set_mark", self.lib)

    def wait_mark(self, stream_ptr):
        _check(self.lib.dnn_plan_wait_mark(self.h, ctypes.c_void_p(stream_ptr)), "wait_mark", self.lib)

    def close(self):
        if getattr(self, "h", None):
            self.lib.dnn_plan_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
