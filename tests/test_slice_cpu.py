"""CPU: the channel-slice plan entry (dnn_plan_add_slice) without a device: its argument checks, the
fp16 refusal, that a failed call leaves the plan unchanged, its lines in dnn_plan_describe and
dnn_plan_kernel_info, that it stops the conv / pool fusions, the ChannelSlice node and its lowering,
and that both libraries export the new symbols the headers declare."""
import ctypes
import os

import pytest

import dnn_hip

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = dnn_hip.mylib


class _Handle(object):
    """A bare dnn_plan handle (no device: never finalized)."""

    def __init__(self, batch, shape, precision="fp32", latency=False):
        self.h = ctypes.c_void_p()
        dnn_hip._check(LIB.dnn_plan_create(batch, *shape, ctypes.byref(self.h)), "dnn_plan_create")
        dnn_hip._check(LIB.dnn_plan_set_precision(self.h, dnn_hip.PRECISIONS[precision]), "dnn_plan_set_precision")
        if latency:
            dnn_hip._check(LIB.dnn_plan_set_latency_mode(self.h, 1), "dnn_plan_set_latency_mode")

    def describe(self):
        buf = ctypes.create_string_buffer(65536)
        dnn_hip._check(LIB.dnn_plan_describe(self.h, buf, 65536), "dnn_plan_describe")
        return buf.value.decode()

    def kernels(self):
        out = []
        for k in range(LIB.dnn_plan_num_kernels(self.h)):
            name = ctypes.create_string_buffer(64)
            fl, by = ctypes.c_double(), ctypes.c_double()
            dnn_hip._check(LIB.dnn_plan_kernel_info(self.h, k, name, 64, ctypes.byref(fl), ctypes.byref(by)), "kernel_info")
            out.append((name.value.decode(), fl.value, by.value))
        return out

    def shape(self):
        v = [ctypes.c_int() for _ in range(4)]
        dnn_hip._check(LIB.dnn_plan_output_shape(self.h, *[ctypes.byref(x) for x in v]), "dnn_plan_output_shape")
        return tuple(x.value for x in v)

    def close(self):
        LIB.dnn_plan_destroy(self.h)


@pytest.fixture
def handle():
    hs = []

    def make(*a, **kw):
        hs.append(_Handle(*a, **kw))
        return hs[-1]
    yield make
    for h in hs:
        h.close()


def test_both_libraries_export_the_new_symbols_and_the_headers_declare_them():
    plan_h = open(os.path.join(REPO, "include", "dnn_hip_plan.h")).read()
    post_h = open(os.path.join(REPO, "include", "dnn_hip_post.h")).read()
    plan_syms = ("dnn_plan_add_slice", "dnn_slice_host")
    post_syms = ("dnn_yolo_postprocess_multi_xy", "dnn_yolo_postprocess_multi_xy_host", "dnn_yolo_postprocess_wide_xy",
                 "dnn_yolo_postprocess_wide_xy_host")
    for name in ("libdnn_hip.so", "libdnn_hip_avx.so"):
        lib = dnn_hip.load_library(name)
        for sym in plan_syms + post_syms:
            assert hasattr(lib, sym), f"{name} does not export {sym}"
    for sym in plan_syms:
        assert f"int {sym}(" in plan_h
    for sym in post_syms:
        assert f"int {sym}(const dnn_yolo_multi* multi, const float* scale_x_y," in post_h
    doc = " ".join(plan_h[plan_h.index("Channel slice"):plan_h.index("int dnn_plan_add_slice")].replace("*", " ").split())
    assert "The reference has no such node" in doc


@pytest.mark.parametrize("first,channels", [(-1, 4), (0, 0), (0, -3), (4, 13), (16, 1), (0, 17), (2 ** 31 - 1, 2)])
def test_a_range_outside_the_tensor_fails_and_leaves_the_plan_unchanged(handle, first, channels):
    p = handle(2, (8, 8, 16))
    assert LIB.dnn_plan_add_slice(p.h, 4, 8) == 0
    before, shape = p.describe(), p.shape()
    assert shape == (2, 8, 8, 8)
    q = handle(2, (8, 8, 16))
    assert LIB.dnn_plan_add_slice(q.h, first, channels) != 0
    assert "dnn_plan_add_slice" in dnn_hip.last_error()
    assert q.describe() == "" and q.shape() == (2, 8, 8, 16)
    # ... and after an entry: 8 channels now, (4, 13), (0, 17), (16, 1) are still outside
    assert LIB.dnn_plan_add_slice(p.h, first, channels) != 0
    assert p.describe() == before and p.shape() == shape and len(p.kernels()) == 1


def test_fp16_plans_refuse_it_naming_fp16_as_the_stash_does(handle):
    p = handle(1, (8, 8, 16), precision="fp16")
    slot = ctypes.c_int(-1)
    assert LIB.dnn_plan_add_stash(p.h, ctypes.byref(slot)) != 0
    stash_err = dnn_hip.last_error()
    assert LIB.dnn_plan_add_slice(p.h, 0, 8) != 0
    err = dnn_hip.last_error()
    assert "fp16" in stash_err and "fp16" in err and "dnn_plan_add_slice" in err
    assert err.split(":", 1)[1] == stash_err.split(":", 1)[1]  # the same words after the entry's name
    assert p.describe() == "" and p.shape() == (1, 8, 8, 16)


def test_null_plan_is_refused():
    assert LIB.dnn_plan_add_slice(None, 0, 1) != 0


@pytest.mark.parametrize("latency", [False, True], ids=["batch", "latency"])
def test_describe_and_kernel_info(handle, latency):
    p = handle(3, (13, 13, 64), latency=latency)
    assert LIB.dnn_plan_add_slice(p.h, 32, 32) == 0
    assert LIB.dnn_plan_add_slice(p.h, 0, 32) == 0  # the whole tensor: allowed, still a kernel
    assert LIB.dnn_plan_add_slice(p.h, 5, 3) == 0
    assert p.describe().splitlines() == ["slice 13x13x64 -> 13x13x32 first=32", "slice 13x13x32 -> 13x13x32 first=0",
                                         "slice 13x13x32 -> 13x13x3 first=5"]
    assert p.shape() == (3, 13, 13, 3)
    px = 3 * 13 * 13
    assert p.kernels() == [("slice0", 0.0, 2.0 * 4 * px * 32), ("slice1", 0.0, 2.0 * 4 * px * 32),
                           ("slice2", 0.0, 2.0 * 4 * px * 3)]


def _conv(h, od, k=3):  # (kernel NULL: the shape only)
    return LIB.dnn_plan_add_conv(h, k, k, od, 1, 1, 1, None, None, None, None, None, 0.0, 1)


def test_it_stops_the_conv_and_pool_fusions(handle):
    """conv -> pool fuses; conv -> slice -> pool does not, and a conv after a slice reads plain NHWC."""
    fused = handle(2, (16, 16, 32))
    assert _conv(fused.h, 64) == 0 and LIB.dnn_plan_add_max_pool(fused.h, 2, 2, 2, 2, 1) == 0
    assert len(fused.describe().splitlines()) == 1 and "+pool2x2s2" in fused.describe()
    p = handle(2, (16, 16, 32))
    assert _conv(p.h, 64) == 0
    assert LIB.dnn_plan_add_slice(p.h, 32, 32) == 0
    assert LIB.dnn_plan_add_max_pool(p.h, 2, 2, 2, 2, 1) == 0
    assert _conv(p.h, 64) == 0
    lines = p.describe().splitlines()
    assert [l.split()[0] for l in lines] == ["conv", "slice", "pool", "conv"]
    assert "+pool" not in lines[0] and lines[1] == "slice 16x16x64 -> 16x16x32 first=32"
    assert lines[2].startswith("pool 16x16x32 -> 8x8x32")
    names = [k[0] for k in p.kernels()]
    assert "slice0" in names and "pool0" in names
    # a 3x3 conv behind a slice takes the mode it takes behind the plan's input (plain NHWC in)
    q = handle(2, (16, 16, 64))
    assert LIB.dnn_plan_add_slice(q.h, 0, 32) == 0 and _conv(q.h, 64) == 0
    r = handle(2, (16, 16, 32))
    assert _conv(r.h, 64) == 0
    assert q.describe().splitlines()[1] == r.describe().splitlines()[0]


def test_slot_and_tap_entries_around_a_slice(handle):
    p = handle(2, (8, 8, 16))
    slot, tap = ctypes.c_int(-1), ctypes.c_int(-1)
    assert LIB.dnn_plan_add_stash(p.h, ctypes.byref(slot)) == 0  # the caller's input
    assert LIB.dnn_plan_add_slice(p.h, 8, 8) == 0
    assert LIB.dnn_plan_add_tap(p.h, ctypes.byref(tap)) == 0     # the slice writes the tap's region
    assert LIB.dnn_plan_add_route(p.h, 1, slot.value, 0) == 0
    assert p.shape() == (2, 8, 8, 24)
    wb, sb = ctypes.c_size_t(), ctypes.c_size_t()
    assert LIB.dnn_plan_memory(p.h, ctypes.byref(wb), ctypes.byref(sb)) == 0
    assert sb.value >= 2 * 8 * 8 * 8 * 4


# ------------------------------------------------------------------------------ node and lowering
def _input(shape):
    g = dnn_hip.DnnGraphBuilder()
    return g, g.create_input(list(shape))


@pytest.mark.parametrize("first,channels", [(-1, 2), (0, 0), (3, 6), (8, 1), (0.5, 2), (0, True)])
def test_node_refuses_a_bad_range(first, channels):
    g, x = _input([1, 4, 4, 8])
    with pytest.raises(ValueError):
        g.create_channel_slice(x, first, channels)


def test_node_shape_and_lowering():
    g, x = _input([2, 6, 5, 12])
    t = g.create_channel_slice(x, 4, 8)
    assert t.result.shape == (2, 6, 5, 8) and t.name == "channel_slice_0" and (t.first, t.channels) == (4, 8)
    t = g.create_max_pool2d(t, [1, 2, 2, 1], [1, 2, 2, 1], "SAME")
    t = g.create_channel_slice(t, 0, 8)
    g.set_out_node(t)
    entries = dnn_hip.lower_graph(g)
    assert [type(e).__name__ for e in entries] == ["SliceEntry", "PoolEntry", "SliceEntry"]
    assert [(e.first, e.channels) for e in entries if isinstance(e, dnn_hip.SliceEntry)] == [(4, 8), (0, 8)]
    text = dnn_hip.Plan.lowering(2, (6, 5, 12), entries)
    assert text.splitlines() == ["slice 6x5x12 -> 6x5x8 first=4", "pool 6x5x8 -> 3x3x8 k2x2 s2",
                                 "slice 3x3x8 -> 3x3x8 first=0"]
    wb, sb = dnn_hip.Plan.memory(2, (6, 5, 12), entries)
    assert sb >= 2 * 2 * 6 * 5 * 12 * 4
    with pytest.raises(dnn_hip.DnnHipError, match="fp16"):
        dnn_hip.Plan.lowering(2, (6, 5, 12), entries, precision="fp16")
