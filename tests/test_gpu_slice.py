"""GPU: the channel-slice kernel (csrc/slice.hip) bit for bit against numpy slicing, in plans on
poisoned, guarded buffers (batch and latency mode, as the first entry, behind another entry, into a
slot region) and through dnn_slice_host; both widths of the kernel, aligned and not."""
import numpy as np
import pytest

import dnn_hip
import plan_fuzz_checks as K
import residual_cases as RS

pytestmark = pytest.mark.gpu

# (n, h, w, c, first, channels)
SHAPES = {
    "smallest": (1, 1, 1, 2, 1, 1),
    "16_byte_path": (2, 5, 7, 12, 4, 8),
    "first_not_multiple_of_4": (2, 5, 7, 12, 6, 6),
    "odd_counts": (2, 5, 7, 10, 5, 5),
    "several_workgroups": (3, 13, 13, 64, 32, 32),  # 507 pixels: the copy before it two passes of 256, itself one of 512
    "whole_tensor": (1, 26, 26, 128, 0, 128),       # 676 pixels in passes of 128: six workgroups, the last partial
}


def _x(shape, seed):
    return np.random.default_rng(6000 + seed).standard_normal(shape).astype(np.float32)


def _run(B, shape, entries, x, what, **kw):
    gp = RS.GuardedPlan(B, shape, entries, **kw)
    try:
        outs = [gp.run(x[:n], f"{what} n={n}") for n in sorted({B, 1})]
        return outs[-1], outs[0], gp.plan.describe(), [k["name"] for k in gp.plan.kernels()]
    finally:
        gp.close()


@pytest.mark.parametrize("name", list(SHAPES))
def test_slice_is_numpy_slicing_bit_for_bit(name):
    n, h, w, c, first, channels = SHAPES[name]
    x = _x((n, h, w, c), list(SHAPES).index(name))
    want = np.ascontiguousarray(x[..., first:first + channels])
    # behind another entry: the whole-tensor copy writes an activation buffer, the slice reads it
    entries = [dnn_hip.SliceEntry(0, c), dnn_hip.SliceEntry(first, channels)]
    full, one, text, kernels = _run(n, (h, w, c), entries, x, name)
    assert kernels == ["slice0", "slice1"]
    assert text.splitlines()[1] == f"slice {h}x{w}x{c} -> {h}x{w}x{channels} first={first}"
    K.check_bits(full, want, f"{name}: slice in a plan")
    K.check_bits(one, want[:1], f"{name}: slice in a plan, one image of {n}")
    # the host entry
    out = np.full(want.shape, np.nan, np.float32)
    rc = dnn_hip.mylib.dnn_slice_host(dnn_hip._vp(x), dnn_hip._vp(out), n, h, w, c, first, channels)
    assert rc == 0, dnn_hip.last_error()
    K.check_bits(out, want, f"{name}: dnn_slice_host")
    # and the node
    g = dnn_hip.DnnGraphBuilder()
    t = g.create_channel_slice(g.create_input([n, h, w, c]), first, channels)
    g.in_node.set_input(x)
    t.run()
    K.check_bits(t.result, want, f"{name}: ChannelSlice.run")


def test_slice_in_a_latency_plan():
    n, h, w, c, first, channels = 1, 13, 13, 64, 32, 32
    x = _x((n, h, w, c), 20)
    full, _, text, _ = _run(n, (h, w, c), [dnn_hip.SliceEntry(0, c), dnn_hip.SliceEntry(first, channels)], x, "latency",
                            latency=True)
    K.check_bits(full, x[..., first:first + channels], "slice in a latency plan")


@pytest.mark.parametrize("name", ["16_byte_path", "odd_counts"])
def test_slice_as_the_first_entry_reads_the_callers_input(name):
    n, h, w, c, first, channels = SHAPES[name]
    x = _x((n, h, w, c), 30)
    full, one, text, kernels = _run(n, (h, w, c), [dnn_hip.SliceEntry(first, channels)], x, f"first entry {name}")
    assert kernels == ["slice0"]
    K.check_bits(full, x[..., first:first + channels], "slice of the caller's input")
    K.check_bits(one, x[:1, ..., first:first + channels], "slice of the caller's input, one image")


def test_slice_into_a_slot_region_and_out_of_one():
    """slice -> stash (the slice writes the slot's region) -> slice of it -> concat with the slot."""
    n, h, w, c = 2, 6, 9, 16
    x = _x((n, h, w, c), 40)
    entries = [dnn_hip.SliceEntry(8, 8), dnn_hip.StashEntry(0), dnn_hip.SliceEntry(1, 3),
               dnn_hip.RouteEntry(1, 0, slot_first=False), dnn_hip.ReleaseEntry(0)]
    full, _, _, kernels = _run(n, (h, w, c), entries, x, "slot region")
    assert kernels == ["slice0", "slice1", "route0"]
    K.check_bits(full, np.concatenate([x[..., 9:12], x[..., 8:16]], axis=3), "slice around a slot")


@pytest.mark.parametrize("in_off,out_off", [(1, 0), (0, 1), (3, 2)])
def test_unaligned_tensors_take_the_4_byte_path(in_off, out_off):
    """Channel counts that allow 16-byte accesses, tensors that do not (offsets in floats)."""
    import torch
    n, h, w, c, first, channels = SHAPES["16_byte_path"]
    x = _x((n, h, w, c), 50)
    want = np.ascontiguousarray(x[..., first:first + channels])
    plan = dnn_hip.Plan(n, (h, w, c), [dnn_hip.SliceEntry(first, channels)], device=0)
    try:
        xin = torch.full((x.size + 8,), float("nan"), dtype=torch.float32, device="cuda")
        xin[in_off:in_off + x.size] = torch.from_numpy(x.reshape(-1)).cuda()
        out = torch.full((want.size + 8,), K.CANARY, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        plan.run_device(n, xin.data_ptr() + 4 * in_off, out.data_ptr() + 4 * out_off)
        torch.cuda.synchronize()
        flat = out.cpu().numpy()
        K.check_bits(flat[out_off:out_off + want.size].view(np.float32).reshape(want.shape), want, "unaligned slice")
        assert (flat[:out_off] == K.CANARY).all() and (flat[out_off + want.size:] == K.CANARY).all()
    finally:
        plan.close()


def test_host_entry_refuses_bad_arguments():
    x = np.zeros((1, 2, 2, 4), np.float32)
    out = np.zeros((1, 2, 2, 4), np.float32)
    for first, channels in ((-1, 2), (0, 0), (2, 3), (4, 1)):
        assert dnn_hip.mylib.dnn_slice_host(dnn_hip._vp(x), dnn_hip._vp(out), 1, 2, 2, 4, first, channels) != 0
        assert "dnn_slice_host" in dnn_hip.last_error()
    # >= 2 GiB is refused from the arguments, before any allocation
    assert dnn_hip.mylib.dnn_slice_host(dnn_hip._vp(x), dnn_hip._vp(out), 64, 2048, 2048, 4, 0, 1) != 0
    assert "2 GiB" in dnn_hip.last_error()
