"""GPU: scale_x_y in the multi-scale decode (the dnn_yolo_postprocess_*_xy entries;
yolo_post.MultiHead / WideHead with scale_x_y): rows, counts and per-image codes equal to
tests/post_xy_oracle.py in all three mode pairs, through the device and the host entries of both
decodes; with every scale at 1, or NULL, the bytes of the existing entries; the refused mode pair
and the refused values.  Every device call runs on poisoned buffers between guard bands."""
import ctypes

import numpy as np
import pytest

import dnn_hip
import plan_fuzz_checks as C
import post_head_cases as HK
import post_xy_cases as XK
import post_xy_oracle as XO
import yolo_post

pytestmark = pytest.mark.gpu

LIB = dnn_hip.mylib
KINDS = {"multi": yolo_post.MultiHead, "wide": yolo_post.WideHead}


def _guarded(torch, dev, nbytes):
    t = torch.full((2 * C.GUARD_BYTES + nbytes,), C.POISON, dtype=torch.uint8, device=dev)
    return t, t[C.GUARD_BYTES:C.GUARD_BYTES + nbytes]


def _old_call(head):
    """The existing device entry of a head's kind and mode, as (function, trailing mode arguments)."""
    if isinstance(head, yolo_post.WideHead):
        return LIB.dnn_yolo_postprocess_wide, (yolo_post.NMS_MODES[head.nms], yolo_post.LABEL_MODES[head.labels])
    if head.labels == "multi":
        return LIB.dnn_yolo_postprocess_multi_labels, (1,)
    if head.nms == "per_class":
        return LIB.dnn_yolo_postprocess_multi_nms, (1,)
    return LIB.dnn_yolo_postprocess_multi, ()


def _run_guarded(head, preds, entry="xy", xy="head"):
    """One device call on poisoned dets / counts / workspace between guard bands: (rc, counts as a
    list, dets as uint8 [n, max_det, 40], the workspace's bytes).  entry "xy": the _xy entry of the
    head's kind with `xy` (the head's array, None for NULL, or a ctypes float array); "old": the
    existing entry of the head's kind and mode."""
    import torch
    dev = torch.device("cuda", 0)
    n, max_det = preds[0].shape[0], head.max_det
    n_ws = head.workspace_bytes(n)
    stream = torch.cuda.current_stream(dev).cuda_stream
    xs = [torch.from_numpy(np.array(p)).to(dev) for p in preds]
    ptrs = (ctypes.c_void_p * len(xs))(*[x.data_ptr() for x in xs])
    dets_all, dets = _guarded(torch, dev, n * max_det * 40)
    counts_all, counts = _guarded(torch, dev, n * 4)
    ws_all, ws = _guarded(torch, dev, n_ws)
    torch.cuda.synchronize()
    if entry == "old":
        fn, tail = _old_call(head)
        rc = fn(ctypes.byref(head.c), ptrs, n, dets.data_ptr(), max_det, counts.data_ptr(), ws.data_ptr(), n_ws,
                *tail, stream)
    else:
        fn = LIB.dnn_yolo_postprocess_wide_xy if isinstance(head, yolo_post.WideHead) else LIB.dnn_yolo_postprocess_multi_xy
        rc = fn(ctypes.byref(head.c), head.xy if isinstance(xy, str) else xy, ptrs, n, dets.data_ptr(), max_det,
                counts.data_ptr(), ws.data_ptr(), n_ws, yolo_post.NMS_MODES[head.nms],
                yolo_post.LABEL_MODES[head.labels], stream)
    torch.cuda.synchronize()
    for buf, what in ((dets_all, "dets"), (counts_all, "counts"), (ws_all, "workspace")):
        C.check_guard(buf.cpu().numpy(), what)
    return (rc, [int(c) for c in counts.cpu().numpy().view(np.int32)], dets.cpu().numpy().reshape(n, max_det, 40),
            ws.cpu().numpy().copy())


def _check_images(counts, dets, want, what):
    assert counts == XK.counts_of(want), what
    for i, w in enumerate(want):
        if isinstance(w, int):
            assert (dets[i] == C.POISON).all(), f"{what} image {i}: rows written beside the code {w}"
            continue
        k = len(w)
        rows = yolo_post.DetectionBuffers.to_rows(dets[i:i + 1, :k], [k], max_det=k)[0]
        HK.same_rows(rows, list(w), f"{what} image {i}")
        assert [r[1:5] for r in rows] == [r[1:5] for r in w]  # the corners exactly
        assert (dets[i, k:] == C.POISON).all(), f"{what} image {i}: rows written after the count"


# ------------------------------------------------------------------ 1. against the oracle
@pytest.mark.parametrize("kind", sorted(KINDS))
@pytest.mark.parametrize("mode", XO.MODES)
@pytest.mark.parametrize("name", sorted(XK.HEADS))
def test_device_and_host_entries_against_the_oracle(name, mode, kind):
    head = XK.device_head(name, mode, KINDS[kind])
    assert head.scale_x_y == XK.xy_of(name) and "scale_x_y" in repr(head)
    preds, want = XK.inputs(name), XK.refs(name, mode)
    rc, counts, dets, _ = _run_guarded(head, preds)
    assert rc == 0, dnn_hip.last_error()
    print(f"{name} {mode} {kind}: device {counts}, oracle {XK.counts_of(want)}")
    _check_images(counts, dets, want, f"{name} {mode} {kind} device")
    rows = yolo_post.detect_batch_multi(list(preds), head, raise_errors=False)  # the _xy_host entry
    for i, w in enumerate(want):
        HK.same_rows(rows[i], w if isinstance(w, int) else list(w), f"{name} {mode} {kind} host image {i}")


def test_multi_detection_buffers_run_the_xy_entry():
    import torch
    name, mode = "two_scales", "multi"
    preds, want = XK.inputs(name), XK.refs(name, mode)
    for kind in sorted(KINDS):
        head = XK.device_head(name, mode, KINDS[kind])
        bufs = yolo_post.MultiDetectionBuffers(XK.IMAGES, torch.device("cuda", 0), head)
        xs = [torch.from_numpy(np.array(p)).cuda() for p in preds]
        bufs.run([x.data_ptr() for x in xs], XK.IMAGES, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        rows = yolo_post.DetectionBuffers.to_rows(bufs.dets.cpu().numpy(), bufs.counts.cpu().numpy(), bufs.max_det,
                                                  raise_errors=False)
        for i, w in enumerate(want):
            HK.same_rows(rows[i], w if isinstance(w, int) else list(w), f"buffers {kind} image {i}")


# ------------------------------------------------------------------ 2. identity at 1 and NULL
@pytest.mark.parametrize("kind", sorted(KINDS))
@pytest.mark.parametrize("mode", XO.MODES)
def test_all_ones_and_null_give_the_existing_entrys_bytes(mode, kind):
    name = "two_scales"
    preds = XK.inputs(name)
    plain = XK.device_head(name, mode, KINDS[kind], xy=None)
    assert plain.xy is None and "scale_x_y" not in repr(plain)
    ones = XK.device_head(name, mode, KINDS[kind], xy=(1.0, 1.0))
    rc0, counts0, dets0, ws0 = _run_guarded(plain, preds, entry="old")
    assert rc0 == 0 and any(c > 0 for c in counts0)
    for what, head, xy in (("ones", ones, "head"), ("NULL", plain, None)):
        rc, counts, dets, ws = _run_guarded(head, preds, xy=xy)
        assert rc == 0, dnn_hip.last_error()
        assert counts == counts0, what
        assert dets.tobytes() == dets0.tobytes(), f"{mode} {kind} {what}: dets differ from the existing entry's"
        # the workspace: every box's corners (what scale_x_y could move; the candidate lists behind
        # them are appended with atomics, in no fixed order)
        nb, base = plain.boxes, (XK.IMAGES * 64 if kind == "wide" else 0)
        for i in range(XK.IMAGES):
            lo = base + i * nb * 40
            assert ws[lo:lo + nb * 32].tobytes() == ws0[lo:lo + nb * 32].tobytes(), \
                f"{mode} {kind} {what}: image {i}'s boxes in the workspace differ from the existing entry's"
            assert (ws[lo:lo + nb * 32] != C.POISON).any()
    # ... and they are the oracle's rows at 1, not the moved ones
    _check_images(counts0, dets0, XK.refs(name, mode, (1.0, 1.0)), f"{mode} {kind} existing entry")
    assert XK.refs(name, mode, (1.0, 1.0)) != XK.refs(name, mode)


# ------------------------------------------------------------------ 3. refusals, before any launch
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_any_class_with_multi_label_returns_minus_two(kind):
    head = XK.device_head("two_scales", "multi", KINDS[kind])
    head.nms = "any"  # (the constructor refuses the pair; the C entry must too)
    rc, counts, dets, ws = _run_guarded(head, XK.inputs("two_scales"))
    assert rc == -2 and dnn_hip.last_error()
    for buf in (dets, ws, np.array(counts, np.int32).view(np.uint8)):
        assert (np.asarray(buf) == C.POISON).all()  # nothing ran
    dets_h = np.zeros((XK.IMAGES, 4), yolo_post.DETECTION_DTYPE)
    counts_h = np.zeros(XK.IMAGES, np.int32)
    ps = [np.ascontiguousarray(p) for p in XK.inputs("two_scales")]
    ptrs = (ctypes.c_void_p * 2)(*[p.ctypes.data for p in ps])
    fn = LIB.dnn_yolo_postprocess_wide_xy_host if kind == "wide" else LIB.dnn_yolo_postprocess_multi_xy_host
    assert fn(ctypes.byref(head.c), head.xy, ptrs, XK.IMAGES, dets_h.ctypes.data, 4, counts_h.ctypes.data, 0, 1) == -2


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), 0.0, -1.05])
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_a_bad_scale_fails_before_any_launch(kind, bad):
    head = XK.device_head("two_scales", "per_class", KINDS[kind], xy=None)
    xy = (ctypes.c_float * 2)(1.05, bad)
    rc, counts, dets, ws = _run_guarded(head, XK.inputs("two_scales"), xy=xy)
    assert rc == -2 and "scale_x_y" in dnn_hip.last_error()
    for buf in (dets, ws, np.array(counts, np.int32).view(np.uint8)):
        assert (np.asarray(buf) == C.POISON).all()  # nothing ran
    with pytest.raises(ValueError, match="scale_x_y"):
        XK.device_head("two_scales", "per_class", KINDS[kind], xy=(1.05, bad))
    with pytest.raises(ValueError, match="scale_x_y"):
        XK.device_head("two_scales", "per_class", KINDS[kind], xy=(1.05,))  # one value for two scales
