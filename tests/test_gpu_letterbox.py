"""Letterbox ingest and box correction on the MI355X against tests/letterbox_oracle.py: the kernel's
bits, a ragged batch at odd offsets, the box mapping on device buffers, the two-slot RaggedIngest
pipeline, and DarknetModel.detect_images end to end."""
import ctypes

import numpy as np
import pytest

import darknet_cases as DC
import darknet_import as D
import darknet_oracle as DO
import dnn_hip
import ingest
import letterbox_cases as LC
import letterbox_oracle as LB
import post_multi_oracle as MO
import post_multilabel_oracle as LO
import yolo_post

pytestmark = pytest.mark.gpu
lib = dnn_hip.mylib

_ORACLE = {}


def oracle(case, order="bgr", seed=0):
    """(image, letterbox_f32 of it), computed once per (case, order, seed) and shared; callers do not write to it."""
    key = (case, order, seed)
    if key not in _ORACLE:
        im = LC.image(case[0], case[1], seed)
        want = LB.letterbox_f32(im, case[2], case[3], order)
        want.setflags(write=False)
        _ORACLE[key] = (im, want)
    return _ORACLE[key]


# ------------------------------------------------------------------ 1. the kernel's bits
@pytest.mark.parametrize("order", ["bgr", "rgb"])
@pytest.mark.parametrize("case", LC.SMALL)
def test_letterbox_is_bit_exact(case, order):
    """Every table case of at most 100 pixels a side, both orders; net_w = 33 (3 * 33 = 99 floats a
    row) takes the one-float store path, the others the 16-byte one."""
    im, want = oracle(case, order)
    got = ingest.letterbox_gpu(im, case[2:], order)
    assert got.shape == want.shape and got.dtype == np.float32
    bad = np.argwhere(got != want)
    assert np.array_equal(got, want), f"{case} {order}: {len(bad)} elements differ, first {bad[:3].tolist()}"


def test_host_entry_equals_the_device_entry():
    case = (37, 53, 64, 96)
    im, want = oracle(case)
    out = np.full(want.shape, np.nan, np.float32)
    fr = (ingest.Frame * 1)(ingest.Frame(0, 37, 53))
    dnn_hip._check(lib.dnn_letterbox_frames_host(im.ctypes.data, im.size, fr, 1, out.ctypes.data, 64, 96, 0),
                   "dnn_letterbox_frames_host")
    assert np.array_equal(out, want)


def test_output_off_a_16_byte_boundary_takes_the_one_float_path():
    """3 * net_w is a multiple of 4 but the output pointer is not 16-byte aligned: the same bits,
    and the floats on either side of the frame stay."""
    import torch
    dev = torch.device("cuda", 0)
    case = (37, 53, 64, 96)
    im, want = oracle(case)
    flat = torch.full((want.size + 2,), float("nan"), dtype=torch.float32, device=dev)
    assert flat.data_ptr() % 16 == 0
    fr = (ingest.Frame * 1)(ingest.Frame(0, 37, 53))
    src = torch.from_numpy(im).to(dev)
    ingest.letterbox_device(src.data_ptr(), im.size, fr, 1, flat.data_ptr() + 4,
                            torch.cuda.current_stream(dev).cuda_stream, case[2:])
    got = flat.cpu().numpy()
    assert np.isnan(got[0]) and np.isnan(got[-1]) and np.array_equal(got[1:-1].reshape(want.shape), want)


# ------------------------------------------------------------------ 2. a ragged batch
RAGGED = [(37, 53), (5, 7), (100, 37), (48, 64), (16, 8)]  # images of one 64 x 96 batch


def test_ragged_batch_at_odd_offsets_in_another_order():
    import torch
    dev = torch.device("cuda", 0)
    net = (64, 96)
    pairs = [oracle(hw + net) for hw in RAGGED]
    # addresses: image 3 first, then 0, 4, 1, 2, each after an odd gap; listed in index order 0..4
    place, at, offsets = [3, 0, 4, 1, 2], 1, {}
    for k in place:
        offsets[k] = at
        at += pairs[k][0].size + (8 if pairs[k][0].size % 2 == 0 else 7)  # a gap that keeps every offset odd
    assert all(o % 2 == 1 for o in offsets.values())
    buf = np.full(at + 5, 0xAB, np.uint8)
    for k, (im, _) in enumerate(pairs):
        buf[offsets[k]:offsets[k] + im.size] = im.reshape(-1)
    frames = (ingest.Frame * 5)(*[ingest.Frame(offsets[k], *RAGGED[k]) for k in range(5)])
    d_px = torch.from_numpy(buf).to(dev)
    frame_floats = net[0] * net[1] * 3
    guard = 4096
    flat = torch.full((5 * frame_floats + guard,), float("nan"), dtype=torch.float32, device=dev)
    flat[5 * frame_floats:] = 12345.0
    s = torch.cuda.current_stream(dev).cuda_stream
    ingest.letterbox_device(d_px.data_ptr(), buf.size, frames, 5, flat.data_ptr(), s, net)
    got = flat.cpu().numpy()
    out, tail = got[:5 * frame_floats].reshape((5,) + net + (3,)), got[5 * frame_floats:]
    assert not np.isnan(out).any() and np.all(tail == np.float32(12345.0))
    for k, (_, want) in enumerate(pairs):
        assert np.array_equal(out[k], want), f"image {k} of the ragged batch"
    # fewer frames on the same stream: the slices beyond n stay as they are
    flat[:5 * frame_floats] = float("nan")
    two = (ingest.Frame * 2)(frames[4], frames[1])
    ingest.letterbox_device(d_px.data_ptr(), buf.size, two, 2, flat.data_ptr(), s, net)
    got = flat.cpu().numpy()
    out, tail = got[:5 * frame_floats].reshape((5,) + net + (3,)), got[5 * frame_floats:]
    assert np.array_equal(out[0], pairs[4][1]) and np.array_equal(out[1], pairs[1][1])
    assert np.isnan(out[2:]).all() and np.all(tail == np.float32(12345.0))


def test_more_frames_than_one_launch_carries():
    """70 frames: two launches (64 descriptors travel per launch), the second at its own output offset."""
    import torch
    dev = torch.device("cuda", 0)
    net = (32, 32)
    a, b = oracle((5, 7) + net), oracle((33, 17) + (32, 64))[0]
    b_want = LB.letterbox_f32(b, 32, 32)
    buf = np.concatenate([a[0].reshape(-1), b.reshape(-1)])
    frames = (ingest.Frame * 70)(*[ingest.Frame(0, 5, 7) if k % 3 else ingest.Frame(a[0].size, 33, 17)
                                   for k in range(70)])
    d_px = torch.from_numpy(buf).to(dev)
    out = torch.full((70,) + net + (3,), float("nan"), dtype=torch.float32, device=dev)
    ingest.letterbox_device(d_px.data_ptr(), buf.size, frames, 70, out.data_ptr(),
                            torch.cuda.current_stream(dev).cuda_stream, net)
    got = out.cpu().numpy()
    for k in range(70):
        assert np.array_equal(got[k], a[1] if k % 3 else b_want), f"frame {k}"


# ------------------------------------------------------------------ 3. boxes back
def _crafted():
    rng = np.random.default_rng(17)
    max_det = 300  # more rows than one workgroup's threads
    dets = np.zeros((3, max_det), yolo_post.DETECTION_DTYPE)
    for f in ("left", "top", "right", "bottom"):
        dets[f] = rng.integers(-40, 110, dets.shape)
    dets["cls"], dets["score"] = rng.integers(0, 3, dets.shape), rng.random(dets.shape)
    big = 2 ** 62
    dets[0, 0] = (1, 0.5, -big, -big, big, big)
    dets[0, 1] = (2, 0.25, big, big, -big, -big)
    dets[0, 2] = (0, 0.75, 5, 0, 9, 12)       # wholly in the top pad of image 0
    dets[2, 299] = (1, 0.5, -2 ** 63, 2 ** 63 - 1, 2 ** 63 - 1, -2 ** 63)
    counts = np.array([7, -2, max_det], np.int32)
    sizes = [(48, 80), (90, 40), (37, 53)]
    return dets, counts, sizes, max_det


def test_correct_detections_on_device_buffers_and_host():
    import torch
    dev = torch.device("cuda", 0)
    dets, counts, sizes, max_det = _crafted()
    net = (64, 64)
    want = LB.correct_dets(dets, counts, sizes, net)
    assert want[1].tobytes() == dets[1].tobytes() and want[0, 7:].tobytes() == dets[0, 7:].tobytes()
    assert want[0, 0].tolist()[2:] == (0, 0, 79, 47) and want[0, :7].tobytes() != dets[0, :7].tobytes()
    d = torch.from_numpy(dets.view(np.uint8).reshape(3, max_det, 40).copy()).to(dev)
    c = torch.from_numpy(counts).to(dev)
    dnn_hip._check(lib.dnn_yolo_correct_detections(d.data_ptr(), c.data_ptr(), 3, max_det, yolo_post._sizes(sizes),
                                                   net[0], net[1], torch.cuda.current_stream(dev).cuda_stream),
                   "dnn_yolo_correct_detections")
    got = d.cpu().numpy().view(yolo_post.DETECTION_DTYPE).reshape(3, max_det)
    assert got.tobytes() == want.tobytes()
    assert np.array_equal(c.cpu().numpy(), counts)
    host = dets.copy()
    assert yolo_post.correct_rows_host(host, counts, sizes, net) is host
    assert host.tobytes() == want.tobytes()
    # the buffers' method: the same call on self.dets / self.counts
    head = yolo_post.MultiHead.yolov3_tiny(64, 64, classes=3)
    bufs = yolo_post.MultiDetectionBuffers(3, dev, head, max_det=max_det)
    bufs.dets.copy_(torch.from_numpy(dets.view(np.uint8).reshape(3, max_det, 40).copy()))
    bufs.counts.copy_(torch.from_numpy(counts))
    bufs.correct(sizes, net, 3, torch.cuda.current_stream(dev).cuda_stream)
    assert bufs.dets.cpu().numpy().tobytes() == want.tobytes()
    with pytest.raises(ValueError):
        bufs.correct(sizes[:2], net, 3, None)


# ------------------------------------------------------------------ 4. RaggedIngest
SUBMITS = [[(37, 53), (5, 7), (100, 37)], [(48, 64)], [(16, 8), (33, 17), (3, 2), (64, 64)], [],
           [(100, 37), (100, 37)], [(5, 7), (48, 64), (37, 53)]]
NET = (64, 96)


def _set(hws, seed):
    pairs = [oracle(hw + NET, "rgb", seed) for hw in hws]
    return [p[0] for p in pairs], [p[1] for p in pairs]


@pytest.mark.parametrize("use_side", [False, True], ids=["compute", "side+release"])
def test_ragged_ingest_six_submits_through_two_slots(use_side):
    """Six submits of varying image sets; each batch is read by a late reader (a matmul chain
    first, so the copy stream runs ahead) on the compute stream with no release(), or on a side
    stream recorded with release(side).  Every batch equals the oracle of its own images: slot
    reuse corrupts nothing that is still being read."""
    import torch
    dev = torch.device("cuda", 0)
    busy = torch.randn(1024, 1024, device=dev)
    ri = ingest.RaggedIngest(4, 3 * 100 * 37 * 3, NET, dev, order="rgb")
    side = torch.cuda.Stream(dev)
    outs, wants = [], []
    for k, hws in enumerate(SUBMITS):
        ims, want = _set(hws, k % 2)
        x, sizes = ri.submit(ims)
        assert sizes == hws and tuple(x.shape) == (len(hws),) + NET + (3,)
        reader = side if use_side else ri.compute
        reader.wait_stream(ri.compute)
        with torch.cuda.stream(reader):
            y = busy
            for _ in range(6):
                y = y @ busy  # keeps the reader late
            outs.append(x.clone())  # the dependent kernel
        if use_side:
            ri.release(side)
        wants.append(want)
    torch.cuda.synchronize()
    for k, (o, want) in enumerate(zip(outs, wants)):
        o = o.cpu().numpy()
        for i, w in enumerate(want):
            assert np.array_equal(o[i], w), f"submit {k} image {i}"


def test_ragged_ingest_rejected_submit_changes_nothing():
    import torch
    dev = torch.device("cuda", 0)
    ri = ingest.RaggedIngest(2, 3 * 64 * 64 * 2, NET, dev)
    ims, want = _set([(48, 64), (5, 7)], 0)
    slot = ri.slot
    for bad in ([ims[0]] * 3, [ims[0].astype(np.float32)], [LC.image(100, 100), LC.image(100, 100)],
                [LC.image(100, 2)]):
        with pytest.raises(ValueError):
            ri.submit(bad)
        assert ri.slot == slot and ri.last is None and ri.uploaded == [None, None]
    x, _ = ri.submit(ims)
    torch.cuda.synchronize()
    bgr = [LB.letterbox_f32(im, NET[0], NET[1], "bgr") for im in ims]
    assert all(np.array_equal(x[i].cpu().numpy(), bgr[i]) for i in range(2))


# ------------------------------------------------------------------ 5. end to end
E2E_SIZES, E2E_THR = [(48, 80), (90, 40)], 0.05


def test_detect_images_equals_detect_on_the_oracle_frames_corrected(tmp_path):
    """The narrow YOLOv3-tiny (width_div 4, 64 x 64, 3 classes), B = 2, score threshold 0.05:
    detect_images(images) == correct_rows(detect(letterbox_f32 frames)) row for row, scores
    included: the plan and the decode are the same device code on bit-identical inputs.  The
    float64 Darknet oracle with the numpy multi-label decode gives 88 + 95 rows for these inputs
    (checked below), so the comparison is not of empty lists."""
    cfg = DC.narrow_cfg("yolov3-tiny")
    secs = D.parse_cfg(cfg)
    m = D.DarknetModel(cfg, DC.darknet_layers(secs), in_shape=[2, 64, 64, 3], score_thr=E2E_THR)
    images = [LC.image(h, w, 0) for h, w in E2E_SIZES]
    x = np.stack([LB.letterbox_f32(im, 64, 64) for im in images])
    outs = DO.forward(secs, m.layers, x)
    multi = MO.Multi(tuple(m.head.scales), "logistic")
    cpu_rows = [LO.detect_or_code([np.asarray(o[i], np.float32) for o in outs], multi) for i in range(2)]
    assert all(not isinstance(r, int) for r in cpu_rows) and sum(len(r) for r in cpu_rows) >= 8

    plain = m.detect(x)
    want = LB.correct_rows(plain, E2E_SIZES, (64, 64))
    got = m.detect_images(images)
    n_rows = sum(len(r) for r in want)
    changed = sum(a != b for p, w in zip(plain, want) for a, b in zip(p, w))
    print(f"detect_images: rows {[len(r) for r in got]}, {changed} of {n_rows} changed by the correction")
    assert n_rows >= 4 and changed >= 1
    assert got == want
    for rows, (h, w) in zip(got, E2E_SIZES):
        assert all(0 <= l <= r <= w - 1 and 0 <= t <= b <= h - 1 for _, l, t, r, b, _ in rows)
    # a second call (the other slot), fewer images, RGB order: the oracle frames again
    x1 = LB.letterbox_f32(images[1], 64, 64, "rgb")[None]
    assert m.detect_images(images[1:], order="rgb") == LB.correct_rows(m.detect(x1), E2E_SIZES[1:], (64, 64))
