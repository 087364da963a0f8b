"""GPU: the grid-wide multi-scale decode (dnn_yolo_postprocess_wide, csrc/postprocess_wide.hip;
yolo_post.WideHead) in its three modes: byte for byte against the existing entries below their
16,384-box cap, against the existing oracles above it, the candidate cap and the per-image
counters, the 65,536-box limit, repeated calls and graph replay, and an imported Darknet model with
17,340 boxes end to end.  Every device call runs on poisoned buffers between guard bands."""
import ctypes

import numpy as np
import pytest

import dnn_hip
import plan_fuzz_checks as C
import post_head_cases as HK
import post_multi_cases as K
import post_multi_oracle as MO
import post_multilabel_cases as LK
import post_multilabel_oracle as LO
import post_wide_cases as W
import yolo_post

pytestmark = pytest.mark.gpu

MODES = sorted(W.MODES)


def _guarded(torch, dev, nbytes):
    t = torch.full((2 * C.GUARD_BYTES + nbytes,), C.POISON, dtype=torch.uint8, device=dev)
    return t, t[C.GUARD_BYTES:C.GUARD_BYTES + nbytes]


def _old_entry(head):
    """The existing device entry of a MultiHead's mode, as (function, trailing mode argument)."""
    if head.labels == "multi":
        return dnn_hip.mylib.dnn_yolo_postprocess_multi_labels, (1,)
    return dnn_hip.mylib.dnn_yolo_postprocess_multi_nms, (yolo_post.NMS_MODES[head.nms],)


def _run_guarded(head, preds, max_det=None, calls=1):
    """The device entry of `head` (the wide one for a WideHead) on poisoned dets / counts / workspace
    between guard bands, `calls` times on the same buffers without clearing them: (counts as a
    list, dets as uint8 [n, max_det, 40]) after the last call; the guards are checked."""
    import torch
    dev = torch.device("cuda", 0)
    n = preds[0].shape[0]
    max_det = head.max_det if max_det is None else max_det
    n_ws = head.workspace_bytes(n)
    stream = torch.cuda.current_stream(dev).cuda_stream
    xs = [torch.from_numpy(np.array(p)).to(dev) for p in preds]
    ptrs = (ctypes.c_void_p * len(xs))(*[x.data_ptr() for x in xs])
    dets_all, dets = _guarded(torch, dev, n * max_det * 40)
    counts_all, counts = _guarded(torch, dev, n * 4)
    ws_all, ws = _guarded(torch, dev, n_ws)
    if isinstance(head, yolo_post.WideHead):
        assert n_ws == n * (head.boxes * 40 + 16384 * 8 + 64)
        entry = dnn_hip.mylib.dnn_yolo_postprocess_wide
        tail = (yolo_post.NMS_MODES[head.nms], yolo_post.LABEL_MODES[head.labels])
    else:
        entry, tail = _old_entry(head)
    for _ in range(calls):
        rc = entry(ctypes.byref(head.c), ptrs, n, dets.data_ptr(), max_det, counts.data_ptr(), ws.data_ptr(), n_ws,
                   *tail, stream)
        assert rc == 0, dnn_hip.last_error()
    torch.cuda.synchronize()
    for buf, what in ((dets_all, "dets"), (counts_all, "counts"), (ws_all, "workspace")):
        C.check_guard(buf.cpu().numpy(), what)
    return [int(c) for c in counts.cpu().numpy().view(np.int32)], dets.cpu().numpy().reshape(n, max_det, 40)


def _check_images(counts, dets, want, what):
    """counts are the oracle's numbers or codes, the rows the oracle's, and nothing is written after
    them or beside a code."""
    assert counts == W.counts_of(want), what
    for i, w in enumerate(want):
        if isinstance(w, int):
            assert (dets[i] == C.POISON).all(), f"{what} image {i}: rows written beside the code {w}"
            continue
        k = len(w)
        rows = yolo_post.DetectionBuffers.to_rows(dets[i:i + 1, :k], [k], max_det=k)[0]
        HK.same_rows(rows, list(w), f"{what} image {i}")
        assert (dets[i, k:] == C.POISON).all(), f"{what} image {i}: rows written after the count"


# ------------------------------------------------------------------ 1. below the old cap: the same bytes
def _below_cap_inputs():
    small = K.yolov3_multi(*K.PARITY["small"][:2], score_thr=K.PARITY["small"][4])
    yolov3 = K.yolov3_multi(*K.PARITY["yolov3"][:2], score_thr=K.PARITY["yolov3"][4])
    labels = LK.seeded_multi("small")  # its boxes carry second labels (252 rows of 252 boxes and more)
    softmax = LK.seeded_multi("small_softmax")
    return {"small": (small, MO.batch(K.PARITY["small"][3], small, K.PARITY["small"][2])),
            "yolov3": (yolov3, MO.batch(K.PARITY["yolov3"][3], yolov3, K.PARITY["yolov3"][2])),
            "second_labels": (labels, MO.batch(LK.SEEDED["small"][3], labels, LK.SEEDED["small"][2])),
            "softmax": (softmax, MO.batch(LK.SEEDED["small_softmax"][3], softmax, LK.SEEDED["small_softmax"][2]))}


@pytest.mark.parametrize("name", ["small", "yolov3", "second_labels", "softmax"])
def test_same_bytes_as_the_existing_entries_below_their_cap(name):
    """Counts equal, negative codes included, and rows [0, count) byte for byte, in all three modes."""
    multi, preds = _below_cap_inputs()[name]
    seen = []
    for mode in MODES:
        wide = W.device_head(multi, mode)
        old = W.device_head(multi, mode, yolo_post.MultiHead)
        assert wide.boxes == old.boxes <= W.OLD_CAP and wide.max_det == old.max_det
        got, want = _run_guarded(wide, preds), _run_guarded(old, preds)
        print(f"{name} {mode}: wide {got[0]}, existing {want[0]}")
        assert got[0] == want[0], mode
        assert any(c > 0 for c in got[0]), mode
        seen += got[0]
        for i, c in enumerate(got[0]):
            if c > 0:
                assert got[1][i, :c].tobytes() == want[1][i, :c].tobytes(), f"{name} {mode} image {i}"
        if name == "second_labels" and mode == "multi":
            assert max(got[0]) > wide.boxes // 2  # more rows than the single-label modes can give
    assert any(c < 0 for c in seen)  # codes were compared too


@pytest.mark.parametrize("name", sorted(W.SMALL))
def test_small_cases_of_the_one_workgroup_entries_through_the_wide_entry(name):
    """The cases built for the one-workgroup kernels' segment scheduling and merges (post_wide_cases.
    SMALL) through the wide entry, whose index field is 16 bits wide: the oracle's rows and codes,
    and counts and rows [0, count) byte for byte those of the existing entry."""
    multi, preds, mode, want, _ = W.small(name)
    wide = W.device_head(multi, mode)
    old = W.device_head(multi, mode, yolo_post.MultiHead)
    assert wide.boxes == old.boxes <= W.OLD_CAP and wide.max_det == old.max_det
    got, ref = _run_guarded(wide, preds), _run_guarded(old, preds)
    print(f"{name} {mode}: wide {got[0]}, existing {ref[0]}, oracle {W.counts_of(want)}")
    _check_images(got[0], got[1], want, f"{name} {mode}")
    assert got[0] == ref[0] and any(c > 0 for c in got[0])
    for i, c in enumerate(got[0]):
        if c > 0:
            assert got[1][i, :c].tobytes() == ref[1][i, :c].tobytes(), f"{name} {mode} image {i}"


# ------------------------------------------------------------------ 2. above the old cap, against the oracles
@pytest.mark.parametrize("name", sorted(W.ABOVE))
def test_above_the_old_cap_against_the_oracles(name):
    preds, refs, high = W.above(name)
    multi = W.above_multi(name)
    assert W.above_ok(refs, high)
    for mode in MODES:
        head = W.device_head(multi, mode)
        assert head.boxes == W.boxes_of(multi) > W.OLD_CAP
        counts, dets = _run_guarded(head, preds, max_det=512)
        print(f"{name} {mode}: device {counts}, oracle {W.counts_of(refs[mode])}, rows of boxes >= 16384: {high[mode]}")
        _check_images(counts, dets, refs[mode], f"{name} {mode}")


def test_608_with_80_classes_against_the_oracles():
    preds, refs = W.coco608()
    multi = W.coco608_multi()
    for mode in MODES:
        head = W.device_head(multi, mode)
        assert head.boxes == 22743 and head.max_det == 16384
        counts, dets = _run_guarded(head, preds, max_det=1024)
        print(f"608 x 608 x 80 {mode}: device {counts}, oracle {W.counts_of(refs[mode])}")
        _check_images(counts, dets, refs[mode], f"608 x 608 x 80 {mode}")
    rows = yolo_post.detect_batch_multi(preds, W.device_head(multi, "multi"), raise_errors=False)
    HK.same_rows(rows[0], refs["multi"][0] if isinstance(refs["multi"][0], int) else list(refs["multi"][0]),
                 "detect_batch_multi")


# ------------------------------------------------------------------ 3. the candidate cap, the per-image counters
@pytest.mark.parametrize("mode", MODES)
def test_candidate_cap_and_per_image_counters(mode):
    """Exactly 16,384 candidates give the oracle's rows, 16,385 give -3; the batch [at the cap, over,
    clean, bad corner, empty] gets each image's own rows or code."""
    preds, refs = W.cap(mode)
    head = W.device_head(W.cap_multi(), mode)
    assert head.boxes == 17391 and head.max_det == 16384
    assert [r if isinstance(r, int) else "rows" for r in refs] == ["rows", -3, "rows", -1, "rows"] and refs[4] == []
    counts, dets = _run_guarded(head, preds, max_det=64)
    print(f"cap {mode}: device {counts}, oracle {W.counts_of(refs)}")
    _check_images(counts, dets, refs, f"cap {mode}")
    with pytest.raises(dnn_hip.DnnHipError, match="16384"):
        yolo_post.detect_batch_multi([p[1:2] for p in preds], head)


# ------------------------------------------------------------------ 4. the wide limit
def test_65536_boxes_with_the_last_box_a_candidate():
    preds, refs = W.edge()
    multi = W.edge_multi()
    assert not isinstance(refs[0], int) and len(refs[0]) >= 3
    for mode in MODES:  # one class: every mode is the class-agnostic function
        head = W.device_head(multi, mode)
        assert head.boxes == yolo_post.WIDE_MAX_BOXES == 65536
        counts, dets = _run_guarded(head, preds, max_det=16)
        _check_images(counts, dets, refs, f"65536 boxes {mode}")


# ------------------------------------------------------------------ 5. repeat and replay
def test_a_second_call_on_the_same_buffers_gives_the_same_bytes():
    """The counters are cleared by the call itself: two calls without clearing anything between
    them leave what one call leaves."""
    preds, refs, _ = W.above("four")
    for mode in MODES:
        head = W.device_head(W.above_multi("four"), mode)
        once, twice = _run_guarded(head, preds, max_det=512), _run_guarded(head, preds, max_det=512, calls=2)
        assert once[0] == twice[0] == W.counts_of(refs[mode]), mode
        assert once[1].tobytes() == twice[1].tobytes(), mode


def test_graph_replay_equals_the_eager_run_on_a_second_input():
    import torch
    dev = torch.device("cuda", 0)
    multi = W.above_multi("four")
    first, second = W.above_preds("four"), W.above_preds("four", seed=W.ABOVE["four"][3] + 100)
    n = first[0].shape[0]
    head = W.device_head(multi, "multi")
    xs = [torch.from_numpy(np.array(p)).to(dev) for p in first]
    bufs = yolo_post.MultiDetectionBuffers(n, dev, head, max_det=512)

    def state():
        torch.cuda.synchronize()
        return bufs.counts.cpu().numpy().copy(), bufs.dets.cpu().numpy().copy()

    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        bufs.run([x.data_ptr() for x in xs], n, side.cuda_stream)
    eager_first = state()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        bufs.run([x.data_ptr() for x in xs], n, torch.cuda.current_stream(dev).cuda_stream)
    for x, p in zip(xs, second):
        x.copy_(torch.from_numpy(np.array(p)))
    with torch.cuda.stream(side):
        bufs.run([x.data_ptr() for x in xs], n, side.cuda_stream)
    eager_second = state()
    assert not np.array_equal(eager_first[0], eager_second[0]) or not np.array_equal(eager_first[1], eager_second[1])
    bufs.dets.fill_(C.POISON)
    bufs.counts.fill_(-7)
    graph.replay()
    replayed = state()
    assert replayed[0].tolist() == eager_second[0].tolist()
    for i, c in enumerate(replayed[0]):
        if c > 0:
            assert replayed[1][i, :c].tobytes() == eager_second[1][i, :c].tobytes(), f"image {i}"


# ------------------------------------------------------------------ 6. end to end
def test_imported_model_with_17340_boxes_detects_with_wide():
    """The narrow YOLOv3-tiny at 1088 x 1088 of test_gpu_darknet (head=None by default) built with
    wide=True: detect gives the multi-label oracle's rows on the device's own outputs."""
    import darknet_import as D
    import letterbox_cases as LC
    import letterbox_oracle as LB
    cfg, _, layers, x = W.e2e_model()
    for thr in (0.5, W.E2E_LOW_THR):
        m = D.DarknetModel(cfg, layers, wide=True, score_thr=thr)
        assert isinstance(m.head, yolo_post.WideHead) and m.head.boxes == 17340
        outs = [o.copy() for o in m.inference(x)]
        multi = MO.Multi(tuple(m.head.scales), "logistic")
        want = LO.detect_or_code([o[0] for o in outs], multi)
        rows = m.detect(x, raise_errors=False)
        print(f"1088 x 1088 narrow YOLOv3-tiny, score > {thr}: {W.counts_of([want])} rows")
        HK.same_rows(rows[0], want, f"detect at {thr}")
        assert isinstance(want, int) or m.postprocessing(outs) == yolo_post.label_boxes(rows[0], m.head)
    assert not isinstance(want, int) and len(want) >= 1
    # detect_images: two images of different sizes against detect on their letterboxed frames
    m = D.DarknetModel(cfg, layers, in_shape=[2, 1088, 1088, 3], wide=True, score_thr=W.E2E_LOW_THR)
    sizes = [(480, 800), (900, 400)]
    images = [LC.image(h, w, 0) for h, w in sizes]
    frames = np.stack([LB.letterbox_f32(im, 1088, 1088) for im in images])
    plain = m.detect(frames, raise_errors=False)
    dets = np.zeros((2, m.head.max_det), yolo_post.DETECTION_DTYPE)
    counts = np.zeros(2, np.int32)
    for i, rows in enumerate(plain):
        counts[i] = rows if isinstance(rows, int) else len(rows)
        for k, r in enumerate([] if isinstance(rows, int) else rows):
            dets[i, k] = (r[0], np.float32(r[5]), r[1], r[2], r[3], r[4])
    yolo_post.correct_rows_host(dets, counts, sizes, (1088, 1088))
    want = yolo_post.DetectionBuffers.to_rows(dets.view(np.uint8).reshape(2, -1, 40), counts, m.head.max_det,
                                              raise_errors=False)
    got = m.detect_images(images, raise_errors=False)
    assert got == want and any(not isinstance(r, int) and len(r) for r in got)
