"""Letterbox ingest and box correction without a GPU: the size rule against the table, the numpy
oracle against itself, the box mapping's edge cases, and every refusal of the new C entries and
Python wrappers (all return before any device call)."""
import ctypes

import numpy as np
import pytest

import darknet_cases as DC
import darknet_import as D
import dnn_hip
import ingest
import letterbox_cases as LC
import letterbox_oracle as LB
import yolo_post

lib = dnn_hip.mylib


# ------------------------------------------------------------------------------------ geometry
@pytest.mark.parametrize("case", sorted(LC.GEOMETRY))
def test_geometry_matches_the_table_and_the_oracle(case):
    want = LC.GEOMETRY[case]
    assert LB.geometry(*case) == want
    got = ingest.letterbox_geometry(*case)
    assert tuple(got) == want and (got.new_h, got.new_w, got.pad_y, got.pad_x) == want


@pytest.mark.parametrize("case", LC.REFUSED)
def test_geometry_refuses_a_one_pixel_side(case):
    assert LB.geometry(*case) is None
    with pytest.raises(ValueError, match="below 2 pixels"):
        ingest.letterbox_geometry(*case)
    for bad in [(0, 5, 32, 32), (5, -1, 32, 32), (5, 5, 0, 32), (5, 5, 32, 0)]:
        with pytest.raises(ValueError):
            ingest.letterbox_geometry(*bad)
    out = [ctypes.c_int(7) for _ in range(4)]
    assert lib.dnn_letterbox_geometry(5, 7, 32, 32, None, *[ctypes.byref(o) for o in out[1:]]) != 0
    assert "NULL" in dnn_hip.last_error()


def test_geometry_on_a_sweep_of_sizes_equals_the_oracle():
    rng = np.random.default_rng(11)
    for _ in range(2000):
        case = tuple(int(v) for v in rng.integers(1, 700, 4))
        want = LB.geometry(*case)
        if want is None:
            with pytest.raises(ValueError):
                ingest.letterbox_geometry(*case)
        else:
            assert tuple(ingest.letterbox_geometry(*case)) == want, case


# ------------------------------------------------------------------- the oracle against itself
def test_identity_and_pad_are_exact():
    for order in ("bgr", "rgb"):
        im = LC.image(64, 64, 1)
        want = (im.astype(np.float64) / 255.0).astype(np.float32)
        want = want[:, :, ::-1] if order == "bgr" else want
        assert np.array_equal(LB.letterbox_f32(im, 64, 64, order), want)
        im = LC.image(48, 64, 2)
        got = LB.letterbox_f32(im, 64, 64, order)
        want = (im.astype(np.float64) / 255.0).astype(np.float32)
        want = want[:, :, ::-1] if order == "bgr" else want
        assert np.array_equal(got[8:56], want)  # scale 1: dx = dy = 0
        assert np.all(got[:8] == np.float32(0.5)) and np.all(got[56:] == np.float32(0.5))
    got = LB.letterbox_f32(LC.image(33, 17, 3), 32, 64)
    assert np.all(got[:, :24] == np.float32(0.5)) and np.all(got[:, 40:] == np.float32(0.5))
    assert got.dtype == np.float32 and not np.all(got[:, 24:40] == np.float32(0.5))


@pytest.mark.parametrize("case", LC.SMALL)
def test_f32_oracle_is_within_1e5_of_float64_outside_the_last_row(case):
    src_h, src_w, net_h, net_w = case
    new_h, new_w, pad_y, pad_x = LC.GEOMETRY[case]
    worst = 0.0
    for seed in range(3):
        im = LC.image(src_h, src_w, seed)
        a = LB.letterbox_f32(im, net_h, net_w).astype(np.float64)
        b = LB.letterbox_f64(im, net_h, net_w)
        keep = np.ones(net_h, bool)
        keep[pad_y + new_h - 1] = False  # the last resized row has Darknet's rule (its own test)
        worst = max(worst, float(np.abs(a - b)[keep].max()))
        assert a.min() >= 0.0 and a.max() <= 1.0
    print(f"letterbox {case}: f32 oracle vs float64, worst {worst:.2e}")
    assert worst < 1e-5


def test_last_row_rule_is_pinned_on_16_to_96_rows():
    """(float)95 * ((float)15 / (float)95) rounds below 15: iy = 14, dy = 0.99999905, and the
    second term is skipped, so row 95 is (1 - dy) * part(14): nearly black."""
    scale = np.float32(15) / np.float32(95)
    sy = np.float32(95) * scale
    assert int(sy) == 14 and abs(float(sy - np.float32(14)) - 0.99999905) < 1e-7
    im = np.full((16, 8, 3), 200, np.uint8)
    got = LB.letterbox_f32(im, 96, 96)[:, 24:72]
    assert got[95].max() < 1e-5
    assert got[94].min() > 0.78  # 200 / 255
    assert abs(LB.letterbox_f64(im, 96, 96)[95, 24:72] - 200 / 255).max() < 1e-5  # what the rule loses


# ------------------------------------------------------------------------------- correct_rows
NET = (64, 64)


def test_correct_rows_by_hand():
    # 48 x 80 into 64 x 64: new 38 x 64 at pad_y 13; x' = x * 80 // 64, y' = (y - 13) * 48 // 38
    assert LB.geometry(48, 80, 64, 64) == (38, 64, 13, 0)
    rows = [[(2, 10, 20, 30, 40, 0.5)]]
    assert LB.correct_rows(rows, [(48, 80)], NET) == [[(2, 12, 8, 37, 34, 0.5)]]
    # corners of +-2^62 clamp without overflow; right / bottom never exceed src - 1
    wild = [[(0, -2 ** 62, -2 ** 62, 2 ** 62, 2 ** 62, 0.25)]]
    assert LB.correct_rows(wild, [(48, 80)], NET) == [[(0, 0, 0, 79, 47, 0.25)]]
    # wholly in the top pad: zero height at the border; wholly in the bottom pad likewise
    assert LB.correct_rows([[(1, 5, 0, 9, 12, 0.5)]], [(48, 80)], NET) == [[(1, 6, 0, 11, 0, 0.5)]]
    assert LB.correct_rows([[(1, 5, 52, 9, 63, 0.5)]], [(48, 80)], NET) == [[(1, 6, 47, 11, 47, 0.5)]]
    # error codes pass through
    assert LB.correct_rows([-1, [], -3], [(48, 80)] * 3, NET) == [-1, [], -3]


def test_correct_dets_leaves_error_images_and_rows_past_the_count_alone():
    rng = np.random.default_rng(5)
    dets = np.zeros((4, 6), yolo_post.DETECTION_DTYPE)
    for f in ("left", "top", "right", "bottom"):
        dets[f] = rng.integers(-100, 200, dets.shape)
    dets["cls"], dets["score"] = rng.integers(0, 3, dets.shape), rng.random(dets.shape)
    counts = np.array([-1, 3, -2, -3], np.int32)
    sizes = [(48, 80), (90, 40), (30, 30), (7, 9)]
    out = LB.correct_dets(dets, counts, sizes, NET)
    for i in (0, 2, 3):
        assert out[i].tobytes() == dets[i].tobytes()
    assert out[1, 3:].tobytes() == dets[1, 3:].tobytes() and out[1, :3].tobytes() != dets[1, :3].tobytes()
    assert np.array_equal(out["cls"], dets["cls"]) and np.array_equal(out["score"], dets["score"])
    assert out[1, :3]["right"].max() <= 39 and out[1, :3]["bottom"].max() <= 89
    assert min(out[1, :3][f].min() for f in ("left", "top", "right", "bottom")) >= 0
    # a count above max_det is clamped
    out = LB.correct_dets(dets, np.array([9, 0, 0, 0], np.int32), sizes, NET)
    assert out[0]["right"].max() <= 79 and out[1:].tobytes() == dets[1:].tobytes()


# ---------------------------------------------------------------- ABI refusals without a GPU
def _frames(*items):
    arr = (ingest.Frame * len(items))()
    for k, it in enumerate(items):
        arr[k] = ingest.Frame(*it)
    return arr


LETTERBOX_ENTRIES = [("dnn_letterbox_frames", (None,)), ("dnn_letterbox_frames_host", ())]


@pytest.mark.parametrize("name,tail", LETTERBOX_ENTRIES)
def test_letterbox_entries_refuse_bad_arguments(name, tail):
    fn = getattr(lib, name)
    px = np.zeros(1000, np.uint8)
    out = np.zeros((2, 32, 32, 3), np.float32)
    p, o = px.ctypes.data, out.ctypes.data
    ok = _frames((0, 8, 8), (192, 10, 10))

    def call(pixels=p, nbytes=1000, frames=ok, n=2, dst=o, net_h=32, net_w=32, order=0):
        return fn(pixels, nbytes, frames, n, dst, net_h, net_w, order, *tail)

    cases = [
        (dict(pixels=None), "NULL"), (dict(frames=None), "NULL"), (dict(dst=None), "NULL"),
        (dict(n=-1), "n = -1"),
        (dict(net_h=0), "network input 0 x 32"), (dict(net_w=-4), "network input 32 x -4"),
        (dict(net_h=50000, net_w=50000), "2^31 floats"),  # the kernel indexes a frame's floats in 32 bits
        (dict(order=2), "order 2"), (dict(order=-1), "order -1"),
        (dict(frames=_frames((0, 8, 8), (192, 0, 10))), "frame 1 has size 0 x 10"),
        (dict(frames=_frames((0, 8, -8), (192, 10, 10))), "frame 0 has size 8 x -8"),
        (dict(frames=_frames((0, 8, 8), (701, 10, 10))), "frame 1 (10 x 10 at byte 701) ends past the 1000"),
        (dict(frames=_frames((2 ** 64 - 8, 8, 8), (192, 10, 10))), "frame 0"),
        (dict(frames=_frames((0, 8, 8), (0, 100, 3))), "frame 1 (100 x 3)"),
        (dict(frames=_frames((0, 3, 100), (192, 10, 10))), "frame 0 (3 x 100)"),
    ]
    for kw, text in cases:
        assert call(**kw) != 0, kw
        err = dnn_hip.last_error()
        assert name in err and text in err, (kw, err)
    assert out.tobytes() == bytes(out.nbytes)  # nothing ran
    # n == 0 returns 0 whatever the pointers hold; a frame that ends exactly at pixels_bytes passes the check
    assert call(pixels=None, frames=None, dst=None, n=0) == 0


CORRECT_ENTRIES = [("dnn_yolo_correct_detections", (None,)), ("dnn_yolo_correct_detections_host", ())]


@pytest.mark.parametrize("name,tail", CORRECT_ENTRIES)
def test_correct_entries_refuse_bad_arguments(name, tail):
    fn = getattr(lib, name)
    dets = np.zeros((2, 4), yolo_post.DETECTION_DTYPE)
    dets["left"] = 77
    counts = np.array([4, 4], np.int32)
    before = dets.tobytes()

    def call(d=dets.ctypes.data, c=counts.ctypes.data, n=2, max_det=4, sizes=((48, 80), (90, 40)), net_h=64, net_w=64):
        return fn(d, c, n, max_det, yolo_post._sizes(sizes) if sizes is not None else None, net_h, net_w, *tail)

    cases = [
        (dict(d=None), "NULL"), (dict(c=None), "NULL"), (dict(sizes=None), "NULL"),
        (dict(n=-1), "n_images = -1"), (dict(max_det=-1), "max_det = -1"),
        (dict(net_h=0), "network input 0 x 64"), (dict(net_w=0), "network input 64 x 0"),
        (dict(sizes=((48, 80), (0, 40))), "image 1 has size 0 x 40"),
        (dict(sizes=((48, -2), (90, 40))), "image 0 has size 48 x -2"),
        (dict(sizes=((48, 80), (100, 3))), "image 1 (100 x 3)"),
    ]
    for kw, text in cases:
        assert call(**kw) != 0, kw
        err = dnn_hip.last_error()
        assert name in err and text in err, (kw, err)
    assert dets.tobytes() == before
    assert call(d=None, c=None, sizes=None, n=0) == 0
    assert call(d=None, max_det=0) == 0  # no rows: nothing to do, nothing launched


def test_python_wrappers_refuse_before_any_device_work():
    im = LC.image(20, 30)
    with pytest.raises(ValueError, match="uint8"):
        ingest.ragged_layout([im.astype(np.float32)], 4, 1 << 20, (32, 32))
    with pytest.raises(ValueError, match="image 1"):
        ingest.ragged_layout([im, im[:, :, 0]], 4, 1 << 20, (32, 32))
    with pytest.raises(ValueError, match="image 0"):
        ingest.ragged_layout([im[:, :, :2]], 4, 1 << 20, (32, 32))
    with pytest.raises(ValueError, match="5 images > batch 4"):
        ingest.ragged_layout([im] * 5, 4, 1 << 20, (32, 32))
    with pytest.raises(ValueError, match="max_bytes"):
        ingest.ragged_layout([im, im], 4, 3 * 20 * 30 * 2 - 1, (32, 32))
    with pytest.raises(ValueError, match="image 1.*below 2 pixels"):
        ingest.ragged_layout([im, LC.image(100, 3)], 4, 1 << 20, (64, 64))
    arrays, frames, sizes, nbytes = ingest.ragged_layout([im, LC.image(7, 5)], 4, 1 << 20, (32, 32))
    assert sizes == [(20, 30), (7, 5)] and nbytes == 1800 + 105
    assert [(f.offset, f.h, f.w) for f in frames[:2]] == [(0, 20, 30), (1800, 7, 5)]
    for bad in ("BGR", "gbr", 0, None):
        with pytest.raises(ValueError, match="order"):
            ingest.letterbox_gpu(im, (32, 32), order=bad)
    with pytest.raises(ValueError, match="uint8"):
        ingest.letterbox_gpu(im.astype(np.int32), (32, 32))
    with pytest.raises(ValueError, match="DETECTION_DTYPE"):
        yolo_post.correct_rows_host(np.zeros((2, 4, 40), np.uint8), [0, 0], [(8, 8)] * 2, (32, 32))
    with pytest.raises(ValueError, match="sizes"):
        yolo_post.correct_rows_host(np.zeros((2, 4), yolo_post.DETECTION_DTYPE), [0, 0], [(8, 8)], (32, 32))


def test_detect_images_refuses_before_any_device_work():
    cfg = DC.narrow_cfg("yolov3-tiny")
    m = D.DarknetModel(cfg, DC.darknet_layers(D.parse_cfg(cfg)), in_shape=[2, 64, 64, 3])
    im = LC.image(48, 80)
    with pytest.raises(ValueError, match="3 images > batch 2"):
        m.detect_images([im, im, im])
    with pytest.raises(ValueError, match="uint8"):
        m.detect_images([im.astype(np.float32)])
    with pytest.raises(ValueError, match="image 1"):
        m.detect_images([im, im[0]])
    with pytest.raises(ValueError, match="order"):
        m.detect_images([im], order="yuv")
    with pytest.raises(ValueError, match="below 2 pixels"):
        m.detect_images([LC.image(100, 2)])
    assert m._dev is None and m._ingest == {}
    # it needs a head, as detect does
    big = D.cfg_text("yolov3-tiny", classes=3, width=1088, height=1088, width_div=16)
    m = D.DarknetModel(big, DC.darknet_layers(D.parse_cfg(big)))
    with pytest.raises(ValueError, match="17340 boxes"):
        m.detect_images([im])


def test_both_libraries_export_the_new_entries_and_the_headers_declare_them():
    import os
    from conftest import PKG, REPO
    names = {"dnn_hip_ingest.h": ["dnn_letterbox_geometry", "dnn_letterbox_frames", "dnn_letterbox_frames_host"],
             "dnn_hip_post.h": ["dnn_yolo_correct_detections", "dnn_yolo_correct_detections_host"]}
    for header, syms in names.items():
        text = open(os.path.join(REPO, "include", header)).read()
        for so in ("libdnn_hip.so", "libdnn_hip_avx.so"):
            other = ctypes.CDLL(os.path.join(PKG, so))
            for s in syms:
                assert hasattr(other, s), f"{so} does not export {s}"
                assert f"int {s}(" in text
    assert ctypes.sizeof(ingest.Frame) == 16 and ctypes.sizeof(yolo_post.ImageSize) == 8
