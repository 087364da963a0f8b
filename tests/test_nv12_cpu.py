"""NV12 letterbox ingest without a GPU: the conversion oracle on values worked by hand, every
refusal of the C entries (all return before any device call) and of the Python wrappers, and the
exports of both libraries."""
import ctypes

import numpy as np
import pytest

import darknet_cases as DC
import darknet_import as D
import dnn_hip
import ingest
import nv12_oracle as NV

lib = dnn_hip.mylib


def _one(y, u, v, matrix):
    return NV.nv12_to_rgb(np.array([[y]], np.uint8), np.array([[[u, v]]], np.uint8), matrix)[0, 0].tolist()


@pytest.mark.parametrize("matrix", sorted(NV.MATRICES))
def test_oracle_on_values_worked_by_hand(matrix):
    for y in (0, 16, 100, 235, 255):  # grey: U = V = 128 gives R = G = B
        r, g, b = _one(y, 128, 128, matrix)
        assert r == g == b
    if matrix.endswith("limited"):
        assert _one(16, 128, 128, matrix) == [0, 0, 0] and _one(235, 128, 128, matrix) == [255, 255, 255]
        assert _one(0, 128, 128, matrix) == [0, 0, 0] and _one(255, 128, 128, matrix) == [255, 255, 255]  # clipped
        assert _one(126, 128, 128, matrix) == [128] * 3  # (298 * 110 + 128) >> 8
    else:
        assert [_one(y, 128, 128, matrix)[0] for y in (0, 1, 200, 255)] == [0, 1, 200, 255]
    rv, bu = NV.MATRICES[matrix][2], NV.MATRICES[matrix][5]
    assert _one(255, 255, 255, matrix)[::2] == [255, 255] and _one(0, 0, 0, matrix)[::2] == [0, 0]  # both ends
    y0, cy = NV.MATRICES[matrix][:2]
    assert _one(100, 128, 138, matrix)[0] == (cy * (100 - y0) + rv * 10 + 128) >> 8
    assert _one(100, 118, 128, matrix)[2] == (cy * (100 - y0) - bu * 10 + 128) >> 8


def test_oracle_takes_the_chroma_of_the_2x2_block_and_the_lone_last_column():
    y = np.full((3, 3), 126, np.uint8)
    uv = np.array([[[128, 128], [128, 255]], [[0, 128], [128, 128]]], np.uint8)
    rgb = NV.nv12_to_rgb(y, uv)
    assert rgb[0, 0].tolist() == rgb[1, 1].tolist() == rgb[2, 2].tolist() == [128] * 3
    assert rgb[0, 2].tolist() == rgb[1, 2].tolist() != [128] * 3 and rgb[0, 2, 0] == 255
    assert rgb[2, 0].tolist() == rgb[2, 1].tolist() and rgb[2, 0, 2] == 0
    buf, desc = NV.surface(y, uv, pitch=7, gap_rows=2, offset=3)
    assert desc == (3, 3 + 5 * 7, 3, 3, 7) and buf.size == 38 + 14 and buf[38:42].tolist() == [128, 128, 128, 255]


def _frames(*items):
    arr = (ingest.FrameNV12 * len(items))()
    for k, it in enumerate(items):
        arr[k] = ingest.FrameNV12(*it)
    return arr


@pytest.mark.parametrize("name,tail", [("dnn_letterbox_frames_nv12", (None,)), ("dnn_letterbox_frames_nv12_host", ())])
def test_nv12_entries_refuse_bad_arguments(name, tail):
    fn = getattr(lib, name)
    px = np.zeros(1000, np.uint8)
    out = np.zeros((2, 32, 32, 3), np.float32)
    ok = _frames((0, 64, 8, 8, 8), (96, 300, 10, 9, 20))  # frame 1: Y 9 * 20 + 9 bytes, UV 4 * 20 + 10 at 300

    def call(pixels=px.ctypes.data, nbytes=1000, frames=ok, n=2, dst=out.ctypes.data, net_h=32, net_w=32, matrix=0):
        return fn(pixels, nbytes, frames, n, dst, net_h, net_w, matrix, *tail)

    cases = [
        (dict(pixels=None), "NULL"), (dict(frames=None), "NULL"), (dict(dst=None), "NULL"),
        (dict(n=-1), "n = -1"),
        (dict(net_h=0), "network input 0 x 32"), (dict(net_w=-4), "network input 32 x -4"),
        (dict(net_h=50000, net_w=50000), "2^31 floats"),
        (dict(matrix=3), "matrix 3"), (dict(matrix=-1), "matrix -1"), (dict(matrix=0x300), "matrix 768"),
        (dict(frames=_frames((0, 64, 8, 8, 8), (96, 300, 0, 9, 20))), "frame 1 has size 0 x 9"),
        (dict(frames=_frames((0, 64, 8, -8, 8), (96, 300, 10, 9, 20))), "frame 0 has size 8 x -8"),
        (dict(frames=_frames((0, 64, 8, 8, 8), (96, 300, 10, 9, 9))), "frame 1 (10 x 9) has pitch 9, below the 10"),
        (dict(frames=_frames((0, 64, 8, 8, 7), (96, 300, 10, 9, 20))), "frame 0 (8 x 8) has pitch 7"),
        (dict(frames=_frames((0, 64, 8, 8, 8), (812, 300, 10, 9, 20))), "frame 1 (10 x 9, pitch 20): the Y plane at "
                                                                          "byte 812 ends past the 1000"),
        (dict(frames=_frames((0, 64, 8, 8, 8), (96, 911, 10, 9, 20))), "frame 1 (10 x 9, pitch 20): the UV plane at "
                                                                         "byte 911 ends past the 1000"),
        (dict(frames=_frames((2 ** 64 - 8, 64, 8, 8, 8), (96, 300, 10, 9, 20))), "frame 0"),
        (dict(frames=_frames((0, 2 ** 64 - 1, 8, 8, 8), (96, 300, 10, 9, 20))), "frame 0"),
        (dict(frames=_frames((0, 64, 8, 8, 8), (0, 500, 100, 3, 4))), "frame 1 (100 x 3)"),
        (dict(frames=_frames((0, 500, 3, 100, 100), (96, 300, 10, 9, 20))), "frame 0 (3 x 100)"),
        # the staged form forced on a 9-fold reduction: a tile samples more than the LDS buffer holds
        (dict(frames=_frames((0, 0, 300, 300, 300)), n=1, nbytes=10 ** 6, matrix=0x200), "frame 0 (300 x 300): "
                                                                                       "DNN_NV12_FORCE_STAGED"),
    ]
    for kw, text in cases:
        assert call(**kw) != 0, kw
        err = dnn_hip.last_error()
        assert name in err and text in err, (kw, err)
    assert out.tobytes() == bytes(out.nbytes)  # nothing ran
    assert call(pixels=None, frames=None, dst=None, n=0) == 0


def test_python_wrappers_refuse_before_any_device_work():
    y, uv = NV.frame(20, 31)
    layout = lambda frames, **kw: ingest.nv12_layout(frames, 4, 1 << 20, (32, 32), **kw)  # noqa: E731
    for bad in ([(y, uv[:, :15])], [(y.astype(np.int32), uv)], [y], [(y, uv), (y[None], uv)]):
        with pytest.raises(ValueError, match=f"frame {len(bad) - 1}"):
            layout(bad)
    with pytest.raises(ValueError, match="5 frames > batch 4"):
        layout([(y, uv)] * 5)
    with pytest.raises(ValueError, match="max_bytes"):
        ingest.nv12_layout([(y, uv)], 4, 959, (32, 32))
    with pytest.raises(ValueError, match="frame 0.*below 2 pixels"):
        ingest.nv12_layout([NV.frame(100, 3)], 4, 1 << 20, (64, 64))
    copies, frames, sizes, nbytes = layout([(y, uv), NV.frame(7, 5, 1)])
    assert sizes == [(20, 31), (7, 5)] and nbytes == 30 * 32 + 11 * 6  # 1.5 bytes a pixel, widths rounded to even
    assert [(f.y_offset, f.uv_offset, f.h, f.w, f.pitch) for f in frames[:2]] == [(0, 640, 20, 31, 32),
                                                                                 (960, 1002, 7, 5, 6)]
    assert [at for at, _ in copies] == [0, 640, 960, 1002]
    buf, desc = NV.surface(y, uv, pitch=40, gap_rows=3, offset=5)
    _, frames, sizes, nbytes = layout(buf, descriptors=[desc])
    assert sizes == [(20, 31)] and nbytes == buf.size and frames[0].uv_offset == 5 + 23 * 40
    for bad in ((5, desc[1], 20, 31, 30), (5, buf.size - 100, 20, 31, 40), (-1, desc[1], 20, 31, 40)):
        with pytest.raises(ValueError, match="frame 0"):
            layout(buf, descriptors=[bad])
    for kw in (dict(pixel_format="yuy2"), dict(pixel_format="nv12", matrix="bt2020")):
        with pytest.raises(ValueError, match="pixel_format|matrix"):
            ingest.RaggedIngest(2, 1000, (32, 32), **kw)  # (raises before any allocation)
    cfg = DC.narrow_cfg("yolov3-tiny")
    m = D.DarknetModel(cfg, DC.darknet_layers(D.parse_cfg(cfg)), in_shape=[2, 64, 64, 3])
    for bad, text in (([(y, uv)] * 3, "3 frames > batch 2"), ([(y, uv[1:])], "frame 0"), ([NV.frame(100, 2)], "below 2")):
        with pytest.raises(ValueError, match=text):
            m.detect_frames_nv12(bad)
    with pytest.raises(ValueError, match="matrix"):
        m.detect_frames_nv12([(y, uv)], matrix="rgb")
    assert m._dev is None and m._ingest == {}


def test_both_libraries_export_the_nv12_entries():
    import os
    from conftest import PKG
    for so in ("libdnn_hip.so", "libdnn_hip_avx.so"):
        other = ctypes.CDLL(os.path.join(PKG, so))
        for s in ("dnn_letterbox_frames_nv12", "dnn_letterbox_frames_nv12_host"):
            assert hasattr(other, s), f"{so} does not export {s}"
    assert ctypes.sizeof(ingest.FrameNV12) == 32
