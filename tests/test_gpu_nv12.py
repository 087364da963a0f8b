"""NV12 letterbox ingest on the MI355X: dnn_letterbox_frames_nv12 bit for bit against
letterbox_oracle(nv12_to_rgb(surface)), both forms of the kernel, a ragged batch past one launch's
64 frames, and DarknetModel.detect_frames_nv12 end to end.  Every comparison is exact."""
import numpy as np
import pytest

import darknet_cases as DC
import darknet_import as D
import ingest
import letterbox_oracle as LB
import nv12_oracle as NV

pytestmark = pytest.mark.gpu


def run(buf, descs, net, matrix="bt601_limited", form=None, prefill=float("nan")):
    """The device entry on one surface buffer: fp32 [n, net_h, net_w, 3] (numpy)."""
    import torch
    dev = torch.device("cuda", 0)
    frames = (ingest.FrameNV12 * len(descs))(*[ingest.FrameNV12(*d) for d in descs])
    src = torch.from_numpy(buf).to(dev)
    out = torch.full((len(descs),) + tuple(net) + (3,), prefill, dtype=torch.float32, device=dev)
    ingest.letterbox_nv12_device(src.data_ptr(), buf.size, frames, len(descs), out.data_ptr(),
                                 torch.cuda.current_stream(dev).cuda_stream, net, matrix, form)
    return out.cpu().numpy()


def want(y, uv, net, matrix="bt601_limited"):
    return LB.letterbox_f32(NV.nv12_to_rgb(y, uv, matrix), net[0], net[1], "rgb")


# (src_h, src_w, net_h, net_w, surface(...) arguments, forms): the smallest shapes where each thing can break
CASES = {
    "minimum": (2, 2, 32, 32, {}, (None,)),
    "odd sizes, lone chroma column": (5, 7, 32, 48, {}, (None,)),
    "last-row rule": (16, 16, 96, 96, {}, (None,)),
    "pitch, planes apart": (40, 24, 48, 32, dict(pitch=64, gap_rows=3), (None,)),
    "odd byte offset": (40, 24, 48, 32, dict(pitch=64, gap_rows=3, offset=1), (None, "gather")),
    "three tiles wide, side pads": (64, 200, 32, 160, {}, (None, "gather")),
    "reduction beyond the staged form": (300, 300, 32, 32, {}, (None,)),
    "both forms forced": (30, 30, 32, 32, {}, ("staged", "gather")),
    "one-float stores": (31, 19, 35, 33, {}, ("staged", "gather")),
}


@pytest.mark.parametrize("name", list(CASES))
def test_nv12_letterbox_is_bit_exact(name):
    h, w, net_h, net_w, kw, forms = CASES[name]
    y, uv = NV.frame(h, w)
    buf, desc = NV.surface(y, uv, **kw)
    ref = want(y, uv, (net_h, net_w))
    for form in forms:
        got = run(buf, [desc], (net_h, net_w), form=form)[0]
        bad = np.argwhere(got != ref)
        assert np.array_equal(got, ref), f"{name}, form {form}: {len(bad)} elements differ, first {bad[:3].tolist()}"


@pytest.mark.parametrize("matrix", sorted(NV.MATRICES))
def test_every_matrix_on_full_range_bytes(matrix):
    y, uv = NV.frame(37, 53, 1)
    rgb = NV.nv12_to_rgb(y, uv, matrix)
    assert (rgb == 0).any() and (rgb == 255).any()  # both clips are exercised
    buf, desc = NV.surface(y, uv)
    assert np.array_equal(run(buf, [desc], (64, 96), matrix)[0], want(y, uv, (64, 96), matrix))


def test_ragged_batch_of_66_frames_writes_every_element_once():
    """66 tiny frames of mixed sizes (two launches), a reduction that gathers (200 x 120: a tile
    samples 99 rows of 120 pixels) among frames that stage, into a NaN-filled output; a repeat into
    a buffer of another fill gives the same bytes."""
    sizes = [(5, 7), (40, 24), (200, 120), (16, 16), (2, 2), (33, 70)]
    pairs = [NV.frame(*sizes[k % len(sizes)], seed=k % 2) for k in range(66)]
    refs = {}
    bufs, descs, at = [], [], 3
    for k, (y, uv) in enumerate(pairs):
        buf, d = NV.surface(y, uv, pitch=2 * ((y.shape[1] + 1) // 2) + k % 3, gap_rows=k % 2)
        bufs.append(buf)
        descs.append((d[0] + at, d[1] + at) + d[2:])
        at += buf.size + 1
        refs.setdefault((y.shape, k % 2), want(y, uv, (32, 48)))
    whole = np.concatenate([np.full(3, 0xAB, np.uint8)] + [np.append(b, np.uint8(0xAB)) for b in bufs])
    got = run(whole, descs, (32, 48))
    assert not np.isnan(got).any()
    for k, (y, _) in enumerate(pairs):
        assert np.array_equal(got[k], refs[(y.shape, k % 2)]), f"frame {k}"
    assert run(whole, descs, (32, 48), prefill=7.0).tobytes() == got.tobytes()


def test_detect_frames_nv12_equals_detect_images_on_the_converted_frames():
    """The narrow YOLOv3-tiny of the letterbox tests (64 x 64, 3 classes, B = 2), two frames of
    different sizes: the same rows, scores included, as detect_images on nv12_to_rgb of the surfaces."""
    cfg = DC.narrow_cfg("yolov3-tiny")
    m = D.DarknetModel(cfg, DC.darknet_layers(D.parse_cfg(cfg)), in_shape=[2, 64, 64, 3], score_thr=0.05)
    frames = [NV.frame(48, 80), NV.frame(91, 41)]
    for matrix in ("bt601_limited", "bt709_limited"):
        rows = m.detect_images([NV.nv12_to_rgb(y, uv, matrix) for y, uv in frames], order="rgb")
        assert sum(len(r) for r in rows) >= 4  # not a comparison of empty lists
        assert m.detect_frames_nv12(frames, matrix=matrix) == rows
    # the other slot, one frame, given as a surface buffer with a descriptor
    buf, desc = NV.surface(*frames[1], pitch=48, gap_rows=1, offset=7)
    ing = m._ingest[("nv12", "bt601_limited")]
    x, sizes = ing.submit(buf, descriptors=[desc])
    assert sizes == [(91, 41)] and np.array_equal(x[0].cpu().numpy(), want(*frames[1], (64, 64)))
