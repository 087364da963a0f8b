"""GPU: the DFL head decode (dnn_yolo_postprocess_dfl, csrc/postprocess_dfl.hip; yolo_post.DflHead) against the
float64 oracle of tests/post_dfl_oracle.py on the decision-stable cases of tests/post_dfl_cases.py."""
import numpy as np
import pytest

import post_dfl_cases as K
import yolo_post

pytestmark = pytest.mark.gpu


def _same(rows, want, what):
    """Codes and counts equal; per row the class and the corners equal and the score within 4 ulp of fp32.
    The corners are integers: the device's fp32 corner is within K.CORNER_PX of the oracle's (derived at the
    top of post_dfl_cases.py) and no oracle corner of a case is that close to a whole pixel, so both truncate
    to the same integer; class, corners and order together are the (box index, class) sequence."""
    assert K.counts_of(rows) == K.counts_of(want), what
    for i, (got, ref) in enumerate(zip(rows, want)):
        if isinstance(ref, int):
            continue
        assert [g[:5] for g in got] == [r[:5] for r in ref], f"{what} image {i}"
        err = [abs(g[5] - r[5]) / np.spacing(np.float32(r[5])) for g, r in zip(got, ref)]
        print(f"{what} image {i}: {len(ref)} rows, largest score error {max(err, default=0.0):.2f} ulp")
        assert max(err, default=0.0) <= 4.0, f"{what} image {i}"


@pytest.mark.parametrize("mode", sorted(K.MODES))
@pytest.mark.parametrize("name", sorted(K.CASES))
def test_host_entry_gives_the_oracles_rows(name, mode):
    rows = yolo_post.detect_batch_multi(K.preds(name), K.device_head(name, mode), raise_errors=False)
    _same(rows, K.want(name, mode), f"{name} {mode}")


def test_device_entry_through_the_buffers():
    """Device pointers (torch's allocations are 16-byte aligned: the 16-byte loads), twice on the same buffers."""
    import torch
    dev = torch.device("cuda", 0)
    name, mode = "three_r16_c80", "multi"
    head, n = K.device_head(name, mode), K.CASES[name].batch
    xs = [torch.from_numpy(np.array(p)).to(dev) for p in K.preds(name)]
    bufs = yolo_post.MultiDetectionBuffers(n, dev, head)
    for _ in range(2):
        bufs.run([x.data_ptr() for x in xs], n, torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    rows = bufs.to_rows(bufs.dets.cpu().numpy(), bufs.counts.cpu().numpy(), head.max_det, raise_errors=False)
    _same(rows, K.want(name, mode), "device entry")


@pytest.mark.parametrize("mode", sorted(K.MODES))
def test_an_image_has_the_same_rows_alone_and_in_a_batch(mode):
    """Every field of every row equal (the score compared as the fp32 value it is), and the codes."""
    head, preds = K.device_head("nan", mode), K.preds("nan")
    rows = yolo_post.detect_batch_multi(preds, head, raise_errors=False)
    for i in range(3):
        assert yolo_post.detect_batch_multi([p[i:i + 1] for p in preds], head, raise_errors=False) == rows[i:i + 1], i
