"""GPU: a narrow YOLOv4-tiny imported from cfg text and Darknet-order weights, end to end: both
outputs against the float64 oracle with the group route (tests/darknet_v4_oracle.py), the plan (three
slice kernels) and the node-by-node path, and detect against the scale_x_y decode oracle
(tests/post_xy_oracle.py) on the plan's own outputs, with the default and the wide head."""
import functools

import numpy as np
import pytest

import darknet_import as D
import darknet_v4_oracle as V4O
import plan_fuzz_checks as K
import post_head_cases as HK
import post_multi_oracle as MO
import post_xy_oracle as XO
import ref_numpy as R
import v4tiny_cases as VK
import yolo_post

pytestmark = pytest.mark.gpu

NET_TOL = 1e-4  # normwise, the importer's existing bar (tests/test_gpu_darknet.py)


@functools.lru_cache(maxsize=None)
def _case():
    """(cfg, sections, layers, frames, the oracle's two outputs), computed once."""
    cfg = VK.narrow_cfg()
    secs = D.parse_cfg(cfg)
    layers = VK.random_layers(secs)
    x = VK.frames(VK.BATCH)
    want = V4O.forward(secs, layers, x)
    for a in want:
        a.setflags(write=False)
    return cfg, secs, layers, x, tuple(want)


def _model(**kw):
    cfg, secs, layers, x, want = _case()
    return D.DarknetModel(cfg, layers, in_shape=[VK.BATCH, VK.HEIGHT, VK.WIDTH, 3], **kw)


def _gold(m, outs, n):
    multi = MO.Multi(tuple(m.head.scales), "logistic")
    assert m.head.scale_x_y == (1.05, 1.05) and (m.head.nms, m.head.labels) == ("per_class", "multi")
    return [XO.detect_or_code([o[i] for o in outs], multi, m.head.scale_x_y, "multi") for i in range(n)]


def test_imported_narrow_yolov4_tiny_against_the_oracle_and_the_decode():
    cfg, secs, layers, x, want = _case()
    m = _model(score_thr=0.05)
    assert type(m.head) is yolo_post.MultiHead
    outs = [o.copy() for o in m.inference(x)]
    assert m.sess._plan is not None  # the plan ran, not the node-by-node path
    plan = m.sess.plan()
    names = [k["name"] for k in plan.kernels()]
    assert [n for n in names if n.startswith("slice")] == ["slice0", "slice1", "slice2"]
    assert sum(l.startswith("slice ") for l in plan.describe().splitlines()) == 3
    assert sum(l.startswith("conv ") for l in plan.describe().splitlines()) == 21
    assert [o.shape for o in outs] == [w.shape for w in want] == [(2, 2, 3, 24), (2, 4, 6, 24)]
    for k, (o, w) in enumerate(zip(outs, want)):
        K.check_finite(o, f"narrow YOLOv4-tiny head {k}")
        assert 0.01 < float(np.abs(w).mean()) < 100
        err = R.normwise_err(o, w)
        print(f"imported narrow YOLOv4-tiny head {k}: normwise error {err:.3e}")
        assert err < NET_TOL, f"head {k}: normwise error {err:.3e} >= {NET_TOL:.0e}"
    # detect: the device decode's rows are the scale_x_y oracle's on the plan's own outputs, exactly
    gold = _gold(m, outs, VK.BATCH)
    rows = m.detect(x, raise_errors=False)
    print(f"imported narrow YOLOv4-tiny: rows at score 0.05: {[r if isinstance(r, int) else len(r) for r in rows]}")
    assert len(rows) == VK.BATCH and any(not isinstance(r, int) and len(r) > 0 for r in rows)
    for i in range(VK.BATCH):
        HK.same_rows(rows[i], gold[i], f"detect image {i}")
    # ... which are not the rows of a decode that ignores scale_x_y
    multi = MO.Multi(tuple(m.head.scales), "logistic")
    plain = [XO.detect_or_code([o[i] for o in outs], multi, (1.0, 1.0), "multi") for i in range(VK.BATCH)]
    assert plain != gold
    # postprocessing (the host entry) of one image
    clean = [i for i in range(VK.BATCH) if not isinstance(gold[i], int)]
    assert clean
    boxes = m.postprocessing([o[clean[0]:clean[0] + 1] for o in outs])
    assert [(b[1], b[2]) for b in boxes] == [((r[1], r[2]), (r[3], r[4])) for r in gold[clean[0]]]
    # the wide head gives the same rows
    w = _model(score_thr=0.05, wide=True)
    assert type(w.head) is yolo_post.WideHead and w.head.scale_x_y == (1.05, 1.05)
    wide_rows = w.detect(x, raise_errors=False)
    for i in range(VK.BATCH):
        HK.same_rows(wide_rows[i], gold[i], f"wide detect image {i}")
    assert wide_rows == rows


def test_node_by_node_agrees_with_the_plan(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)  # debug=True saves every layer under ./intermediate
    cfg, secs, layers, x, want = _case()
    m = D.DarknetModel(cfg, layers, in_shape=[1, VK.HEIGHT, VK.WIDTH, 3], debug=True)
    outs = m.inference(x[:1])
    assert m.sess._plan is None  # node by node
    for k, (o, w) in enumerate(zip(outs, want)):
        err = R.normwise_err(o, w[:1])
        print(f"narrow YOLOv4-tiny node by node, head {k}: normwise error {err:.3e}")
        assert err < NET_TOL
    p = D.DarknetModel(cfg, layers, in_shape=[1, VK.HEIGHT, VK.WIDTH, 3])
    for k, (o, q) in enumerate(zip(outs, p.inference(x[:1]))):
        assert R.normwise_err(o, q) < NET_TOL, f"head {k}: node by node vs the plan"
    assert p.sess._plan is not None


def test_detect_images_runs_the_same_decode():
    """Letterboxed uint8 images through the model: rows in each image's pixels, none outside it."""
    m = _model(score_thr=0.05)
    rng = np.random.default_rng(9)
    images = [rng.integers(0, 256, (50, 80, 3), dtype=np.uint8), rng.integers(0, 256, (64, 96, 3), dtype=np.uint8)]
    rows = m.detect_images(images, raise_errors=False)
    assert len(rows) == 2
    for img, r in zip(images, rows):
        if isinstance(r, int):
            continue
        for _, l, t, rt, b, _ in r:
            assert 0 <= l <= rt < img.shape[1] and 0 <= t <= b < img.shape[0]
