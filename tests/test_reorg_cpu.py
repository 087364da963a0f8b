"""CPU: the YOLOv2 cfg definitions and their shapes, a weight-file round trip, the [reorg] / [region]
keys the importer refuses, the Reorg node's host path against the triple loop, and the lowering of
the passthrough to one reorg entry."""
import numpy as np
import pytest

import darknet_cases as DC
import darknet_import as D
import dnn_hip
import reorg_cases as RC


@pytest.mark.parametrize("model,n_out", [("yolov2", 425), ("yolov2_voc", 125), ("yolov2_tiny", 425),
                                         ("yolov2_tiny_voc", 125)])
def test_cfg_text_parses_to_the_published_shapes(model, n_out):
    secs = RC.parse(D.cfg_text(model))
    assert D.net_shape(secs) == (416, 416, 3) and secs[-1]["type"] == "region"
    shapes = D.layer_shapes(secs)
    assert shapes[-1] == shapes[-2] == (13, 13, n_out)
    kinds = [s["type"] for s in secs[1:]]
    assert kinds.count("convolutional") == (9 if "tiny" in model else 23)
    if "tiny" not in model:
        at = kinds.index("reorg")
        assert at == 27 and kinds[at + 1] == "route"
        assert shapes[at - 1:at + 2] == [(26, 26, 64), (13, 13, 256), (13, 13, 1280)]
    num, classes, anchors = D.region_params(secs[-1], secs[-2])
    assert (num, 5 * (5 + classes), len(anchors)) == (5, n_out, 10)


def test_weights_round_trip_the_region_head_and_the_lowering(tmp_path):
    secs = RC.parse(RC.narrow_cfg("yolov2"))
    layers = DC.darknet_layers(secs)
    path = str(tmp_path / "yolov2.weights")
    D.save_weights(path, layers)
    back = D.load_weights(path, secs)
    assert len(back) == 23
    for a, b in zip(layers, back):
        assert sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k]) for k in a)
    g, outs, yolos = D.build_graph(dnn_hip.DnnGraphBuilder, secs, back, [2, 96, 96, 3])
    assert outs[0].result.shape == (2, 3, 3, 40) and yolos[0]["grid"] == (3, 3)
    head = D.multi_head(yolos, 96, 96)
    assert (head.class_mode, head.nms, head.labels) == ("softmax", "per_class", "multi")
    assert (head.score_thr, head.iou_thr) == (D.SCORE_THR, D.IOU_THR)
    s = head.scales[0]  # region anchors are in cells: taken as they stand; the cell is input / grid
    assert (s.n_anchors, s.n_classes, s.cell) == (5, 3, 32.0)
    assert s.anchors == tuple(float(v) for v in secs[-1]["anchors"].split(","))
    # the passthrough ends in one reorg entry: no route or slice entry serves the reorg + concat pair
    joins = [e for e in dnn_hip.lower_graph(g)
             if isinstance(e, (dnn_hip.ReorgEntry, dnn_hip.RouteEntry, dnn_hip.SliceEntry))]
    assert [type(e) for e in joins] == [dnn_hip.ReorgEntry]
    assert (joins[0].stride, joins[0].slot, joins[0].slot_first) == (2, 1, False)
    assert [type(n) for n in joins[0].nodes] == [dnn_hip.Reorg, dnn_hip.Concat]


REFUSED = [  # (section, its line, the line instead, what the error names)
    ("reorg", "stride=2", "stride=2\nreverse=1", "reverse"),
    ("reorg", "stride=2", "stride=2\nflatten=1", "flatten"),
    ("reorg", "stride=2", "stride=2\nextra=4", "extra"),
    ("reorg", "stride=2", "stride=4", "stride"),  # a 6 x 6 map
    ("region", "softmax=1", "softmax=1\nsoftmax_tree=data/9k.tree", "softmax_tree"),
    ("region", "softmax=1", "softmax=1\nbackground=1", "background"),
    ("region", "softmax=1", "softmax=1\nclassfix=1", "classfix"),
    ("region", "softmax=1", "softmax=0", "softmax"),
    ("region", "coords=4", "coords=6", "coords"),
    ("region", "num=5", "num=4", "num"),
    ("region", "num=5", "num=17", "DNN_YOLO_MAX_ANCHORS"),
    ("region", "classes=3", "classes=129", "DNN_YOLO_MAX_CLASSES"),
    ("region", "classes=3", "classes=4", "filters"),
    ("convolutional", "activation=linear", "activation=leaky", "activation"),  # the conv before [region]
    ("region", "random=1", "random=1\n[maxpool]\nsize=2\nstride=1", "last section"),
]


@pytest.mark.parametrize("kind,old,new,word", REFUSED, ids=[f"{r[0]}-{r[3]}" for r in REFUSED])
def test_refused_keys_are_named(kind, old, new, word):
    head, sep, tail = RC.narrow_cfg("yolov2").rpartition(f"[{kind}]")
    assert sep and old in tail
    with pytest.raises(D.DarknetError, match=word):
        D.layer_shapes(RC.parse(head + sep + tail.replace(old, new, 1)))


@pytest.mark.parametrize("case", [RC.KERNEL_CASES[1], RC.KERNEL_CASES[4]], ids=["4x6x8s2", "6x9x9s3"])
def test_reorg_node_host_path_is_the_triple_loop(case):
    h, w, c, stride, _, _, n = case
    a, _ = RC.arange_inputs(n, h, w, c, stride, 0)
    g = dnn_hip.DnnGraphBuilder()
    x = g.create_input([n, h, w, c])
    node = g.create_reorg(x, stride)
    x.result[...] = a
    node.run()
    np.testing.assert_array_equal(node.result, RC.reorg_loops(a, stride))
    g.set_out_node(node)  # alone it is an entry of its own with no slot
    (alone,) = dnn_hip.lower_graph(g)
    assert isinstance(alone, dnn_hip.ReorgEntry) and (alone.stride, alone.slot) == (stride, -1)
