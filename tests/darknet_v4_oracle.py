"""TEST INFRASTRUCTURE ONLY: tests/darknet_oracle.py's float64 Darknet forward, extended by the
channel-group [route] of YOLOv4-tiny's CSP blocks.  Every other section is darknet_oracle's own
function, imported, not copied.

Darknet's route layer (parse_route, forward_route_layer) with `groups` and `group_id` takes of each
input layer the channels [group_id * c / groups, (group_id + 1) * c / groups) and concatenates the
parts; with groups = 1 (the default) that is the plain concat."""
import numpy as np

import darknet_oracle as DO


def route_layer(sec, srcs):
    groups, gid = int(sec.get("groups", 1)), int(sec.get("group_id", 0))
    parts = []
    for t in srcs:
        c = t.shape[3]
        assert c % groups == 0 and 0 <= gid < groups
        part = c // groups
        parts.append(t[..., gid * part:(gid + 1) * part])
    return np.ascontiguousarray(np.concatenate(parts, axis=3))


def forward(sections, layers, x):
    """The tensors the [yolo] sections read (the conv before each), in cfg order, fp32."""
    outs, heads = [], []
    weights = iter(layers)
    cur = np.asarray(x, np.float32)
    for at, sec in enumerate(sections[1:]):
        kind = sec["type"]

        def ref(v):
            v = int(v)
            return outs[at + v if v < 0 else v]

        if kind == "convolutional":
            cur = DO.conv_layer(cur, sec, next(weights))
        elif kind == "shortcut":
            cur = (cur.astype(np.float64) + ref(sec["from"]).astype(np.float64)).astype(np.float32)
        elif kind == "route":
            cur = route_layer(sec, [ref(v) for v in sec["layers"].split(",")])
        elif kind == "upsample":
            f = int(sec.get("stride", 2))
            cur = cur.repeat(f, axis=1).repeat(f, axis=2)
        elif kind == "maxpool":
            cur = DO.maxpool_layer(cur, sec)
        elif kind == "yolo":
            heads.append(cur)
        else:
            raise ValueError(f"section [{kind}]")
        outs.append(cur)
    return heads
