"""Shared cases of tests/test_darknet_v4tiny_cpu.py and tests/test_gpu_darknet_v4tiny.py: the narrow
YOLOv4-tiny the tests import, a one-line form of a lowered entry, and a replay of a plan's slots."""
import numpy as np

import darknet_import as D
import dnn_hip

CLASSES, WIDTH, HEIGHT, WIDTH_DIV = 3, 96, 64, 4
BATCH = 2


def narrow_cfg():
    return D.cfg_text("yolov4-tiny", classes=CLASSES, width=WIDTH, height=HEIGHT, width_div=WIDTH_DIV)


def random_layers(sections, seed=0):
    """Seeded random weights and BatchNorm statistics in load_weights' format (tests/darknet_cases.py's
    style with numpy's generator): He-scaled kernels, gamma of mixed sign with one exact zero, variance in
    [0.5, 1.5), non-trivial beta; a linear head's weights and biases are a quarter of that, so the
    decode's exp() gives boxes of about an anchor's size."""
    rng = np.random.default_rng(4000 + seed)
    layers = []
    for n, c, size, bn in D.conv_shapes(sections):
        w = (rng.standard_normal((n, c, size, size)) * np.sqrt(2.0 / (c * size * size))).astype(np.float32)
        if not bn:
            layers.append({"biases": (rng.standard_normal(n) * 0.25).astype(np.float32), "weights": w * np.float32(0.25)})
            continue
        gamma = rng.uniform(0.75, 1.5, n).astype(np.float32)
        gamma[::3] *= np.float32(-1)
        if n > 4:
            gamma[4] = 0
        layers.append({"biases": (rng.standard_normal(n) * 0.5).astype(np.float32), "weights": w, "scales": gamma,
                       "rolling_mean": (rng.standard_normal(n) * 0.2).astype(np.float32),
                       "rolling_variance": rng.uniform(0.5, 1.5, n).astype(np.float32)})
    return layers


def frames(n, seed=1):
    return np.random.default_rng(5000 + seed).uniform(0, 1, (n, HEIGHT, WIDTH, 3)).astype(np.float32)


def entry_line(e):
    """One lowered entry as text: its type and the arguments the plan call takes."""
    name = type(e).__name__
    if isinstance(e, dnn_hip.PaddedConvEntry):
        c = e.conv
        return (f"{name} k{'x'.join(map(str, c.kernel.shape))} s{c.strides[1]},{c.strides[2]} pads{e.pads[0]},{e.pads[1]} "
                f"affine={e.affine is not None} leaky={e.leaky}")
    if isinstance(e, dnn_hip.ConvEntry):
        c = e.conv
        return (f"{name} k{'x'.join(map(str, c.kernel.shape))} s{c.strides[1]},{c.strides[2]} {c.padding} "
                f"bias={e.bias is not None} bn={e.bn is not None} leaky={bool(e.leaky)}")
    if isinstance(e, dnn_hip.PoolEntry):
        p = e.pool
        return f"{name} k{p.ksize[1]},{p.ksize[2]} s{p.strides[1]},{p.strides[2]} {p.padding}"
    if isinstance(e, dnn_hip.RouteEntry):
        return f"{name} block={e.block} slot={e.slot} slot_first={e.slot_first}"
    if isinstance(e, dnn_hip.ShortcutEntry):
        return f"{name} slot={e.slot} leaky={bool(e.leaky)}"
    if isinstance(e, dnn_hip.UpsampleEntry):
        return f"{name} factor={e.factor}"
    if isinstance(e, dnn_hip.SppEntry):
        return f"{name} ksizes={e.ksizes} x_first={e.x_first}"
    if isinstance(e, dnn_hip.SliceEntry):
        return f"{name} first={e.first} channels={e.channels}"
    if isinstance(e, dnn_hip.TapEntry):
        return f"{name} index={e.index}"
    return f"{name} slot={e.slot}"  # stash, restore, release


def replay_slots(entries):
    """Walks the entries as dnn_plan_add_* would: (the most slots live at once, the slots still live at
    the end).  Asserts that a stash takes the lowest free number and that restore, route, shortcut and
    release name a live slot."""
    live, most = set(), 0
    for e in entries:
        if isinstance(e, dnn_hip.StashEntry):
            assert e.slot == dnn_hip._free_slots(live, 1)[0], (e.slot, live)
            live.add(e.slot)
            most = max(most, len(live))
        elif isinstance(e, (dnn_hip.RestoreEntry, dnn_hip.ShortcutEntry)):
            assert e.slot in live, (type(e).__name__, e.slot, live)
        elif isinstance(e, dnn_hip.RouteEntry):
            assert e.slot == -1 or e.slot in live, (e.slot, live)
        elif isinstance(e, dnn_hip.ReleaseEntry):
            assert e.slot in live, (e.slot, live)
            live.discard(e.slot)
    return most, live
