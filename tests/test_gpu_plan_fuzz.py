"""Multi-layer plans on poisoned, guarded, caller-owned buffers against the float64 oracle.

The per-layer tests run plans that own their workspace (a fresh allocation: zero pages) and
mostly one layer deep.  bench.py and the multi-rank runner instead hand plans torch.empty
buffers that earlier plans have used, and the chooser picks a layer's kernel from its
predecessor.  Here every case of tests/plan_fuzz_cases.py is lowered through the product path
(DnnGraphBuilder + lower_graph + Plan.memory) onto torch buffers that were filled with 0xFF
(a NaN as fp32, fp16 and bf16) BEFORE the plan was created, with 4096-byte guards around the
weight arena and the workspace, NaN guards around the input frames and a canary-filled output:

  * a plan whose result depends on bytes it did not write this run (im2col padding columns,
    rows past M of a ragged tile, an activation slot of an earlier run, packed-weight padding)
    produces NaNs or differs from the same plan on zeroed buffers;
  * a kernel that writes outside what dnn_plan_memory reported, or past the n rows of a ragged
    run, hits a guard or a canary;
  * every block is checked against the oracle by teacher forcing (the prefix plan's output is
    the oracle's input for the next block), so the bar is the per-layer one at any depth.

Poison reaches arithmetic only: the one workspace word a kernel uses as a counter is the
split-K ticket (gemm_f32.h splitk_combine / splitk_sum), which dnn_plan_finalize zeroes, and no
kernel spins on memory."""
import contextlib

import numpy as np
import pytest
import torch

import dnn_hip
import plan_fuzz_cases as F
import plan_fuzz_checks as K

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _graph(B, shape, blocks, ws):
    g = dnn_hip.DnnGraphBuilder()
    y = g.create_input([B] + list(shape))
    for b, (kern, bias, bn, leaky) in zip(blocks, ws):
        if b["pre_pool"]:
            y = g.create_max_pool2d(y, [1, 2, 2, 1], [1, 1, 1, 1], "SAME")
        y = g.create_conv2d(y, kern, [1, 1, 1, 1], "SAME")
        if bias is not None:
            y = g.create_bias_add(y, bias)
        if bn is not None:
            y = g.create_batch_norm(y, *bn, 1e-5)
        if leaky:
            y = g.create_leaky_relu(y)
        if b["pool"]:
            s = 2 if b["pool"] == "s2" else 1
            y = g.create_max_pool2d(y, [1, 2, 2, 1], [1, s, s, 1], "SAME")
    g.set_out_node(y)
    return g


class GuardedPlan(object):
    """A plan on caller-owned buffers.  poison=True: arena and workspace (guards included) are
    0xFF before the plan exists; poison=False: zeros (the state a plan-owned allocation has)."""

    def __init__(self, kind, B, shape, blocks, ws, poison=True):
        entries = dnn_hip.lower_graph(_graph(B, shape, blocks, ws))
        assert entries is not None
        kw = {"precision": "fp16" if kind == "fp16" else "fp32", "latency": kind == "latency"}
        wb, sb = dnn_hip.Plan.memory(B, shape, entries, **kw)
        fill = K.POISON if poison else 0
        self.poison = poison
        self.wbuf = torch.full((wb + 2 * K.GUARD_BYTES,), fill, dtype=torch.uint8, device=DEV)
        self.sbuf = torch.full((sb + 2 * K.GUARD_BYTES,), fill, dtype=torch.uint8, device=DEV)
        torch.cuda.synchronize()
        self.plan = dnn_hip.Plan(B, shape, entries, device=0, weights_ptr=self.wbuf.data_ptr() + K.GUARD_BYTES,
                                 workspace_ptr=self.sbuf.data_ptr() + K.GUARD_BYTES, **kw)
        self.B, self.shape = B, tuple(shape)
        self.in_floats = int(np.prod(shape))
        self.row = int(np.prod(self.plan.out_shape))
        self.xin = torch.empty(2 * K.GUARD_FLOATS + B * self.in_floats, dtype=torch.float32, device=DEV)
        self.out = torch.empty(2 * K.GUARD_FLOATS + B * self.row, dtype=torch.int32, device=DEV)

    def describe(self):
        return self.plan.describe()

    def run(self, x, what):
        """Run the first n = len(x) rows; returns y [n, OH, OW, OC] after checking the canaries
        (output guards and rows >= n) and the guards of the arena and the workspace."""
        n = x.shape[0]
        assert n <= self.B and tuple(x.shape[1:]) == self.shape
        self.xin.fill_(float("nan"))
        self.xin[K.GUARD_FLOATS:K.GUARD_FLOATS + n * self.in_floats] = torch.from_numpy(x.reshape(-1)).to(DEV)
        self.out.fill_(K.CANARY)
        self.plan.run_device(n, self.xin.data_ptr() + 4 * K.GUARD_FLOATS, self.out.data_ptr() + 4 * K.GUARD_FLOATS)
        torch.cuda.synchronize()
        flat = self.out.cpu().numpy()
        K.check_canary(flat, n, self.row, self.B, f"{what}: output")
        if self.poison:
            for name, buf in (("workspace", self.sbuf), ("weight arena", self.wbuf)):
                ends = torch.cat([buf[:K.GUARD_BYTES], buf[-K.GUARD_BYTES:]]).cpu().numpy()
                K.check_guard(ends, f"{what}: {name}")
        y = flat[K.GUARD_FLOATS:K.GUARD_FLOATS + n * self.row].view(np.float32)
        return y.reshape((n,) + self.plan.out_shape).copy()

    def close(self):
        self.plan.close()


@contextlib.contextmanager
def _case_info(info):
    try:
        yield
    except AssertionError as e:
        raise AssertionError(f"{e}\n{info()}") from None


@pytest.mark.parametrize("seed", range(F.NSEEDS))
def test_plan_chain_fuzz(seed):
    kind, B, shape, blocks = F.chain_case(seed)
    X, X2, ws = F.case_tensors(seed, B, shape, blocks)
    tol = K.FP16_LAYER_TOL if kind == "fp16" else K.LAYER_TOL
    plans = []

    def make(*a, **kw):
        plans.append(GuardedPlan(*a, **kw))
        return plans[-1]

    def info():
        return (f"seed {seed}: kind={kind} B={B} frame={shape} blocks={blocks}\n" +
                "\n".join(p.describe() for p in plans[:1]))

    try:
        with _case_info(info):
            # 1, 2: poisoned buffers, three runs through one plan; the same inputs on zeroed buffers
            full = make(kind, B, shape, blocks, ws)
            k = max(1, B // 2)
            y1 = full.run(X, "run 1 (n = B)")
            y2 = full.run(X2[:k], "run 2 (n < B)") if B > 1 else None
            y3 = full.run(X, "run 3 (n = B)")
            K.check_finite(y1, "run 1")
            K.check_bits(y3, y1, "run 3 against run 1")
            clean = make(kind, B, shape, blocks, ws, poison=False)
            K.check_bits(y1, clean.run(X, "clean run"), "poisoned run 1 against the zeroed-buffer plan")
            if y2 is not None:
                K.check_finite(y2, "run 2")
                fresh = make(kind, B, shape, blocks, ws, poison=False)  # has run nothing else
                K.check_bits(y2, fresh.run(X2[:k], "fresh clean run"),
                             "poisoned run 2 (n < B) against a fresh zeroed-buffer plan")
            # 3: per-block accuracy by teacher forcing through the prefix plans
            a_prev = X
            for j in range(1, len(blocks) + 1):
                a_j = y1 if j == len(blocks) else make(kind, B, shape, blocks[:j], ws[:j]).run(X, f"prefix {j}")
                err = K.check_layer_err(a_j, K.oracle_block(a_prev, blocks[j - 1], ws[j - 1]), tol,
                                        f"block {j} of {len(blocks)} (teacher forced)")
                print(f"seed {seed} block {j}: normwise error {err:.3e}")
                a_prev = a_j
            # 4: batch rows equal the one-frame plan's where it runs the same kernels
            if kind != "latency" and B > 1:
                one = make(kind, 1, shape, blocks, ws)
                same = ([F.layer_config(ln) for ln in one.describe().splitlines()] ==
                        [F.layer_config(ln) for ln in full.describe().splitlines()])
                if same:
                    K.check_bits(y1[:1], one.run(X[:1], "one-frame plan"), "row 0 against the one-frame plan")
    finally:
        for p in plans:
            p.close()


def test_plan_mark_and_post_after():
    """dnn_plan_set_mark / dnn_plan_wait_mark through ShardedRunner(post_after=...), the bench's
    default path: a step's postprocess waits for the mark inside the NEXT step's forward.  The
    detections of 4 steps of different frames must equal, step by step and byte for byte, those
    of the same runner without post_after."""
    import dist as D
    import yolo_post
    B, shape = 3, (26, 26, 32)
    rng = np.random.default_rng(77)
    ws = []
    for k, c, oc, head in ((3, 32, 64, False), (3, 64, 128, False), (1, 128, 125, True)):
        kern = (rng.standard_normal((k, k, c, oc)) * np.sqrt(2.0 / (k * k * c))).astype(np.float32)
        if head:
            kern *= 2.0  # peaked class scores: some boxes pass the detection threshold
        ws.append((kern, (rng.standard_normal(oc) * 0.1).astype(np.float32), None, not head))
    blocks = [{"pre_pool": False, "pool": "s2"}, {"pre_pool": False, "pool": None}, {"pre_pool": False, "pool": None}]
    plan = dnn_hip.Plan.from_graph(_graph(B, shape, blocks, ws), device=0)
    assert plan.out_shape == (13, 13, 125)
    dev = torch.device("cuda", 0)
    frames = [torch.from_numpy(rng.standard_normal((B,) + shape).astype(np.float32)).to(dev) for _ in range(4)]
    stream = torch.cuda.current_stream(dev)

    def compute(inp, out, n):
        plan.run_device(n, inp.data_ptr(), out.data_ptr(), stream.cuda_stream)

    def steps(post_after):
        runner = D.ShardedRunner(compute, B, shape, (13, 13, 125), dev, post_after=post_after)
        dbufs = [yolo_post.DetectionBuffers(runner.shard_cap, dev) for _ in range(runner.slots)]

        def post(out, n, slot, post_stream):
            dbufs[slot].run(out.data_ptr(), n, post_stream)
            return dbufs[slot].pack(n, post_stream)

        got, pending = [], []
        for i, f in enumerate(frames):
            pending.append(runner.launch_detections(f, post, i % runner.slots))
            if len(pending) == runner.inflight:
                got.append(runner.finish_detections(pending.pop(0)))
        while pending:
            got.append(runner.finish_detections(pending.pop(0)))
        got.append(runner.flush_detections())
        torch.cuda.synchronize()
        return [r for r in got if r is not None]

    with pytest.raises(dnn_hip.DnnHipError, match="no mark set"):
        plan.wait_mark(stream.cuda_stream)
    last_conv = [k["name"] for k in plan.kernels() if k["name"].startswith("conv")][-1]
    plan.set_mark(last_conv)
    marked = steps(plan.wait_mark)
    side = torch.cuda.Stream(dev)
    y_g = torch.empty((B, 13, 13, 125), device=dev)
    with pytest.raises(dnn_hip.DnnHipError, match="a mark is set"):
        plan.run_graph(B, frames[0].data_ptr(), y_g.data_ptr(), side.cuda_stream)
    plan.set_mark(None)
    with pytest.raises(dnn_hip.DnnHipError, match="no mark set"):
        plan.wait_mark(stream.cuda_stream)
    plan.run_graph(B, frames[0].data_ptr(), y_g.data_ptr(), side.cuda_stream)
    side.synchronize()
    y_e = torch.empty_like(y_g)
    plan.run_device(B, frames[0].data_ptr(), y_e.data_ptr(), stream.cuda_stream)
    torch.cuda.synchronize()
    assert torch.equal(y_g, y_e)
    plain = steps(None)
    assert len(marked) == len(plain) == len(frames)
    for i, ((d0, c0), (d1, c1)) in enumerate(zip(marked, plain)):
        assert np.array_equal(c0, c1), i
        assert d0.shape == d1.shape and d0.tobytes() == d1.tobytes(), i
    per_step = [int(np.clip(c, 0, None).sum()) for _, c in plain]
    assert all(n > 0 for n in per_step), per_step  # the comparison is not of empty lists
    assert len({d.tobytes() for d, _ in plain}) == len(frames)  # different frames, different detections
    plan.close()
