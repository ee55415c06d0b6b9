"""The device-resident training log: xggm_train_log_append against a numpy restatement of its contract (ring, masks,
ordered fp64 sums, first non-finite record; bit for bit), bit-equality of eager launches, graph replays and launches
beside foreign work, and its users -- ``CapturedTrainer(train_log=)`` and the eager ``train_iteration(train_log=)``:
the log observes only, holds exactly what the passes return, and is never read before ``read()``."""
import collections
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from xggm_amd import synth  # noqa: E402
from helpers import batch_tensors  # noqa: E402

DEV = "cuda"
COLS, KINDS = 8, 4


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


# ----------------------------------------------------------------------------- the contract, restated
class Restated:
    """xggm_train_log_append as include/xggm.h states it, in numpy on the host"""

    def __init__(self, capacity):
        self.capacity = capacity
        self.values = np.zeros((capacity, COLS), np.float32)
        self.steps = np.zeros(capacity, np.int64)
        self.kinds = np.zeros(capacity, np.int32)
        self.cursor = 0
        self.sums = np.zeros((KINDS, COLS), np.float64)
        self.counts = np.zeros(KINDS, np.int64)
        self.first_bad = -1

    def append(self, cols, mul, kind, step):
        """``cols``: np.float32 values or None; ``mul``: floats or None"""
        r = self.cursor
        row = r % self.capacity
        mask, bad = 0, False
        with np.errstate(all="ignore"):
            for i in range(COLS):
                v = np.float32(0)
                if i < len(cols) and cols[i] is not None:
                    v = np.float32(cols[i]) * np.float32(1.0 if mul is None else mul[i])  # ONE fp32 multiply
                    mask |= 1 << i
                    self.sums[kind, i] = self.sums[kind, i] + np.float64(v)
                    bad = bad or not np.isfinite(v)
                self.values[row, i] = v
        if step is not None:
            self.steps[row] = step
        self.kinds[row] = kind | (mask << 8)
        self.counts[kind] += 1
        if self.first_bad < 0 and bad:
            self.first_bad = r
        self.cursor = r + 1


def _bits(a, dt):
    return np.ascontiguousarray(a).view(dt)


def _assert_equals_restated(log, want):
    torch.cuda.synchronize()
    assert int(log.cursor.item()) == want.cursor
    assert int(log.first_bad_word.item()) == want.first_bad
    assert log.counts.cpu().numpy().tolist() == want.counts.tolist()
    assert np.array_equal(_bits(log.values.cpu().numpy(), np.int32), _bits(want.values, np.int32))  # floats by bit pattern
    assert np.array_equal(_bits(log.sums.cpu().numpy(), np.int64), _bits(want.sums, np.int64))     # fp64 by bit pattern
    assert np.array_equal(log.steps.cpu().numpy(), want.steps)
    assert np.array_equal(log.kinds.cpu().numpy(), want.kinds)


def _ring_plan(seed=3):
    """the issue's 11 appends: n cycles 1, 3, 8 with NULL columns in the middle, kinds cycle 0, 1, 2, factors on the odd
    appends -> (values fp32 [11, 8], [(present columns or None per column, mul or None, kind, step)])"""
    g = torch.Generator().manual_seed(seed)
    vals = (torch.randn(11, COLS, generator=g) * torch.exp(torch.randn(11, COLS, generator=g) * 4.0)).float()
    plan = []
    for k in range(11):
        n = (1, 3, 8)[k % 3]
        present = [True] * n
        if n == 3:
            present[1] = False
        if n == 8:
            present[2] = present[5] = False
        mul = [float(np.float32(m)) for m in (0.5, 1.0 / 3.0, 3.0, 1.0 / 464.0, 1.0 / 6.0, 7.25, 1e-3, 1e3)[:n]] if k % 2 else None
        plan.append((present, mul, k % 3, 1000 + 7 * k))
    return vals, plan


def _run_plan(log, dvals, dsteps, plan):
    from xggm_amd import ops
    for k, (present, mul, kind, _) in enumerate(plan):
        # 0-dim and 1-element views alike
        cols = [(dvals[k, i] if i % 2 else dvals[k, i:i + 1]) if p else None for i, p in enumerate(present)]
        ops.train_log_append(log, kind, cols, mul, step=dsteps[k:k + 1])


def test_ring_masks_kinds_and_sums_equal_the_restated_rules():
    from xggm_amd.engine import TrainLog
    vals, plan = _ring_plan()
    log = TrainLog(4, DEV)
    want = Restated(4)
    dsteps = torch.tensor([s for _, _, _, s in plan], dtype=torch.int64, device=DEV)
    _run_plan(log, vals.to(DEV), dsteps, plan)
    v = vals.numpy()
    for k, (present, mul, kind, step) in enumerate(plan):
        want.append([v[k, i] if p else None for i, p in enumerate(present)], mul, kind, step)
    assert want.cursor == 11
    _assert_equals_restated(log, want)
    rec = log.read()
    assert int(rec["cursor"]) == 11 and int(rec["first_bad"]) == -1
    # the retained records are records 7 .. 10, oldest first
    assert rec["steps"].tolist() == [1000 + 7 * k for k in (7, 8, 9, 10)]
    assert rec["kinds"].tolist() == [k % 3 for k in (7, 8, 9, 10)]
    for j, k in enumerate((7, 8, 9, 10)):
        present, mul, _, _ = plan[k]
        assert rec["present"][j].tolist() == (present + [False] * COLS)[:COLS]
        for i in range(COLS):
            x = np.float32(v[k, i]) * np.float32(1.0 if mul is None else mul[i]) if i < len(present) and present[i] else np.float32(0)
            assert rec["values"][j, i].numpy().view(np.int32) == x.view(np.int32), (k, i)
    assert rec["counts"].tolist() == [4, 4, 3, 0]
    assert np.array_equal(_bits(rec["sums"].numpy(), np.int64), _bits(want.sums, np.int64))
    # reset() empties it, in stream order
    log.reset()
    _assert_equals_restated(log, Restated(4))


@pytest.mark.parametrize("order,total", [((2.0 ** 60, 1.0, -2.0 ** 60), 0.0), ((1.0, 2.0 ** 60, -2.0 ** 60), 0.0),
                                         ((2.0 ** 60, -2.0 ** 60, 1.0), 1.0)])
def test_the_fp64_sum_is_taken_in_append_order(order, total):
    """2**60, 1 and -2**60 are exact in fp32 and 2**60 + 1 is not representable in fp64: only the append order gives
    these totals"""
    from xggm_amd import ops
    from xggm_amd.engine import TrainLog
    log = TrainLog(2, DEV)
    src = torch.tensor(order, dtype=torch.float32, device=DEV)
    other = torch.tensor([5.0], device=DEV)
    for k in range(3):
        ops.train_log_append(log, 1, [src[k]])
        ops.train_log_append(log, 2, [other])  # another kind in between: its sums are its own
    rec = log.read()
    assert float(rec["sums"][1, 0]) == total
    assert float(rec["sums"][2, 0]) == 15.0 and rec["counts"].tolist() == [0, 3, 3, 0]
    assert rec["sums"].flatten().count_nonzero() == (2 if total else 1)


def test_first_bad_names_the_first_non_finite_record():
    from xggm_amd import _lib, ops
    from xggm_amd.engine import TrainLog
    inf, nan = float("inf"), float("nan")
    log = TrainLog(8, DEV)
    col0 = torch.tensor([1.0, 2.0, 3.0, 4.0, 5.0], device=DEV)
    col1 = torch.tensor([0.5, 0.25, inf, nan, 8.0], device=DEV)
    for k in range(5):  # non-finite values are plain data here
        ops.train_log_append(log, 0, [col0[k], col1[k]])
    rec = log.read()
    assert int(rec["first_bad"]) == 2 == log.first_bad() == log.first_bad(rec) and int(rec["cursor"]) == 5
    assert np.isnan(float(rec["sums"][0, 1])) and float(rec["sums"][0, 0]) == 15.0
    assert rec["sums"].flatten()[2:].count_nonzero() == 0
    assert np.isinf(float(rec["values"][2, 1])) and np.isnan(float(rec["values"][3, 1])) and float(rec["values"][4, 1]) == 8.0

    # what does not count: a non-finite factor at an absent (NULL) column, and a non-finite value at a column >= n
    log = TrainLog(8, DEV)
    bad = torch.tensor([inf, nan], device=DEV)
    ops.train_log_append(log, 3, [col0[0], None, col0[1]], mul=[1.0, nan, 1.0])
    src = (ctypes.c_void_p * COLS)(col0[2:].data_ptr(), col0[3:].data_ptr(), bad[0:].data_ptr(), bad[1:].data_ptr(),
                                   bad[0:].data_ptr(), bad[1:].data_ptr(), bad[0:].data_ptr(), bad[1:].data_ptr())
    d = ops.TrainLogDesc(log.values.data_ptr(), log.steps.data_ptr(), log.kinds.data_ptr(), log.cursor.data_ptr(),
                         log.sums.data_ptr(), log.counts.data_ptr(), log.first_bad_word.data_ptr(), log.capacity)
    _lib.call("xggm_train_log_append", ctypes.cast(src, ctypes.c_void_p), None, 2, 3, None, ctypes.addressof(d), _lib.stream())
    rec = log.read()
    assert int(rec["first_bad"]) == -1 and int(rec["cursor"]) == 2
    assert rec["values"].tolist() == [[1.0, 0.0, 2.0, 0, 0, 0, 0, 0], [3.0, 4.0, 0, 0, 0, 0, 0, 0]]
    assert rec["present"].tolist() == [[True, False, True] + [False] * 5, [True, True] + [False] * 6]
    assert rec["sums"][3].tolist() == [4.0, 4.0, 2.0, 0, 0, 0, 0, 0] and rec["steps"].tolist() == [0, 0]
    # ... and one that does: the log notices it however late it comes
    ops.train_log_append(log, 3, [col0[0], None, bad[1]])
    assert log.first_bad() == 2


def test_same_bits_eagerly_replayed_and_beside_foreign_work():
    from xggm_amd.engine import TrainLog
    vals, plan = _ring_plan(seed=9)
    plan = plan[:6]
    dvals = vals.to(DEV)
    dsteps = torch.tensor([s for _, _, _, s in plan], dtype=torch.int64, device=DEV)
    eager, replayed, beside = TrainLog(4, DEV), TrainLog(4, DEV), TrainLog(4, DEV)
    _run_plan(eager, dvals, dsteps, plan)

    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _run_plan(replayed, dvals, dsteps, plan)
    torch.cuda.synchronize()
    assert int(replayed.cursor.item()) == 0  # a capture runs nothing
    g.replay()

    big = torch.empty(64 << 20, dtype=torch.float32, device=DEV)  # 256 MB: a copy that is still busy while the appends run
    big2 = torch.empty_like(big)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for _ in range(4):
            big2.copy_(big)
    _run_plan(beside, dvals, dsteps, plan)
    torch.cuda.synchronize()
    assert torch.equal(eager.buf, replayed.buf) and torch.equal(eager.buf, beside.buf)
    assert int(eager.cursor.item()) == 6


# ----------------------------------------------------------------------------- the tiny model (local twin of the engine tests')
def _tiny(seed_w, seed_rt, dtype, A=29):
    from oracle import shapes
    from xggm_amd import param
    from xggm_amd.lxrt.modeling import BertConfig, VISUAL_CONFIG
    from xggm_amd.vqa.vqacpv2 import make_optimizer
    from xggm_amd.vqa.vqacpv2_model import VQAModel
    cfg = dict(shapes.TINY, l_layers=2, x_layers=2, r_layers=1)  # H = 128
    VISUAL_CONFIG.set_visual_dims(cfg["feat_dim"], 4)
    a = param.parse_args(["--llayers", "2", "--xlayers", "2", "--rlayers", "1"])
    bc = BertConfig(cfg["vocab"], hidden_size=cfg["hidden"], num_attention_heads=cfg["heads"],
                    intermediate_size=cfg["inter"], max_position_embeddings=cfg["max_pos"])
    m = VQAModel(A, gnn="GCN", n_layers=2, args=a, config=bc, compute_dtype=dtype)
    m.load_state_dict({k: torch.from_numpy(synth.seeded_param(k, v.shape, seed_w)) for k, v in m.state_dict().items()})
    m = m.to(DEV)
    m.seed = seed_rt
    return cfg, m, make_optimizer(m, 1e-4, T_TOTAL)


B, A, T_TOTAL, WARMUP = 4, 29, 40, 0.1  # make_optimizer's warmup
BRANCHES = ("rel", "node", "rel")
WARM_PASSES = 3  # CapturedTrainer(warmup_iters=1) runs plain, rel, node once before it captures (a capture runs nothing)


def _state(m):
    from xggm_amd.runtime import runtime_of
    rt = runtime_of(m)
    arena = rt.arena
    st = {k: getattr(arena, k).clone() for k in ("params", "m", "v", "shadow") if getattr(arena, k) is not None}
    st["steps"], st["lr_scale"], st["rng"] = arena.steps.clone(), arena.lr_scale.clone(), rt.rng.clone()
    return st


@pytest.fixture(scope="module", params=[torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def runs(request):
    """three iterations (rel, node, rel) on three batches, five ways from the same seed: captured with a log of 4 records
    (under the host-synchronisation spies), captured without one (reading every pass's outputs with ``float()`` -- the
    very sync the log removes), eager ``CapturedTrainer(use_graph=False)`` with a log, the eager
    ``train_iteration(train_log=)`` with a log, and eager passes without one that read the loss terms"""
    from xggm_amd import ops
    from xggm_amd.engine import CapturedTrainer, TrainLog
    from xggm_amd.vqa.vqacpv2 import train_iteration, plain_pass, ggm_pass
    dtype = request.param
    out = {"dtype": dtype}
    real_call = ops.call
    mp = pytest.MonkeyPatch()
    for name in ("logged", "bare", "eager", "iteration", "bare_eager"):
        cfg, m, o = _tiny(5, 11, dtype)
        b = [batch_tensors(synth.vqa_batch(B, A=A, F=cfg["feat_dim"], vocab=cfg["vocab"], seed=s), DEV) for s in (3, 4, 5, 6)]
        log = TrainLog(4, DEV) if name in ("logged", "eager", "iteration") else None
        seen, floats, syncs = [], [], []

        def spy(fn, *a, _seen=seen):
            _seen.append(fn)
            return real_call(fn, *a)

        ops.call = spy
        try:
            t = CapturedTrainer(m, o, b[0], sigma=1.0, warmup_iters=1, use_graph=name in ("logged", "bare"),
                                train_log=log if name != "iteration" else None)
            if not t.use_graph:
                for kind in ("plain", "rel", "node"):  # the constructor's warm-up passes, by hand
                    t._eager_pass(kind)
                if log is not None:
                    log.reset()
            if name == "logged":
                # from here to read(): no synchronising call.  Counted always; where torch's sync debug mode catches a
                # deliberate .item() it is in force as well
                use_mode = _sync_mode_raises()
                for meth in ("cpu", "item", "tolist", "numpy"):
                    _count(mp, torch.Tensor, meth, syncs, lambda x: x.is_cuda)
                for owner in (torch.cuda.Stream, torch.cuda.Event):
                    _count(mp, owner, "synchronize", syncs, lambda s: True)
                real_sync = torch.cuda.synchronize
                mp.setattr(torch.cuda, "synchronize", lambda *a, **k: (syncs.append("synchronize"), real_sync(*a, **k))[1])
                torch.cuda.synchronize()
                syncs.clear()
                if use_mode:
                    torch.cuda.set_sync_debug_mode("error")
            try:
                for i, br in enumerate(BRANCHES):
                    if name == "iteration":
                        x = b[i + 1]
                        batch = dict(x, sent=(x["input_ids"], x["input_mask"], x["segment_ids"]))
                        train_iteration(m, o, t.bce, batch, sigma=1.0, order="vqa", branch=br, clip=5.0, train_log=log)
                    elif name == "bare_eager":
                        x = b[i + 1]
                        sent = (x["input_ids"], x["input_mask"], x["segment_ids"])
                        loss, _ = plain_pass(m, o, t.bce, x["feats"], x["boxes"], sent, x["target"], advance=True)
                        floats.append(dict(kind="plain", loss=np.float32(float(loss))))
                        loss, _, ex = ggm_pass(m, o, t.bce, x["feats"], x["boxes"], sent, x["target"], x["adj_true"], br, 1.0,
                                               8.0, advance=True)
                        floats.append(dict(kind=br, loss=np.float32(float(loss)),
                                           terms={k: (np.float32(float(s.t)), s.c) for k, s in ex.items()}))
                    elif name == "bare":
                        t.load_batch(b[i + 1])
                        for kind in ("plain", br):
                            loss, _, total = t.run_pass(kind)
                            floats.append(dict(kind=kind, loss=np.float32(float(loss)), total=np.float32(float(total))))
                    else:
                        t.load_batch(b[i + 1])
                        t.iteration(br)
            finally:
                torch.cuda.set_sync_debug_mode("default")
            if name == "logged":
                out["syncs_before_read"] = list(syncs)
                syncs.clear()
                out["rec"] = log.read()
                out["syncs_of_read"] = list(syncs)
                mp.undo()
                out["average_loss"] = log.average_loss(B)
        finally:
            ops.call = real_call
            mp.undo()
        torch.cuda.synchronize()
        out[name] = dict(trainer=t, log=log, seen=seen, floats=floats, state=_state(m))
    return out


def _sync_mode_raises():
    """does torch.cuda.set_sync_debug_mode("error") catch a deliberate ``.item()`` on this build?"""
    t = torch.ones(1, device=DEV)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        t.item()
        return False
    except RuntimeError:
        return True
    finally:
        torch.cuda.set_sync_debug_mode("default")


def _count(mp, owner, name, calls, is_dev):
    real = getattr(owner, name)

    def wrapped(self, *a, **k):
        if is_dev(self):
            calls.append(name)
        return real(self, *a, **k)
    mp.setattr(owner, name, wrapped)


def test_the_log_observes_only(runs):
    a, b = runs["logged"]["state"], runs["bare"]["state"]
    assert sorted(a) == sorted(b)
    for k in a:  # parameters, Adam moments, (bf16 weights,) step counters, schedule values, the RNG words
        assert torch.equal(a[k], b[k]), k
    assert a["steps"].max().item() == WARM_PASSES + 6


def test_the_log_holds_what_the_passes_return(runs):
    """``LR_SCALE``: the record with step k holds warmup_linear((k - 1) / t_total, warmup) -- the value the pass's own
    update multiplied its lr by (``vqa.vqacpv2.log_pass``), evaluated in fp32 on the device: within 1 ulp of the host's"""
    from xggm_amd.engine import TrainLog as L
    from xggm_amd.lxrt.optimization import warmup_linear
    rec, passes, eager = runs["rec"], runs["bare"]["floats"], runs["bare_eager"]["floats"]
    assert len(passes) == 6 == len(eager) == int(rec["cursor"]) and int(rec["first_bad"]) == -1
    # the eager un-logged run IS the captured un-logged run, bit for bit: its loss terms are that run's
    for p, e in zip(passes, eager):
        assert p["kind"] == e["kind"] and p["loss"].view(np.int32) == e["loss"].view(np.int32)
    kept = list(range(2, 6))  # six records in a ring of four
    assert rec["values"].shape == (4, COLS) and rec["counts"].tolist() == [3, 2, 1, 0]
    assert rec["kinds"].tolist() == [{"plain": L.PLAIN, "rel": L.REL, "node": L.NODE}[passes[r]["kind"]] for r in kept]
    assert rec["steps"].tolist() == [WARM_PASSES + r + 1 for r in kept]
    v = rec["values"].numpy()
    for j, r in enumerate(kept):
        p, e = passes[r], eager[r]
        plain = p["kind"] == "plain"
        assert rec["present"][j].tolist() == [True, True, not plain, not plain, True, True, False, False]
        assert v[j, L.LOSS].view(np.int32) == p["loss"].view(np.int32)
        assert v[j, L.GRAD_NORM].view(np.int32) == p["total"].view(np.int32)
        if plain:
            assert v[j, L.BCE].view(np.int32) == p["loss"].view(np.int32) and v[j, L.KL] == 0 and v[j, L.DSM] == 0
        else:
            for col, key in ((L.BCE, "bce"), (L.KL, "d_loss"), (L.DSM, "loss_grad")):
                slot, c = e["terms"][key]
                want = np.float32(slot) * np.float32(1 / c)
                assert v[j, col].view(np.int32) == want.view(np.int32), (r, key)
        assert v[j, 6] == 0 and v[j, 7] == 0
        step = int(rec["steps"][j])
        want = np.float32(warmup_linear((step - 1) / T_TOTAL, WARMUP))
        ulps = abs(int(v[j, L.LR_SCALE].view(np.int32)) - int(want.view(np.int32)))
        assert ulps <= 1, (step, float(v[j, L.LR_SCALE]), float(want))
    # Train/average_loss: every plain pass since reset(), not only the retained ones
    plain_losses = [p["loss"] for p in passes if p["kind"] == "plain"]
    s = np.float64(0)
    for x in plain_losses:
        s = s + np.float64(x)
    assert float(rec["sums"][L.PLAIN, L.LOSS]) == float(s)
    assert runs["average_loss"] == float(s) / B / 3
    assert abs(runs["average_loss"] - float(np.mean(np.float64(plain_losses))) / B) <= 1e-15 * abs(runs["average_loss"])
    # the sums of the other columns cover all six records too
    assert float(rec["sums"][L.REL, L.GRAD_NORM]) == float(np.float64(passes[1]["total"]) + np.float64(passes[5]["total"]))


def test_captured_and_eager_logs_agree(runs):
    cap = runs["logged"]
    for name in ("eager", "iteration"):
        assert torch.equal(cap["log"].buf, runs[name]["log"].buf), name
        for k in cap["state"]:
            assert torch.equal(cap["state"][k], runs[name]["state"][k]), (name, k)


def test_no_launch_is_added_without_a_log(runs):
    """the launches Python issued while the trainers were built and run (warm-up passes and captures: a replay runs no
    Python): with a log one append per pass, without one exactly the others"""
    logged, bare = collections.Counter(runs["logged"]["seen"]), collections.Counter(runs["bare"]["seen"])
    assert "xggm_train_log_append" not in bare and bare["xggm_bce_fwd"] > 0
    assert logged - bare == {"xggm_train_log_append": 2 * WARM_PASSES} and not bare - logged
    # the eager twins: one append per pass (3 warm-up + 6 logged), nothing else differs
    eager, bare_eager = collections.Counter(runs["eager"]["seen"]), collections.Counter(runs["bare_eager"]["seen"])
    assert eager - bare_eager == {"xggm_train_log_append": WARM_PASSES + 6} and not bare_eager - eager
    assert collections.Counter(runs["iteration"]["seen"]) - bare_eager == {"xggm_train_log_append": 6}


def test_logged_iterations_never_synchronise_and_read_does_once(runs):
    assert runs["syncs_before_read"] == [], runs["syncs_before_read"]
    assert runs["syncs_of_read"] == ["synchronize"], runs["syncs_of_read"]
