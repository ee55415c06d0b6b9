"""The device-resident answer log: xggm_answer_pick_f32 against torch.max on the CPU (index for index), the appended
scores and their ordered fp64 sum, the append / rows / overflow protocol, bit-equality of eager launches, graph replays
and launches beside foreign work, and the two users -- the logging CapturedPredictor under ``predict`` and the
CapturedTrainer's train score."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from xggm_amd import synth  # noqa: E402
from helpers import batch_tensors  # noqa: E402

DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SHAPES = [(1, 1), (3, 7), (5, 2274), (33, 3129), (130, 29)]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _pick(logits, target=None, rows=None, log=None):
    from xggm_amd import ops
    from xggm_amd.engine import AnswerLog
    if log is None:
        log = AnswerLog(logits.shape[0], DEV, with_scores=target is not None)
    ops.answer_pick(logits, log, target=target, rows=rows)
    return log


def _special_rows(A, seed):
    """rows built to break a (value, index) reduction; the expectation is torch.max on the CPU, and where the issue
    names an index it is asserted as well.  -> (rows [S, A], {row: index named by the construction})"""
    g = torch.Generator().manual_seed(seed)
    rows, named = [], {}

    def add(r, idx=None):
        if idx is not None:
            named[len(rows)] = idx
        rows.append(r)

    base = lambda: torch.randn(A, generator=g).clamp_(max=3.0)  # noqa: E731
    # equal maxima straddling a thread's vector, a lane pair, a wave and the workgroup's stride
    for i in (3, 63, 255, 1023):
        if i + 1 < A:
            r = base()
            r[i] = r[i + 1] = 10.0
            add(r, i)
    r = base(); r[0] = 11.0; add(r, 0)  # noqa: E702
    r = base(); r[A - 1] = 11.0; add(r, A - 1)  # noqa: E702
    add(torch.full((A,), 0.5), 0)
    add(torch.full((A,), float("-inf")), 0)
    add(torch.full((A,), float("inf")), 0)
    r = base(); r[0] = float("nan"); add(r, 0)  # noqa: E702
    if A >= 3:
        r = base(); r[A // 3] = r[2 * A // 3 if 2 * A // 3 > A // 3 else A - 1] = float("inf"); add(r, A // 3)  # noqa: E702
        r = base(); r[A // 2 - 1] = 100.0; r[A // 2] = float("nan"); add(r, A // 2)  # noqa: E702  NaN after a larger value
        r = base(); r[A // 2] = float("nan"); r[A - 1] = float("nan"); r[0] = float("inf"); add(r, A // 2)  # noqa: E702
        r = torch.full((A,), -1.0); r[1] = -0.0; r[A - 1] = 0.0; add(r, 1)  # noqa: E702  -0 == +0: the first one
        r = torch.full((A,), -1e-42); r[A - 2] = -1e-45; add(r, A - 2)  # noqa: E702  denormals are values, not zeros
    return torch.stack(rows), named


# ----------------------------------------------------------------------------- 1. arg-max == torch on the CPU
def test_reference_semantics_of_the_issue_hold_on_this_torch():
    x = torch.tensor([[1, 3, 3, 2], [float("nan"), 5, float("nan"), 1], [2, float("nan"), 9, float("nan")],
                      [float("-inf")] * 4, [float("inf"), 1, float("inf"), 0]])
    assert x.max(1)[1].tolist() == [1, 0, 1, 0, 0]
    assert _pick(x.to(DEV)).read()[0].tolist() == [1, 0, 1, 0, 0]


@pytest.mark.parametrize("B,A", SHAPES)
def test_argmax_equals_torch_cpu(B, A):
    """random rows at the issue's shapes (A below one wave and one vector; A = 2 mod 4: odd rows 8-byte aligned; A = 1
    mod 4: rows 4-byte aligned; more rows than the 128 workgroups), the constructed rows, and a row_stride > A view"""
    g = torch.Generator().manual_seed(100 + A)
    x = torch.randn(B, A, generator=g)
    sp, named = _special_rows(A, 7 + A)
    for name, t in (("random", x), ("special", sp)):
        want = t.max(1)[1]
        if name == "special":
            for r, idx in named.items():
                assert int(want[r]) == idx, (r, idx)
        labels, scores, _, n = _pick(t.to(DEV)).read()
        assert n == t.shape[0] and scores is None
        assert torch.equal(labels, want), (name, (labels != want).nonzero().flatten().tolist())
        # rows of a wider buffer: every row starts at another alignment
        wide = torch.full((t.shape[0], A + 5), float("inf"))
        wide[:, :A] = t
        assert torch.equal(_pick(wide.to(DEV)[:, :A]).read()[0], want), name
    # an offset view: the first row itself starts 4 bytes past a 16-byte boundary
    flat = torch.zeros(B * A + 1)
    flat[1:] = x.flatten()
    assert torch.equal(_pick(flat.to(DEV)[1:].view(B, A)).read()[0], x.max(1)[1])


# ----------------------------------------------------------------------------- 2. scores and their sum
def test_scores_and_ordered_fp64_sum():
    """scores == target[b, label] bit for bit; the sum is the sequential fp64 sum of those fp32 scores in row order
    across the appends -- magnitudes over many binades, so that any other order or an fp32 accumulator shows"""
    from xggm_amd.engine import AnswerLog
    B, A = 130, 29
    g = torch.Generator().manual_seed(5)
    log = AnswerLog(3 * B, DEV)
    want_l, want_s = [], []
    for k in range(3):
        x = torch.randn(B, A, generator=g)
        t = torch.exp(torch.randn(B, A, generator=g) * 8.0)
        _pick(x.to(DEV), t.to(DEV), log=log)
        want_l.append(x.max(1)[1])
        want_s.append(t.gather(1, want_l[-1][:, None])[:, 0])
    labels, scores, total, n = log.read()
    want_l, want_s = torch.cat(want_l), torch.cat(want_s)
    assert n == 3 * B and torch.equal(labels, want_l)
    assert torch.equal(scores.view(torch.int32), want_s.view(torch.int32))
    seq = np.cumsum(want_s.numpy().astype(np.float64), dtype=np.float64)[-1]
    assert seq != np.cumsum(want_s.numpy()[::-1].astype(np.float64), dtype=np.float64)[-1]  # the order is visible
    assert total == seq, (total, seq)
    assert log.score() == seq / n


def test_score_equals_the_evaluator_on_the_dataset_golden():
    """``score()`` against ``VQAEvaluator.evaluate`` of the decoded dict on the synthetic dataset golden, to 1e-6 (the
    evaluator adds the JSON's doubles, the target holds their fp32 roundings)"""
    from xggm_amd.answers import to_quesid2ans
    from xggm_amd.engine import AnswerLog
    from xggm_amd.vqa.vqacpv2_data import VQAEvaluator
    gd = json.load(open(os.path.join(GOLDEN, "dataset.json")))
    label2ans, data = gd["label2ans"], gd["vqa"]

    class DSet:
        id2datum = {d["question_id"]: d for d in data}
        ans2label = {a: i for i, a in enumerate(label2ans)}

    n, A = len(data), len(label2ans)
    target = torch.zeros(n, A)
    logits = torch.randn(n, A, generator=torch.Generator().manual_seed(2))
    for i, d in enumerate(data):
        for l, s in zip(d["label"], d["score"]):
            target[i, l] = s
        logits[i, DSet.ans2label[gd["pred_vqa"][str(d["question_id"])]]] = 9.0
    log = AnswerLog(n, DEV)
    _pick(logits.to(DEV), target.to(DEV), log=log)
    quesid2ans = to_quesid2ans([d["question_id"] for d in data], log.read()[0], label2ans)
    assert quesid2ans == {int(k): v for k, v in gd["pred_vqa"].items()}
    want = VQAEvaluator(DSet).evaluate(quesid2ans)
    assert 0.0 < want < 1.0 and abs(log.score() - want) <= 1e-6


# ----------------------------------------------------------------------------- 3. append, rows, overflow
def test_append_rows_and_overflow():
    from xggm_amd import ops
    from xggm_amd.engine import AnswerLog
    B, A, b = 9, 37, 4
    g = torch.Generator().manual_seed(8)
    xs = [torch.randn(B, A, generator=g) for _ in range(4)]
    ts = [torch.rand(B, A, generator=g) for _ in range(4)]
    xs[2][b:] += 100.0  # the padded tail holds larger logits than any kept row
    log = AnswerLog(2 * B + b + B - 1, DEV)  # one short of a fourth full batch
    rows = torch.tensor([B], dtype=torch.int32, device=DEV)
    for k, n in enumerate((B, B, b)):
        rows.fill_(n)
        _pick(xs[k].to(DEV), ts[k].to(DEV), rows=rows, log=log)
    labels, scores, total, n = log.read()
    want_l = torch.cat([xs[0].max(1)[1], xs[1].max(1)[1], xs[2][:b].max(1)[1]])
    want_s = torch.cat([t.gather(1, x.max(1)[1][:, None])[:, 0] for x, t in zip(xs[:3], ts[:3])])[:2 * B + b]
    assert n == 2 * B + b and torch.equal(labels, want_l) and torch.equal(scores, want_s)
    assert total == np.cumsum(want_s.numpy().astype(np.float64))[-1]
    assert int(log.flags[0]) == 0
    # rows is clamped to [0, B]: a stale larger word can never read or log past the batch
    before = log.buf.clone()
    rows.fill_(0)
    _pick(xs[3].to(DEV), ts[3].to(DEV), rows=rows, log=log)
    assert torch.equal(log.buf, before)
    # a fourth append that does not fit: nothing moves but the flag
    rows.fill_(B)
    for refused in (1, 2):
        _pick(xs[3].to(DEV), ts[3].to(DEV), rows=rows, log=log)
        after = log.buf.clone()
        assert int(after[2:3].view(torch.int32)[0]) == 1 + 2 * refused
        after[2] = before[2]
        assert torch.equal(after, before)
    with pytest.raises(RuntimeError, match=r"capacity %d, %d samples logged, 2 append" % (log.capacity, 2 * B + b)):
        log.read()
    with pytest.raises(RuntimeError, match="overflow"):
        log.score()
    log.reset()
    assert log.read()[3] == 0 and int(log.flags[0]) == 0
    rows.fill_(b)
    _pick(xs[3].to(DEV), rows=rows, log=log)  # a log with scores also takes an append without a target
    assert torch.equal(log.read()[0], xs[3][:b].max(1)[1])
    # the host mirror refuses at once what the device would refuse later
    log.note(log.capacity - 1)
    with pytest.raises(RuntimeError, match="overflow"):
        log.note(2)
    # bad arguments: refused on the host, the log untouched
    snap = log.buf.clone()
    x = xs[0].to(DEV)
    with pytest.raises(ValueError):
        ops.answer_pick(x, log, target=ts[0][:, :A - 1].to(DEV))
    with pytest.raises(ValueError):
        ops.answer_pick(x, AnswerLog(B, DEV, with_scores=False), target=ts[0].to(DEV))
    with pytest.raises(RuntimeError):
        ops.answer_pick(x.t(), log)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.answer_pick(xs[0], log)
    with pytest.raises(TypeError):
        ops.answer_pick(x.double(), log)
    assert torch.equal(log.buf, snap)


# ----------------------------------------------------------------------------- 4. determinism
def test_same_bits_eager_replayed_and_beside_foreign_work():
    from xggm_amd.engine import AnswerLog
    B, A = 130, 2274
    g = torch.Generator().manual_seed(9)
    xs = [torch.randn(B, A, generator=g).to(DEV) for _ in range(3)]
    ts = [torch.exp(torch.randn(B, A, generator=g) * 8.0).to(DEV) for _ in range(3)]
    rows = [torch.tensor([n], dtype=torch.int32, device=DEV) for n in (B, B, 77)]

    def appends(log):
        for x, t, r in zip(xs, ts, rows):
            _pick(x, t, rows=r, log=log)

    eager = AnswerLog(3 * B, DEV)
    appends(eager)
    torch.cuda.synchronize()
    # replayed from a captured graph (twice, with a reset between: the second replay must land on the same bits)
    replayed = AnswerLog(3 * B, DEV)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        appends(replayed)
    for _ in range(2):
        replayed.reset()
        graph.replay()
    # beside foreign work: the appends on a second stream while the first one multiplies matrices
    beside = AnswerLog(3 * B, DEV)
    side = torch.cuda.Stream()
    a = torch.randn(2048, 2048, device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    for _ in range(8):
        a = (a @ a).clamp_(-1.0, 1.0)
    with torch.cuda.stream(side):
        appends(beside)
    for _ in range(8):
        a = (a @ a).clamp_(-1.0, 1.0)
    torch.cuda.synchronize()
    assert int(eager.cursor[0]) == 2 * B + 77
    assert torch.equal(eager.buf, replayed.buf) and torch.equal(eager.buf, beside.buf)
    want = torch.cat([x[:int(r[0])].cpu().max(1)[1] for x, r in zip(xs, rows)])
    assert torch.equal(eager.read()[0], want)


# ----------------------------------------------------------------------------- the tiny model (local twin of the engine tests')
def _tiny(seed_w, seed_rt, A=29, layers=(1, 1, 1)):
    from oracle import shapes
    from xggm_amd import param
    from xggm_amd.lxrt.modeling import BertConfig, VISUAL_CONFIG
    from xggm_amd.vqa.vqacpv2 import make_optimizer
    from xggm_amd.vqa.vqacpv2_model import VQAModel
    cfg = dict(shapes.TINY, l_layers=layers[0], x_layers=layers[1], r_layers=layers[2])
    VISUAL_CONFIG.set_visual_dims(cfg["feat_dim"], 4)
    a = param.parse_args(["--llayers", str(cfg["l_layers"]), "--xlayers", str(cfg["x_layers"]), "--rlayers",
                          str(cfg["r_layers"])])
    bc = BertConfig(cfg["vocab"], hidden_size=cfg["hidden"], num_attention_heads=cfg["heads"],
                    intermediate_size=cfg["inter"], max_position_embeddings=cfg["max_pos"])
    m = VQAModel(A, gnn="GCN", n_layers=2, args=a, config=bc, compute_dtype=torch.bfloat16)
    m.load_state_dict({k: torch.from_numpy(synth.seeded_param(k, v.shape, seed_w)) for k, v in m.state_dict().items()})
    m = m.to(DEV)
    m.seed = seed_rt
    return cfg, m, make_optimizer(m, 1e-4, 40)


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


# ----------------------------------------------------------------------------- 5. predictor
def test_logging_predictor_sweeps_without_a_host_sync(monkeypatch):
    """``predict`` with a logging predictor == with a plain CapturedPredictor == eager, on a 21-sample loader at batch 8
    (8, 8, 5: the padded rows of the last replay never enter the log), and between the first and the last batch the
    host is never synchronised.  Which check is in force is decided on the spot and printed: torch's sync debug mode
    ("error") where a deliberate ``.item()`` raises under it, else a count of the synchronising tensor methods and
    ``synchronize`` calls on CUDA tensors / streams."""
    from xggm_amd.engine import AnswerLog, CapturedPredictor
    from xggm_amd.vqa import vqacpv2
    from xggm_amd.vqa.vqacpv2 import predict
    A, n, bs = 29, 21, 8
    cfg, m, _ = _tiny(14, 3, A=A)
    bc = batch_tensors(synth.vqa_batch(n, A=A, F=cfg["feat_dim"], vocab=cfg["vocab"], seed=14))

    class DSet:
        label2ans = ["ans%d" % i for i in range(A)]

    class Evaluator:
        def dump_result(self, quesid2ans, path):
            self.dumped = (dict(quesid2ans), path)

    def loader():
        for lo in range(0, n, bs):
            hi = min(lo + bs, n)
            sent = tuple(bc[k][lo:hi] for k in ("input_ids", "input_mask", "segment_ids"))
            yield torch.arange(1000 + lo, 1000 + hi), bc["feats"][lo:hi], bc["boxes"][lo:hi], sent, bc["target"][lo:hi]

    ev = Evaluator()
    eager = predict(m, (DSet, loader(), ev))
    plain = predict(m, (DSet, loader(), ev), predictor=CapturedPredictor(m, bs))
    assert sorted(eager) == list(range(1000, 1000 + n)) and plain == eager

    log = AnswerLog(n, DEV, with_scores=False)
    pred = CapturedPredictor(m, bs, log=log)
    assert m.training and log.read()[3] == 0
    use_mode = _sync_mode_raises()
    print("sync check in force:", "torch.cuda.set_sync_debug_mode('error')" if use_mode else "call counting")
    calls = []
    real_read = AnswerLog.read

    def read(self):  # the sweep's one read-back: the check ends here
        if use_mode:
            torch.cuda.set_sync_debug_mode("default")
        calls.append("read")
        return real_read(self)

    monkeypatch.setattr(AnswerLog, "read", read)
    if not use_mode:
        def spy(owner, name, is_dev):
            real = getattr(owner, name)

            def wrapped(self, *a, **k):
                if "read" not in calls and is_dev(self):
                    calls.append(name)
                return real(self, *a, **k)
            monkeypatch.setattr(owner, name, wrapped)
        for name in ("cpu", "item", "tolist", "numpy"):
            spy(torch.Tensor, name, lambda t: t.is_cuda)
        for owner in (torch.cuda.Stream, torch.cuda.Event):
            spy(owner, "synchronize", lambda s: True)
        real_sync = torch.cuda.synchronize
        monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: (calls.append("synchronize"), real_sync(*a, **k))[1])
    torch.cuda.synchronize()
    calls.clear()
    try:
        if use_mode:
            torch.cuda.set_sync_debug_mode("error")
        logged = predict(m, (DSet, loader(), ev), dump="out.json", predictor=pred)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    monkeypatch.undo()
    assert calls == ["read"], calls
    assert logged == eager and ev.dumped == (eager, "out.json") and m.training
    # a second sweep starts from an empty log; __call__ keeps working and returns views of the newest labels
    assert predict(m, (DSet, loader(), ev), predictor=pred) == eager
    log.reset()
    sent = tuple(bc[k][:5] for k in ("input_ids", "input_mask", "segment_ids"))
    label, logit = pred(bc["feats"][:5].to(DEV), bc["boxes"][:5].to(DEV), sent)
    assert label.shape == (5,) and torch.equal(label.cpu(), logit.cpu().max(1)[1])
    assert [DSet.label2ans[l] for l in label.tolist()] == [eager[1000 + i] for i in range(5)]
    with pytest.raises(ValueError):
        pred.push(bc["feats"][:9].to(DEV), bc["boxes"][:9].to(DEV), tuple(bc[k][:9] for k in
                                                                           ("input_ids", "input_mask", "segment_ids")))
    # the eager predictor logs the same answers
    log2 = AnswerLog(n, DEV, with_scores=False)
    assert predict(m, (DSet, loader(), ev), predictor=CapturedPredictor(m, bs, use_graph=False, log=log2)) == eager


# ----------------------------------------------------------------------------- 6. trainer
@pytest.fixture(scope="module")
def trained():
    """three iterations on three different batches: a captured trainer with a log, its twin without one (under a spy on
    ``ops.call``), and an eager trainer with a log that runs the constructor's warm-up passes by hand"""
    from xggm_amd import ops
    from xggm_amd.engine import AnswerLog, CapturedTrainer
    from xggm_amd.runtime import runtime_of
    B, A = 4, 29
    out = {}
    real_call = ops.call
    for name in ("logged", "bare", "eager"):
        cfg, m, o = _tiny(5, 11, A=A)
        b = [batch_tensors(synth.vqa_batch(B, A=A, F=cfg["feat_dim"], vocab=cfg["vocab"], seed=s), DEV) for s in (3, 4, 5, 6)]
        log = AnswerLog(3 * B, DEV) if name != "bare" else None
        seen = []

        def spy(fn, *a, _seen=seen):
            _seen.append(fn)
            return real_call(fn, *a)

        ops.call = spy
        try:
            t = CapturedTrainer(m, o, b[0], sigma=1.0, warmup_iters=1, use_graph=name != "eager", answer_log=log)
            if name == "eager":
                for kind in ("plain", "rel", "node"):
                    t._eager_pass(kind)
                log.reset()
            logits = []
            for i, br in enumerate(("rel", "node", "rel")):
                t.load_batch(b[i + 1])
                (_, logit, _), _ = t.iteration(br)
                logits.append(logit.float().cpu().clone())  # the comparison's copy; the log itself is never read here
        finally:
            ops.call = real_call
        arena, rt = runtime_of(m).arena, runtime_of(m)
        out[name] = dict(trainer=t, log=log, seen=seen, logits=logits, targets=[x["target"].cpu() for x in b[1:]],
                         state={k: getattr(arena, k).clone() for k in ("params", "grads", "m", "v", "shadow")},
                         steps=arena.steps.tolist(), rng=rt.rng.tolist())
    return out


def test_trainer_log_holds_the_plain_answers(trained):
    r = trained["logged"]
    labels, scores = r["trainer"].answers()
    want_l = torch.cat([x.max(1)[1] for x in r["logits"]])
    want_s = torch.cat([t.gather(1, x.max(1)[1][:, None])[:, 0] for x, t in zip(r["logits"], r["targets"])])
    assert labels.shape == (12,) and torch.equal(labels, want_l) and torch.equal(scores, want_s)
    assert r["trainer"].train_score() == np.cumsum(want_s.numpy().astype(np.float64))[-1] / 12
    assert abs(r["trainer"].train_score() - float(want_s.double().mean())) < 1e-12
    assert "xggm_answer_pick_f32" in r["seen"]


def test_trainer_log_observes_and_changes_nothing(trained):
    a, b = trained["logged"], trained["bare"]
    for k in a["state"]:
        assert torch.equal(a["state"][k], b["state"][k]), k
    assert a["steps"] == b["steps"] and a["rng"] == b["rng"]
    assert all(torch.equal(x, y) for x, y in zip(a["logits"], b["logits"]))
    # without a log the new entry point is never called (and the spy did see the step's launches)
    assert "xggm_answer_pick_f32" not in b["seen"] and "xggm_bce_fwd" in b["seen"]
    with pytest.raises(RuntimeError, match="answer_log"):
        b["trainer"].train_score()


def test_eager_trainer_logs_the_same_bits(trained):
    a, e = trained["logged"], trained["eager"]
    assert torch.equal(a["log"].buf, e["log"].buf)
    for k in a["state"]:
        assert torch.equal(a["state"][k], e["state"][k]), k
