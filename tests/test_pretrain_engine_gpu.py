"""The captured pre-training step (``engine.CapturedPretrainer``) and the driver behind the reference's interface
(``pretrain.lxmert_pretrain.LXMERT``) on the tiny 2-head LXRTPretraining of tests/test_pretrain_model_gpu.py, dropout on:
captured, eager, hand-written and restored runs give the same bits; logs observe only; validation changes nothing; an
overflowing masked-LM selection is named; the driver's per-batch and per-epoch interfaces."""
import json
import os
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import GOLDEN, load_golden  # noqa: E402
from test_pretrain_cpu import _tiny_model, _restore_visual_config  # noqa: E402

DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
K = 3  # answer keys per example
SID = 0x70726500
# Philox seed of every model here (``model.seed``, read when its runtime is made).  Rows 0 and 1 of a batch carry answer labels;
# a step in which the swap unmatches both has no QA label left and its QA loss is 0 / 0 = NaN, as the reference's
# CrossEntropyLoss(ignore_index=-1) gives for such a batch -- faithful, but bit comparisons and printed numbers want finite
# values.  With this seed one of the two stays matched in each of the first eight steps (``_seed_keeps_a_label``).
SEED = 7


def _seed_keeps_a_label():
    import pretrain_mask_ref as R
    us = [R.philox_uniform(SEED, off, SID + 5, 3) for off in range(8)]
    return all(max(float(u[0]), float(u[1])) >= 0.5 for u in us) and sum(int((u < 0.5).sum()) for u in us[:3]) >= 2


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(autouse=True)
def _visual_config():
    """every model of a test is built by ``_tiny_model``, which edits the global VISUAL_CONFIG: put it back afterwards"""
    from xggm_amd.lxrt import modeling as M
    saved = dict(M.VISUAL_CONFIG.__dict__)
    yield
    _restore_visual_config(saved)


def _cfg():
    return json.loads(str(load_golden("pretrain")["meta_json"]))


def clean_batch(seed, B=None):
    """a CLEAN batch at the fixture's shapes: three examples over two images, all matched, every answer case"""
    from xggm_amd import synth
    from xggm_amd.pretrain.lxmert_pretrain import pack_labels
    meta = _cfg()
    c = meta["cfg"]
    B = B or c["B"]
    x = synth.pretrain_case(B, c["T"], c["O"], c["F"], c["vocab"], c["n_obj"], c["n_attr"], c["n_ans"], seed=seed)
    lab, sc = pack_labels(([{3: 0.3, 7: 0.6, 11: 1.0}, {5: 1.0}, None] * B)[:B], K)
    b = dict(input_ids=x["input_ids"], input_mask=x["input_mask"], segment_ids=x["segment_ids"], feats=x["feats"], boxes=x["boxes"],
             obj_labels=x["obj_label"], obj_confs=x["obj_conf"], attr_labels=x["attr_label"], attr_confs=x["attr_conf"],
             is_matched=np.ones(B, dtype=np.int64), img_ids=(np.arange(B) % 2).astype(np.int64))
    b = {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in b.items()}
    b["label_ids"], b["label_scores"] = lab.to(DEV), sc.to(DEV)
    return b


def features(**kw):
    from xggm_amd.pretrain.lxmert_pretrain import DeviceFeatures
    c = _cfg()["cfg"]
    kw = dict(dict(word_mask_rate=0.5, obj_mask_rate=0.15, vocab_size=c["vocab"], mask_id=103, max_labels=K, match_rate=0.5), **kw)
    return DeviceFeatures(**kw)


def setup(dt, use_graph=True, logs=True, **model_kw):
    """-> (model, optim, trainer): the seeded tiny model in training mode (dropout on), BertAdam, a CapturedPretrainer on
    clean_batch(3) with a swap"""
    from xggm_amd.engine import AnswerLog, CapturedPretrainer, TrainLog
    from xggm_amd.lxrt.optimization import BertAdam
    model, *_ = _tiny_model("full", compute_dtype=dt, **model_kw)
    model = model.to(DEV).train()
    model.seed = SEED
    assert _seed_keeps_a_label()
    optim = BertAdam(list(model.parameters()), lr=1e-3, warmup=0.1, t_total=20)
    kw = dict(train_log=TrainLog(8, DEV), valid_log=TrainLog(8, DEV), answer_log=AnswerLog(64, DEV, with_scores=False)) if logs else {}
    tr = CapturedPretrainer(model, optim, clean_batch(3), features(), use_graph=use_graph, warmup_iters=1, **kw)
    return model, optim, tr


def state(model):
    """every parameter, the optimiser moments and counters, the Philox state"""
    from xggm_amd.runtime import runtime_of
    rt = runtime_of(model)
    torch.cuda.synchronize()
    out = {"p." + k: v.detach().clone() for k, v in model.named_parameters()}
    out.update(m=rt.arena.m.clone(), v=rt.arena.v.clone(), steps=rt.arena.steps.clone(), rng=rt.rng.clone())
    return out


def same(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def same_records(a, b):
    for k in ("values", "steps", "kinds", "present", "sums", "counts"):
        assert torch.equal(a[k], b[k]), k
    assert int(a["cursor"]) == int(b["cursor"]) and int(a["first_bad"]) == int(b["first_bad"])


BATCHES = (3, 4, 6)  # seeds of the batches of the three steps


@pytest.mark.parametrize("dt", [F32, BF16])
def test_captured_steps_equal_eager_steps(dt):
    """three replayed steps against three eager steps of the same calls from the same seed: every column of every record,
    every parameter, the moments, the counters and rng"""
    from xggm_amd import trainlog as T
    runs = []
    for use_graph in (True, False):
        model, optim, tr = setup(dt, use_graph)
        start = state(model)
        for s in BATCHES:
            tr.step(clean_batch(s))
        tr.check()
        labels, _, _, n = tr.answer_log.read()
        runs.append((tr.train_log.read(), state(model), labels, n, start))
    (rec, st, labels, n, start), (rec_e, st_e, labels_e, n_e, start_e) = runs
    same(start, start_e)  # the warm-up and the capture left nothing behind
    assert int(start["steps"].max()) == 0 and int(start["rng"][1]) == 0 and not bool(start["m"].any())
    same_records(rec, rec_e)
    same(st, st_e)
    assert n == n_e == 9 and torch.equal(labels, labels_e)
    assert int(rec["cursor"]) == 3 and rec["kinds"].tolist() == [T.PRETRAIN] * 3 and rec["steps"].tolist() == [1, 2, 3]
    assert bool(rec["present"].all()) and bool(torch.isfinite(rec["values"]).all())  # all six tasks are on: LOSS, six terms, norm
    assert int(st["rng"][1]) == 3 and int(rec["first_bad"]) == -1
    assert not torch.equal(rec["values"][0], rec["values"][1])
    assert not torch.equal(st["p.cls.predictions.bias"], start["p.cls.predictions.bias"])  # it trained
    total = rec["values"][:, T.PT_MASK_LM:T.PT_QA + 1].sum(1)
    assert torch.allclose(total, rec["values"][:, T.LOSS], rtol=1e-5)  # LOSS is the sum of the six terms


@pytest.mark.parametrize("dt", [F32, BF16])
def test_eager_engine_equals_the_hand_written_sequence(dt):
    """use_graph=False against DeviceFeatures -> forward -> runtime.backward -> clip_and_step(..., advance=True) by hand"""
    from xggm_amd.engine import CapturedPretrainer
    from xggm_amd.runtime import runtime_of
    from xggm_amd.vqa.vqacpv2 import clip_and_step
    model, optim, tr = setup(dt, use_graph=False, logs=False)
    got = []
    for s in BATCHES:
        loss, losses, ans, norm = tr.step(clean_batch(s))
        got.append((loss.clone(), losses.clone(), ans.clone(), norm.clone()))
    model2, optim2, _ = setup(dt, use_graph=False, logs=False)
    feat, rt = features(), runtime_of(model2)
    for s, g in zip(BATCHES, got):
        b = clean_batch(s)
        total, losses, ans = model2(*feat(*[b[k] for k in CapturedPretrainer.KEYS], rt.rng, img_ids=b["img_ids"]))
        rt.backward(total)
        norm = clip_and_step(model2, optim2, 1.0, advance=True)
        assert torch.equal(total.detach(), g[0]) and torch.equal(losses, g[1]) and torch.equal(ans, g[2]) and torch.equal(norm, g[3])
    same(state(model), state(model2))


@pytest.mark.parametrize("dt", [F32, BF16])
def test_logs_observe_only(dt):
    """train_log, valid_log and answer_log attached against none of them: the parameters are bit-identical"""
    states = []
    for logs in (True, False):
        model, optim, tr = setup(dt, logs=logs)
        for s in BATCHES[:2]:
            tr.step(clean_batch(s))
            tr.valid_step()
        states.append(state(model))
    same(*states)


def test_valid_step_changes_no_state_and_logs_to_valid_log_only():
    from xggm_amd import trainlog as T
    model, optim, tr = setup(BF16)
    tr.step(clean_batch(3))
    before = state(model)
    cursor = int(tr.train_log.read()["cursor"])
    for s in (4, 6):
        out = tr.valid_step(clean_batch(s))
        assert out[3] is None
    after = state(model)
    rng0, rng1 = before.pop("rng"), after.pop("rng")
    same(before, after)  # parameters, moments, step counters
    assert int(rng1[1]) == int(rng0[1]) + 2  # the draws moved on
    assert int(tr.train_log.read()["cursor"]) == cursor == 1
    rec = tr.valid_log.read()
    assert int(rec["cursor"]) == 2 and rec["kinds"].tolist() == [T.PRETRAIN] * 2 and rec["steps"].tolist() == [1, 1]
    want = [True] * 7 + [False]  # no backward: no gradient norm
    assert rec["present"].tolist() == [want, want] and bool(torch.isfinite(rec["values"]).all())
    assert not torch.equal(rec["values"][0], rec["values"][1])
    labels, _, _, n = tr.answer_log.read()
    assert n == 9  # one training step and two validation steps of three examples
    assert model.training


def test_overflow_is_named_by_check():
    """mlm_capacity one slot short of a LATER step's labelled rows (the steps before it fit): check() raises and names that
    step, its record's Mask_LM column is NaN and every other term is finite.  LOSS is the sum of the six terms and GRAD_NORM
    the norm of the gradients that NaN produced, so those two columns are NaN with it: "the other columns are finite" can
    only hold for the five other terms.  The flag is cleared by the report."""
    from xggm_amd import ops, trainlog as T
    from xggm_amd.engine import CapturedPretrainer
    def labelled(seed, offset):  # labelled rows of batch ``seed`` at the rng state of step ``offset + 1``
        rng, b = ops.make_rng(SEED, DEV), clean_batch(seed)
        ops.rng_advance(rng, offset)
        return int((features()(*[b[k] for k in CapturedPretrainer.KEYS], rng, img_ids=b["img_ids"])[3] != -1).sum())

    # a sequence of batches whose LAST step labels more rows than every step before it, so that a capacity can sit between
    # them: per step the batch with the fewest labelled rows, then the one with the most (what a step labels depends on its
    # batch and on the rng state alone)
    counts = {(seed, off): labelled(seed, off) for seed in BATCHES for off in range(4)}
    print("labelled rows", counts)
    few = [min(BATCHES, key=lambda seed: counts[seed, off]) for off in range(4)]
    last = next(off for off in range(1, 4)
                if max(counts[seed, off] for seed in BATCHES) > max(counts[few[k], k] for k in range(off)))
    order = few[:last] + [max(BATCHES, key=lambda seed: counts[seed, last])]
    n = [counts[seed, off] for off, seed in enumerate(order)]
    assert max(n[:-1]) < n[-1] and min(n) >= 3, n
    model, optim, tr = setup(BF16, mlm_capacity=n[-1])
    for s in order:
        tr.step(clean_batch(s))
    tr.check()  # exactly enough slots: nothing to report
    model, optim, tr = setup(BF16, mlm_capacity=n[-1] - 1)
    for s in order:
        tr.step(clean_batch(s))
    with pytest.raises(RuntimeError, match=r"mlm_capacity=%d.*training record with a NaN Mask_LM is number %d .*step %d of this window, "
                                           r"optimiser step %d\)" % (n[-1] - 1, last, last + 1, last + 1)):
        tr.check()
    rec = tr.train_log.read()
    print("records", rec["values"].tolist())
    assert bool(torch.isfinite(rec["values"][:last]).all())  # the steps before it fitted
    v = rec["values"][last]
    assert bool(torch.isnan(v[T.PT_MASK_LM])) and bool(torch.isfinite(v[T.PT_MATCHED:T.PT_QA + 1]).all())
    assert bool(torch.isnan(v[T.LOSS])) and bool(torch.isnan(v[T.PT_GRAD_NORM])) and bool(rec["present"][last].all())
    assert int(rec["first_bad"]) == last and int(rec["cursor"]) == last + 1
    tr.check()  # reported once: the flag was cleared
    assert int(model.mlm_overflow) == 0


def test_restored_run_continues_bit_for_bit(tmp_path):
    """save_training_state after two steps, two more; a fresh model and trainer with a history of their own load the
    snapshot under live graphs and run the same two steps: same records, same state"""
    from xggm_amd.vqa.vqacpv2 import save_training_state, load_training_state
    ma, oa, ta = setup(BF16)
    for s in (3, 4):
        ta.step(clean_batch(s))
    path = str(tmp_path / "state.pth")
    save_training_state(path, ma, oa, step=2)
    ta.train_log.reset()
    for s in (6, 3):
        ta.step(clean_batch(s))
    mb, ob, tb = setup(BF16)
    tb.step(clean_batch(6))
    assert load_training_state(path, mb, ob) == {"step": 2}
    tb.train_log.reset()
    for s in (6, 3):
        tb.step(clean_batch(s))
    ra, rb = ta.train_log.read(), tb.train_log.read()
    same_records(ra, rb)
    assert ra["steps"].tolist() == [3, 4]
    same(state(ma), state(mb))


# ------------------------------------------------------------------------------------------------ the driver
def _examples(n, seed, first_uid=0):
    from xggm_amd.pretrain.lxmert_pretrain import InputExample
    c = _cfg()["cfg"]
    r = np.random.default_rng(seed)
    words = ["what", "is", "the", "man", "woman"]
    labels = [{3: 0.3, 7: 0.6, 11: 1.0}, {5: 1.0}, None]
    out = []
    for i in range(n):
        sent = " ".join(r.choice(words, size=int(r.integers(1, 9))))
        out.append(InputExample("img%d_vqa_%03d" % ((first_uid + i) % 4, first_uid + i), sent,
                                (r.random((c["O"], c["F"]), dtype=np.float32), r.random((c["O"], 4), dtype=np.float32)),
                                (r.integers(0, c["n_obj"], size=c["O"]), r.random(c["O"], dtype=np.float32)),
                                (r.integers(0, c["n_attr"], size=c["O"]), r.random(c["O"], dtype=np.float32)), 1, labels[i % 3]))
    return out


def _driver(tmp_path, **kw):
    from xggm_amd import param
    from xggm_amd.lxrt.tokenization import BertTokenizer
    from xggm_amd.pretrain.lxmert_pretrain import LXMERT
    tok = BertTokenizer(os.path.join(GOLDEN, "vocab_small.txt"), do_lower_case=True)
    args = param.parse_args(["--taskMatched", "--taskMaskLM", "--taskObjPredict", "--taskQA", "--epochs", "1", "--lr", "1e-3",
                             "--wordMaskRate", "0.5", "--output", str(tmp_path / "snap")])
    model, *_ = _tiny_model("full", compute_dtype=BF16)
    model = model.to(DEV).train()
    model.seed = SEED
    return LXMERT(_cfg()["cfg"]["T"], model, tok, args=args, max_labels=K, **kw)


def test_train_batch_returns_what_the_log_recorded(tmp_path):
    from xggm_amd import trainlog as T
    from xggm_amd.lxrt.optimization import BertAdam
    lx = _driver(tmp_path)
    assert lx.features.match_rate == 0.5 and lx.features.vocab_size == 81 and lx.features.mask_id == 4
    optim = BertAdam(list(lx.model.parameters()), lr=1e-3, warmup=0.05, t_total=10)
    for seed in (1, 2):
        loss, losses, logit = lx.train_batch(optim, _examples(3, seed))
        assert isinstance(loss, float) and isinstance(losses, np.ndarray) and losses.shape == (1, 6) and losses.dtype == np.float32
        assert torch.is_tensor(logit) and tuple(logit.shape) == (3, _cfg()["cfg"]["n_ans"])
        rec = lx.engine.train_log.read()
        assert int(rec["cursor"]) == 1 and rec["steps"].tolist() == [seed]
        assert float(rec["values"][0, T.LOSS]) == loss
        assert rec["values"][0, T.PT_MASK_LM:T.PT_QA + 1].tolist() == losses[0].tolist()
        labels, _, _, n = lx.engine.answer_log.read()
        assert n == 3 and labels.tolist() == logit.float().max(1)[1].tolist()
    lx.model.eval()
    before = state(lx.model)
    loss, losses, logit = lx.valid_batch(_examples(3, 5))
    assert isinstance(loss, float) and losses.shape == (1, 6) and float(lx.engine.valid_log.read()["values"][0, T.LOSS]) == loss
    after = state(lx.model)
    before.pop("rng"), after.pop("rng")
    same(before, after)


def test_one_short_epoch_through_the_reference_interface(tmp_path, capsys, monkeypatch):
    """three training batches (the last one ragged: it runs eagerly) and two validation batches: the reference's lines, one
    answer per uid for the evaluator, each log read once"""
    from xggm_amd import engine
    lx = _driver(tmp_path)
    train_batches = [_examples(3, 1, 0), _examples(3, 2, 3), _examples(2, 3, 6)]
    eval_batches = [_examples(3, 4, 100), _examples(3, 5, 103)]
    seen = []

    class Evaluator:
        def evaluate(self, uid2ans, pprint=False):
            seen.append((dict(uid2ans), pprint))
            return 0.0

    dataset = types.SimpleNamespace(answer_table=types.SimpleNamespace(id2ans=lambda i: "ans%d" % i))
    reads = []
    read = engine.TrainLog.read
    monkeypatch.setattr(engine.TrainLog, "read", lambda self: (reads.append(self), read(self))[1])
    capsys.readouterr()  # what building the model printed
    lx.train((dataset, train_batches, Evaluator()), (dataset, eval_batches, Evaluator()))
    out = capsys.readouterr().out.splitlines()
    assert out[:3] == ["Batch per epoch: 3", "Total Iters: 3", "Warm up Iters: 0"]
    import re
    num = r"-?\d+\.\d{4}"
    terms = "The losses are " + "".join("%s: %s " % (name, num) for name in ('Mask_LM', 'Matched', 'Obj', 'Attr', 'Feat', 'QA'))
    assert re.fullmatch(r"The training loss for Epoch 0 is " + num, out[3]), out[3]
    assert re.fullmatch(terms, out[4]), out[4]
    assert re.fullmatch(r"The valid loss is " + num, out[5]), out[5]
    assert re.fullmatch(terms, out[6]), out[6]
    assert len(out) == 7
    (train_ans, pp1), (eval_ans, pp2) = seen
    assert pp1 and pp2
    assert sorted(train_ans) == sorted(e.uid for b in train_batches for e in b) and len(train_ans) == 8
    assert sorted(eval_ans) == sorted(e.uid for b in eval_batches for e in b) and len(eval_ans) == 6
    assert all(re.fullmatch(r"ans\d+", a) for a in list(train_ans.values()) + list(eval_ans.values()))
    assert reads == [lx.engine.train_log, lx.engine.valid_log]  # one read per sweep
    for name in ("BEST_EVAL_LOSS", "Epoch01"):
        assert os.path.exists(str(tmp_path / "snap" / (name + "_LXRT.pth")))
    sd = torch.load(str(tmp_path / "snap" / "Epoch01_LXRT.pth"), map_location="cpu", weights_only=True)
    assert sorted(sd) == sorted(lx.model.state_dict())


def test_log_every_reads_once_per_window_and_forward_is_one_eager_pass(tmp_path, capsys, monkeypatch):
    """log_every=2 over three validation batches: two read-backs, every uid answered, the same mean as one read-back gives;
    ``forward`` returns the reference's (loss, losses on the host, ans_logit)"""
    from xggm_amd import engine
    batches = [_examples(3, 4, 100), _examples(3, 5, 103), _examples(3, 6, 106)]
    dataset = types.SimpleNamespace(answer_table=types.SimpleNamespace(id2ans=lambda i: "ans%d" % i))
    got = []
    for log_every in (2, None):
        lx = _driver(tmp_path, log_every=log_every)
        lx.model.eval()
        seen, reads = [], []
        evaluator = types.SimpleNamespace(evaluate=lambda uid2ans, pprint=False: seen.append(dict(uid2ans)))
        read = engine.TrainLog.read
        with monkeypatch.context() as m:
            m.setattr(engine.TrainLog, "read", lambda self: (reads.append(self), read(self))[1])
            avg = lx.evaluate_epoch((dataset, batches, evaluator))
        assert lx.engine is None and lx.valid_engine.optim is None and sorted(lx.valid_engine.graphs) == ["valid"]
        assert len(reads) == (2 if log_every else 1) and all(r is lx.valid_engine.valid_log for r in reads)
        assert sorted(seen[0]) == sorted(e.uid for b in batches for e in b)
        got.append((avg, seen[0]))
    assert got[0][0] == pytest.approx(got[1][0], rel=1e-6) and got[0][1] == got[1][1]
    assert "The valid loss is %0.4f" % got[1][0] in capsys.readouterr().out
    loss, losses, logit = lx.forward(batches[0])
    assert loss.dim() == 0 and loss.is_cuda and not losses.is_cuda and tuple(losses.shape) == (1, 6) and tuple(logit.shape) == (3, 19)


def test_validation_at_its_own_batch_size_replays_its_own_graph(tmp_path, monkeypatch):
    """training batches of 2, validation batches of 3 (the reference validates at 512 against --bs), log_every=2 and three
    full validation batches plus a ragged one: the epoch runs through (an answer log of 2 steps x 2 training rows would
    overflow at the second validation batch), validation has an engine of its own captured at 3 rows without an optimiser,
    its full batches are replays -- only the ragged one runs eagerly -- and it changes no weight and no moment"""
    lx = _driver(tmp_path, log_every=2)
    train_batches = [_examples(2, 1, 0), _examples(2, 2, 2), _examples(2, 3, 4)]
    eval_batches = [_examples(3, 4, 100), _examples(3, 5, 103), _examples(3, 6, 106), _examples(1, 7, 109)]
    seen = []
    evaluator = types.SimpleNamespace(evaluate=lambda uid2ans, pprint=False: seen.append(dict(uid2ans)))
    dataset = types.SimpleNamespace(answer_table=types.SimpleNamespace(id2ans=lambda i: "ans%d" % i))
    lx.train((dataset, train_batches, evaluator), (dataset, eval_batches, evaluator))
    assert sorted(seen[0]) == sorted(e.uid for b in train_batches for e in b)
    assert sorted(seen[1]) == sorted(e.uid for b in eval_batches for e in b) and len(seen[1]) == 10
    ve = lx.valid_engine
    assert lx.engine.B == 2 and ve is not lx.engine and ve.B == 3 and ve.optim is None and sorted(ve.graphs) == ["valid"]
    assert ve.answer_log.capacity == 2 * 3 and ve.train_log is None
    with pytest.raises(RuntimeError, match="validation only"):
        ve.step()
    eager, replays = [], []
    run, replay = ve._valid_pass, ve.graphs["valid"].replay
    monkeypatch.setattr(ve, "_valid_pass", lambda s: (eager.append(s["input_ids"].shape[0]), run(s))[1])
    ve.graphs["valid"] = types.SimpleNamespace(replay=lambda: (replays.append(1), replay())[1])
    before = state(lx.model)
    lx.evaluate_epoch((dataset, eval_batches, evaluator))
    after = state(lx.model)
    assert eager == [1] and len(replays) == 3 and lx.valid_engine is ve
    before.pop("rng"), after.pop("rng")
    same(before, after)
    assert sorted(seen[2]) == sorted(seen[1])
