"""The fine-tuning drivers on the GPU (``vqa.vqacpv2.VQA``, ``gqa.gqa_ood.GQA``): ``predict`` / ``evaluate`` / ``oracle_score``
against the module's ``predict`` and the evaluators, and a two-epoch ``train`` against a loop written by hand from the pieces
the drivers are made of -- every weight and moment bit for bit, the reference's log, files and writer scalars."""
import os
import random
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import GOLDEN  # noqa: E402

DEV = "cuda"
BF16 = torch.bfloat16
TOL = 2.0 ** -24  # one fp32 rounding of a score <= 1 (the store holds fp32, the evaluator adds Python doubles)
B, A = 4, 29
TYPES = ("number", "other", "yes/no")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


# ----------------------------------------------------------------------------- the tiny model and shards (local copies of
# the helpers of tests/test_resident_gpu.py, with a GQA kind whose data set repeats a question once per label)
def _tok():
    from xggm_amd.lxrt.tokenization import BertTokenizer
    return BertTokenizer(os.path.join(GOLDEN, "vocab_small.txt"), do_lower_case=True)


def _model():
    from oracle import shapes
    from test_model_gpu import build_model
    cfg = dict(shapes.TINY, l_layers=3, x_layers=2, r_layers=2, vocab=96)  # the test vocabulary has 81 entries
    m = build_model(cfg, A, seed=5, dt=BF16)
    m.seed = 11
    return cfg, m


def _split(tmp_path, kind, name, n_img, n_q, F, vocab, seed, many=False):
    """(dataset, torch dataset, evaluator) of ``n_q`` questions over ``n_img`` images, one to three answers each (``many``: ten
    to twelve, so that an untrained model scores above zero and ``BEST`` is written); every datum carries an ``answer_type``.
    kind "gqa": string ids, label dicts, and a torch data set that keeps a datum once per label -- question ids repeat"""
    from xggm_amd import synth
    from xggm_amd.gqa.gqa_ood_data import GQADataset, GQAEvaluator, GQATorchDataset
    from xggm_amd.tools.shards import ShardWriter
    from xggm_amd.vqa.vqacpv2_data import VQADataset, VQAEvaluator, VQATorchDataset
    words = [w for w in open(os.path.join(GOLDEN, "vocab_small.txt")).read().split() if w.isalpha()][:40]
    rng = np.random.default_rng(seed)
    w = ShardWriter(str(tmp_path / ("%s_%s_obj36.xgs" % (name, kind))), n_objects=36, feat_dim=F)
    src = synth.vqa_batch(n_img, A=A, F=F, vocab=vocab, seed=seed)
    for i in range(n_img):
        w.add(i, src["feats"][i], src["boxes"][i] * 0.99, 1.0, 1.0, src["adj_true"][i])
    l2a = ["a%d" % k for k in range(A)]
    data = []
    for q in range(n_q):
        k = (10 if many else 1) + q % 3
        labels = [int(x) for x in rng.choice(A, k, replace=False)]
        scores = [float(x) for x in rng.choice([0.3, 0.6, 0.9, 1.0], k)]
        sent = " ".join(rng.choice(words, size=int(rng.integers(3, 9))))
        d = dict(answer_type=TYPES[q % 3])
        if kind == "vqa":
            d.update(question_id=100 + q, image_id=int((5 * q) % n_img), label=labels, score=scores, question=sent)
        else:
            d.update(question_id="q%03d" % q, img_id=int((5 * q) % n_img), label={l2a[l]: s for l, s in zip(labels, scores)}, sent=sent)
        data.append(d)
    DS, TS, EV = (VQADataset, VQATorchDataset, VQAEvaluator) if kind == "vqa" else (GQADataset, GQATorchDataset, GQAEvaluator)
    dset = DS(name, data=data, ans2label={a: k for k, a in enumerate(l2a)}, label2ans=l2a)
    return dset, TS(dset, shard=w.close()), EV(dset)


def _stores(tmp_path, kind, cfg, n_train):
    from xggm_amd.lxrt.entry import SentenceBatcher
    from xggm_amd.tools.resident import ResidentDataset, group_ids
    batcher = SentenceBatcher(_tok(), 20)
    out = {}
    for name, n_q, seed in (("train", n_train, 21), ("valid", 9, 22)):
        dset, ts, ev = _split(tmp_path, kind, name, 6, n_q, cfg["feat_dim"], cfg["vocab"], seed, many=name == "valid")
        store = ResidentDataset(ts, batcher, DEV, groups=group_ids(ts.data, "answer_type"), chunk_bytes=1 << 16)
        out[name] = (dset, ts, ev, store)
    return batcher, out


def _args(tmp_path, epochs=2):
    from xggm_amd import param
    return param.parse_args(["--bs", str(B), "--epochs", str(epochs), "--lr", "1e-4", "--seed", "4", "--output", str(tmp_path / "snap")])


def _cls(kind):
    from xggm_amd.gqa.gqa_ood import GQA
    from xggm_amd.vqa.vqacpv2 import VQA
    return VQA if kind == "vqa" else GQA


class Writer:
    def __init__(self):
        self.rows, self.closed = [], False

    def add_scalar(self, tag, value, step):
        self.rows.append((tag, float(value), int(step)))

    def close(self):
        self.closed = True


# ----------------------------------------------------------------------------- sweeps
@pytest.mark.parametrize("kind", ["vqa", "gqa"])
def test_predict_evaluate_and_oracle_score(tmp_path, kind):
    """``predict`` == the module's ``predict`` through a predictor of its own; ``evaluate`` (no dict is built: the log is scored
    on the device) within 2^-24 of the evaluator on that dict, per group too; ``oracle_score`` within 2^-24 of the evaluator on
    the targets' arg-max.  The GQA validation set repeats question ids: the keep mask gives the dict's count."""
    from xggm_amd.engine import AnswerLog, CapturedPredictor
    from xggm_amd.vqa.vqacpv2 import predict
    cfg, m = _model()
    _, st = _stores(tmp_path, kind, cfg, 8)
    dset, ts, ev, store = st["valid"]
    n = len(store)
    assert n == (9 if kind == "vqa" else 99) and n % B and store.K == 12
    drv = _cls(kind)(m, (st["train"][0], st["train"][3], st["train"][2]), (dset, store, ev), args=_args(tmp_path), valid_batch_size=B)
    assert drv.valid_B == B
    tup = (dset, store, ev)
    want = predict(m, tup, predictor=CapturedPredictor(m, B, log=AnswerLog(n, DEV, with_scores=False)), resident=store)
    assert len(want) == 9 and drv.predict(tup) == want
    score = drv.evaluate(tup)
    print(kind, "evaluate", score, "evaluator", ev.evaluate(want))
    assert isinstance(score, float) and abs(score - ev.evaluate(want)) <= TOL
    dumped = str(tmp_path / "dump.json")
    assert abs(drv.evaluate(tup, dump=dumped) - ev.evaluate(want)) < 1e-15 and os.path.exists(dumped)  # the host path
    by = drv.evaluate(tup, by_group=True)
    assert sorted(by) == sorted(("all",) + TYPES) and abs(by["all"] - ev.evaluate(want)) <= TOL
    for t in TYPES:
        sub = {d["question_id"]: want[d["question_id"]] for d in dset.data if d["answer_type"] == t}
        assert abs(by[t] - ev.evaluate(sub)) <= TOL, t
    assert drv.sweeps == 4 and drv.predictor.log.count == n
    top = {ts.data[i]["question_id"]: dset.label2ans[int(ts[i][4].max(0)[1])] for i in range(n)}
    oracle = drv.oracle_score(tup)
    print(kind, "oracle", oracle, "evaluator", ev.evaluate(top))
    assert abs(oracle - ev.evaluate(top)) <= TOL and oracle > score
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------- training
@pytest.mark.parametrize("kind", ["vqa", "gqa"])
def test_two_epochs_equal_a_hand_written_loop(tmp_path, kind):
    from test_engine_gpu import _same_state
    from xggm_amd.answers import to_quesid2ans
    from xggm_amd.engine import AnswerLog, CapturedPredictor, CapturedTrainer, TrainLog
    from xggm_amd.vqa.vqacpv2 import make_optimizer, pick_branch, predict, val_schedule
    cfg, m = _model()
    _, m2 = _model()
    n_train = 24 if kind == "vqa" else 12  # the GQA torch data set holds a datum per label: 24 samples either way
    _, st = _stores(tmp_path, kind, cfg, n_train)
    dset, ts, ev, store = st["train"]
    vset, vts, vev, vstore = st["valid"]
    assert len(store) == 24
    args = _args(tmp_path)
    n_b, epochs, seed = len(store) // B, args.epochs, args.seed
    val = [int(v) for v in val_schedule(n_b)]
    assert val == [1, 3, 4]

    # ---- the driver
    writer = Writer()
    drv = _cls(kind)(m, (dset, store, ev), (vset, vstore, vev), args=args, valid_batch_size=B, writer=writer)
    random.seed(7)
    drv.train((dset, store, ev), (vset, vstore, vev))

    # ---- the twin: the existing pieces, the same seeds, the same validations
    opt2 = make_optimizer(m2, args.lr, 2 * n_b * epochs, optim=args.optim)
    order = store.order(0, shuffle=True, seed=seed, drop_last=True, batch_size=B)
    batch0 = {k: v.to(DEV) for k, v in store.host_batch(order[:B]).items() if k not in ("sample", "bias_index")}
    tr2 = CapturedTrainer(m2, opt2, batch0, sigma=args.sigma, order=kind, answer_log=AnswerLog(n_b * B, DEV),
                          train_log=TrainLog(2 * n_b, DEV))
    pred2 = []  # built at the first sweep, as the driver builds its own
    random.seed(7)
    best, want_valid, want_train, last_loss, plain_loss, want_rows, it = 0.0, [], [], [], [], [], 0
    extra = _cls(kind).extra_tags

    def sweep(epoch):
        nonlocal best
        if not pred2:
            pred2.append(CapturedPredictor(m2, B, log=AnswerLog(len(vstore), DEV, with_scores=False)))
        s = vev.evaluate(predict(m2, (vset, None, vev), predictor=pred2[0], resident=vstore))
        want_valid.append(s)
        best = max(best, s)
        want_rows.append(("Val/acc", epoch))

    for epoch in range(epochs):
        order = store.order(epoch, shuffle=True, seed=seed, drop_last=True, batch_size=B)
        tr2.answer_log.reset()
        for i in range(n_b):
            tr2.load_resident(store, i * B)
            (lp, _, _), (lg, _, _) = tr2.iteration(pick_branch(args.delta, model=m2))
            last_loss.append(float(lg) if kind == "vqa" else float(lp))
            plain_loss.append(float(lp))
            want_rows += [(t, it) for t in ("Train/batch_loss", "Train/average_loss", "lr") + extra]
            it += 1
            if i in val:
                sweep(epoch)
        labels = tr2.answer_log.read()[0]
        want_train.append(ev.evaluate(to_quesid2ans(store.ques_ids(order), labels, dset.label2ans)))
        want_rows.append(("Train/acc", epoch))
        sweep(epoch)

    # ---- what the twin must show
    _same_state(m, m2)  # weights, gradients, moments, step counters, Philox state: bit for bit
    sd, sd2 = m.state_dict(), m2.state_dict()
    assert all(torch.equal(sd[k], sd2[k]) for k in sd2)
    assert drv.sweeps == epochs * (len(val) + 1) == len(want_valid)
    print(kind, "train", [h["train"] for h in drv.history], want_train, "valid", drv.valid_scores, want_valid)
    for e in range(epochs):
        assert abs(drv.history[e]["train"] / 100. - want_train[e]) <= TOL, e
    assert len(drv.valid_scores) == len(want_valid) and all(abs(a - b) <= TOL for a, b in zip(drv.valid_scores, want_valid))
    if kind == "gqa":
        assert len(set(store.ques_ids(order))) < len(order)  # the train score's divisor is NOT the number of logged rows
    # log.log: the reference's lines, from the driver's unrounded numbers (held to the evaluator above)
    text = open(os.path.join(args.output, "log.log")).read()
    gap = "\n" if kind == "vqa" else ""
    assert text == "".join("\nEpoch %d: Train %.2f\n%sEpoch %d: Valid %.2f\nEpoch %d: Best %.2f\n"
                           % (e, h["train"], gap, e, h["valid"] * 100., e, h["best"] * 100.) for e, h in enumerate(drv.history))
    assert re.fullmatch(r"(\nEpoch \d: Train \d+\.\d\d\n%sEpoch \d: Valid \d+\.\d\d\nEpoch \d: Best \d+\.\d\d\n){2}" % gap, text)
    assert abs(drv.history[-1]["best"] - best) <= TOL and drv.history[0]["valid"] == drv.valid_scores[len(val)]
    # the writer: the reference's tags at the reference's steps, in its order
    assert [(t, s) for t, _, s in writer.rows] == want_rows and writer.closed
    got_last = [v for t, v, _ in writer.rows if t == "Train/batch_loss"]
    assert got_last == last_loss
    div = B if kind == "vqa" else A
    avg = np.cumsum(np.asarray(plain_loss) / div) / np.arange(1, len(plain_loss) + 1)
    assert np.allclose([v for t, v, _ in writer.rows if t == "Train/average_loss"], avg, rtol=1e-6, atol=0)
    assert {v for t, v, _ in writer.rows if t == "lr"} == {4 * args.lr}
    assert all(v == 0.0 for t, v, _ in writer.rows if t in extra)
    # the snapshots
    final = {k: v.clone() for k, v in m.state_dict().items()}
    for name in ["BEST"] + ["BEST_%d" % e for e in range(epochs)]:
        path = os.path.join(args.output, name)
        assert os.path.exists(path + ".pth"), name
        saved = torch.load(path + ".pth", map_location="cpu", weights_only=True)
        drv.load(path)
        now = m.state_dict()
        assert sorted(now) == sorted(saved) and all(torch.equal(now[k].cpu(), saved[k]) for k in saved), name
    assert all(torch.equal(now[k], final[k]) for k in final)  # BEST_<last epoch> is the final model
    torch.cuda.synchronize()


def test_host_fed_epoch_and_the_refusal(tmp_path):
    """a ``DataLoaderX``-fed epoch completes through ``load_batch`` and the module's ``predict`` (the host path): the log's
    format and the saved files; a model prepared for data parallelism is refused"""
    from xggm_amd.tools.data_loader import DataLoaderX
    from xggm_amd.vqa.vqacpv2 import VQA
    cfg, m = _model()
    batcher, st = _stores(tmp_path, "vqa", cfg, 12)
    dset, ts, ev, _ = st["train"]
    vset, vts, vev, _ = st["valid"]
    args = _args(tmp_path, epochs=1)
    train = (dset, DataLoaderX(ts, B, shuffle=True, seed=args.seed, drop_last=True, device=DEV, batcher=batcher), ev)
    valid = (vset, DataLoaderX(vts, B, device=DEV, batcher=batcher), vev)
    drv = VQA(m, train, valid, args=args)
    random.seed(3)
    drv.train(train, valid)
    text = open(os.path.join(args.output, "log.log")).read()
    assert re.fullmatch(r"\nEpoch 0: Train \d+\.\d\d\n\nEpoch 0: Valid \d+\.\d\d\nEpoch 0: Best \d+\.\d\d\n", text)
    assert drv.sweeps == 4 and len(drv.history) == 1 and 0.0 <= drv.history[0]["train"] <= 100.0
    assert os.path.exists(os.path.join(args.output, "BEST_0.pth"))
    assert abs(drv.evaluate(valid) - drv.valid_scores[-1]) < 1e-15
    object.__setattr__(m, "_grad_sync", object())
    with pytest.raises(NotImplementedError, match="enable_data_parallel"):
        VQA(m, train, valid, args=args)
    torch.cuda.synchronize()
