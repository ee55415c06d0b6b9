"""Resident pre-training set on the GPU: ``ops.pretrain_gather`` against its numpy restatement (``gather_pretrain_host``,
which tests/test_pretrain_resident_cpu.py holds to ``collate_examples`` and ``swap_rule``) -- every field bit for bit, inside
canary buffers --, the fused swap against ``ops.pretrain_swap`` composed behind a clean gather, a captured gather, and the
store feeding ``CapturedPretrainer.load_resident`` and ``LXMERT.train`` against twins fed by ``load_batch`` / a list loader."""
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import pretrain_mask_ref as R  # noqa: E402
from pretrain_resident_cases import tok  # noqa: E402
from test_resident_gpu import Canary, _bits, _check, _order, _tables, _to_device, N_IMG, N_ORDER, N_Q  # noqa: E402
from test_pretrain_engine_gpu import (BF16, F32, K, SEED, SID, _cfg, _examples, _tiny_model, _visual_config,  # noqa: E402,F401
                                      features, same, same_records, state)

DEV = "cuda"
TRIES = 8
I64 = torch.int64


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


# ----------------------------------------------------------------------------- 1. the kernel
def _host_tables(O, F, T, Kk, f32, one_image=False):
    """13 samples over 6 images in the kernel's layout; the features (rounding ties, values that round to inf, denormals),
    boxes, image rows, labels and scores are those of tests/test_resident_gpu.py::_tables"""
    base = _tables(O, F, 29, Kk, f32)
    rng = np.random.default_rng([11, O, F, T, Kk])
    t = {k: base[k] for k in ("feats", "boxes", "q_row", "q_label", "q_score")}
    t["obj_labels"] = rng.integers(0, 1600, (N_IMG, O)).astype(np.int32)
    t["attr_labels"] = rng.integers(-1, 400, (N_IMG, O)).astype(np.int32)
    t["obj_confs"], t["attr_confs"] = rng.random((N_IMG, O), dtype=np.float32), rng.random((N_IMG, O), dtype=np.float32)
    t["q_len"] = rng.integers(2, T + 1, N_Q).astype(np.int32)
    t["q_len"][:2] = (T, 2)
    t["q_ids"] = (rng.integers(1, 30000, (N_Q, T)) * (np.arange(T)[None] < t["q_len"][:, None])).astype(np.int32)
    if one_image:
        t["q_row"] = np.zeros(N_Q, dtype=np.int32)
    return t


def _canaries(R_, O, F, T, Kk, out_f32):
    """every output inside a sentinel buffer; leads keep feats / boxes 16-byte aligned and give every other field its element
    alignment only; feature rows are padded (stride > row)"""
    f4 = torch.float32
    return dict(feats=Canary(R_, (O, F), f4 if out_f32 else BF16, lead=8, stride=O * F + 8), boxes=Canary(R_, (O, 4), f4, lead=4),
                obj_labels=Canary(R_, (O,), I64, lead=1), attr_labels=Canary(R_, (O,), I64, lead=3),
                obj_confs=Canary(R_, (O,), f4, lead=1), attr_confs=Canary(R_, (O,), f4, lead=3),
                input_ids=Canary(R_, (T,), I64, lead=1), input_mask=Canary(R_, (T,), I64, lead=2), segment_ids=Canary(R_, (T,), I64, lead=3),
                label_ids=Canary(R_, (Kk,), I64, lead=1), label_scores=Canary(R_, (Kk,), f4, lead=1),
                is_matched=Canary(R_, (), I64, lead=1), img_ids=Canary(R_, (), I64, lead=2), sample=Canary(R_, (), I64, lead=3),
                swapped_from=Canary(R_, (), I64, lead=1))


def _views(c):
    return {k: v.view for k, v in c.items()}


@pytest.mark.parametrize("O,F", [(36, 64), (5, 8)])
@pytest.mark.parametrize("feats_f32,out_f32", [(False, False), (False, True), (True, False), (True, True)])
def test_pretrain_gather_equals_the_host_restatement(O, F, feats_f32, out_f32):
    """every field ``torch.equal`` (on the bit patterns) to ``gather_pretrain_host`` without a swap for T in {20, 7}, K in
    {1, 3}, B in {1, 4, 7} ending exactly at the end of an order with repeated samples and images; every output sits in a
    sentinel buffer: nothing in front of the first row, in the padding between rows or in rows b >= B is written"""
    from xggm_amd import ops
    from xggm_amd.pretrain.resident import gather_pretrain_host
    order = _order()
    d_order = torch.from_numpy(order).to(DEV)
    for T in (20, 7):
        for Kk in (1, 3):
            host = _host_tables(O, F, T, Kk, feats_f32)
            dev = _to_device(host)
            for B, start in ((1, N_ORDER - 1), (4, N_ORDER - 4), (7, N_ORDER - 7), (4, 0)):
                c = _canaries(B + 2, O, F, T, Kk, out_f32)
                ops.pretrain_gather(dev, d_order, start, B, _views(c))
                ref = gather_pretrain_host(host, order[start:start + B], out_f32=out_f32)
                assert ref["is_matched"].tolist() == [1] * B and ref["swapped_from"].tolist() == [-1] * B
                _check(c, ref, B, (T, Kk, B, start))
    if feats_f32 and not out_f32:  # the planted values are in the batches above: more infinities out than went in
        last = gather_pretrain_host(host, order[N_ORDER - 7:])["feats"]
        assert int(torch.isinf(last.float()).sum()) > int(np.isinf(host["feats"][host["q_row"][order[N_ORDER - 7:]]]).sum()) > 0


# ----------------------------------------------------------------------------- 2. the fused swap
def _edge_draws(host, samples):
    """supplied draws that hit the edges: u == rate, the float below it, own image twice then another, the float below 1,
    picks outside [0, 1)"""
    B, q_row = len(samples), host["q_row"]
    rng = np.random.default_rng(5)
    u_swap, u_pick = rng.random(B, dtype=np.float32), rng.random((B, TRIES), dtype=np.float32)
    half, top = np.float32(0.5), np.nextafter(np.float32(1), np.float32(0))
    u_swap[0] = half
    if B > 1:
        u_swap[1] = np.nextafter(half, np.float32(0))
    if B > 2:
        s = samples[2]
        own = [j for j in range(N_Q) if q_row[j] == q_row[s]]
        other = [j for j in range(N_Q) if q_row[j] != q_row[s]][0]
        u_swap[2] = 0.0
        u_pick[2, :3] = [(own[0] + 0.5) / N_Q, (own[-1] + 0.5) / N_Q, (other + 0.5) / N_Q]
    if B > 3:
        u_swap[3], u_pick[3, 0] = 0.0, top
    if B > 5:
        u_swap[4:6] = 0.0
        u_pick[4], u_pick[5] = -3.0, 17.5  # held inside the store: sample 0 resp. n_q - 1 at every try
    return u_swap, u_pick


def _swap_case(host, dev, d_order, order, start, B, O, F, T, Kk, draws, rng):
    """the fused launch and the two existing launches composed -> (fused canaries, composed dict, fused exhausted)"""
    from xggm_amd import ops
    from xggm_amd.pretrain.resident import ResidentPretrainSet
    clean = _canaries(B + 1, O, F, T, Kk, False)
    ops.pretrain_gather(dev, d_order, start, B, _views(clean))
    pool = ResidentPretrainSet(host, DEV, chunk_bytes=1 << 12).sent_pool()  # every sample of the store, keyed by q_row
    ddraws = {k: torch.from_numpy(v).to(DEV) for k, v in (draws or {}).items()}
    comp = ops.pretrain_swap(clean["input_ids"].view[:B].contiguous(), clean["input_mask"].view[:B].contiguous(),
                             clean["img_ids"].view[:B].contiguous(), 0.5, pool=pool, rng=rng, sid_base=SID, draws=dict(ddraws))
    fused = _canaries(B + 1, O, F, T, Kk, False)
    ex = Canary(1, (), torch.int32, lead=1)
    ex.view.zero_()
    ops.pretrain_gather(dev, d_order, start, B, _views(fused), match_rate=0.5, rng=rng, sid_base=SID, draws=dict(ddraws), exhausted=ex.view)
    for k in ("input_ids", "input_mask", "is_matched"):
        assert torch.equal(fused[k].view[:B], comp[k]), (k, B, start)
    assert torch.equal(ex.view.reshape(1), comp["exhausted"]) and ex.untouched(1)
    # what the swap must not touch equals the clean gather; nothing outside rows 0 .. B - 1 is written
    for k, cv in fused.items():
        assert cv.untouched(B), k
        if k not in ("input_ids", "input_mask", "is_matched", "swapped_from"):
            assert torch.equal(_bits(cv.view[:B]), _bits(clean[k].view[:B])), k
    # swapped_from is consistent with the sentences and the flags
    frm, m = fused["swapped_from"].view[:B].cpu().numpy(), fused["is_matched"].view[:B].cpu().numpy()
    samples = order[start:start + B]
    assert ((frm == -1) == (m == 1)).all() and set(m.tolist()) <= {0, 1}
    sent = np.where(m == 0, frm, samples)
    assert fused["input_ids"].view[:B].cpu().tolist() == host["q_ids"][sent].tolist()
    assert (host["q_row"][sent[m == 0]] != host["q_row"][samples[m == 0]]).all()
    return fused, comp, int(ex.view)


@pytest.mark.parametrize("O,F,T,Kk", [(36, 64, 20, 3), (5, 8, 7, 1)])
def test_fused_swap_equals_gather_then_pretrain_swap(O, F, T, Kk):
    """``pretrain_gather(match_rate=0.5)`` == ``pretrain_gather`` + ``ops.pretrain_swap(pool = every sample)``: input_ids,
    input_mask, is_matched and exhausted bit for bit, once from Philox (nothing supplied) and once from supplied draws that hit
    the edges; the supplied case also equals ``gather_pretrain_host``; a one-image store leaves every row matched and counts
    the rows that tried"""
    from xggm_amd.pretrain.resident import gather_pretrain_host
    host = _host_tables(O, F, T, Kk, False)
    dev = _to_device(host)
    order = _order()
    d_order = torch.from_numpy(order).to(DEV)
    rng = torch.tensor([2025, 3], dtype=I64, device=DEV)
    swapped = 0
    for B, start in ((1, N_ORDER - 1), (4, N_ORDER - 4), (7, N_ORDER - 7)):
        fused, _, _ = _swap_case(host, dev, d_order, order, start, B, O, F, T, Kk, None, rng)
        u = R.philox_uniform(2025, 3, SID + 5, B)
        assert ((u < 0.5) >= (fused["is_matched"].view[:B].cpu().numpy() == 0)).all()  # only rows whose draw says so swap
        swapped += int((fused["is_matched"].view[:B] == 0).sum())
        samples = order[start:start + B]
        u_swap, u_pick = _edge_draws(host, samples)
        fused, _, n_ex = _swap_case(host, dev, d_order, order, start, B, O, F, T, Kk, dict(u_swap=u_swap, u_pick=u_pick), None)
        ref = gather_pretrain_host(host, samples, draws=dict(u_swap=u_swap, u_pick=u_pick), match_rate=0.5)
        assert n_ex == int(ref["exhausted"])
        _check(fused, ref, B, ("edges", B))
        m = ref["is_matched"].tolist()
        assert m[0] == 1 and (B < 2 or m[1] == 0)  # u == rate stays matched, the float below swaps
        if B == 7:
            assert int(ref["swapped_from"][2]) >= 0  # own image twice, then another: the third candidate wins
    assert swapped > 0
    # one image: nobody finds another one
    host1 = _host_tables(O, F, T, Kk, False, one_image=True)
    dev1 = _to_device(host1)
    B, start = 7, N_ORDER - 7
    u_swap, u_pick = _edge_draws(host, order[start:])
    fused, _, n_ex = _swap_case(host1, dev1, d_order, order, start, B, O, F, T, Kk, dict(u_swap=u_swap, u_pick=u_pick), None)
    assert fused["is_matched"].view[:B].tolist() == [1] * B and n_ex == int((u_swap < 0.5).sum()) > 0


# ----------------------------------------------------------------------------- 3. capture
def test_pretrain_gather_replays_follow_order_and_rng():
    """captured in a graph (nothing in the call allocates, copies or synchronises) and replayed with ``order`` rewritten and
    ``rng`` advanced in between: every replay reads what it finds, swap decisions included"""
    from xggm_amd import ops
    from xggm_amd.pretrain.resident import gather_pretrain_host
    O, F, T, Kk, B, start = 36, 64, 20, 3, 7, 5
    host = _host_tables(O, F, T, Kk, True)
    dev = _to_device(host)
    o1, o2 = _order(1), _order(2)
    d_order = torch.from_numpy(o1).to(DEV)
    rng = torch.tensor([SEED, 0], dtype=I64, device=DEV)
    ex = torch.zeros(1, dtype=torch.int32, device=DEV)
    c = _canaries(B + 1, O, F, T, Kk, False)
    call = lambda: ops.pretrain_gather(dev, d_order, start, B, _views(c), match_rate=0.5, rng=rng, sid_base=SID, exhausted=ex)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    decisions = []
    for off, o in ((0, o1), (1, o2), (5, o2)):
        d_order.copy_(torch.from_numpy(o))
        rng.copy_(torch.tensor([SEED, off], dtype=I64))
        ex.zero_()
        for cv in c.values():
            cv.raw.fill_(0xA5)
        g.replay()
        draws = dict(u_swap=R.philox_uniform(SEED, off, SID + 5, B), u_pick=R.philox_uniform(SEED, off, SID + 6, B * TRIES).reshape(B, TRIES))
        ref = gather_pretrain_host(host, o[start:start + B], draws=draws, match_rate=0.5)
        _check(c, ref, B, ("replay", off))
        assert int(ex) == int(ref["exhausted"])
        decisions.append(ref["swapped_from"].tolist())
    assert decisions[1] != decisions[2] and any(x >= 0 for d in decisions for x in d)  # the advance moved the swap


# ----------------------------------------------------------------------------- 4. the engine
N_EX = 9  # samples of the engine's store: identity order, batches of 3 -> rows 0 and 1 of every batch carry answer labels


def _engine_store(match_rate=0.5, n=N_EX, **kw):
    from xggm_amd.pretrain.resident import ResidentPretrainSet
    c = _cfg()["cfg"]
    return ResidentPretrainSet(_examples(n, 31), DEV, tokenizer=tok(), max_seq_length=c["T"], max_labels=K, n_answers=c["n_ans"],
                               vocab_size=c["vocab"], match_rate=match_rate, sid_base=SID, batch_size=3, chunk_bytes=1 << 12, **kw)


def _seed_keeps_a_label(labelled, u_swaps):
    """in every step a row that carries an answer label keeps its sentence (u_swap >= 0.5): the QA loss stays finite"""
    return all(any(l and float(u) >= 0.5 for l, u in zip(ls, us)) for ls, us in zip(labelled, u_swaps))


def _engine(dt, store, twin=False, use_graph=True):
    from xggm_amd.engine import AnswerLog, CapturedPretrainer, TrainLog
    from xggm_amd.lxrt.optimization import BertAdam
    model, *_ = _tiny_model("full", compute_dtype=dt)
    model = model.to(DEV).train()
    model.seed = SEED
    optim = BertAdam(list(model.parameters()), lr=1e-3, warmup=0.1, t_total=20)
    logs = dict(train_log=TrainLog(8, DEV), valid_log=TrainLog(8, DEV), answer_log=AnswerLog(64, DEV, with_scores=False))
    batch = store.fill(store.buffers(3), 0, 3, swap=False)
    if twin:
        batch = {k: v for k, v in batch.items() if k != "sample"}
        batch.update(zip(("pool_ids", "pool_mask", "pool_img"), (t.clone() for t in store.sent_pool())), feat_pool=store.feat_pool().clone())
        tr = CapturedPretrainer(model, optim, batch, features(), use_graph=use_graph, warmup_iters=1, **logs)
    else:
        tr = CapturedPretrainer(model, optim, batch, features(match_rate=None), use_graph=use_graph, warmup_iters=1, resident=store, **logs)
        assert tr.static["feat_pool"].data_ptr() == store.tables["feats"].data_ptr()  # by reference
    return model, optim, tr


def _feed(tr, store, step, twin=False):
    if twin:
        rows = store._order_host[3 * step:3 * step + 3]
        tr.load_batch({k: v.to(DEV) for k, v in store.host_batch(rows).items()})
    else:
        tr.load_resident(store, 3 * step)
    tr.step()


def _result(model, tr, exhausted):
    tr.check()
    labels, _, _, n = tr.answer_log.read()
    return tr.train_log.read(), state(model), labels, n, int(exhausted)


@pytest.mark.parametrize("dt", [F32, BF16])
def test_load_resident_equals_the_load_batch_twin(dt):
    """three steps fed by ``load_resident`` from a swapping store (``resident=store``) against a twin fed by ``load_batch`` of
    ``host_batch`` rows whose ``DeviceFeatures(match_rate=0.5)`` owns clones of the same pools: parameters, moments, counters,
    rng, every record and the answer log bit for bit -- captured and eager"""
    store = _engine_store()
    store.order(0, shuffle=False, drop_last=False)
    labelled = [[bool((store.host["q_label"][s] >= 0).any()) for s in range(3 * k, 3 * k + 3)] for k in range(3)]
    assert _seed_keeps_a_label(labelled, [R.philox_uniform(SEED, k, SID + 5, 3) for k in range(3)])
    runs = []
    for twin, use_graph in ((False, True), (True, True), (False, False)):
        store.swap_exhausted.zero_()
        model, optim, tr = _engine(dt, store, twin, use_graph)
        start = state(model)
        for k in range(3):
            _feed(tr, store, k, twin)
            if not twin:
                assert tr.static["sample"].tolist() == [3 * k, 3 * k + 1, 3 * k + 2]
                assert tr.static["img_ids"].tolist() == store.host["q_row"][3 * k:3 * k + 3].tolist()
        runs.append(_result(model, tr, tr.features.swap_exhausted if twin else store.swap_exhausted) + (start,))
    rec, st, labels, n, ex, start = runs[0]
    assert int(start["rng"][1]) == 0 and int(st["rng"][1]) == 3 and n == 9 and rec["steps"].tolist() == [1, 2, 3]
    assert bool(torch.isfinite(rec["values"]).all())
    for other in runs[1:]:
        same(start, other[5])
        same_records(rec, other[0])
        same(st, other[1])
        assert torch.equal(labels, other[2]) and n == other[3] and ex == other[4]


def test_restored_resident_run_continues_bit_for_bit(tmp_path):
    from xggm_amd.vqa.vqacpv2 import save_training_state, load_training_state
    store = _engine_store()
    ma, oa, ta = _engine(BF16, store)
    for k in (0, 1):
        _feed(ta, store, k)
    path = str(tmp_path / "state.pth")
    save_training_state(path, ma, oa, step=2)
    ta.train_log.reset()
    _feed(ta, store, 2)
    mb, ob, tb = _engine(BF16, store)
    _feed(tb, store, 1)  # a history of its own
    assert load_training_state(path, mb, ob) == {"step": 2}
    tb.train_log.reset()
    _feed(tb, store, 2)
    ra, rb = ta.train_log.read(), tb.train_log.read()
    same_records(ra, rb)
    assert ra["steps"].tolist() == [3]
    same(state(ma), state(mb))
    assert torch.equal(ta.static["input_ids"], tb.static["input_ids"]) and torch.equal(ta.static["is_matched"], tb.static["is_matched"])


def test_double_swap_and_dtype_mismatch_are_refused():
    from xggm_amd.engine import CapturedPretrainer
    store = _engine_store()
    model, *_ = _tiny_model("full", compute_dtype=BF16)
    model = model.to(DEV).train()
    batch = store.fill(store.buffers(3), 0, 3, swap=False)
    tr = CapturedPretrainer(model, None, batch, features(), use_graph=False, resident=store)
    with pytest.raises(ValueError, match="swapped twice"):
        tr.load_resident(store, 0)
    tr.load_resident(_engine_store(match_rate=None), 3)  # a store that does not swap under features that do: fine
    assert tr.static["sample"].tolist() == [3, 4, 5] and tr.static["is_matched"].tolist() == [1, 1, 1]
    with pytest.raises(ValueError, match="feature table"):
        CapturedPretrainer(model, None, batch, features(match_rate=None), use_graph=False, resident=_engine_store(feats_bf16=True))
    with pytest.raises(ValueError):
        tr.load_resident(_engine_store(match_rate=None), N_EX - 2)  # the batch would run past the order


# ----------------------------------------------------------------------------- 5. the driver
DRIVER_SEED = 30  # Philox seed of the driver tests' models: the one seed below 40 that meets the conditions both tests assert
N_TRAIN, N_EVAL = 8, 7


def _lx(tmp_path, matched, resident):
    from xggm_amd import param
    from xggm_amd.pretrain.lxmert_pretrain import LXMERT
    flags = ["--taskMaskLM", "--taskObjPredict", "--taskQA", "--epochs", "1", "--lr", "1e-3", "--wordMaskRate", "0.5", "--output",
             str(tmp_path / "snap")] + (["--taskMatched"] if matched else [])
    args = param.parse_args(flags)
    model, *_ = _tiny_model("full", compute_dtype=BF16)
    model = model.to(DEV).train()
    model.seed = DRIVER_SEED
    return LXMERT(_cfg()["cfg"]["T"], model, tok(), args=args, max_labels=K, resident=resident), args


def _shared_images(examples):
    """``_examples`` draws fresh arrays per example; an image has ONE set of arrays: every example takes those of the first
    example of its image, as a data set that looks the image up does"""
    from xggm_amd.pretrain.lxmert_pretrain import image_key
    first = {}
    for ex in examples:
        f = first.setdefault(image_key(ex), ex)
        ex.visual_feats, ex.obj_labels, ex.attr_labels = f.visual_feats, f.obj_labels, f.attr_labels
    return examples


def _stores(args, **kw):
    from xggm_amd.pretrain.resident import ResidentPretrainSet
    c = _cfg()["cfg"]
    mk = lambda ex: ResidentPretrainSet.from_args(args, ex, DEV, tokenizer=tok(), max_seq_length=c["T"], max_labels=K,
                                                  n_answers=c["n_ans"], sid_base=SID, batch_size=3, **kw)
    tr_ex, ev_ex = _shared_images(_examples(N_TRAIN, 41)), _shared_images(_examples(N_EVAL, 42, 100))
    return (tr_ex, mk(tr_ex)), (ev_ex, mk(ev_ex))


class _Evaluator:
    def __init__(self):
        self.seen = []

    def evaluate(self, uid2ans, pprint=False):
        self.seen.append(dict(uid2ans))
        return 0.0


_DATASET = types.SimpleNamespace(answer_table=types.SimpleNamespace(id2ans=lambda i: "ans%d" % i))


def _labelled_rows(store, order):
    return [[bool((store.host["q_label"][s] >= 0).any()) for s in order[i:i + 3]] for i in range(0, len(order), 3)]


def test_an_epoch_over_a_store_equals_the_epoch_over_a_list_loader(tmp_path, capsys):
    """--taskMatched off: ``LXMERT.train`` over a store == the same epoch over a list loader that yields the same examples in
    the store's order (training: 2 whole batches of 8 samples, the tail dropped; validation: 7 samples, the last batch
    ragged): printed lines, answers and every parameter.  The one thing a store changes without a swap is the pool of the
    object masking (every object of the store instead of the batch's own), so the condition this comparison rests on is
    asserted: no object draw of the 5 steps falls into the random-replacement band"""
    (tr_ex, tr_store), (ev_ex, ev_store) = _stores(_lx(tmp_path, False, True)[1])
    B, O = 3, _cfg()["cfg"]["O"]
    for off, rows in enumerate((3, 3, 3, 3, 1)):
        u = R.philox_uniform(DRIVER_SEED, off, SID + 2, rows * O).astype(np.float64)
        assert not ((u < 0.15) & (u / 0.15 >= 0.8) & (u / 0.15 < 0.9)).any(), off
    outs = []
    for resident in (True, False):
        lx, args = _lx(tmp_path, False, resident)
        assert lx.features.match_rate is None
        ev_a, ev_b = _Evaluator(), _Evaluator()
        capsys.readouterr()
        if resident:
            order = lx.resident_order(tr_store, "train", 0)
            assert len(order) == 6 and order.tolist() != sorted(order.tolist())
            lx.train((_DATASET, tr_store, ev_a), (_DATASET, ev_store, ev_b))
            assert lx.engine.static["feat_pool"].data_ptr() == tr_store.tables["feats"].data_ptr()
        else:
            train_ld = [[tr_ex[int(s)] for s in order[i:i + B]] for i in range(0, 6, B)]
            eval_ld = [ev_ex[i:i + B] for i in range(0, N_EVAL, B)]
            lx.train((_DATASET, train_ld, ev_a), (_DATASET, eval_ld, ev_b))
        outs.append((capsys.readouterr().out.splitlines(), ev_a.seen, ev_b.seen, state(lx.model)))
    (out, tr_ans, ev_ans, st), (out2, tr_ans2, ev_ans2, st2) = outs
    assert out[:3] == ["Batch per epoch: 2", "Total Iters: 2", "Warm up Iters: 0"] and len(out) == 7
    assert out == out2 and "nan" not in " ".join(out)
    assert tr_ans == tr_ans2 and ev_ans == ev_ans2
    assert sorted(tr_ans[0]) == sorted(tr_store.uids(order)) and len(ev_ans[0]) == N_EVAL
    same(st, st2)


def test_an_epoch_over_a_swapping_store(tmp_path, capsys):
    """--taskMatched on: the swap is fused into the store's launch (``features`` has none of its own), the losses are finite
    -- the condition, as ``_seed_keeps_a_label`` of tests/test_pretrain_engine_gpu.py: in every step a labelled row keeps its
    sentence --, ``uid2ans`` has the store's uids of the order, and validation with a ragged last batch lands all its answers"""
    lx, args = _lx(tmp_path, True, True)
    (_, tr_store), (_, ev_store) = _stores(args)
    assert tr_store.match_rate == 0.5 and lx.features.match_rate is None
    order = lx.resident_order(tr_store, "train", 0).copy()
    ev_order = lx.resident_order(ev_store, "valid", 0).copy()
    assert len(order) == 6 and ev_order.tolist() == list(range(N_EVAL))
    draws = [R.philox_uniform(DRIVER_SEED, off, SID + 5, 3) for off in range(5)]
    assert _seed_keeps_a_label(_labelled_rows(tr_store, order), draws[:2])
    assert _seed_keeps_a_label(_labelled_rows(ev_store, ev_order), [d[:r] for d, r in zip(draws[2:], (3, 3, 1))])
    ev_a, ev_b = _Evaluator(), _Evaluator()
    capsys.readouterr()
    lx.train((_DATASET, tr_store, ev_a), (_DATASET, ev_store, ev_b))
    out = capsys.readouterr().out.splitlines()
    assert len(out) == 7 and "nan" not in " ".join(out).lower() and "inf" not in " ".join(out).lower()
    from xggm_amd import trainlog as T
    assert sorted(ev_a.seen[0]) == sorted(tr_store.uids(order)) and len(ev_a.seen[0]) == 6
    assert sorted(ev_b.seen[0]) == sorted(ev_store.uids(ev_order)) and len(ev_b.seen[0]) == N_EVAL
    assert int(tr_store.swap_exhausted) + int(ev_store.swap_exhausted) >= 0 and int(lx.model.mlm_overflow or 0) == 0
    # the per-batch interface takes (store, start[, rows]) too
    from xggm_amd.lxrt.optimization import BertAdam
    loss, losses, logit = lx.valid_batch((ev_store, 3))
    assert isinstance(loss, float) and losses.shape == (1, 6) and tuple(logit.shape) == (3, _cfg()["cfg"]["n_ans"])
    # a driver whose features swap as well is refused by the engine
    lx2, _ = _lx(tmp_path, True, False)
    with pytest.raises(ValueError, match="swapped twice"):
        lx2.valid_batch((ev_store, 0))
