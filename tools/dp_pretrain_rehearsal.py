"""Rehearsal of data-parallel LXMERT pre-training on ONE GPU: world size 2 over gloo, both ranks on cuda:0, the TINY model
of oracle/shapes.py with one layer of each kind, all four tasks on, 4 samples per rank out of a resident store of 24.
  python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 tools/dp_pretrain_rehearsal.py
Every check is asserted AND printed by rank 0 (tests/test_pretrain_dp_gpu.py looks for the lines):
  1. after 3 captured steps weights, moments and step counters are torch.equal across the ranks;
  2. the captured and the eager data-parallel run give the same bits;
  3. ONE data-parallel step equals a single-process emulation bit for bit: each rank's half batch through an eager forward
     and backward on a copy of the model with that rank's folded seed, the two gradient arenas added in fp32 (two addends
     commute), scaled by 0.5, then clip and step.  Replicas that never exchanged but saw different data would fail 1.;
     replicas that saw the same data would pass 1., so the halves are asserted to differ;
  4. the folded training log on both ranks equals ``trainlog.fold_host`` over the two rings read separately;
  5. ``LXMERT.train`` for one epoch: rank 0's loss line is the mean of the per-rank step means, the snapshot files are
     written once, and ``evaluate_epoch`` over 9 validation samples (5 + 4: ragged and uneven) scores every uid once;
  6. an ``mlm_capacity`` too small on rank 1 only: both ranks raise the overflow RuntimeError at the same ``check()``;
  7. bf16 storage with ``wire_dtype=torch.bfloat16``: the replicas are identical after 3 steps (no tolerance against the
     fp32 wire is claimed);
  8. the masked-LM and matched tasks off on the bf16 wire (the sparse exchange of the word table): replicas identical,
     captured == eager.
"""
import contextlib
import io
import os
import shutil
import sys
import tempfile
import types

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

DEV = "cuda"
T, O, K, B = 8, 5, 3, 4          # tokens, objects, answer keys, samples per rank
N_OBJ, N_ATTR, N_ANS = 37, 11, 19
N_TRAIN, N_EVAL = 24, 9
MASK_ID, SID = 4, 0x70726500
FOLD = 0x9E3779B97F4A7C15        # the constant enable_data_parallel folds the rank into the seed with


def cfg():
    from oracle import shapes
    return dict(shapes.TINY, l_layers=1, x_layers=1, r_layers=1)


class Tok:
    """whitespace tokenizer over a vocabulary that fits TINY's 64 rows"""

    def __init__(self):
        words = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"] + ["w%d" % i for i in range(5, cfg()["vocab"])]
        self.vocab = {w: i for i, w in enumerate(words)}

    def tokenize(self, s):
        return s.split()

    def convert_tokens_to_ids(self, tokens):
        return [self.vocab.get(t, 1) for t in tokens]


def examples(n, seed, first_uid=0):
    """n labelled examples over n // 2 images (two sentences per image: the swap finds other images)"""
    from xggm_amd.pretrain.lxmert_pretrain import InputExample
    c = cfg()
    r = np.random.default_rng(seed)
    imgs = [(r.random((O, c["feat_dim"]), dtype=np.float32), r.random((O, 4), dtype=np.float32),
             (r.integers(0, N_OBJ, size=O), r.random(O, dtype=np.float32)),
             (r.integers(0, N_ATTR, size=O), r.random(O, dtype=np.float32))) for _ in range(max(n // 2, 1))]
    labels = [{3: 0.3, 7: 0.6, 11: 1.0}, {5: 1.0}, {2: 0.9, 13: 0.3}]
    out = []
    for i in range(n):
        f, b, ol, al = imgs[i % len(imgs)]
        sent = " ".join("w%d" % w for w in r.integers(5, c["vocab"], size=int(r.integers(2, T - 1))))
        out.append(InputExample("img%d_vqa_%03d" % (i % len(imgs), first_uid + i), sent, (f, b), ol, al, 1, labels[i % 3]))
    return out


def build_model(dt, seed, mask_lm=True, mlm_capacity=None):
    """``mask_lm`` False: the two heads of ``cls`` are both off (masked LM and matched), so its arena group takes no part"""
    from xggm_amd import synth
    from xggm_amd.lxrt import modeling as M
    c = cfg()
    vc = M.VISUAL_CONFIG
    vc.l_layers, vc.x_layers, vc.r_layers = c["l_layers"], c["x_layers"], c["r_layers"]
    vc.obj_id_num, vc.attr_id_num = N_OBJ, N_ATTR
    vc.set_visual_dims(c["feat_dim"], 4)
    vc.visual_losses = ["obj", "attr", "feat"]
    F = c["feat_dim"]
    vc.visual_loss_config = {"obj": (N_OBJ, "ce", (-1,), 1 / 0.15), "attr": (N_ATTR, "ce", (-1,), 1 / 0.15),
                             "feat": (F, "l2", (-1, F), 1 / 0.15)}
    bc = M.BertConfig(c["vocab"], hidden_size=c["hidden"], num_attention_heads=c["heads"], intermediate_size=c["inter"],
                      max_position_embeddings=c["max_pos"])
    model = M.LXRTPretraining(bc, task_mask_lm=mask_lm, task_matched=mask_lm, visual_losses="obj,attr,feat", task_qa=True, num_answers=N_ANS,
                              mlm_capacity=mlm_capacity, compute_dtype=dt)
    tied = "bert.embeddings.word_embeddings.weight"
    model.load_state_dict({k: torch.from_numpy(synth.seeded_param(tied if k == "cls.predictions.decoder.weight" else k, v.shape, 5))
                           for k, v in model.state_dict().items()})
    model = model.to(DEV).train()
    model.seed = seed
    return model


def flags(out_dir="snap"):
    from xggm_amd import param
    return param.parse_args(["--taskMatched", "--taskMaskLM", "--taskObjPredict", "--taskQA", "--epochs", "1", "--lr", "1e-3",
                             "--wordMaskRate", "0.5", "--output", out_dir])


def make_store(args, ex):
    from xggm_amd.pretrain.resident import ResidentPretrainSet
    return ResidentPretrainSet.from_args(args, ex, DEV, tokenizer=Tok(), max_seq_length=T, max_labels=K, n_answers=N_ANS,
                                         vocab_size=cfg()["vocab"], sid_base=SID, batch_size=B)


def features(args):
    from xggm_amd.pretrain.lxmert_pretrain import DeviceFeatures
    return DeviceFeatures.from_args(args, swap=False, vocab_size=cfg()["vocab"], mask_id=MASK_ID, max_labels=K, sid_base=SID)


def folded_seed(seed, rank):
    return (seed + rank * FOLD) & 0x7FFFFFFFFFFFFFFF


def pick_seed(world):
    """the first model seed with which, on every rank and in each of the first 12 steps, at least one of a batch's rows keeps
    its sentence (every example carries an answer label; a batch whose rows were ALL swapped has no QA label left and its
    QA loss is 0 / 0 = NaN, as the reference's CrossEntropyLoss(ignore_index=-1) gives -- faithful, but bit comparisons
    want finite values).  The swap draws u_swap at Philox stream SID + 5 of the rank's folded seed."""
    import pretrain_mask_ref as R
    for seed in range(1, 200):
        if all(float(R.philox_uniform(folded_seed(seed, r), off, SID + 5, B).max()) >= 0.5 for r in range(world) for off in range(12)) \
                and float(R.philox_uniform(seed, 4, SID + 5, 1)[0]) >= 0.5:  # rank 0's ragged validation batch: ONE row
            return seed
    raise RuntimeError("no seed found")


def state(model):
    from xggm_amd.runtime import runtime_of
    rt = runtime_of(model)
    torch.cuda.synchronize()
    out = {"p." + k: v.detach().clone() for k, v in model.named_parameters()}
    out.update(m=rt.arena.m.clone(), v=rt.arena.v.clone(), steps=rt.arena.steps.clone())
    return out


def flat(st):
    return torch.cat([st[k].detach().double().flatten() for k in sorted(st)])


def bits_equal(a, b):
    """torch.equal key by key (NaN-free states: asserted by the callers)"""
    return sorted(a) == sorted(b) and all(torch.equal(a[k], b[k]) for k in a)


def all_ranks(v):
    parts = [torch.empty_like(v) for _ in range(dist.get_world_size())]
    dist.all_gather(parts, v)
    return parts


def agree(ok):
    """True only when ``ok`` holds on every rank"""
    t = torch.tensor([1 if ok else 0])
    dist.all_reduce(t, op=dist.ReduceOp.MIN)
    return bool(t.item())


def say(rank, msg):
    if rank == 0:
        print(msg, flush=True)


def engine(args, store, dt, seed, use_graph=True, wire=None, steps=3, fold=False, mask_lm=True, mlm_capacity=None, warmup=0.0,
           check_every=None):
    """a data-parallel engine on this rank's share of epoch 0, ``steps`` steps -> (model, trainer, own ring, folded ring)"""
    from xggm_amd.engine import AnswerLog, CapturedPretrainer, TrainLog
    from xggm_amd.lxrt.optimization import BertAdam
    from xggm_amd.pretrain.lxmert_pretrain import enable_data_parallel
    rank, world = dist.get_rank(), dist.get_world_size()
    model = build_model(dt, seed, mask_lm=mask_lm, mlm_capacity=mlm_capacity)
    optim = BertAdam(list(model.parameters()), lr=1e-3, warmup=warmup, t_total=20)  # warmup 0: the first step moves the weights
    enable_data_parallel(model, wire_dtype=wire, check_every=check_every, check_level="state")
    store.order(0, shuffle=True, seed=9, rank=rank, world=world, drop_last=True, batch_size=B)
    first = store.fill(store.buffers(B), 0, B, swap=False)
    tr = CapturedPretrainer(model, optim, first, features(args), use_graph=use_graph, warmup_iters=1, resident=store,
                            train_log=TrainLog(8, DEV), valid_log=TrainLog(8, DEV),
                            answer_log=AnswerLog(64, DEV, with_scores=False))
    for k in range(steps):
        tr.load_resident(store, B * k)
        tr.step()
    own = folded = None
    if fold:
        own = tr.train_log.read()
        folded = tr.train_log.fold(steps)
    return model, tr, own, folded


def emulate_one_step(args, store, dt, seed):
    """check 3: the single-process emulation of ONE data-parallel step, on this rank alone -> (state, the halves differ)"""
    from xggm_amd.engine import CapturedPretrainer
    from xggm_amd.lxrt.optimization import BertAdam
    from xggm_amd.runtime import runtime_of
    from xggm_amd.vqa.vqacpv2 import clip_and_step
    rank, world = dist.get_rank(), dist.get_world_size()
    grads, samples, mine = [], [], None
    for r in range(world):
        model = build_model(dt, seed)
        optim = BertAdam(list(model.parameters()), lr=1e-3, warmup=0.0, t_total=20)
        rt = runtime_of(model)
        rt.rng[0] = folded_seed(seed, r)
        rt.arena.sq_enabled = False       # as under data parallelism: the norm is read from the gradient buffer ...
        rt.arena.row_list_enabled = False  # ... and the word table's gradient is cleared as a whole
        store.order(0, shuffle=True, seed=9, rank=r, world=world, drop_last=True, batch_size=B)
        b = store.fill(store.buffers(B), 0, B, rng=rt.rng, sid_base=SID)
        samples.append(b["sample"].tolist())
        feat = features(args)
        total, losses, ans = model(*feat(*[b[k] for k in CapturedPretrainer.KEYS], rt.rng, pool=store.feat_pool(), img_ids=b["img_ids"]))
        rt.backward(total)
        grads.append(rt.arena.grads.clone())
        if r == rank:
            mine = (model, optim, rt)
    model, optim, rt = mine
    g = grads[0]
    for other in grads[1:]:
        g = g + other
    rt.arena.grads.copy_(g * 0.5)
    clip_and_step(model, optim, 1.0, advance=True)
    return state(model), samples[0] != samples[1] and not torch.equal(grads[0], grads[1])


def finite(st):
    return all(bool(torch.isfinite(v).all()) for v in st.values() if v.is_floating_point())


def check_engine(args, store, seed):
    """checks 1 - 4"""
    from xggm_amd import trainlog as TL
    rank = dist.get_rank()
    F32 = torch.float32
    m_c, tr_c, own, folded = engine(args, store, F32, seed, use_graph=True, fold=True)
    st_c = state(m_c)
    assert finite(st_c) and bool(torch.isfinite(own["values"]).all()), "a non-finite loss: the seed was meant to prevent it"
    same = all(torch.equal(p, all_ranks(flat(st_c))[0]) for p in all_ranks(flat(st_c)))
    say(rank, "1. replicas identical after 3 captured steps (weights, moments, step counters): %s" % same)
    assert same, "replicas diverged: the gradient exchange did not happen"
    assert isinstance(tr_c.graphs["train"], tuple) and len(tr_c.graphs["train"]) == 3  # forward + backward | update
    assert int(st_c["steps"].max()) == 3

    m_e, tr_e, own_e, _ = engine(args, store, F32, seed, use_graph=False, fold=True)
    ok = agree(bits_equal(st_c, state(m_e)) and all(torch.equal(own[k], own_e[k]) for k in ("values", "steps", "kinds", "present")))
    say(rank, "2. captured == eager under data parallelism, bit for bit: %s" % ok)
    assert ok

    m_1, *_ = engine(args, store, F32, seed, use_graph=True, steps=1)
    st_1 = state(m_1)
    emu, differ = emulate_one_step(args, store, F32, seed)
    moved = not torch.equal(st_1["p.bert.encoder.layer.0.attention.self.query.weight"],
                            state(build_model(F32, seed))["p.bert.encoder.layer.0.attention.self.query.weight"])
    ok = agree(bits_equal(st_1, emu) and finite(emu) and moved)
    differ = agree(differ)
    say(rank, "3. one data-parallel step == the single-process emulation (halves differ: %s), bit for bit: %s" % (differ, ok))
    if not ok:
        for k in sorted(st_1):
            if not torch.equal(st_1[k], emu[k]):
                print("   rank %d differs in %s: max |d| %.3e" % (rank, k, float((st_1[k].double() - emu[k].double()).abs().max())), flush=True)
    assert ok and differ

    # 4. the two rings read separately (before the fold) against the restatement, and the fold's own read-back
    rings = [None] * dist.get_world_size()
    dist.all_gather_object(rings, {k: own[k].numpy() for k in ("values", "kinds", "present", "steps")})
    want = TL.fold_host(np.stack([r["values"] for r in rings]), np.stack([r["kinds"] for r in rings]),
                        np.stack([r["present"] for r in rings]), np.stack([r["steps"] for r in rings]), cursor=3)
    ok = (want["flag"] == -1 and np.array_equal(folded["values"].numpy(), want["values"])
          and np.array_equal(folded["present"].numpy(), want["present"]) and np.array_equal(folded["kinds"].numpy(), want["kinds"])
          and np.array_equal(folded["sums"].numpy(), want["sums"]) and np.array_equal(folded["counts"].numpy(), want["counts"])
          and int(folded["first_bad"]) == want["first_bad"] and folded["steps"].tolist() == [1, 2, 3]
          and not np.array_equal(rings[0]["values"], rings[1]["values"]))
    ok = agree(ok)
    say(rank, "4. folded training log == the restatement over the two rings, on both ranks: %s" % ok)
    assert ok


class Evaluator:
    def __init__(self):
        self.seen = []

    def evaluate(self, uid2ans, pprint=False):
        self.seen.append(dict(uid2ans))
        return 0.0


DATASET = types.SimpleNamespace(answer_table=types.SimpleNamespace(id2ans=lambda i: "ans%d" % i))


def check_driver(seed):
    """check 5"""
    from xggm_amd import trainlog as TL
    from xggm_amd.engine import TrainLog
    from xggm_amd.pretrain.lxmert_pretrain import LXMERT, enable_data_parallel
    rank, world = dist.get_rank(), dist.get_world_size()
    box = [tempfile.mkdtemp(prefix="dp_pretrain_") if rank == 0 else None]
    dist.broadcast_object_list(box, src=0)
    args = flags(os.path.join(box[0], "snap"))
    tr_store, ev_store = make_store(args, examples(N_TRAIN, 41)), make_store(args, examples(N_EVAL, 42, 100))
    model = build_model(torch.float32, seed)
    enable_data_parallel(model)
    lx = LXMERT(T, model, Tok(), args=args, max_labels=K, vocab_size=cfg()["vocab"], mask_id=MASK_ID, resident=True)
    # observers: every rank's own ring as it was before each fold, its own answers before each merge, its snapshot writes
    rings, own_answers, writes = [], [], []
    fold, merge, save = TrainLog.fold, lx._merge_ranks, torch.save

    def watching_fold(self, n, group=None):
        rings.append(self.read())
        return fold(self, n, group)

    def watching_merge(uid2ans):
        own_answers.append(dict(uid2ans))
        return merge(uid2ans)

    def watching_save(obj, path, *a, **k):
        writes.append(os.path.basename(path))
        return save(obj, path, *a, **k)

    TrainLog.fold, lx._merge_ranks, torch.save = watching_fold, watching_merge, watching_save
    ev_a, ev_b = Evaluator(), Evaluator()
    printed = io.StringIO()
    try:
        with contextlib.redirect_stdout(printed):
            lx.train((DATASET, tr_store, ev_a), (DATASET, ev_store, ev_b))
    finally:
        TrainLog.fold, torch.save = fold, save
    lines = printed.getvalue().splitlines()
    dist.barrier()
    # the loss line: every rank's step means, gathered; their mean as the fold takes it, and as plain fp64 arithmetic
    assert len(rings) == 1 and int(rings[0]["cursor"]) == 3
    per_rank = [None] * world
    dist.all_gather_object(per_rank, rings[0]["values"][:, TL.LOSS].numpy())
    assert all(np.isfinite(v).all() for v in per_rank)
    step_means = (per_rank[0] + per_rank[1]) * np.float32(0.5)          # fp32, per step: what the fold leaves
    line = "The training loss for Epoch 0 is %0.4f" % (float(step_means.astype(np.float64).sum()) / 3)
    plain = float(np.mean([np.mean(v.astype(np.float64)) for v in per_rank]))  # the mean of the per-rank step means
    if rank == 0:
        ok = (lines[:3] == ["Batch per epoch: 3", "Total Iters: 3", "Warm up Iters: 0"] and lines[3] == line
              and abs(plain - float(step_means.astype(np.float64).sum()) / 3) < 1e-6 * abs(plain) and len(lines) == 7
              and lines[5].startswith("The valid loss is "))
    else:
        ok = lines == []  # only rank 0 prints
    ok = agree(ok)
    say(rank, "5. LXMERT.train: rank 0's loss line == the mean of the per-rank step means: %s  (%s)" % (ok, line))
    if not ok:
        print("rank %d printed %r" % (rank, lines), flush=True)
    assert ok
    files = sorted(os.listdir(args.output)) if rank == 0 else []
    # (BEST_EVAL_LOSS is written when the validation loss is a number: a validation batch whose rows were all swapped has
    # a NaN QA loss, as in the reference)
    ok = agree((sorted(writes) == files and len(set(writes)) == len(writes) and "Epoch01_LXRT.pth" in files) if rank == 0
               else writes == [])
    say(rank, "5. snapshots written once, by rank 0: %s" % ok)
    assert ok
    # answers: the training sweep's (24 samples, 12 per rank) and the validation sweep's (9 samples: 5 + 4)
    lens = [None] * world
    dist.all_gather_object(lens, [len(a) for a in own_answers])
    ev_uids = ev_store.uids(range(N_EVAL))
    if rank == 0:
        ok = (lens == [[12, 5], [12, 4]] and len(ev_a.seen) == 1 and len(ev_a.seen[0]) == 24 and len(ev_b.seen) == 1
              and sorted(ev_b.seen[0]) == sorted(ev_uids) and len(set(ev_uids)) == N_EVAL
              and sorted(own_answers[1]) == sorted(ev_uids[:5]))
    else:
        ok = ev_a.seen == [] and ev_b.seen == [] and sorted(own_answers[1]) == sorted(ev_uids[5:])
    ok = agree(ok)
    say(rank, "5. evaluate_epoch over 9 samples (5 + 4, ragged): every uid scored exactly once: %s" % ok)
    assert ok
    # the replicas are still equal after the driver's epoch
    v = flat(state(model))
    assert all(torch.equal(p, all_ranks(v)[0]) for p in all_ranks(v))
    dist.barrier()
    if rank == 0:
        shutil.rmtree(box[0], ignore_errors=True)


def check_overflow(args, store, seed):
    """check 6: a raised Python error on a set flag, not a device fault"""
    rank = dist.get_rank()
    model, tr, _, _ = engine(args, store, torch.float32, seed, steps=1, mlm_capacity=1 if rank == 1 else None)
    local = int(model.mlm_overflow.item() != 0)
    raised = ""
    try:
        tr.check()
    except RuntimeError as e:
        raised = str(e)
    every = [None] * dist.get_world_size()
    dist.all_gather_object(every, (local, raised.startswith("masked-LM overflow")))
    ok = every == [(0, True), (1, True)]  # set on rank 1 alone, raised on both
    tr.check()  # the flag was cleared on both: the next read-back is quiet, and the group still answers
    say(rank, "6. an overflow on rank 1 alone raises on both ranks at the same check(): %s" % ok)
    assert ok


def check_bf16_wire(args, store, seed):
    """checks 7 and 8"""
    from xggm_amd.runtime import runtime_of
    rank = dist.get_rank()
    BF16 = torch.bfloat16
    model, tr, own, _ = engine(args, store, BF16, seed, wire=BF16, fold=True, check_every=1)
    rt = runtime_of(model)
    assert model._replica_guard.checks == 3  # the drift guard compared the replicas after every step and stayed quiet
    assert rt.arena.wire is not None and model._grad_sync.arena is rt.arena  # exchanged in place on the wire arena
    st = state(model)
    st["shadow"] = rt.arena.shadow.float().clone()
    assert finite(st) and bool(torch.isfinite(own["values"]).all())
    v = flat(st)
    same = all(torch.equal(p, all_ranks(v)[0]) for p in all_ranks(v))
    say(rank, "7. bf16 storage, bf16 wire: replicas identical after 3 steps: %s" % same)
    assert same
    out = []
    for use_graph in (True, False):
        model, tr, own, _ = engine(args, store, BF16, seed, use_graph=use_graph, wire=BF16, fold=True, mask_lm=False)
        assert getattr(model._grad_sync, "table", None) is not None  # the sparse exchange of the word table is on
        assert not bool(own["present"][:, 1:3].any())  # no Mask_LM, no Matched column
        st = state(model)
        st["shadow"] = runtime_of(model).arena.shadow.float().clone()
        assert finite(st)
        out.append(st)
    v = flat(out[0])
    same = agree(all(torch.equal(p, all_ranks(v)[0]) for p in all_ranks(v)) and bits_equal(out[0], out[1]))
    say(rank, "8. masked-LM off, sparse word-table exchange on the bf16 wire: replicas identical, captured == eager: %s" % same)
    assert same


def main():
    rank = int(os.environ["RANK"])
    torch.cuda.set_device(0)
    dist.init_process_group("gloo")
    world = dist.get_world_size()
    assert world == 2, "the rehearsal is written for two ranks"
    seed = pick_seed(world)
    args = flags()
    store = make_store(args, examples(N_TRAIN, 41))
    assert store.match_rate == 0.5
    check_engine(args, store, seed)
    check_driver(seed)
    check_overflow(args, store, seed)
    check_bf16_wire(args, store, seed)
    dist.barrier()
    dist.destroy_process_group()
    say(rank, "process group shut down cleanly")


if __name__ == "__main__":
    main()
