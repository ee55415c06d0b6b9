"""Rehearsal of the data-parallel fine-tuning drivers (``VQA`` / ``GQA`` with ``data_parallel=True``) on ONE GPU: world size 2
over gloo, both ranks on cuda:0, the tiny model of the driver tests, a resident store of 24 training samples at 4 per rank
(3 global steps) and 9 validation samples (5 + 4: uneven slices), one question id on both sides of the rank boundary.
  python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 tools/dp_finetune_rehearsal.py
Every check is asserted AND printed by rank 0 (tests/test_finetune_dp_gpu.py looks for the lines):
  1. after one epoch of ``VQA.train`` weights, moments and step counters are torch.equal across the ranks (which took
     DIFFERENT rows of every global step);
  2. ``history``, ``valid_scores`` and ``best_valid`` are equal on both ranks;
  3. ``log.log`` and the ``BEST*.pth`` files are written once, by rank 0;
  4. ``total_loss`` equals the value rebuilt from the two rings with ``trainlog.fold_host``;
  5. the train score is bit-equal to ``answers.score_host`` over the merged labels in the global order and within 2^-24 of
     ``evaluator.evaluate`` on the merged ``quesid2ans``;
  6. validation: every question is scored once, the merged labels are the ranks' own in slice order, the score is bit-equal
     on both ranks;
  7. ``predict(dump=)`` writes one file;
  8. a refused-append flag planted on rank 1 raises on both ranks at the same fold;
  9. the ``GQA`` driver (GGM pass first, validation at twice the batch size) completes one epoch with equal replicas;
 10. without ``data_parallel=True`` the prepared model is still refused.
"""
import contextlib
import datetime
import io
import os
import pathlib
import random
import shutil
import sys
import tempfile

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

DEV = "cuda"
TOL = 2.0 ** -24  # one fp32 rounding of a score <= 1: the bound INTEGRATION.md states for the device score
N_TRAIN, N_VALID = 24, 9


def say(rank, msg):
    if rank == 0:
        print(msg, flush=True)


def agree(ok):
    """True only when ``ok`` holds on every rank"""
    t = torch.tensor([1 if ok else 0])
    dist.all_reduce(t, op=dist.ReduceOp.MIN)
    return bool(t.item())


def every(obj):
    out = [None] * dist.get_world_size()
    dist.all_gather_object(out, obj)
    return out


def replicas_equal(model):
    from xggm_amd.runtime import runtime_of
    rt = runtime_of(model)
    torch.cuda.synchronize()
    v = torch.cat([p.detach().double().flatten() for _, p in sorted(model.named_parameters())]
                  + [rt.arena.m.double().flatten(), rt.arena.v.double().flatten(), rt.arena.steps.double().flatten()]).cpu()
    parts = [torch.empty_like(v) for _ in range(dist.get_world_size())]
    dist.all_gather(parts, v)
    return bool(torch.isfinite(v).all()) and all(torch.equal(parts[0], p) for p in parts[1:])


def stores(tmp, kind, cfg, n_train):
    """the splits of tests/test_finetune_driver_gpu.py as resident stores; the validation split's sample 5 is made a second
    copy of sample 4 (same question id, image and labels): the id then lies on both sides of the 5 + 4 rank boundary"""
    import test_finetune_driver_gpu as T
    from xggm_amd.lxrt.entry import SentenceBatcher
    from xggm_amd.tools.resident import ResidentDataset, group_ids
    batcher = SentenceBatcher(T._tok(), 20)
    out = {}
    with contextlib.redirect_stdout(io.StringIO()):  # the data sets print their sizes on every rank
        for name, n_q, seed in (("train", n_train, 21), ("valid", N_VALID, 22)):
            dset, ts, ev = T._split(tmp, kind, name, 6, n_q, cfg["feat_dim"], cfg["vocab"], seed, many=name == "valid")
            if name == "valid" and kind == "vqa":
                ts.data[5], ts.rows[5] = ts.data[4], ts.rows[4]
            store = ResidentDataset(ts, batcher, DEV, groups=group_ids(ts.data, "answer_type"), chunk_bytes=1 << 16)
            out[name] = (dset, store, ev)
    return out


def flags(out_dir):
    from xggm_amd import param
    return param.parse_args(["--bs", "4", "--epochs", "1", "--lr", "1e-4", "--seed", "4", "--output", out_dir])


class Watch:
    """observers around one driver call: every rank's own ring before each ``TrainLog.fold``, its own answers before and the
    merged ones behind each ``AnswerLog.fold``, its snapshot writes; ``plant``: rank 1 raises its log's refused-append flag
    in front of the next answer fold"""

    def __init__(self, plant=False):
        self.rings, self.own, self.merged, self.layouts, self.writes, self.plant = [], [], [], [], [], plant

    def __enter__(self):
        from xggm_amd.engine import AnswerLog, TrainLog
        self.saved = (TrainLog.fold, AnswerLog.fold, torch.save)
        t_fold, a_fold, save = self.saved
        watch = self

        def train_fold(log, n, group=None):
            watch.rings.append(log.read())
            return t_fold(log, n, group)

        def answer_fold(log, layout, expect, block=None, group=None):
            if watch.plant and dist.get_rank() == 1:
                log.flags.fill_(3)  # bit 0: an append did not fit; the bits above it: one refused append
                watch.plant = False
            else:
                watch.own.append(log.read()[0].clone())
            out = a_fold(log, layout, expect, block=block, group=group)
            watch.merged.append(out.read()[0].clone())
            watch.layouts.append(layout)
            return out

        def watching_save(obj, path, *a, **k):
            watch.writes.append(os.path.basename(str(path)))
            return save(obj, path, *a, **k)

        TrainLog.fold, AnswerLog.fold, torch.save = train_fold, answer_fold, watching_save
        return self

    def __exit__(self, *a):
        from xggm_amd.engine import AnswerLog, TrainLog
        TrainLog.fold, AnswerLog.fold, torch.save = self.saved


def check_vqa(box):
    import test_finetune_driver_gpu as T
    from xggm_amd import answers as A, ops, trainlog as TL
    from xggm_amd.dist import shard_range
    from xggm_amd.engine import TrainLog
    from xggm_amd.vqa.vqacpv2 import VQA, enable_data_parallel
    rank, world = dist.get_rank(), dist.get_world_size()
    cfg, model = T._model()
    st = stores(pathlib.Path(tempfile.mkdtemp(prefix="shards_", dir=box)), "vqa", cfg, N_TRAIN)
    (dset, store, ev), (vset, vstore, vev) = st["train"], st["valid"]
    assert len(store) == N_TRAIN and len(vstore) == N_VALID
    args = flags(os.path.join(box, "snap_vqa"))
    enable_data_parallel(model)

    # 10. (first: nothing has run yet) the prepared model without the keyword
    try:
        VQA(model, st["train"], st["valid"], args=args)
        refused = False
    except NotImplementedError as e:
        refused = "enable_data_parallel" in str(e)

    printed = io.StringIO()
    random.seed(7 + rank)  # only rank 0's draws may count
    with contextlib.redirect_stdout(printed):
        drv = VQA(model, st["train"], st["valid"], args=args, valid_batch_size=4, data_parallel=True)
        with Watch() as w:
            drv.train(st["train"], st["valid"])
    lines = printed.getvalue()
    B, steps = drv.B, N_TRAIN // (4 * world)
    assert steps == 3

    # 1.
    perm = np.random.default_rng([args.seed, 0]).permutation(N_TRAIN)
    mine = store.order(0, shuffle=True, seed=args.seed, rank=rank, world=world, batch_size=B)
    slices = every(mine.tolist())
    differ = not set(slices[0]) & set(slices[1]) and sorted(slices[0] + slices[1]) == sorted(perm.tolist())
    same = agree(replicas_equal(model) and differ)
    say(rank, "1. replicas identical after one epoch of VQA.train (the ranks' rows differ: %s): %s" % (differ, same))
    assert same

    # 2.
    seen = every((drv.history, drv.valid_scores, drv.best_valid, drv.sweeps, drv.total_loss))
    ok = agree(seen[0] == seen[1] and len(drv.history) == 1 and len(drv.valid_scores) == 4 and drv.best_valid == max(drv.valid_scores)
               and drv.best_valid > 0)
    say(rank, "2. history, valid_scores and best_valid equal on both ranks: %s" % ok)
    assert ok, seen

    # 3.
    files = sorted(os.listdir(args.output)) if rank == 0 else []
    if rank == 0:
        text = open(os.path.join(args.output, "log.log")).read()
        h = drv.history[0]
        ok = (files == ["BEST.pth", "BEST_0.pth", "log.log"] and set(w.writes) == {"BEST.pth", "BEST_0.pth"}
              and w.writes.count("BEST_0.pth") == 1
              and text == "\nEpoch 0: Train %.2f\n\nEpoch 0: Valid %.2f\nEpoch 0: Best %.2f\n" % (h["train"], h["valid"] * 100., h["best"] * 100.)
              and "BertAdam Total Iters: 3\n" in lines and text in lines and lines.count(": Valid ") == 4)
    else:
        ok = w.writes == [] and "Epoch" not in lines and "Total Iters" not in lines  # rank 0 alone prints, writes and saves
    ok = agree(ok)
    say(rank, "3. log.log and the BEST*.pth files written once, by rank 0: %s" % ok)
    assert ok, (rank, files, w.writes, lines)

    # 4. val_schedule(3) validates after every iteration: three folds of one iteration's two records
    rings = every([{k: r[k].numpy() for k in ("values", "kinds", "present", "steps")} for r in w.rings])
    total, n_rec = 0.0, 0
    for k in range(len(w.rings)):
        both = [rings[r][k] for r in range(world)]
        want = TL.fold_host(np.stack([b["values"] for b in both]), np.stack([b["kinds"] for b in both]),
                            np.stack([b["present"] for b in both]), np.stack([b["steps"] for b in both]))
        assert want["flag"] == -1
        n_rec += len(want["kinds"])
        for j in np.nonzero(want["kinds"] == TrainLog.PLAIN)[0]:
            total += float(want["values"][j, TrainLog.LOSS]) / B
    ok = agree(total == drv.total_loss and n_rec == 2 * steps and total > 0
               and not np.array_equal(rings[0][0]["values"], rings[1][0]["values"]))
    say(rank, "4. total_loss == the value rebuilt from the two rings with trainlog.fold_host: %s" % ok)
    assert ok, (total, drv.total_loss, n_rec)

    # 5. the epoch's merged answers, in the global order
    il = [i for i, l in enumerate(w.layouts) if l == ops.FOLD_INTERLEAVE]
    assert len(il) == 1 and w.layouts.count(ops.FOLD_CONCAT) == 4
    labels = w.merged[il[0]].numpy()
    gorder = perm[:steps * B * world]
    own = every(w.own[il[0]].numpy())
    rebuilt = np.stack([o.reshape(steps, B) for o in own], axis=1).reshape(-1)  # step, rank, row
    words = A.score_host(labels, store.host, order=gorder, keep=A.last_occurrence_mask(store.qid_index[gorder]), cursor=len(labels))
    host_score = A.decode_score(words, 0)["score"] * 100.
    ev_score = ev.evaluate(A.to_quesid2ans(store.ques_ids(gorder), labels, dset.label2ans))
    ok = agree(np.array_equal(labels, rebuilt) and host_score == drv.history[0]["train"]
               and abs(drv.history[0]["train"] / 100. - ev_score) <= TOL)
    say(rank, "5. train score bit-equal to score_host over the merged labels, within 2^-24 of the evaluator: %s" % ok)
    assert ok, (host_score, drv.history[0]["train"], ev_score)

    # 6. a sweep of its own
    with Watch() as w:
        score = drv.evaluate(st["valid"])
        by = drv.evaluate(st["valid"], by_group=True)
    own = every(w.own[0].numpy())
    counts = [len(shard_range(N_VALID, r, world)) for r in range(world)]
    merged = drv.predictor.log._merged
    res = merged.score_store(vstore, keep=vstore.keep_mask())
    qids = vstore.ques_ids(range(N_VALID))
    quesid2ans = A.to_quesid2ans(qids, w.merged[0], vset.label2ans)
    scores = every((score, by))
    ok = agree(counts == [5, 4] and [len(o) for o in own] == counts and np.array_equal(np.concatenate(own), w.merged[0].numpy())
               and qids[4] == qids[5] and len(set(qids)) == N_VALID - 1 and res["count"] == N_VALID - 1 and res["score"] == score
               and scores[0] == scores[1] and by["all"] == score and abs(score - vev.evaluate(quesid2ans)) <= TOL
               and score == drv.valid_scores[-1])
    say(rank, "6. validation (5 + 4): every question scored once, merged labels == the ranks' own in slice order, the score "
              "bit-equal on both ranks: %s" % ok)
    assert ok, (counts, res, scores)

    # 7.
    dump = os.path.join(box, "dump_rank%d.json" % rank)
    got = drv.predict(st["valid"], dump=dump)
    dist.barrier()
    ok = agree(got == quesid2ans and os.path.exists(dump) == (rank == 0) and not os.path.exists(os.path.join(box, "dump_rank1.json")))
    say(rank, "7. predict(dump=) writes one file, the same dict on both ranks: %s" % ok)
    assert ok

    # 8.
    raised = ""
    with Watch(plant=True):
        try:
            drv.evaluate(st["valid"])
        except RuntimeError as e:
            raised = str(e)
    seen = every(raised)
    ok = all(s.startswith("answer log fold: a rank's log refused appends") and "lowest such rank is 1" in s for s in seen)
    again = drv.evaluate(st["valid"])  # the next sweep resets the log: the group still answers
    ok = agree(ok and again == score)
    say(rank, "8. a refused-append flag on rank 1 alone raises on both ranks at the same fold: %s" % ok)
    assert ok, seen
    return refused


def check_gqa(box):
    import test_finetune_driver_gpu as T
    from xggm_amd.gqa.gqa_ood import GQA
    from xggm_amd.vqa.vqacpv2 import enable_data_parallel
    rank = dist.get_rank()
    cfg, model = T._model()
    st = stores(pathlib.Path(tempfile.mkdtemp(prefix="shards_", dir=box)), "gqa", cfg, 12)  # a datum per label: 24 samples
    assert len(st["train"][1]) == N_TRAIN and len(st["valid"][1]) == 99
    enable_data_parallel(model)
    random.seed(3 + rank)
    with contextlib.redirect_stdout(io.StringIO()):
        drv = GQA(model, st["train"], st["valid"], args=flags(os.path.join(box, "snap_gqa")), data_parallel=True)
        drv.train(st["train"], st["valid"])
    assert drv.valid_B == 8 and drv.order == "gqa"
    seen = every((drv.history, drv.valid_scores))
    ok = agree(replicas_equal(model) and seen[0] == seen[1] and len(drv.history) == 1 and drv.sweeps == 4)
    say(rank, "9. the GQA driver (GGM pass first, valid_factor 2) completes one epoch with equal replicas: %s" % ok)
    assert ok


def main():
    rank = int(os.environ["RANK"])
    torch.cuda.set_device(0)
    # a short timeout: a rank that died ends its peer instead of hanging it
    dist.init_process_group("gloo", timeout=datetime.timedelta(seconds=120))
    assert dist.get_world_size() == 2, "the rehearsal is written for two ranks"
    box = [tempfile.mkdtemp(prefix="dp_finetune_") if rank == 0 else None]
    dist.broadcast_object_list(box, src=0)
    try:
        refused = check_vqa(box[0])
        check_gqa(box[0])
        ok = agree(refused)
        say(rank, "10. without data_parallel=True the prepared model is still refused: %s" % ok)
        assert ok
        dist.barrier()
    finally:
        if rank == 0:
            shutil.rmtree(box[0], ignore_errors=True)
    dist.destroy_process_group()
    say(rank, "process group shut down cleanly")


if __name__ == "__main__":
    main()
