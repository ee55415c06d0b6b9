"""Rehearsal of the replica drift guard (dist.ReplicaGuard) on ONE GPU: world size 2 over gloo, both ranks on cuda:0, a
tiny model, DIFFERENT batches per rank, four iterations per configuration with ``enable_data_parallel(check_every=1)``:
the eager loop ``vqacpv2.train_iteration`` and the captured engine ``CapturedTrainer.iteration``, each under the
replicated and the sharded update.
  python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 tools/dp_drift_rehearsal.py [--drift master]
--drift none     no alarm may be raised; prints the number of checks per configuration (4) and exits 0.
--drift master   between iterations 2 and 3 rank 1 overwrites ONE element of the fp32 master of a named encoder tensor (a
                 plain indexed write): a matrix under the replicated update, a LayerNorm weight under the sharded update
                 (where a matrix has ONE owner whose result every rank receives: it cannot differ between ranks).  Every
                 rank must raise ReplicaDrift at iteration 3 naming that tensor; exits 3 when every configuration did.
--drift shadow   the same write to the bf16 SHADOW element (lowest mantissa bit).  Nothing may be raised: the update of
                 iteration 3 rewrites the shadow from the masters, which an exchange of summed gradients keeps identical,
                 so the replicas are equal again when the iteration's check runs.  (Why --drift master writes the master.)
--checkpoint DIR the guard in ``save_training_state`` (eager loop, both update modes, check_every so large that no tick
                 fires): healthy replicas write DIR/clean_<update>.pt; after the master write of --drift master both ranks
                 raise ReplicaDrift "(checkpoint)" and DIR/drift_<update>.pt is NOT written.  Exits 0 when all of that held.
--check-every N | none | absent    ``none`` passes check_every=None, ``absent`` calls enable_data_parallel without the two
                 arguments; both must launch no fingerprint kernel and train the same bits (the digest line)."""
import argparse
import os
import sys

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

MATRIX = "layer.0.attention.self.query.weight"
VECTOR = "layer.0.attention.output.LayerNorm.weight"
launches = [0]


def report(lines):
    """the lines of every rank, printed by rank 0 (two processes writing to one pipe interleave)"""
    every = [None] * dist.get_world_size()
    dist.all_gather_object(every, list(lines))
    if dist.get_rank() == 0:
        for ls in every:
            for l in ls:
                print(l, flush=True)


def count_fingerprint_launches():
    from xggm_amd import ops
    plain = ops.fingerprint_spans

    def counted(*a, **k):
        launches[0] += 1
        return plain(*a, **k)

    ops.fingerprint_spans = counted


def run(rank, use_graph, zero1, drift, check_every):
    from xggm_amd import synth
    from xggm_amd.dist import ReplicaDrift
    from xggm_amd.engine import CapturedTrainer
    from xggm_amd.fingerprint import state_fingerprint
    from xggm_amd.vqa.vqacpv2 import enable_data_parallel, make_optimizer
    from test_model_gpu import build_model, batch_tensors
    cfg = dict(hidden=128, heads=2, inter=256, vocab=64, max_pos=32, feat_dim=64, l_layers=2, x_layers=2, r_layers=1)
    A, B = 29, 4
    m = build_model(cfg, A, seed=5, dt=torch.bfloat16)
    b = batch_tensors(synth.vqa_batch(B, A=A, F=cfg["feat_dim"], vocab=cfg["vocab"], seed=100 + rank), "cuda")
    m(b["feats"], b["boxes"], (b["input_ids"], b["input_mask"], b["segment_ids"]))
    opt = make_optimizer(m, 1e-3, 20)
    kw = {} if check_every == "absent" else dict(check_every=None if check_every == "none" else int(check_every))
    enable_data_parallel(m, wire_dtype=torch.bfloat16, overlap=use_graph, zero1=zero1, **kw)
    if use_graph:
        tr = CapturedTrainer(m, opt, b, sigma=1.0, order="vqa", use_graph=True, warmup_iters=1)
        iterate = tr.iteration
    else:  # the eager loop a training script calls
        from xggm_amd.vqa.vqacpv2 import train_iteration, BCEWithLogitsLoss
        bce, eb = BCEWithLogitsLoss(), dict(b, sent=(b["input_ids"], b["input_mask"], b["segment_ids"]))
        iterate = lambda br: train_iteration(m, opt, bce, eb, branch=br)  # noqa: E731
    guard = getattr(m, "_replica_guard", None)
    arena = m.arena()
    tag = "engine=%s update=%s" % ("captured" if use_graph else "eager", "sharded" if zero1 else "replicated")
    want = VECTOR if (zero1 and drift == "master") else MATRIX
    name = [n for n in arena.info if n.endswith(want)][0]
    before = launches[0]
    raised, lines = None, []
    try:
        for it, br in enumerate(("rel", "node", "rel", "node"), 1):
            if it == 3 and rank == 1 and drift != "none":
                o = arena.info[name][0]
                torch.cuda.synchronize()
                if drift == "master":
                    arena.params[o + 5] = arena.params[o + 5] * 2 + 1
                else:
                    arena.shadow.view(torch.int16)[o + 5] ^= 1
            iterate(br)
    except ReplicaDrift as e:
        raised = e
        lines.append("rank %d %s: ReplicaDrift: %s" % (rank, tag, e))
    torch.cuda.synchronize()
    n_launch = launches[0] - before
    if raised is not None:
        ok = raised.iteration == 3 and name in raised.params and raised.ranks == [1]
        lines.append("rank %d %s: alarm at iteration %d names %s: %s" % (rank, tag, raised.iteration, name, ok))
        report(lines)
        return "alarm" if ok else "wrong alarm"
    fp = state_fingerprint(m, "weights")  # (under the sharded update the bf16 weights are whole on every rank)
    digest = " ".join("%s=%s" % kv for kv in sorted(fp["shadow"].items()))
    lines.append("rank %d %s: no alarm, %d checks, %d fingerprint launches while training"
                 % (rank, tag, guard.checks if guard else 0, n_launch))
    lines.append("rank %d %s: digest %s" % (rank, tag, digest))
    report(lines)
    return "clean"


def run_checkpoint(rank, zero1, out_dir):
    """save_training_state with a guard that has never ticked: a clean save writes, a drifted one raises and writes nothing"""
    from xggm_amd import synth
    from xggm_amd.dist import ReplicaDrift
    from xggm_amd.vqa.vqacpv2 import (enable_data_parallel, make_optimizer, train_iteration, BCEWithLogitsLoss,
                                      save_training_state)
    from test_model_gpu import build_model, batch_tensors
    cfg = dict(hidden=128, heads=2, inter=256, vocab=64, max_pos=32, feat_dim=64, l_layers=2, x_layers=2, r_layers=1)
    m = build_model(cfg, 29, seed=5, dt=torch.bfloat16)
    b = batch_tensors(synth.vqa_batch(4, A=29, F=cfg["feat_dim"], vocab=cfg["vocab"], seed=100 + rank), "cuda")
    b["sent"] = (b["input_ids"], b["input_mask"], b["segment_ids"])
    m(b["feats"], b["boxes"], b["sent"])
    opt = make_optimizer(m, 1e-3, 20)
    enable_data_parallel(m, wire_dtype=torch.bfloat16, overlap=False, zero1=zero1, check_every=1000)
    guard, arena, bce = m._replica_guard, m.arena(), BCEWithLogitsLoss()
    tag = "checkpoint update=%s" % ("sharded" if zero1 else "replicated")
    mode = "sharded" if zero1 else "replicated"
    name = [n for n in arena.info if n.endswith(VECTOR if zero1 else MATRIX)][0]
    paths = {k: os.path.join(out_dir, "%s_%s.pt" % (k, mode)) for k in ("clean", "drift")}
    for br in ("rel", "node"):
        train_iteration(m, opt, bce, b, branch=br)
    save_training_state(paths["clean"] if rank == 0 else None, m, opt)  # every rank calls; rank 0 writes
    lines = ["rank %d %s: clean save, %d ticks checked, %d checkpoint checks" % (rank, tag, guard.checks - 1, 1)]
    if rank == 1:
        o = arena.info[name][0]
        arena.params[o + 5] = arena.params[o + 5] * 2 + 1
    train_iteration(m, opt, bce, b, branch="rel")
    ok = False
    try:
        save_training_state(paths["drift"] if rank == 0 else None, m, opt)
        lines.append("rank %d %s: drifted save went through" % (rank, tag))
    except ReplicaDrift as e:
        ok = "(checkpoint)" in str(e) and name in e.params and e.ranks == [1] and e.iteration == 3
        lines.append("rank %d %s: ReplicaDrift: %s" % (rank, tag, e))
    dist.barrier()
    written = {k: os.path.exists(v) for k, v in paths.items()}
    lines.append("rank %d %s: files written: clean %s, drift %s" % (rank, tag, written["clean"], written["drift"]))
    report(lines)
    return ok and written["clean"] and not written["drift"] and guard.checks == 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--drift", default="none", choices=["none", "master", "shadow"])
    ap.add_argument("--check-every", default="1")
    ap.add_argument("--checkpoint", metavar="DIR", default=None)
    args = ap.parse_args()
    rank = int(os.environ["RANK"])
    torch.cuda.set_device(0)
    dist.init_process_group("gloo")
    count_fingerprint_launches()
    if args.checkpoint:
        good = [run_checkpoint(rank, zero1, args.checkpoint) for zero1 in (False, True)]
        report(["rank %d: checkpoint guard %s" % (rank, "ok" if all(good) else "FAILED")])
        dist.destroy_process_group()
        sys.exit(0 if all(good) else 6)
    res = []
    for use_graph in (False, True):
        for zero1 in (False, True):
            res.append(run(rank, use_graph, zero1, args.drift, args.check_every))
            dist.barrier()  # every rank has left the configuration the same way (an alarm on one rank only would hang here)
    report(["rank %d: %s" % (rank, " ".join(res))])
    dist.destroy_process_group()
    if args.drift == "master":
        sys.exit(3 if all(r == "alarm" for r in res) else 4)
    sys.exit(0 if all(r == "clean" for r in res) else 5)


if __name__ == "__main__":
    main()
