"""Rehearsal of replicated data parallelism with an attached debias loss on ONE GPU: world size 2 over gloo, both ranks
on cuda:0, the tiny model with ``LearnedMixin`` attached, DIFFERENT batches (and bias rows) per rank, one training
iteration (eager ``train_iteration`` or, with ``--captured``, ``CapturedTrainer.iteration``).
  python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 tools/dp_debias_rehearsal.py
Rank 0 prints ``debias_loss.<name>: moved <bool> equal <bool>`` per parameter of the loss -- every one must have been
trained and must be bit-identical on both ranks afterwards (the exchange covered the loss's arena group) -- and
``replicas equal <bool>`` for the whole state_dict.  Exits 0 when all of that held."""
import argparse
import os
import sys

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--captured", action="store_true")
    args = ap.parse_args()
    rank = int(os.environ["RANK"])
    torch.cuda.set_device(0)
    dist.init_process_group("gloo")
    from xggm_amd import synth
    from xggm_amd.engine import CapturedTrainer
    from xggm_amd.module.vqa_debias_loss_functions import LearnedMixin
    from xggm_amd.vqa.vqacpv2 import (attach_debias_loss, enable_data_parallel, make_optimizer, train_iteration,
                                      BCEWithLogitsLoss)
    from test_model_gpu import build_model, batch_tensors
    cfg = dict(hidden=128, heads=2, inter=256, vocab=64, max_pos=32, feat_dim=64, l_layers=2, x_layers=2, r_layers=1)
    A, B = 29, 4
    m = build_model(cfg, A, seed=5, dt=torch.bfloat16)
    loss = LearnedMixin(0.36, hidden_dim=cfg["hidden"])
    loss.load_state_dict({k: torch.from_numpy(synth.seeded_param("debias_loss." + k, v.shape, 5)) for k, v in loss.state_dict().items()})
    attach_debias_loss(m, loss)
    b = batch_tensors(synth.vqa_batch(B, A=A, F=cfg["feat_dim"], vocab=cfg["vocab"], seed=100 + rank), "cuda")
    b["bias"] = torch.from_numpy(synth.debias_case(B, A, 0, 200 + rank)["bias"]).cuda()
    before = {k: v.detach().clone() for k, v in m.state_dict().items() if k.startswith("debias_loss.")}
    opt = make_optimizer(m, 1e-3, 20)  # (the warm-up leaves the first pass at lr 0: the iteration's second pass moves them)
    enable_data_parallel(m, wire_dtype=torch.bfloat16, overlap=args.captured)
    if args.captured:
        CapturedTrainer(m, opt, b, sigma=1.0, order="vqa", use_graph=True, warmup_iters=1).iteration("rel")
    else:
        train_iteration(m, opt, BCEWithLogitsLoss(), dict(b, sent=(b["input_ids"], b["input_mask"], b["segment_ids"])),
                        branch="rel")
    torch.cuda.synchronize()
    sd = {k: v.detach().float().cpu() for k, v in m.state_dict().items()}
    every = [None] * dist.get_world_size()
    dist.all_gather_object(every, sd)
    ok = True
    if rank == 0:
        for k in sorted(before):
            moved = not torch.equal(before[k].float().cpu(), sd[k])
            equal = all(torch.equal(sd[k], o[k]) for o in every[1:])
            ok = ok and moved and equal
            print("%s: moved %s equal %s" % (k, moved, equal), flush=True)
        whole = all(torch.equal(sd[k], o[k]) for o in every[1:] for k in sd)
        ok = ok and whole and len(before) == 3
        print("replicas equal %s" % whole, flush=True)
    flag = [ok]
    dist.broadcast_object_list(flag, src=0)
    dist.destroy_process_group()
    sys.exit(0 if flag[0] else 7)


if __name__ == "__main__":
    main()
