"""What data parallelism adds to one captured LXMERT pre-training step, on ONE GPU: a one-rank RCCL group with
XGGM_DP_FORCE=1 (the collectives are issued although the reduction is the identity), full LXMERT 9/5/5
(``LXRTPretraining``, all six tasks, 9500 answers), bf16 storage and bf16 wire, T = 20, 36 objects of 2048 features, batch 32:
the model and batch of tools/bench_pretrain_step.py.
  python tools/bench_pretrain_dp.py [--out profiles/pretrain/dp_step_ab.txt] [--rounds 3] [--iters 30] [--warmup 3]
  (1) the one-graph step of a model that was never prepared for data parallelism;
  (2) the two-graph step with the forced exchange between the graphs (``pretrain.lxmert_pretrain.enable_data_parallel``);
alternating windows of --iters steps between device events, as tools/bench_pretrain_step.py times them; then, alone,
  (x) the step's whole exchange (``GradSync.sync`` of the active ranges: vector casts + all-reduces on the wire arena);
  (t) the all-reduce of the dense word table at full size, 30522 x 768 bf16 -- what the tied decoder makes dense.
On one rank RCCL moves nothing between devices: (2) - (1) is the cost of cutting the graph and of issuing the exchange from
the host, NOT the cost of the links, and nothing here says anything about scaling, which this tool does not measure.
No ratio is asserted anywhere: this file is where the numbers come from."""
import argparse
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
T, O, F, VOCAB, N_ANS, K, B = 20, 36, 2048, 30522, 9500, 4, 32


def build(dev, dp):
    import torch
    from xggm_amd import synth
    from xggm_amd.engine import CapturedPretrainer
    from xggm_amd.lxrt import modeling as M
    from xggm_amd.lxrt.optimization import BertAdam
    from xggm_amd.pretrain.lxmert_pretrain import DeviceFeatures, enable_data_parallel, pack_labels
    torch.manual_seed(0)
    vc = M.VISUAL_CONFIG
    vc.l_layers, vc.x_layers, vc.r_layers = 9, 5, 5
    model = M.LXRTPretraining(M.BertConfig(VOCAB), visual_losses="obj,attr,feat", task_qa=True, num_answers=N_ANS,
                              mlm_capacity=int(math.ceil(0.25 * B * T)), compute_dtype=torch.bfloat16).to(dev).train()
    optim = BertAdam(list(model.parameters()), lr=1e-4, warmup=0.05, t_total=100000)
    x = synth.pretrain_case(B, T, O, F, VOCAB, 1600, 400, N_ANS, seed=B)
    lab, sc = pack_labels([{int(a): 1.0} for a in x["ans"].clip(0)], K)
    batch = dict(input_ids=x["input_ids"], input_mask=x["input_mask"], segment_ids=x["segment_ids"], feats=x["feats"], boxes=x["boxes"],
                 obj_labels=x["obj_label"], obj_confs=x["obj_conf"], attr_labels=x["attr_label"], attr_confs=x["attr_conf"],
                 is_matched=0 * x["matched_label"] + 1, img_ids=x["ans"] % max(B // 2, 1))
    batch = {k: torch.from_numpy(v).to(dev) for k, v in batch.items()}
    batch["label_ids"], batch["label_scores"] = lab.to(dev), sc.to(dev)
    if dp:
        enable_data_parallel(model, wire_dtype=torch.bfloat16)
    feats = DeviceFeatures(vocab_size=VOCAB, mask_id=103, max_labels=K, match_rate=0.5)
    return model, CapturedPretrainer(model, optim, batch, feats, warmup_iters=2)


def window(fn, iters):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pretrain", "dp_step_ab.txt"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import torch
    import torch.distributed as dist
    if not torch.cuda.is_available():
        sys.exit("bench_pretrain_dp: no GPU -- nothing is measured without one")
    os.environ["XGGM_DP_FORCE"] = "1"
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29541")
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        def say(msg):
            f.write(msg + "\n")
            f.flush()
            print(msg, flush=True)

        say("one captured LXMERT pre-training step, LXRTPretraining 9/5/5, bf16 storage, batch %d, T=%d, %d x %d features, %d "
            "answers; one-rank RCCL group, XGGM_DP_FORCE=1, bf16 wire arena" % (B, T, O, F, N_ANS))
        say("(1) one graph, no data parallelism   (2) two graphs, the forced exchange between them")
        say("%d rounds alternating, %d steps per window between device events after %d warm-up steps; ms per step"
            % (args.rounds, args.iters, args.warmup))
        m1, t1 = build(dev, False)
        m2, t2 = build(dev, True)
        assert not isinstance(t1.graphs["train"], tuple) and isinstance(t2.graphs["train"], tuple)
        for tr in (t1, t2):
            for _ in range(args.warmup):
                tr.step()
        torch.cuda.synchronize()
        ms = {1: [], 2: []}
        for _ in range(args.rounds):
            ms[1].append(window(t1.step, args.iters))
            ms[2].append(window(t2.step, args.iters))
        med = {k: statistics.median(v) for k, v in ms.items()}
        for k in (1, 2):
            say("  (%d) %s   median %.3f   spread %.3f" % (k, "  ".join("%.3f" % v for v in ms[k]), med[k], max(ms[k]) - min(ms[k])))
        say("  (2) - (1) = %+.3f ms per step (%.3f x): the cut between the graphs and the host-issued exchange, no link traffic"
            % (med[2] - med[1], med[2] / med[1]))
        gs, ranges = m2._grad_sync, t2.graphs["train"][2]
        n = sum(e - s for s, e in ranges)
        x = [window(lambda: gs.sync(ranges), args.iters) for _ in range(args.rounds)]
        say("  (x) the step's exchange alone (%d ranges, %.1f M elements on the bf16 wire): %s   median %.3f ms"
            % (len(ranges), n / 1e6, "  ".join("%.3f" % v for v in x), statistics.median(x)))
        table = torch.zeros(VOCAB * 768, dtype=torch.bfloat16, device=dev)
        t = [window(lambda: dist.all_reduce(table), args.iters) for _ in range(args.rounds)]
        say("  (t) all-reduce of the dense word table alone, %d x 768 bf16 = %.1f MB: %s   median %.3f ms"
            % (VOCAB, table.numel() * 2 / 1e6, "  ".join("%.3f" % v for v in t), statistics.median(t)))
        say("(x) and (t) on ONE rank: RCCL reduces nothing and moves nothing -- these are the costs of issuing the exchange, not link times")
        say("scaling over several GPUs is UNMEASURED: one rank on one GPU (two ranks on one card would measure nothing)")
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
