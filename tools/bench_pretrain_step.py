"""What one LXMERT pre-training step costs, eagerly against ``engine.CapturedPretrainer``: full LXMERT 9/5/5
(``LXRTPretraining``, all six tasks, 9500 answers), bf16, T = 20, 36 objects of 2048 features, mlm_capacity = ceil(0.25 B T),
swap rate 0.5, at batch 32 and 256.
  python tools/bench_pretrain_step.py [--out profiles/pretrain/step_ab.txt] [--rounds 3] [--iters 30] [--warmup 3]
Three variants of the SAME calls (swap, masking, forward, backward, clip at 1.0 + BertAdam + the rng advance) on one
model, one fresh child process per batch size under its own time limit; the first child that fails ends the run.
  (e) eager: ``CapturedPretrainer(use_graph=False)`` -- what a hand-written loop over ``DeviceFeatures``,
      ``LXRTPretraining.forward``, ``Runtime.backward`` and ``clip_and_step`` issues from Python, plus the swap's one launch;
  (c) captured: one graph replay per step, no logs;
  (l) captured with ``train_log`` and ``answer_log`` attached (two more launches inside the graph).
A child warms every variant up, then times --iters steps of one variant between two device events (the window ends in an
event synchronise, so an eager window includes the time the device waits for the host), the variants alternating e / c / l
for --rounds rounds; reported: each window's ms per step, each variant's median, the spread between the windows of one
variant, and the ratios of the medians.  No ratio is asserted anywhere: this file is where the numbers come from."""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CHILD_LIMIT = 540  # seconds per child process
T, O, F, VOCAB, N_ANS, K = 20, 36, 2048, 30522, 9500, 4


def child(B, rounds, iters, warmup):
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_pretrain_step: no GPU -- nothing is measured without one")
    from xggm_amd import synth
    from xggm_amd.engine import AnswerLog, CapturedPretrainer, TrainLog
    from xggm_amd.lxrt import modeling as M
    from xggm_amd.lxrt.optimization import BertAdam
    from xggm_amd.pretrain.lxmert_pretrain import DeviceFeatures, pack_labels
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    vc = M.VISUAL_CONFIG
    vc.l_layers, vc.x_layers, vc.r_layers = 9, 5, 5  # the pre-training configuration (--llayers 9 --xlayers 5 --rlayers 5)
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
    n = warmup + rounds * iters + 8
    feats = lambda: DeviceFeatures(vocab_size=VOCAB, mask_id=103, max_labels=K, match_rate=0.5)
    trainers = {
        "e": CapturedPretrainer(model, optim, batch, feats(), use_graph=False),
        "c": CapturedPretrainer(model, optim, batch, feats(), warmup_iters=2),
        "l": CapturedPretrainer(model, optim, batch, feats(), warmup_iters=2, train_log=TrainLog(n, dev),
                                answer_log=AnswerLog(n * B, dev, with_scores=False)),
    }
    losses = {}
    for name, tr in trainers.items():
        for _ in range(warmup):
            out = tr.step()
        torch.cuda.synchronize()
        losses[name] = float(out[0])
    ms = {name: [] for name in trainers}
    for _ in range(rounds):
        for name, tr in trainers.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                tr.step()
            e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1) / iters)
    trainers["l"].check()
    rec = trainers["l"].train_log.read()
    print("RESULT " + json.dumps({"B": B, "ms": ms, "loss": losses, "logged": int(rec["cursor"]),
                                  "exhausted": int(trainers["c"].features.swap_exhausted)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pretrain", "step_ab.txt"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, help="run one batch size in this process (a child)")
    args = ap.parse_args()
    if args.batch:
        return child(args.batch, args.rounds, args.iters, args.warmup)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        def say(msg):
            f.write(msg + "\n")
            f.flush()
            print(msg, flush=True)

        say("one LXMERT pre-training step (swap, masking, forward, backward, clip + BertAdam), LXRTPretraining 9/5/5, bf16, "
            "T=%d, %d x %d features, %d answers, mlm_capacity = ceil(0.25 B T)" % (T, O, F, N_ANS))
        say("(e) eager: the same calls issued from Python   (c) captured: one graph replay   (l) captured + train_log + answer_log")
        say("%d rounds e / c / l alternating, %d steps per window between device events after %d warm-up steps; ms per step"
            % (args.rounds, args.iters, args.warmup))
        for B in (32, 256):
            p = subprocess.run(["timeout", "-k", "10", str(CHILD_LIMIT), sys.executable, os.path.abspath(__file__), "--batch",
                                str(B), "--rounds", str(args.rounds), "--iters", str(args.iters), "--warmup", str(args.warmup)],
                               capture_output=True, text=True, cwd=ROOT)
            res = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
            if p.returncode != 0 or not res:
                msg = "child for batch %d ended with status %d; nothing further was started\n%s" % (B, p.returncode, p.stderr[-2000:])
                f.write(msg)
                sys.exit(msg)
            r = json.loads(res[-1][len("RESULT "):])
            med = {k: statistics.median(v) for k, v in r["ms"].items()}
            say("batch %d (%d records logged, %d rows exhausted their swap candidates)" % (B, r["logged"], r["exhausted"]))
            for k in ("e", "c", "l"):
                say("  (%s) %s   median %.3f   spread %.3f   last warm-up loss %.4f"
                    % (k, "  ".join("%.3f" % v for v in r["ms"][k]), med[k], max(r["ms"][k]) - min(r["ms"][k]), r["loss"][k]))
            say("  (e) / (c) = %.2f x  -- the captured step is %s;  (l) / (c) = %.3f x" %
                (med["e"] / med["c"], "faster" if med["c"] < med["e"] else "NOT faster", med["l"] / med["c"]))


if __name__ == "__main__":
    main()
