"""What an attached debias loss costs per iteration (xggm_debias_fwd / xggm_debias_bwd, vqa.vqacpv2.attach_debias_loss).
  python tools/bench_debias.py [--out profiles/debias/debias_ab.txt] [--rounds 2] [--windows 7] [--steps 20]
The ``bench.build`` configuration (LXMERT 9/5/5, bf16, hipGraph replay) at batch 32 and 3129 answers, with the head loss of
the parent (arm A: BCEWithLogits x answers, nothing attached) and with ``LearnedMixin(0.36, hidden_dim=768)`` attached and a
[B, A] bias in the batch (arm B).  Every run is a fresh child process under its own time limit, the arms alternate
A/B/A/B, and the first child that fails ends the run.  A child times --windows windows of --steps iterations after
--warmup iterations, like ``bench.py``'s timed region (wall time between two device synchronisations), and takes the
median.  Printed: the median ms_per_step of every child, of each arm over all its windows, B - A in ms and in per cent of
A, the A/A spread -- the larger of the differences between the two children of the SAME arm -- that a difference has to
exceed to mean anything, and the launches of the loss per pass (forward + backward), counted at the C ABI while the
trainer is built (the warm-up and capture passes run the Python of a pass; a replay runs none)."""
import argparse
import collections
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CHILD_LIMIT = 300  # seconds per child process
BATCH, ANSWERS = 32, 3129


def child(arm, windows, steps, warmup):
    import random
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_debias: no GPU -- nothing is measured without one")
    import bench
    from xggm_amd import ops, synth
    from xggm_amd.engine import CapturedTrainer
    from xggm_amd.module.vqa_debias_loss_functions import LearnedMixin
    from xggm_amd.vqa.vqacpv2 import attach_debias_loss, make_optimizer
    torch.cuda.set_device(0)
    device = torch.device("cuda", 0)
    args = bench.parse(["--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), "--batch", str(BATCH), "--answers",
                        str(ANSWERS)])
    model, optim, batch = bench.build(args, device)
    if arm == "B":
        attach_debias_loss(model, LearnedMixin(0.36, hidden_dim=model.lxrt_encoder.dim))
        # the loss's parameters have to be the optimiser's: the same groups and schedule as bench.build's, made again
        optim = make_optimizer(model, optim.param_groups[-1]["lr"], optim.defaults["t_total"])
        batch["bias"] = torch.from_numpy(synth.debias_case(BATCH, ANSWERS, 0, args.seed)["bias"]).to(device)
    seen, real_call = [], ops.call

    def spy(fn, *a):
        seen.append(fn)
        return real_call(fn, *a)

    ops.call = spy
    warm = 2
    trainer = CapturedTrainer(model, optim, batch, sigma=1.0, order=args.order, warmup_iters=warm)
    ops.call = real_call
    counts = collections.Counter(seen)
    passes = 3 * (warm + 1)  # plain, rel, node: ``warm`` eager rounds, then the captures
    pyrng = random.Random(args.seed)

    def branch():
        return "rel" if pyrng.randint(1, 10) <= args.delta else "node"

    for _ in range(warmup):
        trainer.iteration(branch())
    torch.cuda.synchronize()
    ms = []
    for _ in range(windows):
        t0 = time.perf_counter()
        for _ in range(steps):
            trainer.iteration(branch())
        torch.cuda.synchronize()
        ms.append(1000.0 * (time.perf_counter() - t0) / steps)
    out = {"arm": arm, "ms_per_step": ms, "loss_calls_per_pass": (counts["xggm_debias_fwd_bf16"] + counts["xggm_debias_bwd_bf16"]) / passes,
           "bce_calls_per_pass": (counts["xggm_bce_fwd"] + counts["xggm_bce_bwd_f32"]) / passes,
           "abi_calls_per_pass": len(seen) / passes}
    if arm == "B":
        sd = model.state_dict()
        out["finite"] = all(bool(torch.isfinite(sd[k]).all()) for k in sd if k.startswith("debias_loss."))
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "debias", "debias_ab.txt"))
    ap.add_argument("--rounds", type=int, default=2, help="A/B pairs (at least 2: the A/A spread needs two runs per arm)")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--arm", choices=["A", "B"])
    args = ap.parse_args()
    if args.arm:
        return child(args.arm, args.windows, args.steps, args.warmup)
    if args.rounds < 2:
        sys.exit("bench_debias: --rounds must be at least 2")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    runs, last = {"A": [], "B": []}, {}
    with open(args.out, "w") as f:
        def say(msg):
            f.write(msg + "\n")
            f.flush()
            print(msg, flush=True)

        say("debias loss A/B: bench.build configuration at batch %d, %d answers, bf16, graph replay; %d windows of %d "
            "iterations per child after %d warm-up iterations; ms_per_step, median (min .. max)"
            % (BATCH, ANSWERS, args.windows, args.steps, args.warmup))
        say("A: BCEWithLogits x answers (nothing attached)    B: LearnedMixin(0.36, hidden_dim=768) attached, [B, A] bias")
        for r in range(args.rounds):
            for arm in ("A", "B"):
                p = subprocess.run(["timeout", "-k", "10", str(CHILD_LIMIT), sys.executable, os.path.abspath(__file__), "--arm",
                                    arm, "--windows", str(args.windows), "--steps", str(args.steps), "--warmup",
                                    str(args.warmup)], capture_output=True, text=True, cwd=ROOT)
                res = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
                if p.returncode != 0 or not res:
                    msg = "arm %s of round %d ended with status %d; nothing further was started\n%s" % (arm, r, p.returncode,
                                                                                                        p.stderr[-2000:])
                    f.write(msg)
                    sys.exit(msg)
                out = last[arm] = json.loads(res[-1][len("RESULT "):])
                runs[arm].append(out["ms_per_step"])
                say("  round %d arm %s: %8.4f  (%.4f .. %.4f)" % (r, arm, statistics.median(out["ms_per_step"]),
                                                                 min(out["ms_per_step"]), max(out["ms_per_step"])))
        med = {a: statistics.median([x for run in runs[a] for x in run]) for a in runs}
        spread = {a: max(statistics.median(x) for x in runs[a]) - min(statistics.median(x) for x in runs[a]) for a in runs}
        say("median ms_per_step: A %.4f   B %.4f   B - A %+.4f ms = %+.2f %% of A (two passes per iteration)"
            % (med["A"], med["B"], med["B"] - med["A"], 100.0 * (med["B"] - med["A"]) / med["A"]))
        say("A/A spread (between the runs of the same arm): A %.4f   B %.4f   -> %.4f ms"
            % (spread["A"], spread["B"], max(spread.values())))
        say("B - A %s the A/A spread" % ("is within" if abs(med["B"] - med["A"]) <= max(spread.values()) else "EXCEEDS"))
        say("launches of the head loss per pass (forward + backward): A %.0f (bce)   B %.0f C-ABI calls = %d launches (the "
            "backward call is two: rows, then parameter sums)   all C-ABI calls per pass: A %.1f   B %.1f"
            % (last["A"]["bce_calls_per_pass"], last["B"]["loss_calls_per_pass"], int(last["B"]["loss_calls_per_pass"]) + 1,
               last["A"]["abi_calls_per_pass"], last["B"]["abi_calls_per_pass"]))
        say("B's loss parameters finite after the run: %s" % last["B"]["finite"])


if __name__ == "__main__":
    main()
