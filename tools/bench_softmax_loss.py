"""What the softmax answer losses cost (xggm_softmax_loss_fwd_f32 / _bwd_f32; ``Focal``, ``CrossEntropy``).
  python tools/bench_softmax_loss.py [--out profiles/softmax_loss/softmax_loss_ab.txt] [--rounds 2] [--windows 5] [--steps 20]
Two measurements at batch 32 and 3129 answers, every one in a fresh child process under its own time limit; the first child
that fails ends the run.
  1. per launch: the forward and the backward launch of either kind beside the yardstick, the BCE forward + backward pair
     (xggm_bce_fwd / xggm_bce_bwd_f32) on the same logits.  --launches launches of ONE kernel are captured into a graph
     (no host launch cost in the window), the graph is replayed --replays times between two device events after a warm-up
     replay, and the median replay over the launch count is reported: the launch-to-launch time of the kernel in a
     stream, which is what a captured pass pays for it.
  2. per iteration: the ``bench.build`` configuration (LXMERT 9/5/5, bf16, hipGraph replay) with nothing attached (arm A),
     ``CrossEntropy()`` attached (arm C) and ``Focal()`` attached with a [B, A] bias in the batch (arm F); the arms
     alternate A/C/F/A/C/F.  A child times --windows windows of --steps iterations after --warmup iterations, like
     ``bench.py``'s timed region (wall time between two device synchronisations), and takes the median.  Printed: every
     child's median, each arm's median over all its windows, the differences to A in ms and per cent, and the A/A spread
     -- the largest difference between two children of the SAME arm -- that a difference has to exceed to mean anything."""
import argparse
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
ARMS = {"A": "BCEWithLogits x answers (nothing attached)", "C": "CrossEntropy() attached",
        "F": "Focal() attached, [B, A] bias in the batch"}


def micro(launches, replays):
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_softmax_loss: no GPU -- nothing is measured without one")
    from xggm_amd import ops, synth
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    x = {k: torch.from_numpy(v).to(dev) for k, v in synth.debias_case(BATCH, ANSWERS, 0, 21).items()}
    one = torch.ones((), device=dev)
    coef = 1.0 / BATCH
    slot = ops.zeros_f32(1, dev)
    prs = {}
    for name, kind, bias in (("focal", ops.SOFTMAX_FOCAL, x["bias"]), ("ce", ops.SOFTMAX_CE, None)):
        prs[name] = ops.softmax_loss_fwd(kind, x["logits"], x["labels"], None, bias, out=slot)[1]

    def fwd(name):
        pr = prs[name]
        return lambda: ops.softmax_loss_fwd(pr.kind, x["logits"], x["labels"], None, pr.t["bias"], out=slot, save=pr.save)

    work = {
        "bce fwd": lambda: ops.bce_fwd(x["logits"], x["labels"], coef, out=slot),
        "bce bwd": lambda: ops.bce_bwd(x["logits"], x["labels"], one, coef, torch.float32),
        "focal fwd": fwd("focal"),
        "focal bwd": lambda: ops.softmax_loss_bwd(prs["focal"], one, d_logit=None),
        "ce fwd": fwd("ce"),
        "ce bwd": lambda: ops.softmax_loss_bwd(prs["ce"], one, d_logit=None),
    }
    out = {}
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        for name, fn in work.items():
            fn()
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side):
                for _ in range(launches):
                    fn()
            g.replay()
            torch.cuda.synchronize()
            us = []
            for _ in range(replays):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(side)
                g.replay()
                e1.record(side)
                e1.synchronize()
                us.append(1000.0 * e0.elapsed_time(e1) / launches)
            out[name] = [statistics.median(us), min(us), max(us)]
    print("RESULT " + json.dumps(out), flush=True)


def child(arm, windows, steps, warmup):
    import random
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_softmax_loss: no GPU -- nothing is measured without one")
    import bench
    from xggm_amd import synth
    from xggm_amd.engine import CapturedTrainer
    from xggm_amd.module.answer_losses import CrossEntropy, Focal
    from xggm_amd.vqa.vqacpv2 import attach_debias_loss
    torch.cuda.set_device(0)
    device = torch.device("cuda", 0)
    args = bench.parse(["--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), "--batch", str(BATCH), "--answers",
                        str(ANSWERS)])
    model, optim, batch = bench.build(args, device)
    if arm == "C":
        attach_debias_loss(model, CrossEntropy())
    elif arm == "F":
        attach_debias_loss(model, Focal())
        batch["bias"] = torch.from_numpy(synth.debias_case(BATCH, ANSWERS, 0, args.seed)["bias"]).to(device)
    trainer = CapturedTrainer(model, optim, batch, sigma=1.0, order=args.order, warmup_iters=2)
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
            out = trainer.iteration(branch())
        torch.cuda.synchronize()
        ms.append(1000.0 * (time.perf_counter() - t0) / steps)
    print("RESULT " + json.dumps({"arm": arm, "ms_per_step": ms, "loss_plain": float(out[0][0]), "loss_ggm": float(out[1][0])}),
          flush=True)


def run_child(extra, f):
    p = subprocess.run(["timeout", "-k", "10", str(CHILD_LIMIT), sys.executable, os.path.abspath(__file__)] + extra,
                       capture_output=True, text=True, cwd=ROOT)
    res = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
    if p.returncode != 0 or not res:
        msg = "child %s ended with status %d; nothing further was started\n%s" % (" ".join(extra), p.returncode, p.stderr[-2000:])
        f.write(msg)
        sys.exit(msg)
    return json.loads(res[-1][len("RESULT "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "softmax_loss", "softmax_loss_ab.txt"))
    ap.add_argument("--rounds", type=int, default=2, help="A/C/F triples (at least 2: the A/A spread needs two runs per arm)")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--replays", type=int, default=21)
    ap.add_argument("--arm", choices=list(ARMS))
    ap.add_argument("--micro", action="store_true")
    args = ap.parse_args()
    if args.micro:
        return micro(args.launches, args.replays)
    if args.arm:
        return child(args.arm, args.windows, args.steps, args.warmup)
    if args.rounds < 2:
        sys.exit("bench_softmax_loss: --rounds must be at least 2")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        def say(msg):
            f.write(msg + "\n")
            f.flush()
            print(msg, flush=True)

        say("softmax answer losses, batch %d, %d answers (fp32 logits, labels, bias: %.2f MB per array)"
            % (BATCH, ANSWERS, BATCH * ANSWERS * 4 / 1e6))
        say("1. per launch: %d launches of one kernel in a graph, %d timed replays, us per launch, median (min .. max)"
            % (args.launches, args.replays))
        m = run_child(["--micro", "--launches", str(args.launches), "--replays", str(args.replays)], f)
        for name, (med, lo, hi) in m.items():
            say("  %-10s %7.2f  (%.2f .. %.2f)" % (name, med, lo, hi))
        pair = {k: m[k + " fwd"][0] + m[k + " bwd"][0] for k in ("bce", "focal", "ce")}
        say("  forward + backward: bce %.2f   focal %.2f (%+.2f)   ce %.2f (%+.2f)"
            % (pair["bce"], pair["focal"], pair["focal"] - pair["bce"], pair["ce"], pair["ce"] - pair["bce"]))
        say("2. per iteration: bench.build configuration, bf16, graph replay; %d windows of %d iterations per child after %d "
            "warm-up iterations; ms_per_step, median (min .. max)" % (args.windows, args.steps, args.warmup))
        for a, what in ARMS.items():
            say("  %s: %s" % (a, what))
        runs = {a: [] for a in ARMS}
        for r in range(args.rounds):
            for arm in ARMS:
                out = run_child(["--arm", arm, "--windows", str(args.windows), "--steps", str(args.steps), "--warmup",
                                 str(args.warmup)], f)
                runs[arm].append(out["ms_per_step"])
                say("  round %d arm %s: %8.4f  (%.4f .. %.4f)   last losses: plain %.4f, ggm %.4f"
                    % (r, arm, statistics.median(out["ms_per_step"]), min(out["ms_per_step"]), max(out["ms_per_step"]),
                       out["loss_plain"], out["loss_ggm"]))
        med = {a: statistics.median([x for run in runs[a] for x in run]) for a in runs}
        spread = {a: max(statistics.median(x) for x in runs[a]) - min(statistics.median(x) for x in runs[a]) for a in runs}
        noise = max(spread.values())
        say("median ms_per_step: " + "   ".join("%s %.4f" % (a, med[a]) for a in ARMS))
        for a in ("C", "F"):
            diff = med[a] - med["A"]
            say("%s - A %+.4f ms = %+.2f %% of A (two passes per iteration): %s the A/A spread"
                % (a, diff, 100.0 * diff / med["A"], "within" if abs(diff) <= noise else "EXCEEDS"))
        say("A/A spread (between the runs of the same arm): " + "   ".join("%s %.4f" % (a, spread[a]) for a in ARMS)
            + "   -> %.4f ms" % noise)


if __name__ == "__main__":
    main()
