"""What the device-resident training log costs per iteration (xggm_train_log_append, engine.TrainLog).
  python tools/bench_trainlog.py [--out profiles/r05_experiments/trainlog_ab.txt] [--rounds 2] [--windows 7] [--steps 20]
The default ``bench.build`` configuration (LXMERT 9/5/5, batch 32, bf16, hipGraph replay) with ``train_log=None`` (arm
A: the graphs of the parent) and with ``train_log=TrainLog(...)`` (arm B: one more launch at the end of each of the two
passes of an iteration).  Every run is a fresh child process under its own time limit, the arms alternate A/B/A/B, and
the first child that fails ends the run.  A child times --windows windows of --steps iterations after --warmup
iterations, like ``bench.py``'s timed region (wall time between two device synchronisations), and takes the median.
Printed: the median ms_per_step of every child, of each arm over all its windows, B - A, and the A/A spread -- the
larger of the differences between the two children of the SAME arm -- that a difference has to exceed to mean anything.
The logged arm ends with one ``read()`` (outside the timed windows) and checks the record count."""
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


def child(arm, windows, steps, warmup):
    import random
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_trainlog: no GPU -- nothing is measured without one")
    import bench
    from xggm_amd.engine import CapturedTrainer, TrainLog
    torch.cuda.set_device(0)
    device = torch.device("cuda", 0)
    args = bench.parse(["--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)])
    model, optim, batch = bench.build(args, device)
    n_iters = warmup + windows * steps
    log = TrainLog(2 * n_iters, device) if arm == "B" else None
    trainer = CapturedTrainer(model, optim, batch, sigma=1.0, order=args.order, train_log=log)
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
    out = {"arm": arm, "ms_per_step": ms}
    if log is not None:
        rec = log.read()
        assert int(rec["cursor"]) == 2 * n_iters and int(rec["counts"][TrainLog.PLAIN]) == n_iters, rec["counts"]
        out["records"], out["first_bad"] = int(rec["cursor"]), int(rec["first_bad"])
        out["average_loss"] = log.average_loss(args.batch)
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r05_experiments", "trainlog_ab.txt"))
    ap.add_argument("--rounds", type=int, default=2, help="A/B pairs (at least 2: the A/A spread needs two runs per arm)")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--arm", choices=["A", "B"])
    args = ap.parse_args()
    if args.arm:
        return child(args.arm, args.windows, args.steps, args.warmup)
    if args.rounds < 2:
        sys.exit("bench_trainlog: --rounds must be at least 2")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    runs = {"A": [], "B": []}
    with open(args.out, "w") as f:
        def say(msg):
            f.write(msg + "\n")
            f.flush()
            print(msg, flush=True)

        say("training log A/B: default bench.build configuration, %d windows of %d iterations per child after %d warm-up "
            "iterations; ms_per_step, median (min .. max)" % (args.windows, args.steps, args.warmup))
        say("A: train_log=None    B: train_log=TrainLog (two appends per iteration)")
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
                out = json.loads(res[-1][len("RESULT "):])
                runs[arm].append(out["ms_per_step"])
                extra = "" if arm == "A" else "   %d records, first_bad %d, average_loss %.6f" % (
                    out["records"], out["first_bad"], out["average_loss"])
                say("  round %d arm %s: %8.4f  (%.4f .. %.4f)%s" % (r, arm, statistics.median(out["ms_per_step"]),
                                                                   min(out["ms_per_step"]), max(out["ms_per_step"]), extra))
        med = {a: statistics.median([x for run in runs[a] for x in run]) for a in runs}
        spread = {a: max(statistics.median(x) for x in runs[a]) - min(statistics.median(x) for x in runs[a]) for a in runs}
        say("median ms_per_step: A %.4f   B %.4f   B - A %+.4f ms = %+.2f us per append"
            % (med["A"], med["B"], med["B"] - med["A"], (med["B"] - med["A"]) * 1e3 / 2))
        say("A/A spread (between the runs of the same arm): A %.4f   B %.4f   -> %.4f ms"
            % (spread["A"], spread["B"], max(spread.values())))
        say("B - A %s the A/A spread" % ("is within" if med["B"] - med["A"] <= max(spread.values()) else "EXCEEDS"))


if __name__ == "__main__":
    main()
