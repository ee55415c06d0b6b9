"""Launch time of every update rule of ``xggm_optim_multi``, BertAdam first, on an arena-sized vector (110 M
parameters, as tools/bench_adam.py): warm-up, then ROUNDS rounds that alternate the rules, each timed with events over
REPS launches; the median over the rounds is printed with the rule's bytes per parameter."""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from xggm_amd import ops  # noqa: E402

N, ROUNDS, REPS = 110_000_000, 7, 10
# bytes per parameter: p read + written (8), g read (4), bf16 shadow written (2), every state buffer read + written (8)
RULES = [("bertadam", {}, 30), ("adam", dict(b1=0.9, b2=0.999), 30), ("adamw", dict(b1=0.9, b2=0.999), 30),
         ("adamax", dict(b1=0.9, b2=0.999), 30), ("sgd", {}, 14), ("sgd", dict(momentum=0.9), 22),
         ("rmsprop", dict(alpha=0.99), 22), ("rmsprop", dict(alpha=0.99, momentum=0.9), 30)]


def main():
    p, g, m, v = (torch.randn(N, device="cuda") * 0.01 for _ in range(4))
    v.abs_()
    sh = torch.empty(N, device="cuda", dtype=torch.bfloat16)
    sqn = torch.ones(1, device="cuda")
    steps = torch.zeros(1, device="cuda", dtype=torch.int64)
    sc, hs = torch.ones(1, device="cuda"), torch.zeros(4, device="cuda")
    ops.sched_step_ex(steps, sc, hs, [(0, -1, 0.0, "warmup_linear", 0.9, 0.999)])
    ops.sched_step_ex(steps, sc, hs, [(0, -1, 0.0, "warmup_linear", 0.9, 0.999)])  # (not the first step)

    def launch(rule, kw):
        a = (p, g, m, v, sh, sqn, 5.0, 1e-5, sc, 0.9, 0.999, 1e-6 if rule == "bertadam" else 1e-8, 0.01)
        ops.optim_multi(rule, [(a, {}, {} if rule == "bertadam" else dict(kw, step_scalars=hs))])

    times = {i: [] for i in range(len(RULES))}
    for r in range(ROUNDS + 1):
        for i, (rule, kw, _) in enumerate(RULES):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            launch(rule, kw)
            e0.record()
            for _ in range(REPS):
                launch(rule, kw)
            e1.record()
            e1.synchronize()
            if r:  # round 0 warms up
                times[i].append(e0.elapsed_time(e1) * 1e-3 / REPS)
    for i, (rule, kw, nbytes) in enumerate(RULES):
        t = statistics.median(times[i])
        print("%-9s %-28s %2d B/param: %7.1f us per launch (min %7.1f), %4.0f GB/s"
              % (rule, ",".join("%s=%s" % kv for kv in kw.items()), nbytes, t * 1e6, min(times[i]) * 1e6, nbytes * N / t / 1e9),
              flush=True)


if __name__ == "__main__":
    main()
