"""BertLamb's update against BertAdam's, same build, same process, at the full-size arena.

Part 1, the launches.  Flat buffers with the layout of the full 9/5/5 model (``arena.layout`` over ``oracle.shapes``: the
real offsets, groups and tensor table; no model is built), fp32 gradients, bf16 shadow on, the clip's norm given.  Two legs
alternate: ``ops.optim_multi("bertadam")`` over the arena groups (the code every run uses today) and ``ops.lamb_multi``
over the same spans (phase A, finish, phase B).  ROUNDS + 1 rounds of REPS calls each, timed with device events; the first
round is discarded; median and spread (max - min over the median) per leg.  Byte model: BertAdam reads 16 and writes 14 B
per parameter, phase A reads 16 and writes 8, phase B reads 12 and writes 6: 42 / 30 = 1.40.

Part 2 (``--iteration``), the captured iteration.  Two full-size models from bench.py's own ``build`` (batch 32, bf16), one
with ``make_optimizer``'s BertAdam and one with ``optim='bertlamb'``; ROUNDS + 1 rounds that alternate ITERS replayed
iterations of each trainer, wall time per iteration between device synchronisations; first round discarded.

    python tools/bench_lamb.py [--rounds 7] [--reps 10] [--iteration] [--iters 10] [--out profiles/optim/lamb_ab.txt]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class _Shape:
    def __init__(self, s):
        self.shape = tuple(s)

    def dim(self):
        return len(self.shape)

    def numel(self):
        return int(np.prod(self.shape))


def summary(times):
    med = statistics.median(times)
    return dict(median=round(med, 2), min=round(min(times), 2), max=round(max(times), 2),
                spread_pct=round(100.0 * (max(times) - min(times)) / med, 2))


def launches(a):
    from oracle import shapes
    from xggm_amd import arena, ops
    dev = "cuda"
    sh = shapes.model_shapes(shapes.FULL, 3129)
    order, groups, info, total = arena.layout([(n, _Shape(s)) for n, s in sh.items()], arena.default_group_of)
    table, names = arena.lamb_tensor_table(info, {n: not (n.endswith("bias") or len(sh[n]) == 1) for n in info}, total)
    params = int(table[:, 1].sum())
    p = torch.zeros(total, device=dev)
    g = torch.zeros(total, device=dev)
    for o, k, _ in table.tolist():  # the gaps hold zeros, as in an arena
        p[o:o + k].normal_(0.0, 0.02)
        g[o:o + k].normal_(0.0, 1e-3)
    m = torch.zeros(total, device=dev)
    v = torch.zeros(total, device=dev)
    shd = torch.zeros(total, device=dev, dtype=torch.bfloat16)
    sq = torch.ones(1, device=dev)
    scale = torch.ones(1, device=dev)
    jobs = []
    for gname in order:
        G = groups[gname]
        sl = slice(G.start, G.end)
        jobs.append(((p[sl], g[sl], m[sl], v[sl], shd[sl], sq, 5.0, 1e-6, scale, 0.9, 0.999, 1e-6, 0.01), dict(elem0=G.start), {}))
    tensors = torch.from_numpy(table).to(dev)
    ratios = torch.ones(len(names), device=dev)
    ws = ops.lamb_workspace(total, len(names), dev)
    run = {"bertadam": lambda: ops.optim_multi("bertadam", jobs),
           "bertlamb": lambda: ops.lamb_multi(jobs, tensors, ratios, ws)}
    times = {k: [] for k in run}
    for r in range(a.rounds + 1):
        for k, f in run.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            f()
            e0.record()
            for _ in range(a.reps):
                f()
            e1.record()
            e1.synchronize()
            if r:  # round 0 warms up: code objects, clocks
                times[k].append(e0.elapsed_time(e1) * 1e3 / a.reps)
    out = {k: summary(t) for k, t in times.items()}
    ratio = out["bertlamb"]["median"] / out["bertadam"]["median"]
    rl = ratios.tolist()
    return dict(part="launches, us per call", elements=total, parameters=params, tensors=len(names), spans=len(jobs),
                rounds=a.rounds, reps=a.reps, us=out, bertadam_GBps=round(30.0 * params / out["bertadam"]["median"] / 1e3),
                bertlamb_GBps=round(42.0 * params / out["bertlamb"]["median"] / 1e3), byte_model_ratio=1.4,
                measured_ratio=round(ratio, 3), workspace_bytes=int(ws.numel() * 8), table_bytes=int(tensors.numel() * 8),
                ratios_finite=bool(np.isfinite(rl).all()), ratio_min=round(min(rl), 4), ratio_max=round(max(rl), 4))


def iterations(a):
    import random
    import bench
    from xggm_amd.engine import CapturedTrainer
    from xggm_amd.vqa.vqacpv2 import make_optimizer
    args = bench.parse(["--gpus", "1", "--steps", str(a.iters), "--warmup", "2"])
    args.batch, args.answers = args.batch or 32, args.answers or 2274
    trainers = {}
    for name in ("bertadam", "bertlamb"):
        model, optim, batch = bench.build(args, "cuda")
        if name == "bertlamb":
            optim = make_optimizer(model, optim.param_groups[-1]["lr"], optim.param_groups[-1]["t_total"], optim="bertlamb")
        trainers[name] = CapturedTrainer(model, optim, batch, sigma=1.0, order=args.order)
    rng = random.Random(args.seed)
    plan = [["rel" if rng.randint(1, 10) <= args.delta else "node" for _ in range(a.iters)] for _ in range(a.rounds + 1)]
    times = {k: [] for k in trainers}
    for r, branches in enumerate(plan):
        for k, tr in trainers.items():
            tr.iteration(branches[0])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for br in branches:
                tr.iteration(br)
            torch.cuda.synchronize()
            if r:
                times[k].append((time.perf_counter() - t0) * 1e3 / len(branches))
    out = {k: summary(t) for k, t in times.items()}
    return dict(part="captured iteration, ms (batch %d, bf16, one GPU)" % args.batch, rounds=a.rounds, iters=a.iters, ms=out,
                bertlamb_minus_bertadam_ms=round(out["bertlamb"]["median"] - out["bertadam"]["median"], 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--iteration", action="store_true")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: a time taken anywhere else says nothing"
    lines = ["tool: tools/bench_lamb.py; device: %s" % torch.cuda.get_device_name(0), json.dumps(launches(a))]
    print(lines[-1], flush=True)
    if a.iteration:
        lines.append(json.dumps(iterations(a)))
        print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
