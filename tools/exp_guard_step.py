"""What the replica drift guard costs INSIDE the captured engine, on one GPU: the full-size step of bench.py on the
one-rank RCCL group (XGGM_DP_FORCE=1, the N > 1 code path: exchanges between the graphs), the SAME trainer and graphs with
the guard checking after every iteration (check_every=1) against the guard switched off (every = None: ``tick`` does
nothing, the parent's path), in alternating blocks.
  XGGM_DP_FORCE=1 MASTER_ADDR=127.0.0.1 MASTER_PORT=29591 python tools/exp_guard_step.py [--blocks 8] [--iters 20]
Host clock around blocks that end in a device synchronise; medians over the blocks.  (per-iteration difference) is the cost
of ONE ``weights`` check in the loop, the read-back's stall of the launch queue included; divided by the iteration time
it gives the check_every at which the overhead falls below 0.1 %.  A one-GPU number: the collective has one rank."""
import argparse
import os
import random
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=8)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--level", default="weights", choices=["weights", "state"])
    args = ap.parse_args()
    if not os.environ.get("XGGM_DP_FORCE"):
        sys.exit("set XGGM_DP_FORCE=1 (and MASTER_ADDR / MASTER_PORT): the guard compares nothing without a process group")
    import torch.distributed as dist
    import bench
    from xggm_amd.engine import CapturedTrainer
    from xggm_amd.runtime import runtime_of
    from xggm_amd.vqa.vqacpv2 import enable_data_parallel
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda:0"))
    model, optim, batch = bench.build(bench.parse(["--batch", "32", "--answers", "2274"]), "cuda")
    runtime_of(model)
    enable_data_parallel(model, wire_dtype=torch.bfloat16, check_every=1, check_level=args.level)
    guard = model._replica_guard
    trainer = CapturedTrainer(model, optim, batch, sigma=1.0, order="vqa")
    rng = random.Random(9595)

    def block(every):
        guard.every = every
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.iters):
            trainer.iteration("rel" if rng.randint(1, 10) <= 5 else "node")
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / args.iters

    for every in (None, 1):  # warm-up of both paths
        block(every)
    ms = {None: [], 1: []}
    for _ in range(args.blocks):
        for every in (None, 1):
            ms[every].append(block(every))
    off, on = statistics.median(ms[None]), statistics.median(ms[1])
    print("guard off: median %.3f ms per iteration (blocks: %s)" % (off, " ".join("%.3f" % x for x in ms[None])))
    print("guard on, check_every=1, level %s: median %.3f ms per iteration (blocks: %s)"
          % (args.level, on, " ".join("%.3f" % x for x in ms[1])))
    cost = on - off
    print("one check in the loop: %.3f ms = %.2f %% of an iteration; below 0.1 %% from check_every = %d  (%d checks made)"
          % (cost, 100 * cost / off, max(1, -(-cost // (0.001 * off))), guard.checks))
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
