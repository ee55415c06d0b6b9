"""What a replica drift check costs on ONE GPU at full size: the fingerprint kernel (xggm_fingerprint_spans) over the
tables of ``dist.ReplicaGuard`` at levels "weights" and "state" of the model bench.py builds, beside the project's
existing read-only streaming kernel, xggm_sqnorm_multi_f32, over the same fp32 ranges in the same process.
  python tools/bench_fingerprint.py [--reps 60]
Every figure is the median of event-timed launches after warm-up, fingerprint and yardstick alternating.
With XGGM_DP_FORCE=1 (MASTER_ADDR / MASTER_PORT set) it also times ``ReplicaGuard.check`` end to end -- launch, the MAX
all-reduce of the one-rank RCCL group, the read-back -- by the host clock around a device synchronise: the single-rank
cost of a check between two replays.  One-GPU numbers: nothing here says how the collective behaves across GPUs."""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, reps):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in ev]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=60)
    args = ap.parse_args()
    import bench
    from xggm_amd import ops
    from xggm_amd.dist import ReplicaGuard
    from xggm_amd.fingerprint import SALT, fingerprint_table
    from xggm_amd.runtime import runtime_of
    force = bool(os.environ.get("XGGM_DP_FORCE"))
    if force:
        import torch.distributed as dist
        torch.cuda.set_device(0)
        dist.init_process_group("nccl", rank=0, world_size=1)
    model, _, _ = bench.build(bench.parse(["--batch", "32", "--answers", "2274"]), "cuda")
    arena = runtime_of(model).arena
    print("arena: %d elements in %d groups (%s)" % (arena.total, len(arena.groups), ", ".join(arena.groups)))
    sq = torch.zeros(1, device="cuda")
    for level in ("weights", "state"):
        guard = ReplicaGuard(arena, level=level)
        plan = guard.plan()
        items = [(getattr(arena, buf), s, e, SALT[buf]) for buf, g, s, e in plan]
        nbytes = sum((e - s) * t.element_size() for t, s, e, _ in items)
        f32 = {}
        for buf, g, s, e in plan:
            if getattr(arena, buf).dtype == torch.float32 and e > s:
                f32.setdefault(buf, []).append((s, e))
        f32_bytes = 4 * sum(e - s for rs in f32.values() for s, e in rs)
        f32_items = [(getattr(arena, buf), s, e, SALT[buf]) for buf, rs in f32.items() for s, e in rs]

        def yard():
            for buf, rs in f32.items():
                ops.sqnorm_multi(getattr(arena, buf), rs, sq)

        fns = {"fingerprint, whole table": lambda: fingerprint_table(items),
               "fingerprint, fp32 ranges": lambda: fingerprint_table(f32_items),
               "sqnorm_multi, fp32 ranges": yard}
        for fn in fns.values():
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        ts = {k: [] for k in fns}
        per = 10
        for _ in range(max(1, args.reps // per)):  # alternating blocks
            for k, fn in fns.items():
                ts[k] += timed(fn, per)
        med = {k: statistics.median(v) for k, v in ts.items()}
        print("level %-7s: %d ranges, %.1f MB (%.1f MB of it fp32 in %d launch pair(s) of the yardstick)"
              % (level, len(plan), nbytes / 1e6, f32_bytes / 1e6, len(f32)))
        for k, b in (("fingerprint, whole table", nbytes), ("fingerprint, fp32 ranges", f32_bytes),
                     ("sqnorm_multi, fp32 ranges", f32_bytes)):
            v = sorted(ts[k])
            print("   %-26s median %8.1f us  (min %8.1f, p90 %8.1f; %d launches)  %7.1f GB/s"
                  % (k, 1e3 * med[k], 1e3 * v[0], 1e3 * v[int(0.9 * (len(v) - 1))], len(v), b / med[k] / 1e6))
        print("   fingerprint / sqnorm_multi on the same fp32 ranges: %.3f"
              % (med["fingerprint, fp32 ranges"] / med["sqnorm_multi, fp32 ranges"]))
        if force:
            guard = ReplicaGuard(arena, level=level)
            for _ in range(3):
                guard.check()
            torch.cuda.synchronize()
            host = []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                guard.check()
                torch.cuda.synchronize()
                host.append(1e3 * (time.perf_counter() - t0))
            host.sort()
            print("   ReplicaGuard.check end to end (one-rank RCCL group, host clock): median %.3f ms (min %.3f, p90 %.3f)"
                  % (statistics.median(host), host[0], host[int(0.9 * (len(host) - 1))]))
    if force:
        import torch.distributed as dist
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
