"""The mapped update (split_groups: lr / weight decay per tensor from a device map) against the unmapped launch of the
same build, at the size of the full model: 220.8 M elements in synthetic flat buffers, bf16 gradients, bf16 shadow on,
BertAdam rule, one span.  The two are timed alternating, ROUNDS times REPS launches each, with device events; per round
the mean launch time.  Bytes: 4 + 2 + 4 + 4 read, 4 + 4 + 4 + 2 written = 28 B per element with bf16 gradients (30 B
with fp32 ones), + 1/8 B of map.  Prints one JSON line; ``--out FILE`` also writes it there.

    python tools/bench_split_update.py [--n 220800000] [--groups 5] [--rounds 7] [--reps 10] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=220_800_000)
    ap.add_argument("--groups", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: a time taken anywhere else says nothing"
    from xggm_amd import arena, ops
    dev = "cuda"
    n = a.n // 256 * 256
    p = torch.randn(n, device=dev) * 0.02
    g = (torch.randn(n, device=dev) * 1e-3).to(torch.bfloat16)
    m = torch.zeros(n, device=dev)
    v = torch.zeros(n, device=dev)
    sh = torch.empty(n, device=dev, dtype=torch.bfloat16)
    sq = torch.ones(1, device=dev)
    scale = torch.ones(1, device=dev)
    # tensors of a transformer's sizes, param_groups round-robin: matrices of 768 x 768 and 3072 x 768 with their biases and
    # LayerNorm vectors in between, so that the ids change inside waves as they do in the arena's vector regions
    info, owner, off, i = {}, {}, 0, 0
    sizes = [768 * 768, 768, 768, 3072 * 768, 3072, 768 * 3072, 768, 768, 768]
    while off < n:
        k = min(sizes[i % len(sizes)], n - off)
        info["t%d" % i] = (off, k, "g", False)
        owner["t%d" % i] = 1 + i % a.groups
        off = (off + k + 7) // 8 * 8
        i += 1
    ids = torch.from_numpy(arena.hyper_id_map(info, owner, n)).to(dev)
    table = torch.tensor([[0.0, 0.0]] + [[1e-5 * (1 + j), 0.01 * (j % 2)] for j in range(a.groups)], device=dev)
    job = ((p, g, m, v, sh, sq, 5.0, 1e-5, scale, 0.9, 0.999, 1e-6, 0.01), dict(elem0=0), {})
    run = {"unmapped": lambda: ops.optim_multi("bertadam", [job]),
           "mapped": lambda: ops.optim_multi("bertadam", [job], hyper_map=(ids, table))}
    for f in run.values():  # warm-up: code objects, clocks
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in run}
    for _ in range(a.rounds):
        for k, f in run.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                f()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1e3 / a.reps)  # us per launch
    med = {k: statistics.median(t) for k, t in times.items()}
    out = dict(tool="bench_split_update", device=torch.cuda.get_device_name(0), elements=n, tensors=i, groups=a.groups,
               rounds=a.rounds, reps=a.reps, map_bytes=int(ids.numel()), bytes_per_element=28.0,
               byte_growth_pct=round(100.0 * (ids.numel() / n) / 28.0, 3),  # (0.417 against the 30 B of fp32 gradients)
               us_per_launch={k: [round(x, 1) for x in t] for k, t in times.items()},
               median_us={k: round(x, 1) for k, x in med.items()},
               spread_pct={k: round(100.0 * (max(t) - min(t)) / med[k], 2) for k, t in times.items()},
               unmapped_GBps=round(28.0 * n / med["unmapped"] / 1e3, 0),
               mapped_over_unmapped_pct=round(100.0 * (med["mapped"] / med["unmapped"] - 1.0), 2),
               finite=bool(np.isfinite(float(p.abs().max()))))
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
