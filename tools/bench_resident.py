"""What the device-resident data set costs and saves (xggm_amd.tools.resident), one process, GPU only:

  (a) the gather launch alone: ``ops.batch_gather`` at B = 32 and 92, N = 36, F = 2048, A = 2274, T = 20 over a random
      order of 4096 images (604 MB of bf16 features: the rows of a launch are cold), device events around 256 launches,
      repeated -- replayed from one graph (the device's time) and issued from Python (the host's); us per launch and GB/s
      over the bytes the algorithm moves (read + written, from the shapes below);
  (b) the full-size captured iteration at batch 32 bf16 under three feeds of the SAME trainer -- the static batch,
      ``load_packed`` from ``DataLoaderX(handover="inline")`` and ``load_resident`` -- legs alternating and repeated, host
      clock around windows that end in a synchronise.  The spread of the static leg between its repeats is the yardstick:
      the resident leg must not be slower than the loader leg by more than it.

    python tools/bench_resident.py [--out profiles/resident/resident_ab.txt] [--repeats 5] [--steps 30]
"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def gather_bytes(B, N, F, A, T, K, feat_bytes=2):
    """bytes one launch reads + writes: per row the feature row, boxes and adjacency in and out, the question's ids / length /
    image row / label slots and its order entry in, three int64 sentence rows and the target row out"""
    read = N * F * feat_bytes + N * 16 + N * N * 4 + T * 4 + 4 + 4 + K * 8 + 8
    written = N * F * feat_bytes + N * 16 + N * N * 4 + 3 * T * 8 + A * 4
    return B * (read + written)


def leg_gather(out, dev, n_img=4096, launches=256, repeats=5):
    from xggm_amd import ops
    N, F, A, T, K = 36, 2048, 2274, 20, 3
    g = torch.Generator(device="cpu").manual_seed(0)
    n_q = 2 * n_img
    tables = dict(feats=torch.randn(n_img, N, F, device=dev).to(torch.bfloat16), boxes=torch.rand(n_img, N, 4, device=dev),
                  adj=torch.rand(n_img, N, N, device=dev),
                  q_row=torch.randint(0, n_img, (n_q,), generator=g).to(torch.int32).to(dev),
                  q_ids=torch.randint(1, 30000, (n_q, T), generator=g).to(torch.int32).to(dev),
                  q_len=torch.randint(2, T + 1, (n_q,), generator=g).to(torch.int32).to(dev),
                  q_label=torch.stack([torch.randperm(A, generator=g)[:K] for _ in range(n_q)]).to(torch.int32).to(dev),
                  q_score=torch.rand(n_q, K, device=dev))
    for B in (32, 92):
        order = torch.randint(0, n_q, (launches * B,), generator=g).to(dev)
        outs = dict(feats=torch.empty(B, N, F, device=dev, dtype=torch.bfloat16), boxes=torch.empty(B, N, 4, device=dev),
                    adj_true=torch.empty(B, N, N, device=dev), input_ids=torch.empty(B, T, device=dev, dtype=torch.int64),
                    input_mask=torch.empty(B, T, device=dev, dtype=torch.int64),
                    segment_ids=torch.empty(B, T, device=dev, dtype=torch.int64), target=torch.empty(B, A, device=dev))
        def issue():
            for i in range(launches):
                ops.batch_gather(tables, order, i * B, B, outs)

        # the same 256 launches (every one its own rows of the order) as ONE graph: the device's time per launch without the
        # host's -- issued from Python the stream runs dry between two launches and the events time the interpreter
        issue()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            issue()
        nb = gather_bytes(B, N, F, A, T, K)
        for how, run in (("replayed from one graph", graph.replay), ("issued from Python", issue)):
            us = []
            for r in range(repeats + 1):  # the first repeat warms up
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                run()
                e1.record()
                e1.synchronize()
                if r:
                    us.append(1000.0 * e0.elapsed_time(e1) / launches)
            med = statistics.median(us)
            out("(a) batch_gather B=%d N=%d F=%d A=%d T=%d K=%d bf16->bf16, %d images, %d launches x %d repeats, %s: "
                "median %.2f us/launch (min %.2f, max %.2f), %d bytes/launch read+written -> %.0f GB/s at the median"
                % (B, N, F, A, T, K, n_img, launches, repeats, how, med, min(us), max(us), nb, nb / med / 1e3))


def leg_iteration(out, dev, repeats, steps):
    import random
    from xggm_amd.engine import CapturedTrainer
    from xggm_amd.tools.resident import ResidentDataset
    args = bench.parse(["--steps", str(steps), "--warmup", "5"])
    model, optim, batch = bench.build(args, dev)
    loader, _, tmp = bench.make_loader(model, args, dev)
    assert loader.handover == "inline"
    tr = CapturedTrainer(model, optim, batch, sigma=1.0, order="vqa", packed_spec=loader.spec)
    store = ResidentDataset(loader.ds, model.lxrt_encoder.batcher, dev, batch_size=args.batch)
    order = store.order(0, seed=args.seed)
    starts = list(range(0, len(order) - args.batch + 1, args.batch))
    rng = random.Random(0)
    it = iter(loader)
    k = [0]

    def br():
        return "rel" if rng.randint(1, 10) <= args.delta else "node"

    def static():
        tr.iteration(br())

    def packed():
        next(it)
        tr.load_packed(it)
        tr.iteration(br())

    def resident():
        tr.load_resident(store, starts[k[0] % len(starts)])
        k[0] += 1
        tr.iteration(br())

    legs = (("static batch", static), ("load_packed (DataLoaderX inline)", packed), ("load_resident", resident))
    ms = {name: [] for name, _ in legs}
    for r in range(repeats + 1):  # the first round warms every leg up
        for name, step in legs:
            for _ in range(3):
                step()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                step()
            torch.cuda.synchronize()
            if r:
                ms[name].append(1000.0 * (time.perf_counter() - t0) / steps)
    it.close()
    med = {name: statistics.median(v) for name, v in ms.items()}
    for name, _ in legs:
        out("(b) batch %d bf16 captured iteration, %-34s median %.3f ms (min %.3f, max %.3f; %d repeats x %d steps; %+.3f vs static)"
            % (args.batch, name + ":", med[name], min(ms[name]), max(ms[name]), repeats, steps, med[name] - med["static batch"]))
    spread = max(ms["static batch"]) - min(ms["static batch"])
    diff = med["load_resident"] - med["load_packed (DataLoaderX inline)"]
    out("(b) spread of the static leg between its repeats (max - min): %.3f ms; load_resident - load_packed = %+.3f ms: %s"
        % (spread, diff, "within the condition (not slower than the loader leg by more than the spread)" if diff <= spread
           else "CONDITION MISSED (slower than the loader leg by more than the spread)"))
    import shutil
    shutil.rmtree(tmp, ignore_errors=True)
    return diff <= spread


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "resident", "resident_ab.txt"))
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--steps", type=int, default=30)
    p.add_argument("--only", choices=["a", "b"], default=None)
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_resident: needs a GPU (nothing here is measured on a CPU)")
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)

    out("# python tools/bench_resident.py --repeats %d --steps %d   (%s)" % (a.repeats, a.steps, torch.cuda.get_device_name(0)))
    ok = True
    if a.only != "b":
        leg_gather(out, dev, repeats=a.repeats)
    if a.only != "a":
        ok = leg_iteration(out, dev, a.repeats, a.steps)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
