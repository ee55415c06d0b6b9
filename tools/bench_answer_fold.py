"""What merging the data-parallel ranks' answer logs costs on the device; one process, one GPU, synthetic gathered logs at
VQA-CP v2 test size (219 928 answers) for a world of 8:

  leg A  the fold launch (``ops.answer_log_fold`` / xggm_answer_log_fold): labels, scores, the header and the flag in ONE launch;
  leg B  the torch composition of the same merge: one slice copy per rank and buffer (labels, scores) plus the ranks' cursors.

Two shapes: CONCAT without scores (a validation sweep cut by ``dist.shard_range``) and INTERLEAVE with scores at block 32 (a
training epoch of 859 global steps).  Each leg is measured twice: alone, 64 issues replayed from one graph between device
events (leg B then without its read of the cursors, which is a host synchronisation); and as a whole call under the host
clock, ending in the read-back the caller needs (A: the flag word; B: the ``world`` cursors).  Legs alternate; the first
round is discarded.  No target: the file records what was measured.  Nothing here says anything about the sweep itself, which
a world of 8 divides over 8 GPUs: that cannot be measured on one card.

    python tools/bench_answer_fold.py [--out profiles/finetune/answer_fold_ab.txt] [--repeats 7]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_TEST, WORLD, BLOCK, LAUNCHES = 219928, 8, 32, 64


def _stats(v):
    return "median %.3f (min %.3f, max %.3f)" % (statistics.median(v), min(v), max(v))


def shape(out, dev, repeats, layout_name):
    from xggm_amd import answers as A, ops
    from xggm_amd.dist import shard_range
    from xggm_amd.engine import AnswerLog
    concat = layout_name == "CONCAT"
    with_scores = not concat
    if concat:
        layout, expect = ops.FOLD_CONCAT, [len(shard_range(N_TEST, r, WORLD)) for r in range(WORLD)]
    else:
        layout, expect = ops.FOLD_INTERLEAVE, [N_TEST // (BLOCK * WORLD) * BLOCK] * WORLD
    cap, total = max(expect), sum(expect)
    W = A.packed_words(cap, with_scores)
    rng = np.random.default_rng(0)
    bufs = np.zeros((WORLD, W), dtype=np.int64)
    for r, n in enumerate(expect):
        bufs[r, 0] = n
        bufs[r, 3:3 + cap] = rng.integers(0, 3129, cap)
        if with_scores:
            bufs[r, 3 + cap:].view(np.float32)[:cap] = rng.random(cap, dtype=np.float32)
    g = torch.from_numpy(bufs).to(dev)
    dst, ref = AnswerLog(total, dev, with_scores=with_scores), AnswerLog(total, dev, with_scores=with_scores)
    flag = torch.zeros(1, dtype=torch.int64, device=dev)
    flag_host, cur_host = torch.zeros(1, dtype=torch.int64).pin_memory(), torch.zeros(WORLD, dtype=torch.int64).pin_memory()
    first = np.concatenate([[0], np.cumsum(expect)[:-1]])
    steps = expect[0] // BLOCK

    def fold():
        ops.answer_log_fold(g, dst, flag, cap, with_scores, layout, expect, block=BLOCK)

    def torch_copies():
        for r, n in enumerate(expect):
            src_l = g[r, 3:3 + n]
            src_s = g[r, 3 + cap:].view(torch.float32)[:n] if with_scores else None
            if concat:
                ref.labels[first[r]:first[r] + n].copy_(src_l)
                if with_scores:
                    ref.scores[first[r]:first[r] + n].copy_(src_s)
            else:
                ref.labels[:total].view(steps, WORLD, BLOCK)[:, r].copy_(src_l.view(steps, BLOCK))
                if with_scores:
                    ref.scores[:total].view(steps, WORLD, BLOCK)[:, r].copy_(src_s.view(steps, BLOCK))

    def call_a():
        fold()
        flag_host.copy_(flag, non_blocking=True)
        torch.cuda.current_stream().synchronize()
        return int(flag_host[0])

    def call_b():
        torch_copies()
        cur_host.copy_(g[:, 0], non_blocking=True)
        torch.cuda.current_stream().synchronize()
        return cur_host.tolist() == expect

    assert call_a() == 0 and call_b()
    same = torch.equal(dst.labels[:total], ref.labels[:total]) and (not with_scores or torch.equal(dst.scores[:total], ref.scores[:total]))
    nbytes = total * (8 + (4 if with_scores else 0)) * 2
    out("%s, world %d, %d answers (%s per rank), %s: the two legs leave the same labels%s: %s; %d bytes read + written"
        % (layout_name, WORLD, total, "%d .. %d" % (min(expect), max(expect)), "with scores, block %d" % BLOCK if with_scores else "no scores",
           " and scores" if with_scores else "", same, nbytes))
    assert same
    graphs = {}
    for name, fn in (("A", fold), ("B", torch_copies)):
        graphs[name] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[name]):
            for _ in range(LAUNCHES):
                fn()
    us, ms = {"A": [], "B": []}, {"A": [], "B": []}
    for r in range(repeats + 1):  # the first round warms both legs up and is discarded
        for name in ("A", "B"):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            graphs[name].replay()
            e1.record()
            e1.synchronize()
            if r:
                us[name].append(1000.0 * e0.elapsed_time(e1) / LAUNCHES)
        for name, fn in (("A", call_a), ("B", call_b)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            if r:
                ms[name].append(1000.0 * (time.perf_counter() - t0))
    out("  leg A  xggm_answer_log_fold alone, %d launches replayed from one graph: %s us per fold -> %.0f GB/s at the median"
        % (LAUNCHES, _stats(us["A"]), nbytes / statistics.median(us["A"]) / 1e3))
    out("  leg B  torch slice copies alone (%d copies per merge), %d merges replayed from one graph: %s us per merge"
        % (WORLD * (2 if with_scores else 1), LAUNCHES, _stats(us["B"])))
    out("  leg A  whole call, host clock (launch + read-back of the flag): %s ms, %d repeats" % (_stats(ms["A"]), repeats))
    out("  leg B  whole call, host clock (copies + read-back of %d cursors): %s ms, %d repeats" % (WORLD, _stats(ms["B"]), repeats))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "finetune", "answer_fold_ab.txt"))
    p.add_argument("--repeats", type=int, default=7)
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_answer_fold: needs a GPU (nothing here is measured on a CPU)")
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)

    out("# python tools/bench_answer_fold.py --repeats %d   (%s)" % (a.repeats, torch.cuda.get_device_name(0)))
    for name in ("CONCAT", "INTERLEAVE"):
        shape(out, dev, a.repeats, name)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
