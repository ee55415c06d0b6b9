"""What the label adjacency costs and saves (preprocess.compute_adjacency, csrc/label_adjacency.hip), one process, GPU only:

  (a) a split's adjacency by ``build_adjacency`` (gather two [chunk, N, 768] embedding tensors per chunk of 4096 images,
      one cosine workgroup per image) against ``label_pair_table`` + ``build_adjacency_from_labels`` (one 1600 x 400 table,
      then look-ups): 123 000 images x 36 boxes and 148 000 x 100 boxes, synthetic ids, 1600 x 400 labels, D = 768.  Host
      clock around calls that end in a synchronise, legs alternating and repeated; the two results are compared with
      ``torch.equal`` once.  Byte floors from the shapes: the n N N 4 bytes of output are in both;
  (b) the gather launch at B = 32, F = 2048, A = 2274, T = 20 over a random order of 4096 images with a STORED adjacency
      (``xggm_batch_gather``) against one MADE from labels (``xggm_batch_gather_labels``), N = 36 and 100: 256 launches
      replayed from one graph, device events, legs alternating and repeated.  No threshold: the trade is memory (the
      [n_img, N, N] table against a 2.56 MB pair table), and it is opt-in; a difference beyond the run-to-run spread is
      reported as such.

    python tools/bench_label_adjacency.py [--out profiles/ingest/label_adjacency_ab.txt] [--repeats 5]
"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VC, VA, D = 1600, 400, 768
SPEC_TBS = 8.0  # HBM3E peak of the MI355X


def copy_rate(dev):
    """measured device-to-device copy rate, TB/s over bytes read + written (1 GiB, median of 5)"""
    a = torch.empty(1 << 28, device=dev)
    b = torch.empty_like(a)
    ms = []
    for r in range(6):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        b.copy_(a)
        e1.record()
        e1.synchronize()
        if r:
            ms.append(e0.elapsed_time(e1))
    return 2 * a.numel() * 4 / statistics.median(ms) / 1e9


def builder_bytes(n, N):
    """(parent, label path): bytes each must move at the least.  Parent: the gathered embeddings written and read again
    (2 n N D 4 each way) on top of the table rows the gather reads (at least the two tables once), ids, and the output.
    Label path: the embeddings once for the table, the table written, per image 2 N ids and the output (the table itself
    stays in cache)."""
    out = n * N * N * 4
    parent = 2 * (2 * n * N * D * 4) + (VC + VA) * D * 4 + 2 * n * N * 8 + out
    label = (VC + VA) * D * 4 + VC * VA * 4 + 2 * n * N * 4 + out
    return parent, label, out


def leg_builder(out, dev, repeats, rate):
    from xggm_amd.preprocess.compute_adjacency import build_adjacency, build_adjacency_from_labels, label_pair_table
    g = torch.Generator(device="cpu").manual_seed(0)
    cls, att = torch.randn(VC, D, generator=g).to(dev), torch.randn(VA, D, generator=g).to(dev)
    for n, N in ((123_000, 36), (148_000, 100)):
        oid, aid = torch.randint(0, VC, (n, N), generator=g).to(dev), torch.randint(0, VA, (n, N), generator=g).to(dev)

        def parent():
            return build_adjacency(cls, att, oid, aid)

        def label():
            return build_adjacency_from_labels(label_pair_table(cls, att), oid, aid)

        same = torch.equal(parent(), label())  # also the warm-up of both legs
        torch.cuda.synchronize()
        ms = {"parent": [], "label": []}
        for _ in range(repeats):
            for name, fn in (("parent", parent), ("label", label)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                r = fn()
                torch.cuda.synchronize()
                ms[name].append(1000.0 * (time.perf_counter() - t0))
                del r
        pb, lb, ob = builder_bytes(n, N)
        mp, ml = statistics.median(ms["parent"]), statistics.median(ms["label"])
        out("(a) %d images x %d boxes, %d x %d labels, D = %d: results torch.equal: %s; output n N N 4 = %.1f MB"
            % (n, N, VC, VA, D, same, ob / 1e6))
        out("(a)   build_adjacency (chunks of 4096):               median %.1f ms (min %.1f, max %.1f; %d repeats); %.1f GB at the least "
            "-> floor %.1f ms at %.2f TB/s (measured copy rate), %.1f ms at %.0f TB/s (spec): %.1fx the measured-rate floor"
            % (mp, min(ms["parent"]), max(ms["parent"]), repeats, pb / 1e9, pb / rate / 1e9, rate, pb / SPEC_TBS / 1e9, SPEC_TBS,
               mp / (pb / rate / 1e9)))
        out("(a)   label_pair_table + build_adjacency_from_labels: median %.1f ms (min %.1f, max %.1f); %.3f GB at the least "
            "-> floor %.2f ms (measured rate), %.2f ms (spec): %.1fx the measured-rate floor"
            % (ml, min(ms["label"]), max(ms["label"]), lb / 1e9, lb / rate / 1e9, lb / SPEC_TBS / 1e9, ml / (lb / rate / 1e9)))
        spread = max(max(v) - min(v) for v in ms.values())
        out("(a)   parent - label = %.1f ms at the medians (parent / label = %.1fx), the larger spread of either side's repeats is %.1f ms: %s"
            % (mp - ml, mp / ml, spread, "the label path is faster by more than the spread" if mp - ml > spread else
               "the label path is slower by more than the spread" if ml - mp > spread else "no difference beyond the spread"))
        del oid, aid
        torch.cuda.empty_cache()


def leg_gather(out, dev, repeats, n_img=4096, launches=256):
    from xggm_amd import ops
    from xggm_amd.preprocess.compute_adjacency import build_adjacency_from_labels, label_pair_table
    F, A, T, K, B = 2048, 2274, 20, 3, 32
    g = torch.Generator(device="cpu").manual_seed(1)
    pair = label_pair_table(torch.randn(VC, D, generator=g).to(dev), torch.randn(VA, D, generator=g).to(dev))
    n_q = 2 * n_img
    for N in (36, 100):
        ol = torch.randint(0, VC, (n_img, N), generator=g).to(torch.int32).to(dev)
        al = torch.randint(0, VA, (n_img, N), generator=g).to(torch.int32).to(dev)
        base = dict(feats=torch.randn(n_img, N, F, device=dev).to(torch.bfloat16), boxes=torch.rand(n_img, N, 4, device=dev),
                    q_row=torch.randint(0, n_img, (n_q,), generator=g).to(torch.int32).to(dev),
                    q_ids=torch.randint(1, 30000, (n_q, T), generator=g).to(torch.int32).to(dev),
                    q_len=torch.randint(2, T + 1, (n_q,), generator=g).to(torch.int32).to(dev),
                    q_label=torch.stack([torch.randperm(A, generator=g)[:K] for _ in range(n_q)]).to(torch.int32).to(dev),
                    q_score=torch.rand(n_q, K, device=dev))
        stored = dict(base, adj=build_adjacency_from_labels(pair, ol, al))
        labels = dict(base, pair_table=pair, obj_labels=ol, attr_labels=al)
        order = torch.randint(0, n_q, (launches * B,), generator=g).to(dev)
        graphs, outs = {}, {}
        for name, tables in (("stored", stored), ("labels", labels)):
            o = dict(feats=torch.empty(B, N, F, device=dev, dtype=torch.bfloat16), boxes=torch.empty(B, N, 4, device=dev),
                     adj_true=torch.empty(B, N, N, device=dev), input_ids=torch.empty(B, T, device=dev, dtype=torch.int64),
                     input_mask=torch.empty(B, T, device=dev, dtype=torch.int64),
                     segment_ids=torch.empty(B, T, device=dev, dtype=torch.int64), target=torch.empty(B, A, device=dev))

            def issue(tables=tables, o=o):
                for i in range(launches):
                    ops.batch_gather(tables, order, i * B, B, o)

            issue()
            torch.cuda.synchronize()
            graphs[name] = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graphs[name]):
                issue()
            outs[name] = o
        same = all(torch.equal(outs["stored"][k], outs["labels"][k]) for k in outs["stored"])
        us = {"stored": [], "labels": []}
        for r in range(repeats + 1):  # the first round warms both up
            for name in ("stored", "labels"):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                graphs[name].replay()
                e1.record()
                e1.synchronize()
                if r:
                    us[name].append(1000.0 * e0.elapsed_time(e1) / launches)
        ms_, ml_ = statistics.median(us["stored"]), statistics.median(us["labels"])
        spread = max(max(v) - min(v) for v in us.values())
        rest = B * (2 * N * F * 2 + 2 * N * 16 + T * 4 + 4 + 4 + K * 8 + 8 + 3 * T * 8 + A * 4)  # everything but the adjacency
        out("(b) batch_gather B=%d N=%d F=%d A=%d T=%d bf16, %d images, %d launches replayed from one graph x %d repeats; last batches "
            "torch.equal: %s" % (B, N, F, A, T, n_img, launches, repeats, same))
        out("(b)   stored adjacency (%d bytes/launch, %d of them the adjacency read + written; the table holds %.1f MB): median %.2f us/launch "
            "(min %.2f, max %.2f)" % (rest + 2 * B * N * N * 4, 2 * B * N * N * 4, n_img * N * N * 4 / 1e6, ms_, min(us["stored"]), max(us["stored"])))
        out("(b)   made from labels (%d bytes/launch, %d of them ids read + adjacency written; the pair table holds %.2f MB): median %.2f us/launch "
            "(min %.2f, max %.2f)" % (rest + B * (2 * N * 4 + N * N * 4), B * (2 * N * 4 + N * N * 4), VC * VA * 4 / 1e6, ml_, min(us["labels"]),
                                      max(us["labels"])))
        out("(b)   labels - stored = %+.2f us/launch at the medians, the larger spread of either side's repeats is %.2f us: %s"
            % (ml_ - ms_, spread, "the label-fed gather is SLOWER beyond the spread (the trade is memory; it is opt-in)" if ml_ - ms_ > spread else
               "the label-fed gather is faster beyond the spread" if ms_ - ml_ > spread else "no difference beyond the spread"))
        del stored, labels, base, graphs, outs
        torch.cuda.empty_cache()


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "ingest", "label_adjacency_ab.txt"))
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--only", choices=["a", "b"], default=None)
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_label_adjacency: needs a GPU (nothing here is measured on a CPU)")
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)

    out("# python tools/bench_label_adjacency.py --repeats %d   (%s)" % (a.repeats, torch.cuda.get_device_name(0)))
    rate = copy_rate(dev)
    out("(0) device copy rate, 1 GiB, bytes read + written: %.2f TB/s" % rate)
    if a.only != "b":
        leg_builder(out, dev, a.repeats, rate)
    if a.only != "a":
        leg_gather(out, dev, a.repeats)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
