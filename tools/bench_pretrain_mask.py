"""What making a pre-training batch costs: masked words, masked objects and the drawn QA answer for T = 20 tokens, 36 objects
of 2048 fp32 features, vocabulary 30522, up to 3 answer keys, at batch 32 and 256.
  python tools/bench_pretrain_mask.py [--out profiles/pretrain/mask_ab.txt] [--rounds 3] [--iters 20] [--warmup 5]
Three paths to the same five outputs (input_ids, masked_lm_labels, masked_feat, feat_mask, ans), one fresh child process per
batch size under its own time limit; the first child that fails ends the run.
  (a) the one launch: ``DeviceFeatures.__call__`` (xggm_pretrain_corrupt_f32, Philox draws) + ``ops.rng_advance``;
  (b) the same result composed from torch device ops: five ``torch.rand``, the decisions in float64 with ``torch.where``, a
      row gather for the replaced rows, a cumulative sum for the answer.  Fed the draws of (a) it returns the outputs of (a)
      bit for bit -- the child asserts that before it times anything;
  (c) the reference's way (src/pretrain/lxmert_pretrain.py:76-215, 258-296), restated: Python's ``random`` per token and per
      object, a copy of every example's features, ``np.stack`` and the upload of BOTH ``feat`` and ``masked_feat``.  Timed
      on the wall clock around a device synchronisation, --host-iters batches; the clean upload alone is printed beside it:
      that one remains in front of (a) and (b).
A child warms every path up, then times --iters calls of (a) or (b) between two device events, alternating a / b for --rounds
rounds: ms per call, medians, the spread between windows of one path, the ratio.
The launch against its byte floor: --launches calls of (a) are captured into one graph (no host launch cost inside the
window) and the replay is timed; the floor is a read plus a write of B O F elements minus the reads of the zeroed rows (their
count is taken from the output), at the bandwidth ``Tensor.copy_`` reaches on a buffer of the same size in the same child,
measured the same way.  fp32 and bf16 features."""
import argparse
import json
import os
import random
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CHILD_LIMIT = 300  # seconds per child process
T, O, F, V, K, MASK_ID, RATE = 20, 36, 2048, 30522, 3, 103, 0.15


def make_batch(B, np):
    r = np.random.default_rng(500 + B)
    ids, mask = np.zeros((B, T), dtype=np.int64), np.zeros((B, T), dtype=np.int64)
    for b in range(B):
        L = int(r.integers(5, T + 1))
        ids[b, 0], ids[b, L - 1], mask[b, :L] = 101, 102, 1
        ids[b, 1:L - 1] = r.integers(1000, V, size=L - 2)
    lab, sc = np.full((B, K), -1, dtype=np.int64), np.zeros((B, K), dtype=np.float32)
    for b in range(B):
        n = int(r.integers(0, K + 1))
        lab[b, :n] = r.choice(3000, size=n, replace=False)
        sc[b, :n] = r.random(n, dtype=np.float32) + np.float32(0.1)
    return dict(input_ids=ids, input_mask=mask, feats=r.random((B, O, F), dtype=np.float32),
                is_matched=r.integers(0, 2, size=B).astype(np.int64), label_ids=lab, label_scores=sc)


def torch_path(torch, b, draws=None):
    """(b): the kernel's contract in torch device ops"""
    ids, mask, feats = b["input_ids"], b["input_mask"], b["feats"]
    B, dev = ids.shape[0], ids.device
    if draws is None:
        draws = [torch.rand(n, device=dev) for n in (B * T, B * T, B * O, B * O, B)]
    u_w, u_wp, u_o, u_op, u_a = [d.double() for d in draws]
    elig = torch.zeros((B, T), dtype=torch.bool, device=dev)
    elig[:, 1:T - 1] = (mask[:, 1:T - 1] == 1) & (mask[:, 2:] == 1)
    p = u_w.view(B, T) / RATE
    lab = elig & (u_w.view(B, T) < RATE)
    pick = (u_wp.view(B, T) * V).long()
    out_ids = torch.where(lab & (p < 0.8), MASK_ID, torch.where(lab & (p >= 0.8) & (p < 0.9), pick, ids))
    labels = torch.where(lab, ids, -1)
    R = B * O
    m = u_o < RATE
    po = u_o / RATE
    rows = torch.where(m & (po >= 0.8) & (po < 0.9), (u_op * R).long(), torch.arange(R, device=dev))
    masked = torch.where((m & (po < 0.8)).unsqueeze(1), 0.0, feats.view(R, F)[rows]).view(B, O, F)
    feat_mask = m.float().view(B, O)
    valid = b["label_ids"] >= 0
    s = torch.where(valid, b["label_scores"].double(), 0.0)
    cols = [s[:, 0]]
    for j in range(1, K):  # left to right, as the kernel adds (a parallel scan may associate differently)
        cols.append(cols[-1] + s[:, j])
    cum = torch.stack(cols, 1)
    n = valid.sum(1)
    k = torch.minimum(((u_a * cum[:, -1]).unsqueeze(1) >= cum).sum(1), (n - 1).clamp(min=0))
    ans = torch.where((n > 0) & (b["is_matched"] == 1), b["label_ids"].gather(1, k.unsqueeze(1)).squeeze(1), -1)
    return dict(input_ids=out_ids, masked_lm_labels=labels, masked_feat=masked, feat_mask=feat_mask, ans=ans)


def host_path(torch, np, nb, dev):
    """(c): per example on the host, then the upload of feat and masked_feat"""
    B = nb["input_ids"].shape[0]
    all_ids, all_lab, all_mf, all_fm, all_ans = [], [], [], [], []
    for b in range(B):
        ids, lab = nb["input_ids"][b].tolist(), [-1] * T
        L = int(nb["input_mask"][b].sum())
        for t in range(1, L - 1):
            prob = random.random()
            if prob < RATE:
                prob /= RATE
                lab[t] = ids[t]
                if prob < 0.8:
                    ids[t] = MASK_ID
                elif prob < 0.9:
                    ids[t] = int(random.random() * V)
        feats = nb["feats"][b]
        mf, fm = feats.copy(), np.zeros(O, dtype=np.float32)
        for o in range(O):
            prob = random.random()
            if prob < RATE:
                prob /= RATE
                if prob < 0.8:
                    mf[o, :] = 0.
                elif prob < 0.9:
                    mf[o, :] = nb["feats"][int(random.random() * B), int(random.random() * O)]
                fm[o] = 1.
        keys = [(int(k), float(s)) for k, s in zip(nb["label_ids"][b], nb["label_scores"][b]) if k >= 0]
        ans = -1
        if keys and nb["is_matched"][b] == 1:
            ans = keys[0][0] if len(keys) == 1 else keys[int(np.random.multinomial(1, [s / sum(v for _, v in keys) for _, s in keys]).argmax())][0]
        all_ids.append(ids), all_lab.append(lab), all_mf.append(mf), all_fm.append(fm), all_ans.append(ans)
    out = dict(input_ids=torch.tensor(all_ids, dtype=torch.long).to(dev), masked_lm_labels=torch.tensor(all_lab, dtype=torch.long).to(dev),
               masked_feat=torch.from_numpy(np.stack(all_mf)).to(dev), feats=torch.from_numpy(np.stack(list(nb["feats"]))).to(dev),
               feat_mask=torch.from_numpy(np.stack(all_fm)).to(dev), ans=torch.tensor(all_ans, dtype=torch.long).to(dev))
    torch.cuda.synchronize()
    return out


def child(B, rounds, iters, warmup, launches, replays, host_iters):
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_pretrain_mask: no GPU -- nothing is measured without one")
    from xggm_amd import ops
    from xggm_amd.pretrain.lxmert_pretrain import DeviceFeatures, SID_BASE
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    nb = make_batch(B, np)
    b = {k: torch.from_numpy(v).to(dev) for k, v in nb.items()}
    seg = torch.zeros_like(b["input_ids"])
    none = [None] * 5
    rng = ops.make_rng(9, dev)
    feat = DeviceFeatures(RATE, RATE, V, MASK_ID, max_labels=K)

    def path_a(bb=b):
        a = feat(bb["input_ids"], bb["input_mask"], seg, bb["feats"], *none, bb["is_matched"], bb["label_ids"], bb["label_scores"], rng)
        ops.rng_advance(rng)
        return dict(input_ids=a[0], masked_lm_labels=a[3], masked_feat=a[4], feat_mask=a[6]["feat"][1], ans=a[8])

    # (b) is the same function: fed the draws of (a) it gives the outputs of (a)
    draws = [ops.uniform(n, rng, SID_BASE + i) for i, n in enumerate((B * T, B * T, B * O, B * O, B))]
    want = {k: v.clone() for k, v in path_a().items()}
    got = torch_path(torch, b, draws)
    torch.cuda.synchronize()
    for k in want:
        assert torch.equal(got[k], want[k]), "torch composition differs from the launch in " + k

    def window(fn, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / n

    work = {"a": path_a, "b": lambda: torch_path(torch, b)}
    for fn in work.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    res = {"a": [], "b": []}
    for _ in range(rounds):
        for name in ("a", "b"):
            res[name].append(window(work[name], iters))
    # (c) and the upload that stays
    host_path(torch, np, nb, dev)
    host = []
    for _ in range(host_iters):
        t0 = time.perf_counter()
        host_path(torch, np, nb, dev)
        host.append((time.perf_counter() - t0) * 1e3)
    up = []
    for _ in range(host_iters):
        t0 = time.perf_counter()
        torch.from_numpy(np.stack(list(nb["feats"]))).to(dev)
        torch.cuda.synchronize()
        up.append((time.perf_counter() - t0) * 1e3)

    # the launch against its byte floor, by graph replay
    def replayed(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(launches):
                fn()
        g.replay()
        torch.cuda.synchronize()
        ts = []
        for _ in range(replays):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            g.replay()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1) / launches * 1e3)
        return statistics.median(ts)

    floor = {}
    for name, dt in (("f32", torch.float32), ("bf16", torch.bfloat16)):
        bb = dict(b, feats=b["feats"].to(dt))
        call = lambda: feat(bb["input_ids"], bb["input_mask"], seg, bb["feats"], *none, bb["is_matched"], bb["label_ids"],
                            bb["label_scores"], rng)  # noqa: E731  (rng is not advanced: every replay moves the same rows)
        src, dst = bb["feats"], torch.empty_like(bb["feats"])
        nbytes = src.numel() * src.element_size()
        t_copy = replayed(lambda: dst.copy_(src))
        t_kernel = replayed(call)
        o = call()
        torch.cuda.synchronize()
        zero = int(((o[6]["feat"][1] == 1) & (o[4] == 0).all(-1)).sum())
        bw = 2 * nbytes / (t_copy * 1e-6)
        need = nbytes * (2 - zero / (B * O))
        floor[name] = dict(us=t_kernel, copy_us=t_copy, copy_tbs=bw / 1e12, bytes=need, floor_us=need / bw * 1e6, zero_rows=zero)
    print(json.dumps(dict(B=B, a=res["a"], b=res["b"], host=host, upload=up, floor=floor)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pretrain", "mask_ab.txt"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--replays", type=int, default=7)
    ap.add_argument("--host-iters", type=int, default=3)
    ap.add_argument("--child", type=int, default=0)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.rounds, a.iters, a.warmup, a.launches, a.replays, a.host_iters)
    lines = ["pre-training batch masking: T=%d, %d objects x %d fp32 features, V=%d, K=%d, rates %.2f" % (T, O, F, V, K, RATE),
             "(a) one launch (DeviceFeatures + rng_advance)   (b) torch device ops, same outputs bit for bit on the same draws",
             "(c) per example on the host + upload of feat and masked_feat (wall clock)",
             "%d rounds a / b alternating, %d calls per window between device events after %d warm-up calls; ms per call"
             % (a.rounds, a.iters, a.warmup)]
    for B in (32, 256):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", str(B)]
        for k in ("rounds", "iters", "warmup", "launches", "replays"):
            cmd += ["--" + k, str(getattr(a, k))]
        cmd += ["--host-iters", str(a.host_iters)]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=CHILD_LIMIT)
        if p.returncode != 0:
            sys.stderr.write(p.stdout + p.stderr)
            sys.exit("bench_pretrain_mask: the child for batch %d failed (%d); nothing after it is started" % (B, p.returncode))
        r = json.loads(p.stdout.strip().splitlines()[-1])
        med = {k: statistics.median(r[k]) for k in ("a", "b", "host", "upload")}
        lines.append("batch %d: %d rows of %d bytes" % (B, B * O, F * 4))
        for k in ("a", "b"):
            lines.append("  (%s) %s   median %.4f   spread %.4f" % (k, "  ".join("%.4f" % v for v in r[k]), med[k], max(r[k]) - min(r[k])))
        lines.append("  (b) / (a) = %.2f x  -- (a) is %s" % (med["b"] / med["a"], "faster" if med["a"] < med["b"] else "NOT faster"))
        lines.append("  (c) %s   median %.2f ms;  the clean upload alone %.2f ms;  (c) / (upload + a) = %.1f x"
                     % ("  ".join("%.2f" % v for v in r["host"]), med["host"], med["upload"], med["host"] / (med["upload"] + med["a"])))
        for name, f in r["floor"].items():
            lines.append("  launch, %s features, graph replay: %.2f us;  copy_ of the same buffer %.2f us = %.2f TB/s;  floor for %.1f MB "
                         "(%d zeroed rows not read) %.2f us;  launch / floor = %.2f"
                         % (name, f["us"], f["copy_us"], f["copy_tbs"], f["bytes"] / 1e6, f["zero_rows"], f["floor_us"], f["us"] / f["floor_us"]))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)
    sys.stdout.write(text)


if __name__ == "__main__":
    main()
