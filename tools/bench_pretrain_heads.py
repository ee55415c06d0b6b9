"""What the masked-LM head of pre-training costs from the decoder on: forward + backward, bf16, T = 20 tokens, V = 30522
word pieces, H = 768, 15 % of the rows labelled, at batch 32 and 256.
  python tools/bench_pretrain_heads.py [--out profiles/pretrain/mlm_head_ab.txt] [--rounds 3] [--iters 20] [--warmup 5]
Two variants on the same seeded rows, labels and word table, one fresh child process per batch size under its own time
limit; the first child that fails ends the run.
  (i)  baseline, composed only of what the library had before the compacted path: ``linear_fwd(out_f32=True)`` over all
       B T rows, ``softmax_loss_fwd`` / ``softmax_loss_bwd`` (CE, label_index, ignore -1), a cast of the fp32 gradient to
       bf16, ``linear_dgrad``, ``linear_wgrad`` and ``colsum``.
  (ii) the compacted path: ``mlm_select`` with mlm_capacity = ceil(0.25 B T), then ``pretrain_heads.mlm_decoder_fwd`` /
       ``mlm_decoder_bwd`` (bf16 logits [cap, 30528], in-place gradient) and ``mlm_scatter``.
A child warms both variants up, then times --iters calls of one variant between two device events, the variants
alternating i / ii for --rounds rounds; reported: each window's ms per call, each variant's median over its windows, the
spread between the windows of one variant, the ratio of the medians, and the peak bytes of logits either variant holds.
The two losses are printed too: same rows, same labels -- they agree to bf16 rounding of the logits."""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CHILD_LIMIT = 300  # seconds per child process
T, V, H, MASKED, CAP_SHARE = 20, 30522, 768, 0.15, 0.25


def child(B, rounds, iters, warmup):
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_pretrain_heads: no GPU -- nothing is measured without one")
    from xggm_amd import ops, pretrain_heads as PH
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    BF16, F32 = torch.bfloat16, torch.float32
    M = B * T
    rng = np.random.default_rng(1000 + B)
    labels = np.full(M, -1, dtype=np.int64)
    rows = np.sort(rng.choice(M, size=int(round(MASKED * M)), replace=False))
    labels[rows] = rng.integers(0, V, size=rows.size)
    labels = torch.from_numpy(labels).to(dev)
    x = torch.from_numpy(rng.standard_normal((M, H), dtype=np.float32)).to(dev).to(BF16)
    w = torch.from_numpy(rng.standard_normal((V, H), dtype=np.float32) * 0.02).to(dev).to(BF16)
    bias = torch.zeros(V, device=dev)
    g_table = torch.zeros((V, H), device=dev)
    g_bias = torch.zeros(V, device=dev)
    one = torch.ones((), device=dev)
    cap = int(math.ceil(CAP_SHARE * M))

    def baseline():
        z, _ = ops.linear_fwd(x, w, bias, out_f32=True)
        loss, pr = ops.softmax_loss_fwd(ops.SOFTMAX_CE, z, None, labels, ignore_index=-1)
        dz = ops.cast_from_f32(ops.softmax_loss_bwd(pr, one), BF16)
        d_x = ops.linear_dgrad(dz, w)
        ops.linear_wgrad(dz, x, g_table, False)
        ops.colsum(dz, g_bias)
        return loss, d_x

    def compacted():
        sel = ops.mlm_select(labels, x, cap, V)
        loss, st = PH.mlm_decoder_fwd(sel, sel.x, w, bias)
        d_t = PH.mlm_decoder_bwd(st, one, g_table, False, g_bias)
        return loss, ops.mlm_scatter(sel, d_t)

    variants = {"i": baseline, "ii": compacted}
    losses = {}
    for name, fn in variants.items():
        for _ in range(warmup):
            loss, _ = fn()
        torch.cuda.synchronize()
        losses[name] = float(loss)
    ms = {name: [] for name in variants}
    for _ in range(rounds):
        for name, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1) / iters)
    print("RESULT " + json.dumps({"B": B, "rows": M, "labelled": int(rows.size), "cap": cap, "ms": ms, "loss": losses,
                                  "logit_bytes": {"i": M * V * (4 + 4 + 2), "ii": cap * ops.vocab_ld(V, BF16) * 2}}),
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pretrain", "mlm_head_ab.txt"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, help="run one batch size in this process (a child)")
    args = ap.parse_args()
    if args.batch:
        return child(args.batch, args.rounds, args.iters, args.warmup)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        def say(msg):
            f.write(msg + "\n")
            f.flush()
            print(msg, flush=True)

        say("masked-LM head from the decoder on, forward + backward, bf16, T=%d V=%d H=%d, %.0f %% of the rows labelled"
            % (T, V, H, 100 * MASKED))
        say("(i) all rows: linear_fwd(out_f32) + softmax_loss CE + cast + dgrad + wgrad + colsum")
        say("(ii) compacted: mlm_select(cap = ceil(%.2f B T)) + decoder + vocab_ce + dgrad + wgrad + colsum + mlm_scatter" % CAP_SHARE)
        say("%d rounds i / ii alternating, %d calls per window between device events after %d warm-up calls; ms per call"
            % (args.rounds, args.iters, args.warmup))
        for B in (32, 256):
            p = subprocess.run(["timeout", "-k", "10", str(CHILD_LIMIT), sys.executable, os.path.abspath(__file__), "--batch",
                                str(B), "--rounds", str(args.rounds), "--iters", str(args.iters), "--warmup", str(args.warmup)],
                               capture_output=True, text=True, cwd=ROOT)
            res = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
            if p.returncode != 0 or not res:
                msg = "child for batch %d ended with status %d; nothing further was started\n%s" % (B, p.returncode, p.stderr[-2000:])
                f.write(msg)
                sys.exit(msg)
            r = json.loads(res[-1][len("RESULT "):])
            med = {k: statistics.median(v) for k, v in r["ms"].items()}
            say("batch %d: %d rows, %d labelled, cap %d" % (B, r["rows"], r["labelled"], r["cap"]))
            for k in ("i", "ii"):
                say("  (%-2s) %s   median %.4f   spread %.4f   loss %.6f   logits held: %.1f MB"
                    % (k, "  ".join("%.4f" % v for v in r["ms"][k]), med[k], max(r["ms"][k]) - min(r["ms"][k]), r["loss"][k],
                       r["logit_bytes"][k] / 1e6))
            say("  (i) / (ii) = %.2f x  -- (ii) is %s" % (med["i"] / med["ii"], "faster" if med["ii"] < med["i"] else "NOT faster"))


if __name__ == "__main__":
    main()
