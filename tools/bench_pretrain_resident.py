"""What feeding the captured LXMERT pre-training step costs, from the host against a device-resident corpus
(``pretrain.resident.ResidentPretrainSet``): full LXMERT 9/5/5 (``LXRTPretraining``, all six tasks, 9500 answers), bf16, T = 20,
36 objects of 2048 features, swap rate 0.5, at batch 32 and 256.
  python tools/bench_pretrain_resident.py [--out profiles/pretrain/resident_ab.txt] [--rounds 3] [--iters 30] [--warmup 3]
One fresh child process per batch size under its own time limit; the first child that fails ends the run.  In a child, one
model and a synthetic corpus of --images images and --samples sentences (WordPiece over a synthetic vocabulary), and three
legs alternating A / B / C for --rounds rounds, --iters steps per window between two device events (the window ends in an
event synchronise, so leg A includes the time the device waits for the host):
  (A) the host path: ``collate_examples`` of B examples, thirteen ``.to(device)`` copies, ``step(batch)`` -- ``load_batch`` into
      the static inputs and one graph replay with the swap inside it;
  (B) ``load_resident(store, start)`` -- one gather launch with the swap fused in -- and one graph replay;
  (C) the graph replay of (B) alone, on the batch the static inputs hold.
Then the gather launch alone: --iters ``store.fill`` calls into the static inputs between two events.
Reported: each window's ms per step, each leg's median, the spread between the windows of one leg, and the differences of the
medians.  No threshold is asserted anywhere: this file is where the numbers come from."""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CHILD_LIMIT = 540  # seconds per child process
T, O, F, N_ANS, K, N_WORDS = 20, 36, 2048, 9500, 4, 2000


def corpus(n_img, n_q, tmp):
    import numpy as np
    from xggm_amd.lxrt.tokenization import BertTokenizer
    from xggm_amd.pretrain.lxmert_pretrain import InputExample
    words = ["w%d" % i for i in range(N_WORDS)]
    path = os.path.join(tmp, "vocab.txt")
    with open(path, "w") as f:
        f.write("\n".join(["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"] + words) + "\n")
    tok = BertTokenizer(path, do_lower_case=True)
    rng = np.random.default_rng(0)
    imgs = [(rng.standard_normal((O, F), dtype=np.float32), rng.random((O, 4), dtype=np.float32),
             (rng.integers(0, 1600, O), rng.random(O, dtype=np.float32)), (rng.integers(0, 400, O), rng.random(O, dtype=np.float32)))
            for _ in range(n_img)]
    ex = []
    for q in range(n_q):
        i = int(rng.integers(0, n_img))
        sent = " ".join(words[j] for j in rng.integers(0, N_WORDS, int(rng.integers(4, 15))))
        ex.append(InputExample("img%d_vqa_%06d" % (i, q), sent, imgs[i][:2], imgs[i][2], imgs[i][3], 1, {int(rng.integers(0, N_ANS)): 1.0}))
    return ex, tok


def child(B, rounds, iters, warmup, n_img, n_q):
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_pretrain_resident: no GPU -- nothing is measured without one")
    from xggm_amd.engine import CapturedPretrainer
    from xggm_amd.lxrt import modeling as M
    from xggm_amd.lxrt.optimization import BertAdam
    from xggm_amd.pretrain.lxmert_pretrain import DeviceFeatures, collate_examples
    from xggm_amd.pretrain.resident import ResidentPretrainSet
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    with tempfile.TemporaryDirectory() as tmp:
        ex, tok = corpus(n_img, n_q, tmp)
    vocab = len(tok.vocab)
    vc = M.VISUAL_CONFIG
    vc.l_layers, vc.x_layers, vc.r_layers = 9, 5, 5  # the pre-training configuration (--llayers 9 --xlayers 5 --rlayers 5)
    model = M.LXRTPretraining(M.BertConfig(vocab), visual_losses="obj,attr,feat", task_qa=True, num_answers=N_ANS,
                              mlm_capacity=int(math.ceil(0.25 * B * T)), compute_dtype=torch.bfloat16).to(dev).train()
    optim = BertAdam(list(model.parameters()), lr=1e-4, warmup=0.05, t_total=100000)
    store = ResidentPretrainSet(ex, dev, tokenizer=tok, max_seq_length=T, max_labels=K, n_answers=N_ANS, feats_bf16=True,
                                match_rate=0.5, batch_size=B)
    order = store.order(0, seed=1, batch_size=B)
    steps = len(order) // B
    feats = lambda rate: DeviceFeatures(vocab_size=vocab, mask_id=tok.vocab["[MASK]"], max_labels=K, match_rate=rate)
    host_batch = lambda k: {n: v.to(dev, non_blocking=True) for n, v in
                            collate_examples([ex[int(s)] for s in order[k % steps * B:(k % steps + 1) * B]], tok, T, K).items()}
    tr_a = CapturedPretrainer(model, optim, host_batch(0), feats(0.5), warmup_iters=2)
    tr_b = CapturedPretrainer(model, optim, store.fill(store.buffers(B), 0, B, swap=False), feats(None), warmup_iters=2, resident=store)
    legs = {"A": lambda k: tr_a.step(host_batch(k)),
            "B": lambda k: (tr_b.load_resident(store, k % steps * B), tr_b.step())[1],
            "C": lambda k: tr_b.step()}
    losses, k = {}, 0
    for name, leg in legs.items():
        for _ in range(warmup):
            out = leg(k)
            k += 1
        torch.cuda.synchronize()
        losses[name] = float(out[0])

    def window(fn):
        nonlocal k
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn(k)
            k += 1
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / iters

    ms = {name: [] for name in legs}
    gather = []
    for _ in range(rounds):
        for name, leg in legs.items():
            ms[name].append(window(leg))
        gather.append(window(lambda k: tr_b.load_resident(store, k % steps * B)) * 1000.0)
    print("RESULT " + json.dumps({"B": B, "ms": ms, "gather_us": gather, "loss": losses, "images": store.n_img, "samples": len(store),
                                  "store_bytes": store.nbytes, "exhausted": int(store.swap_exhausted)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pretrain", "resident_ab.txt"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--images", type=int, default=1024)
    ap.add_argument("--samples", type=int, default=8192)
    ap.add_argument("--batch", type=int, help="run one batch size in this process (a child)")
    args = ap.parse_args()
    if args.batch:
        return child(args.batch, args.rounds, args.iters, args.warmup, args.images, args.samples)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        def say(msg):
            f.write(msg + "\n")
            f.flush()
            print(msg, flush=True)

        say("feeding the captured LXMERT pre-training step: LXRTPretraining 9/5/5, bf16, T=%d, %d x %d features, %d answers, swap "
            "rate 0.5; corpus of %d images / %d sentences" % (T, O, F, N_ANS, args.images, args.samples))
        say("(A) host: collate_examples + 13 copies + load_batch + replay (swap in the graph, fp32 features over PCIe)")
        say("(B) resident: load_resident (one gather launch, swap fused, bf16 table) + replay   (C) the replay of (B) alone")
        say("%d rounds A / B / C alternating, %d steps per window between device events after %d warm-up steps; ms per step"
            % (args.rounds, args.iters, args.warmup))
        for B in (32, 256):
            p = subprocess.run(["timeout", "-k", "10", str(CHILD_LIMIT), sys.executable, os.path.abspath(__file__), "--batch",
                                str(B), "--rounds", str(args.rounds), "--iters", str(args.iters), "--warmup", str(args.warmup),
                                "--images", str(args.images), "--samples", str(args.samples)], capture_output=True, text=True, cwd=ROOT)
            res = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
            if p.returncode != 0 or not res:
                msg = "child for batch %d ended with status %d; nothing further was started\n%s" % (B, p.returncode, p.stderr[-2000:])
                f.write(msg)
                sys.exit(msg)
            r = json.loads(res[-1][len("RESULT "):])
            med = {k: statistics.median(v) for k, v in r["ms"].items()}
            say("batch %d (store: %d images, %d sentences, %.1f MB on the device; %d rows exhausted their swap candidates)"
                % (B, r["images"], r["samples"], r["store_bytes"] / 1e6, r["exhausted"]))
            for k in ("A", "B", "C"):
                say("  (%s) %s   median %.3f   spread %.3f   last warm-up loss %.4f"
                    % (k, "  ".join("%.3f" % v for v in r["ms"][k]), med[k], max(r["ms"][k]) - min(r["ms"][k]), r["loss"][k]))
            g = r["gather_us"]
            say("  gather launch alone, us per call: %s   median %.1f   spread %.1f"
                % ("  ".join("%.1f" % v for v in g), statistics.median(g), max(g) - min(g)))
            say("  B - C = %.3f ms;  A - B = %.3f ms;  A / B = %.2f x -- the resident feed is %s the host feed"
                % (med["B"] - med["C"], med["A"] - med["B"], med["A"] / med["B"], "below" if med["B"] < med["A"] else "NOT below"))


if __name__ == "__main__":
    main()
