"""What tokenising on the device costs and saves (xggm_amd.lxrt.tokenization.DeviceTokenizer), one process, same box:

  (0) a seeded synthetic vocabulary (28 000 entries: letters, syllable words, "##" continuations) and a seeded corpus of
      ``--sents`` sentences of 5-14 words (vocabulary words, words with continuations, capitals, accents, punctuation,
      a few words no piece matches); the device and the host must agree on ``--check`` of them, row for row, before
      anything is timed, with no row handed to the host;
  (a) the host loop -- ``tokenize(sent.strip())[:T - 2]`` + ``convert_tokens_to_ids`` per sentence, what
      ``pretrain_tables`` / ``sample_tables`` do -- on the first ``--host-sents`` sentences (the loop is linear in the
      number of sentences; the full corpus takes minutes) against ``DeviceTokenizer.encode`` end to end on the WHOLE
      corpus: pack, one host-to-device copy, one launch, read-back of the flagged count and of ids / len.  Legs
      alternate, ``--repeats`` times, host clock, the device leg ends in the read-back;
  (b) the parts of the device leg: packing alone (host clock) and the kernel alone (device events around the launch).

    python tools/bench_tokenize.py [--out profiles/tokenize/tokenize_ab.txt] [--sents 1000000] [--repeats 3]
"""
import argparse
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SYL = ["ba", "de", "fi", "go", "hu", "ka", "le", "mi", "no", "pu", "ra", "se", "ti", "vo", "wy", "an", "er", "ist", "on", "al",
       "chi", "sto", "ple", "gra", "the", "ing", "ous", "ment", "co", "un"]


def make_vocab(n, rng):
    letters = "abcdefghijklmnoprstuvwy"  # q, x, z: in no piece, a word with one of them is [UNK]
    toks = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"] + list("!\"#$%&'()*+,-./:;<=>?@[\\]^_`{|}~0123456789")
    toks += list(letters) + ["##" + c for c in letters]
    seen = set(toks)
    while len(toks) < n:
        w = "".join(SYL[i] for i in rng.integers(0, len(SYL), rng.integers(1, 5)))
        if rng.random() < 0.35:
            w = "##" + w
        if w not in seen:
            seen.add(w)
            toks.append(w)
    return toks


def make_corpus(n, vocab, rng):
    words = np.array([t for t in vocab if t.isalpha() and len(t) > 1])
    tails = np.array([t[2:] for t in vocab if t.startswith("##") and len(t) > 3])
    n_words = rng.integers(5, 15, n)
    total = int(n_words.sum())
    w = words[rng.integers(0, len(words), total)].tolist()
    kind = rng.random(total)
    t = tails[rng.integers(0, len(tails), total)].tolist()
    for i in np.nonzero(kind < 0.30)[0]:
        w[i] += t[i]                                   # a word of two or more pieces
    for i in np.nonzero((kind >= 0.30) & (kind < 0.38))[0]:
        w[i] = w[i].capitalize()
    for i in np.nonzero((kind >= 0.38) & (kind < 0.41))[0]:
        w[i] = w[i][:1] + "\u0301" + w[i][1:]           # a combining accent
    for i in np.nonzero((kind >= 0.41) & (kind < 0.44))[0]:
        w[i] += "'s"
    for i in np.nonzero((kind >= 0.44) & (kind < 0.45))[0]:
        w[i] += "q"                                    # no piece matches: [UNK]
    ends = np.cumsum(n_words).tolist()
    tail = ["", "", "?", ".", " "]
    pick = rng.integers(0, len(tail), n).tolist()
    return [" ".join(w[a:b]) + tail[p] for a, b, p in zip([0] + ends[:-1], ends, pick)]


def host_loop(tok, sents, T):
    out = []
    for s in sents:
        out.append(tok.convert_tokens_to_ids(["[CLS]"] + tok.tokenize(s.strip())[:T - 2] + ["[SEP]"]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tokenize", "tokenize_ab.txt"))
    ap.add_argument("--sents", type=int, default=1000000)
    ap.add_argument("--host-sents", type=int, default=200000)
    ap.add_argument("--check", type=int, default=20000)
    ap.add_argument("--vocab", type=int, default=28000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("-T", type=int, default=20)
    a = ap.parse_args()
    from xggm_amd import ops
    from xggm_amd.lxrt.tokenization import BertTokenizer, DeviceTokenizer, pack_sentences
    dev, T = "cuda:0", a.T
    rng = np.random.default_rng(20240611)
    vocab = make_vocab(a.vocab, rng)
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "vocab.txt")
        with open(path, "w", encoding="utf-8") as f:
            f.write("\n".join(vocab) + "\n")
        tok = BertTokenizer(path)
    t0 = time.perf_counter()
    dt = DeviceTokenizer(tok, dev)
    t_tables = time.perf_counter() - t0
    sents = make_corpus(a.sents, vocab, rng)
    n_host = min(a.host_sents, a.sents)
    lines = ["# python tools/bench_tokenize.py --sents %d --host-sents %d --repeats %d   (%s)"
             % (a.sents, n_host, a.repeats, torch.cuda.get_device_name(0)),
             "(0) vocabulary %d entries, corpus %d sentences, T=%d; tables built and uploaded once in %.2f s"
             % (len(tok.vocab), len(sents), T, t_tables)]

    # (0) agreement first
    n_chk = min(a.check, a.sents)
    ids, lens = (t.cpu() for t in dt.encode(sents[:n_chk], T))
    want = host_loop(tok, sents[:n_chk], T)
    bad = sum(1 for i, w in enumerate(want) if ids[i, :lens[i]].tolist() != w or bool(ids[i, lens[i]:].any()))
    assert bad == 0 and dt.last_host_rows == 0, "%d of %d rows differ from the host, %d rows went to the host" % (bad, n_chk, dt.last_host_rows)
    mean_tok = float(lens.float().mean())
    lines.append("(0) device rows == host rows on the first %d sentences, 0 rows handed to the host; %.1f tokens per row with [CLS] / [SEP]"
                 % (n_chk, mean_tok))

    # (a) alternating legs
    host_s, dev_s = [], []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        host_loop(tok, sents[:n_host], T)
        host_s.append((time.perf_counter() - t0) / n_host * 1e6)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ids, lens = dt.encode(sents, T)
        ids_h, lens_h = ids.cpu(), lens.cpu()  # the read-back pretrain_tables / sample_tables make
        dev_s.append((time.perf_counter() - t0) / len(sents) * 1e6)
    hm, dm = statistics.median(host_s), statistics.median(dev_s)
    lines.append("(a) host loop, %d sentences:                          median %.2f us/sentence (min %.2f, max %.2f; %d repeats) -> %.1f s per 1 M"
                 % (n_host, hm, min(host_s), max(host_s), a.repeats, hm))
    lines.append("(a) device path end to end (pack, copy, launch, read-back), %d sentences: median %.3f us/sentence (min %.3f, max %.3f) -> %.2f s per 1 M"
                 % (len(sents), dm, min(dev_s), max(dev_s), dm))
    lines.append("(a) host / device = %.0fx at the medians%s" % (hm / dm, "" if dm < hm else "  -- the device path is NOT faster"))

    # (b) the parts
    pack_s = []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        data, off, _ = pack_sentences(sents)
        pack_s.append(time.perf_counter() - t0)
    d_dev, off_dev = torch.from_numpy(data.copy()).to(dev), torch.from_numpy(off).to(dev)
    out = ops.tokenize_wordpiece(d_dev, off_dev, off, T, dt.tables)
    kern = []
    for _ in range(max(a.repeats, 5)):
        out["flagged"].zero_()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ops.tokenize_wordpiece(d_dev, off_dev, off, T, dt.tables, out=out)
        e1.record()
        e1.synchronize()
        kern.append(e0.elapsed_time(e1))
    km = statistics.median(kern)
    lines.append("(b) packing alone (join, encode, offsets), host clock: median %.3f s (min %.3f, max %.3f) for %d sentences, %d bytes"
                 % (statistics.median(pack_s), min(pack_s), max(pack_s), len(sents), len(data)))
    lines.append("(b) kernel alone, device events: median %.3f ms (min %.3f, max %.3f; %d launches) -> %.1f M sentences/s, %.2f GB/s of UTF-8 read"
                 % (km, min(kern), max(kern), len(kern), len(sents) / km / 1e3, len(data) / km / 1e6))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
