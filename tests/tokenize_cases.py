"""Shared cases of the tokeniser tests (tests/test_tokenize_cpu.py, tests/test_tokenize_gpu.py): a seeded synthetic
vocabulary with multi-byte pieces, a seeded corpus that holds every edge the kernel has a branch for, and the host rows
they are compared with -- computed once per (corpus, T) and shared."""
import os
import random

import numpy as np

from xggm_amd.lxrt.tokenization import BertTokenizer

SEED = 20240611
T_MAIN = 20
SPECIALS = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"]
MOJIBAKE = ["caf\u00c3\u00a9", "\u00e4\u00ba\u00ba\u00e5\u00b1\u00b1"]  # the fixture's (tests/golden/tokenizer.json)
# letters no piece of the vocabulary holds: a word with one of them has an unmatched remainder
NO_PIECE = "qxz"
_LETTERS = "abcdefghijklmnoprstuvwy"
_cache = {}


def synth_vocab_tokens(n=2000, seed=SEED):
    """about ``n`` distinct tokens: specials, punctuation, every letter but NO_PIECE alone and as a continuation, seeded
    syllable words and suffixes, and multi-byte pieces (Greek, Cyrillic, CJK, a Deseret letter and an emoji: 4-byte UTF-8)"""
    rng = random.Random(seed)
    toks = list(SPECIALS) + list("!\"#$%&'()*+,-./:;<=>?@[\\]^_`{|}~") + list("0123456789")
    toks += list(_LETTERS) + ["##" + c for c in _LETTERS] + ["the", "cafe", "##ing", "##ed", "##s", "colour", "don", "t"]
    toks += ["\u4eba", "\u5c71", "\u8c48", "\u03b1\u03b2\u03b3", "##\u03b3\u03b1", "\u03c3", "\u03c2", "##\u03c3", "##\u03c2",
             "\u043f\u0440\u0438", "##\u0432\u0435\u0442", "\u00e6", "##\u00e6", "\u00df", "\U00010428", "##\U00010428",
             "\U0001f600", "##\U0001f600", "\u1100", "##\u1161", "##\u11a8", "\u3042", "##\u3044", "\u00c3", "##\u00a9", "\u302e"]
    seen = set(toks)
    syl = ["ba", "de", "fi", "go", "hu", "ka", "le", "mi", "no", "pu", "ra", "se", "ti", "vo", "wy", "an", "er", "ist", "on", "al"]
    while len(toks) < n:
        w = "".join(rng.choice(syl) for _ in range(rng.randint(1, 4)))
        if rng.random() < 0.4:
            w = "##" + w
        if w not in seen:
            seen.add(w)
            toks.append(w)
    return toks


def synth_tokenizer(tmp_dir, n=2000, seed=SEED):
    key = ("tok", n, seed)
    if key not in _cache:
        path = os.path.join(str(tmp_dir), "vocab_synth_%d_%d.txt" % (n, seed))
        with open(path, "w", encoding="utf-8") as f:
            f.write("\n".join(synth_vocab_tokens(n, seed)) + "\n")
        _cache[key] = BertTokenizer(path)
    return _cache[key]


def edge_sentences(T=T_MAIN):
    """the named edges, in a fixed order; none of them holds a HOST code point"""
    L = T - 2
    s = ["", "     ", " \t\n\r ", "  the ba  ", "\tthe\n", "\u00a0the\u3000ba\u2003",
         "a" * 100, "a" * 101, "a\u0301" * 100, "a\u0301" * 101, "the " + "b" * 100 + " the", "the " + "b" * 101 + " the",
         "theq", "bade" + NO_PIECE[1], "the theq the", "q", "aqa b",
         " ".join(["the"] * L), " ".join(["the"] * (L + 1)), " ".join(["the"] * (L - 1)), " ".join(["the"] * 60),
         " ".join(["the"] * (L - 1)) + " thes", " ".join(["the"] * (L - 1)) + " theq the", " ".join(["the"] * (L - 1)) + " " + "a" * 50]
    for t in SPECIALS:
        s += [t, "the %s ba" % t, t[:3] + "\u200b" + t[3:], "the " + t[:2] + "\u00ad" + t[2:] + ".", t.lower(), t + ".", "a" + t,
              t + t, t + "\u4eba", "\u4eba" + t, "\u0301" + t, t[:-1]]
    s += ["\u4eba\u5c71 the", "the\u4eba", "\u4eba", "\uf900 \U0002f800", "caf\u00e9 cafe\u0301 CAF\u00c9", "colour\u0301 of",
          "\u00c5ngstr\u00f6m \u00e6 \u00c6\u00c6 \u00df", MOJIBAKE[0] + " zzz", MOJIBAKE[1] + " what", "\U00010400\U00010428 \U0001f600\U0001f600 the",
          "\U0001f600", "a\U0001f600b", "don't fly", "'''", "the's ba's", "?!?!...", "the,ba;de--fi", "(the)[ba]{de}", "$1,000.50",
          "the\u2028ba\u2029de", "\u2028", "the\u0085ba\u001cde\u000bfi", "\u0130stanbul \u0131", "\u03b1\u03b2\u03b3\u03b3\u03b1 \u0391\u0392\u0393",
          "\u03c3\u03c3 \u03c2", "\u041f\u0420\u0418\u0412\u0415\u0422 \u043f\u0440\u0438", "\uac01 \ud55c", "\u3042\u3044 \u30a2", "\ufffd the\x00ba",
          "\u0301\u0301", "the \u0301 ba", "a\u20dd", "\u1e9e \ufb01", "e\u0301\u0323"]
    return s


def synth_corpus(n=4000, T=T_MAIN, seed=SEED):
    """``n`` seeded sentences, the edges of ``edge_sentences`` first; none of them holds a HOST code point"""
    key = ("corpus", n, T, seed)
    if key in _cache:
        return _cache[key]
    rng = random.Random(seed + 1)
    vocab = synth_vocab_tokens(2000, seed)
    words = [t for t in vocab if not t.startswith("##") and t not in SPECIALS and len(t) > 1] + list(_LETTERS)
    tails = [t[2:] for t in vocab if t.startswith("##")]
    extra = ["\u0301", "\u00e9", "\u4eba", "\U0001f600", "'", ".", "?!", "--", "q", "\u200b", "\u00a0", "\u2028", " ", "\t", MOJIBAKE[0],
             "\u00c4", "\U00010400", "\uac01", "[MASK]", "[UNK]"]
    sents = edge_sentences(T)[:n]
    while len(sents) < n:
        out = []
        for _ in range(rng.randint(1, 14)):
            w = rng.choice(words)
            for _ in range(rng.choice((0, 0, 0, 1, 1, 2, 3))):
                w += rng.choice(tails)
            r = rng.random()
            if r < 0.15 and "\u03a3" not in w.upper():
                w = w.upper()
            elif r < 0.25:
                w = w.capitalize()
            elif r < 0.45:
                i = rng.randint(0, len(w))
                w = w[:i] + rng.choice(extra) + w[i:]
            out.append(w)
        sents.append(rng.choice(("", " ", "  ")) + rng.choice((" ", " ", "  ", "\t")).join(out) + rng.choice(("", "", " ", "?", ".")))
    _cache[key] = sents
    return sents


def host_rows(tok, sents, T):
    """the wrapped host tokenizer's rows -> (ids int64 [n, T] zero padded, len int64 [n]); computed once per corpus and T"""
    key = ("rows", id(tok), id(sents), T)
    if key not in _cache:
        ids, lens = np.zeros((len(sents), T), dtype=np.int64), np.zeros(len(sents), dtype=np.int64)
        for i, s in enumerate(sents):
            w = tok.convert_tokens_to_ids(["[CLS]"] + tok.tokenize(s.strip())[:T - 2] + ["[SEP]"])
            ids[i, :len(w)], lens[i] = w, len(w)
        _cache[key] = (ids, lens, sents)  # the corpus is kept alive: its id() is the key
    return _cache[key][:2]
