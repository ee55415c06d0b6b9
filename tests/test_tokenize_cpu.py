"""CPU-only checks of the device tokenizer: the boundary (symbols, refusals before any launch, no CPU fallback), the kernel's
algorithm restated in Python from the SAME tables (``lxrt.tokenization.Restatement``: table lookups, rolling hash, probing)
against the host tokenizer -- every code point, seeded pairs, the reference's golden rows --, the HOST set, and the hash
tables.  No kernel runs here."""
import ctypes
import json
import os
import random
import unicodedata

import numpy as np
import pytest
import torch

from helpers import GOLDEN
from xggm_amd import _lib, ops
from xggm_amd.lxrt import tokenization as tk
import tokenize_cases as C

NOT_SURROGATE = [cp for cp in range(0x110000) if not 0xD800 <= cp <= 0xDFFF]


@pytest.fixture(scope="module")
def synth(tmp_path_factory):
    tok = C.synth_tokenizer(tmp_path_factory.mktemp("vocab"))
    tables = tk.host_tables(tok)
    return tok, tables, tk.Restatement(tables)


def host_ids(tok, s, T):
    return tok.convert_tokens_to_ids(["[CLS]"] + tok.tokenize(s.strip())[:T - 2] + ["[SEP]"])


# ----------------------------------------------------------------------------- boundary
def test_symbols_are_declared_exported_and_built():
    decl = _lib.parse_header()
    assert decl["xggm_tokenize_wordpiece"] == [ctypes.c_void_p, ctypes.c_void_p]
    assert decl["xggm_tokenize_workspace_bytes"] == [ctypes.c_int64, ctypes.c_int]
    assert hasattr(_lib.lib, "xggm_tokenize_wordpiece") and hasattr(_lib.lib, "xggm_tokenize_workspace_bytes")
    assert _lib.lib.xggm_tokenize_workspace_bytes(1000000, 20) == 0  # the word in flight lives in LDS
    src = open(_lib.HEADER_PATH).read()
    doc = src[src.index("/* xggm_tokenize_wordpiece:"):src.index("#define XGGM_TOKENIZE_MAX_WORD")]
    for cite in ("src/lxrt/tokenization.py:72-348", "src/lxrt/entry.py:37-72", "src/pretrain/lxmert_pretrain.py:149"):
        assert cite in doc, cite
    assert "#define XGGM_TOKENIZE_HASH_MUL 0x%Xull" % tk.HASH_MUL in src and "#define XGGM_TOKENIZE_HASH_MUL_INV 0x%Xull" % tk.HASH_MUL_INV in src
    assert tk.HASH_MUL * tk.HASH_MUL_INV % (1 << 64) == 1
    assert "#define XGGM_TOKENIZE_MAX_WORD %d" % tk.MAX_WORD in src and "#define XGGM_TOKENIZE_MAX_NEVER %d" % tk.MAX_NEVER in src
    mk = open(os.path.join(os.path.dirname(_lib.LIB_PATH), "Makefile")).read()
    assert "tokenize.hip" in [w for line in mk.splitlines() if line.startswith("SRCS") for w in line.split()]
    assert callable(ops.tokenize_wordpiece) and ops.TOKENIZE_OUTPUTS == ("ids", "len", "block", "flags", "flagged")


def _args(host_offsets):
    """a struct of fake, aligned device pointers that are never dereferenced and REAL host offsets.  Every caller passes
    offsets that are refused (the last check before the launch), so nothing can be launched from here whatever else a
    case changes."""
    a = ops.TokenizeArgs()
    fake = 0x7F0000000000
    for k, (name, _) in enumerate(ops.TokenizeArgs._fields_):
        if ops.TokenizeArgs._fields_[k][1] is ctypes.c_void_p:
            setattr(a, name, fake + 4096 * (k + 1))
    a.host_offsets = host_offsets.ctypes.data
    a.n, a.T, a.n_bytes = len(host_offsets) - 1, 20, 8
    a.n_ext, a.n_blob, a.init_cap, a.cont_cap, a.n_never = 4, 4, 16, 16, 5
    a.cls_id, a.sep_id, a.unk_id = 2, 3, 1
    return a


def _refused(a, *words):
    rc = _lib.lib.xggm_tokenize_wordpiece(ctypes.addressof(a) if a is not None else None, None)
    msg = _lib.lib.xggm_last_error().decode()
    assert rc != 0 and all(w in msg for w in words), (rc, msg, words)


def test_refusals_come_before_any_launch():
    falling = np.array([0, 5, 3], dtype=np.int64)
    _refused(None, "null argument struct")
    _refused(_args(falling), "offsets[2]=3", "not monotonic")
    _refused(_args(np.array([-1, 2, 3], dtype=np.int64)), "offsets[0]=-1", "not monotonic")
    _refused(_args(np.array([0, 5, 9], dtype=np.int64)), "offsets[2]=9", "past n_bytes=8")
    cases = [(dict(n=0), ("n=0",)), (dict(T=1), ("T=1",)), (dict(bytes=None), ("null bytes",)), (dict(offsets=None), ("null offsets",)),
             (dict(host_offsets=None), ("host_offsets",)), (dict(cp_table=None), ("null table",)), (dict(blob=None), ("null table",)),
             (dict(init_slots=None), ("null table",)), (dict(cont_slots=None), ("null table",)), (dict(cp_ext=None), ("null cp_ext",)),
             (dict(init_cap=24), ("capacity 24", "power of two")), (dict(cont_cap=0), ("power of two",)),
             (dict(n_never=9), ("n_never=9",)), (dict(never_cps=None), ("never_cps",)),
             (dict(ids=None, len=None, block=None, flags=None, flagged=None), ("every output pointer is null",)),
             (dict(ids=0x7F0000000002), ("misaligned pointer",)), (dict(len=0x7F0000000001), ("misaligned pointer",)),
             (dict(block=0x7F0000000004), ("misaligned pointer",)), (dict(flagged=0x7F0000000002), ("misaligned pointer",)),
             (dict(offsets=0x7F0000000004), ("misaligned pointer",)), (dict(init_slots=0x7F0000000008), ("misaligned table",)),
             (dict(cont_slots=0x7F0000000004), ("misaligned table",)), (dict(cp_table=0x7F0000000002), ("misaligned table",))]
    for change, words in cases:
        a = _args(falling)
        for k, v in change.items():
            setattr(a, k, v)
        _refused(a, "xggm_tokenize_wordpiece", *words)


def test_ops_and_device_tokenizer_refuse_the_cpu(synth):
    tok, tables, _ = synth
    off = np.array([0, 3], dtype=np.int64)
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        ops.tokenize_wordpiece(torch.zeros(3, dtype=torch.uint8), torch.from_numpy(off), off, 20, {})
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tk.DeviceTokenizer(tok, "cpu")


def test_packer():
    data, off, host = tk.pack_sentences(["ab", "", " c "])
    assert bytes(data) == b"ab c " and off.tolist() == [0, 2, 2, 5] and host == [] and off.dtype == np.int64
    data, off, host = tk.pack_sentences(["caf\u00e9", "x\ud800y", "\U0001f600"])
    assert bytes(data) == "caf\u00e9\U0001f600".encode() and off.tolist() == [0, 5, 5, 9] and host == [1]


# ----------------------------------------------------------------------------- the restatement against the host tokenizer
@pytest.mark.parametrize("part", range(8))
def test_restatement_every_code_point(synth, part):
    """"a" + c + "b" and c alone for every non-surrogate code point: the words the restatement hands to WordPiece are the
    tokens of ``BasicTokenizer`` and its ids the host tokenizer's -- except where it flags the row, which happens for the
    HOST code points and for nothing else"""
    tok, tables, R = synth
    basic = tok.basic_tokenizer
    T = 16
    for cp in NOT_SURROGATE[part::8]:
        c = chr(cp)
        is_host = tk.needs_host(cp, tk.fold_of(c))
        for s in ("a" + c + "b", c):
            R.trace = []
            ids, flag = R.row(s.encode("utf-8"), T)
            assert flag == is_host, (hex(cp), flag)
            if not flag:
                assert R.trace == basic.tokenize(s.strip()), (hex(cp), s, R.trace)
                assert ids == host_ids(tok, s, T), (hex(cp), s, ids)
    R.trace = None


def test_restatement_seeded_pairs(synth):
    """200 000 seeded pairs "a" + c + d + "b" of non-HOST code points, half of them drawn from the code points whose entry is
    not the trivial one (folds, drops, spaces, punctuation, CJK): tokens and ids equal the host's, nothing is flagged"""
    tok, tables, R = synth
    basic = tok.basic_tokenizer
    table = tables["cp_table"]
    ok = np.array([cp for cp in NOT_SURROGATE if int(table[cp]) & 7 != tk.ACT_HOST])
    special = ok[table[ok] != ((ok.astype(np.uint32) << 8) | 8)]
    rng = random.Random(C.SEED)
    assert len(special) > 50000
    for i in range(200000):
        c = chr(int(special[rng.randrange(len(special))] if i & 1 else ok[rng.randrange(len(ok))]))
        d = chr(int(special[rng.randrange(len(special))] if i & 2 else ok[rng.randrange(len(ok))]))
        s = "a" + c + d + "b"
        R.trace = []
        ids, flag = R.row(s.encode("utf-8"), 16)
        assert not flag and R.trace == basic.tokenize(s.strip()) and ids == host_ids(tok, s, 16), (hex(ord(c)), hex(ord(d)), R.trace, ids)
    R.trace = None


def test_restatement_golden_rows():
    """every sentence of tests/golden/tokenizer.json (the reference's own tokenizer) at every T of the fixture"""
    tok = tk.BertTokenizer(os.path.join(GOLDEN, "vocab_small.txt"), do_lower_case=True)
    R = tk.Restatement(tk.host_tables(tok))
    g = json.load(open(os.path.join(GOLDEN, "tokenizer.json")))
    for T_s, feats in g["features"].items():
        T = int(T_s)
        for s, (ids, mask, seg) in zip(g["sents"], feats):
            got, flag = R.row(s.encode("utf-8"), T)
            assert not flag and got + [0] * (T - len(got)) == ids and [1] * len(got) + [0] * (T - len(got)) == mask, (s, T, got)
    for s, toks in zip(g["sents"], g["tokens"]):
        assert tok.convert_ids_to_tokens(R.row(s.encode("utf-8"), 512)[0][1:-1]) == toks


def test_restatement_corpus_and_its_edges(synth):
    """the corpus of the GPU test: the restatement equals the host on its first 600 rows at T = 2, 3, 20, and the corpus
    holds what it is meant to hold -- rows of exactly T - 2, T - 1 and more tokens, words of 100 (pieces) and 101 ([UNK])
    code points, a matched prefix with an unmatched remainder, every never_split token, no HOST code point"""
    tok, tables, R = synth
    sents = C.synth_corpus(4000, C.T_MAIN)
    assert len(sents) == 4000 and all(int(tables["cp_table"][ord(c)]) & 7 != tk.ACT_HOST for s in sents for c in s)
    for T in (2, 3, C.T_MAIN):
        for s in sents[:600]:
            got, flag = R.row(s.encode("utf-8"), T)
            assert not flag and got == host_ids(tok, s, T), (s, T, got)
    n_tok = [len(tok.tokenize(s.strip())) for s in sents]
    L = C.T_MAIN - 2
    assert {L - 1, L, L + 1} <= set(n_tok) and max(n_tok) >= 60 and 0 in n_tok
    unk, a_id = tok.vocab["[UNK]"], tok.vocab["a"]
    assert tok.tokenize("a" * 100) == ["a"] + ["##a"] * 99 and tok.tokenize("a" * 101) == ["[UNK]"]
    assert tok.tokenize("a\u0301" * 100)[0] == "a" and tok.tokenize("a\u0301" * 101) == ["[UNK]"]
    assert tok.tokenize("theq") == ["[UNK]"] and tok.tokenize("the") == ["the"]
    for t in C.SPECIALS:
        assert t in sents and tok.tokenize(t[:3] + "\u200b" + t[3:]) == [t] and t[:3] + "\u200b" + t[3:] in sents
    assert R.row(("a" * 101).encode(), 8)[0][1] == unk and R.row(("a" * 100).encode(), 8)[0][1] == a_id
    for needle in ("", "     ", "\u2028", "\U0001f600", C.MOJIBAKE[0] + " zzz", "'''", "?!?!..."):
        assert needle in sents, repr(needle)


# ----------------------------------------------------------------------------- the HOST set and the hash tables
def test_host_set_is_exactly_sigma_and_the_surviving_non_starters():
    """the rows the kernel hands back are those with U+03A3 (final sigma) or a code point whose fold keeps a character of
    non-zero combining class (canonical reordering) -- computed here from ``unicodedata`` alone -- so the fallback cannot
    quietly grow"""
    table, ext = tk.code_point_table()
    got = set(np.nonzero((table & 7) == tk.ACT_HOST)[0].tolist())
    want = {0x3A3}
    for cp in range(0x110000):
        fold = [c for c in unicodedata.normalize("NFD", chr(cp).lower()) if unicodedata.category(c) != "Mn"]
        if any(unicodedata.combining(c) for c in fold):
            want.add(cp)
    assert got == want and 0x302E in got and 0x1B44 in got and len(got) < 64
    # the entries say what the host does with one character
    for cp in (0x41, 0xC9, 0x130, 0xDF, 0x4EBA, 0xF900, 0xAC01, 0x2028, 0xA0, 0xAD, 0xFFFD, 0x301, 0x2D, 0x1F600, 0x10400):
        e = int(table[cp])
        nf, payload = (e >> 3) & 3, e >> 8
        fold = [payload] if nf == 1 else [int(x) for x in ext[payload:payload + nf]]
        if e & 7 in (tk.ACT_KEEP, tk.ACT_CJK):
            assert fold == [ord(c) for c in tk.fold_of(chr(cp))], hex(cp)
            assert [bool(e >> (5 + f) & 1) for f in range(nf)] == [tk._is_punct(chr(c)) for c in fold]
    assert int(table[0x4EBA]) & 7 == tk.ACT_CJK and int(table[0x2028]) & 7 == tk.ACT_SPACE and int(table[0xAD]) & 7 == tk.ACT_DROP
    assert int(table[0xFFFD]) & 7 == tk.ACT_DROP and int(table[0]) & 7 == tk.ACT_DROP and int(table[0xA0]) & 7 == tk.ACT_SPACE


def test_hash_tables_resolve_every_entry(synth):
    tok, tables, R = synth
    for t, idx in tok.vocab.items():
        cps = [ord(c) for c in t]
        assert R.lookup(False, tk.piece_hash(cps), cps, 0, len(cps)) == idx, t
        if t.startswith("##") and len(t) > 2:
            assert R.lookup(True, tk.piece_hash(cps[2:]), cps, 2, len(cps)) == idx, t
    ab = [ord("x"), ord("a"), ord("b")]
    for cont in (False, True):  # absent keys, and a window inside a longer word
        assert R.lookup(cont, tk.piece_hash(ab), ab, 0, 3) == -1
    # dropping the last code point rolls the hash back
    h = tk.piece_hash(ab)
    assert ((h - (ab[-1] + 1)) * tk.HASH_MUL_INV) & ((1 << 64) - 1) == tk.piece_hash(ab[:2])


def test_word_and_continuation_are_distinct(tmp_path):
    p = tmp_path / "v.txt"
    p.write_text("\n".join(["[PAD]", "[UNK]", "[CLS]", "[SEP]", "ab", "##ab", "c", "", "ab"]) + "\n")
    tok = tk.BertTokenizer(str(p))
    assert tok.vocab["ab"] == 8 and tok.vocab["##ab"] == 5  # the later duplicate line wins, the blank line keeps its number
    R = tk.Restatement(tk.host_tables(tok))
    for s in ("ab", "abab", "cab", "ab ab", "abc", "ababab"):
        assert R.row(s.encode(), 16)[0] == host_ids(tok, s, 16), s
    assert R.row(b"abab", 16)[0] == [2, 8, 5, 3]


def test_full_table_long_probe_chains_and_failed_inserts():
    """1000 entries in 1024 slots -- the smallest capacity that fits -- still resolve, through probe chains far longer than
    the default load factor gives; an insert without room, a capacity that is no power of two and a repeated key raise"""
    rng = random.Random(5)
    keys = set()
    while len(keys) < 1000:
        keys.add(tuple(rng.randrange(97, 123) for _ in range(rng.randint(1, 6))))
    keys = sorted(keys)
    blob, entries = [], []
    for i, k in enumerate(keys):
        entries.append((k, i, len(blob)))
        blob.extend(k)
    slots = tk.build_hash_table(entries, 1024)
    assert slots.shape == (1024, 4) and int((slots[:, 1] != 0xFFFFFFFF).sum()) == 1000
    t = dict(cp_table=np.zeros(1, np.uint32), cp_ext=np.zeros(1, np.uint32), init_slots=slots, cont_slots=slots,
             blob=np.asarray(blob, dtype=np.uint32), n_blob=len(blob), never_off=np.zeros(1, np.int32), never_cps=np.zeros(1, np.uint32))
    R = tk.Restatement(t)
    longest = 0
    for k, i, _ in entries:
        assert R.lookup(False, tk.piece_hash(k), list(k), 0, len(k)) == i
        h = tk.piece_hash(k)
        home = (h ^ (h >> 32)) & 1023
        at = next(j for j in range(1024) if slots[(home + j) & 1023, 1] == i)
        longest = max(longest, at)
    assert longest >= 16
    absent = (1, 2, 3)
    assert R.lookup(False, tk.piece_hash(absent), list(absent), 0, 3) == -1
    with pytest.raises(ValueError, match="do not fit"):
        tk.build_hash_table(entries + [((1,), 1000, 0)] * 24, 1024)
    with pytest.raises(ValueError, match="power of two"):
        tk.build_hash_table(entries, 1500)
    with pytest.raises(ValueError, match="repeated key"):
        tk.build_hash_table(entries[:3] + entries[:1], 16)
