"""WordPiece on the GPU (xggm_tokenize_wordpiece, ``ops.tokenize_wordpiece``, ``lxrt.tokenization.DeviceTokenizer``): the
reference's own rows (tests/golden/tokenizer.json), a seeded corpus that holds every edge the kernel has a branch for
against the host tokenizer at the sizes where the launch changes shape, the host fallback -- which rows are flagged and
that an unflagged corpus needs no host row --, and the three places that take a ``DeviceTokenizer``.  Integer work: every
comparison is ``torch.equal``."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import GOLDEN  # noqa: E402
from xggm_amd import ops  # noqa: E402
from xggm_amd.lxrt.tokenization import ACT_HOST, BertTokenizer, DeviceTokenizer, code_point_table, pack_sentences  # noqa: E402
import tokenize_cases as C  # noqa: E402

DEV = "cuda"
ALL = ("ids", "len", "block", "flags", "flagged")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def small():
    tok = BertTokenizer(os.path.join(GOLDEN, "vocab_small.txt"), do_lower_case=True)
    return tok, DeviceTokenizer(tok, DEV)


@pytest.fixture(scope="module")
def synth(tmp_path_factory):
    tok = C.synth_tokenizer(tmp_path_factory.mktemp("vocab"))
    return tok, DeviceTokenizer(tok, DEV)


def launch(dt, rows, T, sentinel=None):
    """ONE launch with every output.  ``rows``: strings, or raw byte strings"""
    if isinstance(rows[0], bytes):
        data = np.frombuffer(b"".join(rows), dtype=np.uint8)
        off = np.cumsum([0] + [len(r) for r in rows]).astype(np.int64)
    else:
        data, off, unencodable = pack_sentences(rows)
        assert not unencodable
    n = len(rows)
    out = None
    if sentinel is not None:
        out = dict(ids=torch.full((n, T), sentinel, dtype=torch.int32, device=DEV), len=torch.full((n,), sentinel, dtype=torch.int32, device=DEV),
                   block=torch.full((3, n, T), sentinel, dtype=torch.int64, device=DEV),
                   flags=torch.full((n,), 0xA5, dtype=torch.uint8, device=DEV))
    d = torch.from_numpy(data.copy()).to(DEV) if len(data) else torch.empty(0, dtype=torch.uint8, device=DEV)
    return ops.tokenize_wordpiece(d, torch.from_numpy(off).to(DEV), off, T, dt.tables, outputs=ALL, out=out)


def check_rows(out, want_ids, want_len, T):
    """both output forms against host rows (numpy int64 [n, T], [n])"""
    ids, lens = torch.from_numpy(want_ids), torch.from_numpy(want_len)
    assert torch.equal(out["ids"].cpu(), ids.int()) and torch.equal(out["len"].cpu(), lens.int())
    mask = (torch.arange(T)[None, :] < lens[:, None]).long()
    assert torch.equal(out["block"].cpu(), torch.stack([ids, mask, torch.zeros_like(ids)]))


def test_golden_rows_in_one_launch(small):
    """the sentences of tests/golden/tokenizer.json (recorded from the reference's tokenizer) give the golden ids, mask and
    segment ids at every T of the fixture, as int32 ids / len and as the int64 block, all from one launch"""
    tok, dt = small
    g = json.load(open(os.path.join(GOLDEN, "tokenizer.json")))
    for T_s, feats in g["features"].items():
        T = int(T_s)
        want = torch.tensor(feats, dtype=torch.int64).permute(1, 0, 2).contiguous()  # [3, n, T]
        out = launch(dt, g["sents"], T, sentinel=-7)
        assert torch.equal(out["block"].cpu(), want)
        assert torch.equal(out["ids"].cpu(), want[0].int()) and torch.equal(out["len"].cpu(), want[1].sum(1).int())
        assert int(out["flagged"]) == 0 and not bool(out["flags"].any())
        f = dt.features(g["sents"], T)
        assert all(torch.equal(a.cpu(), b) for a, b in zip(f, want)) and dt.last_host_rows == 0


@pytest.mark.parametrize("T", [2, 3, C.T_MAIN])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4000])
def test_synthetic_corpus_equals_the_host_rows(synth, n, T):
    """the seeded corpus of tests/tokenize_cases.py (empty and blank strings, words of 100 and 101 code points, unmatched
    remainders, exactly T - 2 / T - 1 / many tokens, every never_split token, CJK, accents, mojibake, 4-byte UTF-8,
    punctuation runs, U+2028) over a 2000-entry vocabulary with multi-byte pieces: every row equals the host's, nothing is
    flagged, nothing is left unwritten (the outputs start as a sentinel).  n: below, at and above one workgroup, and many."""
    tok, dt = synth
    sents = C.synth_corpus(4000, C.T_MAIN)
    want_ids, want_len = C.host_rows(tok, sents, T)
    order = np.arange(n) if n == 4000 else (np.arange(n) * 61) % 4000  # small n: a stride through the corpus, edges included
    out = launch(dt, [sents[i] for i in order], T, sentinel=-7)
    check_rows(out, want_ids[order], want_len[order], T)
    assert int(out["flagged"]) == 0 and not bool(out["flags"].any())


def _has_host(s):
    table = code_point_table()[0]
    return any(int(table[ord(c)]) & 7 == ACT_HOST for c in s)


def test_fallback_flags_exactly_the_host_rows(synth):
    """a row is flagged if and only if it holds a HOST code point (T large enough that no sentence stops early); the
    flagged rows come back as the host's rows and are counted; a corpus without one needs NO host row -- the cap that keeps
    the fallback from hiding a kernel error"""
    tok, dt = synth
    T = 128
    sents = list(C.synth_corpus(4000, C.T_MAIN)[400:600])
    hosts = ["the \u03a3 ba", "\u03a3", "\u039f\u0394\u039f\u03a3 \u03a3\u039f\u03a6\u039f\u03a3", "a\u302e\u302fb", "ka\u1b44", "the\u03a3", "[MASK] \u03a3"]
    for k, h in enumerate(hosts):
        sents.insert(7 + 23 * k, h)
    expect = torch.tensor([_has_host(s) for s in sents])
    assert int(expect.sum()) == len(hosts)
    out = launch(dt, sents, T)
    assert torch.equal(out["flags"].cpu().bool(), expect) and int(out["flagged"]) == len(hosts)
    want_ids, want_len = C.host_rows(tok, sents, T)
    ids, lens = dt.encode(sents, T)
    assert dt.last_host_rows == len(hosts)
    assert torch.equal(ids.cpu(), torch.from_numpy(want_ids).int()) and torch.equal(lens.cpu(), torch.from_numpy(want_len).int())
    f = dt.features(sents, T)
    assert torch.equal(f[0].cpu(), torch.from_numpy(want_ids)) and torch.equal(f[1].sum(1).cpu(), torch.from_numpy(want_len))
    clean = C.synth_corpus(4000, C.T_MAIN)
    dt.encode(clean, C.T_MAIN)
    assert dt.last_host_rows == 0
    # a string strict UTF-8 cannot encode never reaches the kernel: the packer hands it to the host
    odd = ["the ba", "the \ud800 ba", "de"]
    ids, lens = dt.encode(odd, 8)
    w_ids, w_len = C.host_rows(tok, odd, 8)
    assert dt.last_host_rows == 1 and torch.equal(ids.cpu(), torch.from_numpy(w_ids).int()) and torch.equal(lens.cpu(), torch.from_numpy(w_len).int())


def test_host_character_behind_the_truncation_point(synth):
    """the kernel stops a sentence at T - 2 tokens: a HOST character behind that point is not read, and the row still
    equals the host's (whether it was flagged or not)"""
    tok, dt = synth
    T = C.T_MAIN
    sents = [" ".join(["the"] * 30) + " \u03a3", " ".join(["the"] * (T - 2)) + "\u03a3", " ".join(["the"] * (T - 3)) + " \u03a3 the",
             " ".join(["the"] * (T - 2)) + " a\u302e\u302fb"]
    want_ids, want_len = C.host_rows(tok, sents, T)
    ids, lens = dt.encode(sents, T)
    assert torch.equal(ids.cpu(), torch.from_numpy(want_ids).int()) and torch.equal(lens.cpu(), torch.from_numpy(want_len).int())
    out = launch(dt, sents, T)
    assert out["flags"].cpu().tolist() == [0, 1, 1, 0]  # row 1: the character belongs to the word that reaches the limit


def test_malformed_bytes_are_flagged_and_fully_written(synth):
    """raw rows with a cut-off multi-byte tail, stray continuation bytes, an overlong form, a surrogate and a value past
    U+10FFFF, through the low-level op: flagged, every element written, ids inside the vocabulary, the bytes around the
    bad ones tokenised as if it were dropped"""
    tok, dt = synth
    T = 12
    rows = [b"the caf\xc3", b"\xe4\xba", b"\xf0\x9f\x98", b"\xff\xfe the", b"a\xc0\xafb", b"\xed\xa0\x80 the", b"[UN\xffK] [MAS\xf0\x9f",
            b"\xf4\x90\x80\x80", b"the ba", "caf\u00e9".encode(), b"\x80", b"the \xe2\x80"]
    out = launch(dt, rows, T, sentinel=-7)
    assert out["flags"].cpu().tolist() == [1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 1, 1] and int(out["flagged"]) == 10
    ids, lens, block = out["ids"].cpu(), out["len"].cpu(), out["block"].cpu()
    V = len(tok.vocab)
    assert int(ids.min()) >= 0 and int(ids.max()) < V and int(lens.min()) >= 2 and int(lens.max()) <= T
    assert torch.equal(block[0], ids.long()) and torch.equal(block[1], (torch.arange(T)[None, :] < lens[:, None]).long())
    assert not bool(block[2].any())
    as_dropped = ["the caf", "", "", " the", "ab", " the", "[UNK] [MAS", "", "the ba", "caf\u00e9", "", "the "]
    want_ids, want_len = C.host_rows(tok, as_dropped, T)
    assert torch.equal(ids, torch.from_numpy(want_ids).int()) and torch.equal(lens, torch.from_numpy(want_len).int())


def test_pretrain_tables_take_a_device_tokenizer(small):
    from pretrain_resident_cases import make_examples
    from xggm_amd.pretrain.resident import pretrain_tables
    tok, dt = small
    ex = make_examples(4, 8, 3, 20)
    host, dev = pretrain_tables(ex, tok, 20, 3), pretrain_tables(ex, dt, 20, 3)
    assert dt.last_host_rows == 0
    for k in ("q_ids", "q_len", "q_row", "q_label"):
        assert torch.equal(torch.from_numpy(dev[k]), torch.from_numpy(host[k])), k


def test_sample_tables_take_a_batcher_with_a_device_tokenizer(small, tmp_path):
    from test_resident_gpu import _shard
    from xggm_amd.lxrt.entry import SentenceBatcher
    from xggm_amd.tools.resident import sample_tables
    tok, dt = small
    ts = _shard(tmp_path, 6, 13, 64, 11, 96)
    host, dev = sample_tables(ts, SentenceBatcher(tok, 20)), sample_tables(ts, SentenceBatcher(dt, 20))
    assert dt.last_host_rows == 0
    for k in ("q_ids", "q_len", "q_row", "q_label", "q_score"):
        assert torch.equal(torch.from_numpy(dev[k]), torch.from_numpy(host[k])), k


def test_string_fed_forward_uses_the_device_tokenizer(small):
    """``LXRTEncoderFeature.enable_device_tokenizer()``: a tiny model's forward on strings equals its forward on the
    host-built id tensors"""
    from oracle import shapes
    from test_model_gpu import build_model
    from xggm_amd import synth as S
    from xggm_amd.lxrt.entry import convert_sents_to_features
    from helpers import batch_tensors
    tok, _ = small
    cfg = dict(shapes.TINY, vocab=96)
    m = build_model(cfg, 11, seed=3, dt=torch.bfloat16).eval()
    m.lxrt_encoder.tokenizer = tok
    dt = m.lxrt_encoder.enable_device_tokenizer()
    sents = ["What is the man holding?", "how many people are there", "is it a dog-like cat?!", "", "caf\u00e9 [MASK] \u4eba"]
    b = batch_tensors(S.vqa_batch(len(sents), A=11, F=cfg["feat_dim"], vocab=cfg["vocab"], seed=1), DEV)
    with torch.no_grad():
        (l1, v1), mask1, x1 = m(b["feats"], b["boxes"], sents)
        assert dt.last_host_rows == 0
        f = convert_sents_to_features(sents, m.lxrt_encoder.max_seq_length, tok)
        ids, msk, seg = (torch.tensor([getattr(q, k) for q in f], device=DEV) for k in ("input_ids", "input_mask", "segment_ids"))
        (l2, v2), mask2, x2 = m(b["feats"], b["boxes"], (ids, msk, seg))
    assert torch.equal(mask1, mask2) and torch.equal(l1, l2) and torch.equal(v1, v2) and torch.equal(x1, x2)
