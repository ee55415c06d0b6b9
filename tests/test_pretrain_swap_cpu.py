"""CPU-only checks of the pre-training loop's new pieces: the swap's entry point is exported and documented, refuses bad
arguments before anything is launched (no device is present here), ``ops.pretrain_swap`` refuses CPU tensors, the golden
recorded from the reference (tests/golden/pretrain_swap.npz) follows the stated rule, the seed of the GPU distribution test
satisfies that test's conditions, ``collate_examples`` builds the clean batch and ``trainlog.pretrain_means`` decodes a
packed log."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import pretrain_mask_ref as R
from helpers import GOLDEN, load_golden

P = 4096  # a non-null, 16-byte aligned address nothing dereferences: every call below is refused on the host
SID = 0x70726500
TRIES = 8
# the GPU distribution test's case (tests/test_pretrain_swap_gpu.py imports these)
DIST_B, DIST_IMAGES, DIST_SEED = 4096, 64, 2025


def swap_rule(u_swap, u_pick, img, pool_img, matched_in=None, rate=0.5):
    """the contract of xggm_pretrain_swap in numpy and Python floats -> (sentence index per row, is_matched, exhausted)"""
    n, p = len(u_swap), len(pool_img)
    u_pick = np.asarray(u_pick).reshape(n, -1)
    idx = np.arange(n, dtype=np.int64)
    matched = np.ones(n, dtype=np.int64) if matched_in is None else np.array(matched_in, dtype=np.int64)
    exhausted = 0
    for b in range(n):
        if matched[b] != 1 or not float(u_swap[b]) < rate:
            continue
        for r in range(u_pick.shape[1]):
            j = min(int(float(u_pick[b, r]) * p), p - 1)
            if pool_img[j] != img[b]:
                idx[b], matched[b] = j, 0
                break
        else:
            exhausted += 1
    return idx, matched, exhausted


def dist_case():
    """-> (img [B] int64, u_swap, u_pick [B, 8]) of the distribution test: 64 images, Philox draws of DIST_SEED at offset 0"""
    img = np.random.default_rng(DIST_SEED).integers(0, DIST_IMAGES, size=DIST_B).astype(np.int64)
    return img, R.philox_uniform(DIST_SEED, 0, SID + 5, DIST_B), R.philox_uniform(DIST_SEED, 0, SID + 6, DIST_B * TRIES).reshape(DIST_B, TRIES)


def test_symbol_is_exported_and_cites_the_reference():
    from xggm_amd import _lib, ops
    assert "xggm_pretrain_swap" in _lib.parse_header() and hasattr(_lib.lib, "xggm_pretrain_swap")
    src = open(_lib.HEADER_PATH).read()
    doc = src[src.index("/* xggm_pretrain_swap:"):src.index("#define XGGM_PRETRAIN_SWAP_TRIES")]
    assert "src/pretrain/lxmert_data.py:173-183" in doc
    assert "no bound" in doc and "floor(u * n)" in doc  # the two deviations are stated in the contract
    assert "#define XGGM_PRETRAIN_SWAP_TRIES %d" % ops.PRETRAIN_SWAP_TRIES in src and ops.PRETRAIN_SWAP_TRIES == TRIES
    assert callable(ops.pretrain_swap) and ops.PRETRAIN_SWAP_DRAWS == ("u_swap", "u_pick")
    mk = open(os.path.join(os.path.dirname(_lib.HEADER_PATH), "..", "x-ggm_amd", "csrc", "Makefile")).read()
    assert "pretrain_swap.hip" in mk


def _refused(a):
    from xggm_amd import _lib
    rc = _lib.lib.xggm_pretrain_swap(ctypes.addressof(a) if a is not None else None, None)
    assert rc != 0
    return _lib.lib.xggm_last_error()


def _good():
    from xggm_amd import ops
    a = ops.PretrainSwapArgs()
    a.ids, a.mask, a.img, a.matched_in = P, 2 * P, 3 * P, 4 * P
    a.pool_ids, a.pool_mask, a.pool_img = 5 * P, 6 * P, 7 * P
    a.out_ids, a.out_mask, a.is_matched, a.exhausted = 8 * P, 9 * P, 10 * P, 11 * P
    a.B, a.T, a.P, a.rate = 6, 7, 7, 0.5
    a.u_swap, a.u_pick, a.rng, a.sid_base = 12 * P, 13 * P, 14 * P, SID
    return a


def test_every_listed_refusal_comes_before_a_launch():
    assert b"null argument struct" in _refused(None)
    for field in ("ids", "mask", "img"):
        a = _good()
        setattr(a, field, None)
        assert b"null ids / mask / img" in _refused(a), field
    for field in ("out_ids", "out_mask", "is_matched", "exhausted"):
        a = _good()
        setattr(a, field, None)
        assert b"null output pointer" in _refused(a), field
    for field, bad in (("B", 0), ("B", -2), ("T", 0), ("T", -1)):
        a = _good()
        setattr(a, field, bad)
        assert b"must both be positive" in _refused(a), field
    for bad in (0, -5):
        a = _good()
        a.P = bad
        assert b"pool of" in _refused(a)
    for field in ("pool_ids", "pool_mask", "pool_img"):
        a = _good()
        setattr(a, field, None)
        assert b"a pool needs" in _refused(a), field
    for field in ("pool_ids", "pool_mask", "pool_img"):  # ... and one of the three alone
        a = _good()
        for other in {"pool_ids", "pool_mask", "pool_img"} - {field}:
            setattr(a, other, None)
        assert b"a pool needs" in _refused(a), field
    for rate in (-0.01, 1.01, float("nan")):
        a = _good()
        a.rate = rate
        assert b"outside [0, 1]" in _refused(a), rate
    for field in ("u_swap", "u_pick"):
        a = _good()
        setattr(a, field, None)
        a.rng = None
        assert b"needs rng" in _refused(a), field
    a = _good()
    a.out_ids = a.ids  # in place: a NULL pool reads the batch's rows while others write them
    assert b"aliases" in _refused(a)
    a = _good()
    a.out_mask = a.pool_mask + 8
    assert b"aliases" in _refused(a)
    for field, other in (("is_matched", "matched_in"), ("is_matched", "img"), ("exhausted", "pool_img"), ("out_ids", "pool_ids")):
        a = _good()
        setattr(a, field, getattr(a, other))
        assert b"aliases" in _refused(a), (field, other)
    for field, other in (("out_mask", "out_ids"), ("is_matched", "out_mask"), ("exhausted", "is_matched")):
        a = _good()
        setattr(a, field, getattr(a, other))
        assert b"two outputs alias" in _refused(a), (field, other)


def test_host_wrapper_checks_operands_and_refuses_cpu_tensors():
    from xggm_amd import ops
    from xggm_amd.pretrain.lxmert_pretrain import DeviceFeatures
    ids = torch.zeros(6, 7, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.pretrain_swap(ids, ids.clone(), torch.zeros(6, dtype=torch.int64), draws=dict(u_swap=torch.zeros(6), u_pick=torch.zeros(6, 8)))
    with pytest.raises(ValueError, match="match_rate"):
        DeviceFeatures(match_rate=1.5)
    assert DeviceFeatures().match_rate is None  # the default launches no swap
    from xggm_amd import param
    assert DeviceFeatures.from_args(param.parse_args(["--taskMatched"]), swap=True).match_rate == 0.5
    assert DeviceFeatures.from_args(param.parse_args([]), swap=True).match_rate is None
    assert DeviceFeatures.from_args(param.parse_args(["--taskMatched"])).match_rate is None  # as before: opt-in


def test_golden_follows_the_stated_rule():
    g = load_golden("pretrain_swap")
    B, T, Pn, Rn = (int(x) for x in g["cfg"])
    assert (B, T, Pn, Rn) == (6, 7, 7, TRIES) and g["u_swap"].dtype == np.float32 and g["u_pick"].shape == (B, Rn)
    assert len(set(g["pool_img"].tolist())) == 3
    idx, matched, exhausted = swap_rule(g["u_swap"], g["u_pick"], g["pool_img"][:B], g["pool_img"], rate=float(g["rate"][0]))
    assert exhausted == 0 and idx.tolist() == g["sent_index"].tolist() and matched.tolist() == g["is_matched"].tolist()
    # the recorded stream holds the cases the kernel can get wrong
    half = np.float32(0.5)
    assert g["u_swap"][0] == half and g["is_matched"][0] == 1                          # u == rate stays matched
    assert g["u_swap"][1] == np.nextafter(half, np.float32(0)) and g["is_matched"][1] == 0
    assert int(g["n_picks"][2]) == 3 and int(g["n_picks"].max()) - 1 <= Rn - 1         # own image twice, then another
    for r in range(2):
        assert g["pool_img"][int(float(g["u_pick"][2, r]) * Pn)] == g["pool_img"][2]
    top = np.nextafter(np.float32(1), np.float32(0))
    assert g["u_pick"][3, 0] == top and g["sent_index"][3] == Pn - 1                   # the draw nearest the pool's end
    assert (g["pool_mask"].sum(1) == T).any() and len(set(g["pool_mask"].sum(1).tolist())) > 2


def test_distribution_seed_satisfies_its_conditions():
    """the GPU test relies on this seed: share of swapped rows within 4 binomial standard deviations of 0.5, no row exhausted,
    every swapped row shows another image -- verified here from the host restatement of the Philox draws"""
    img, u_swap, u_pick = dist_case()
    assert len(set(img.tolist())) == DIST_IMAGES
    idx, matched, exhausted = swap_rule(u_swap, u_pick, img, img)
    share = float((matched == 0).mean())
    bound = 4 * math.sqrt(0.25 / DIST_B)
    print("swapped share %.4f (bound 0.5 +- %.4f), exhausted %d" % (share, bound, exhausted))
    assert abs(bound - 0.03125) < 1e-12 and bound <= 0.032
    assert abs(share - 0.5) <= bound and exhausted == 0
    assert (img[idx[matched == 0]] != img[matched == 0]).all() and (idx[matched == 1] == np.arange(DIST_B)[matched == 1]).all()


# ------------------------------------------------------------------------------------------------ the driver's host side
def _example(uid, sent, label=None, O=2, F=3, k=0.0):
    from xggm_amd.pretrain.lxmert_pretrain import InputExample
    return InputExample(uid, sent, (np.full((O, F), k, dtype=np.float32), np.full((O, 4), k / 10, dtype=np.float32)),
                        (np.arange(O, dtype=np.int64), np.full(O, 0.5, dtype=np.float32)),
                        (np.arange(O, dtype=np.int64) + 1, np.full(O, 0.25, dtype=np.float32)), 1, label)


def test_collate_examples_builds_the_clean_batch():
    from xggm_amd.lxrt.tokenization import BertTokenizer
    from xggm_amd.pretrain.lxmert_pretrain import collate_examples, image_key, InputExample
    tok = BertTokenizer(os.path.join(GOLDEN, "vocab_small.txt"), do_lower_case=True)
    v = tok.vocab
    ex = [_example(("img7_vqa_000",), "What is the man holding woman", {3: 0.3, 7: 1.0}, k=1.0),
          _example(("img9_vqa_001",), " woman ", None, k=2.0),
          _example(("img7_vqa_002",), "", {5: 1.0}, k=3.0)]
    T = 6
    b = collate_examples(ex, tok, T, 2)
    words = tok.convert_tokens_to_ids(tok.tokenize("what is the man holding woman"))
    assert len(words) > T - 2  # the first sentence is cut at max_seq_length - 2 tokens
    want = [[v["[CLS]"]] + words[:T - 2] + [v["[SEP]"]], [v["[CLS]"], v["woman"], v["[SEP]"], 0, 0, 0], [v["[CLS]"], v["[SEP]"], 0, 0, 0, 0]]
    assert b["input_ids"].tolist() == want and b["input_ids"].dtype == torch.int64
    assert b["input_mask"].tolist() == [[1] * 6, [1, 1, 1, 0, 0, 0], [1, 1, 0, 0, 0, 0]]
    assert b["segment_ids"].tolist() == [[0] * 6] * 3
    assert b["feats"].shape == (3, 2, 3) and b["feats"].dtype == torch.float32 and b["feats"][:, 0, 0].tolist() == [1.0, 2.0, 3.0]
    assert b["boxes"].shape == (3, 2, 4) and b["obj_labels"].tolist() == [[0, 1]] * 3 and b["attr_labels"].tolist() == [[1, 2]] * 3
    assert b["obj_confs"].dtype == torch.float32 and b["attr_confs"][0].tolist() == [0.25, 0.25]
    assert b["is_matched"].tolist() == [1, 1, 1] and b["is_matched"].dtype == torch.int64
    assert b["label_ids"].tolist() == [[3, 7], [-1, -1], [5, -1]] and b["label_scores"][0].tolist() == [pytest.approx(0.3), 1.0]
    # img_ids: one integer per distinct image, the same in another batch and for a plain-string uid; no masking, no swap
    k = b["img_ids"].tolist()
    assert k[0] == k[2] != k[1] and min(k) >= 0 and b["img_ids"].dtype == torch.int64
    again = collate_examples([ex[1], InputExample("img7_gqa_010", "man", ex[0].visual_feats, ex[0].obj_labels, ex[0].attr_labels, 1, None)], tok, T, 2)
    assert again["img_ids"].tolist() == [k[1], k[0]] and image_key(ex[0]) == k[0]
    assert sorted(b) == sorted(["input_ids", "input_mask", "segment_ids", "feats", "boxes", "obj_labels", "obj_confs", "attr_labels",
                                "attr_confs", "is_matched", "label_ids", "label_scores", "img_ids"])
    with pytest.raises(ValueError, match="answer keys"):
        collate_examples([_example("a_b_000", "man", {1: 0.1, 2: 0.2, 3: 0.3})], tok, T, 2)


def test_pretrain_means_on_a_synthetic_packed_buffer():
    from xggm_amd import trainlog as T
    assert T.PRETRAIN == 3 < T.KINDS and T.LOSSES_NAME == ('Mask_LM', 'Matched', 'Obj', 'Attr', 'Feat', 'QA')
    assert (T.PT_MASK_LM, T.PT_MATCHED, T.PT_OBJ, T.PT_ATTR, T.PT_FEAT, T.PT_QA, T.PT_GRAD_NORM) == (1, 2, 3, 4, 5, 6, 7) and T.COLS == 8
    cap, steps = 2, 3  # three steps in a ring of two: the means still cover all three (they come from the running sums)
    w = torch.zeros(T.words(cap), dtype=torch.int64)
    o = T.HEADER + cap
    values = w[o:o + cap * T.COLS // 2].view(torch.float32).view(cap, T.COLS)
    kinds = w[o + cap * T.COLS // 2:].view(torch.int32)
    sums = w[2 + T.KINDS:T.HEADER].view(torch.float64).view(T.KINDS, T.COLS)
    present = [T.LOSS, T.PT_MASK_LM, T.PT_MATCHED, T.PT_OBJ, T.PT_FEAT, T.PT_GRAD_NORM]  # Attr and QA are off
    mask = sum(1 << c for c in present)
    rows = [[10.0 * (s + 1) + c if c in present else 0.0 for c in range(T.COLS)] for s in range(steps)]
    for s, row in enumerate(rows):
        values[s % cap] = torch.tensor(row)
        kinds[s % cap] = T.PRETRAIN | (mask << 8)
        w[T.HEADER + s % cap] = s + 1
        sums[T.PRETRAIN] += torch.tensor(row, dtype=torch.float64)
    sums[T.PLAIN, T.LOSS] = 123.0  # another kind's sums do not leak in
    w[0], w[1], w[2 + T.PRETRAIN] = steps, -1, steps
    rec = T.decode_packed(w, cap)
    assert rec["kinds"].tolist() == [T.PRETRAIN] * 2 and rec["steps"].tolist() == [2, 3]
    mean, terms, n = T.pretrain_means(rec)
    assert n == steps and mean == pytest.approx(20.0)
    assert [name for name, _ in terms] == ['Mask_LM', 'Matched', 'Obj', 'Feat']
    assert [v for _, v in terms] == [pytest.approx(20.0 + c) for c in (1, 2, 3, 5)]
    empty = T.decode_packed(torch.zeros(T.words(cap), dtype=torch.int64), cap)
    assert T.pretrain_means(empty) == (0.0, [], 0)
