"""CPU-only checks of the resident pre-training set: ``xggm_pretrain_gather`` is exported and documented and refuses bad
arguments before anything is launched (no device is present here), ``ops.pretrain_gather`` refuses CPU tensors, the numpy
restatement ``gather_pretrain_host`` equals ``collate_examples`` without a swap and ``swap_rule`` (the contract of
xggm_pretrain_swap, imported unchanged) with one, ``pretrain_tables`` validates what the kernel will trust, and ``order``
is ``ResidentDataset.order``."""
import ctypes
import os

import numpy as np
import pytest
import torch

from pretrain_resident_cases import IMG_OF, N_IMG, N_Q, make_examples, tok
from test_pretrain_swap_cpu import swap_rule

P = 1 << 16  # non-null, 16-byte aligned addresses far enough apart that no two buffers of _good() overlap; never dereferenced
TRIES = 8


def test_symbol_is_exported_and_cites_the_reference():
    from xggm_amd import _lib, ops
    assert "xggm_pretrain_gather" in _lib.parse_header() and hasattr(_lib.lib, "xggm_pretrain_gather")
    src = open(_lib.HEADER_PATH).read()
    doc = src[src.index("/* xggm_pretrain_gather:"):src.index("typedef struct xggm_pretrain_gather_args")]
    assert "src/pretrain/lxmert_data.py:148-199" in doc
    assert "Refused before any launch" in doc and "XGGM_PRETRAIN_SWAP_TRIES" in doc
    assert _lib.lib.xggm_version() == 100
    mk = open(os.path.join(os.path.dirname(_lib.HEADER_PATH), "..", "x-ggm_amd", "csrc", "Makefile")).read()
    assert "pretrain_gather.hip" in mk
    assert callable(ops.pretrain_gather) and set(ops.PRETRAIN_GATHER_OUT) == set(_keys()) | {"img_ids"}


def _keys():
    from xggm_amd.engine import CapturedPretrainer
    return CapturedPretrainer.KEYS


def _good():
    from xggm_amd import ops
    a = ops.PretrainGatherArgs()
    ptrs = [k for k, t in ops.PretrainGatherArgs._fields_ if t is ctypes.c_void_p]
    for i, k in enumerate(ptrs):
        setattr(a, k, (i + 1) * P)
    a.n_img, a.n_q, a.n, a.start = 6, 13, 20, 13
    a.B, a.T, a.K, a.O, a.F = 7, 7, 3, 5, 8
    a.out_feats_stride, a.feats_f32, a.out_f32 = 48, 1, 0
    a.swap, a.rate, a.sid_base = 1, 0.5, 0x70726500
    return a


def _refused(a):
    from xggm_amd import _lib
    rc = _lib.lib.xggm_pretrain_gather(ctypes.addressof(a) if a is not None else None, None)
    assert rc != 0
    return _lib.lib.xggm_last_error()


def _with(**kw):
    a = _good()
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_every_listed_refusal_comes_before_a_launch():
    from xggm_amd import ops
    assert b"null argument struct" in _refused(None)
    optional = {"sample", "swapped_from", "u_swap", "u_pick", "rng", "exhausted"}
    required = [k for k, t in ops.PretrainGatherArgs._fields_ if t is ctypes.c_void_p and k not in optional]
    assert len(required) == 11 + 1 + 13  # tables, order, outputs
    for k in required:  # a null required pointer; an output whose table is NULL (every output's table is required)
        assert b"null" in _refused(_with(**{k: None})), k
    for k in ("feats", "boxes", "out_feats", "out_boxes"):
        assert b"16-byte aligned" in _refused(_with(**{k: getattr(_good(), k) + 8})), k
    for k in ("obj_labels", "attr_confs", "q_row", "q_ids", "q_len", "q_label", "q_score", "out_obj_confs", "label_scores", "u_swap",
              "u_pick", "exhausted"):
        assert b"4-byte field" in _refused(_with(**{k: getattr(_good(), k) + 2})), k
    for k in ("order", "out_obj_labels", "input_ids", "input_mask", "segment_ids", "label_ids", "is_matched", "img_ids", "sample",
              "swapped_from", "rng"):
        assert b"8-byte field" in _refused(_with(**{k: getattr(_good(), k) + 4})), k
    for b in (0, -1):
        assert b"at least one row" in _refused(_with(B=b))
    assert b"65535" in _refused(_with(B=65536, n=1 << 20))
    for start, n in ((-1, 20), (14, 20), (0, 6)):
        assert b"leave order" in _refused(_with(start=start, n=n)), (start, n)
    for k in ("T", "K", "O", "F", "n_img", "n_q"):
        for bad in (0, -3):
            assert b"must all be positive" in _refused(_with(**{k: bad})), k
    for f in (4, 12, 9):
        assert b"multiple of 8" in _refused(_with(F=f, out_feats_stride=5 * f + 8 - (5 * f) % 8)), f
    assert b"row stride" in _refused(_with(out_feats_stride=32))   # below the row of 40
    assert b"row stride" in _refused(_with(out_feats_stride=44))   # no multiple of 8
    for rate in (-0.01, 1.01, float("nan")):
        assert b"outside [0, 1]" in _refused(_with(rate=rate)), rate
    assert b"exhausted" in _refused(_with(exhausted=None))
    for k in ("u_swap", "u_pick"):
        assert b"needs rng" in _refused(_with(**{k: None, "rng": None})), k
    g = _good()
    for out, table in (("out_feats", "feats"), ("input_ids", "q_ids"), ("img_ids", "q_row"), ("label_scores", "q_score"),
                       ("is_matched", "order"), ("out_boxes", "boxes"), ("exhausted", "u_swap"), ("sample", "rng")):
        assert b"aliases" in _refused(_with(**{out: getattr(g, table)})), (out, table)
    assert b"aliases" in _refused(_with(input_mask=g.q_ids + 13 * 7 * 4 - 4))  # the last four bytes of a table
    for x, y in (("input_mask", "input_ids"), ("sample", "swapped_from"), ("img_ids", "is_matched"), ("exhausted", "label_scores")):
        assert b"two outputs alias" in _refused(_with(**{x: getattr(g, y)})), (x, y)
    assert b"two outputs alias" in _refused(_with(segment_ids=g.input_ids + 6 * 7 * 8))  # its last row
    # without a swap none of the swap's fields is looked at
    from xggm_amd import _lib
    for a in (_good(), _with(swap=0, rate=7.0, exhausted=None, rng=None, u_swap=None, u_pick=None)):
        a.B = 0  # (still refused: nothing may be launched without a device)
        assert b"at least one row" in _refused(a)


def test_host_wrapper_checks_operands_and_refuses_cpu_tensors():
    from xggm_amd import ops
    from xggm_amd.pretrain.resident import ResidentPretrainSet
    store = ResidentPretrainSet(make_examples(5, 8, 3, 7), "cpu", tokenizer=tok(), max_seq_length=7, max_labels=3, batch_size=4)
    out = store.buffers(4)
    with pytest.raises(RuntimeError, match="GPU"):
        store.fill(out, 0, 4)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.pretrain_gather(store.tables, store._order, 0, 4, out)
    with pytest.raises(ValueError, match="O=5 F=8 T=7 K=3"):
        store.fill(dict(out, label_ids=torch.zeros(4, 2, dtype=torch.int64)), 0, 4)


@pytest.mark.parametrize("O,F,T,K", [(36, 64, 20, 3), (5, 8, 7, 1)])
def test_host_gather_without_a_swap_is_collate_examples(O, F, T, K):
    """field by field against ``collate_examples`` on the same ``InputExample``s: images shared by several sentences, a
    sentence longer than T - 2, label dicts with 0, 1 and K keys in insertion order"""
    from xggm_amd.pretrain.lxmert_pretrain import collate_examples
    from xggm_amd.pretrain.resident import gather_pretrain_host, pretrain_tables
    ex, tk = make_examples(O, F, K, T), tok()
    tables = pretrain_tables(ex, tk, T, K, n_answers=29)
    assert tables["feats"].shape == (N_IMG, O, F) and tables["q_row"].tolist() != sorted(tables["q_row"].tolist())
    first = {}
    for q, i in enumerate(IMG_OF):
        first.setdefault(i, len(first))
    assert tables["q_row"].tolist() == [first[i] for i in IMG_OF]  # rows in order of first appearance
    assert tables["q_len"][0] == T and tables["q_len"][1] == 2 and len(tk.tokenize(ex[0].sent)) > T - 2
    used = (tables["q_label"] >= 0).sum(1).tolist()
    assert {0, 1, K} <= set(used) and tables["uids"] == [e.uid for e in ex]
    if K > 1:
        assert tables["q_label"][0].tolist() == sorted(tables["q_label"][0].tolist(), reverse=True)  # insertion order kept
    idx = [12, 0, 3, 3, 1, 7, 0]
    got = gather_pretrain_host(tables, idx, out_f32=True)
    want = collate_examples([ex[i] for i in idx], tk, T, K)
    for k, v in want.items():
        if k == "img_ids":  # collate hashes the image id, the store numbers its rows: the same partition of the batch
            g, w = got[k].tolist(), v.tolist()
            assert [[a == b for b in g] for a in g] == [[a == b for b in w] for a in w]
            continue
        assert got[k].dtype == v.dtype and torch.equal(got[k], v), k
    assert got["sample"].tolist() == idx and got["swapped_from"].tolist() == [-1] * 7 and int(got["exhausted"]) == 0
    bf = gather_pretrain_host(tables, idx)["feats"]
    assert bf.dtype == torch.bfloat16 and torch.equal(bf, want["feats"].to(torch.bfloat16))
    tb16 = pretrain_tables(ex, tk, T, K, feats_bf16=True)
    assert tb16["feats"].dtype == np.uint16
    assert torch.equal(gather_pretrain_host(tb16, idx)["feats"], bf)
    assert torch.equal(gather_pretrain_host(tb16, idx, out_f32=True)["feats"], bf.float())


def test_host_swap_decisions_are_the_swap_rule():
    """on the same draws the decisions equal ``swap_rule`` of tests/test_pretrain_swap_cpu.py with the pool = every sample
    and the image key = q_row; the edges: u == rate, the float below it, own image twice then another, the draw nearest 1"""
    from xggm_amd.pretrain.resident import gather_pretrain_host, pretrain_tables
    T, K = 7, 3
    tables = pretrain_tables(make_examples(5, 8, K, T), tok(), T, K)
    q_row = tables["q_row"].astype(np.int64)
    idx = np.array([0, 3, 8, 9, 5, 5, 1], dtype=np.int64)
    B = len(idx)
    rng = np.random.default_rng(5)
    u_swap, u_pick = rng.random(B, dtype=np.float32), rng.random((B, TRIES), dtype=np.float32)
    half, top = np.float32(0.5), np.nextafter(np.float32(1), np.float32(0))
    u_swap[:4] = (half, np.nextafter(half, np.float32(0)), 0.0, 0.0)
    own = [s for s in range(N_Q) if q_row[s] == q_row[idx[2]]]
    other = [s for s in range(N_Q) if q_row[s] != q_row[idx[2]]][0]
    u_pick[2, :3] = [(own[0] + 0.5) / N_Q, (own[1] + 0.5) / N_Q, (other + 0.5) / N_Q]
    u_pick[3, 0] = top
    u_swap[6] = 0.0
    u_pick[6] = (np.array(own[:1] * TRIES) + 0.25) / N_Q if q_row[idx[6]] == q_row[idx[2]] else u_pick[6]
    for rate in (0.5, 0.0, 1.0):
        want_idx, want_m, want_ex = swap_rule(u_swap, u_pick, q_row[idx], q_row, rate=rate)
        got = gather_pretrain_host(tables, idx, draws=dict(u_swap=u_swap, u_pick=u_pick), match_rate=rate)
        m = got["is_matched"].numpy()
        assert m.tolist() == want_m.tolist() and int(got["exhausted"]) == want_ex, rate
        sent = np.where(m == 0, want_idx, idx)  # swap_rule numbers pool rows; an unswapped row keeps its own sample
        assert got["swapped_from"].tolist() == np.where(m == 0, want_idx, -1).tolist()
        assert got["input_ids"].tolist() == tables["q_ids"][sent].tolist()
        assert got["input_mask"].sum(1).tolist() == tables["q_len"][sent].tolist()
        # labels, features and img_ids always belong to the sample itself
        assert got["label_ids"].tolist() == tables["q_label"][idx].tolist() and got["img_ids"].tolist() == q_row[idx].tolist()
        if rate == 0.5:
            assert m[0] == 1 and m[1] == 0 and got["swapped_from"][2] == other and got["swapped_from"][3] == N_Q - 1
    # a store of one image: every row that tries stays matched and is counted
    one = pretrain_tables(make_examples(5, 8, K, T, n_img=1, img_of=[0] * 4), tok(), T, K)
    got = gather_pretrain_host(one, [0, 1, 2, 3], draws=dict(u_swap=np.float32([0.1, 0.9, 0.2, 0.49]), u_pick=u_pick[:4]), match_rate=0.5)
    assert got["is_matched"].tolist() == [1] * 4 and int(got["exhausted"]) == 3


def test_validation_errors_name_the_example():
    from xggm_amd.pretrain.lxmert_pretrain import InputExample
    from xggm_amd.pretrain.resident import ResidentPretrainSet, pretrain_tables
    T, K, tk = 7, 3, tok()
    ex = make_examples(5, 8, K, T)
    relabel = lambda e, lab: InputExample(e.uid, e.sent, e.visual_feats, e.obj_labels, e.attr_labels, 1, lab)
    with pytest.raises(ValueError, match=r"img3_vqa_004.*label 29 outside"):
        pretrain_tables(ex[:4] + [relabel(ex[4], {29: 1.0})] + ex[5:], tk, T, K, n_answers=29)
    with pytest.raises(ValueError, match=r"img3_vqa_004.*label -1 outside"):
        pretrain_tables(ex[:4] + [relabel(ex[4], {-1: 1.0})] + ex[5:], tk, T, K)
    with pytest.raises(ValueError, match=r"img3_vqa_004.*4 answer keys"):
        pretrain_tables(ex[:4] + [relabel(ex[4], {1: .1, 2: .2, 3: .3, 4: .4})] + ex[5:], tk, T, K)
    odd = make_examples(4, 8, K, T)[6]  # image 4, first seen at sample 6, with another object count
    with pytest.raises(ValueError, match=r"img4_vqa_006.*O=5 F=8"):
        pretrain_tables(ex[:6] + [odd] + ex[7:], tk, T, K)
    short = InputExample(ex[6].uid, ex[6].sent, ex[6].visual_feats, (ex[6].obj_labels[0][:3], ex[6].obj_labels[1]), ex[6].attr_labels, 1, None)
    with pytest.raises(ValueError, match=r"img4_vqa_006"):
        pretrain_tables(ex[:6] + [short] + ex[7:], tk, T, K)
    with pytest.raises(ValueError, match=r"img0_vqa_000.*feat_dim 12"):
        pretrain_tables(make_examples(5, 12, K, T), tk, T, K)
    with pytest.raises(ValueError, match=r"token id outside \[0, 10\)"):
        pretrain_tables(ex, tk, T, K, vocab_size=10)
    tables = pretrain_tables(ex, tk, T, K)
    with pytest.raises(ValueError, match=r"needs \d+ bytes on the device, the limit is 1000"):
        ResidentPretrainSet(tables, "cpu", max_bytes=1000)
    with pytest.raises(ValueError, match="q_row outside"):
        ResidentPretrainSet(dict(tables, q_row=tables["q_row"] + 1), "cpu")
    with pytest.raises(ValueError, match="match_rate"):
        ResidentPretrainSet(tables, "cpu", match_rate=1.5)
    from xggm_amd import param
    assert ResidentPretrainSet.from_args(param.parse_args(["--taskMatched"]), tables, "cpu").match_rate == 0.5
    assert ResidentPretrainSet.from_args(param.parse_args([]), tables, "cpu").match_rate is None


def test_order_is_the_resident_datasets_order(tmp_path):
    from test_resident_cpu import _store, _ts
    from xggm_amd.pretrain.resident import ResidentPretrainSet, pretrain_tables
    ref = _store(_ts(tmp_path))
    n = len(ref)
    img_of = [q % 5 for q in range(n)]
    mine = ResidentPretrainSet(pretrain_tables(make_examples(5, 8, 3, 7, n_img=5, img_of=img_of), tok(), 7, 3), "cpu")
    assert len(mine) == n and mine.feat_pool().shape == (5 * 5, 8)
    assert mine.feat_pool().data_ptr() == mine.tables["feats"].data_ptr()  # a view, not a copy
    for kw in (dict(epoch=0), dict(epoch=3, seed=7), dict(epoch=1, shuffle=False, drop_last=False), dict(epoch=2, batch_size=4),
               dict(epoch=2, batch_size=4, drop_last=False), dict(epoch=1, seed=2, rank=1, world=2, batch_size=2)):
        a, b = ref.order(**kw), mine.order(**kw)
        assert a.tolist() == b.tolist(), kw
        assert mine._order.tolist() == b.tolist()
    for kw in (dict(epoch=0, world=2), dict(epoch=0, rank=2, world=2, batch_size=2), dict(epoch=0, batch_size=n + 1)):
        with pytest.raises(ValueError):
            mine.order(**kw)
    ids, mask, img = mine.sent_pool()
    assert ids.dtype == mask.dtype == img.dtype == torch.int64 and img.tolist() == mine.host["q_row"].tolist()
    assert mask.sum(1).tolist() == mine.host["q_len"].tolist() and ids.tolist() == mine.host["q_ids"].tolist()
    assert mine.uids([2, 0]) == ["img2_vqa_002", "img0_vqa_000"]
