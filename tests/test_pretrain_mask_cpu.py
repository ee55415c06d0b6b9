"""Pre-training batch masking, the parts that need no GPU: the float64 restatement (tests/pretrain_mask_ref.py) against what
the reference's own random_word / random_feat / convert_example_to_features returned on recorded draws
(tests/golden/pretrain_mask.npz, generator tests/golden/make_pretrain_mask_golden.py), ``pack_labels``, the two parser
flags, the header's declarations and the entry points' validation before any launch."""
import ctypes
import re

import numpy as np
import pytest

import pretrain_mask_ref as R
from helpers import load_golden

OUT = ("input_ids", "masked_lm_labels", "masked_feat", "feat_mask", "ans")
DRAWS = ("u_word", "u_word_pick", "u_obj", "u_obj_pick", "u_ans")


def golden_case(g, c):
    B, T, O, F, P, K, V, mask_id = (int(v) for v in g["cfg"])
    d = {k: g["b%d.%s" % (c, k)] for k in DRAWS}
    args = (g["input_ids"], g["input_mask"], g["feats"], g["b%d.is_matched" % c], g["b%d.label_ids" % c], g["b%d.label_scores" % c], d)
    kw = dict(word_mask_rate=float(g["rates"][0]), obj_mask_rate=float(g["rates"][1]), vocab_size=V, mask_id=mask_id, pool=g["pool"])
    return args, kw, {k: g["b%d.out.%s" % (c, k)] for k in OUT}


@pytest.mark.parametrize("c", [0, 1])
def test_restatement_reproduces_the_reference(c):
    g = load_golden("pretrain_mask")
    args, kw, want = golden_case(g, c)
    got = R.corrupt(*args, **kw)
    for k in OUT:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert got[k].tobytes() == want[k].tobytes(), k  # integers equal, features bit-equal
    # the fixture is what its generator promises: every outcome in each batch, nothing on [CLS] / [SEP] / padding
    assert set(got["word_kind"][got["word_kind"] >= 0].tolist()) == {0, 1, 2, 3}
    assert set(got["obj_kind"].reshape(-1).tolist()) == {0, 1, 2, 3}
    mask = g["input_mask"]
    L = mask.sum(1)
    assert sorted(L.tolist()) == [2, 3, mask.shape[1]]
    for b in range(mask.shape[0]):
        assert (want["masked_lm_labels"][b, [0, L[b] - 1]] == -1).all() and (want["masked_lm_labels"][b, L[b]:] == -1).all()
        assert (want["input_ids"][b, L[b] - 1:] == g["input_ids"][b, L[b] - 1:]).all()


def test_golden_draws_sit_on_the_thresholds():
    g = load_golden("pretrain_mask")
    V, P = int(g["cfg"][6]), int(g["cfg"][4])
    top = np.nextafter(np.float32(1), np.float32(0))
    for name, rate in (("b0.u_word", float(g["rates"][0])), ("b0.u_obj", float(g["rates"][1]))):
        u = set(g[name].reshape(-1).tolist())
        assert 0.0 in u
        for th in (0.8, 0.9):
            lo, hi = R.fp32_edges(lambda x: x / rate < th, th * rate)
            assert float(lo) in u and float(hi) in u, (name, th)
        lo, hi = R.fp32_edges(lambda x: x < rate, rate)
        assert float(lo) in u and float(hi) in u and float(lo) < rate <= float(hi)
    assert (g["b0.u_word_pick"] == top).any() and (g["b0.u_obj_pick"] == top).any() and g["b1.u_ans"][2] == top
    assert (g["b0.out.input_ids"] == V - 1).any()
    assert any((row == g["pool"][P - 1]).all() for row in g["b0.out.masked_feat"].reshape(-1, g["pool"].shape[1]))
    # the four answer cases: several keys, one key, no label | unmatched with a label, (empty), several keys
    assert g["b0.out.ans"].tolist() == [7, 5, -1] and g["b1.out.ans"].tolist() == [-1, -1, 9]
    assert g["b1.is_matched"][0] == 0 and g["b1.label_ids"][0, 0] >= 0


def test_answer_draw_is_the_inverse_cdf():
    ids = np.array([[3, -1, 7, 11]], dtype=np.int64)
    sc = np.array([[0.25, 9.0, 0.25, 0.5]], dtype=np.float32)
    z = dict(u_word=np.zeros((1, 2), np.float32), u_word_pick=np.zeros((1, 2), np.float32), u_obj=np.ones((1, 1), np.float32),
             u_obj_pick=np.zeros((1, 1), np.float32))
    base = (np.zeros((1, 2), np.int64), np.zeros((1, 2), np.int64), np.zeros((1, 1, 2), np.float32), np.ones(1, np.int64), ids, sc)
    for u, want in ((0.0, 3), (0.2499, 3), (0.25, 7), (0.4999, 7), (0.5, 11), (0.99999, 11)):
        got = R.corrupt(*base, dict(z, u_ans=np.array([u], np.float32)))
        assert got["ans"].tolist() == [want], u


def test_pack_labels():
    import torch
    from xggm_amd.pretrain.lxmert_pretrain import pack_labels
    ids, sc = pack_labels([{3: 0.3, 7: 0.6, 11: 1.0}, {5: 1.0}, None, {}], 3)
    assert ids.dtype == torch.int64 and sc.dtype == torch.float32 and tuple(ids.shape) == (4, 3)
    assert ids.tolist() == [[3, 7, 11], [5, -1, -1], [-1, -1, -1], [-1, -1, -1]]
    assert sc[0].tolist() == [float(np.float32(0.3)), float(np.float32(0.6)), 1.0] and sc[1:].sum() == 1.0
    ids, _ = pack_labels([{9: 1.0, 2: 0.5}], 4)  # insertion order, not sorted
    assert ids.tolist() == [[9, 2, -1, -1]]
    with pytest.raises(ValueError, match="3 answer keys"):
        pack_labels([{1: 1.0, 2: 1.0, 3: 1.0}], 2)
    with pytest.raises(ValueError):
        pack_labels([{-1: 1.0}], 2)
    with pytest.raises(ValueError):
        pack_labels([], 0)


def test_mask_rate_flags():
    from xggm_amd import param
    a = param.parse_args([])
    assert a.word_mask_rate == 0.15 and a.obj_mask_rate == 0.15  # src/param.py:102-105
    a = param.parse_args(["--wordMaskRate", "0.2", "--objMaskRate", "0.05"])
    assert a.word_mask_rate == 0.2 and a.obj_mask_rate == 0.05
    from xggm_amd.pretrain.lxmert_pretrain import DeviceFeatures
    f = DeviceFeatures.from_args(a, vocab_size=81, mask_id=4)
    assert (f.word_mask_rate, f.obj_mask_rate, f.vocab_size, f.mask_id) == (0.2, 0.05, 81, 4)
    param.parse_args([])


def test_header_declares_the_new_symbols():
    from xggm_amd import _lib, ops
    decl = _lib.parse_header()
    for name in ("xggm_pretrain_corrupt_f32", "xggm_pretrain_corrupt_bf16", "xggm_uniform"):
        assert name in decl and hasattr(_lib.lib, name), name
    assert len(decl["xggm_uniform"]) == 5
    src = open(_lib.HEADER_PATH).read()
    for cite in ("src/pretrain/lxmert_pretrain.py:76-215", ":76-112", ":115-136", ":186-199"):
        assert cite in src, cite
    # the ctypes mirror has the header's fields in the header's order
    body = re.search(r"typedef struct xggm_pretrain_corrupt_args \{(.*?)\} xggm_pretrain_corrupt_args;", src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", " ", body, flags=re.S)
    names = [n.strip(" *") for stmt in body.split(";") if stmt.strip() for n in stmt.split(",")]
    names = [n.split()[-1].strip("*") for n in names]
    assert names == [f[0] for f in ops.PretrainCorruptArgs._fields_]
    assert ctypes.sizeof(ops.PretrainCorruptArgs) == 12 * 8 + 5 * 4 + 4 + 3 * 8 + 2 * 8 + 6 * 8 + 8
    assert ops.PRETRAIN_DRAWS == DRAWS


def _fake_args(ops):
    """every pointer a distinct, never dereferenced address: validation runs before any launch"""
    a = ops.PretrainCorruptArgs()
    a.B, a.T, a.O, a.F, a.K = 2, 4, 3, 8, 2
    a.vocab_size, a.mask_id, a.word_mask_rate, a.obj_mask_rate = 81, 4, 0.15, 0.15
    for i, (name, tp) in enumerate(ops.PretrainCorruptArgs._fields_):
        if tp is ctypes.c_void_p and name != "pool":
            setattr(a, name, 0x10000 * (i + 1))
    return a


def test_validation_fails_before_launch():
    from xggm_amd import _lib, ops
    L = _lib.lib
    for fn in (L.xggm_pretrain_corrupt_f32, L.xggm_pretrain_corrupt_bf16):
        assert fn(None, None) != 0 and b"null argument struct" in L.xggm_last_error()
        a = _fake_args(ops)
        a.B = 0
        assert fn(ctypes.addressof(a), None) != 0 and b"B=0" in L.xggm_last_error()
        for name in ("feats", "masked_feat", "feat_mask", "input_ids", "input_mask", "input_ids_out", "masked_lm_labels",
                     "label_ids", "label_scores", "is_matched", "ans"):
            a = _fake_args(ops)
            setattr(a, name, None)
            assert fn(ctypes.addressof(a), None) != 0 and b"null" in L.xggm_last_error(), name
        a = _fake_args(ops)
        a.masked_feat = a.feats  # in place
        assert fn(ctypes.addressof(a), None) != 0 and b"aliases feats" in L.xggm_last_error()
        a = _fake_args(ops)
        a.masked_feat = a.feats + 2 * 3 * 8 * 2 - 2  # the last element of feats, for either element size
        assert fn(ctypes.addressof(a), None) != 0 and b"aliases feats" in L.xggm_last_error()
        a = _fake_args(ops)
        a.pool, a.P = a.masked_feat + 16, 5
        assert fn(ctypes.addressof(a), None) != 0 and b"aliases pool" in L.xggm_last_error()
        a = _fake_args(ops)
        a.u_ans, a.rng = None, None
        assert fn(ctypes.addressof(a), None) != 0 and b"needs rng" in L.xggm_last_error()
        a = _fake_args(ops)
        a.obj_mask_rate = 1.5
        assert fn(ctypes.addressof(a), None) != 0 and b"rates" in L.xggm_last_error()
        a = _fake_args(ops)
        a.vocab_size = 0
        assert fn(ctypes.addressof(a), None) != 0 and b"vocab_size" in L.xggm_last_error()
    assert L.xggm_uniform(None, 4, None, 0, None) != 0 and b"xggm_uniform" in L.xggm_last_error()
    assert L.xggm_uniform(0x10000, 0, 0x20000, 0, None) != 0


def test_wrappers_refuse_cpu_tensors():
    import torch
    from xggm_amd import ops
    from xggm_amd.pretrain.lxmert_pretrain import DeviceFeatures, pack_labels
    ids = torch.zeros(2, 4, dtype=torch.int64)
    lab, sc = pack_labels([None, None], 2)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.pretrain_corrupt(ids, ids, torch.zeros(2, 3, 8), torch.ones(2, dtype=torch.int64), lab, sc, 0.15, 0.15, 81, 4,
                             rng=torch.zeros(2, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="GPU"):
        ops.uniform(4, torch.zeros(2, dtype=torch.int64), 0)
    with pytest.raises(ValueError, match="pack_labels"):
        DeviceFeatures(max_labels=3)(ids, ids, ids, torch.zeros(2, 3, 8), None, None, None, None, None,
                                     torch.ones(2, dtype=torch.int64), lab, sc, None)
