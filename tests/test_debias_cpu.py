"""The debias answer losses without a GPU: ABI, argument refusal before any launch, the reference's class contract
(names, constructor defaults, ``to_json()``, ``state_dict`` keys -- recorded from the reference's own classes by
tests/golden/make_debias_golden.py), ``answer_prior_table`` and the golden file's contents."""
import ctypes
import inspect
import json

import numpy as np
import pytest

from helpers import load_golden

SYMBOLS = ["xggm_debias_fwd_f32", "xggm_debias_fwd_bf16", "xggm_debias_bwd_f32", "xggm_debias_bwd_bf16"]


def test_header_declares_and_library_exports_the_debias_entry_points():
    from xggm_amd import _lib, ops
    decl = _lib.parse_header()
    src = open(_lib.HEADER_PATH).read()
    for s in SYMBOLS:
        assert s in decl and decl[s] == [ctypes.c_void_p, ctypes.c_void_p], s
        assert getattr(_lib.lib, s) is not None
    assert "src/module/vqa_debias_loss_functions.py:84-207" in src and "typedef struct xggm_debias_args" in src
    for name, val in (("XGGM_DEBIAS_REWEIGHT", ops.DEBIAS_REWEIGHT), ("XGGM_DEBIAS_BIAS_PRODUCT", ops.DEBIAS_BIAS_PRODUCT),
                      ("XGGM_DEBIAS_LEARNED_MIXIN", ops.DEBIAS_LEARNED_MIXIN)):
        assert "#define %s %d\n" % (name, val) in src
    assert len({ops.DEBIAS_REWEIGHT, ops.DEBIAS_BIAS_PRODUCT, ops.DEBIAS_LEARNED_MIXIN}) == 3


def _args(**kw):
    """arguments that would pass (host memory the library must never touch: every case below is refused first)"""
    from xggm_amd import ops
    keep = [(ctypes.c_float * 64)() for _ in range(8)]
    a = ops.DebiasArgs()
    a.logits, a.labels, a.bias, a.hidden, a.lin_w, a.lin_b, a.loss, a.save = (ctypes.addressof(k) for k in keep)
    a.ws = a.d_logit = a.part = ctypes.addressof(keep[0])
    a.bias_row_stride, a.bias_rows, a.Hd, a.kind, a.B, a.A = 4, 2, 8, ops.DEBIAS_LEARNED_MIXIN, 2, 4
    for k, v in kw.items():
        setattr(a, k, v)
    a._keep = keep
    return a


@pytest.mark.parametrize("bad,word", [(dict(kind=0), "kind"), (dict(kind=4), "kind"), (dict(A=0), "shape"), (dict(A=-3), "shape"),
                                      (dict(B=0), "shape"), (dict(logits=None), "logits"), (dict(hidden=None), "hidden"),
                                      (dict(Hd=0), "hidden"), (dict(lin_w=None), "hidden"), (dict(bias_rows=1), "bias_index"),
                                      (dict(bias_row_stride=3), "stride"), (dict(save=None), "save")])
@pytest.mark.parametrize("fn", SYMBOLS)
def test_bad_arguments_are_refused_before_any_launch(fn, bad, word):
    from xggm_amd import _lib
    a = _args(**bad)
    assert getattr(_lib.lib, fn)(ctypes.addressof(a), None) != 0
    assert word in _lib.last_error(), _lib.last_error()


def test_null_struct_and_missing_outputs_are_refused():
    from xggm_amd import _lib, ops
    for fn in SYMBOLS:
        assert getattr(_lib.lib, fn)(None, None) != 0
    assert _lib.lib.xggm_debias_fwd_f32(ctypes.addressof(_args(loss=None)), None) != 0
    assert _lib.lib.xggm_debias_fwd_f32(ctypes.addressof(_args(ws=None)), None) != 0
    assert _lib.lib.xggm_debias_bwd_f32(ctypes.addressof(_args(d_logit=None)), None) != 0
    one = (ctypes.c_float * 8)()
    # parameter gradients without the scratch; a smoothing gradient without the parameter; bias_lin for a kind without it
    assert _lib.lib.xggm_debias_bwd_f32(ctypes.addressof(_args(d_lin_w=ctypes.addressof(one), d_lin_b=ctypes.addressof(one),
                                                               part=None)), None) != 0
    assert _lib.lib.xggm_debias_bwd_f32(ctypes.addressof(_args(d_smooth=ctypes.addressof(one))), None) != 0
    assert _lib.lib.xggm_debias_bwd_f32(ctypes.addressof(_args(kind=ops.DEBIAS_BIAS_PRODUCT, d_lin_w=ctypes.addressof(one),
                                                               d_lin_b=ctypes.addressof(one))), None) != 0
    assert _lib.lib.xggm_debias_fwd_f32(ctypes.addressof(_args(kind=ops.DEBIAS_REWEIGHT, smooth_param=ctypes.addressof(one))),
                                        None) != 0


def _contract():
    return json.loads(str(load_golden("debias")["meta_json"]))["contract"]


def test_classes_keep_the_reference_contract():
    from xggm_amd.module import vqa_debias_loss_functions as D
    want = _contract()
    assert sorted(want) == ["BiasProduct", "LearnedMixin", "Plain", "ReweightByInvBias"]
    assert issubclass(D.DebiasLossFn, __import__("torch").nn.Module)
    for cls, c in want.items():
        k = getattr(D, cls)
        assert [b.__name__ for b in k.__mro__[1:2]] == c["base"] == ["DebiasLossFn"]
        named = [(n, p) for n, p in inspect.signature(k).parameters.items() if p.kind == p.POSITIONAL_OR_KEYWORD]
        pos = [n for n, p in named if p.default is p.empty]
        dfl = [[n, p.default] for n, p in named if p.default is not p.empty]
        assert pos == c["positional"] and dfl == c["defaults"], cls
        m = k(*([0.36] if c["positional"] else []))
        assert [list(kv) for kv in m.to_json().items()] == c["to_json"], cls
        assert list(m.state_dict().keys()) == c["state_dict"], cls
    # the one addition: LearnedMixin's keyword-only width (the reference hard-codes 1024)
    extra = {n: p for n, p in inspect.signature(D.LearnedMixin).parameters.items() if p.kind == p.KEYWORD_ONLY}
    assert list(extra) == ["hidden_dim"] and extra["hidden_dim"].default == 1024
    assert D.LearnedMixin(0.36).bias_lin.in_features == 1024 and D.LearnedMixin(0.36, hidden_dim=768).bias_lin.in_features == 768
    m = D.LearnedMixin(0.2, False, -2, 0.1, hidden_dim=16)
    assert m.smooth_param is None and list(m.state_dict()) == ["bias_lin.weight", "bias_lin.bias"]
    assert dict(m.to_json()) == dict(name="LearnedMixin", w=0.2, smooth=False, smooth_init=-2, constant_smooth=0.1)
    assert float(D.BiasProduct(smooth_init=-3).smooth_param.detach()) == -3.0
    # the prior table is a buffer: saved with the module
    m.set_bias_table(np.zeros((4, 5), np.float32))
    assert "bias_table" in m.state_dict() and tuple(m.bias_table.shape) == (4, 5)
    assert not hasattr(D, "Focal")


def test_answer_prior_table_matches_a_hand_example():
    from xggm_amd.vqa.vqacpv2 import answer_prior_table
    from xggm_amd.gqa import gqa_ood
    assert gqa_ood.answer_prior_table is answer_prior_table
    targets = np.array([[1.0, 0.0, 0.3], [0.0, 0.6, 0.3], [0.0, 1.0, 0.0], [0.9, 0.0, 0.0]], np.float32)
    t = answer_prior_table(targets, [0, 0, 2, 0], 4)
    assert t.dtype == np.float32 and t.shape == (4, 3)
    want = np.array([[1.9 / 3, 0.2, 0.2], [0, 0, 0], [0, 1, 0], [0, 0, 0]], np.float64)
    assert np.allclose(t, want, rtol=0, atol=1e-7)
    with pytest.raises(ValueError):
        answer_prior_table(targets, [0, 0, 4, 0], 4)
    with pytest.raises(ValueError):
        answer_prior_table(targets, [0, 0], 4)


CASES = dict(a=("LearnedMixin", 3, 3129, 768), b=("LearnedMixin", 1, 1, 1024), c=("LearnedMixin", 5, 1842, 768),
             d=("LearnedMixin", 33, 3129, 768), e=("BiasProduct", 3, 3129, 0), f=("BiasProduct", 2, 5, 0),
             g=("ReweightByInvBias", 3, 3129, 0), h=("ReweightByInvBias", 2, 7, 0))


def test_golden_file_holds_every_case():
    g = load_golden("debias")
    meta = json.loads(str(g["meta_json"]))
    assert sorted(meta["cases"]) == sorted(CASES) and meta["stride"] == 97
    for name, (kind, B, A, Hd) in CASES.items():
        c = meta["cases"][name]
        assert (c["kind"], c["B"], c["A"], c["Hd"]) == (kind, B, A, Hd), name
        assert c["bf16"] == (name in "acd") and c["whole"] == (name not in "ad")
        assert c["bias_max"] == (0.99 if name in "gh" else None)
        for tag in [name] + ([name + ".bf16"] if c["bf16"] else []):
            assert np.isfinite(g[tag + ".loss"])
            if c["whole"]:
                assert g[tag + ".d_logit"].shape == (B, A)
            else:
                assert g[tag + ".d_logit_every97"].shape == ((B * A + 96) // 97,)
                assert g[tag + ".d_logit_rowsum"].shape == (B,) and g[tag + ".d_logit_rowabs"].shape == (B,)
            if Hd:
                assert g[tag + ".d_hidden"].shape == (B, Hd) and g[tag + ".d_lin_w"].shape == (1, Hd)
                assert g[tag + ".d_lin_b"].shape == (1,) and g[tag + ".d_lin_b_abs"] >= abs(g[tag + ".d_lin_b"][0]) * (1 - 1e-12)
            has_smooth = kind != "ReweightByInvBias" and c["kwargs"].get("smooth", True)
            assert ((tag + ".d_smooth") in g.files) == has_smooth
            if has_smooth:
                assert g[tag + ".d_smooth_abs"] >= abs(g[tag + ".d_smooth"][0]) * (1 - 1e-12)
    assert meta["cases"]["a"]["kwargs"] == dict(w=0.36)
    assert meta["cases"]["c"]["kwargs"] == dict(w=0.36, smooth=False, constant_smooth=0.1)
    assert meta["cases"]["f"]["kwargs"] == dict(smooth=False, constant_smooth=0.05)


def test_case_inputs_are_what_the_issue_describes():
    from xggm_amd import synth
    x = synth.debias_case(3, 3129, 768, 11)
    assert all(v.dtype == np.float32 for v in x.values())
    assert (np.abs(x["logits"]) == 30).sum() >= 4 and (x["logits"] == 30).any() and (x["logits"] == -30).any()
    nz = x["labels"] > 0
    assert 0.005 < nz.mean() < 0.02 and x["labels"].max() <= 1 and x["labels"][nz].min() > 0
    assert (x["bias"] == 0).any() and (x["bias"] == 1).any() and x["bias"].min() >= 0 and x["bias"].max() <= 1
    y = synth.debias_case(3, 3129, 0, 17, 0.99)
    assert y["bias"].max() == np.float32(0.99) and (y["bias"] == 0).any() and "hidden" not in y
    assert np.array_equal(synth.debias_case(3, 3129, 768, 11)["hidden"], x["hidden"])
