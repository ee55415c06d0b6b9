"""The softmax answer losses (Focal, --mceLoss cross-entropy) without a GPU: ABI, argument refusal before any launch, the
reference's ``Focal`` contract (recorded from the reference's own class by tests/golden/make_softmax_loss_golden.py),
``CrossEntropy`` defaults, the flag and the golden file's contents."""
import ctypes
import inspect
import json

import numpy as np
import pytest

from helpers import load_golden

SYMBOLS = ["xggm_softmax_loss_fwd_f32", "xggm_softmax_loss_bwd_f32"]
FWD, BWD = SYMBOLS


def test_header_declares_and_library_exports_the_entry_points():
    from xggm_amd import _lib, ops
    decl = _lib.parse_header()
    src = open(_lib.HEADER_PATH).read()
    for s in SYMBOLS:
        assert s in decl and decl[s] == [ctypes.c_void_p, ctypes.c_void_p], s
        assert getattr(_lib.lib, s) is not None
    assert "xggm_softmax_loss_fwd_bf16" not in decl  # logits and d_logit are fp32 under every compute dtype
    assert "src/module/vqa_debias_loss_functions.py:74-81" in src and "typedef struct xggm_softmax_loss_args" in src
    for name, val in (("XGGM_SOFTMAX_FOCAL", ops.SOFTMAX_FOCAL), ("XGGM_SOFTMAX_CE", ops.SOFTMAX_CE)):
        assert "#define %s %d\n" % (name, val) in src
    assert ops.SOFTMAX_FOCAL != ops.SOFTMAX_CE


def test_the_ctypes_mirror_follows_the_header_field_by_field():
    import re
    from xggm_amd import _lib, ops
    src = open(_lib.HEADER_PATH).read()
    body = src[src.index("typedef struct xggm_softmax_loss_args {"):src.index("} xggm_softmax_loss_args;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S).split("{", 1)[1]
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        pointer = "*" in decl
        base = decl.replace("const", "").replace("*", " ").split()[0]
        for name in decl.replace("*", " ").split(base, 1)[1].split(","):
            ct = ctypes.c_void_p if pointer else dict(int64_t=ctypes.c_int64, float=ctypes.c_float, int=ctypes.c_int)[base]
            fields.append((name.strip(), ct))
    assert fields == list(ops.SoftmaxLossArgs._fields_)


def _args(**kw):
    """arguments that would pass (host memory the library must never touch: every case below is refused first)"""
    from xggm_amd import ops
    keep = [(ctypes.c_float * 64)() for _ in range(8)]
    a = ops.SoftmaxLossArgs()
    a.logits, a.labels, a.bias, a.loss, a.ws, a.save, a.gout, a.d_logit = (ctypes.addressof(k) for k in keep)
    a.bias_row_stride, a.bias_rows, a.kind, a.B, a.A, a.ignore_index, a.scale = 4, 2, ops.SOFTMAX_FOCAL, 2, 4, -1, 1.0
    for k, v in kw.items():
        setattr(a, k, v)
    a._keep = keep
    return a


def _refused(fn, word, **bad):
    from xggm_amd import _lib
    a = _args(**bad)
    assert getattr(_lib.lib, fn)(ctypes.addressof(a), None) != 0, (fn, bad)
    assert word in _lib.last_error(), (fn, bad, _lib.last_error())


@pytest.mark.parametrize("bad,word", [(dict(kind=0), "unknown kind"), (dict(kind=3), "unknown kind"), (dict(A=0), "bad shape"),
                                      (dict(A=-3), "bad shape"), (dict(B=0), "bad shape"), (dict(logits=None), "logits is required"),
                                      (dict(labels=None), "needs labels"), (dict(bias=None), "needs bias"),
                                      (dict(bias_rows=1), "needs bias_index"), (dict(bias_row_stride=3), "row stride"),
                                      (dict(save=None), "save buffer"),
                                      (dict(kind=2, labels=None), "labels or label_index"),
                                      (dict(kind=2, A=0), "bad shape"), (dict(kind=2, logits=None), "logits is required"),
                                      (dict(kind=2, save=None), "save buffer")])
@pytest.mark.parametrize("fn", SYMBOLS)
def test_bad_arguments_are_refused_before_any_launch(fn, bad, word):
    _refused(fn, word, **bad)


def test_null_struct_and_missing_outputs_are_refused():
    from xggm_amd import _lib
    for fn in SYMBOLS:
        assert getattr(_lib.lib, fn)(None, None) != 0
        assert "null arguments" in _lib.last_error()
    for kind in (1, 2):
        _refused(FWD, "loss slot", kind=kind, loss=None)
        _refused(FWD, "workspace ws", kind=kind, ws=None)
        _refused(BWD, "d_logit is required", kind=kind, d_logit=None)
        _refused(BWD, "gout", kind=kind, gout=None)


def _meta():
    return json.loads(str(load_golden("softmax_loss")["meta_json"]))


def test_focal_keeps_the_reference_contract():
    import torch
    from xggm_amd import ops
    from xggm_amd.module import answer_losses as D
    from xggm_amd.module.vqa_debias_loss_functions import DebiasLossFn
    c = _meta()["contract"]
    assert sorted(c) == ["Focal"]
    c = c["Focal"]
    k = D.Focal
    assert [b.__name__ for b in k.__mro__[1:2]] == c["base"] == ["DebiasLossFn"] and k.__mro__[1] is DebiasLossFn
    named = [(n, p) for n, p in inspect.signature(k).parameters.items() if p.kind == p.POSITIONAL_OR_KEYWORD]
    assert [n for n, p in named if p.default is p.empty] == c["positional"] == []
    assert [[n, p.default] for n, p in named if p.default is not p.empty] == c["defaults"] == []
    m = k()
    assert [list(kv) for kv in m.to_json().items()] == c["to_json"] == [["name", "Focal"]]
    assert list(m.state_dict().keys()) == c["state_dict"] == [] and not list(m.parameters())
    assert m.kind == ops.SOFTMAX_FOCAL and m.needs_bias and not m.needs_hidden
    m.set_bias_table(np.zeros((4, 5), np.float32))  # the prior table is a buffer, as for the other classes
    assert list(m.state_dict()) == ["bias_table"] and tuple(m.bias_table.shape) == (4, 5)
    with pytest.raises(ValueError, match="no bias given"):
        D.Focal()(None, torch.zeros(2, 4), None, torch.zeros(2, 4))
    assert k.__name__ == "Focal" and "vqa_debias_loss_functions.py (:74-81)" in D.__doc__


def test_cross_entropy_defaults_and_the_flag():
    from xggm_amd import ops, param
    from xggm_amd.gqa import gqa_ood
    from xggm_amd.module.answer_losses import CrossEntropy
    from xggm_amd.module.vqa_debias_loss_functions import DebiasLossFn
    from xggm_amd.vqa.vqacpv2 import make_answer_loss
    m = CrossEntropy()
    assert isinstance(m, DebiasLossFn) and m.kind == ops.SOFTMAX_CE and not m.needs_bias and not m.needs_hidden
    assert m.ignore_index == -1 and m.scale == 1.0 and not list(m.parameters()) and not list(m.state_dict())
    assert dict(m.to_json()) == dict(name="CrossEntropy", ignore_index=-1, scale=1.0)
    m = CrossEntropy(-100, 3.5)
    assert (m.ignore_index, m.scale) == (-100, 3.5)
    sig = inspect.signature(CrossEntropy.forward)
    assert list(sig.parameters) == ["self", "hidden", "logits", "bias", "labels", "bias_index", "slot"]
    assert all(sig.parameters[k].kind == inspect.Parameter.KEYWORD_ONLY for k in ("bias_index", "slot"))
    assert param.parse_args([]).mce_loss is False and param.parse_args(["--mceLoss"]).mce_loss is True
    assert make_answer_loss(param.parse_args([])) is None
    got = make_answer_loss(param.parse_args(["--mceLoss"]))
    assert type(got) is CrossEntropy and got.ignore_index == -1 and got.scale == 1.0
    assert gqa_ood.make_answer_loss is make_answer_loss
    param.parse_args([])


CASES = dict(a=(1, 1, None), b=(2, 5, None), c=(3, 263, None), d=(3, 3129, None), e=(5, 1842, None), f=(2, 4097, None),
             g=(130, 64, None), h=(2, 7, "all_ignored"), i=(3, 3129, "label_index"))


def test_golden_file_holds_every_case_of_its_table():
    g = load_golden("softmax_loss")
    meta = _meta()
    assert sorted(meta["cases"]) == sorted(CASES) and meta["ignore_index"] == -1 and meta["gate"] == 1e-5
    for name, (B, A, variant) in CASES.items():
        c = meta["cases"][name]
        assert (c["B"], c["A"], c["variant"]) == (B, A, variant), name
        assert c["kinds"] == (["focal", "ce"] if variant is None else ["ce"])
        for kind in c["kinds"]:
            tag = "%s.%s" % (name, kind)
            assert g[tag + ".d_logit"].shape == (B, A) and g[tag + ".d_logit"].dtype == np.float32
            # the gate of the generator: the reference in float32 against itself in float64
            assert 0 <= c["gate"][kind]["loss"] <= 1e-5 and 0 <= c["gate"][kind]["d_logit"] <= 1e-5, tag
            if variant == "all_ignored":
                assert np.isnan(g[tag + ".loss"]) and not g[tag + ".d_logit"].any()  # what torch did when it was recorded
            else:
                assert np.isfinite(g[tag + ".loss"])
        lab = g[name + ".ce.labels"]
        assert lab.shape == (B,) and lab.dtype == np.int64 and ((lab == -1) | ((lab >= 0) & (lab < A))).all()
        assert not g[name + ".ce.d_logit"][lab == -1].any()
    assert (g["b.ce.labels"] == -1).sum() == 1  # (2, 5): one row without a positive score
    assert (g["h.ce.labels"] == -1).all()
    assert g["i.label_index"][1] == -1 and np.array_equal(g["i.label_index"], g["i.ce.labels"])
    assert (g["i.label_index"][[0, 2]] >= 0).all()
    assert [k for k in g.files if k.endswith(".label_index")] == ["i.label_index"]


def test_case_labels_follow_the_rule_of_the_header():
    """first index of the row maximum of the soft scores, -1 where that maximum is <= 0 (from the seeded inputs alone)"""
    from xggm_amd import synth
    g = load_golden("softmax_loss")
    for name, c in _meta()["cases"].items():
        if c["variant"] is not None:
            continue
        y = synth.debias_case(c["B"], c["A"], 0, c["seed"])["labels"]
        want = np.where(y.max(1) > 0, y.argmax(1), -1)
        assert np.array_equal(g[name + ".ce.labels"], want), name
