"""The attention bound at 65 .. 128 rows, the refusals of the C ABI and of the model classes: host-only.

  * Both arithmetic models of the kernels (attention_cases.Case.emulate: ``mfma`` = bf16 operands P D and dS, ``scalar`` =
    fp32 throughout, bf16 or fp32 store) stay inside the bound of attention_long_cases.LongCase on every long shape, with
    and without dropout, and are not trivially exact.  Largest |err| / bound over out / dq / dk / dv seen here (B = 4,
    two heads, p = 0 and 0.5): 0.89 (mfma), 0.96 (scalar, bf16 store), 0.007 (scalar, fp32 store) -- the range of the 64-row
    cases.
  * Each planted defect of Case.emulate leaves the bound at a long shape, so the matrix of test_attention_long_gpu.py can
    fail at the new sizes.
  * xggm_attn_{fwd,bwd}_grouped_* refuse 129 rows on either side, and a long problem that asks for the e4m3 copy, while
    checking the group -- before the valid problem in front of it could be launched (there is no GPU here: a launch
    would fail with a different message).  The plain entry points keep their 64-row contract.
  * VQAModel / GQAModel / LXRTEncoderFeature / the LXMERT driver refuse max_seq_length = 129, 129 objects and a
    max_seq_length beyond the position table when they are built.
"""
import ctypes

import pytest

from attention_cases import BF16, F32, ids, shifted
from attention_long_cases import LONG_DROPOUT_SHAPES, LONG_SHAPES, LongCase
from helpers import ATTN_D, excess_argmax

B, HEADS = 4, 2  # the mask rows of the GPU test in turn: every key, half the keys, exactly one key, every key
MODELS = {"mfma": ("mfma", BF16), "scalar-bf16": ("scalar", BF16), "scalar-f32": ("scalar", F32)}


@pytest.fixture(scope="module")
def cases():
    """(shape, storage type, p) -> LongCase, built on first use: the fp64 references are shared and never written"""
    made = {}

    def get(shape, dt, p):
        key = (shape, dt, p)
        if key not in made:
            c = LongCase(B, HEADS, shape[0], shape[1], dt, "cpu", masked=True, p=p)
            made[key] = c.host_keep() if p else c
        return made[key]
    return get


@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("model", list(MODELS))
@pytest.mark.parametrize("shape", LONG_SHAPES, ids=ids)
def test_emulated_kernels_stay_inside_the_bound(cases, shape, model, p):
    path, dt = MODELS[model]
    c = cases(shape, dt, p)
    c.reset()
    c.store(c.emulate(path))
    mx = c.check("emulated " + model, path)  # canaries, every element of every output <= 1: nothing is excluded
    print("emulated %s %s: max |err| / bound %s" % (c.name, model, ", ".join("%s %.3f" % kv for kv in sorted(mx.items()))))
    for name in ("out", "dq", "dk", "dv"):
        if shape[1] == 1 and name != "dv":
            # one key: the softmax is the identity, dS = 0 and out = v times a keep-scale of 0, 1 or 2 -- all exact
            assert mx[name] == 0.0, (name, mx[name])
        else:
            assert 0.0 < mx[name] <= 1.0, (name, mx[name])


@pytest.mark.parametrize("model", list(MODELS))
@pytest.mark.parametrize("shape", LONG_DROPOUT_SHAPES, ids=ids)
def test_emulated_kernels_with_light_dropout(cases, shape, model):
    path, dt = MODELS[model]
    c = cases(shape, dt, 0.1)
    c.reset()
    c.store(c.emulate(path))
    mx = c.check("emulated " + model, path)
    assert all(0.0 < mx[name] <= 1.0 for name in ("out", "dq", "dk", "dv")), mx


def test_long_reference_is_the_64_row_reference_up_to_64_keys():
    """attention_long_cases.LongAttnRef repeats the constructor of helpers.AttnRef with one term changed (max(Sk, 64) u for
    64 u).  Where Sk <= 64 the two must give identical references and bound parts, bit for bit, with and without dropout:
    a change to helpers.AttnRef that the copy does not follow fails here."""
    import torch
    from attention_cases import Case
    from helpers import U32
    for shape, p in (((20, 36), 0.0), ((64, 64), 0.5), ((100, 20), 0.1), ((128, 63), 0.0)):
        plain = Case(B, HEADS, shape[0], shape[1], BF16, "cpu", masked=True, p=p, seed=3)
        long_ = LongCase(B, HEADS, shape[0], shape[1], BF16, "cpu", masked=True, p=p, seed=3)
        if p:
            plain.host_keep()
            long_.host_keep()
        Ra, Rb = plain.reference(), long_.reference()
        assert type(Ra) is not type(Rb) and set(Ra.terms) == set(Rb.terms) == {"out", "dq", "dk", "dv"}
        assert torch.equal(Ra.rho, Rb.rho)
        for name in Ra.terms:
            for ta, tb in zip(Ra.terms[name][:3], Rb.terms[name][:3]):
                assert torch.equal(ta, tb), (shape, name)
            assert Ra.terms[name][3] == Rb.terms[name][3]
            for mfma in (False, True):
                for a_, b_ in zip(Ra.bound(name, BF16, mfma), Rb.bound(name, BF16, mfma)):
                    assert torch.equal(a_, b_)
                for a_, b_ in zip(Ra.bias_bound(name, mfma), Rb.bias_bound(name, mfma)):
                    assert torch.equal(a_, b_)
    # past 64 keys only the row-sum term moves: rho grows by (Sk - 64) u
    plain, long_ = (cls(B, HEADS, 20, 100, BF16, "cpu", masked=True, seed=3) for cls in (Case, LongCase))
    d = long_.reference().rho - plain.reference().rho
    assert torch.allclose(d, torch.full_like(d, 36 * U32), rtol=1e-6, atol=0.0)


def cols_of(h):
    return range(h * ATTN_D, (h + 1) * ATTN_D)


def leaves(c, path, name, bad, rows, h, note):
    """the corrupted result leaves the bound of ``name`` and the reported arg-max lies in ``rows`` x the columns of head h"""
    mx, idx = excess_argmax(c.excess(name, bad[name], path))
    print("%s %s: %s, %s: |err| / bound %.1f at %s" % (c.name, path, note, name, mx, idx))
    assert mx > 1.0 and idx[0] in rows and idx[1] in cols_of(h), (note, name, mx, idx)


@pytest.mark.parametrize("path", ["mfma", "scalar"])
@pytest.mark.parametrize("shape", LONG_SHAPES, ids=ids)
def test_planted_defects_leave_the_bound(cases, shape, path):
    """the seven defects of test_attention_edges_cpu.py, each wherever it is defined, at the long shapes"""
    Sq, Sk = shape
    c = cases(shape, BF16, 0.0)
    b0, h0, i0 = at = (0, HEADS - 1, Sq // 2)  # sample 0 sees every key
    good = c.emulate(path)
    for name in ("out", "dq", "dk", "dv", "bdq", "bdk", "bdv"):
        assert float(c.excess(name, good[name], path).max()) <= 1.0
    rows_k = range(b0 * Sk, (b0 + 1) * Sk)
    if Sk > 1:
        bad = c.emulate(path, "dropped_key", at)
        for name in ("out", "dq"):
            leaves(c, path, name, bad, [b0 * Sq + i0], h0, "dropped key")
    if Sk % 16:
        # planted in sample 2, which sees one key: the zero-score padding key takes a large share of every row there.  (Among
        # all Sk > 64 random-score keys of sample 0 its share is about 1 / Sk, which the bf16 operands' 2^-8 can hide.)
        bad = c.emulate(path, "padding_key", (2, h0, i0))
        for name in ("out", "dq") if Sk > 1 else ("out",):
            leaves(c, path, name, bad, range(2 * Sq, 3 * Sq), h0, "padding key")
    if Sq % 32:
        bad = c.emulate(path, "padding_query", at)
        for name in ("dk", "dv") if Sk > 1 else ("dv",):
            leaves(c, path, name, bad, rows_k, h0, "padding query row")
    if Sq > 1 and Sk > 1:  # one key: every row of out is that key's value row, a copy shows nothing
        bad = c.emulate(path, "copied_row", at)
        for name in ("out", "dq"):
            leaves(c, path, name, bad, [b0 * Sq + Sq - 1], h0, "copied row")
    if Sk > 1:  # the two mask rows differ
        bad = c.emulate(path, "wrong_mask_row", at)
        for name in ("out", "dq"):
            mx, idx = excess_argmax(c.excess(name, bad[name], path))
            assert mx > 1.0, (name, mx, idx)
    for name, S in (("bdq", Sq), ("bdk", Sk), ("bdv", Sk)):
        # one key: dq = dk = 0, nothing to miss.  A last tile of ONE row (S % 16 == 1) is one term of S in the column sum:
        # the fp32 arithmetic shows its absence, the bf16 operands' share of the matrix-core bound can hide it
        if S > 16 and not (name in ("bdq", "bdk") and Sk == 1) and (path == "scalar" or (S - 1) % 16):
            bad = c.emulate(path, "short_partial", at)
            leaves(c, path, name, bad, [b0], h0, "short bias partial")
    d = cases(shape, BF16, 0.5)
    assert float(d.excess("out", d.emulate(path)["out"], path).max()) <= 1.0
    bad = d.emulate(path, "shifted_keep", at)
    mx, idx = excess_argmax(d.excess("out", bad["out"], path))
    b, i, h = idx[0] // Sq, idx[0] % Sq, idx[1] // ATTN_D
    print("%s %s: shifted keep mask, out: |err| / bound %.1f at %s" % (d.name, path, mx, idx))
    assert mx > 1.0 and bool((shifted(d.keep)[b, h, i] != d.keep[b, h, i]).any()), (mx, idx)


# ---- the C ABI ---------------------------------------------------------------------------------------------------------
FAKE = 0x10000  # a 16-byte aligned address nobody dereferences: validation happens on the host, before any launch


def problem(ops, Sq, Sk, out8=False):
    H = 64
    pr = ops.AttnProblem(FAKE, FAKE, FAKE, None, FAKE, 1, 1, Sq, Sk, H, H, H, H, 0.125, 0.0, 0, FAKE, FAKE, FAKE, FAKE, H, H, H,
                         None, None, None, 0)
    if out8:
        pr.out8 = FAKE
    return pr


@pytest.mark.parametrize("sfx", ["f32", "bf16"])
@pytest.mark.parametrize("kind", ["fwd", "bwd"])
def test_grouped_entries_refuse_more_than_128_rows_before_launch(kind, sfx):
    from xggm_amd import _lib, ops
    L = _lib.lib
    entry = getattr(L, "xggm_attn_%s_grouped_%s" % (kind, sfx))
    for Sq, Sk in ((129, 20), (20, 129), (129, 129)):
        # a valid short problem in front: it is not launched, the whole group is checked first
        arr = (ops.AttnProblem * 2)(problem(ops, 20, 36), problem(ops, Sq, Sk))
        rc = entry(ctypes.cast(arr, ctypes.c_void_p), 2, 64, None, None, None)
        msg = L.xggm_last_error()
        assert rc != 0 and b"128" in msg and (b"Sq=%d Sk=%d" % (Sq, Sk)) in msg, msg


def test_long_problem_with_the_e4m3_copy_is_refused_before_launch():
    from xggm_amd import _lib, ops
    L = _lib.lib
    for Sq, Sk in ((65, 20), (20, 65), (128, 128)):
        arr = (ops.AttnProblem * 2)(problem(ops, 20, 36), problem(ops, Sq, Sk, out8=True))
        rc = L.xggm_attn_fwd_grouped_bf16(ctypes.cast(arr, ctypes.c_void_p), 2, 64, None, None, None)
        msg = L.xggm_last_error()
        assert rc != 0 and b"e4m3" in msg and b"64 rows" in msg, msg


def test_plain_entries_keep_their_64_row_contract():
    from xggm_amd import _lib
    L = _lib.lib
    rc = L.xggm_attn_fwd_bf16(FAKE, FAKE, FAKE, None, FAKE, 1, 1, 100, 100, 64, 64, 64, 64, 64, 0.125, 0.0, None, 0, None)
    assert rc != 0 and b"64-row" in L.xggm_last_error()
    rc = L.xggm_attn_bwd_f32(FAKE, FAKE, FAKE, None, FAKE, FAKE, FAKE, FAKE, 1, 1, 20, 65, 64, 64, 64, 64, 64, 64, 64, 64, 0.125,
                             0.0, None, 0, None, None, None, 0, None)
    assert rc != 0 and b"64-row" in L.xggm_last_error()


# ---- the model classes ---------------------------------------------------------------------------------------------------
def tiny(max_pos):
    from oracle import shapes
    from xggm_amd import param
    from xggm_amd.lxrt.modeling import BertConfig, VISUAL_CONFIG
    cfg = shapes.TINY
    VISUAL_CONFIG.set_visual_dims(cfg["feat_dim"], 4)
    a = param.parse_args(["--llayers", "1", "--xlayers", "1", "--rlayers", "1"])
    bc = BertConfig(cfg["vocab"], hidden_size=cfg["hidden"], num_attention_heads=cfg["heads"], intermediate_size=cfg["inter"],
                    max_position_embeddings=max_pos)
    return a, bc


def test_model_classes_refuse_what_the_attention_core_cannot_run():
    from xggm_amd.gqa.gqa_ood_model import GQAModel
    from xggm_amd.lxrt.entry import LXRTEncoderFeature
    from xggm_amd.lxrt.modeling import LXRTPretraining
    from xggm_amd.pretrain.lxmert_pretrain import LXMERT
    from xggm_amd.vqa.vqacpv2_model import VQAModel
    a, bc = tiny(512)
    for build in (lambda: VQAModel(5, args=a, config=bc, max_seq_length=129), lambda: GQAModel(5, args=a, config=bc, max_seq_length=129),
                  lambda: LXRTEncoderFeature(a, 129, mode="lxr", config=bc), lambda: VQAModel(5, args=a, config=bc, n_objects=129),
                  lambda: LXMERT(129, LXRTPretraining(bc, visual_losses="obj", num_answers=3), None, args=a)):
        with pytest.raises(ValueError, match="128"):
            build()
    a, bc = tiny(64)
    for build in (lambda: VQAModel(5, args=a, config=bc, max_seq_length=72), lambda: GQAModel(5, args=a, config=bc, max_seq_length=72),
                  lambda: LXRTEncoderFeature(a, 65, mode="lxr", config=bc),
                  lambda: LXMERT(72, LXRTPretraining(bc, visual_losses="obj", num_answers=3), None, args=a)):
        with pytest.raises(ValueError, match="position table"):
            build()
    # the new corner itself is accepted
    a, bc = tiny(128)
    m = VQAModel(5, args=a, config=bc, max_seq_length=128, n_objects=100)
    assert m.lxrt_encoder.max_seq_length == 128
    assert GQAModel(5, args=a, config=bc, max_seq_length=72).lxrt_encoder.max_seq_length == 72
    assert VQAModel(5, args=a, config=bc).lxrt_encoder.max_seq_length == 20  # the default did not move
