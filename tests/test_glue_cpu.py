"""What the glue kernels' yardstick (tests/glue_cases.py) and their host checks promise without a GPU.

  * the references are the operations they claim to be: the backward rules written in the OUTPUT of elu / sigmoid / tanh
    equal fp64 autograd through the activation, the fills and masks equal the framework expressions they replace, the
    bit-level bf16 rounding equals ``tensor.to(torch.bfloat16)``;
  * every bound admits an honest fp32 evaluation of the same formula (torch on the CPU, rounded to bf16 where the kernel
    stores bf16) and rejects a planted fault of the kind the kernel could have;
  * every entry point refuses null pointers, empty sizes and the layouts its kernel cannot take on the host, with its own
    name in xggm_last_error() -- nothing is enqueued (there is no GPU here to enqueue on).
"""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import glue_cases as C
from glue_cases import F32, BF16

FAKE = 0x10000  # a 16-byte aligned address nobody dereferences: validation happens on the host, before any launch
DTS = [F32, BF16]
NS = C.FLAT_NS


def _mx(exc):
    return float(exc.max())


# ---------------------------------------------------------------------------------------------------- reference validity
def test_backward_rules_in_the_output_equal_fp64_autograd_of_the_activation():
    g = C.randn(1027, 1).double()
    x = C.elu_inputs(79, 13, 2, F32).reshape(-1).double().requires_grad_(True)
    y = F.elu(x)
    (y * g).sum().backward()
    ref, _ = C.elu_bwd_ref(g, y.detach(), F32)
    # y + 1 = exp(x) up to one fp64 rounding of y (2^-53, absolute): all the rule written in y can lose
    assert torch.allclose(ref, x.grad, rtol=1e-13, atol=1e-14)
    fwd, _ = C.elu_fwd_ref(x.detach(), F32)
    assert torch.equal(fwd, y.detach())
    for act, rule in ((torch.sigmoid, C.sigmoid_bwd_ref), (torch.tanh, C.tanh_bwd_ref)):
        x = C.randn(1027, 3, scale=3.0).double().requires_grad_(True)
        y = act(x)
        (y * g).sum().backward()
        ref, _ = rule(g, y.detach(), F32)
        assert torch.allclose(ref, x.grad, rtol=1e-12, atol=1e-14)  # (1 - y, 1 - y^2 near |y| = 1: fp64 roundings of y)


@pytest.mark.parametrize("N", C.ZERO_DIAG_NS)
def test_zero_diag_reference_is_triu_plus_tril(N):
    a = C.zero_diag_input(C.ZERO_DIAG_B, N, N)
    assert not torch.isfinite(torch.diagonal(a, dim1=1, dim2=2)).any()
    ref = C.zero_diag_ref(a)
    assert torch.isfinite(ref).all()
    assert C.same_bits(ref, a.triu(1) + a.tril(-1))


def test_additive_mask_and_scalar_sum_references():
    m = (torch.rand(3, 20, generator=torch.Generator().manual_seed(0)) < 0.6).long()
    assert C.same_bits(C.additive_mask_ref(m), (1.0 - m.float()) * -10000.0)
    assert float(C.add_scalars_ref(C.SCALAR_TERMS)) == 0.5            # left to right in fp32
    assert sum(float(v) for v in C.SCALAR_TERMS) == 1.5               # what a wider accumulator returns
    t = torch.tensor(C.SCALAR_TERMS, dtype=F32)
    assert float(((t[0] + t[1]) + t[2]) + t[3]) == float(C.add_scalars_ref(C.SCALAR_TERMS))


def test_bf16_rounding_reference_is_the_framework_conversion():
    x = C.cast_input(1027, 5)
    assert C.same_bits(C.bf16_rne_ref(x), x.to(BF16))
    sp = torch.from_numpy(C.CAST_SPECIAL.view(np.float32).copy())
    got = C.bits(C.bf16_rne_ref(sp)).numpy().view(np.uint16)
    assert got[0] == 0x3F80 and got[1] == 0x3F82 and got[2] == 0xBF80 and got[3] == 0xBF82   # ties go to even, both ways
    assert got[6] == 0x7F80 and got[7] == 0xFF80 and got[9] == 0x7F7F                        # rounds to inf / survives
    assert torch.isnan(C.bf16_rne_ref(sp)[12].float())


# ---------------------------------------------------------------------------------------------------- honest fp32 evaluations
def _honest(name, n, dt, seed=0):
    """(fp32-evaluated result stored as dt, reference, bound) of one flat op"""
    if name == "scale":
        x, s, e = C.randn(n, seed, dt), 0.75, np.float32(0.3)
        s32 = torch.tensor(s, dtype=F32) * (torch.tensor(1.0, dtype=F32) + torch.tensor(e, dtype=F32))
        return (s32 * x.float()).to(dt), *C.scale_ref(x, s, e, dt)
    if name == "sigmoid_bwd":
        dy, y = C.sigmoid_inputs(n, seed)
        return (dy * y * (1.0 - y)).to(dt), *C.sigmoid_bwd_ref(dy, y, dt)
    if name == "tanh_bwd":
        dy, t = C.tanh_inputs(n, seed, dt)
        return (dy.float() * (1.0 - t.float() * t.float())).to(dt), *C.tanh_bwd_ref(dy, t, dt)
    if name == "elu_fwd":
        x = C.elu_inputs(n, 1, seed, dt).reshape(-1)
        v = x.float()
        return torch.where(v > 0, v, torch.expm1(v)).to(dt), *C.elu_fwd_ref(x, dt)
    if name == "elu_bwd":
        g, y = C.randn(n, seed, dt), C.elu_inputs(n, 1, seed + 1, dt).reshape(-1)
        return torch.where(y.float() > 0, g.float(), g.float() * (y.float() + 1.0)).to(dt), *C.elu_bwd_ref(g, y, dt)
    if name.startswith("dropout"):
        p = float(name[7:])
        x, mask = C.randn(n, seed, dt), C.dropout_mask_host(n, p, 9595, 3, 48)
        return (x.float() * mask).to(dt), *C.dropout_ref(x, mask, p, dt)
    raise KeyError(name)


OPS = ["scale", "sigmoid_bwd", "tanh_bwd", "elu_fwd", "elu_bwd", "dropout0.5", "dropout0.1"]


@pytest.mark.parametrize("dt", DTS, ids=["f32", "bf16"])
@pytest.mark.parametrize("name", OPS)
def test_each_bound_admits_an_honest_fp32_evaluation(name, dt):
    for n in NS + (20011,):
        got, ref, bound = _honest(name, n, dt, seed=n)
        assert _mx(C.excess(got, ref, bound)) <= 1.0, (name, n)


def test_dropout_host_mask_keeps_about_one_minus_p_and_half_is_exact():
    for p in C.DROPOUT_PS:
        m = C.dropout_mask_host(20011, p, 9595, 0, 16)
        kept = float((m != 0).float().mean())
        assert abs(kept - (1 - p)) < 0.02 and set(m.unique().tolist()) == {0.0, float(np.float32(1) / (np.float32(1) - np.float32(p)))}
    x, m = C.randn(1027, 1), C.dropout_mask_host(1027, 0.5, 9595, 0, 16)
    ref, bound = C.dropout_ref(x, m, 0.5, F32)
    assert torch.equal((x * m).double(), ref)


# ---------------------------------------------------------------------------------------------------- planted faults
def _truncate_to_bf16(x32):
    return (C.bits(x32.float()) & -65536).view(F32).to(BF16)  # drop the low 16 bits: exact in bf16


@pytest.mark.parametrize("name", [o for o in OPS if o != "dropout0.5"])  # p = 0.5: 2 x is a bf16 value, nothing to truncate
def test_bounds_reject_a_truncating_bf16_store(name):
    n = 1027
    _, ref, bound = _honest(name, n, BF16, seed=n)
    exc = C.excess(_truncate_to_bf16(ref.float()), ref, bound)
    assert _mx(exc) > 1.0 and int((exc > 1).sum()) > n // 20, (name, _mx(exc))


def test_bounds_reject_wrong_backward_formulas():
    for dt in DTS:
        g, y = C.randn(1027, 1, dt), C.elu_inputs(1027, 1, 2, dt).reshape(-1)
        ref, bound = C.elu_bwd_ref(g, y, dt)
        bad = torch.where(y.float() > 0, g.float(), g.float() * y.float()).to(dt)        # g * y for g * (y + 1)
        assert _mx(C.excess(bad, ref, bound)) > 1.0
        swapped = torch.where(y.float() >= 0, g.float(), g.float() * (y.float() + 1.0)).to(dt)
        assert _mx(C.excess(swapped, ref, bound)) <= 1.0   # y == 0: both branches give g, the rule has no edge there
        dy, t = C.tanh_inputs(1027, 3, dt)
        ref, bound = C.tanh_bwd_ref(dy, t, dt)
        bad = (dy.float() * (1.0 - t.float())).to(dt)                                     # 1 - t for 1 - t^2
        assert _mx(C.excess(bad, ref, bound)) > 1.0
    # the absolute term is needed and no wider than needed: at |t| = 0.996 an fp32 evaluation uses most of it ...
    dy, t = C.tanh_inputs(20011, 5, F32)
    ref, bound = C.tanh_bwd_ref(dy, t, F32)
    got = dy * (1.0 - t * t)
    rel_only = 2.0 * C.U32 * ref.abs()
    assert _mx(C.excess(got, ref, bound)) <= 1.0 < _mx(C.excess(got, ref, rel_only.clamp_min(1e-300)))
    # ... and a result off by one fp32 ulp of dy (2^-23 |dy|) near |t| = 1 is caught
    near = t.abs() > 0.99
    assert near.any() and _mx(C.excess(got + near * dy * 2.0 ** -22, ref, bound)) > 1.0


def test_fills_are_compared_exactly():
    for name, (L, rs) in C.range_cases().items():
        buf = C.fill_pattern(L)
        ref = C.zero_ranges_ref(buf, rs)
        assert int((ref == 0).sum()) == sum(e - s for s, e in rs) and C.same_bits(ref, ref.clone())
        s, e = rs[-1]
        missed = ref.clone()
        missed[e - 4:e] = buf[e - 4:e]                     # the last float4 of a range left as it was
        assert not C.same_bits(missed, ref)
        over = ref.clone()
        over[e] = 0.0                                      # one element past a range zeroed
        assert not C.same_bits(over, ref)
    R, H, t0 = C.ROWS_R, C.ROWS_H, 16
    buf = C.fill_pattern(t0 + R * H + 8)
    ids = C.row_ids(R, C.ROWS_CAP, 0)
    ref = C.zero_ranges_rows_ref(buf, [(0, 8)], t0, R, H, ids, 20)
    rows = ref[t0:t0 + R * H].view(R, H)
    zeroed = sorted(set(int(i) for i in ids[:20] if 0 <= int(i) < R))
    assert [r for r in range(R) if bool((rows[r] == 0).all())] == zeroed and len(zeroed) < 20  # duplicates, -1 and R
    assert bool((rows[30:] != 0).all())                    # rows only entries past the count name
    clamp = C.zero_ranges_rows_ref(buf, [], t0, R, H, ids, 1000)
    assert bool((clamp[t0 + 30 * H:t0 + R * H].view(-1, H) == 0).all(1).any()) and bool((clamp[:t0] != 0).all())
    assert C.same_bits(C.zero_ranges_rows_ref(buf, [], t0, R, H, ids, 0), buf)


def test_zero_diag_dropout_and_cast_references_reject_their_faults():
    a = C.zero_diag_input(3, 36, 1)
    ref = C.zero_diag_ref(a)
    kept = ref.clone()
    kept[2, 35, 35] = a[2, 35, 35]                         # one diagonal element kept
    assert not C.same_bits(kept, ref)
    for p in C.DROPOUT_PS:
        m = C.dropout_mask_host(1027, p, 9595, 1, 32)
        assert not C.same_bits(torch.roll(m, 1), m)        # the mask shifted by one element
        assert not C.same_bits(C.dropout_mask_host(1027, p, 9595, 1, 33), m)
        for dt in DTS:
            x = C.randn(1027, 2, dt)
            ref, bound = C.dropout_ref(x, m, p, dt)
            assert _mx(C.excess((x.float() * torch.roll(m, 1)).to(dt), ref, bound)) > 1.0
    for r in (1, 2, 3):
        x = C.cast_input(1024 + r, r)
        ref = C.bf16_rne_ref(x)
        tail = ref.clone()
        tail[-r:] = -1234.0                                # the tail elements left as the sentinel
        assert not C.same_bits(tail, ref)
        assert not C.same_bits(_truncate_to_bf16(x), ref)  # and a truncating conversion


# ---------------------------------------------------------------------------------------------------- host refusals
def _arr(vals):
    a = (ctypes.c_int64 * len(vals))(*vals)
    return a, ctypes.cast(a, ctypes.c_void_p)


def _refused(L, name, rc, what=""):
    msg = L.xggm_last_error().decode()
    assert rc != 0 and name in msg and what in msg, (name, rc, msg)


def _flat_entries():
    """name -> callable(L, ptr, n): the entry with every pointer = ptr and element count n"""
    E = {}
    for s in ("f32", "bf16"):
        E["xggm_scale_" + s] = lambda L, p, n, k="xggm_scale_" + s: getattr(L, k)(p, p, n, 1.0, None, None)
        E["xggm_sigmoid_bwd_" + s] = lambda L, p, n, k="xggm_sigmoid_bwd_" + s: getattr(L, k)(p, p, p, n, None)
        E["xggm_tanh_bwd_" + s] = lambda L, p, n, k="xggm_tanh_bwd_" + s: getattr(L, k)(p, p, p, n, None)
        E["xggm_cast_from_f32_" + s] = lambda L, p, n, k="xggm_cast_from_f32_" + s: getattr(L, k)(p, p, n, None)
        E["xggm_dropout_" + s] = lambda L, p, n, k="xggm_dropout_" + s: getattr(L, k)(p, p, n, 0.5, p, 16, None)
        E["xggm_elu_fwd_" + s] = lambda L, p, n, k="xggm_elu_fwd_" + s: getattr(L, k)(p, p, n, 8, 8, None)
        E["xggm_elu_bwd_" + s] = lambda L, p, n, k="xggm_elu_bwd_" + s: getattr(L, k)(p, p, p, n, 8, 8, None)
    E["xggm_cast_f32_to_bf16"] = lambda L, p, n: L.xggm_cast_f32_to_bf16(p, p, n, None)
    E["xggm_dropout_mask"] = lambda L, p, n: L.xggm_dropout_mask(p, n, 0.5, p, 16, None)
    E["xggm_additive_mask"] = lambda L, p, n: L.xggm_additive_mask(p, p, n, None)
    E["xggm_zero_diag_f32"] = lambda L, p, n: L.xggm_zero_diag_f32(p, p, 2, n, None)
    E["xggm_gather_rows_bf16"] = lambda L, p, n: L.xggm_gather_rows_bf16(p, p, p, n, 8, 10, None)
    E["xggm_scatter_rows_bf16"] = lambda L, p, n: L.xggm_scatter_rows_bf16(p, p, p, n, 8, 10, None)
    return E


@pytest.mark.parametrize("name", sorted(_flat_entries()))
def test_entries_refuse_null_pointers_and_empty_sizes_before_launch(name):
    from xggm_amd import _lib
    L, call = _lib.lib, _flat_entries()[name]
    _refused(L, name, call(L, None, 8))
    for n in (0, -3):
        _refused(L, name, call(L, FAKE, n))


def test_zero_ranges_refusals():
    from xggm_amd import _lib
    L = _lib.lib
    name = "xggm_zero_ranges_f32"
    keep, offs = _arr([0] + [8 * i for i in range(1, 17)])
    keep2, lens = _arr([4] * 17)
    _refused(L, name, L.xggm_zero_ranges_f32(None, offs, lens, 1, None))
    _refused(L, name, L.xggm_zero_ranges_f32(FAKE, None, lens, 1, None))
    _refused(L, name, L.xggm_zero_ranges_f32(FAKE, offs, None, 1, None))
    for n in (0, -1, 17):
        _refused(L, name, L.xggm_zero_ranges_f32(FAKE, offs, lens, n, None), "n = %d" % n)
    _refused(L, name, L.xggm_zero_ranges_f32(FAKE + 4, offs, lens, 2, None), "16-byte aligned")
    k3, bad_off = _arr([0, 6])
    _refused(L, name, L.xggm_zero_ranges_f32(FAKE, bad_off, lens, 2, None), "range 1")
    k4, bad_len = _arr([4, 4, 7])
    _refused(L, name, L.xggm_zero_ranges_f32(FAKE, offs, bad_len, 3, None), "range 2")
    k5, neg = _arr([-4])
    _refused(L, name, L.xggm_zero_ranges_f32(FAKE, neg, lens, 1, None), "range 0")

    name = "xggm_zero_ranges_rows_f32"
    rows = lambda base=FAKE, o=offs, l=lens, n=1, table=FAKE, ids=FAKE, cnt=FAKE, cap=8, R=37, H=12: \
        L.xggm_zero_ranges_rows_f32(base, o, l, n, table, ids, cnt, cap, R, H, None)
    _refused(L, name, rows(base=None))
    _refused(L, name, rows(n=17), "n = 17")
    _refused(L, name, rows(n=-1))
    _refused(L, name, rows(o=None))
    for kw in (dict(table=None), dict(ids=None), dict(cnt=None), dict(cap=0), dict(R=0), dict(H=0), dict(H=-4)):
        _refused(L, name, rows(**kw), "bad row list")
    for H in (1, 6, 1027):
        _refused(L, name, rows(H=H), "bad row list")          # H % 4 != 0
    _refused(L, name, rows(table=FAKE + 8), "16-byte aligned")
    _refused(L, name, rows(base=FAKE + 4), "16-byte aligned")
    _refused(L, name, rows(o=bad_off, n=2), "range 1")


def test_elu_dropout_and_scalar_refusals():
    from xggm_amd import _lib
    L = _lib.lib
    for s in ("f32", "bf16"):
        fwd, bwd, drop = (getattr(L, "xggm_%s_%s" % (k, s)) for k in ("elu_fwd", "elu_bwd", "dropout"))
        for M, D, ld in ((4, 8, 7), (4, 0, 8), (4, -1, 8), (0, 8, 8)):   # ld < D; empty
            _refused(L, "xggm_elu_fwd_" + s, fwd(FAKE, FAKE, M, D, ld, None))
            _refused(L, "xggm_elu_bwd_" + s, bwd(FAKE, FAKE, FAKE, M, D, ld, None))
        for p in (0.0, 1.0, -0.1, 1.5):
            _refused(L, "xggm_dropout_" + s, drop(FAKE, FAKE, 8, p, FAKE, 16, None))
        _refused(L, "xggm_dropout_" + s, drop(FAKE, FAKE, 8, 0.5, None, 16, None))  # null rng
    for p in (1.0, -0.1):
        _refused(L, "xggm_dropout_mask", L.xggm_dropout_mask(FAKE, 8, p, FAKE, 16, None))
    _refused(L, "xggm_dropout_mask", L.xggm_dropout_mask(FAKE, 8, 0.5, None, 16, None))
    _refused(L, "xggm_add_scalars_f32", L.xggm_add_scalars_f32(FAKE, FAKE, None, None, None, None))
    for B, N in ((0, 4), (-1, 4)):
        _refused(L, "xggm_zero_diag_f32", L.xggm_zero_diag_f32(FAKE, FAKE, B, N, None))


def test_vector_accesses_refuse_misaligned_pointers():
    """four elements per access: a 16-byte store needs a 16-byte aligned address (cast_from_f32_f32's ``out`` was held
    to 8 only, the row gather / scatter to nothing)"""
    from xggm_amd import _lib
    L = _lib.lib
    what = "misaligned"
    _refused(L, "xggm_cast_from_f32_f32", L.xggm_cast_from_f32_f32(FAKE, FAKE + 8, 8, None), what)
    _refused(L, "xggm_cast_from_f32_f32", L.xggm_cast_from_f32_f32(FAKE + 8, FAKE, 8, None), what)
    _refused(L, "xggm_cast_from_f32_bf16", L.xggm_cast_from_f32_bf16(FAKE, FAKE + 4, 8, None), what)
    _refused(L, "xggm_cast_from_f32_bf16", L.xggm_cast_from_f32_bf16(FAKE + 8, FAKE, 8, None), what)
    g, s = L.xggm_gather_rows_bf16, L.xggm_scatter_rows_bf16
    _refused(L, "xggm_gather_rows_bf16", g(FAKE + 8, FAKE, FAKE, 4, 8, 10, None), what)   # src: 16
    _refused(L, "xggm_gather_rows_bf16", g(FAKE, FAKE, FAKE + 4, 4, 8, 10, None), what)   # dst: 8
    _refused(L, "xggm_scatter_rows_bf16", s(FAKE + 4, FAKE, FAKE, 4, 8, 10, None), what)
    _refused(L, "xggm_scatter_rows_bf16", s(FAKE, FAKE, FAKE + 2, 4, 8, 10, None), what)
    for fn, name in ((g, "xggm_gather_rows_bf16"), (s, "xggm_scatter_rows_bf16")):
        _refused(L, name, fn(FAKE, FAKE, FAKE, 4, 6, 10, None))                             # H % 4 != 0
        _refused(L, name, fn(FAKE, FAKE, FAKE, 4, 8, 0, None))                              # empty table
