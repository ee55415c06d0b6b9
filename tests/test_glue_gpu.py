"""The element-wise glue kernels and the train-mode GAT path on the GPU, against tests/glue_cases.py.

Every op is called through its ``ops`` wrapper and compared element by element with the fp64 reference of the stored
operands (bound derived in glue_cases.py) or, where the op is exact, bit for bit.  Inputs sit in a moat of NaNs.  Where the
wrapper allocates its own output the same launch is repeated through the C ABI into a band of sentinels: the band must be
intact and the window must hold the wrapper's bits.  Sizes: below / around one workgroup, and one past the capped grid so
that the second trip of the grid-stride loop runs.  Passes with and without XGGM_POISON_EMPTY=1.
"""
import ctypes

import numpy as np
import pytest
import torch

import glue_cases as C
from glue_cases import F32, BF16
from graph_long_cases import SENTINEL, banded, moated
from helpers import assert_excess, probe, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTS = [F32, BF16]
IDS = ["f32", "bf16"]


@pytest.fixture(scope="module")
def ops():
    from xggm_amd import ops
    return ops


def _abi(ops, name, shape, dt, args):
    """the launch ``name`` with its output in a band of sentinels; ``args(out)`` -> the argument tuple (stream appended)"""
    from xggm_amd._lib import call, stream
    f = banded(shape, dt, DEV)
    call(name, *args(f.view), stream())
    torch.cuda.synchronize()
    assert f.untouched_outside(), "%s wrote outside its %s output" % (name, tuple(shape))
    return f.view


def _check(got, ref, bound, what):
    return assert_excess(C.excess(got, ref, bound), what)


# ---------------------------------------------------------------------------------------------------- flat ops with a bound
@pytest.mark.parametrize("n", C.FLAT_NS + (C.N_PAST_CAP,))
@pytest.mark.parametrize("dt", DTS, ids=IDS)
def test_scale_with_a_device_scalar(ops, dt, n):
    x = C.randn(n, n, dt)
    xd = moated(x, DEV)
    e = torch.tensor([0.3], dtype=F32, device=DEV)
    got = ops.scale(xd, 0.75, e)
    _check(got, *C.scale_ref(x, 0.75, 0.3, dt), "scale %s n=%d" % (dt, n))
    out = _abi(ops, "xggm_scale_" + ops.sfx(dt), (n,), dt, lambda o: (xd.data_ptr(), o.data_ptr(), n, 0.75, e.data_ptr()))
    assert C.same_bits(out, got)
    if n == 257:  # without the scalar: one rounding
        _check(ops.scale(xd, 0.75), *C.scale_ref(x, 0.75, None, dt), "scale without scale_ptr")


@pytest.mark.parametrize("n", C.FLAT_NS + (C.N_PAST_CAP,))
@pytest.mark.parametrize("dt", DTS, ids=IDS)
def test_sigmoid_bwd(ops, dt, n):
    dy, y = C.sigmoid_inputs(n, n)
    dyd, yd = moated(dy, DEV), moated(y, DEV)
    got = ops.sigmoid_bwd(dyd, yd, dt)
    assert got.dtype == dt
    _check(got, *C.sigmoid_bwd_ref(dy, y, dt), "sigmoid_bwd %s n=%d" % (dt, n))
    out = _abi(ops, "xggm_sigmoid_bwd_" + ops.sfx(dt), (n,), dt, lambda o: (dyd.data_ptr(), yd.data_ptr(), o.data_ptr(), n))
    assert C.same_bits(out, got)


@pytest.mark.parametrize("n", C.FLAT_NS + (C.N_PAST_CAP,))
@pytest.mark.parametrize("dt", DTS, ids=IDS)
def test_tanh_bwd(ops, dt, n):
    dy, t = C.tanh_inputs(n, n, dt)
    dyd, td = moated(dy, DEV), moated(t, DEV)
    got = ops.tanh_bwd(dyd, td)
    _check(got, *C.tanh_bwd_ref(dy, t, dt), "tanh_bwd %s n=%d" % (dt, n))
    out = _abi(ops, "xggm_tanh_bwd_" + ops.sfx(dt), (n,), dt, lambda o: (dyd.data_ptr(), td.data_ptr(), o.data_ptr(), n))
    assert C.same_bits(out, got)


# ---------------------------------------------------------------------------------------------------- elu in a column window
def _wide(val, ld, col0, fill):
    """``val`` [M, D] (CPU) as columns col0.. of a contiguous [M, ld] device matrix whose other columns hold ``fill``, the
    whole matrix inside a moat of NaNs"""
    M, D = val.shape
    w = torch.full((M, ld), fill, dtype=val.dtype)
    w[:, col0:col0 + D] = val
    return moated(w, DEV)


@pytest.mark.parametrize("shape", C.ELU_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dt", DTS, ids=IDS)
def test_elu_fwd_writes_its_column_window_only(ops, dt, shape):
    M, D, ld, col0 = shape
    x = C.elu_inputs(M, D, M + D, dt)
    f = banded((M, ld), dt, DEV)
    ops.elu_fwd(moated(x, DEV), f.view, col0)
    torch.cuda.synchronize()
    assert f.untouched_outside()
    got = f.view.cpu()
    _check(got[:, col0:col0 + D], *C.elu_fwd_ref(x, dt), "elu_fwd %s %s" % (dt, shape))
    outside = torch.cat([got[:, :col0], got[:, col0 + D:]], dim=1)
    assert C.same_bits(outside, torch.full_like(outside, SENTINEL)), "elu_fwd wrote outside columns [%d, %d)" % (col0, col0 + D)


@pytest.mark.parametrize("shape", C.ELU_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dt", DTS, ids=IDS)
def test_elu_bwd_reads_its_column_window_only(ops, dt, shape):
    M, D, ld, col0 = shape
    g, y = C.randn(M * D, M, dt).view(M, D), C.elu_inputs(M, D, M + D + 1, dt)
    gd, yd = _wide(g, ld, col0, float("nan")), _wide(y, ld, col0, float("nan"))  # a read outside the window poisons dx
    got = ops.elu_bwd(gd, yd, col0, D)
    assert tuple(got.shape) == (M, D)
    _check(got, *C.elu_bwd_ref(g, y, dt), "elu_bwd %s %s" % (dt, shape))
    off = col0 * gd.element_size()
    out = _abi(ops, "xggm_elu_bwd_" + ops.sfx(dt), (M, D), dt,
               lambda o: (gd.data_ptr() + off, yd.data_ptr() + off, o.data_ptr(), M, D, ld))
    assert C.same_bits(out, got)


# ---------------------------------------------------------------------------------------------------- exact: fills
@pytest.mark.parametrize("name", sorted(C.range_cases()))
def test_zero_ranges_small_cases(ops, name):
    L, rs = C.range_cases()[name]
    buf = C.fill_pattern(L)
    f = banded((L,), F32, DEV, init=buf)
    ops.zero_ranges(f.view, rs)
    torch.cuda.synchronize()
    assert f.untouched_outside()
    assert C.same_bits(f.view, C.zero_ranges_ref(buf, rs)), name


def test_zero_ranges_with_empty_ranges_through_the_abi(ops):
    """the wrapper drops empty ranges; the entry point takes them: first, in the middle, last, and nothing but empty"""
    from xggm_amd._lib import call, stream
    buf = C.fill_pattern(64)
    rs = [(4, 4), (8, 16), (20, 20), (24, 28), (40, 40), (44, 56), (60, 60)]
    f = banded((64,), F32, DEV, init=buf)
    offs = (ctypes.c_int64 * len(rs))(*[s for s, _ in rs])
    lens = (ctypes.c_int64 * len(rs))(*[e - s for s, e in rs])
    call("xggm_zero_ranges_f32", f.view.data_ptr(), ctypes.cast(offs, ctypes.c_void_p), ctypes.cast(lens, ctypes.c_void_p),
         len(rs), stream())
    torch.cuda.synchronize()
    assert f.untouched_outside() and C.same_bits(f.view, C.zero_ranges_ref(buf, rs))
    g = banded((64,), F32, DEV, init=buf)
    call("xggm_zero_ranges_f32", g.view.data_ptr(), ctypes.cast(offs, ctypes.c_void_p), ctypes.cast((ctypes.c_int64 * 2)(0, 0), ctypes.c_void_p),
         2, stream())
    torch.cuda.synchronize()
    assert g.untouched_outside() and C.same_bits(g.view, buf)


def test_zero_ranges_one_range_past_the_grid_cap(ops):
    n, lead = C.BIG_RANGE, 8
    buf = torch.full((lead + n + 8,), 7.0, dtype=F32)
    buf[lead + n - 4:lead + n] = torch.tensor([1.0, 2.0, 3.0, 4.0])  # the last float4 of the range
    f = banded((lead + n + 8,), F32, DEV, init=buf)
    ops.zero_ranges(f.view, [(lead, lead + n)])
    torch.cuda.synchronize()
    assert f.untouched_outside()
    assert C.same_bits(f.view, C.zero_ranges_ref(buf, [(lead, lead + n)]))


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1027])
def test_zeros_f32(ops, n):
    z = ops.zeros_f32(n, DEV)
    assert z.dtype == F32 and tuple(z.shape) == (n,) and C.same_bits(z, torch.zeros(n))


@pytest.mark.parametrize("with_ranges", [True, False], ids=["ranges", "rows_only"])
@pytest.mark.parametrize("count", [20, 1000, 0], ids=["below_cap", "clamped", "none"])
@pytest.mark.parametrize("H", [C.ROWS_H, C.ROWS_H_WIDE])
def test_zero_ranges_rows(ops, H, count, with_ranges):
    R, cap = (C.ROWS_R, C.ROWS_CAP) if H == C.ROWS_H else (5, 8)
    t0 = 16
    L = t0 + R * H + 24
    buf = C.fill_pattern(L)
    rs = [(0, 8), (t0 + R * H + 4, t0 + R * H + 16)] if with_ranges else []
    ids = C.row_ids(R, cap, H)
    f = banded((L,), F32, DEV, init=buf)
    table = f.view[t0:t0 + R * H].view(R, H)
    ops.zero_ranges(f.view, rs, rows=(table, moated(ids, DEV), torch.tensor([count], dtype=torch.int32, device=DEV)))
    torch.cuda.synchronize()
    assert f.untouched_outside()
    ref = C.zero_ranges_rows_ref(buf, rs, t0, R, H, ids, count)
    assert C.same_bits(f.view, ref), (H, count, with_ranges, (C.bits(f.view) != C.bits(ref)).nonzero().flatten()[:8].tolist())


# ---------------------------------------------------------------------------------------------------- exact: zero_diag, masks, sums
@pytest.mark.parametrize("N", C.ZERO_DIAG_NS)
def test_zero_diag(ops, N):
    B = C.ZERO_DIAG_B
    a = C.zero_diag_input(B, N, N)
    ad = moated(a, DEV)
    got = ops.zero_diag(ad)
    assert C.same_bits(got, C.zero_diag_ref(a))
    out = _abi(ops, "xggm_zero_diag_f32", (B, N, N), F32, lambda o: (ad.data_ptr(), o.data_ptr(), B, N))
    assert C.same_bits(out, got)


@pytest.mark.parametrize("n", [1, 3, 257, C.N_PAST_CAP])
def test_additive_mask(ops, n):
    m = (torch.rand(n, generator=torch.Generator().manual_seed(n)) < 0.6).long().view(1, n)
    md = moated(m, DEV)
    got = ops.additive_mask(md)
    assert C.same_bits(got, C.additive_mask_ref(m))
    out = _abi(ops, "xggm_additive_mask", (1, n), F32, lambda o: (md.data_ptr(), o.data_ptr(), n))
    assert C.same_bits(out, got)


def test_add_scalars_sums_left_to_right_in_fp32(ops):
    vals = C.SCALAR_TERMS
    ts = [moated(torch.tensor([v], dtype=F32), DEV) for v in vals]
    for k in (1, 2, 3, 4):
        got = ops.add_scalars([t.view(()) for t in ts[:k]])
        assert got.dim() == 0 and float(got) == float(C.add_scalars_ref(vals[:k])), (k, float(got))
    out = _abi(ops, "xggm_add_scalars_f32", (1,), F32, lambda o: tuple(t.data_ptr() for t in ts) + (o.data_ptr(),))
    assert float(out[0]) == 0.5
    out = _abi(ops, "xggm_add_scalars_f32", (1,), F32, lambda o: (ts[0].data_ptr(), None, ts[1].data_ptr(), None, o.data_ptr()))
    assert float(out[0]) == float(C.add_scalars_ref(vals[:2]))  # NULL terms are skipped wherever they stand


# ---------------------------------------------------------------------------------------------------- exact: casts
@pytest.mark.parametrize("n", C.FLAT_NS + (C.N_PAST_CAP_BIG,))
def test_cast_bf16_rounds_to_nearest_even(ops, n):
    x = C.cast_input(n, n)
    f = banded((n,), BF16, DEV)
    ops.cast_bf16(moated(x, DEV), f.view)
    torch.cuda.synchronize()
    assert f.untouched_outside()
    assert C.same_bits(f.view, C.bf16_rne_ref(x)) and C.same_bits(f.view, x.to(BF16))


@pytest.mark.parametrize("n", C.FLAT_NS + C.N_CAST_FROM)
def test_cast_from_f32_both_types_and_every_tail(ops, n):
    x = C.cast_input(n, n)
    xd = moated(x, DEV)
    got = ops.cast_from_f32(xd, BF16)
    assert C.same_bits(got, C.bf16_rne_ref(x)) and C.same_bits(got, x.to(BF16))
    out = _abi(ops, "xggm_cast_from_f32_bf16", (n,), BF16, lambda o: (xd.data_ptr(), o.data_ptr(), n))
    assert C.same_bits(out, got)
    assert ops.cast_from_f32(xd, F32) is xd                      # the wrapper skips the identity copy; the entry makes it
    out = _abi(ops, "xggm_cast_from_f32_f32", (n,), F32, lambda o: (xd.data_ptr(), o.data_ptr(), n))
    assert C.same_bits(out, x)


def test_cast_from_f32_f32_refuses_an_output_that_is_only_8_byte_aligned(ops):
    from xggm_amd import _lib
    x, o = torch.zeros(16, device=DEV), torch.zeros(16, device=DEV)
    rc = _lib.lib.xggm_cast_from_f32_f32(x.data_ptr(), o.data_ptr() + 8, 8, _lib.stream())
    assert rc != 0 and "xggm_cast_from_f32_f32: misaligned" in _lib.last_error()
    torch.cuda.synchronize()
    assert not o.any()


def test_run_side_jobs_equal_the_stand_alone_launches(ops):
    n = 1027
    m = (torch.rand(n, generator=torch.Generator().manual_seed(1)) < 0.5).long()
    x = C.cast_input(n, 2)
    md, xd = moated(m, DEV), moated(x, DEV)
    fm, fx = banded((n,), F32, DEV), banded((n,), BF16, DEV)
    ops.run_side_jobs([(ops.SIDE_ADDITIVE_MASK, md, fm.view), (ops.SIDE_CAST_BF16, xd, fx.view)])
    torch.cuda.synchronize()
    assert fm.untouched_outside() and fx.untouched_outside()
    assert C.same_bits(fm.view, ops.additive_mask(md)) and C.same_bits(fm.view, C.additive_mask_ref(m))
    ref = torch.empty(n, dtype=BF16, device=DEV)
    ops.cast_bf16(xd, ref)
    assert C.same_bits(fx.view, ref) and C.same_bits(fx.view, C.bf16_rne_ref(x))


# ---------------------------------------------------------------------------------------------------- dropout
def _rng_state(rng):
    s = rng.cpu().tolist()
    return s[0], s[1]


@pytest.mark.parametrize("p", C.DROPOUT_PS)
def test_dropout_mask_is_the_one_the_philox_state_prescribes(ops, p):
    rng = ops.make_rng(4321, DEV)
    ops.rng_advance(rng, 3)
    seed, off = _rng_state(rng)
    assert (seed, off) == (4321, 3)
    for n in (1, 3, 257, 1027, C.N_PAST_CAP):
        got = ops.dropout_mask(n, p, rng, 48, DEV)
        assert C.same_bits(got, C.dropout_mask_host(n, p, seed, off, 48)), (p, n)
    out = _abi(ops, "xggm_dropout_mask", (1027,), F32, lambda o: (o.data_ptr(), 1027, p, rng.data_ptr(), 48))
    assert C.same_bits(out, C.dropout_mask_host(1027, p, seed, off, 48))
    assert not C.same_bits(ops.dropout_mask(1027, p, rng, 49, DEV), out)
    assert _rng_state(rng) == (seed, off)  # drawing a mask does not move the state


@pytest.mark.parametrize("n", C.FLAT_NS + (C.N_PAST_CAP,))
@pytest.mark.parametrize("dt", DTS, ids=IDS)
@pytest.mark.parametrize("p", C.DROPOUT_PS)
def test_dropout_applies_that_mask(ops, p, dt, n):
    rng = ops.make_rng(99, DEV)
    ops.rng_advance(rng, 2)
    seed, off = _rng_state(rng)
    x = C.randn(n, n, dt)
    xd = moated(x, DEV)
    mask = C.dropout_mask_host(n, p, seed, off, 32)
    got = ops.dropout(xd, p, rng, 32)
    _check(got, *C.dropout_ref(x, mask, p, dt), "dropout p=%g %s n=%d" % (p, dt, n))
    assert bool(((got.cpu() == 0) | (mask != 0)).all())                     # dropped elements are zeros
    if p == 0.5:
        assert torch.equal(got.cpu().float(), x.float() * mask)            # 2 x: exact in both types
    assert C.same_bits(ops.dropout(xd, p, rng, 32), got)                    # the same state: the same bits
    out = _abi(ops, "xggm_dropout_" + ops.sfx(dt), (n,), dt, lambda o: (xd.data_ptr(), o.data_ptr(), n, p, rng.data_ptr(), 32))
    assert C.same_bits(out, got)
    if n >= 255:
        other = ops.dropout(xd, p, rng, 33).cpu()
        assert not torch.equal(other == 0, got.cpu() == 0)                  # another stream id: another mask


# ---------------------------------------------------------------------------------------------------- gemm_raw
@pytest.mark.parametrize("dt", DTS, ids=IDS)
def test_gemm_raw_in_the_masked_lm_decoder_form(ops, dt):
    """``ops.gemm_raw`` itself (every other test reaches it through linear_* / bmm_nt): logits [cap, V] + fp32 bias into rows
    of stride vocab_ld(V) > V, as pretrain_heads.mlm_decoder_fwd calls it; helpers.gemm_excess is the bound"""
    from helpers import gemm_excess
    M, V, K = 33, 70, 64
    ld = ops.vocab_ld(V, dt)
    assert ld == 72
    t, w, bias = C.randn(M * K, 1, dt).view(M, K), C.randn(V * K, 2, dt, scale=0.2).view(V, K), C.randn(V, 3)
    f = banded((M, ld), dt, DEV)
    ops.gemm_raw(dt, moated(t, DEV), moated(w, DEV), f.view, M, V, K, K, 1, K, 1, ld, bias=moated(bias, DEV))
    torch.cuda.synchronize()
    assert f.untouched_outside()
    got = f.view.cpu()
    assert C.same_bits(got[:, V:], torch.full_like(got[:, V:], SENTINEL))
    ref = t.double() @ w.double().t() + bias.double()
    S = t.double().abs() @ w.double().abs().t() + bias.double().abs()
    assert_excess(gemm_excess(got[:, :V], ref, S, K, dt), "gemm_raw %s" % dt)


# ---------------------------------------------------------------------------------------------------- GAT in .train()
def _gat_module(H, D, dt, long_graph, seed=7):
    from xggm_amd import synth
    from xggm_amd.module.gat import GAT
    from xggm_amd.runtime import bind_root
    gat = GAT(H, D, n_head=2)
    # three times the seeded scale (0.05): attention logits of order 1, so that the attention path carries gradient
    gat.load_state_dict({k: 3.0 * torch.from_numpy(synth.seeded_param("gat." + k, v.shape, seed)) for k, v in gat.state_dict().items()})
    return bind_root(gat.to(DEV), compute_dtype=dt, long_graph=long_graph)


def _gat_inputs(B, N, H, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, N, H, generator=g)
    adj = (torch.rand(B, N, N, generator=g) < 0.4).float()
    adj[:, torch.arange(N), torch.arange(N)] = 1.0
    adj[0, 3, :] = 0.0  # a fully masked row: uniform attention
    return x, adj


def _gat_pass(gat, x, adj, pr):
    """forward + backward; (out, dx, {name: parameter gradient}) as CPU copies, gradients cleared afterwards"""
    from xggm_amd.runtime import runtime_of
    xg = x.clone().requires_grad_(True)
    out = gat(xg, adj)
    (out.float() * pr).sum().backward()
    torch.cuda.synchronize()
    res = out.detach().cpu(), xg.grad.detach().cpu(), {k: p.grad.detach().double().cpu() for k, p in gat.named_parameters()}
    for p in gat.parameters():
        p.grad = None
    runtime_of(gat).arena.begin_pass()
    return res


@pytest.mark.parametrize("B,N,H,D,dt,long_graph", [(3, 17, 64, 24, F32, False), (3, 17, 64, 24, BF16, False), (3, 72, 64, 24, BF16, True)],
                         ids=["f32_n17", "bf16_n17", "bf16_n72_long"])
def test_gat_train_mode_uses_the_prescribed_mask_forward_and_backward(B, N, H, D, dt, long_graph):
    """GATFn drops its input in the forward and, by stream id, ``dx`` in the backward: both with the mask the Philox state
    prescribes (p = 0.5: keep = 2, every product exact), and the whole pass agrees with the fp64 oracle under that mask"""
    from oracle import xggm_oracle as O
    from test_oracle_golden import check_grad_summary
    from xggm_amd.runtime import runtime_of
    gat = _gat_module(H, D, dt, long_graph)
    x0, adj0 = _gat_inputs(B, N, H, N)
    x0 = x0.to(dt)                                   # as stored
    xd, adj = x0.to(DEV), adj0.to(DEV)
    pr = probe("gat_out", (B, N, 2 * D), 7, device=DEV)

    gat.train()
    rt = runtime_of(gat)
    assert rt.long_graph is long_graph and rt.p(gat.dropout) == 0.5
    seed, off = _rng_state(rt.rng)
    keep = C.dropout_mask_host(B * N * H, 0.5, seed, off, gat._sid).view(B, N, H)
    assert set(keep.unique().tolist()) == {0.0, 2.0} and 0.4 < float((keep == 0).float().mean()) < 0.6
    out_t, dx_t, G_t = _gat_pass(gat, xd, adj, pr)
    assert _rng_state(rt.rng) == (seed, off)

    gat.eval()
    xk = (x0.float() * keep).to(dt)                  # exact: 0 or 2 x
    assert torch.equal(xk.float(), x0.float() * keep)
    out_e, dx_e, G_e = _gat_pass(gat, xk.to(DEV), adj, pr)

    # 1. the forward dropped exactly the prescribed elements
    assert C.same_bits(out_t, out_e)
    # 2. the backward dropped the same ones: zero where dropped, keep * (gradient at x * keep) elsewhere
    dropped = keep == 0
    assert bool((dx_t.float()[dropped] == 0).all())
    assert torch.equal(dx_t.float(), dx_e.float() * keep)
    for k in G_t:
        assert torch.equal(G_t[k], G_e[k]), k

    # 3. against the fp64 oracle with the host mask
    P = {k: p.detach().double().cpu().requires_grad_(True) for k, p in gat.named_parameters()}
    x64 = x0.double().requires_grad_(True)
    ref = O.gat(P, "", x64, adj0.double(), 2, drop=lambda t, p, tag: t * keep.double())
    (ref * pr.double().cpu()).sum().backward()
    # test_model_gpu.test_generator_against_reference_golden: ``t = 1e-4 if dt == F32 else 3e-2`` on the output,
    e_out = rel_err(out_t, ref)
    # ``tg = 2e-3 if dt == F32 else 6e-2`` on the input gradient
    e_dx = rel_err(dx_t, x64.grad)
    print("gat train %s N=%d: output rel_err %.3e, dx rel_err %.3e" % (dt, N, e_out, e_dx))
    assert e_out < (1e-4 if dt == F32 else 3e-2)
    assert e_dx < (2e-3 if dt == F32 else 6e-2)
    names = sorted(P)
    norms = [float(P[k].grad.norm()) for k in names]
    for k, rn in zip(names, norms):
        print("  %s: |g| %.6e, oracle %.6e" % (k, float(G_t[k].norm()), rn))
    if dt == F32:
        # ``check_grad_summary(g, G, seed, 2e-3)``: norms and probe projections of every parameter gradient
        dots = [float((P[k].grad * probe(k, P[k].shape, 7).double()).sum()) for k in names]
        check_grad_summary({"grad_names": np.array(names), "grad_norms": np.array(norms), "grad_dots": np.array(dots)}, G_t, 7, 2e-3)
    else:
        # ``elif rn > 1e-3: assert abs(float(G[str(n)].norm()) - rn) < 8e-2 * rn``
        for k, rn in zip(names, norms):
            if rn > 1e-3:
                assert abs(float(G_t[k].norm()) - rn) < 8e-2 * rn, (k, float(G_t[k].norm()), rn)
