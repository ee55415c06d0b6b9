"""Thin tensor-level wrappers over the C ABI (one Python function per kernel family).

No arithmetic happens here: each function checks shapes on the host -- a kernel that
faults can reset the whole GPU node -- and enqueues one HIP kernel on the current stream.
"""
import torch

from . import _lib
from ._lib import call, ptr, stream

ACT_NONE, ACT_GELU, ACT_SIGMOID, ACT_TANH, ACT_GELU_GRAD = 0, 1, 2, 3, 4
AGG_PLAIN, AGG_TRANSPOSE, AGG_SYMMETRIZE = 0, 1, 2
F32 = torch.float32
BF16 = torch.bfloat16


def sfx(dt):
    if dt == F32:
        return "f32"
    if dt == BF16:
        return "bf16"
    raise TypeError("xggm_amd supports float32 and bfloat16 activations, got %s" % dt)


def _chk(t, dt=None, name="tensor"):
    if not t.is_cuda:
        raise RuntimeError("xggm_amd: %s must live on the GPU (no CPU fallback)" % name)
    if dt is not None and t.dtype != dt:
        raise TypeError("xggm_amd: %s has dtype %s, expected %s" % (name, t.dtype, dt))
    return t


def _c(t, dt=None, name="tensor"):
    _chk(t, dt, name)
    if not t.is_contiguous():
        raise RuntimeError("xggm_amd: %s must be contiguous" % name)
    return t


# ----------------------------------------------------------------------------- GEMM
def gemm_raw(dt, A, B, C, M, N, K, a_rs, a_ks, b_ns, b_ks, ldc, batch=1, a_bs=0, b_bs=0, c_bs=0,
             bias=None, residual=None, preact=None, aux=None, act=ACT_NONE, c_f32=False,
             accumulate=False, alpha=1.0, colsum=None):
    """``colsum``: fp32 [batch * ceil(M/32), N] partial rows (see xggm.h), overwritten"""
    if colsum is not None:
        assert colsum.dtype == F32 and colsum.numel() >= batch * colsum_rows(M) * N
    call("xggm_gemm_" + sfx(dt), ptr(A), ptr(B), ptr(C), M, N, K, a_rs, a_ks, b_ns, b_ks, ldc, batch,
         a_bs, b_bs, c_bs, ptr(bias), ptr(residual), ptr(preact), ptr(aux), ptr(colsum), act, int(c_f32),
         int(accumulate), float(alpha), stream())


def _rows(x):
    """(M, K, row stride) of a 2-D view whose last dim is contiguous."""
    if x.dim() != 2 or x.stride(1) != 1:
        raise RuntimeError("xggm_amd: expected a 2-D operand with unit inner stride")
    return x.shape[0], x.shape[1], x.stride(0)


def linear_fwd(x, w, bias=None, act=ACT_NONE, want_preact=False, out_f32=False, residual=None):
    """y[M,N] = act(x[M,K] @ w[N,K]^T + bias) (+ residual).  Returns (y, preact|None)."""
    M, K, a_rs = _rows(_chk(x))
    N, K2 = w.shape
    if K2 != K or w.dtype != x.dtype or not w.is_contiguous():
        raise RuntimeError("linear_fwd: weight %s/%s does not match input %s/%s"
                           % (tuple(w.shape), w.dtype, tuple(x.shape), x.dtype))
    if bias is not None:
        _c(bias, F32, "bias")
        assert bias.numel() == N
    y = torch.empty((M, N), device=x.device, dtype=F32 if out_f32 else x.dtype)
    pre = torch.empty((M, N), device=x.device, dtype=x.dtype) if want_preact else None
    if residual is not None:
        assert residual.shape == y.shape and residual.dtype == x.dtype and residual.is_contiguous()
    gemm_raw(x.dtype, x, w, y, M, N, K, a_rs, 1, K, 1, N, bias=bias, preact=pre, act=act,
             c_f32=out_f32, residual=residual)
    return y, pre


# ----------------------------------------------------------------------------- fp8 forward (config C5)
FP8 = torch.float8_e4m3fn
FP8_MAX = 448.0


def quantize_fp8(x, qscale=None, amax=None, out=None):
    """x (fp32 / bf16, contiguous, numel % 8 == 0) -> e4m3fn(clamp(x * qscale, +-448)); ``qscale``: 1-element fp32
    device tensor or None (1); ``amax``: 1-element fp32 device tensor raised to max |x|, or None; ``out``: a
    contiguous 1-byte tensor of the same number of elements to write into."""
    _c(x)
    if x.dtype not in (F32, BF16):
        raise RuntimeError("quantize_fp8: fp32 or bf16 input expected, got %s" % x.dtype)
    if out is not None:
        _c(out)
        assert out.numel() == x.numel() and out.element_size() == 1
    y = out if out is not None else torch.empty(x.shape, device=x.device, dtype=FP8)
    call("xggm_quantize_fp8e4m3_" + sfx(x.dtype), ptr(x), ptr(y), x.numel(), ptr(qscale), ptr(amax), stream())
    return y


def fp8_scale_for(amax):
    """(quantisation scale, its reciprocal) of a tensor whose max |x| is ``amax`` (1-element fp32 device tensor):
    amax lands on the largest e4m3 value; an all-zero tensor gets scale 1."""
    q = torch.where(amax > 0, FP8_MAX / amax, torch.ones_like(amax))
    return q, 1.0 / q


def linear_fwd_fp8(x8, w8, sx, sw, bias=None, act=ACT_NONE, want_preact=False, out_f32=False, residual=None):
    """y[M,N] = act(sx * sw * (x8[M,K] @ w8[N,K]^T) + bias) (+ residual) with e4m3 operands; bf16 (or fp32) result.
    ``sx`` / ``sw``: 1-element fp32 device tensors, the reciprocals of the operands' quantisation scales."""
    M, K, a_rs = _rows(x8)
    N, K2 = w8.shape
    if x8.dtype != FP8 or w8.dtype != FP8 or K2 != K or w8.stride(1) != 1:
        raise RuntimeError("linear_fwd_fp8: e4m3 operands [M,K] / [N,K] expected")
    y = torch.empty((M, N), device=x8.device, dtype=F32 if out_f32 else BF16)
    pre = torch.empty((M, N), device=x8.device, dtype=BF16) if want_preact else None
    if residual is not None:
        assert residual.shape == y.shape and residual.dtype == BF16 and residual.is_contiguous()
    call("xggm_gemm_fp8e4m3", ptr(x8), ptr(w8), ptr(y), M, N, K, a_rs, w8.stride(0), N, ptr(sx), ptr(sw), ptr(bias),
         ptr(residual), ptr(pre), act, int(out_f32), stream())
    return y, pre


def linear_dgrad(dy, w, residual=None, gelu_aux=None):
    """dx[M,K] = dy[M,N] @ w[N,K] (+ residual), optionally times gelu'(aux) (aux, dx same shape)."""
    M, N, a_rs = _rows(_chk(dy))
    N2, K = w.shape
    if N2 != N or w.dtype != dy.dtype or not w.is_contiguous():
        raise RuntimeError("linear_dgrad: weight %s does not match grad %s" % (tuple(w.shape), tuple(dy.shape)))
    dx = torch.empty((M, K), device=dy.device, dtype=dy.dtype)
    if residual is not None:
        assert residual.shape == dx.shape and residual.dtype == dy.dtype and residual.is_contiguous()
    if gelu_aux is not None:
        assert gelu_aux.shape == dx.shape and gelu_aux.dtype == dy.dtype and gelu_aux.is_contiguous()
    # B(k=n', n=k') = w[n', k']: column index contiguous, reduction index strided by K
    gemm_raw(dy.dtype, dy, w, dx, M, K, N, a_rs, 1, 1, K, K, residual=residual, aux=gelu_aux,
             act=ACT_GELU_GRAD if gelu_aux is not None else ACT_NONE)
    return dx


def linear_wgrad(dy, x, gw, accumulate):
    """gw[N,K] (+)= dy[M,N]^T @ x[M,K]; gw fp32, or bf16 (the data-parallel wire arena: the gradient is born in the
    type it crosses the links in)."""
    M, N, dy_rs = _rows(_chk(dy))
    M2, K, x_rs = _rows(_chk(x))
    if M2 != M or x.dtype != dy.dtype:
        raise RuntimeError("linear_wgrad: %s vs %s" % (tuple(dy.shape), tuple(x.shape)))
    _c(gw)
    assert tuple(gw.shape) == (N, K) and (gw.dtype == F32 or gw.dtype == dy.dtype)
    # A(m=n, k=m') = dy[m', n]: row index contiguous; B(k=m', n=k) = x[m', k]
    gemm_raw(dy.dtype, dy, x, gw, N, K, M, 1, dy_rs, 1, x_rs, K, c_f32=gw.dtype == F32, accumulate=accumulate)


def _ws(nbytes, device):
    """scratch for the two-stage reductions (caller-owned, as the C ABI requires)."""
    return torch.empty((nbytes + 3) // 4, device=device, dtype=F32), nbytes


# ---- grouped launches: several independent products in one grid -------------------------------
import ctypes as _ct
import os


class GemmProblem(_ct.Structure):
    """mirror of ``xggm_gemm_problem`` (include/xggm.h)"""
    _fields_ = [("A", _ct.c_void_p), ("B", _ct.c_void_p), ("C", _ct.c_void_p),
                ("M", _ct.c_int), ("N", _ct.c_int), ("K", _ct.c_int),
                ("a_rs", _ct.c_int64), ("a_ks", _ct.c_int64), ("b_ns", _ct.c_int64), ("b_ks", _ct.c_int64),
                ("ldc", _ct.c_int64), ("batch", _ct.c_int),
                ("a_bs", _ct.c_int64), ("b_bs", _ct.c_int64), ("c_bs", _ct.c_int64),
                ("bias", _ct.c_void_p), ("residual", _ct.c_void_p), ("preact", _ct.c_void_p), ("aux", _ct.c_void_p),
                ("colsum", _ct.c_void_p), ("act", _ct.c_int), ("c_f32", _ct.c_int), ("accumulate", _ct.c_int), ("alpha", _ct.c_float),
                ("sqsum", _ct.c_void_p),
                ("scale_a", _ct.c_void_p), ("scale_b", _ct.c_void_p), ("c8", _ct.c_void_p), ("c8_qscale", _ct.c_void_p),
                ("c8_amax", _ct.c_void_p), ("amax_slots", _ct.c_int)]


def _problem(A, B, C, M, N, K, a_rs, a_ks, b_ns, b_ks, ldc, bias=None, residual=None, preact=None, aux=None,
             act=ACT_NONE, c_f32=False, accumulate=False, colsum=None):
    p = GemmProblem(ptr(A), ptr(B), ptr(C), M, N, K, a_rs, a_ks, b_ns, b_ks, ldc, 1, 0, 0, 0, ptr(bias),
                    ptr(residual), ptr(preact), ptr(aux), ptr(colsum), act, int(c_f32), int(accumulate), 1.0)
    # the descriptor holds raw pointers and may be launched later (grouped with other problems): it keeps its
    # operands alive, otherwise the caching allocator can hand their memory to the next torch.empty
    p.keep = (A, B, C, bias, residual, preact, aux, colsum)
    return p


def p_fwd(x, w, bias=None, act=ACT_NONE, want_preact=False, out_f32=False, emit8=None):
    """problem for y = act(x @ w^T + bias); returns (problem, y, preact).  ``emit8`` = (y8, qscale, amax): also
    write y as e4m3 (see p_fwd8)."""
    M, K, a_rs = _rows(_chk(x))
    N = w.shape[0]
    assert w.shape[1] == K and w.dtype == x.dtype and w.is_contiguous()
    y = torch.empty((M, N), device=x.device, dtype=F32 if out_f32 else x.dtype)
    pre = torch.empty((M, N), device=x.device, dtype=x.dtype) if want_preact else None
    p = _problem(x, w, y, M, N, K, a_rs, 1, K, 1, N, bias=bias, preact=pre, act=act, c_f32=out_f32)
    if emit8 is not None:
        y8, q, amax = emit8
        assert y8.shape == y.shape and y8.element_size() == 1 and y8.is_contiguous() and x.dtype == BF16 and not out_f32
        p.c8, p.c8_qscale, p.c8_amax = ptr(y8), ptr(q), ptr(amax)
        p.amax_slots = amax.numel() if amax is not None else 0  # a table entry spread over several floats (fp8.AMAX_SLOTS)
        p.keep = p.keep + (y8, q, amax)
    return p, y, pre


def p_fwd_splitk(x, w, S):
    """problem for the S partial products of y = x @ w^T over K / S wide slices of the reduction, fp32 [S, M, N]
    (the batch dimension of the GEMM walks the slices); summed by the consumer (``LnFwdReq``).  For long-K
    products with few tiles (FFN output: K = 3072, N = 768): S times the workgroups, 1 / S of the k-loop each."""
    M, K, a_rs = _rows(_chk(x))
    N = w.shape[0]
    assert w.shape[1] == K and w.dtype == x.dtype and w.is_contiguous()
    if K % (64 * S):
        raise RuntimeError("p_fwd_splitk: K = %d is not a multiple of 64 * %d" % (K, S))
    part = torch.empty((S, M, N), device=x.device, dtype=F32)
    p = _problem(x, w, part, M, N, K // S, a_rs, 1, K, 1, N, c_f32=True)
    p.batch, p.a_bs, p.b_bs, p.c_bs = S, K // S, K // S, M * N
    return p, part


def p_fwd8(x8, w8, sx, sw, bias=None, act=ACT_NONE, want_preact=False, emit8=None, split=0):
    """problem for y = act(sx * sw * (x8 @ w8^T) + bias) with e4m3 operands x8 [M, K], w8 [N, K] (1-byte tensors, k
    contiguous); ``sx`` / ``sw``: 1-element fp32 device tensors (reciprocal quantisation scales).  ``emit8`` =
    (y8, qscale, amax): the producer also writes y as e4m3 (operand of the next fp8 product).  ``split`` > 1: the
    partial products over K / split wide slices as fp32 [split, M, N] (see p_fwd_splitk).
    Returns (problem, y, preact)."""
    M, K, a_rs = _rows(_chk(x8))
    N = w8.shape[0]
    assert w8.shape[1] == K and x8.element_size() == 1 and w8.element_size() == 1 and w8.stride(1) == 1
    if split > 1:
        if K % (128 * split):
            raise RuntimeError("p_fwd8: K = %d is not a multiple of 128 * %d" % (K, split))
        y = torch.empty((split, M, N), device=x8.device, dtype=F32)
        p = _problem(x8, w8, y, M, N, K // split, a_rs, 1, w8.stride(0), 1, N, c_f32=True)
        p.batch, p.a_bs, p.b_bs, p.c_bs = split, K // split, K // split, M * N
        pre = None
    else:
        y = torch.empty((M, N), device=x8.device, dtype=BF16)
        pre = torch.empty((M, N), device=x8.device, dtype=BF16) if want_preact else None
        p = _problem(x8, w8, y, M, N, K, a_rs, 1, w8.stride(0), 1, N, bias=bias, preact=pre, act=act)
    p.scale_a, p.scale_b = ptr(sx), ptr(sw)
    p.keep = p.keep + (sx, sw)
    if emit8 is not None:
        y8, q, amax = emit8
        assert y8.shape == y.shape and y8.element_size() == 1 and y8.is_contiguous()
        p.c8, p.c8_qscale, p.c8_amax = ptr(y8), ptr(q), ptr(amax)
        p.amax_slots = amax.numel() if amax is not None else 0  # a table entry spread over several floats (fp8.AMAX_SLOTS)
        p.keep = p.keep + (y8, q, amax)
    return p, y, pre


GROUP_MAX = 6  # MAX_GROUP of gemm.hip: problems one grouped launch takes


def gemm_group8(problems, tile=0):
    """``gemm_group`` for e4m3 forward products (p_fwd8)."""
    gemm_group("e4m3", problems, tile)


def p_dgrad(dy, w, residual=None, gelu_aux=None, colsum=None, into=None, defer=None):
    """problem for dx = dy @ w (+ residual) (* gelu'(aux)); ``colsum`` (fp32 [K]) += column sums of dx
    (the bias gradient of the Linear that produced the activation) -- the epilogue leaves one partial row per 32
    output rows, a reduce job adds them to ``colsum`` in a fixed order: appended to ``defer`` (the backward pass's
    list, see functional.Runtime.defer_list) or, without one, run by ``gemm_group`` right behind the launch;
    ``into``: an existing gradient of the same input, the result is ADDED to it (second consumer of one tensor);
    returns (problem, dx)."""
    M, N, a_rs = _rows(_chk(dy))
    K = w.shape[1]
    assert w.shape[0] == N and w.dtype == dy.dtype and w.is_contiguous()
    if into is not None:
        assert tuple(into.shape) == (M, K) and into.dtype == dy.dtype and into.is_contiguous()
        assert gelu_aux is None and colsum is None
        return _problem(dy, w, into, M, K, N, a_rs, 1, 1, K, K, residual=residual, accumulate=True), into
    dx = torch.empty((M, K), device=dy.device, dtype=dy.dtype)
    part = job = None
    if colsum is not None:
        _c(colsum, F32, "colsum")
        assert colsum.numel() == K
        if K % 4:
            raise RuntimeError("p_dgrad: column sums need a width that is a multiple of 4 (got %d)" % K)
        part = torch.empty((colsum_rows(M), K), device=dy.device, dtype=F32)
        job = (part, colsum_rows(M), 1, K, (colsum,))
    p = _problem(dy, w, dx, M, K, N, a_rs, 1, 1, K, K, residual=residual, aux=gelu_aux,
                 act=ACT_GELU_GRAD if gelu_aux is not None else ACT_NONE, colsum=part)
    if job is not None:
        if defer is not None:
            defer.append(job)
        else:
            p.post = job
    return p, dx


def p_wgrad(dy, x, gw, accumulate, sqsum=None):
    """problem for gw (+)= dy^T @ x (fp32).  ``sqsum``: fp32 [ceil(N/64) * ceil(K/64)] slots that receive the sums of
    squares of the stored gradient per 64 x 64 block (tuned bf16 kernels only), or None."""
    M, N, dy_rs = _rows(_chk(dy))
    M2, K, x_rs = _rows(_chk(x))
    assert M2 == M and x.dtype == dy.dtype and tuple(gw.shape) == (N, K) and gw.is_contiguous()
    assert gw.dtype == F32 or gw.dtype == dy.dtype  # bf16: the data-parallel wire arena
    p = _problem(dy, x, gw, N, K, M, 1, dy_rs, 1, x_rs, K, c_f32=gw.dtype == F32, accumulate=accumulate)
    if sqsum is not None:
        _c(sqsum, F32, "sqsum slots")
        assert sqsum.numel() == ((N + 63) // 64) * ((K + 63) // 64)
        p.sqsum = ptr(sqsum)
        p.keep = p.keep + (sqsum,)
    return p


# ---- measured tile choice -----------------------------------------------------------------------
# The library picks the tile of a grouped launch from a fitted cost model (gemm.hip: pick_group_tile).  Where a
# measurement on the hardware disagrees, the measurement wins: ``gemm_tiles_gfx950.json`` (written by tools/tune_gemm.py
# from in-step timings of every distinct launch of the training iteration under every tile) maps a launch SIGNATURE --
# shapes and operand layouts of its problems -- to the tile that was fastest; unknown signatures keep the model's choice.
# The tile changes speed, not values: every tile walks k in the same order and the column sums are taken per 32 output
# rows whatever the tile, so products, gradients and bias gradients are bit-identical under every tile (tests); only the
# 64 x 64 norm slots add their squares in a tile-dependent -- fixed -- order, i.e. the clip norm can differ in its last
# bit between two TABLES.  The table is part of the configuration: one table, one set of bits.
def _load_tile_table():
    import json
    import os
    path = os.environ.get("XGGM_TILE_TABLE") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "gemm_tiles_gfx950.json")
    if os.environ.get("XGGM_TILE_TABLE") == "0" or not os.path.exists(path):
        return {}
    try:
        return {k: int(v) for k, v in json.load(open(path)).get("tiles", {}).items()}
    except (ValueError, OSError):
        return {}


TILE_TABLE = _load_tile_table()
TILE_HOOK = None  # tools/tune_gemm.py: callable(dt, chunk, signature, problem array) -> tile pin (or None) run in front of every launch


def gemm_signature(dt, chunk):
    """what the tile choice of a grouped launch may depend on: per problem M x N x K (x batch), which operands have
    the reduction index contiguous, fp32 output, the epilogue's extras"""
    parts = []
    for p in chunk:
        ext = ("f" if p.c_f32 else "") + ("a" if p.accumulate else "") + ("r" if p.residual else "") + \
              ("g" if p.act == ACT_GELU_GRAD else ("G" if p.act == ACT_GELU else "")) + ("c" if p.colsum else "")
        parts.append("%dx%dx%d%s:%d%d%s" % (p.M, p.N, p.K, ("b%d" % p.batch) if p.batch != 1 else "", int(p.a_ks == 1),
                                            int(p.b_ks == 1), ext))
    return (dt if isinstance(dt, str) else sfx(dt)) + "|" + "+".join(parts)


def gemm_group(dt, problems, tile=0):
    """launch up to GROUP_MAX independent products in one grid (more: consecutive groups).  ``dt``: the storage type, or
    "e4m3" for forward products with e4m3 operands (p_fwd8).  The tile travels with the launch: ``tile`` if given, else
    the measured table's entry for the launch's signature, else 0 = the library chooses (xggm.h: argument ``tile``)."""
    name = "xggm_gemm_grouped_" + ("fp8e4m3" if dt == "e4m3" else sfx(dt))
    for i in range(0, len(problems), GROUP_MAX):
        chunk = problems[i:i + GROUP_MAX]
        arr = (GemmProblem * len(chunk))(*chunk)
        pin = tile
        if TILE_TABLE or TILE_HOOK is not None:
            sig = gemm_signature(dt, chunk)
            pin = tile or TILE_TABLE.get(sig, 0)
            if TILE_HOOK is not None:
                pin = TILE_HOOK(dt, chunk, sig, arr) or pin
        call(name, _ct.cast(arr, _ct.c_void_p), len(chunk), pin, stream())
        reduce_batch([p.post for p in chunk if getattr(p, "post", None) is not None])  # column sums nobody deferred


def colsum(x, out):
    """out[n] += sum_m x[m, n]  (fp32 accumulator)."""
    M, N, ld = _rows(_chk(x))
    _c(out, F32, "colsum out")
    assert out.numel() == N
    ws, nb = _ws(_lib.lib.xggm_colsum_workspace_bytes(M, N), x.device)
    call("xggm_colsum_" + sfx(x.dtype), ptr(x), ptr(out), M, N, ld, ptr(ws), nb, stream())


def bmm_nt(a, b, out_f32=True, into=None):
    """out[z] = a[z] @ b[z]^T for contiguous a [Z,M,K], b [Z,N,K] -> [Z,M,N].  ``into``: an existing [Z,M,N] result the
    product is ADDED to (returned)."""
    Z, M, K = a.shape
    Z2, N, K2 = b.shape
    assert Z == Z2 and K == K2 and a.dtype == b.dtype
    _c(a), _c(b)
    if into is not None:
        _c(into, F32 if out_f32 else a.dtype)
        assert tuple(into.shape) == (Z, M, N)
        out = into
    else:
        out = torch.empty((Z, M, N), device=a.device, dtype=F32 if out_f32 else a.dtype)
    gemm_raw(a.dtype, a, b, out, M, N, K, K, 1, K, 1, N, batch=Z, a_bs=M * K, b_bs=N * K, c_bs=M * N,
             c_f32=out_f32, accumulate=into is not None)
    return out


# ----------------------------------------------------------------------------- attention
def attn_fwd(q, k, v, mask, B, heads, Sq, Sk, p, rng, sid):
    """q/k/v: 2-D row views [B*S, heads*64] with unit inner stride (may be slices of a fused
    QKV buffer).  Returns ctx [B*Sq, heads*64]."""
    d = 64
    H = heads * d
    for t, S in ((q, Sq), (k, Sk), (v, Sk)):
        _chk(t)
        if t.dim() != 2 or t.shape[0] != B * S or t.shape[1] != H or t.stride(1) != 1:
            raise RuntimeError("attn_fwd: bad operand shape %s" % (tuple(t.shape),))
    if mask is not None:
        _c(mask, F32, "mask")
        assert tuple(mask.shape) == (B, Sk)
    out = torch.empty((B * Sq, H), device=q.device, dtype=q.dtype)
    call("xggm_attn_fwd_" + sfx(q.dtype), ptr(q), ptr(k), ptr(v), ptr(mask), ptr(out), B, heads, Sq, Sk, d,
         q.stride(0), k.stride(0), v.stride(0), H, 0.125, float(p), ptr(rng), sid, stream())
    return out


def _bias_partials(B, H, dev, dbq, dbk, dbv):
    """workspace [B][3][H] the attention backward leaves the per-sample column sums of dq / dk / dv in, and the reduce
    job that adds them into the q / k / v bias gradients (fixed order: no atomics)"""
    if dbq is None and dbk is None:
        return None, None
    for t in (dbq, dbk, dbv):
        if t is not None:
            _c(t, F32, "bias gradient")
            assert t.numel() == H
    ws = torch.empty((B, 3, H), device=dev, dtype=F32)
    return ws, (ws, B, 3, H, (dbq, dbk, dbv))


def attn_bwd(q, k, v, mask, d_out, dq, dk, dv, B, heads, Sq, Sk, p, rng, sid, dbq=None, dbk=None, dbv=None):
    """dbq/dbk/dbv: fp32 [heads*64] accumulators of the query/key/value bias gradients"""
    d = 64
    H = heads * d
    _c(d_out)
    assert tuple(d_out.shape) == (B * Sq, H) and d_out.dtype == q.dtype
    for t, S in ((dq, Sq), (dk, Sk), (dv, Sk)):
        if t.dim() != 2 or t.shape[0] != B * S or t.shape[1] != H or t.stride(1) != 1 or t.dtype != q.dtype:
            raise RuntimeError("attn_bwd: bad gradient buffer %s" % (tuple(t.shape),))
    ws, job = _bias_partials(B, H, q.device, dbq, dbk, dbv)
    call("xggm_attn_bwd_" + sfx(q.dtype), ptr(q), ptr(k), ptr(v), ptr(mask), ptr(d_out), ptr(dq), ptr(dk),
         ptr(dv), B, heads, Sq, Sk, d, q.stride(0), k.stride(0), v.stride(0), H, dq.stride(0),
         dk.stride(0), dv.stride(0), 0.125, float(p), ptr(rng), sid,
         ptr(ws[0, 0]) if (ws is not None and dbq is not None) else None,
         ptr(ws[0, 1]) if (ws is not None and dbk is not None) else None,
         ptr(ws[0, 2]) if (ws is not None and dbv is not None) else None, 3 * H, stream())
    if job is not None:
        reduce_batch([job])


class AttnProblem(_ct.Structure):
    """mirror of ``xggm_attn_problem`` (include/xggm.h)"""
    _fields_ = [("q", _ct.c_void_p), ("k", _ct.c_void_p), ("v", _ct.c_void_p), ("mask", _ct.c_void_p), ("out", _ct.c_void_p),
                ("B", _ct.c_int), ("heads", _ct.c_int), ("Sq", _ct.c_int), ("Sk", _ct.c_int),
                ("q_rs", _ct.c_int64), ("k_rs", _ct.c_int64), ("v_rs", _ct.c_int64), ("o_rs", _ct.c_int64),
                ("scale", _ct.c_float), ("p", _ct.c_float), ("sid", _ct.c_uint32),
                ("d_out", _ct.c_void_p), ("dq", _ct.c_void_p), ("dk", _ct.c_void_p), ("dv", _ct.c_void_p),
                ("dq_rs", _ct.c_int64), ("dk_rs", _ct.c_int64), ("dv_rs", _ct.c_int64),
                ("dbq", _ct.c_void_p), ("dbk", _ct.c_void_p), ("dbv", _ct.c_void_p), ("db_bs", _ct.c_int64),
                ("out8", _ct.c_void_p), ("qscale", _ct.c_void_p), ("amax", _ct.c_void_p), ("amax_slots", _ct.c_int)]


class AttnFwdReq:
    """attention core forward handed to ``functional.drive`` (see LnFwdReq).  Result: ``out``."""

    def __init__(self, q, k, v, mask, B, heads, Sq, Sk, p, rng, sid, emit8=None):
        """``emit8`` = (qscale, amax): 1-element fp32 device tensors; the context is then ALSO written as e4m3
        (``out8``), the operand of the fp8 output projection"""
        d = 64
        H = heads * d
        for t, S in ((q, Sq), (k, Sk), (v, Sk)):
            _chk(t)
            if t.dim() != 2 or t.shape[0] != B * S or t.shape[1] != H or t.stride(1) != 1:
                raise RuntimeError("attn_fwd: bad operand shape %s" % (tuple(t.shape),))
        if mask is not None:
            _c(mask, F32, "mask")
            assert tuple(mask.shape) == (B, Sk)
        self.key = ("attn_fwd", q.dtype)
        self.rng = rng
        self.out = torch.empty((B * Sq, H), device=q.device, dtype=q.dtype)
        self.out8 = None
        self.keep = (q, k, v, mask)
        self.prob = AttnProblem(ptr(q), ptr(k), ptr(v), ptr(mask), ptr(self.out), B, heads, Sq, Sk, q.stride(0), k.stride(0),
                                v.stride(0), H, 0.125, float(p), sid, None, None, None, None, 0, 0, 0, None, None, None)
        if emit8 is not None:
            self.out8 = torch.empty((B * Sq, H), device=q.device, dtype=torch.uint8)
            self.prob.out8, self.prob.qscale, self.prob.amax = ptr(self.out8), ptr(emit8[0]), ptr(emit8[1])
            self.prob.amax_slots = emit8[1].numel() if emit8[1] is not None else 0
            self.keep = self.keep + tuple(emit8)


class AttnBwdReq:
    """attention core backward; gradients are written into the caller's dq/dk/dv views."""

    def __init__(self, q, k, v, mask, d_out, dq, dk, dv, B, heads, Sq, Sk, p, rng, sid, dbq=None, dbk=None, dbv=None,
                 defer=None):
        """``dbq / dbk / dbv``: the fp32 [heads*64] gradients of the query / key / value biases (+=); the kernel leaves
        per-sample partial rows and a reduce job adds them: appended to ``defer`` (the running backward's list) or kept in
        ``self.post`` for ``launch_row_requests`` to run right behind the launch"""
        d = 64
        H = heads * d
        _c(d_out)
        assert tuple(d_out.shape) == (B * Sq, H) and d_out.dtype == q.dtype
        for t, S in ((dq, Sq), (dk, Sk), (dv, Sk)):
            if t.dim() != 2 or t.shape[0] != B * S or t.shape[1] != H or t.stride(1) != 1 or t.dtype != q.dtype:
                raise RuntimeError("attn_bwd: bad gradient buffer %s" % (tuple(t.shape),))
        self.key = ("attn_bwd", q.dtype)
        self.rng = rng
        ws, job = _bias_partials(B, H, q.device, dbq, dbk, dbv)
        self.post = None
        if job is not None:
            if defer is not None:
                defer.append(job)
            else:
                self.post = job
        self.keep = (q, k, v, mask, d_out, dq, dk, dv, dbq, dbk, dbv, ws)
        self.prob = AttnProblem(ptr(q), ptr(k), ptr(v), ptr(mask), None, B, heads, Sq, Sk, q.stride(0), k.stride(0),
                                v.stride(0), H, 0.125, float(p), sid, ptr(d_out), ptr(dq), ptr(dk), ptr(dv), dq.stride(0),
                                dk.stride(0), dv.stride(0),
                                ptr(ws[0, 0]) if (ws is not None and dbq is not None) else None,
                                ptr(ws[0, 1]) if (ws is not None and dbk is not None) else None,
                                ptr(ws[0, 2]) if (ws is not None and dbv is not None) else None, 3 * H)


ROW_REQUESTS = ()  # filled below: the request classes ``functional.drive`` recognises


# ----------------------------------------------------------------------------- row kernels
def ln_fwd(x, bias, residual, gamma, beta, eps, p_pre=0.0, p_post=0.0, rng=None, sid_pre=0, sid_post=0,
           out=None, accumulate=False, out_scale=1.0, save=True):
    """Returns (out, z, stats).  ``z`` overwrites ``x`` in place when ``save``."""
    _c(x)
    M, H = x.shape
    _c(gamma, F32, "gamma"), _c(beta, F32, "beta")
    assert gamma.numel() == H and beta.numel() == H
    if bias is not None:
        _c(bias, F32, "bias")
        assert bias.numel() == H
    if residual is not None:
        _c(residual, x.dtype, "residual")
        assert residual.shape == x.shape
    if out is None:
        out = torch.empty_like(x)
    else:
        assert out.shape == x.shape and out.dtype == x.dtype and out.is_contiguous()
    stats = torch.empty((M, 2), device=x.device, dtype=F32) if save else None
    z = x if save else None
    call("xggm_ln_fwd_" + sfx(x.dtype), ptr(x), ptr(bias), ptr(residual), ptr(gamma), ptr(beta), ptr(out),
         ptr(z), ptr(stats), M, H, float(eps), float(p_pre), float(p_post), ptr(rng), sid_pre, sid_post,
         int(accumulate), float(out_scale), stream())
    return out, z, stats


class LnFwdProblem(_ct.Structure):
    """mirror of ``xggm_ln_fwd_problem`` (include/xggm.h)"""
    _fields_ = [("inp", _ct.c_void_p), ("bias", _ct.c_void_p), ("residual", _ct.c_void_p), ("gamma", _ct.c_void_p),
                ("beta", _ct.c_void_p), ("out", _ct.c_void_p), ("z_out", _ct.c_void_p), ("stats", _ct.c_void_p),
                ("M", _ct.c_int), ("sid_pre", _ct.c_uint32), ("sid_post", _ct.c_uint32), ("in_slabs", _ct.c_int),
                ("out8", _ct.c_void_p), ("qscale", _ct.c_void_p), ("amax", _ct.c_void_p), ("amax_slots", _ct.c_int)]


class LnBwdProblem(_ct.Structure):
    """mirror of ``xggm_ln_bwd_problem`` (include/xggm.h)"""
    _fields_ = [("dy", _ct.c_void_p), ("z", _ct.c_void_p), ("stats", _ct.c_void_p), ("gamma", _ct.c_void_p),
                ("d_in", _ct.c_void_p), ("d_res", _ct.c_void_p), ("dgamma", _ct.c_void_p), ("dbeta", _ct.c_void_p),
                ("dbias", _ct.c_void_p), ("gelu_aux", _ct.c_void_p), ("ws", _ct.c_void_p), ("ws_bytes", _ct.c_size_t),
                ("M", _ct.c_int), ("sid_pre", _ct.c_uint32), ("sid_post", _ct.c_uint32), ("accumulate_dres", _ct.c_int)]


class LnFwdReq:
    """a residual-LayerNorm forward a block generator hands to ``functional.drive``: requests of the
    same round (language + vision stream) are launched together.  Results: ``out``, ``z``, ``stats``."""

    def __init__(self, x, bias, residual, gamma, beta, eps, p_pre=0.0, rng=None, sid_pre=0, dtype=None, emit8=None):
        """``x``: [M, H] activations, or the fp32 split-K partial sums [S, M, H] of ``p_fwd_splitk`` (then
        ``dtype`` = the activation type of out / z / residual).  ``emit8`` = (qscale, amax): ``out`` is also
        written as e4m3 (``out8``), the operand of the next fp8 product."""
        _c(x)
        slabs = 0
        if x.dim() == 3:
            slabs, M, H = x.shape
            if x.dtype != F32 or dtype is None:
                raise RuntimeError("LnFwdReq: split-K input is fp32 [S, M, H] and needs the activation dtype")
        else:
            M, H = x.shape
            dtype = x.dtype
        _c(gamma, F32, "gamma"), _c(beta, F32, "beta")
        assert gamma.numel() == H and beta.numel() == H
        if bias is not None:
            _c(bias, F32, "bias")
            assert bias.numel() == H
        if residual is not None:
            _c(residual, dtype, "residual")
            assert tuple(residual.shape) == (M, H)
        self.key = ("ln_fwd", dtype, H, float(eps), float(p_pre))
        self.rng = rng
        self.out = torch.empty((M, H), device=x.device, dtype=dtype)
        self.z = torch.empty((M, H), device=x.device, dtype=dtype) if slabs else x  # pre-LN sum: in place when it can
        self.stats = torch.empty((M, 2), device=x.device, dtype=F32)
        self.keep = (x, bias, residual, gamma, beta)
        self.prob = LnFwdProblem(ptr(x), ptr(bias), ptr(residual), ptr(gamma), ptr(beta), ptr(self.out), ptr(self.z),
                                 ptr(self.stats), M, sid_pre, 0, slabs)
        self.out8 = None
        if emit8 is not None:
            assert dtype == BF16
            self.out8 = torch.empty((M, H), device=x.device, dtype=torch.uint8)
            self.prob.out8, self.prob.qscale, self.prob.amax = ptr(self.out8), ptr(emit8[0]), ptr(emit8[1])
            self.prob.amax_slots = emit8[1].numel() if emit8[1] is not None else 0
            self.keep = self.keep + tuple(emit8)


class LnBwdReq:
    """backward of LnFwdReq; ``defer`` as in ``ln_bwd``.  Results: ``d_in``, ``d_res``."""

    def __init__(self, dy, z, stats, gamma, dgamma, dbeta, dbias, p_pre=0.0, rng=None, sid_pre=0, defer=None):
        _c(dy), _c(z, dy.dtype)
        M, H = dy.shape
        assert z.shape == dy.shape and tuple(stats.shape) == (M, 2)
        for t in (dgamma, dbeta, dbias):
            if t is not None:
                _c(t, F32, "param grad")
                assert t.numel() == H
        self.key = ("ln_bwd", dy.dtype, H, float(p_pre))
        self.rng = rng
        self.d_in = torch.empty_like(dy)
        self.d_res = torch.empty_like(dy)
        ws, nb = _ws(_lib.lib.xggm_ln_bwd_workspace_bytes(M, H), dy.device)
        now = (dgamma, dbeta, dbias)
        if defer is not None and any(t is not None for t in now):
            defer.append((ws, nb // (12 * H), 3, H, now))
            now = (None, None, None)
        self.keep = (dy, z, stats, gamma, ws)
        self.prob = LnBwdProblem(ptr(dy), ptr(z), ptr(stats), ptr(gamma), ptr(self.d_in), ptr(self.d_res), ptr(now[0]),
                                 ptr(now[1]), ptr(now[2]), None, ptr(ws), nb, M, sid_pre, 0, 0)


class LnSumArgs(_ct.Structure):
    """mirror of ``xggm_ln_sum_args`` (include/xggm.h)"""
    _fields_ = [("inp", _ct.c_void_p * 4), ("gamma", _ct.c_void_p * 4), ("beta", _ct.c_void_p * 4), ("stats", _ct.c_void_p * 4),
                ("sid_post", _ct.c_uint32 * 4), ("out", _ct.c_void_p), ("n", _ct.c_int), ("M", _ct.c_int), ("H", _ct.c_int),
                ("eps", _ct.c_float), ("p_post", _ct.c_float), ("rng", _ct.c_void_p)]


def ln_sum_fwd(xs, gammas, betas, eps, p_post=0.0, rng=None, sids=None):
    """sum_k dropout(LayerNorm(xs[k])) for up to four [M, H] terms in ONE launch (the read-out of the graph blocks).
    Returns (out, [stats_k]); the saved pre-normalisation rows are ``xs`` themselves."""
    n = len(xs)
    assert 1 <= n <= 4 and len(gammas) == n and len(betas) == n
    M, H = xs[0].shape
    a = LnSumArgs()
    stats = []
    for k, (x, g, b) in enumerate(zip(xs, gammas, betas)):
        _c(x, xs[0].dtype), _c(g, F32, "gamma"), _c(b, F32, "beta")
        assert tuple(x.shape) == (M, H) and g.numel() == H and b.numel() == H
        st = torch.empty((M, 2), device=x.device, dtype=F32)
        stats.append(st)
        a.inp[k], a.gamma[k], a.beta[k], a.stats[k] = ptr(x), ptr(g), ptr(b), ptr(st)
        a.sid_post[k] = int(sids[k]) if sids is not None else 0
    out = torch.empty_like(xs[0])
    a.out, a.n, a.M, a.H, a.eps, a.p_post, a.rng = ptr(out), n, M, H, float(eps), float(p_post), ptr(rng)
    call("xggm_ln_sum_fwd_" + sfx(xs[0].dtype), _ct.byref(a), stream())
    return out, stats


def ln_bwd_group(items, p_pre=0.0, p_post=0.0, rng=None, out_scale=1.0):
    """several LayerNorm backwards with one H and one pair of dropout rates in ONE launch (xggm_ln_bwd_grouped_*, four
    problems per launch).  ``items``: dicts of the per-problem arguments of ``ln_bwd`` (dy, z, stats, gamma, dgamma, dbeta,
    dbias, and optionally want_din, want_dres, d_res, sid_pre, sid_post, gelu_aux, defer).  Returns [(d_in, d_res)]."""
    probs, outs, keep = [], [], []
    dt, H = items[0]["dy"].dtype, items[0]["dy"].shape[1]
    for it in items:
        dy, z, stats = it["dy"], it["z"], it["stats"]
        _c(dy, dt), _c(z, dt)
        M = dy.shape[0]
        assert dy.shape[1] == H and z.shape == dy.shape and tuple(stats.shape) == (M, 2)
        now = (it.get("dgamma"), it.get("dbeta"), it.get("dbias"))
        for t in now:
            if t is not None:
                _c(t, F32, "param grad")
                assert t.numel() == H
        d_in = torch.empty_like(dy) if it.get("want_din", True) else None
        d_res = it.get("d_res")
        acc = d_res is not None
        if it.get("want_dres", False) and d_res is None:
            d_res = torch.empty_like(dy)
        if d_res is not None:
            assert d_res.shape == dy.shape and d_res.dtype == dt and d_res.is_contiguous()
        ws, nb = _ws(_lib.lib.xggm_ln_bwd_workspace_bytes(M, H), dy.device)
        defer = it.get("defer")
        if defer is not None and any(t is not None for t in now):
            defer.append((ws, nb // (12 * H), 3, H, now))
            now = (None, None, None)
        probs.append(LnBwdProblem(ptr(dy), ptr(z), ptr(stats), ptr(it["gamma"]), ptr(d_in), ptr(d_res), ptr(now[0]), ptr(now[1]),
                                  ptr(now[2]), ptr(it.get("gelu_aux")), ptr(ws), nb, M, it.get("sid_pre", 0),
                                  it.get("sid_post", 0), int(acc)))
        outs.append((d_in, d_res))
        keep.append(ws)
    arr = (LnBwdProblem * len(probs))(*probs)
    call("xggm_ln_bwd_grouped_" + sfx(dt), _ct.cast(arr, _ct.c_void_p), len(probs), H, float(p_pre), float(p_post), ptr(rng),
         float(out_scale), None, stream())
    return outs


class Prefetch(_ct.Structure):
    """mirror of ``xggm_prefetch`` (include/xggm.h)"""
    _fields_ = [("ptr", _ct.c_void_p * 4), ("bytes", _ct.c_size_t * 4), ("n", _ct.c_int)]


PREFETCH = os.environ.get("XGGM_PREFETCH") != "0"  # read once; 0: no launch carries weight ranges


def prefetch_ranges(tensors):
    """the ``xggm_prefetch`` argument (or None) of a row launch that reads ``tensors`` (weight slices, or None) beside its
    work: each range from its first 16-byte border, those of 16 bytes or less after it skipped, four at most"""
    pf = Prefetch()
    for t in tensors if PREFETCH else ():
        a, n = (t.data_ptr(), t.numel() * t.element_size()) if t is not None else (0, 0)
        pad = (-a) % 16
        if n > pad + 16 and pf.n < 4:
            pf.ptr[pf.n], pf.bytes[pf.n] = a + pad, n - pad
            pf.n += 1
    return _ct.byref(pf) if pf.n else None


def launch_row_requests(reqs):
    """launch LnFwdReq / LnBwdReq / Attn*Req objects with their ``prefetch`` ranges, grouping those with equal key."""
    groups = {}
    for r in reqs:
        groups.setdefault(r.key, []).append(r)
    for key, rs in groups.items():
        pf = prefetch_ranges([t for r in rs for t in getattr(r, "prefetch", ())])
        if key[0] in ("attn_fwd", "attn_bwd"):
            arr = (AttnProblem * len(rs))(*[r.prob for r in rs])
            call("xggm_%s_grouped_%s" % (key[0], sfx(key[1])), _ct.cast(arr, _ct.c_void_p), len(rs), 64, ptr(rs[0].rng), pf,
                 stream())
            reduce_batch([r.post for r in rs if getattr(r, "post", None) is not None])
        elif key[0] == "ln_fwd":
            _, dt, H, eps, p = key
            arr = (LnFwdProblem * len(rs))(*[r.prob for r in rs])
            call("xggm_ln_fwd_grouped_" + sfx(dt), _ct.cast(arr, _ct.c_void_p), len(rs), H, eps, p, 0.0, ptr(rs[0].rng), 0,
                 1.0, pf, stream())
        else:
            _, dt, H, p = key
            arr = (LnBwdProblem * len(rs))(*[r.prob for r in rs])
            call("xggm_ln_bwd_grouped_" + sfx(dt), _ct.cast(arr, _ct.c_void_p), len(rs), H, p, 0.0, ptr(rs[0].rng), 1.0, pf,
                 stream())


ROW_REQUESTS = (LnFwdReq, LnBwdReq, AttnFwdReq, AttnBwdReq)


class ReduceJob(_ct.Structure):
    """mirror of ``xggm_reduce_job`` (include/xggm.h)"""
    _fields_ = [("ws", _ct.c_void_p), ("nblk", _ct.c_int), ("K", _ct.c_int), ("H", _ct.c_int),
                ("target", _ct.c_void_p * 3)]


REDUCE_JOBS_PER_LAUNCH = 72  # MAX_JOBS of rowops.hip: jobs one launch of xggm_partial_reduce_batch takes


def reduce_batch(jobs):
    """second stage of the two-stage parameter-gradient sums: ``jobs`` = [(ws, nblk, K, H, targets)] with ``ws`` fp32
    [nblk][K][H] partial rows and ``targets`` a tuple of K fp32 [H] gradient vectors (None = not wanted):
    targets[k] += sum_b ws[b][k][:], blocks added in index order.  The producers: LayerNorm backwards (K = 3: dgamma,
    dbeta, dbias), GEMM epilogue column sums (K = 1: a bias gradient), attention backwards (K = 3: q / k / v bias)."""
    if not jobs:
        return
    arr = (ReduceJob * len(jobs))()
    for a, (ws, nblk, K, H, tg) in zip(arr, jobs):
        assert 1 <= K <= 3 and len(tg) == K and ws.dtype == F32 and ws.numel() >= nblk * K * H
        a.ws, a.nblk, a.K, a.H = ptr(ws), nblk, K, H
        for k in range(3):
            a.target[k] = ptr(tg[k]) if k < K else None
    call("xggm_partial_reduce_batch", _ct.cast(arr, _ct.c_void_p), len(jobs), stream())


def colsum_rows(M):
    """partial rows the GEMM epilogue writes per column-sum request: one per block of 32 output rows (xggm.h)"""
    return (M + 31) // 32


def ln_bwd(dy, z, stats, gamma, dgamma, dbeta, dbias, want_din=True, want_dres=False, d_res=None,
           p_pre=0.0, p_post=0.0, rng=None, sid_pre=0, sid_post=0, out_scale=1.0, gelu_aux=None, defer=None):
    """Returns (d_in, d_res).  dgamma/dbeta/dbias (fp32, may be None) are accumulated.
    If ``d_res`` is given the residual gradient is ADDED into it.  ``gelu_aux`` = the
    pre-activation u when the LN input was gelu(u): d_in/dbias become grads of u.
    ``defer``: a list; the parameter-gradient sums are then left in the workspace and a job for
    ``reduce_batch`` is appended instead of running the second-stage kernel now."""
    _c(dy), _c(z, dy.dtype)
    M, H = dy.shape
    assert z.shape == dy.shape and tuple(stats.shape) == (M, 2)
    for t in (dgamma, dbeta, dbias):
        if t is not None:
            _c(t, F32, "param grad")
            assert t.numel() == H
    d_in = torch.empty_like(dy) if want_din else None
    acc = d_res is not None
    if want_dres and d_res is None:
        d_res = torch.empty_like(dy)
    if d_res is not None:
        assert d_res.shape == dy.shape and d_res.dtype == dy.dtype and d_res.is_contiguous()
    ws, nb = _ws(_lib.lib.xggm_ln_bwd_workspace_bytes(M, H), dy.device)
    now = (dgamma, dbeta, dbias)
    if defer is not None and any(t is not None for t in now):
        defer.append((ws, nb // (12 * H), 3, H, now))
        now = (None, None, None)
    call("xggm_ln_bwd_" + sfx(dy.dtype), ptr(dy), ptr(z), ptr(stats), ptr(gamma), ptr(d_in), ptr(d_res),
         ptr(now[0]), ptr(now[1]), ptr(now[2]), M, H, float(p_pre), float(p_post), ptr(rng), sid_pre, sid_post,
         float(out_scale), int(acc), ptr(gelu_aux), ptr(ws), nb, stream())
    return d_in, d_res


def _emit8_args(emit8, shape, device):
    """(out8, qscale ptr, amax ptr, slots) of a row kernel that also writes its output as e4m3; ``emit8`` = (qscale,
    amax) 1-element / slot-spread fp32 device tensors, or None"""
    if emit8 is None:
        return None, None, None, 0
    out8 = torch.empty(shape, device=device, dtype=torch.uint8)
    return out8, ptr(emit8[0]), ptr(emit8[1]), (emit8[1].numel() if emit8[1] is not None else 0)


SIDE_MAX, SIDE_ADDITIVE_MASK, SIDE_CAST_BF16 = 3, 1, 2


class _SideJob(_ct.Structure):
    _fields_ = [("kind", _ct.c_int), ("src", _ct.c_void_p), ("dst", _ct.c_void_p), ("count", _ct.c_int64)]


class SideJobs(_ct.Structure):
    """mirror of ``xggm_side_jobs`` (include/xggm.h)"""
    _fields_ = [("n", _ct.c_int), ("job", _SideJob * SIDE_MAX)]


def run_side_jobs(jobs):
    """the stand-alone launches of side jobs nobody carried: [(kind, src, dst)]"""
    for kind, src, dst in jobs:
        if kind == SIDE_ADDITIVE_MASK:
            call("xggm_additive_mask", ptr(src), ptr(dst), src.numel(), stream())
        else:
            call("xggm_cast_from_f32_bf16", ptr(src), ptr(dst), src.numel(), stream())


def embed_fwd(ids, seg, word, pos, typ, gamma, beta, eps, p, rng, sid, emit8=None, side=None):
    """``emit8`` = (qscale, amax): the output is also written as e4m3 (returned as a 4th value).  ``side``: up to three
    (kind, src, dst) pieces of the pass's input glue (SIDE_ADDITIVE_MASK: int64 mask -> fp32 additive mask;
    SIDE_CAST_BF16: fp32 -> bf16) done by workgroups appended to this launch (xggm_embed_fwd_side_*)."""
    B, T = ids.shape
    _c(ids, torch.int64, "input_ids")
    if seg is not None:
        _c(seg, torch.int64, "segment_ids")
        assert seg.shape == ids.shape
    H = word.shape[1]
    for t in (word, pos, typ):
        _c(t)
        assert t.shape[1] == H and t.dtype == word.dtype
    assert pos.shape[0] >= T, "sequence longer than the position table"
    out = torch.empty((B * T, H), device=word.device, dtype=word.dtype)
    z = torch.empty_like(out)
    stats = torch.empty((B * T, 2), device=word.device, dtype=F32)
    out8, q, am, slots = _emit8_args(emit8 if word.dtype == BF16 else None, (B * T, H), word.device)
    if side:
        assert len(side) <= SIDE_MAX
        sj = SideJobs()
        sj.n = len(side)
        for k, (kind, src, dst) in enumerate(side):
            _c(src, torch.int64 if kind == SIDE_ADDITIVE_MASK else F32), _c(dst, F32 if kind == SIDE_ADDITIVE_MASK else BF16)
            assert dst.numel() == src.numel()
            sj.job[k].kind, sj.job[k].src, sj.job[k].dst, sj.job[k].count = kind, ptr(src), ptr(dst), src.numel()
        call("xggm_embed_fwd_side_" + sfx(word.dtype), ptr(ids), ptr(seg), ptr(word), ptr(pos), ptr(typ), ptr(gamma),
             ptr(beta), ptr(out), ptr(z), ptr(stats), B * T, T, H, float(eps), float(p), ptr(rng), sid, ptr(out8), q, am, slots,
             _ct.byref(sj), stream())
    else:
        call("xggm_embed_fwd_" + sfx(word.dtype), ptr(ids), ptr(seg), ptr(word), ptr(pos), ptr(typ), ptr(gamma),
             ptr(beta), ptr(out), ptr(z), ptr(stats), B * T, T, H, float(eps), float(p), ptr(rng), sid, ptr(out8), q, am, slots,
             stream())
    if emit8 is not None:
        return out, z, stats, out8
    return out, z, stats


def embed_bwd(ids, seg, dy, z, stats, gamma, dword, dpos, dtyp, dgamma, dbeta, p, rng, sid, row_list=None):
    """``row_list`` = (ids int64 [cap], sq fp32 [cap], n int32 [1]), cap >= M: the kernel also lists the word-table rows it
    touched, |row|^2 of the gradient per owner and the count (xggm_embed_bwd_listed_*)"""
    B, T = ids.shape
    M, H = dy.shape
    _c(dy), _c(z, dy.dtype)
    for t in (dword, dpos, dtyp, dgamma, dbeta):
        _c(t, F32, "embedding grad")
    dz = torch.empty_like(dy)
    ws, nb = _ws(_lib.lib.xggm_ln_bwd_workspace_bytes(M, H), dy.device)
    if row_list is None:
        call("xggm_embed_bwd_" + sfx(dy.dtype), ptr(ids), ptr(seg), ptr(dy), ptr(z), ptr(stats), ptr(gamma),
             ptr(dz), ptr(dword), ptr(dpos), ptr(dtyp), ptr(dgamma), ptr(dbeta), M, T, H, float(p), ptr(rng), sid,
             ptr(ws), nb, stream())
        return
    rid, rsq, rn = row_list
    _c(rid, torch.int64), _c(rsq, F32), _c(rn, torch.int32)
    assert rid.numel() >= M and rsq.numel() >= M
    call("xggm_embed_bwd_listed_" + sfx(dy.dtype), ptr(ids), ptr(seg), ptr(dy), ptr(z), ptr(stats), ptr(gamma),
         ptr(dz), ptr(dword), ptr(dpos), ptr(dtyp), ptr(dgamma), ptr(dbeta), M, T, H, float(p), ptr(rng), sid,
         ptr(ws), nb, ptr(rid), ptr(rsq), ptr(rn), stream())


def visn_embed_fwd(u, bf, boxes, Wb, bb, g1, b1, g2, b2, eps, p, rng, sid, emit8=None):
    """``emit8`` = (qscale, amax): the output is also written as e4m3 (returned as a 5th value)"""
    _c(u), _c(boxes, u.dtype, "boxes")
    M, H = u.shape
    assert tuple(boxes.shape) == (M, 4) and tuple(Wb.shape) == (H, 4)
    for t in (bf, Wb, bb, g1, b1, g2, b2):
        _c(t, F32, "visn_fc parameter")
    out = torch.empty_like(u)
    z2 = torch.empty_like(u)
    stats = torch.empty((M, 4), device=u.device, dtype=F32)
    out8, q, am, slots = _emit8_args(emit8 if u.dtype == BF16 else None, (M, H), u.device)
    call("xggm_visn_embed_fwd_" + sfx(u.dtype), ptr(u), ptr(bf), ptr(boxes), ptr(Wb), ptr(bb), ptr(g1),
         ptr(b1), ptr(g2), ptr(b2), ptr(out), ptr(u), ptr(z2), ptr(stats), M, H, float(eps), float(p), ptr(rng),
         sid, ptr(out8), q, am, slots, stream())
    if emit8 is not None:
        return out, u, z2, stats, out8
    return out, u, z2, stats


def visn_embed_bwd(dy, z1, z2, stats, boxes, g1, g2, grads, p, rng, sid):
    """grads: dict with fp32 accumulators dbf, dg1, db1, dWb, dbb, dg2, db2.  Returns du."""
    _c(dy)
    M, H = dy.shape
    du = torch.empty_like(dy)
    ws, nb = _ws(_lib.lib.xggm_visn_embed_bwd_workspace_bytes(M, H), dy.device)
    call("xggm_visn_embed_bwd_" + sfx(dy.dtype), ptr(dy), ptr(z1), ptr(z2), ptr(stats), ptr(boxes), ptr(g1),
         ptr(g2), ptr(du), ptr(grads["dbf"]), ptr(grads["dg1"]), ptr(grads["db1"]), ptr(grads["dWb"]),
         ptr(grads["dbb"]), ptr(grads["dg2"]), ptr(grads["db2"]), M, H, float(p), ptr(rng), sid, ptr(ws), nb,
         stream())
    return du


# ----------------------------------------------------------------------------- graph kernels
SHORT_N = 64  # objects the graph kernels of graph.hip / gat.hip / preprocess.hip take; 65..128: the _long twins (graph_long.hip)


def _lg(name, N, long, suffix=""):
    """symbol of a graph kernel: the ``_long`` twin only when the caller opted in AND N > 64.  N <= 64 always runs
    today's kernel (same launches, same bits); N > 64 without the opt-in reaches today's entry point and its refusal."""
    return name + ("_long" if long and N > SHORT_N else "") + suffix


def aggregate(Mx, x, mode=AGG_PLAIN, scale=1.0, scale_ptr=None, self_w=0.0, out=None, long=False):
    """out = [out +] self_w*x + scale*(1+*scale_ptr) * M' @ x.  Mx fp32 [B,N,N], x T [B,N,H]."""
    _c(Mx, F32, "adjacency"), _c(x)
    B, N, H = x.shape
    assert tuple(Mx.shape) == (B, N, N), "adjacency %s vs nodes %s" % (tuple(Mx.shape), tuple(x.shape))
    acc = out is not None
    if out is None:
        out = torch.empty_like(x)
    else:
        assert out.shape == x.shape and out.dtype == x.dtype and out.is_contiguous()
    call(_lg("xggm_aggregate", N, long, "_" + sfx(x.dtype)), ptr(Mx), ptr(x), ptr(out), B, N, H, mode, float(scale),
         ptr(scale_ptr), float(self_w), int(acc), stream())
    return out


def agg_residual_ln(Mx, y, res, gamma, beta, eps):
    """LayerNorm(res + Mx @ y) per sample in ONE launch (bf16 [B, N, H], H in 64 / 128 / 256 / 768, N <= 64): GCNConv's
    tail once y = x W^T has been taken (xggm_agg_residual_ln_bf16).  Returns (out, z, stats) as ``ln_fwd`` does."""
    _c(Mx, F32, "adjacency"), _c(y, BF16), _c(res, BF16), _c(gamma, F32, "gamma"), _c(beta, F32, "beta")
    B, N, H = y.shape
    assert tuple(Mx.shape) == (B, N, N) and res.shape == y.shape and gamma.numel() == H and beta.numel() == H
    out, z = torch.empty_like(y), torch.empty_like(y)
    stats = torch.empty((B * N, 2), device=y.device, dtype=F32)
    call("xggm_agg_residual_ln_bf16", ptr(Mx), ptr(y), ptr(res), ptr(gamma), ptr(beta), ptr(out), ptr(z), ptr(stats), B, N, H,
         float(eps), stream())
    return out, z, stats


def agg_residual_ln_ok(x, N):
    """shapes the fused GCNConv tail is built for"""
    return x.dtype == BF16 and x.shape[-1] in (64, 128, 256, 768) and N <= 64


def agg_dot(Mx, x, dh, out, long=False):
    B, N, H = x.shape
    _c(Mx, F32), _c(x), _c(dh, x.dtype), _c(out, F32)
    assert tuple(Mx.shape) == (B, N, N) and dh.shape == x.shape
    call(_lg("xggm_agg_dot", N, long, "_" + sfx(x.dtype)), ptr(Mx), ptr(x), ptr(dh), ptr(out), B, N, H, ptr(sum_ws(x.device)), stream())


def adj_regen_fwd(S, long=False):
    _c(S, F32, "S")
    B, N, _ = S.shape
    adj = torch.empty_like(S)
    colmax = torch.empty((B, N), device=S.device, dtype=F32)
    argmax = torch.empty((B, N), device=S.device, dtype=torch.int32)
    call(_lg("xggm_adj_regen", N, long, "_fwd"), ptr(S), ptr(adj), ptr(colmax), ptr(argmax), B, N, stream())
    return adj, colmax, argmax


def adj_regen_bwd(d_adj, S, adj, colmax, argmax, long=False):
    _c(d_adj, F32, "d_adj")
    B, N, _ = S.shape
    assert d_adj.shape == S.shape
    dS = torch.empty_like(S)
    call(_lg("xggm_adj_regen", N, long, "_bwd"), ptr(d_adj), ptr(S), ptr(adj), ptr(colmax), ptr(argmax), ptr(dS), B, N, stream())
    return dS


def adj_init_fwd(e, N, sigma, randn=None, rng=None, sid=0, B=None, want_gradlog=True, long=False):
    if e is not None:
        _c(e, F32, "encoder_adj output")
        B = e.shape[0]
        assert e.shape[1] == N * (N - 1) // 2, "encoder_adj width %d != N(N-1)/2" % e.shape[1]
    dev = e.device if e is not None else (randn.device if randn is not None else rng.device)
    if randn is not None:
        _c(randn, F32, "randn")
        assert tuple(randn.shape) == (B, N, N)
    adj = torch.empty((B, N, N), device=dev, dtype=F32)
    g = torch.empty_like(adj) if want_gradlog else None
    call(_lg("xggm_adj_init", N, long, "_fwd"), ptr(e), ptr(randn), ptr(adj), ptr(g), B, N, float(sigma), ptr(rng), sid, stream())
    return adj, g


def adj_init_bwd(d_adj, long=False):
    _c(d_adj, F32, "d_adj")
    B, N, _ = d_adj.shape
    d_e = torch.empty((B, N * (N - 1) // 2), device=d_adj.device, dtype=F32)
    call(_lg("xggm_adj_init", N, long, "_bwd"), ptr(d_adj), ptr(d_e), B, N, stream())
    return d_e


def feature_noise(x, sigma, randn=None, rng=None, sid=0):
    _c(x)
    if randn is not None:
        _c(randn, F32, "randn")
        assert randn.shape == x.shape
    out = torch.empty_like(x)
    g = torch.empty(x.shape, device=x.device, dtype=F32)
    call("xggm_feature_noise_" + sfx(x.dtype), ptr(x), ptr(randn), ptr(out), ptr(g), x.numel(), float(sigma),
         ptr(rng), sid, stream())
    return out, g


def pool_concat_fwd(x, nodes):
    _c(x), _c(nodes, x.dtype)
    B, N, H = nodes.shape
    assert tuple(x.shape) == (B, H)
    out = torch.empty((B, 2 * H), device=x.device, dtype=x.dtype)
    call("xggm_pool_concat_fwd_" + sfx(x.dtype), ptr(x), ptr(nodes), ptr(out), B, N, H, stream())
    return out


def pool_concat_bwd(d_out, out, N):
    _c(d_out), _c(out, d_out.dtype)
    B, H2 = out.shape
    H = H2 // 2
    dx = torch.empty((B, H), device=out.device, dtype=out.dtype)
    dn = torch.empty((B, N, H), device=out.device, dtype=out.dtype)
    call("xggm_pool_concat_bwd_" + sfx(out.dtype), ptr(d_out), ptr(out), ptr(dx), ptr(dn), B, N, H, 0, stream())
    return dx, dn


def bcast_rows(x, N):
    _c(x)
    B, H = x.shape
    out = torch.empty((B, N, H), device=x.device, dtype=x.dtype)
    call("xggm_bcast_rows_" + sfx(x.dtype), ptr(x), ptr(out), B, N, H, stream())
    return out


def sum_rows(g):
    _c(g)
    B, N, H = g.shape
    out = torch.empty((B, H), device=g.device, dtype=g.dtype)
    call("xggm_sum_rows_" + sfx(g.dtype), ptr(g), ptr(out), B, N, H, stream())
    return out


# ----------------------------------------------------------------------------- losses
def zeros_f32(n, device):
    """n zeroed floats from ONE custom launch (no framework fill kernel inside a captured pass)"""
    m = (n + 3) // 4 * 4
    t = torch.empty(m, device=device, dtype=F32)
    zero_ranges(t, [(0, m)])
    return t[:n]


def _scalar(out, device):
    """the 0-dim accumulator of a loss kernel: a caller-provided zeroed slot, or a fresh zeroed one"""
    return out.view(()) if out is not None else zeros_f32(1, device).view(())


SUM_WS_FLOATS = 4104  # XGGM_SUM_WS_FLOATS (include/xggm.h)
_SUM_WS = {}
_SUM_WS_HOME = {}


def sum_ws(device):
    """workspace of the grid-wide sums without atomics (losses, GIN's eps gradient): per-workgroup partials + an
    arrival counter every kernel leaves at zero, so ONE zeroed buffer per device serves every launch -- the package
    launches all its kernels on one stream, and launches of one stream run in order.  Created on first use;
    ``functional.Runtime`` touches it at construction so that it exists before any graph capture."""
    device = torch.device(device)
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    ws = _SUM_WS.get(device)
    if ws is None:
        ws = _SUM_WS[device] = torch.zeros(SUM_WS_FLOATS, device=device, dtype=F32)
        _SUM_WS_HOME[device] = torch.cuda.current_stream(device).cuda_stream
        return ws
    # launches on ANOTHER stream (an evaluation beside the training stream, tools/exp_two_streams.py) may overlap the
    # home stream's: two kernels sharing the arrival counter corrupt it for good (no workgroup ever draws the last ticket
    # again).  Every other stream gets a workspace of its own; a capture keeps the home one (its graph replays where the
    # trainer runs, and allocating inside a capture would tie the buffer to the graph's pool).
    sid = torch.cuda.current_stream(device).cuda_stream
    if sid == _SUM_WS_HOME[device] or torch.cuda.is_current_stream_capturing():
        return ws
    key = (device, sid)
    side = _SUM_WS.get(key)
    if side is None:
        side = _SUM_WS[key] = torch.zeros(SUM_WS_FLOATS, device=device, dtype=F32)
    return side


def dsm_fwd(s, g, coef, out=None):
    _c(s), _c(g, F32, "grad_log_noise")
    assert s.shape == g.shape
    loss = _scalar(out, s.device)
    call("xggm_dsm_loss_fwd_" + sfx(s.dtype), ptr(s), ptr(g), ptr(loss), s.numel(), float(coef), ptr(sum_ws(s.device)),
         stream())
    return loss


def dsm_bwd(s, g, gout, coef):
    ds = torch.empty_like(s)
    call("xggm_dsm_loss_bwd_" + sfx(s.dtype), ptr(s), ptr(g), ptr(gout), ptr(ds), s.numel(), float(coef), stream())
    return ds


def symkl_fwd(x, y, coef, out=None):
    _c(x), _c(y, x.dtype)
    assert x.shape == y.shape
    W = x.shape[-1]
    loss = _scalar(out, x.device)
    call("xggm_symkl_" + sfx(x.dtype), ptr(x), ptr(y), ptr(loss), None, None, None, x.numel() // W, W,
         float(coef), 0, ptr(sum_ws(x.device)), stream())
    return loss


def symkl_bwd(x, y, gout, coef, need_x, need_y):
    W = x.shape[-1]
    dx = torch.empty_like(x) if need_x else None
    dy = torch.empty_like(y) if need_y else None
    call("xggm_symkl_" + sfx(x.dtype), ptr(x), ptr(y), None, ptr(gout), ptr(dx), ptr(dy), x.numel() // W, W,
         float(coef), 0, None, stream())
    return dx, dy


def bce_fwd(logit, target, coef, out=None):
    _c(logit, F32, "logit"), _c(target, F32, "target")
    assert logit.shape == target.shape
    loss = _scalar(out, logit.device)
    call("xggm_bce_fwd", ptr(logit), ptr(target), ptr(loss), logit.numel(), float(coef), ptr(sum_ws(logit.device)), stream())
    return loss


def bce_bwd(logit, target, gout, coef, dt):
    dl = torch.empty(logit.shape, device=logit.device, dtype=dt)
    call("xggm_bce_bwd_" + sfx(dt), ptr(logit), ptr(target), ptr(gout), ptr(dl), logit.numel(), float(coef), stream())
    return dl


DEBIAS_REWEIGHT, DEBIAS_BIAS_PRODUCT, DEBIAS_LEARNED_MIXIN = 1, 2, 3  # XGGM_DEBIAS_* (include/xggm.h)


class DebiasArgs(_ct.Structure):
    """mirror of ``xggm_debias_args`` (include/xggm.h)"""
    _fields_ = [("logits", _ct.c_void_p), ("labels", _ct.c_void_p), ("bias", _ct.c_void_p), ("bias_row_stride", _ct.c_int64),
                ("bias_rows", _ct.c_int64), ("bias_index", _ct.c_void_p), ("hidden", _ct.c_void_p), ("Hd", _ct.c_int),
                ("lin_w", _ct.c_void_p), ("lin_b", _ct.c_void_p), ("smooth_param", _ct.c_void_p),
                ("constant_smooth", _ct.c_float), ("w", _ct.c_float), ("kind", _ct.c_int), ("B", _ct.c_int), ("A", _ct.c_int),
                ("loss", _ct.c_void_p), ("save", _ct.c_void_p), ("ws", _ct.c_void_p), ("gout", _ct.c_void_p),
                ("d_logit", _ct.c_void_p), ("dlogit_f32", _ct.c_int), ("d_hidden", _ct.c_void_p), ("d_lin_w", _ct.c_void_p),
                ("d_lin_b", _ct.c_void_p), ("d_smooth", _ct.c_void_p), ("part", _ct.c_void_p), ("accumulate", _ct.c_int)]


class DebiasProblem:
    """the operands of one debias loss (``debias_fwd`` makes it, ``debias_bwd`` reads it): checked on the host once"""

    def __init__(self, kind, logits, labels, bias, bias_index, hidden, lin_w, lin_b, smooth_param, constant_smooth, w):
        _c(logits, F32, "logits"), _c(labels, F32, "labels"), _chk(bias, F32, "bias")
        if logits.dim() != 2 or labels.shape != logits.shape:
            raise ValueError("debias: logits %s and labels %s must be one [B, A]" % (tuple(logits.shape), tuple(labels.shape)))
        B, A = logits.shape
        rows, ba, ld = _rows(bias)
        if ba != A or (rows > 1 and ld < A):
            raise ValueError("debias: bias %s does not have the %d answers of the logits" % (tuple(bias.shape), A))
        if bias_index is not None:
            _c(bias_index, torch.int64, "bias_index")
            if bias_index.numel() != B:
                raise ValueError("debias: bias_index holds %d entries for %d samples" % (bias_index.numel(), B))
        elif rows != B:
            raise ValueError("debias: bias has %d rows for %d samples (a prior table needs bias_index)" % (rows, B))
        self.kind, self.B, self.A, self.Hd = int(kind), B, A, 0
        self.dt = F32
        if kind == DEBIAS_LEARNED_MIXIN:
            if hidden is None or lin_w is None or lin_b is None:
                raise ValueError("debias: LearnedMixin needs hidden, bias_lin.weight and bias_lin.bias")
            _c(hidden), _c(lin_w, F32, "bias_lin.weight"), _c(lin_b, F32, "bias_lin.bias")
            self.dt, self.Hd = hidden.dtype, hidden.shape[-1]
            sfx(self.dt)
            if hidden.dim() != 2 or hidden.shape[0] != B or lin_w.numel() != self.Hd or lin_b.numel() != 1:
                raise ValueError("debias: hidden %s, bias_lin.weight %s, bias_lin.bias %s do not fit %d samples"
                                 % (tuple(hidden.shape), tuple(lin_w.shape), tuple(lin_b.shape), B))
        else:
            hidden = lin_w = lin_b = None
        if smooth_param is not None:
            _c(smooth_param, F32, "smooth_param")
            assert smooth_param.numel() == 1
        for t in (labels, bias, bias_index, hidden, lin_w, lin_b, smooth_param):
            if t is not None and t.device != logits.device:
                raise RuntimeError("debias: all operands must live on one device")
        self.t = dict(logits=logits, labels=labels, bias=bias, bias_index=bias_index, hidden=hidden, lin_w=lin_w, lin_b=lin_b,
                      smooth_param=smooth_param)
        self.bias_ld, self.bias_rows = max(ld, A), rows
        self.constant_smooth, self.w = float(constant_smooth), float(w)
        self.save = None

    def args(self):
        a, t = DebiasArgs(), self.t
        for k, v in t.items():
            setattr(a, k, ptr(v))
        a.bias_row_stride, a.bias_rows, a.Hd = self.bias_ld, self.bias_rows, self.Hd
        a.constant_smooth, a.w, a.kind, a.B, a.A = self.constant_smooth, self.w, self.kind, self.B, self.A
        a.save = ptr(self.save)
        return a


def debias_fwd(kind, logits, labels, bias, bias_index=None, hidden=None, lin_w=None, lin_b=None, smooth_param=None,
               constant_smooth=0.0, w=0.0, out=None, save=None):
    """ReweightByInvBias / BiasProduct / LearnedMixin (``DEBIAS_*``) on fp32 logits, labels and bias; contract:
    xggm_debias_fwd_* in xggm.h.  One launch.  -> (0-dim loss, DebiasProblem for ``debias_bwd``).  ``out``: a zeroed
    1-element slot to accumulate into; ``save``: the per-row buffer (2 B floats) when the caller owns it."""
    pr = DebiasProblem(kind, logits, labels, bias, bias_index, hidden, lin_w, lin_b, smooth_param, constant_smooth, w)
    if save is None:
        save = torch.empty(2 * pr.B, device=logits.device, dtype=F32)
    _c(save, F32, "save")
    assert save.numel() >= 2 * pr.B
    pr.save = save
    loss = _scalar(out, logits.device)
    a = pr.args()
    a.loss, a.ws = ptr(loss), ptr(sum_ws(logits.device))
    call("xggm_debias_fwd_" + sfx(pr.dt), _ct.addressof(a), stream())
    return loss, pr


def debias_bwd(pr, gout=None, need_hidden=True, need_params=True, dlogit_dtype=None, targets=None):
    """backward of ``debias_fwd``: -> (d_logit, d_hidden | None, d_lin_w | None, d_lin_b | None, d_smooth | None).
    ``dlogit_dtype``: F32, or None = the dtype of hidden (the kernel's suffix).  ``targets`` = (d_lin_w, d_lin_b,
    d_smooth) fp32 tensors (None entries where the loss has no such parameter) the parameter gradients are ADDED to --
    the arena's cleared vector gradients; None: fresh tensors, overwritten.  One launch, two with parameter gradients."""
    t, dev = pr.t, pr.t["logits"].device
    mixin = pr.kind == DEBIAS_LEARNED_MIXIN
    dl_dt = pr.dt if dlogit_dtype is None else dlogit_dtype
    if dl_dt not in (pr.dt, F32):
        raise TypeError("debias_bwd: d_logit is %s or float32" % pr.dt)
    a = pr.args()
    d_logit = torch.empty((pr.B, pr.A), device=dev, dtype=dl_dt)
    a.d_logit, a.dlogit_f32 = ptr(d_logit), int(dl_dt == F32)
    if gout is not None:
        a.gout = ptr(_c(gout, F32, "gout"))
    d_hidden = torch.empty_like(t["hidden"]) if (mixin and need_hidden) else None
    a.d_hidden = ptr(d_hidden)
    d_w = d_b = d_s = part = None
    if need_params and (mixin or t["smooth_param"] is not None):
        if targets is not None:
            d_w, d_b, d_s = targets
            a.accumulate = 1
        else:
            d_w = torch.empty(pr.Hd, device=dev, dtype=F32) if mixin else None
            d_b = torch.empty(1, device=dev, dtype=F32) if mixin else None
            d_s = torch.empty(1, device=dev, dtype=F32) if t["smooth_param"] is not None else None
        if not mixin:
            d_w = d_b = None
        if t["smooth_param"] is None:
            d_s = None
        for x, n, name in ((d_w, pr.Hd, "d bias_lin.weight"), (d_b, 1, "d bias_lin.bias"), (d_s, 1, "d smooth_param")):
            if x is not None:
                _c(x, F32, name)
                assert x.numel() == n and x.device == dev
        part = torch.empty(2 * pr.B, device=dev, dtype=F32)
        a.d_lin_w, a.d_lin_b, a.d_smooth, a.part = ptr(d_w), ptr(d_b), ptr(d_s), ptr(part)
    call("xggm_debias_bwd_" + sfx(pr.dt), _ct.addressof(a), stream())
    return d_logit, d_hidden, d_w, d_b, d_s


SOFTMAX_FOCAL, SOFTMAX_CE = 1, 2  # XGGM_SOFTMAX_* (include/xggm.h)


class SoftmaxLossArgs(_ct.Structure):
    """mirror of ``xggm_softmax_loss_args`` (include/xggm.h)"""
    _fields_ = [("logits", _ct.c_void_p), ("labels", _ct.c_void_p), ("label_index", _ct.c_void_p), ("bias", _ct.c_void_p),
                ("bias_row_stride", _ct.c_int64), ("bias_rows", _ct.c_int64), ("bias_index", _ct.c_void_p),
                ("ignore_index", _ct.c_int64), ("scale", _ct.c_float), ("kind", _ct.c_int), ("B", _ct.c_int), ("A", _ct.c_int),
                ("loss", _ct.c_void_p), ("ws", _ct.c_void_p), ("save", _ct.c_void_p), ("gout", _ct.c_void_p),
                ("d_logit", _ct.c_void_p), ("accumulate", _ct.c_int)]


class SoftmaxLossProblem:
    """the operands of one softmax answer loss (``softmax_loss_fwd`` makes it, ``softmax_loss_bwd`` reads it): checked on
    the host once.  ``save``: what the forward left for the backward (5 B + 1 floats, xggm.h)."""

    def __init__(self, kind, logits, labels, label_index, bias, bias_index, ignore_index, scale):
        _c(logits, F32, "logits")
        if logits.dim() != 2:
            raise ValueError("softmax_loss: logits %s must be [B, A]" % (tuple(logits.shape),))
        B, A = logits.shape
        if kind not in (SOFTMAX_FOCAL, SOFTMAX_CE):
            raise ValueError("softmax_loss: unknown kind %r" % (kind,))
        if labels is not None:
            _c(labels, F32, "labels")
            if labels.shape != logits.shape:
                raise ValueError("softmax_loss: labels %s do not fit logits %s" % (tuple(labels.shape), tuple(logits.shape)))
        if label_index is not None:
            _c(label_index, torch.int64, "label_index")
            if kind != SOFTMAX_CE or label_index.numel() != B:
                raise ValueError("softmax_loss: label_index is cross-entropy's [B] int64 (%d entries, %d samples)"
                                 % (label_index.numel(), B))
        if kind == SOFTMAX_CE:
            if labels is None and label_index is None:
                raise ValueError("softmax_loss: cross-entropy needs labels [B, A] or label_index [B]")
            bias = bias_index = None
        elif labels is None or bias is None:
            raise ValueError("softmax_loss: Focal needs labels and bias")
        self.bias_ld = self.bias_rows = 0
        if bias is not None:
            _chk(bias, F32, "bias")
            rows, ba, ld = _rows(bias)
            if ba != A or (rows > 1 and ld < A):
                raise ValueError("softmax_loss: bias %s does not have the %d answers of the logits" % (tuple(bias.shape), A))
            if bias_index is not None:
                _c(bias_index, torch.int64, "bias_index")
                if bias_index.numel() != B:
                    raise ValueError("softmax_loss: bias_index holds %d entries for %d samples" % (bias_index.numel(), B))
            elif rows != B:
                raise ValueError("softmax_loss: bias has %d rows for %d samples (a prior table needs bias_index)" % (rows, B))
            self.bias_ld, self.bias_rows = max(ld, A), rows
        for t in (labels, label_index, bias, bias_index):
            if t is not None and t.device != logits.device:
                raise RuntimeError("softmax_loss: all operands must live on one device")
        self.kind, self.B, self.A = int(kind), B, A
        self.ignore_index, self.scale = int(ignore_index), float(scale)
        self.t = dict(logits=logits, labels=labels, label_index=label_index, bias=bias, bias_index=bias_index)
        self.save = None

    def args(self):
        a = SoftmaxLossArgs()
        for k, v in self.t.items():
            setattr(a, k, ptr(v))
        a.bias_row_stride, a.bias_rows, a.ignore_index, a.scale = self.bias_ld, self.bias_rows, self.ignore_index, self.scale
        a.kind, a.B, a.A, a.save = self.kind, self.B, self.A, ptr(self.save)
        return a

    def labels_int32(self):
        """the int32 label per row the forward left in ``save`` (cross-entropy; -1: ignored)"""
        return self.save[4 * self.B:5 * self.B].view(torch.int32)

    def n_valid(self):
        return self.save[5 * self.B]


def softmax_loss_fwd(kind, logits, labels=None, label_index=None, bias=None, bias_index=None, ignore_index=-1, scale=1.0,
                     out=None, save=None):
    """Focal / cross-entropy (``SOFTMAX_*``) on fp32 logits; contract: xggm_softmax_loss_fwd_f32 in xggm.h.  One launch.
    -> (0-dim loss, SoftmaxLossProblem for ``softmax_loss_bwd``).  ``out``: a zeroed 1-element slot to accumulate into;
    ``save``: the 5 B + 1 floats between forward and backward when the caller owns them."""
    pr = SoftmaxLossProblem(kind, logits, labels, label_index, bias, bias_index, ignore_index, scale)
    if save is None:
        save = torch.empty(5 * pr.B + 1, device=logits.device, dtype=F32)
    _c(save, F32, "save")
    assert save.numel() >= 5 * pr.B + 1 and save.device == logits.device
    pr.save = save
    loss = _scalar(out, logits.device)
    a = pr.args()
    a.loss, a.ws = ptr(loss), ptr(sum_ws(logits.device))
    call("xggm_softmax_loss_fwd_f32", _ct.addressof(a), stream())
    return loss, pr


def softmax_loss_bwd(pr, gout, d_logit=None):
    """backward of ``softmax_loss_fwd``: -> d_logit [B, A] fp32 (``*gout`` x d loss / d logits; exactly 0 on the rows
    cross-entropy ignores).  ``d_logit``: an existing fp32 [B, A] gradient to ADD to (None: a fresh tensor, overwritten).
    One launch."""
    a = pr.args()
    if d_logit is None:
        d_logit = torch.empty((pr.B, pr.A), device=pr.t["logits"].device, dtype=F32)
    else:
        _c(d_logit, F32, "d_logit")
        assert tuple(d_logit.shape) == (pr.B, pr.A) and d_logit.device == pr.t["logits"].device
        a.accumulate = 1
    a.d_logit, a.gout = ptr(d_logit), ptr(_c(gout, F32, "gout"))
    call("xggm_softmax_loss_bwd_f32", _ct.addressof(a), stream())
    return d_logit


# ----------------------------------------------------------------------------- pre-training heads (LXRTPretraining)
VISUAL_CE, VISUAL_L2, VISUAL_MAX_JOBS = 1, 2, 3  # XGGM_VISUAL_* (include/xggm.h)
VOCAB_CE_REG_MAX = 32768  # XGGM_VOCAB_CE_REG_MAX: the longest row the forward keeps in registers
VOCAB_CE_FWD_GRID, VOCAB_CE_BWD_GRID, VISUAL_LOSS_GRID = 1024, 2048, 128  # XGGM_*_GRID: rows beyond them are walked
MLM_SELECT_MAX_ROWS = 65536  # XGGM_MLM_SELECT_MAX_ROWS


class MlmSelectArgs(_ct.Structure):
    """mirror of ``xggm_mlm_select_args`` (include/xggm.h)"""
    _fields_ = [("labels", _ct.c_void_p), ("x", _ct.c_void_p), ("M", _ct.c_int), ("H", _ct.c_int), ("cap", _ct.c_int),
                ("V", _ct.c_int), ("ignore_index", _ct.c_int64), ("row_index", _ct.c_void_p), ("label", _ct.c_void_p),
                ("n", _ct.c_void_p), ("overflow", _ct.c_void_p), ("out", _ct.c_void_p)]


class VocabCeArgs(_ct.Structure):
    """mirror of ``xggm_vocab_ce_args`` (include/xggm.h)"""
    _fields_ = [("logits", _ct.c_void_p), ("label", _ct.c_void_p), ("n", _ct.c_void_p), ("overflow", _ct.c_void_p),
                ("cap", _ct.c_int), ("V", _ct.c_int), ("ld", _ct.c_int64), ("loss", _ct.c_void_p), ("ws", _ct.c_void_p),
                ("save", _ct.c_void_p), ("gout", _ct.c_void_p)]


class VisualJob(_ct.Structure):
    """mirror of ``xggm_visual_job`` (include/xggm.h)"""
    _fields_ = [("kind", _ct.c_int), ("W", _ct.c_int), ("scores", _ct.c_void_p), ("label_index", _ct.c_void_p),
                ("target", _ct.c_void_p), ("mask_conf", _ct.c_void_p), ("weight", _ct.c_float), ("loss", _ct.c_void_p),
                ("d_score", _ct.c_void_p)]


class VisualLossArgs(_ct.Structure):
    """mirror of ``xggm_visual_loss_args`` (include/xggm.h)"""
    _fields_ = [("job", VisualJob * VISUAL_MAX_JOBS), ("n_jobs", _ct.c_int), ("R", _ct.c_int), ("ignore_index", _ct.c_int64),
                ("ws", _ct.c_void_p), ("save", _ct.c_void_p), ("gout", _ct.c_void_p)]


def vocab_ld(V, dt):
    """row stride of masked-LM logits of ``V`` columns: the next multiple of 16 bytes (30522 -> 30528)"""
    g = 16 // torch.empty((), dtype=dt).element_size()
    return (int(V) + g - 1) // g * g


class MlmSelection:
    """what ``mlm_select`` left on the device: ``row_index`` / ``label`` int32 [cap], ``n`` and ``overflow`` int32 [1], the
    gathered rows ``x`` [cap, H]; nothing of it is read by the host"""

    def __init__(self, M, H, cap, V, row_index, label, n, overflow, x):
        self.M, self.H, self.cap, self.V = M, H, cap, V
        self.row_index, self.label, self.n, self.overflow, self.x = row_index, label, n, overflow, x


def mlm_select(labels, x, cap, V, ignore_index=-1, overflow=None):
    """rows of ``x`` [M, H] whose ``labels`` [M] (int64) count, compacted in ascending row order into ``cap`` slots;
    contract: xggm_mlm_select_* in xggm.h.  One launch, no host read.  ``overflow``: an int32 [1] flag the caller owns."""
    _c(labels, torch.int64, "masked_lm_labels"), _c(x)
    sfx(x.dtype)
    if x.dim() != 2 or labels.numel() != x.shape[0]:
        raise ValueError("mlm_select: %d labels for activations %s" % (labels.numel(), tuple(x.shape)))
    M, H = x.shape
    cap, V = int(cap), int(V)
    if cap <= 0 or V <= 0:
        raise ValueError("mlm_select: capacity %d and vocabulary %d must be positive" % (cap, V))
    if M > MLM_SELECT_MAX_ROWS:
        raise ValueError("mlm_select: %d rows, at most %d (every workgroup counts the labels in front of its chunk)"
                         % (M, MLM_SELECT_MAX_ROWS))
    if (H * x.element_size()) % 16:
        raise ValueError("mlm_select: rows of %d bytes are no multiple of 16" % (H * x.element_size()))
    if labels.device != x.device:
        raise RuntimeError("mlm_select: all operands must live on one device")
    dev = x.device
    idx = torch.empty(2 * cap + 1, device=dev, dtype=torch.int32)
    if overflow is None:
        overflow = torch.empty(1, device=dev, dtype=torch.int32)
    _c(overflow, torch.int32, "overflow")
    out = torch.empty((cap, H), device=dev, dtype=x.dtype)
    a = MlmSelectArgs()
    a.labels, a.x, a.M, a.H, a.cap, a.V, a.ignore_index = ptr(labels), ptr(x), M, H, cap, V, int(ignore_index)
    sel = MlmSelection(M, H, cap, V, idx[:cap], idx[cap:2 * cap], idx[2 * cap:], overflow, out)
    a.row_index, a.label, a.n, a.overflow, a.out = ptr(sel.row_index), ptr(sel.label), ptr(sel.n), ptr(overflow), ptr(out)
    call("xggm_mlm_select_" + sfx(x.dtype), _ct.addressof(a), stream())
    return sel


def mlm_scatter(sel, src):
    """backward of the gather of ``mlm_select``: -> [M, H] with row j of ``src`` [cap, H] at row ``row_index[j]``, exact
    zeros elsewhere.  One launch."""
    _c(src)
    if tuple(src.shape) != (sel.cap, sel.H) or src.device != sel.n.device:
        raise ValueError("mlm_scatter: src %s does not fit the selection [%d, %d]" % (tuple(src.shape), sel.cap, sel.H))
    out = torch.empty((sel.M, sel.H), device=src.device, dtype=src.dtype)
    call("xggm_mlm_scatter_" + sfx(src.dtype), ptr(src), ptr(sel.row_index), ptr(sel.n), ptr(out), sel.M, sel.H, sel.cap,
         stream())
    return out


class VocabCeProblem:
    """the operands of one masked-LM cross-entropy (``vocab_ce_fwd`` makes it, ``vocab_ce_bwd`` reads it): checked on the
    host once.  ``logits`` [cap, ld] with ld >= V a multiple of 16 bytes (``vocab_ld``); a [cap, V] view of such a buffer
    is what the decoder's product writes."""

    def __init__(self, logits, label, n, V, overflow):
        _chk(logits)
        sfx(logits.dtype)
        cap, cols, ld = _rows(logits)
        V = int(V)
        if cols != V and cols != ld:
            raise ValueError("vocab_ce: logits %s are neither the [cap, V] view nor the padded [cap, ld] buffer (V=%d)"
                             % (tuple(logits.shape), V))
        if cap == 1:
            ld = max(ld, cols)
        g = 16 // logits.element_size()
        if V <= 0 or ld < V or ld % g:
            raise ValueError("vocab_ce: row stride %d must be >= V=%d and a multiple of %d elements" % (ld, V, g))
        _c(label, torch.int32, "label"), _c(n, torch.int32, "n")
        if label.numel() != cap or n.numel() != 1:
            raise ValueError("vocab_ce: %d labels and %d counters for %d rows" % (label.numel(), n.numel(), cap))
        if overflow is not None:
            _c(overflow, torch.int32, "overflow")
        for t in (label, n, overflow):
            if t is not None and t.device != logits.device:
                raise RuntimeError("vocab_ce: all operands must live on one device")
        self.cap, self.V, self.ld = cap, V, ld
        self.t = dict(logits=logits, label=label, n=n, overflow=overflow)
        self.save = None

    def args(self):
        a = VocabCeArgs()
        for k, v in self.t.items():
            setattr(a, k, ptr(v))
        a.cap, a.V, a.ld, a.save = self.cap, self.V, self.ld, ptr(self.save)
        return a


def vocab_ce_fwd(logits, label, n, V, overflow=None, out=None):
    """cross-entropy over the vocabulary on compacted rows (fp32 or bf16 logits); contract: xggm_vocab_ce_fwd_* in xggm.h.
    One launch.  -> (0-dim loss, VocabCeProblem for ``vocab_ce_bwd``).  ``out``: a zeroed 1-element slot to accumulate into."""
    pr = VocabCeProblem(logits, label, n, V, overflow)
    pr.save = torch.empty(2 * pr.cap, device=logits.device, dtype=F32)
    loss = _scalar(out, logits.device)
    a = pr.args()
    a.loss, a.ws = ptr(loss), ptr(sum_ws(logits.device))
    call("xggm_vocab_ce_fwd_" + sfx(logits.dtype), _ct.addressof(a), stream())
    return loss, pr


def vocab_ce_bwd(pr, gout):
    """backward of ``vocab_ce_fwd``: OVERWRITES the logits with ``*gout`` (p - onehot) / n in their own dtype (exact zeros
    on rows >= n and in the padding columns) and returns them.  One launch."""
    a = pr.args()
    a.gout = ptr(_c(gout, F32, "gout"))
    call("xggm_vocab_ce_bwd_" + sfx(pr.t["logits"].dtype), _ct.addressof(a), stream())
    return pr.t["logits"]


class VisualLossProblem:
    """the jobs of one object-loss launch (``visual_loss_fwd`` makes it, ``visual_loss_bwd`` reads it): checked on the host
    once.  ``jobs``: up to three of (kind, scores [R, W], label, mask_conf [R] fp32, weight) with label = int64 [R] class
    indices for ``VISUAL_CE`` and fp32 [R, W] targets for ``VISUAL_L2``."""

    def __init__(self, jobs, ignore_index):
        if not 1 <= len(jobs) <= VISUAL_MAX_JOBS:
            raise ValueError("visual_loss: %d jobs (1 to %d per launch)" % (len(jobs), VISUAL_MAX_JOBS))
        self.jobs, self.R, self.dt, dev = [], None, None, None
        for kind, scores, label, conf, weight in jobs:
            if kind not in (VISUAL_CE, VISUAL_L2):
                raise ValueError("visual_loss: unknown kind %r" % (kind,))
            _c(scores), _c(conf, F32, "mask_conf")
            if scores.dim() != 2:
                raise ValueError("visual_loss: scores %s must be [R, W]" % (tuple(scores.shape),))
            R, W = scores.shape
            if self.R is None:
                self.R, self.dt, dev = R, scores.dtype, scores.device
                sfx(self.dt)
            if R != self.R or scores.dtype != self.dt or conf.numel() != R:
                raise ValueError("visual_loss: every job has the same rows and dtype (%s %s, %d confidences; R=%d %s)"
                                 % (tuple(scores.shape), scores.dtype, conf.numel(), self.R, self.dt))
            if kind == VISUAL_CE:
                _c(label, torch.int64, "label")
                if label.numel() != R:
                    raise ValueError("visual_loss: %d labels for %d rows" % (label.numel(), R))
            else:
                _c(label, F32, "target")
                if label.numel() != R * W:
                    raise ValueError("visual_loss: target %s does not fit scores %s" % (tuple(label.shape), tuple(scores.shape)))
            if label.device != dev or conf.device != dev or scores.device != dev:
                raise RuntimeError("visual_loss: all operands must live on one device")
            self.jobs.append((int(kind), W, scores, label, conf, float(weight)))
        self.ignore_index = int(ignore_index)
        self.device = dev
        self.save = None

    def args(self, losses=None, d_scores=None):
        a = VisualLossArgs()
        for q, (kind, W, scores, label, conf, weight) in enumerate(self.jobs):
            j = a.job[q]
            j.kind, j.W, j.scores, j.mask_conf, j.weight = kind, W, ptr(scores), ptr(conf), weight
            if kind == VISUAL_CE:
                j.label_index = ptr(label)
            else:
                j.target = ptr(label)
            if losses is not None:
                j.loss = losses[q:].data_ptr()
            if d_scores is not None:
                j.d_score = ptr(d_scores[q])
        a.n_jobs, a.R, a.ignore_index, a.save = len(self.jobs), self.R, self.ignore_index, ptr(self.save)
        return a


def visual_loss_fwd(jobs, ignore_index=-1, out=None):
    """the object losses of pre-training, up to three per launch; contract: xggm_visual_loss_fwd_* in xggm.h.
    -> (losses fp32 [len(jobs)], VisualLossProblem for ``visual_loss_bwd``).  ``out``: zeroed slots to accumulate into."""
    pr = VisualLossProblem(jobs, ignore_index)
    pr.save = torch.empty(2 * VISUAL_MAX_JOBS * pr.R, device=pr.device, dtype=F32)
    losses = out if out is not None else zeros_f32(len(pr.jobs), pr.device)
    _c(losses, F32, "losses")
    assert losses.numel() == len(pr.jobs) and losses.device == pr.device
    a = pr.args(losses=losses)
    a.ws = ptr(sum_ws(pr.device))
    call("xggm_visual_loss_fwd_" + sfx(pr.dt), _ct.addressof(a), stream())
    return losses, pr


def visual_loss_bwd(pr, gout):
    """backward of ``visual_loss_fwd``: -> the d_score [R, W] of every job, in the scores' dtype.  One launch."""
    ds = [torch.empty_like(j[2]) for j in pr.jobs]
    a = pr.args(d_scores=ds)
    a.gout = ptr(_c(gout, F32, "gout"))
    call("xggm_visual_loss_bwd_" + sfx(pr.dt), _ct.addressof(a), stream())
    return ds


# ----------------------------------------------------------------------------- optimiser / utils
def zero_ranges(buf, ranges, rows=None):
    """zero buf[s:e] for up to 16 (s, e) element ranges per launch (all float4-aligned).  ``rows`` = (table [R, H] fp32,
    ids int64 [cap], n int32 [1]): the first launch also zeroes rows ids[:n] of the table (device-side list, as
    ``embed_bwd(..., row_list=...)`` left it)."""
    _c(buf, F32)
    rs = [(s, e) for s, e in ranges if e > s]
    for i in range(0, max(len(rs), 1 if rows is not None else 0), 16):
        chunk = rs[i:i + 16]
        offs = (_ct.c_int64 * max(len(chunk), 1))(*[s for s, _ in chunk])
        lens = (_ct.c_int64 * max(len(chunk), 1))(*[e - s for s, e in chunk])
        if rows is not None and i == 0:
            table, ids, n = rows
            _c(table, F32), _c(ids, torch.int64), _c(n, torch.int32)
            assert table.dim() == 2
            call("xggm_zero_ranges_rows_f32", ptr(buf), _ct.cast(offs, _ct.c_void_p), _ct.cast(lens, _ct.c_void_p), len(chunk),
                 ptr(table), ptr(ids), ptr(n), ids.numel(), table.shape[0], table.shape[1], stream())
        else:
            call("xggm_zero_ranges_f32", ptr(buf), _ct.cast(offs, _ct.c_void_p), _ct.cast(lens, _ct.c_void_p), len(chunk), stream())


_SQNORM_WS = {}


def _norm_ws(device):
    """the device's XGGM_SQNORM_WS_FLOATS floats of scratch for the norm entries' partial sums (xggm.h)"""
    ws = _SQNORM_WS.get(device)
    if ws is None:
        ws = _SQNORM_WS[device] = torch.zeros(4100, device=device, dtype=F32)
    return ptr(ws)


def _span_arrays(spans):
    """(offsets, lengths) of [(start, end)] as host int64 arrays, as pointers (never empty arrays)"""
    n = max(len(spans), 1)
    return (_ct.cast((_ct.c_int64 * n)(*[s for s, _ in spans]), _ct.c_void_p),
            _ct.cast((_ct.c_int64 * n)(*[e - s for s, e in spans]), _ct.c_void_p))


def sqnorm(g, out):
    """out += sum g^2 (fixed summation order: see xggm.h)."""
    _c(g, F32), _c(out, F32)
    call("xggm_sqnorm_f32", ptr(g), g.numel(), ptr(out), _norm_ws(g.device), stream())


def sqnorm_multi(buf, spans, out, norm=None, overwrite=True, square=True, mul=1.0):
    """out (1 fp32) = [out +] sum over the (start, end) element ranges ``spans`` of buf^2 (``square`` False: of buf),
    fixed summation order; ``norm`` (1 fp32 or None) = sqrt(out).  Any number of ranges (16 per launch pair; none:
    only seeds / finishes)."""
    _c(buf, F32), _c(out, F32)
    if norm is not None:
        _c(norm, F32)
    rs = [(s, e) for s, e in spans if e > s]
    chunks = [rs[i:i + 16] for i in range(0, len(rs), 16)] or [[]]
    for ci, ch in enumerate(chunks):
        offs, lens = _span_arrays(ch)
        last = ci == len(chunks) - 1
        call("xggm_sqnorm_multi_f32", ptr(buf), offs, lens, len(ch), ptr(out), ptr(norm) if last else None,
             _norm_ws(buf.device), int(overwrite and ci == 0), int(square), float(mul) if last else 1.0, stream())


class FpSpan(_ct.Structure):
    """mirror of ``xggm_fp_span`` (include/xggm.h)"""
    _fields_ = [("ptr", _ct.c_void_p), ("bytes", _ct.c_int64), ("salt", _ct.c_uint32), ("pad", _ct.c_uint32)]


_FP_WS = {}
FP_MAX_WORKGROUPS = 4096  # largest ``max_workgroups`` fingerprint_spans takes: the cached workspace is sized for it, once


def fingerprint_workspace(device, max_workgroups=FP_MAX_WORKGROUPS):
    """a workspace of one's own for ``fingerprint_spans(ws=...)`` (int64 tensor)"""
    nb = _lib.lib.xggm_fingerprint_workspace_bytes(1, int(max_workgroups))
    return torch.empty((nb + 7) // 8, device=device, dtype=torch.int64)


def fingerprint_spans(spans, device, out=None, max_workgroups=0, ws=None):
    """64-bit fingerprints (contract: xggm_fingerprint_spans in xggm.h) of the byte ranges ``spans`` = [(device
    pointer, bytes, salt)] on ``device`` -> int64 tensor [len(spans)] (the uint64 words' bit patterns), every word
    written.  One grid for all ranges + one finishing launch.  ``ws`` None: the workspace cached per device -- made ONCE,
    at the first eager call (inside a stream capture an allocation would belong to that graph's pool), for the largest
    ``max_workgroups`` there is (FP_MAX_WORKGROUPS), and never replaced, so a captured call keeps a valid pointer.  It
    serves calls that are ordered against each other (one stream, or a graph and the stream it is replayed on); calls
    that may run side by side on different streams pass their own ``ws`` (``fingerprint_workspace``)."""
    device = torch.device(device)
    n = len(spans)
    if not 0 <= int(max_workgroups) <= FP_MAX_WORKGROUPS:
        raise ValueError("fingerprint_spans: max_workgroups must lie in [0, %d]" % FP_MAX_WORKGROUPS)
    if out is None:
        out = torch.empty(n, device=device, dtype=torch.int64)
    assert out.is_cuda and out.dtype == torch.int64 and out.is_contiguous() and out.numel() >= n
    if n == 0:
        return out
    if ws is None:
        ws = _FP_WS.get(device)
        if ws is None:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("fingerprint_spans: call it once eagerly on %s before capturing it (workspace)" % device)
            ws = _FP_WS[device] = fingerprint_workspace(device)
    assert ws.is_cuda and ws.dtype == torch.int64 and ws.is_contiguous()
    arr = (FpSpan * n)()
    for i, (p, b, salt) in enumerate(spans):
        arr[i].ptr, arr[i].bytes, arr[i].salt = (int(p) or None), int(b), int(salt) & 0xFFFFFFFF
    call("xggm_fingerprint_spans", _ct.addressof(arr), n, ptr(out), ptr(ws), ws.numel() * 8, int(max_workgroups), stream())
    return out


class AnswerLogDesc(_ct.Structure):
    """mirror of ``xggm_answer_log`` (include/xggm.h)"""
    _fields_ = [("labels", _ct.c_void_p), ("scores", _ct.c_void_p), ("cursor", _ct.c_void_p), ("score_sum", _ct.c_void_p),
                ("flags", _ct.c_void_p), ("capacity", _ct.c_int64)]


def answer_pick(logits, log, target=None, rows=None):
    """append the arg-max of every row of ``logits`` (fp32 [B, A], unit inner stride) to ``log`` -- anything with the
    device tensors ``labels`` int64 [capacity], ``scores`` fp32 [capacity] or None, ``cursor`` int64 [1], ``score_sum``
    fp64 [1] or None, ``flags`` int32 [1] (``engine.AnswerLog``) -- and, with ``target`` (fp32 [B, A]), the rows' soft
    scores and their running sum.  ``rows``: int32 [1] DEVICE tensor, the kept rows of a padded batch (None: all).
    Contract: xggm_answer_pick_f32 in xggm.h.  One launch, nothing returned: the log is read with ``log.read()``."""
    _chk(logits, F32, "logits")
    B, A, ld = _rows(logits)
    if B <= 0 or A <= 0:
        raise ValueError("answer_pick: empty logits %s" % (tuple(logits.shape),))
    t_ld = 0
    if target is not None:
        _chk(target, F32, "target")
        if tuple(target.shape) != (B, A) or target.stride(1) != 1:
            raise ValueError("answer_pick: target %s does not match the logits %s" % (tuple(target.shape), (B, A)))
        if log.scores is None:
            raise ValueError("answer_pick: a target needs a log with scores (AnswerLog(with_scores=True))")
        t_ld = target.stride(0)
    d = AnswerLogDesc()
    cap = int(log.capacity)
    _c(log.labels, torch.int64, "log.labels"), _c(log.cursor, torch.int64, "log.cursor"), _c(log.flags, torch.int32, "log.flags")
    if log.labels.numel() < cap or log.cursor.numel() < 1 or log.flags.numel() < 1:
        raise ValueError("answer_pick: log.labels holds %d entries, the capacity is %d" % (log.labels.numel(), cap))
    if log.scores is not None:
        _c(log.scores, F32, "log.scores")
        assert log.scores.numel() >= cap
    if log.score_sum is not None:
        _c(log.score_sum, torch.float64, "log.score_sum")
    if rows is not None:
        _c(rows, torch.int32, "rows")
        assert rows.numel() >= 1
    for t in (target, rows, log.labels, log.scores, log.cursor, log.score_sum, log.flags):
        if t is not None and t.device != logits.device:
            raise RuntimeError("answer_pick: the log, the target and the logits must live on one device")
    d.labels, d.scores, d.cursor = ptr(log.labels), ptr(log.scores), ptr(log.cursor)
    d.score_sum, d.flags, d.capacity = ptr(log.score_sum), ptr(log.flags), cap
    call("xggm_answer_pick_f32", ptr(logits), ld, ptr(target), t_ld, B, A, ptr(rows), _ct.addressof(d),
         ptr(sum_ws(logits.device)), stream())


FOLD_MAX_RANKS = 64                   # XGGM_FOLD_MAX_RANKS (include/xggm.h)
FOLD_CONCAT, FOLD_INTERLEAVE = 0, 1   # XGGM_FOLD_CONCAT, XGGM_FOLD_INTERLEAVE


def answer_log_fold(logs, dst, flag, src_capacity, with_scores, layout, expect, block=1, log_stride=None):
    """merge the data-parallel ranks' packed answer logs into ``dst`` in sweep order; ONE launch, contract:
    xggm_answer_log_fold in xggm.h.  ``logs``: int64 DEVICE tensor [world, log_stride] (or flat) holding every rank's
    ``AnswerLog.buf`` of ``src_capacity`` entries; ``dst``: anything with the device tensors of an ``engine.AnswerLog``;
    ``flag``: int64 [1] on the device -- 0 afterwards, or the bits of ``answers.FOLD_FLAG_*``; ``expect``: host ints, the
    answers every rank must hold; ``layout``: ``FOLD_CONCAT`` or ``FOLD_INTERLEAVE`` (with ``block``)."""
    from .answers import packed_words
    expect = [int(e) for e in expect]
    world = len(expect)
    if not 1 <= world <= FOLD_MAX_RANKS:
        raise ValueError("answer_log_fold: %d ranks (1 .. %d)" % (world, FOLD_MAX_RANKS))
    _c(logs, torch.int64, "logs"), _c(flag, torch.int64, "flag")
    src_capacity = int(src_capacity)
    words = packed_words(src_capacity, with_scores)
    if log_stride is None:
        log_stride = logs.shape[-1] if logs.dim() == 2 else words
    log_stride = int(log_stride)
    # the last word any rank's log is read at must lie inside the gathered buffer
    if src_capacity < 1 or log_stride < words or (world - 1) * log_stride + words > logs.numel():
        raise ValueError("answer_log_fold: logs holds %d words, %d ranks of capacity %d at stride %d need %d"
                         % (logs.numel(), world, src_capacity, log_stride, (world - 1) * max(log_stride, words) + words))
    cap = int(dst.capacity)
    _c(dst.labels, torch.int64, "dst.labels"), _c(dst.cursor, torch.int64, "dst.cursor"), _c(dst.flags, torch.int32, "dst.flags")
    if dst.labels.numel() < cap or dst.cursor.numel() < 1 or dst.flags.numel() < 1 or flag.numel() < 1:
        raise ValueError("answer_log_fold: the destination's buffers are smaller than its capacity %d says" % cap)
    if dst.scores is not None:
        _c(dst.scores, F32, "dst.scores")
        if dst.scores.numel() < cap:
            raise ValueError("answer_log_fold: dst.scores holds %d entries, the capacity is %d" % (dst.scores.numel(), cap))
    if dst.score_sum is not None:
        _c(dst.score_sum, torch.float64, "dst.score_sum")
    if with_scores and dst.scores is None:
        raise ValueError("answer_log_fold: with_scores needs a destination with scores")
    for t in (flag, dst.labels, dst.scores, dst.cursor, dst.score_sum, dst.flags):
        if t is not None and t.device != logs.device:
            raise RuntimeError("answer_log_fold: the gathered logs, the destination and the flag must live on one device")
    d = AnswerLogDesc(ptr(dst.labels), ptr(dst.scores), ptr(dst.cursor), ptr(dst.score_sum), ptr(dst.flags), cap)
    exp = (_ct.c_int64 * world)(*expect)
    call("xggm_answer_log_fold", ptr(logs), log_stride, src_capacity, 1 if with_scores else 0, world, int(layout), int(block),
         _ct.cast(exp, _ct.c_void_p), _ct.addressof(d), ptr(flag), stream())


SCORE_MAX_GROUPS = 16  # XGGM_SCORE_MAX_GROUPS (include/xggm.h)


def answer_score_workspace(n, G, device):
    """zeroed workspace of ``answer_score`` for sweeps of up to ``n`` positions and ``G`` groups (int64 words; the kernel
    leaves it ready for the next launch)"""
    nbytes = _lib.lib.xggm_answer_score_workspace_bytes(int(n), int(G))
    if nbytes == 0:
        raise ValueError("answer_score_workspace: n=%d, G=%d (n >= 1, 0 <= G <= %d)" % (n, G, SCORE_MAX_GROUPS))
    return torch.zeros(nbytes // 8, dtype=torch.int64, device=device)


def answer_score(labels, q_label, q_score, n=None, order=None, keep=None, q_group=None, G=0, n_q=None, cursor=None, out=None,
                 ws=None):
    """score the first ``n`` (default: all) ``labels`` (int64, an ``AnswerLog``'s) against the tables ``q_label`` int32
    [n_q, K] / ``q_score`` fp32 [n_q, K] of a device-resident split in ONE launch; contract: xggm_answer_score in xggm.h.
    ``order``: int64 [>= n], the sample of every position (None: position i is sample i); ``keep``: uint8 [>= n] (None: all
    count); ``q_group``: int32 [n_q] with ids in [0, G) for per-group counts and sums; ``n_q``: how many rows of the tables
    the launch is told of (default: all); ``cursor``: int64 [1] device word compared with n.  ``out``: int64 [>= 3 + 2 G]
    and ``ws`` (``answer_score_workspace``) are made when not given.  -> ``out[:3 + 2 G]`` on the device:
    [flags, count_all, count_g.., sum_all, sum_g..]; ``answers.decode_score`` reads its host copy."""
    _c(labels, torch.int64, "labels"), _c(q_label, torch.int32, "q_label"), _c(q_score, F32, "q_score")
    dev = labels.device
    n = labels.numel() if n is None else int(n)
    G = int(G)
    if labels.dim() != 1 or not 1 <= n <= labels.numel():
        raise ValueError("answer_score: n=%d of %s labels" % (n, tuple(labels.shape)))
    if q_label.dim() != 2 or tuple(q_score.shape) != tuple(q_label.shape) or q_label.shape[0] < 1 or q_label.shape[1] < 1:
        raise ValueError("answer_score: q_label %s and q_score %s, two [n_q, K] tables expected" % (tuple(q_label.shape), tuple(q_score.shape)))
    rows, K = q_label.shape
    n_q = rows if n_q is None else int(n_q)
    if not 1 <= n_q <= rows:
        raise ValueError("answer_score: n_q=%d, the tables hold %d samples" % (n_q, rows))
    if not 0 <= G <= SCORE_MAX_GROUPS or (q_group is None) != (G == 0):
        raise ValueError("answer_score: G=%d %s q_group (0 <= G <= %d; groups and their number come together)"
                         % (G, "without" if q_group is None else "with", SCORE_MAX_GROUPS))
    if order is not None and (_c(order, torch.int64, "order").dim() != 1 or order.numel() < n):
        raise ValueError("answer_score: order %s for n=%d" % (tuple(order.shape), n))
    if keep is not None and (_c(keep, torch.uint8, "keep").dim() != 1 or keep.numel() < n):
        raise ValueError("answer_score: keep %s for n=%d" % (tuple(keep.shape), n))
    if q_group is not None and tuple(_c(q_group, torch.int32, "q_group").shape) != (rows,):
        raise ValueError("answer_score: q_group %s, [%d] expected" % (tuple(q_group.shape), rows))
    if cursor is not None and _c(cursor, torch.int64, "cursor").numel() < 1:
        raise ValueError("answer_score: cursor must hold ONE int64 word")
    W = 3 + 2 * G
    if out is None:
        out = torch.empty(W, dtype=torch.int64, device=dev)
    if ws is None:
        ws = answer_score_workspace(n, G, dev)
    _c(out, torch.int64, "out"), _c(ws, torch.int64, "ws")
    if out.numel() < W:
        raise ValueError("answer_score: out holds %d words, %d are written" % (out.numel(), W))
    for t in (q_label, q_score, order, keep, q_group, cursor, out, ws):
        if t is not None and t.device != dev:
            raise RuntimeError("answer_score: all operands must live on one device")
    call("xggm_answer_score", ptr(labels), ptr(order), ptr(keep), ptr(q_label), ptr(q_score), ptr(q_group), n, n_q, K, G,
         ptr(cursor), ptr(out), ptr(ws), ws.numel() * 8, stream())
    return out[:W]


TRAINLOG_COLS = 8   # XGGM_TRAINLOG_COLS (include/xggm.h)
TRAINLOG_KINDS = 4  # XGGM_TRAINLOG_KINDS


class TrainLogDesc(_ct.Structure):
    """mirror of ``xggm_train_log`` (include/xggm.h)"""
    _fields_ = [("values", _ct.c_void_p), ("steps", _ct.c_void_p), ("kinds", _ct.c_void_p), ("cursor", _ct.c_void_p),
                ("sums", _ct.c_void_p), ("counts", _ct.c_void_p), ("first_bad", _ct.c_void_p), ("capacity", _ct.c_int64)]


def train_log_append(log, kind, cols, mul=None, step=None):
    """append ONE record to ``log`` -- anything with the device tensors ``values`` fp32 [capacity, 8], ``steps`` int64
    [capacity] or None, ``kinds`` int32 [capacity], ``cursor`` int64 [1], ``sums`` fp64 [4, 8], ``counts`` int64 [4],
    ``first_bad_word`` int64 [1] (``engine.TrainLog``).  ``cols``: up to 8 entries, each a 0-dim or 1-element fp32 DEVICE
    tensor or None (column absent); ``mul``: one host float per column (None: all ones), the record holds ``col * mul``;
    ``step``: 1-element int64 device tensor (an optimiser step counter) or None.  Contract: xggm_train_log_append in
    xggm.h.  One launch, nothing returned and nothing kept alive: the log is read with ``log.read()``."""
    cols = list(cols)
    n = len(cols)
    if not 0 < n <= TRAINLOG_COLS:
        raise ValueError("train_log_append: %d columns (a record holds 1 .. %d)" % (n, TRAINLOG_COLS))
    if mul is not None and len(mul) != n:
        raise ValueError("train_log_append: %d factors for %d columns" % (len(mul), n))
    for i, t in enumerate(cols):
        if t is None:
            continue
        if t.dtype != F32 or t.numel() != 1:
            raise ValueError("train_log_append: column %d is %s %s, expected ONE fp32 value (0-dim or 1-element)"
                             % (i, t.dtype, tuple(t.shape)))
        _chk(t, F32, "column %d" % i)
    _c(log.values, F32, "log.values"), _c(log.kinds, torch.int32, "log.kinds"), _c(log.cursor, torch.int64, "log.cursor")
    _c(log.sums, torch.float64, "log.sums"), _c(log.counts, torch.int64, "log.counts")
    _c(log.first_bad_word, torch.int64, "log.first_bad_word")
    cap = int(log.capacity)
    if log.values.numel() < cap * TRAINLOG_COLS or log.kinds.numel() < cap or log.sums.numel() < TRAINLOG_KINDS * TRAINLOG_COLS \
            or log.counts.numel() < TRAINLOG_KINDS or log.cursor.numel() < 1 or log.first_bad_word.numel() < 1:
        raise ValueError("train_log_append: the log's buffers are smaller than its capacity %d says" % cap)
    if log.steps is not None:
        _c(log.steps, torch.int64, "log.steps")
        if log.steps.numel() < cap:
            raise ValueError("train_log_append: log.steps holds %d entries, the capacity is %d" % (log.steps.numel(), cap))
    if step is not None:
        _c(step, torch.int64, "step")
        if step.numel() != 1:
            raise ValueError("train_log_append: step must be ONE int64 counter")
    dev = log.cursor.device
    for t in cols + [step, log.values, log.steps, log.kinds, log.sums, log.counts, log.first_bad_word]:
        if t is not None and t.device != dev:
            raise RuntimeError("train_log_append: the log, the columns and the step must live on one device")
    d = TrainLogDesc(ptr(log.values), ptr(log.steps), ptr(log.kinds), ptr(log.cursor), ptr(log.sums), ptr(log.counts),
                     ptr(log.first_bad_word), cap)
    src = (_ct.c_void_p * n)(*[ptr(t) for t in cols])
    fac = None if mul is None else (_ct.c_float * n)(*[float(m) for m in mul])
    call("xggm_train_log_append", _ct.cast(src, _ct.c_void_p), None if fac is None else _ct.cast(fac, _ct.c_void_p), n,
         int(kind), ptr(step), _ct.addressof(d), stream())


def train_log_fold(log, vals, kinds, world, n, flag, steps=None, cursors=None, strides=None):
    """the mean of the data-parallel ranks' copies of the ``n`` records of ``log`` (all of them since its reset: record i in
    row i), folded into ``log``; ONE launch, contract: xggm_train_log_fold in xggm.h.  ``vals`` fp32, ``kinds`` int32 (the
    packed kind words), ``steps`` / ``cursors`` int64 or None: DEVICE buffers that hold every rank's copy, rank r's at
    ``r * strides[j]`` elements -- ``strides`` = (values, kinds, steps, cursors), default: dense [world, n, 8], [world, n],
    [world, n], [world].  ``flag``: int64 [1] on the device; the launch leaves -1 there, or the first record the ranks
    disagree on (n: a cursor is not n) -- the caller reads it with the log."""
    world, n = int(world), int(n)
    if world < 1:
        raise ValueError("train_log_fold: world = %d" % world)
    cap = int(log.capacity)
    if not 1 <= n <= cap:
        raise ValueError("train_log_fold: %d records, the log holds 1 .. %d" % (n, cap))
    if strides is None:
        strides = (n * TRAINLOG_COLS, n, n, 1)
    sv, sk, ss, sc = (int(s) for s in strides)
    _chk(vals, F32, "vals"), _chk(kinds, torch.int32, "kinds"), _chk(flag, torch.int64, "flag")
    _c(log.values, F32, "log.values"), _c(log.kinds, torch.int32, "log.kinds"), _c(log.cursor, torch.int64, "log.cursor")
    _c(log.sums, torch.float64, "log.sums"), _c(log.counts, torch.int64, "log.counts")
    _c(log.first_bad_word, torch.int64, "log.first_bad_word")
    if log.values.numel() < cap * TRAINLOG_COLS or log.kinds.numel() < cap or log.sums.numel() < TRAINLOG_KINDS * TRAINLOG_COLS \
            or log.counts.numel() < TRAINLOG_KINDS or log.cursor.numel() < 1 or log.first_bad_word.numel() < 1:
        raise ValueError("train_log_fold: the log's buffers are smaller than its capacity %d says" % cap)
    if flag.numel() < 1:
        raise ValueError("train_log_fold: flag holds no word")
    # the last element any rank's copy is read at must lie inside its buffer
    need = [("vals", vals, sv, n * TRAINLOG_COLS), ("kinds", kinds, sk, n)]
    for name, t, s, dt in (("steps", steps, ss, n), ("cursors", cursors, sc, 1)):
        if t is not None:
            _chk(t, torch.int64, name)
            need.append((name, t, s, dt))
    for name, t, s, per in need:
        if (world > 1 and s < per) or (world - 1) * s + per > t.numel():
            raise ValueError("train_log_fold: %s holds %d elements, %d ranks at stride %d need %d"
                             % (name, t.numel(), world, s, (world - 1) * s + per))
    dev = log.cursor.device
    for t in (vals, kinds, steps, cursors, flag, log.values, log.kinds, log.sums, log.counts, log.first_bad_word):
        if t is not None and t.device != dev:
            raise RuntimeError("train_log_fold: the log and the gathered buffers must live on one device")
    d = TrainLogDesc(ptr(log.values), ptr(log.steps), ptr(log.kinds), ptr(log.cursor), ptr(log.sums), ptr(log.counts),
                     ptr(log.first_bad_word), cap)
    call("xggm_train_log_fold", ptr(vals), ptr(kinds), ptr(steps), ptr(cursors), sv, sk, ss, sc, world, n, _ct.addressof(d),
         ptr(flag), stream())


class _PassTail(_ct.Structure):
    _fields_ = [("steps", _ct.c_void_p), ("lr_scale", _ct.c_void_p), ("index", _ct.c_void_p), ("t_total", _ct.c_void_p),
                ("warmup", _ct.c_void_p), ("n", _ct.c_int), ("rng", _ct.c_void_p), ("rng_by", _ct.c_uint64)]


CLIP_NORM_MAX_SPANS = 24
CLIP_NORM_MAX_SCHED = 16


def _pass_tail(sched, rng):
    """(xggm_pass_tail or None, objects to keep alive) for clip_norm / clip_norm_bf16"""
    if sched is None and rng is None:
        return None, ()
    tail, keep = _PassTail(), []
    if sched is not None:
        steps, lr_scale, entries = sched
        _c(steps, torch.int64), _c(lr_scale, F32)
        n = len(entries)
        assert n <= CLIP_NORM_MAX_SCHED
        idx = (_ct.c_int * max(n, 1))(*[int(e[0]) for e in entries])
        tt = (_ct.c_int64 * max(n, 1))(*[int(e[1]) for e in entries])
        wu = (_ct.c_float * max(n, 1))(*[float(e[2]) for e in entries])
        keep += [idx, tt, wu]
        tail.steps, tail.lr_scale, tail.n = ptr(steps), ptr(lr_scale), n
        tail.index, tail.t_total, tail.warmup = (_ct.cast(a, _ct.c_void_p) for a in (idx, tt, wu))
    if rng is not None:
        tail.rng, tail.rng_by = ptr(rng[0]), int(rng[1])
    return tail, keep


def clip_norm_bf16(g, spans, out, norm=None, accumulate=False, mul=1.0, sched=None, rng=None):
    """out (1 fp32) = ((out if accumulate else 0) + sum over the (start, end) ranges of the bf16 buffer g of g^2) * mul,
    ``norm`` = sqrt(out): the norm pass over the data-parallel wire arena in two launches (at most 24 ranges, starts
    multiples of 8); ``sched`` / ``rng`` as in ``clip_norm``."""
    _c(g, BF16), _c(out, F32)
    rs = [(s, e) for s, e in spans if e > s]
    assert len(rs) <= CLIP_NORM_MAX_SPANS
    offs, lens = _span_arrays(rs)
    tail, keep = _pass_tail(sched, rng)
    call("xggm_clip_norm_bf16", ptr(g), offs, lens, len(rs), ptr(out), ptr(norm) if norm is not None else None,
         _norm_ws(g.device), int(accumulate), float(mul), _ct.byref(tail) if tail is not None else None, stream())


def clip_norm(g, spans, slots, slot_spans, out, norm=None, mul=1.0, sched=None, rng=None):
    """out (1 fp32) = mul * (sum over the (start, end) ranges ``spans`` of g^2 + sum over ``slot_spans`` of slots), fixed
    summation order, ``norm`` (1 fp32 or None) = sqrt(out): the whole norm of a pass in two launches.  The finishing
    launch also takes ``sched`` = (steps, lr_scale, [(index, t_total, warmup)]) (sched_step_multi) and ``rng`` =
    (state, by) (rng_advance) along.  At most 24 ranges and 16 schedule entries."""
    _c(g, F32), _c(out, F32)
    rs = [(s, e) for s, e in spans if e > s]
    ss = [(s, e) for s, e in slot_spans if e > s]
    assert len(rs) + len(ss) <= CLIP_NORM_MAX_SPANS
    if ss:
        _c(slots, F32)
    o1, l1 = _span_arrays(rs)
    o2, l2 = _span_arrays(ss)
    tail, keep = _pass_tail(sched, rng)
    call("xggm_clip_norm_f32", ptr(g), o1, l1, len(rs), ptr(slots) if ss else None, o2, l2, len(ss), ptr(out),
         ptr(norm) if norm is not None else None, _norm_ws(g.device), float(mul),
         _ct.byref(tail) if tail is not None else None, stream())


def additive_mask(mask):
    """(1 - mask) * -10000 as fp32, for an int64 token mask [B, S]"""
    _c(mask, torch.int64, "attention mask")
    out = torch.empty(mask.shape, device=mask.device, dtype=F32)
    call("xggm_additive_mask", ptr(mask), ptr(out), mask.numel(), stream())
    return out


def zero_diag(adj):
    """adj.triu(1) + adj.tril(-1) for fp32 [B, N, N]"""
    _c(adj, F32, "adjacency")
    B, N, N2 = adj.shape
    assert N == N2
    out = torch.empty_like(adj)
    call("xggm_zero_diag_f32", ptr(adj), ptr(out), B, N, stream())
    return out


def add_n(terms, out=None):
    """sum of 2..4 same-shaped contiguous tensors (fp32 or bf16) in ONE launch, fp32 arithmetic; ``out`` may be one of
    them"""
    assert 2 <= len(terms) <= 4
    t0 = terms[0]
    for t in terms:
        assert t.is_cuda and t.dtype == t0.dtype and t.shape == t0.shape and t.is_contiguous()
    if out is None:
        out = torch.empty_like(t0)
    ps = [ptr(t) for t in terms] + [None] * (4 - len(terms))
    call("xggm_add_n_f32" if t0.dtype == F32 else "xggm_add_n_bf16", ps[0], ps[1], ps[2], ps[3], ptr(out), t0.numel(),
         stream())
    return out


def pad_rows(x, ld):
    """[rows, n] fp32 / bf16 -> bf16 [rows, ld] with zero columns n.. (one launch); returns the [rows, n] VIEW with row
    stride ld"""
    assert x.dim() == 2 and x.is_cuda and x.is_contiguous() and x.dtype in (F32, BF16) and ld >= x.shape[1]
    out = torch.empty((x.shape[0], ld), device=x.device, dtype=BF16)
    call("xggm_pad_rows_bf16", ptr(x), int(x.dtype == F32), ptr(out), x.shape[0], x.shape[1], ld, stream())
    return out[:, :x.shape[1]]


def gather_rows(table_f32, idx, out=None):
    """out[i] = bf16(table[idx[i]]): ``table`` fp32 [V, H] (contiguous), ``idx`` int64 [n] on the device"""
    V, H = table_f32.shape
    n = idx.numel()
    if out is None:
        out = torch.empty((n, H), device=table_f32.device, dtype=BF16)
    call("xggm_gather_rows_bf16", ptr(table_f32), ptr(idx), ptr(out), n, H, V, stream())
    return out


def scatter_rows(rows_bf16, idx, table_bf16):
    """table[idx[i]] = rows[i] (duplicate indices carry identical rows)"""
    V, H = table_bf16.shape
    call("xggm_scatter_rows_bf16", ptr(rows_bf16), ptr(idx), ptr(table_bf16), idx.numel(), H, V, stream())


def add_scalars(terms):
    """sum of up to four 0-dim fp32 device tensors"""
    ts = [_c(t, F32) for t in terms]
    assert 1 <= len(ts) <= 4
    out = torch.empty((), device=ts[0].device, dtype=F32)
    ps = [ptr(t) for t in ts] + [None] * (4 - len(ts))
    call("xggm_add_scalars_f32", ps[0], ps[1], ps[2], ps[3], ptr(out), stream())
    return out


class AdamArgs(_ct.Structure):
    """mirror of ``xggm_adam_args`` (include/xggm.h)"""
    _fields_ = [("p", _ct.c_void_p), ("g", _ct.c_void_p), ("m", _ct.c_void_p), ("v", _ct.c_void_p),
                ("shadow_bf16", _ct.c_void_p), ("n", _ct.c_int64), ("sqnorm", _ct.c_void_p), ("max_norm", _ct.c_float),
                ("lr", _ct.c_float), ("lr_dev", _ct.c_void_p), ("lr_scale", _ct.c_void_p),
                ("b1", _ct.c_float), ("b2", _ct.c_float), ("eps", _ct.c_float), ("weight_decay", _ct.c_float),
                ("g_bf16", _ct.c_int), ("shadow8", _ct.c_void_p), ("w8_id", _ct.c_void_p), ("w8_qscale", _ct.c_void_p),
                ("w8_amax", _ct.c_void_p), ("elem0", _ct.c_int64), ("g_scale", _ct.c_float), ("w8_amax_slots", _ct.c_int)]


class HyperMap(_ct.Structure):
    """mirror of ``xggm_hyper_map`` (include/xggm.h)"""
    _fields_ = [("ids", _ct.c_void_p), ("n_ids", _ct.c_int64), ("table", _ct.c_void_p), ("n_table", _ct.c_int)]


HYPER_MAP_ELEMS = 8     # elements of the arena one id of the map stands for (arena.ALIGN)
HYPER_MAP_MAX_ID = 255  # the ids are uint8; 0 = not in the optimiser


def _hyper_map(hyper_map):
    """``hyper_map`` = (ids: uint8 [ceil(arena / 8)], table: fp32 [1 + param_groups, 2] of {lr, weight_decay}), both on the device"""
    ids, table = hyper_map
    _c(ids, torch.uint8), _c(table, F32)
    if table.dim() != 2 or table.shape[1] != 2 or not 1 <= table.shape[0] <= HYPER_MAP_MAX_ID + 1:
        raise ValueError("xggm_amd: the hyper table is [1 + param_groups <= %d, 2], got %s" % (HYPER_MAP_MAX_ID + 1, tuple(table.shape)))
    return HyperMap(ptr(ids), ids.numel(), ptr(table), table.shape[0])


RULES = {"bertadam": 0, "adam": 1, "adamw": 2, "adamax": 3, "sgd": 4, "rmsprop": 5}  # XGGM_RULE_* (include/xggm.h)
SCHED_KINDS = {"warmup_linear": 0, "warmup_cosine": 1, "warmup_constant": 2}            # XGGM_SCHED_*


class OptimArgs(_ct.Structure):
    """mirror of ``xggm_optim_args`` (include/xggm.h)"""
    _fields_ = [("a", AdamArgs), ("rule", _ct.c_int), ("step_scalars", _ct.c_void_p), ("b1", _ct.c_double),
                ("b2", _ct.c_double), ("momentum", _ct.c_double), ("dampening", _ct.c_double), ("alpha", _ct.c_double),
                ("nesterov", _ct.c_int)]


class SchedEntry(_ct.Structure):
    """mirror of ``xggm_sched_entry`` (include/xggm.h)"""
    _fields_ = [("index", _ct.c_int), ("kind", _ct.c_int), ("t_total", _ct.c_int64), ("warmup", _ct.c_double),
                ("b1", _ct.c_double), ("b2", _ct.c_double)]


def optim_multi(rule, jobs, hyper_map=None):
    """the fused update (xggm_optim_multi): ``rule`` a key of ``RULES`` -- "bertadam" (src/lxrt/optimization.py:159-193) or
    a torch.optim rule (src/param.py:9-31); ``jobs``: per span (argument tuple of ``_adam_args``, dict of its keyword
    arguments, dict of the rule's: step_scalars (3 device floats of the span's group, ``sched_step_ex``), b1, b2, momentum,
    dampening, alpha, nesterov -- ``{}`` for bertadam).  ONE launch per 8 spans, in chunks by gradient type.  With
    ``hyper_map`` (see ``_hyper_map``) lr and weight decay are read per tensor from the map; the jobs' own are then not used."""
    if not jobs:
        return
    hm = None if hyper_map is None else _ct.byref(_hyper_map(hyper_map))
    structs = []
    for a, kw, r in jobs:
        hs = r.get("step_scalars")
        if hs is not None:
            _c(hs, F32)
            assert hs.numel() >= 3
        structs.append(OptimArgs(_adam_args(*a, **kw), RULES[rule], ptr(hs), float(r.get("b1", 0.0)), float(r.get("b2", 0.0)),
                                 float(r.get("momentum", 0.0)), float(r.get("dampening", 0.0)), float(r.get("alpha", 0.0)),
                                 int(bool(r.get("nesterov", False)))))
    for bf in (0, 1):
        chunk = [x for x in structs if x.a.g_bf16 == bf]
        if chunk:
            arr = (OptimArgs * len(chunk))(*chunk)
            call("xggm_optim_multi", _ct.cast(arr, _ct.c_void_p), len(chunk), hm, stream())


LAMB_CHUNK = 2048  # XGGM_LAMB_CHUNK (include/xggm.h)


def lamb_workspace(arena_elems, n_tensors, device):
    """the scratch of ``lamb_multi`` for spans that end at or below ``arena_elems`` and a table of ``n_tensors`` entries"""
    nbytes = _lib.lib.xggm_lamb_workspace_bytes(int(arena_elems), int(n_tensors))
    return torch.empty((nbytes + 15) // 16 * 2, device=device, dtype=torch.float64)


def lamb_multi(jobs, tensors, ratios, ws, hyper_map=None):
    """BertLamb's update (xggm_lamb_multi): ``jobs`` as ``optim_multi`` takes them for "bertadam" (no e4m3 copy; ``elem0``
    is required: it places a span against the table), in arena order.  ``tensors``: int64 [n, 3] device table {elem0, n,
    adapted}, sorted (``arena.lamb_tensor_table``); ``ratios``: fp32 [n], receives the trust ratio of every tensor that took
    part; ``ws``: ``lamb_workspace``.  Phase A, a finish and phase B per 8 spans; nothing is allocated or read back."""
    if not jobs:
        return
    _c(tensors, torch.int64), _c(ratios, F32), _c(ws, torch.float64)
    if tensors.dim() != 2 or tensors.shape[1] != 3 or ratios.numel() != tensors.shape[0]:
        raise ValueError("xggm_amd: the tensor table is int64 [n, 3] with one ratio per row, got %s and %d ratios"
                         % (tuple(tensors.shape), ratios.numel()))
    hm = None if hyper_map is None else _ct.byref(_hyper_map(hyper_map))
    structs = [_adam_args(*a, **kw) for a, kw, _ in jobs]
    arr = (AdamArgs * len(structs))(*structs)
    call("xggm_lamb_multi", _ct.cast(arr, _ct.c_void_p), len(structs), ptr(tensors), tensors.shape[0], hm, ptr(ratios), ptr(ws),
         ws.numel() * 8, stream())


def sched_step_ex(steps, lr_scale, step_scalars, entries):
    """``entries``: [(index, t_total, warmup, kind, b1, b2)] with ``kind`` a key of ``SCHED_KINDS``: schedule value and
    counter as ``sched_step_multi``, evaluated in double, plus -- with ``step_scalars`` (fp32 [groups * 4]) -- the bias
    corrections {1 / (1 - b1^t), 1 / sqrt(1 - b2^t), first step} of the step, in double on the device"""
    _c(steps, torch.int64), _c(lr_scale, F32)
    if step_scalars is not None:
        _c(step_scalars, F32)
        assert step_scalars.numel() >= 4 * steps.numel()
    for i in range(0, len(entries), 16):
        ch = entries[i:i + 16]
        arr = (SchedEntry * len(ch))(*[SchedEntry(int(e[0]), SCHED_KINDS[e[3]], int(e[1]), float(e[2]), float(e[4]), float(e[5]))
                                       for e in ch])
        call("xggm_sched_step_ex", ptr(steps), ptr(lr_scale), ptr(step_scalars), _ct.cast(arr, _ct.c_void_p), len(ch), stream())


def _adam_args(p, g, m, v, shadow, sqn, max_norm, lr, lr_scale, b1, b2, eps, wd, lr_dev=None, w8=None, elem0=0, g_scale=1.0):
    """one span of ``optim_multi`` as ``xggm_adam_args``: device-resident lr (``lr_dev``), bf16 gradients (``g.dtype``) and/or
    the e4m3 weight copy ``w8`` = (shadow8 slice, id table, qscale table, amax table[, slots]); ``elem0``: arena offset of p[0]."""
    for t in (p, m, v):
        _c(t, F32)
        assert t.numel() == p.numel()
    _c(g)
    assert g.numel() == p.numel() and g.dtype in (F32, BF16)
    a = AdamArgs(ptr(p), ptr(g), ptr(m), ptr(v), ptr(shadow), p.numel(), ptr(sqn), float(max_norm), float(lr), ptr(lr_dev),
                 ptr(lr_scale), float(b1), float(b2), float(eps), float(wd), int(g.dtype == BF16), None, None, None, None,
                 int(elem0), float(g_scale), 1)
    if w8 is not None:
        s8, ids, q, amax = w8[:4]
        assert s8.numel() == p.numel() and s8.element_size() == 1 and ids.dtype == torch.int16
        a.shadow8, a.w8_id, a.w8_qscale, a.w8_amax = ptr(s8), ptr(ids), ptr(q), ptr(amax)
        a.w8_amax_slots = int(w8[4]) if len(w8) > 4 else 1  # floats per entry of the amax table
    return a


def sqnorm_bf16(g, out):
    """out += sum g^2 of a bf16 tensor, as ``sqnorm``"""
    _c(g, BF16), _c(out, F32)
    call("xggm_sqnorm_bf16", ptr(g), g.numel(), ptr(out), _norm_ws(g.device), stream())


def fp8_scale_update(amax, hist, qscale, dscale, pos, i0, n, hist_len, margin, shrink, bump, slots=1):
    """entries [i0, i0 + n) of a scale table (xggm_fp8_scale_update); ``slots``: floats every amax entry is spread over"""
    for t in (amax, hist, qscale, dscale):
        _c(t, F32)
    _c(pos, torch.int64)
    call("xggm_fp8_scale_update", amax.data_ptr() + 4 * i0 * slots, hist.data_ptr() + 4 * i0 * hist_len,
         qscale.data_ptr() + 4 * i0, dscale.data_ptr() + 4 * i0, ptr(pos), n, hist_len, float(margin), int(shrink),
         int(bump), int(slots), stream())


def sched_step(step, lr_scale, t_total, warmup):
    _c(step, torch.int64), _c(lr_scale, F32)
    call("xggm_sched_step", ptr(step), ptr(lr_scale), int(t_total), float(warmup), stream())


def sched_step_multi(steps, lr_scale, entries):
    """``entries``: [(index, t_total, warmup)] -- one launch for all of them (groups of 16)."""
    _c(steps, torch.int64), _c(lr_scale, F32)
    for i in range(0, len(entries), 16):
        ch = entries[i:i + 16]
        n = len(ch)
        idx = (_ct.c_int * n)(*[int(e[0]) for e in ch])
        tt = (_ct.c_int64 * n)(*[int(e[1]) for e in ch])
        wu = (_ct.c_float * n)(*[float(e[2]) for e in ch])
        call("xggm_sched_step_multi", ptr(steps), ptr(lr_scale), _ct.cast(idx, _ct.c_void_p), _ct.cast(tt, _ct.c_void_p),
             _ct.cast(wu, _ct.c_void_p), n, stream())


def rng_advance(rng, by=1):
    call("xggm_rng_advance", ptr(rng), int(by), stream())


def scale(x, s=1.0, scale_ptr=None):
    """s * (1 + *scale_ptr) * x"""
    _c(x)
    out = torch.empty_like(x)
    call("xggm_scale_" + sfx(x.dtype), ptr(x), ptr(out), x.numel(), float(s), ptr(scale_ptr), stream())
    return out


def sigmoid_bwd(dy, y, dt):
    _c(dy, F32), _c(y, F32)
    out = torch.empty(y.shape, device=y.device, dtype=dt)
    call("xggm_sigmoid_bwd_" + sfx(dt), ptr(dy), ptr(y), ptr(out), y.numel(), stream())
    return out


def tanh_bwd(dy, y):
    _c(dy), _c(y, dy.dtype)
    out = torch.empty_like(y)
    call("xggm_tanh_bwd_" + sfx(y.dtype), ptr(dy), ptr(y), ptr(out), y.numel(), stream())
    return out


def cast_from_f32(x, dt):
    """fp32 -> T copy (identity copy for T = fp32 is skipped)."""
    _c(x, F32)
    if dt == F32:
        return x
    out = torch.empty(x.shape, device=x.device, dtype=dt)
    call("xggm_cast_from_f32_" + sfx(dt), ptr(x), ptr(out), x.numel(), stream())
    return out


def cast_bf16(x, out):
    _c(x, F32), _c(out, BF16)
    assert x.numel() == out.numel()
    if x.numel():
        call("xggm_cast_f32_to_bf16", ptr(x), ptr(out), x.numel(), stream())


def dropout_mask(n, p, rng, sid, device):
    out = torch.empty(n, device=device, dtype=F32)
    call("xggm_dropout_mask", ptr(out), n, float(p), ptr(rng), sid, stream())
    return out


def normal(n, rng, sid, device):
    out = torch.empty(n, device=device, dtype=F32)
    call("xggm_normal", ptr(out), n, ptr(rng), sid, stream())
    return out


def uniform(n, rng, sid, device=None):
    """the uniform [0, 1) draws 0..n-1 of Philox stream ``sid`` at the state ``rng``: what a draw buffer that
    ``pretrain_corrupt`` is not given stands for (``dropout_mask`` does the same for dropout)"""
    _c(rng, torch.int64, "rng")
    out = torch.empty(int(n), device=rng.device if device is None else device, dtype=F32)
    call("xggm_uniform", ptr(out), int(n), ptr(rng), int(sid), stream())
    return out


def make_rng(seed, device):
    """device-resident {seed, offset} pair (int64 storage of the two uint64 words)."""
    return torch.tensor([int(seed) & 0x7FFFFFFFFFFFFFFF, 0], dtype=torch.int64, device=device)


def triu_index(k, N):
    import ctypes
    i, j = ctypes.c_int(), ctypes.c_int()
    _lib.check(_lib.lib.xggm_triu_index(k, N, ctypes.byref(i), ctypes.byref(j)), "xggm_triu_index")
    return i.value, j.value


# ----------------------------------------------------------------------------- pre-training batch masking
PRETRAIN_DRAWS = ("u_word", "u_word_pick", "u_obj", "u_obj_pick", "u_ans")  # Philox streams sid_base + 0..4, in this order


class PretrainCorruptArgs(_ct.Structure):
    """mirror of ``xggm_pretrain_corrupt_args`` (include/xggm.h)"""
    _fields_ = [("feats", _ct.c_void_p), ("pool", _ct.c_void_p), ("masked_feat", _ct.c_void_p), ("feat_mask", _ct.c_void_p),
                ("input_ids", _ct.c_void_p), ("input_mask", _ct.c_void_p), ("input_ids_out", _ct.c_void_p),
                ("masked_lm_labels", _ct.c_void_p), ("label_ids", _ct.c_void_p), ("label_scores", _ct.c_void_p),
                ("is_matched", _ct.c_void_p), ("ans", _ct.c_void_p), ("B", _ct.c_int), ("T", _ct.c_int), ("O", _ct.c_int),
                ("F", _ct.c_int), ("K", _ct.c_int), ("P", _ct.c_int64), ("vocab_size", _ct.c_int64), ("mask_id", _ct.c_int64),
                ("word_mask_rate", _ct.c_double), ("obj_mask_rate", _ct.c_double), ("u_word", _ct.c_void_p),
                ("u_word_pick", _ct.c_void_p), ("u_obj", _ct.c_void_p), ("u_obj_pick", _ct.c_void_p), ("u_ans", _ct.c_void_p),
                ("rng", _ct.c_void_p), ("sid_base", _ct.c_uint32)]


def pretrain_corrupt(input_ids, input_mask, feats, is_matched, label_ids, label_scores, word_mask_rate, obj_mask_rate,
                     vocab_size, mask_id, rng=None, sid_base=0, pool=None, draws=None, out=None):
    """random_word / random_feat / the QA answer draw of src/pretrain/lxmert_pretrain.py:76-215 for a batch on the device, one
    launch; contract: xggm_pretrain_corrupt_* in xggm.h.  ``feats`` [B, O, F] fp32 or bf16, ``input_ids`` / ``input_mask``
    [B, T] int64, ``label_ids`` [B, K] int64 (-1 padded), ``label_scores`` [B, K] fp32, ``is_matched`` [B] int64.  ``draws``:
    a dict with any of ``PRETRAIN_DRAWS`` (fp32, row-major); a missing one is drawn from ``rng`` at stream ``sid_base + k``.
    ``out``: a dict of the five outputs to write into (else they are allocated).
    -> dict(input_ids, masked_lm_labels, masked_feat, feat_mask, ans)"""
    _c(feats, None, "feats")
    sfx(feats.dtype)
    if feats.dim() != 3 or input_ids.dim() != 2 or label_ids.dim() != 2:
        raise ValueError("pretrain_corrupt: feats [B, O, F], input_ids [B, T] and label_ids [B, K] expected")
    B, O, F = feats.shape
    T, K = input_ids.shape[1], label_ids.shape[1]
    dev = feats.device
    _c(input_ids, torch.int64, "input_ids"), _c(input_mask, torch.int64, "input_mask"), _c(is_matched, torch.int64, "is_matched")
    _c(label_ids, torch.int64, "label_ids"), _c(label_scores, F32, "label_scores")
    if (tuple(input_ids.shape) != (B, T) or tuple(input_mask.shape) != (B, T) or tuple(label_ids.shape) != (B, K)
            or tuple(label_scores.shape) != (B, K) or is_matched.numel() != B):
        raise ValueError("pretrain_corrupt: operands do not share B=%d (T=%d, K=%d)" % (B, T, K))
    if min(B, T, O, F, K) <= 0:
        raise ValueError("pretrain_corrupt: empty batch B=%d T=%d O=%d F=%d K=%d" % (B, T, O, F, K))
    a = PretrainCorruptArgs()
    if pool is not None:
        _c(pool, feats.dtype, "pool")
        if pool.dim() != 2 or pool.shape[1] != F or pool.shape[0] <= 0:
            raise ValueError("pretrain_corrupt: pool %s is no [P, %d] table" % (tuple(pool.shape), F))
        a.pool, a.P = ptr(pool), pool.shape[0]
    draws = dict(draws or {})
    sizes = dict(u_word=B * T, u_word_pick=B * T, u_obj=B * O, u_obj_pick=B * O, u_ans=B)
    if set(draws) - set(sizes):
        raise ValueError("pretrain_corrupt: unknown draws %s" % sorted(set(draws) - set(sizes)))
    for k, n in sizes.items():
        d = draws.get(k)
        if d is not None:
            _c(d, F32, k)
            if d.numel() != n:
                raise ValueError("pretrain_corrupt: %s has %d draws, %d expected" % (k, d.numel(), n))
        setattr(a, k, ptr(d))
    if rng is None:
        if any(draws.get(k) is None for k in sizes):
            raise ValueError("pretrain_corrupt: a missing draw buffer needs rng")
    else:
        _c(rng, torch.int64, "rng")
    if out is None:
        out = dict(input_ids=torch.empty_like(input_ids), masked_lm_labels=torch.empty_like(input_ids),
                   masked_feat=torch.empty_like(feats), feat_mask=torch.empty((B, O), device=dev, dtype=F32),
                   ans=torch.empty(B, device=dev, dtype=torch.int64))
    _c(out["input_ids"], torch.int64, "out input_ids"), _c(out["masked_lm_labels"], torch.int64, "out masked_lm_labels")
    _c(out["masked_feat"], feats.dtype, "out masked_feat"), _c(out["feat_mask"], F32, "out feat_mask")
    _c(out["ans"], torch.int64, "out ans")
    if (out["input_ids"].numel() != B * T or out["masked_lm_labels"].numel() != B * T or out["masked_feat"].numel() != B * O * F
            or out["feat_mask"].numel() != B * O or out["ans"].numel() != B):
        raise ValueError("pretrain_corrupt: output buffers do not fit B=%d T=%d O=%d F=%d" % (B, T, O, F))
    for t in (input_ids, input_mask, is_matched, label_ids, label_scores, pool, rng) + tuple(draws.values()) + tuple(out.values()):
        if t is not None and t.device != dev:
            raise RuntimeError("pretrain_corrupt: all operands must live on one device")
    a.feats, a.masked_feat, a.feat_mask = ptr(feats), ptr(out["masked_feat"]), ptr(out["feat_mask"])
    a.input_ids, a.input_mask = ptr(input_ids), ptr(input_mask)
    a.input_ids_out, a.masked_lm_labels = ptr(out["input_ids"]), ptr(out["masked_lm_labels"])
    a.label_ids, a.label_scores, a.is_matched, a.ans = ptr(label_ids), ptr(label_scores), ptr(is_matched), ptr(out["ans"])
    a.B, a.T, a.O, a.F, a.K = B, T, O, F, K
    a.vocab_size, a.mask_id = int(vocab_size), int(mask_id)
    a.word_mask_rate, a.obj_mask_rate = float(word_mask_rate), float(obj_mask_rate)
    a.rng, a.sid_base = ptr(rng), int(sid_base)
    call("xggm_pretrain_corrupt_" + sfx(feats.dtype), _ct.addressof(a), stream())
    return out


PRETRAIN_SWAP_TRIES = 8                      # XGGM_PRETRAIN_SWAP_TRIES (include/xggm.h)
PRETRAIN_SWAP_DRAWS = ("u_swap", "u_pick")   # Philox streams sid_base + 5, sid_base + 6: behind PRETRAIN_DRAWS


class PretrainSwapArgs(_ct.Structure):
    """mirror of ``xggm_pretrain_swap_args`` (include/xggm.h)"""
    _fields_ = [("ids", _ct.c_void_p), ("mask", _ct.c_void_p), ("img", _ct.c_void_p), ("matched_in", _ct.c_void_p),
                ("pool_ids", _ct.c_void_p), ("pool_mask", _ct.c_void_p), ("pool_img", _ct.c_void_p), ("out_ids", _ct.c_void_p),
                ("out_mask", _ct.c_void_p), ("is_matched", _ct.c_void_p), ("exhausted", _ct.c_void_p), ("B", _ct.c_int),
                ("T", _ct.c_int), ("P", _ct.c_int64), ("rate", _ct.c_double), ("u_swap", _ct.c_void_p), ("u_pick", _ct.c_void_p),
                ("rng", _ct.c_void_p), ("sid_base", _ct.c_uint32)]


def pretrain_swap(ids, mask, img, rate=0.5, matched_in=None, pool=None, rng=None, sid_base=0, draws=None, out=None):
    """the matched-sentence swap of src/pretrain/lxmert_data.py:173-183 for a clean batch on the device, one launch;
    contract: xggm_pretrain_swap in xggm.h.  ``ids`` / ``mask`` [B, T] int64, ``img`` [B] int64 (a key per image),
    ``matched_in`` [B] int64 or None (all 1), ``pool``: None (the batch's own rows) or (pool_ids [P, T], pool_mask [P, T],
    pool_img [P]).  ``draws``: a dict with any of ``PRETRAIN_SWAP_DRAWS`` (fp32; u_swap [B], u_pick [B, 8]); a missing one is
    drawn from ``rng`` at stream ``sid_base + 5`` / ``+ 6``.  ``out``: a dict of the four outputs to write into (else they
    are allocated; a fresh ``exhausted`` starts at 0, a supplied one is added to).
    -> dict(input_ids, input_mask, is_matched, exhausted)"""
    _c(ids, torch.int64, "ids"), _c(mask, torch.int64, "mask"), _c(img, torch.int64, "img")
    if ids.dim() != 2 or tuple(mask.shape) != tuple(ids.shape) or img.numel() != ids.shape[0]:
        raise ValueError("pretrain_swap: ids / mask [B, T] and img [B] expected, got %s %s %s"
                         % (tuple(ids.shape), tuple(mask.shape), tuple(img.shape)))
    B, T = ids.shape
    if min(B, T) <= 0:
        raise ValueError("pretrain_swap: empty batch B=%d T=%d" % (B, T))
    dev = ids.device
    a = PretrainSwapArgs()
    if matched_in is not None:
        _c(matched_in, torch.int64, "matched_in")
        if matched_in.numel() != B:
            raise ValueError("pretrain_swap: matched_in has %d entries, %d expected" % (matched_in.numel(), B))
    pool = tuple(pool) if pool is not None else ()
    if pool:
        if len(pool) != 3 or any(t is None for t in pool):
            raise ValueError("pretrain_swap: pool is (pool_ids, pool_mask, pool_img)")
        for t, name in zip(pool, ("pool_ids", "pool_mask", "pool_img")):
            _c(t, torch.int64, name)
        P = pool[2].numel()
        if P <= 0 or tuple(pool[0].shape) != (P, T) or tuple(pool[1].shape) != (P, T):
            raise ValueError("pretrain_swap: pool %s %s %s is no ([P, %d], [P, %d], [P])"
                             % (tuple(pool[0].shape), tuple(pool[1].shape), tuple(pool[2].shape), T, T))
        a.pool_ids, a.pool_mask, a.pool_img, a.P = ptr(pool[0]), ptr(pool[1]), ptr(pool[2]), P
    draws = dict(draws or {})
    sizes = dict(u_swap=B, u_pick=B * PRETRAIN_SWAP_TRIES)
    if set(draws) - set(sizes):
        raise ValueError("pretrain_swap: unknown draws %s" % sorted(set(draws) - set(sizes)))
    for k, n in sizes.items():
        d = draws.get(k)
        if d is not None:
            _c(d, F32, k)
            if d.numel() != n:
                raise ValueError("pretrain_swap: %s has %d draws, %d expected" % (k, d.numel(), n))
        setattr(a, k, ptr(d))
    if rng is None:
        if any(draws.get(k) is None for k in sizes):
            raise ValueError("pretrain_swap: a missing draw buffer needs rng")
    else:
        _c(rng, torch.int64, "rng")
    if not 0.0 <= float(rate) <= 1.0:
        raise ValueError("pretrain_swap: rate %r outside [0, 1]" % (rate,))
    if out is None:
        out = dict(input_ids=torch.empty_like(ids), input_mask=torch.empty_like(mask),
                   is_matched=torch.empty(B, device=dev, dtype=torch.int64), exhausted=torch.zeros(1, device=dev, dtype=torch.int32))
    _c(out["input_ids"], torch.int64, "out input_ids"), _c(out["input_mask"], torch.int64, "out input_mask")
    _c(out["is_matched"], torch.int64, "out is_matched"), _c(out["exhausted"], torch.int32, "out exhausted")
    if (out["input_ids"].numel() != B * T or out["input_mask"].numel() != B * T or out["is_matched"].numel() != B
            or out["exhausted"].numel() != 1):
        raise ValueError("pretrain_swap: output buffers do not fit B=%d T=%d" % (B, T))
    for t in (mask, img, matched_in, rng) + pool + tuple(draws.values()) + tuple(out.values()):
        if t is not None and t.device != dev:
            raise RuntimeError("pretrain_swap: all operands must live on one device")
    a.ids, a.mask, a.img, a.matched_in = ptr(ids), ptr(mask), ptr(img), ptr(matched_in)
    a.out_ids, a.out_mask, a.is_matched, a.exhausted = ptr(out["input_ids"]), ptr(out["input_mask"]), ptr(out["is_matched"]), ptr(out["exhausted"])
    a.B, a.T, a.rate = B, T, float(rate)
    a.rng, a.sid_base = ptr(rng), int(sid_base)
    call("xggm_pretrain_swap", _ct.addressof(a), stream())
    return out


# ----------------------------------------------------------------------------- resident data set
class BatchGatherArgs(_ct.Structure):
    """mirror of ``xggm_batch_gather_args`` (include/xggm.h)"""
    _fields_ = [("feats", _ct.c_void_p), ("boxes", _ct.c_void_p), ("adj", _ct.c_void_p), ("q_row", _ct.c_void_p),
                ("q_ids", _ct.c_void_p), ("q_len", _ct.c_void_p), ("q_label", _ct.c_void_p), ("q_score", _ct.c_void_p),
                ("q_bias_index", _ct.c_void_p), ("order", _ct.c_void_p), ("n", _ct.c_int64), ("start", _ct.c_int64),
                ("out_feats", _ct.c_void_p), ("out_feats_stride", _ct.c_int64), ("out_boxes", _ct.c_void_p),
                ("out_adj", _ct.c_void_p), ("input_ids", _ct.c_void_p), ("input_mask", _ct.c_void_p),
                ("segment_ids", _ct.c_void_p), ("target", _ct.c_void_p), ("target_stride", _ct.c_int64),
                ("bias_index", _ct.c_void_p), ("sample", _ct.c_void_p), ("B", _ct.c_int), ("T", _ct.c_int), ("K", _ct.c_int),
                ("A", _ct.c_int), ("N", _ct.c_int), ("F", _ct.c_int), ("feats_f32", _ct.c_int), ("out_f32", _ct.c_int)]


class LabelAdjArgs(_ct.Structure):
    """mirror of ``xggm_label_adj_args`` (include/xggm.h)"""
    _fields_ = [("table", _ct.c_void_p), ("obj_labels", _ct.c_void_p), ("attr_labels", _ct.c_void_p), ("Vc", _ct.c_int),
                ("Va", _ct.c_int)]


def _rows_of(t, B, row, name, who="batch_gather"):
    """``t``: at least B rows of shape ``row`` whose insides are contiguous (the row stride is free) -> row stride"""
    if t.dim() != 1 + len(row) or tuple(t.shape[1:]) != tuple(row) or t.shape[0] < B:
        raise ValueError("%s: %s is %s, at least [%d, %s] expected" % (who, name, tuple(t.shape), B, ", ".join(map(str, row))))
    if not t[0].is_contiguous():
        raise RuntimeError("xggm_amd: the rows of %s must be contiguous" % name)
    return t.stride(0) if t.shape[0] > 1 else max(t.stride(0), t[0].numel())


def batch_gather(tables, order, start, B, out):
    """rows ``order[start : start + B]`` of a device-resident split into the batch buffers ``out``, one launch; contract:
    xggm_batch_gather in xggm.h.  ``tables``: feats [n_img, N, F] bf16 / fp32, boxes [n_img, N, 4], adj [n_img, N, N] or None,
    q_row [n_q] int32, q_ids [n_q, T] int32, q_len [n_q] int32, q_label [n_q, K] int32, q_score [n_q, K] fp32, q_bias_index
    [n_q] int64 or None.  Instead of adj a store may hold pair_table [Vc, Va] fp32 with obj_labels / attr_labels [n_img, N]
    int32 (1 <= N <= 128, ids inside the table: validated by the store): adj_true is then made in the launch
    (xggm_batch_gather_labels); both at once are refused.  ``order``: [n] int64.  ``out``: feats (bf16 / fp32; the row stride is free), boxes, input_ids,
    input_mask, segment_ids and any of adj_true, target (row stride free), bias_index, sample; each with at least B rows,
    rows past B are not touched.  The indices inside the tables are trusted (``tools.resident.ResidentDataset`` validates
    them once at upload); every shape is checked here."""
    tb, dev = tables, order.device
    for k in ("feats", "boxes", "q_row", "q_ids", "q_len", "q_label", "q_score"):
        _c(tb[k], None, "table " + k)
    _c(order, torch.int64, "order")
    feats, boxes, adj, bias = tb["feats"], tb["boxes"], tb.get("adj"), tb.get("q_bias_index")
    if feats.dtype not in (BF16, F32) or feats.dim() != 3:
        raise TypeError("batch_gather: feature table %s %s, [n_img, N, F] bfloat16 or float32 expected" % (tuple(feats.shape), feats.dtype))
    n_img, N, F = feats.shape
    _c(boxes, F32, "table boxes"), _c(tb["q_row"], torch.int32, "q_row"), _c(tb["q_ids"], torch.int32, "q_ids")
    _c(tb["q_len"], torch.int32, "q_len"), _c(tb["q_label"], torch.int32, "q_label"), _c(tb["q_score"], F32, "q_score")
    n_q = tb["q_row"].numel()
    if tb["q_ids"].dim() != 2 or tb["q_label"].dim() != 2:
        raise ValueError("batch_gather: q_ids [n_q, T] and q_label [n_q, K] expected")
    T, K = tb["q_ids"].shape[1], tb["q_label"].shape[1]
    if (tuple(boxes.shape) != (n_img, N, 4) or tb["q_row"].dim() != 1 or tb["q_ids"].shape[0] != n_q or tuple(tb["q_len"].shape) != (n_q,)
            or tb["q_label"].shape[0] != n_q or tuple(tb["q_score"].shape) != (n_q, K)):
        raise ValueError("batch_gather: the tables do not fit n_img=%d N=%d n_q=%d T=%d K=%d" % (n_img, N, n_q, T, K))
    if adj is not None and (_c(adj, F32, "table adj").shape != (n_img, N, N)):
        raise ValueError("batch_gather: adjacency table %s, [%d, %d, %d] expected" % (tuple(adj.shape), n_img, N, N))
    if bias is not None and tuple(_c(bias, torch.int64, "q_bias_index").shape) != (n_q,):
        raise ValueError("batch_gather: q_bias_index %s, [%d] expected" % (tuple(bias.shape), n_q))
    pair = tb.get("pair_table")
    if pair is not None:
        if adj is not None:
            raise ValueError("batch_gather: the tables hold a stored adjacency AND a pair table (one source of adj_true only)")
        ol, al = tb.get("obj_labels"), tb.get("attr_labels")
        if ol is None or al is None:
            raise ValueError("batch_gather: a pair table needs the tables obj_labels and attr_labels")
        if _c(pair, F32, "pair_table").dim() != 2 or min(pair.shape) < 1:
            raise ValueError("batch_gather: pair table %s, [Vc, Va] expected" % (tuple(pair.shape),))
        if tuple(_c(ol, torch.int32, "obj_labels").shape) != (n_img, N) or tuple(_c(al, torch.int32, "attr_labels").shape) != (n_img, N):
            raise ValueError("batch_gather: label tables %s and %s, [%d, %d] expected" % (tuple(ol.shape), tuple(al.shape), n_img, N))
        if N > 128:
            raise ValueError("batch_gather: N=%d objects, the label adjacency serves 1 .. 128" % N)
    if min(n_img, n_q, N, F, T, K) < 1:
        raise ValueError("batch_gather: empty tables")
    if F % 8:
        raise ValueError("batch_gather: F=%d is no multiple of 8 (feature rows move 16 bytes per lane)" % F)
    start, B, n = int(start), int(B), order.numel()
    if order.dim() != 1 or B < 1 or start < 0 or start + B > n:
        raise ValueError("batch_gather: rows %d .. %d of an order of %d" % (start, start + B, n))
    unknown = set(out) - {"feats", "boxes", "adj_true", "input_ids", "input_mask", "segment_ids", "target", "bias_index", "sample"}
    if unknown:
        raise ValueError("batch_gather: unknown outputs %s" % sorted(unknown))
    a = BatchGatherArgs()
    of = _chk(out["feats"], None, "out feats")
    if of.dtype not in (BF16, F32):
        raise TypeError("batch_gather: out feats %s, bfloat16 or float32 expected" % of.dtype)
    a.out_feats_stride = _rows_of(of, B, (N, F), "out feats")
    _rows_of(_c(out["boxes"], F32, "out boxes"), B, (N, 4), "out boxes")
    for k in ("input_ids", "input_mask", "segment_ids"):
        _rows_of(_c(out[k], torch.int64, "out " + k), B, (T,), "out " + k)
    oa, tg, ob, sm = out.get("adj_true"), out.get("target"), out.get("bias_index"), out.get("sample")
    if oa is not None:
        if adj is None and pair is None:
            raise ValueError("batch_gather: the tables hold no adjacency for out adj_true")
        _rows_of(_c(oa, F32, "out adj_true"), B, (N, N), "out adj_true")
    if tg is not None:
        if _chk(tg, F32, "out target").dim() != 2:
            raise ValueError("batch_gather: out target %s, [B, A] expected" % (tuple(tg.shape),))
        a.A = tg.shape[1]
        a.target_stride = _rows_of(tg, B, (a.A,), "out target")
    else:
        a.A, a.target_stride = 1, 1
    if ob is not None:
        if bias is None:
            raise ValueError("batch_gather: the tables hold no q_bias_index for out bias_index")
        _rows_of(_c(ob, torch.int64, "out bias_index"), B, (), "out bias_index")
    if sm is not None:
        _rows_of(_c(sm, torch.int64, "out sample"), B, (), "out sample")
    for t in list(tb.values()) + list(out.values()):
        if t is not None and t.device != dev:
            raise RuntimeError("batch_gather: all operands must live on one device")
    a.feats, a.boxes, a.adj, a.q_row, a.q_ids, a.q_len = ptr(feats), ptr(boxes), ptr(adj), ptr(tb["q_row"]), ptr(tb["q_ids"]), ptr(tb["q_len"])
    a.q_label, a.q_score, a.q_bias_index = ptr(tb["q_label"]), ptr(tb["q_score"]), ptr(bias)
    a.order, a.n, a.start = ptr(order), n, start
    a.out_feats, a.out_boxes, a.out_adj = ptr(of), ptr(out["boxes"]), ptr(oa)
    a.input_ids, a.input_mask, a.segment_ids = ptr(out["input_ids"]), ptr(out["input_mask"]), ptr(out["segment_ids"])
    a.target, a.bias_index, a.sample = ptr(tg), ptr(ob), ptr(sm)
    a.B, a.T, a.K, a.N, a.F = B, T, K, N, F
    a.feats_f32, a.out_f32 = int(feats.dtype == F32), int(of.dtype == F32)
    if pair is not None:
        l = LabelAdjArgs()
        l.table, l.obj_labels, l.attr_labels, l.Vc, l.Va = ptr(pair), ptr(tb["obj_labels"]), ptr(tb["attr_labels"]), pair.shape[0], pair.shape[1]
        call("xggm_batch_gather_labels", _ct.addressof(a), _ct.addressof(l), stream())
    else:
        call("xggm_batch_gather", _ct.addressof(a), stream())
    return out


class PretrainGatherArgs(_ct.Structure):
    """mirror of ``xggm_pretrain_gather_args`` (include/xggm.h)"""
    _fields_ = ([(k, _ct.c_void_p) for k in ("feats", "boxes", "obj_labels", "attr_labels", "obj_confs", "attr_confs", "q_row",
                                             "q_ids", "q_len", "q_label", "q_score", "order")]
                + [(k, _ct.c_int64) for k in ("n_img", "n_q", "n", "start")]
                + [("out_feats", _ct.c_void_p), ("out_feats_stride", _ct.c_int64)]
                + [(k, _ct.c_void_p) for k in ("out_boxes", "out_obj_labels", "out_attr_labels", "out_obj_confs", "out_attr_confs",
                                               "input_ids", "input_mask", "segment_ids", "label_ids", "label_scores", "is_matched",
                                               "img_ids", "sample", "swapped_from")]
                + [(k, _ct.c_int) for k in ("B", "T", "K", "O", "F", "feats_f32", "out_f32", "swap")]
                + [("rate", _ct.c_double), ("u_swap", _ct.c_void_p), ("u_pick", _ct.c_void_p), ("rng", _ct.c_void_p),
                   ("sid_base", _ct.c_uint32), ("exhausted", _ct.c_void_p)])


PRETRAIN_GATHER_TABLES = ("feats", "boxes", "obj_labels", "attr_labels", "obj_confs", "attr_confs", "q_row", "q_ids", "q_len",
                          "q_label", "q_score")
# the clean batch of ``engine.CapturedPretrainer.KEYS`` plus img_ids; sample and swapped_from are optional
PRETRAIN_GATHER_OUT = ("input_ids", "input_mask", "segment_ids", "feats", "boxes", "obj_labels", "obj_confs", "attr_labels",
                       "attr_confs", "is_matched", "label_ids", "label_scores", "img_ids")


def pretrain_gather(tables, order, start, B, out, match_rate=None, rng=None, sid_base=0, draws=None, exhausted=None):
    """rows ``order[start : start + B]`` of a device-resident pre-training corpus into the clean batch buffers ``out``, the
    matched-sentence swap fused in, one launch; contract: xggm_pretrain_gather in xggm.h.  ``tables``
    (``PRETRAIN_GATHER_TABLES``): feats [n_img, O, F] bf16 / fp32, boxes [n_img, O, 4], obj_labels / attr_labels [n_img, O]
    int32, obj_confs / attr_confs [n_img, O] fp32, q_row [n_q] int32, q_ids [n_q, T] int32, q_len [n_q] int32, q_label
    [n_q, K] int32, q_score [n_q, K] fp32.  ``order``: [n] int64.  ``out``: every name of ``PRETRAIN_GATHER_OUT`` (feats bf16 /
    fp32 with a free row stride) and optionally sample, swapped_from; each with at least B rows, rows past B are not touched.
    ``match_rate`` (None: no swap, no draw is read): a row swaps iff its u_swap < match_rate and then takes the sentence of
    the first of ``PRETRAIN_SWAP_TRIES`` candidates of another image out of ALL samples of the tables.  ``draws``: a dict with
    any of ``PRETRAIN_SWAP_DRAWS`` (fp32; u_swap [B], u_pick [B, 8]); a missing one is drawn from ``rng`` at stream
    ``sid_base + 5`` / ``+ 6``.  ``exhausted``: int32 [1], added to (needed with a swap).  The indices inside the tables are
    trusted (``pretrain.resident.pretrain_tables`` validates them once); every shape is checked here."""
    who = "pretrain_gather"
    tb, dev = tables, order.device
    missing = [k for k in PRETRAIN_GATHER_TABLES if tb.get(k) is None]
    if missing:
        raise ValueError("%s: the tables lack %s" % (who, missing))
    _c(order, torch.int64, "order")
    feats = _c(tb["feats"], None, "table feats")
    if feats.dtype not in (BF16, F32) or feats.dim() != 3:
        raise TypeError("%s: feature table %s %s, [n_img, O, F] bfloat16 or float32 expected" % (who, tuple(feats.shape), feats.dtype))
    n_img, O, F = feats.shape
    for k, dt in (("boxes", F32), ("obj_labels", torch.int32), ("attr_labels", torch.int32), ("obj_confs", F32), ("attr_confs", F32),
                  ("q_row", torch.int32), ("q_ids", torch.int32), ("q_len", torch.int32), ("q_label", torch.int32), ("q_score", F32)):
        _c(tb[k], dt, "table " + k)
    n_q = tb["q_row"].numel()
    if tb["q_ids"].dim() != 2 or tb["q_label"].dim() != 2:
        raise ValueError("%s: q_ids [n_q, T] and q_label [n_q, K] expected" % who)
    T, K = tb["q_ids"].shape[1], tb["q_label"].shape[1]
    if (tuple(tb["boxes"].shape) != (n_img, O, 4) or any(tuple(tb[k].shape) != (n_img, O) for k in ("obj_labels", "attr_labels", "obj_confs", "attr_confs"))
            or tb["q_row"].dim() != 1 or tb["q_ids"].shape[0] != n_q or tuple(tb["q_len"].shape) != (n_q,)
            or tb["q_label"].shape[0] != n_q or tuple(tb["q_score"].shape) != (n_q, K)):
        raise ValueError("%s: the tables do not fit n_img=%d O=%d n_q=%d T=%d K=%d" % (who, n_img, O, n_q, T, K))
    if min(n_img, n_q, O, F, T, K) < 1:
        raise ValueError("%s: empty tables" % who)
    if F % 8:
        raise ValueError("%s: F=%d is no multiple of 8 (feature rows move 16 bytes per lane)" % (who, F))
    start, B, n = int(start), int(B), order.numel()
    if order.dim() != 1 or B < 1 or start < 0 or start + B > n:
        raise ValueError("%s: rows %d .. %d of an order of %d" % (who, start, start + B, n))
    unknown = set(out) - set(PRETRAIN_GATHER_OUT) - {"sample", "swapped_from"}
    lacking = [k for k in PRETRAIN_GATHER_OUT if out.get(k) is None]
    if unknown or lacking:
        raise ValueError("%s: unknown outputs %s, missing outputs %s" % (who, sorted(unknown), lacking))
    a = PretrainGatherArgs()
    of = _chk(out["feats"], None, "out feats")
    if of.dtype not in (BF16, F32):
        raise TypeError("%s: out feats %s, bfloat16 or float32 expected" % (who, of.dtype))
    a.out_feats_stride = _rows_of(of, B, (O, F), "out feats", who)
    for k, dt, row in (("boxes", F32, (O, 4)), ("obj_labels", torch.int64, (O,)), ("attr_labels", torch.int64, (O,)),
                       ("obj_confs", F32, (O,)), ("attr_confs", F32, (O,)), ("input_ids", torch.int64, (T,)),
                       ("input_mask", torch.int64, (T,)), ("segment_ids", torch.int64, (T,)), ("label_ids", torch.int64, (K,)),
                       ("label_scores", F32, (K,)), ("is_matched", torch.int64, ()), ("img_ids", torch.int64, ()),
                       ("sample", torch.int64, ()), ("swapped_from", torch.int64, ())):
        if out.get(k) is not None:
            _rows_of(_c(out[k], dt, "out " + k), B, row, "out " + k, who)
    draws = dict(draws or {})
    sizes = dict(u_swap=B, u_pick=B * PRETRAIN_SWAP_TRIES)
    if set(draws) - set(sizes):
        raise ValueError("%s: unknown draws %s" % (who, sorted(set(draws) - set(sizes))))
    if match_rate is None:
        if draws:
            raise ValueError("%s: swap draws %s without a match_rate" % (who, sorted(draws)))
    else:
        if not 0.0 <= float(match_rate) <= 1.0:
            raise ValueError("%s: match_rate %r outside [0, 1]" % (who, match_rate))
        for k, m in sizes.items():
            d = draws.get(k)
            if d is not None and _c(d, F32, k).numel() != m:
                raise ValueError("%s: %s has %d draws, %d expected" % (who, k, d.numel(), m))
            setattr(a, k, ptr(d))
        if rng is None:
            if any(draws.get(k) is None for k in sizes):
                raise ValueError("%s: a missing draw buffer needs rng" % who)
        else:
            _c(rng, torch.int64, "rng")
        if exhausted is None or _c(exhausted, torch.int32, "exhausted").numel() != 1:
            raise ValueError("%s: a swap needs exhausted, int32 [1]" % who)
        a.swap, a.rate, a.rng, a.exhausted = 1, float(match_rate), ptr(rng), ptr(exhausted)
    for t in [tb[k] for k in PRETRAIN_GATHER_TABLES] + list(out.values()) + list(draws.values()) + [rng, exhausted]:
        if t is not None and t.device != dev:
            raise RuntimeError("%s: all operands must live on one device" % who)
    for k in PRETRAIN_GATHER_TABLES + ("order",):
        setattr(a, k, ptr(order if k == "order" else tb[k]))
    a.n_img, a.n_q, a.n, a.start = n_img, n_q, n, start
    a.out_feats, a.out_boxes = ptr(of), ptr(out["boxes"])
    a.out_obj_labels, a.out_attr_labels = ptr(out["obj_labels"]), ptr(out["attr_labels"])
    a.out_obj_confs, a.out_attr_confs = ptr(out["obj_confs"]), ptr(out["attr_confs"])
    for k in ("input_ids", "input_mask", "segment_ids", "label_ids", "label_scores", "is_matched", "img_ids", "sample", "swapped_from"):
        setattr(a, k, ptr(out.get(k)))
    a.B, a.T, a.K, a.O, a.F = B, T, K, O, F
    a.feats_f32, a.out_f32, a.sid_base = int(feats.dtype == F32), int(of.dtype == F32), int(sid_base)
    call("xggm_pretrain_gather", _ct.addressof(a), stream())
    return out


# ----------------------------------------------------------------------------- tokenisation
class TokenizeArgs(_ct.Structure):
    """mirror of ``xggm_tokenize_args`` (include/xggm.h)"""
    _fields_ = [("bytes", _ct.c_void_p), ("n_bytes", _ct.c_int64), ("offsets", _ct.c_void_p), ("host_offsets", _ct.c_void_p),
                ("n", _ct.c_int64), ("T", _ct.c_int), ("cp_table", _ct.c_void_p), ("cp_ext", _ct.c_void_p), ("n_ext", _ct.c_int64),
                ("init_slots", _ct.c_void_p), ("init_cap", _ct.c_int64), ("cont_slots", _ct.c_void_p), ("cont_cap", _ct.c_int64),
                ("blob", _ct.c_void_p), ("n_blob", _ct.c_int64), ("never_cps", _ct.c_void_p), ("never_off", _ct.c_void_p),
                ("n_never", _ct.c_int), ("cls_id", _ct.c_int32), ("sep_id", _ct.c_int32), ("unk_id", _ct.c_int32),
                ("ids", _ct.c_void_p), ("len", _ct.c_void_p), ("block", _ct.c_void_p), ("flags", _ct.c_void_p),
                ("flagged", _ct.c_void_p)]


TOKENIZE_OUTPUTS = ("ids", "len", "block", "flags", "flagged")
TOKENIZE_TABLES = ("cp_table", "cp_ext", "init_slots", "cont_slots", "blob", "never_cps", "never_off")


def tokenize_wordpiece(data, offsets, host_offsets, T, tables, outputs=("ids", "len", "flags", "flagged"), out=None):
    """WordPiece token ids of n sentences in ONE launch; contract: xggm_tokenize_wordpiece in xggm.h.  ``data`` uint8
    [n_bytes]: the sentences' UTF-8; ``offsets`` int64 [n + 1] on the device and ``host_offsets``, the same values as a
    numpy int64 array (checked on the host before the launch); ``tables``: the device tensors and ids of
    ``lxrt.tokenization.DeviceTokenizer.tables``.  ``outputs``: which of ``TOKENIZE_OUTPUTS`` to produce -- ids int32
    [n, T], len int32 [n], block int64 [3, n, T] (input_ids, input_mask, segment_ids), flags uint8 [n] (1: the row needs
    the host tokenizer), flagged int32 [1] (their number; a fresh one starts at 0, a supplied one is added to) -- into
    ``out`` (a dict) where it holds them.  -> dict of the outputs"""
    import numpy as np
    _c(data, torch.uint8, "data"), _c(offsets, torch.int64, "offsets")
    dev = data.device
    host_offsets = np.ascontiguousarray(host_offsets, dtype=np.int64)
    n, T = offsets.numel() - 1, int(T)
    if n < 1 or host_offsets.shape != (n + 1,):
        raise ValueError("tokenize_wordpiece: offsets hold %d values, host_offsets %s" % (n + 1, host_offsets.shape))
    if set(outputs) - set(TOKENIZE_OUTPUTS) or not outputs:
        raise ValueError("tokenize_wordpiece: outputs %r, some of %r expected" % (outputs, TOKENIZE_OUTPUTS))
    a = TokenizeArgs()
    for k in TOKENIZE_TABLES:
        _c(tables[k], torch.int32, k)
        setattr(a, k, ptr(tables[k]))
    if tables["init_slots"].dim() != 2 or tables["init_slots"].shape[1] != 4 or tables["cont_slots"].dim() != 2 \
            or tables["cont_slots"].shape[1] != 4 or tables["cp_table"].numel() != 0x110000:
        raise ValueError("tokenize_wordpiece: slots are [capacity, 4], cp_table holds 0x110000 entries")
    a.n_ext, a.n_blob = min(int(tables["n_ext"]), tables["cp_ext"].numel()), min(int(tables["n_blob"]), tables["blob"].numel())
    a.init_cap, a.cont_cap = tables["init_slots"].shape[0], tables["cont_slots"].shape[0]
    a.n_never = tables["never_off"].numel() - 1
    if tables["never_cps"].numel() < int(tables["never_end"]):
        raise ValueError("tokenize_wordpiece: never_off points past never_cps")
    a.cls_id, a.sep_id, a.unk_id = int(tables["cls_id"]), int(tables["sep_id"]), int(tables["unk_id"])
    shapes = dict(ids=((n, T), torch.int32), len=((n,), torch.int32), block=((3, n, T), torch.int64),
                  flags=((n,), torch.uint8), flagged=((1,), torch.int32))
    res = {}
    for k in outputs:
        shape, dt = shapes[k]
        t = (out or {}).get(k)
        if t is None:
            t = torch.zeros(1, device=dev, dtype=dt) if k == "flagged" else torch.empty(shape, device=dev, dtype=dt)
        _c(t, dt, "out " + k)
        if tuple(t.shape) != shape:
            raise ValueError("tokenize_wordpiece: out %s is %s, %s expected" % (k, tuple(t.shape), shape))
        res[k] = t
        setattr(a, k, ptr(t))
    for t in [offsets] + [tables[k] for k in TOKENIZE_TABLES] + list(res.values()):
        if t.device != dev:
            raise RuntimeError("tokenize_wordpiece: all operands must live on one device")
    a.bytes, a.n_bytes, a.offsets, a.host_offsets = ptr(data), data.numel(), ptr(offsets), host_offsets.ctypes.data
    a.n, a.T = n, T
    call("xggm_tokenize_wordpiece", _ct.addressof(a), stream())
    return res


# ----------------------------------------------------------------------------- feature files
class TsvDecodeArgs(_ct.Structure):
    """mirror of ``xggm_tsv_decode_args`` (include/xggm.h)"""
    _fields_ = [("text", _ct.c_void_p), ("n_bytes", _ct.c_int64), ("alloc_bytes", _ct.c_int64), ("desc", _ct.c_void_p),
                ("host_desc", _ct.c_void_p), ("n", _ct.c_int64), ("O", _ct.c_int), ("F", _ct.c_int), ("feats_bf16", _ct.c_int),
                ("normalize", _ct.c_int), ("row0", _ct.c_int64), ("capacity", _ct.c_int64), ("feats", _ct.c_void_p),
                ("boxes", _ct.c_void_p), ("obj_labels", _ct.c_void_p), ("attr_labels", _ct.c_void_p), ("obj_confs", _ct.c_void_p),
                ("attr_confs", _ct.c_void_p), ("flags", _ct.c_void_p), ("counts", _ct.c_void_p)]


TSV_TABLES = ("feats", "boxes", "obj_labels", "attr_labels", "obj_confs", "attr_confs")
TSV_DESC = 14  # XGGM_TSV_DESC


def tsv_decode(text, n_bytes, desc, host_desc, O, F, tables, row0, flags=None, counts=None, normalize=True):
    """the six base64 fields of n TSV lines -> rows [row0, row0 + n) of ``tables`` in ONE launch; contract: xggm_tsv_decode
    in xggm.h.  ``text`` uint8 [allocation, a multiple of 16] of which the first ``n_bytes`` are text; ``desc`` int64
    [n, 14] on the device and ``host_desc``, the same values as a numpy int64 array (checked on the host before the
    launch): what ``tools.tsv.scan_chunk`` returns.  ``tables``: dict with some of ``TSV_TABLES`` -- feats [cap, O, F] bf16
    or fp32, boxes [cap, O, 4] fp32, obj_labels / attr_labels [cap, O] int32, obj_confs / attr_confs [cap, O] fp32, one
    capacity.  ``flags`` int32 [n] (the kernel's uint32 bit patterns), ``counts`` int32 [2] (added to).  -> tables"""
    import numpy as np
    who = "tsv_decode"
    _c(text, torch.uint8, "text"), _c(desc, torch.int64, "desc")
    dev, O, F = text.device, int(O), int(F)
    host_desc = np.ascontiguousarray(host_desc, dtype=np.int64)
    n = desc.shape[0] if desc.dim() == 2 else -1
    if n < 1 or desc.shape[1] != TSV_DESC or host_desc.shape != (n, TSV_DESC):
        raise ValueError("%s: desc is %s, host_desc %s, [n >= 1, %d] expected of both" % (who, tuple(desc.shape), host_desc.shape, TSV_DESC))
    if set(tables) - set(TSV_TABLES):
        raise ValueError("%s: tables %r, some of %r expected" % (who, sorted(tables), TSV_TABLES))
    a = TsvDecodeArgs()
    cap = None
    want = dict(feats=((O, F), None), boxes=((O, 4), F32), obj_labels=((O,), torch.int32), attr_labels=((O,), torch.int32),
                obj_confs=((O,), F32), attr_confs=((O,), F32))
    for k, t in tables.items():
        shape, dt = want[k]
        _c(t, dt, k)
        if k == "feats" and t.dtype not in (F32, BF16):
            raise TypeError("%s: feats are %s, bfloat16 or float32 expected" % (who, t.dtype))
        if tuple(t.shape[1:]) != shape or t.dim() != len(shape) + 1 or (cap is not None and t.shape[0] != cap):
            raise ValueError("%s: table %s is %s, [%s, %s] expected" % (who, k, tuple(t.shape), cap if cap is not None else "capacity",
                                                                      ", ".join(map(str, shape))))
        cap = t.shape[0]
        setattr(a, k, ptr(t))
    if flags is not None and _c(flags, torch.int32, "flags").shape != (n,):
        raise ValueError("%s: flags hold %s, [%d] expected" % (who, tuple(flags.shape), n))
    if counts is not None and _c(counts, torch.int32, "counts").numel() != 2:
        raise ValueError("%s: counts int32 [2] expected" % who)
    for t in [desc] + list(tables.values()) + [flags, counts]:
        if t is not None and t.device != dev:
            raise RuntimeError("%s: all operands must live on one device" % who)
    a.text, a.n_bytes, a.alloc_bytes, a.desc, a.host_desc = ptr(text), int(n_bytes), text.numel(), ptr(desc), host_desc.ctypes.data
    a.n, a.O, a.F, a.normalize, a.row0, a.capacity = n, O, F, int(bool(normalize)), int(row0), int(row0) + n if cap is None else cap  # no table: flags / counts alone
    a.feats_bf16 = int("feats" in tables and tables["feats"].dtype == BF16)
    a.flags, a.counts = ptr(flags), ptr(counts)
    call("xggm_tsv_decode", _ct.addressof(a), stream())
    return tables


# ----------------------------------------------------------------------------- graph attention
def gat_att_fwd(s, adj, alpha, long=False):
    _c(s, F32, "s"), _c(adj, F32, "adj")
    B, N, _ = adj.shape
    assert tuple(s.shape) == (B * N, 2)
    att = torch.empty_like(adj)
    call(_lg("xggm_gat_att", N, long, "_fwd"), ptr(s), ptr(adj), ptr(att), B, N, float(alpha), stream())
    return att


def gat_att_bwd(d_att, att, s, adj, alpha, dt, long=False):
    _c(d_att, F32), _c(att, F32), _c(s, F32), _c(adj, F32)
    B, N, _ = adj.shape
    ds = torch.empty((B * N, 2), device=adj.device, dtype=dt)
    call(_lg("xggm_gat_att", N, long, "_bwd_" + sfx(dt)), ptr(d_att), ptr(att), ptr(s), ptr(adj), ptr(ds), B, N, float(alpha), stream())
    return ds


def elu_fwd(x, out, col0):
    """out[:, col0:col0+D] = elu(x) for contiguous x [M,D] and a contiguous wider out [M,ld]."""
    _c(x), _c(out, x.dtype)
    M, D = x.shape
    ld = out.shape[1]
    assert out.shape[0] == M and col0 + D <= ld
    call("xggm_elu_fwd_" + sfx(x.dtype), ptr(x), out.data_ptr() + col0 * out.element_size(), M, D, ld, stream())


def elu_bwd(dy, y, col0, D):
    _c(dy), _c(y, dy.dtype)
    M, ld = y.shape
    assert dy.shape == y.shape and col0 + D <= ld
    dx = torch.empty((M, D), device=y.device, dtype=y.dtype)
    off = col0 * y.element_size()
    call("xggm_elu_bwd_" + sfx(y.dtype), dy.data_ptr() + off, y.data_ptr() + off, ptr(dx), M, D, ld, stream())
    return dx


def dropout(x, p, rng, sid):
    _c(x)
    out = torch.empty_like(x)
    call("xggm_dropout_" + sfx(x.dtype), ptr(x), ptr(out), x.numel(), float(p), ptr(rng), sid, stream())
    return out
