"""shared test helpers: seeded parameters as torch tensors, probes, golden loading."""
import os

import numpy as np
import torch

from xggm_amd import synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_golden(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)


def golden_cfg(g):
    return {str(k): int(v) for k, v in zip(g["cfg_keys"], g["cfg_vals"])}


def seeded_params(shapes, seed, dtype=torch.float32, device="cpu"):
    return {k: torch.from_numpy(synth.seeded_param(k, s, seed)).to(device=device, dtype=dtype)
            for k, s in shapes.items()}


def probe(name, shape, seed, dtype=torch.float32, device="cpu"):
    v = synth._rng(seed, "probe:" + name).standard_normal(tuple(shape), dtype=np.float32)
    return torch.from_numpy(v).to(device=device, dtype=dtype)


def batch_tensors(b, device="cpu", dtype=torch.float32):
    out = {}
    for k, v in b.items():
        t = torch.from_numpy(np.ascontiguousarray(v)).to(device)
        out[k] = t.to(dtype) if t.is_floating_point() else t
    return out


def rel_err(a, b):
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


# ---- element-wise GEMM bound -------------------------------------------------------------------------------------
# rel_err is a norm ratio over the whole tensor: a truncating store, a few dozen wrong elements or a wrong 8 x 8
# corner of a 640 x 768 output all stay under its 1.2e-2 (tests/test_gemm_edges_cpu.py shows it).  gemm_excess
# compares every element with a bound DERIVED from the arithmetic, never fitted to what a kernel returns:
#   accumulation   c * (K + 3) * 2^-24 * S     S = |A| . |B| (+ |bias| + |residual| + |old C|), fp64.  Products of bf16
#                                              (or e4m3) values are exact in fp32 and K - 1 fp32 additions in ANY order
#                                              stay within (K - 1) u S, u = 2^-24; the + 3 covers the epilogue's
#                                              additions; c = 2 is the margin for the MFMA's internal order.
#   bf16 store     2^-8 * |ref|                bf16's unit round-off under round-to-nearest; no margin on this term.
#   extra          caller's term               e.g. 4 * 2^-24 * (1 + |f|) for an activation evaluated in fp32.
# An activation with Lipschitz constant L enters through S (pass L * S).  A non-finite result has excess +inf.
U32 = 2.0 ** -24
U_BF16 = 2.0 ** -8


def gemm_excess(got, ref64, S64, K, out_dtype, extra=0.0, c=2.0):
    """|got - ref| / bound per element (fp64, on ref64's device); the caller asserts max <= 1 (assert_excess)."""
    ref = ref64.double()
    g = got.detach().to(ref.device).double()
    if torch.is_tensor(extra):
        extra = extra.to(ref.device).double()
    bound = c * (K + 3) * U32 * S64.to(ref.device).double() + extra
    if out_dtype == torch.bfloat16:
        bound = bound + U_BF16 * ref.abs()
    elif out_dtype != torch.float32:
        raise TypeError("gemm_excess: fp32 or bf16 outputs, got %s" % out_dtype)
    return bound_excess(g, ref, bound)


def bound_excess(g, ref, bound):
    """|g - ref| / bound per element (fp64 tensors of one shape); a zero bound (ref == 0 and S == 0) admits only the
    exact value, a non-finite result has excess +inf"""
    err = (g - ref).abs()
    inf = torch.full_like(err, float("inf"))
    exc = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err == 0, torch.zeros_like(err), inf))
    return torch.where(torch.isfinite(g), exc, inf)


def excess_argmax(exc):
    """(largest excess, its index as a tuple) of a gemm_excess tensor."""
    flat = int(torch.argmax(exc.reshape(-1)))
    idx = tuple(int(i) for i in np.unravel_index(flat, tuple(exc.shape))) if exc.dim() else ()
    return float(exc.reshape(-1)[flat]), idx


def assert_excess(exc, what):
    """max(exc) <= 1, with the arg-max index (row, column) in the message; returns the maximum."""
    mx, idx = excess_argmax(exc)
    assert mx <= 1.0, "%s: |err| / bound = %.3f at index %s (row %s, column %s); %d of %d elements over the bound" % (
        what, mx, idx, idx[-2] if len(idx) > 1 else 0, idx[-1] if idx else 0, int((exc > 1).sum()), exc.numel())
    return mx


# ---- element-wise attention bound ----------------------------------------------------------------------------------
# The attention core (csrc/attention.hip: fp32 math, "scalar"; csrc/attention_mfma.hip: bf16 operands on the matrix
# cores, "mfma") is compared element by element with an fp64 reference of the SAME stored operands.  As for the GEMMs
# the bound follows from the arithmetic and is never fitted to a kernel's result.  u = 2^-24 (fp32 round-off),
# UB = 2^-8 (bf16 round-off), c = 2 the margin for the MFMA's internal summation order, d = 64 the head width,
# P = softmax(S), D the dropout keep-scales (1 without dropout), rs_i = sum_j P_ij dP_ij.
#   scores         eS_ij = c (64 + 3) u (|q| . |k|)_ij scale + 2 u |S_ij|      64 exact products added in fp32, times
#                  eS_i  = max_j eS_ij                                         scale, plus mask: two roundings of S
#   probabilities  rho_ij = 2 eS_i + (4 + min(m_i - S_ij, 100)) 2^-23 + 64 u   RELATIVE error of P_ij: numerator and
#                  denominator both move with the scores of row i (2 eS_i); the argument S_ij - m_i of __expf is
#                  rounded (relative u of |S_ij - m_i|, which exp turns into an absolute |x| 2^-23 relative error of
#                  the result, the argument reduction included; beyond 100 the result is an exact zero) and its result
#                  is good to a few ulps (4 * 2^-23 with the division); the row sum of <= 64 terms (64 u)
#   forward        bound(O_ic) = sum_j (rho_ij + ub) P_ij D_ij |V_jc| + c (Sk + 35) u sum_j P_ij D_ij |V_jc| + store
#                  ub = UB where P D is rounded to a bf16 operand (mfma), 0 on the scalar kernels; the second term is
#                  the fp32 accumulation over the keys (padded to a multiple of 32: + 35 covers padding and epilogue)
#                  store = UB |O_ic| for bf16 storage, 0 for fp32: round-to-nearest, no margin on this term
#   backward       e_dP_ij = c 67 u (|dO| . |V|^T)_ij D_ij
#                  drs_i   = sum_k (rho_ik P_ik |dP_ik| + P_ik e_dP_ik) + (Sk + 3) u sum_k P_ik |dP_ik|
#                  E_dS_ij = scale (rho_ij P_ij |dP_ij - rs_i| + P_ij (e_dP_ij + drs_i) + 4 u P_ij (|dP_ij| + |rs_i|))
#                            + ub |dS_ij|                                      (4 u: subtraction, two products, scale)
#                  bound(dQ) = E_dS . |K|   + c (Sk + 35) u |dS| . |K|     + store
#                  bound(dK) = E_dS^T . |Q| + c (Sq + 35) u |dS|^T . |Q|   + store
#                  bound(dV) = ((rho + ub) P D)^T . |dO| + c (Sq + 35) u (P D)^T . |dO| + store
#   bias partials  the (sample, head, column) partial is the column sum of the UNROUNDED fp32 gradient tile: the column
#                  sum of the gradient bounds without their store term, plus (S + 3) u sum |g| for the S - 1 additions
# A zero bound admits only the exact value; a non-finite result has excess +inf (bound_excess).
ATTN_D = 64


def _heads_split(x, B, heads):
    return x.reshape(B, -1, heads, ATTN_D).permute(0, 2, 1, 3)


def _heads_merge(x):
    B, h, S, _ = x.shape
    return x.permute(0, 2, 1, 3).reshape(B * S, h * ATTN_D)


class AttnRef:
    """fp64 reference of one attention problem and the magnitude sums of its bound (see the block above).

    q [B*Sq, H], k, v [B*Sk, H], d_out [B*Sq, H] or None: the operands AS STORED (already rounded), any float type;
    mask: additive [B, Sk] or None; keep: the dropout keep-scales [B, heads, Sq, Sk] (0 or 1 / (1 - p)) or None.
    Closed forms, no autograd.  Every product is kept in the kernels' [B*S, H] layout."""

    def __init__(self, q, k, v, mask, d_out, keep, B, heads, scale=0.125, c=2.0):
        u = U32
        Q, K, V = (_heads_split(t.detach().double().cpu(), B, heads) for t in (q, k, v))
        self.B, self.heads, self.Sq, self.Sk, self.c, self.scale = B, heads, Q.shape[2], K.shape[2], c, scale
        Sq, Sk = self.Sq, self.Sk
        S = Q @ K.transpose(-1, -2) * scale
        if mask is not None:
            S = S + mask.detach().double().cpu()[:, None, None, :]
        m = S.max(-1, keepdim=True).values
        P = torch.softmax(S, -1)
        D = torch.ones_like(P) if keep is None else keep.detach().double().cpu().reshape(P.shape)
        PD = P * D
        eS = c * (ATTN_D + 3) * u * (Q.abs() @ K.abs().transpose(-1, -2)) * scale + 2 * u * S.abs()
        rho = 2 * eS.max(-1, keepdim=True).values + (4 + (m - S).clamp(max=100.0)) * 2.0 ** -23 + 64 * u
        self.S, self.P, self.D, self.rho = S, P, D, rho
        # name -> (reference, bound part without ub / accumulation / store, magnitude sum, reduction length)
        self.terms = {"out": (_heads_merge(PD @ V), _heads_merge((rho * PD) @ V.abs()), _heads_merge(PD @ V.abs()), Sk)}
        if d_out is None:
            return
        dO = _heads_split(d_out.detach().double().cpu(), B, heads)
        dP = (dO @ V.transpose(-1, -2)) * D
        e_dP = c * (ATTN_D + 3) * u * (dO.abs() @ V.abs().transpose(-1, -2)) * D
        rs = (P * dP).sum(-1, keepdim=True)
        drs = (rho * P * dP.abs() + P * e_dP).sum(-1, keepdim=True) + (Sk + 3) * u * (P * dP.abs()).sum(-1, keepdim=True)
        dS = P * (dP - rs) * scale
        E0 = scale * (rho * P * (dP - rs).abs() + P * (e_dP + drs) + 4 * u * P * (dP.abs() + rs.abs()))
        self.dP, self.rs, self.dS = dP, rs, dS
        aS, T = dS.abs(), lambda t: t.transpose(-1, -2)
        self.terms["dq"] = (_heads_merge(dS @ K), _heads_merge(E0 @ K.abs()), _heads_merge(aS @ K.abs()), Sk)
        self.terms["dk"] = (_heads_merge(T(dS) @ Q), _heads_merge(T(E0) @ Q.abs()), _heads_merge(T(aS) @ Q.abs()), Sq)
        self.terms["dv"] = (_heads_merge(T(PD) @ dO), _heads_merge(T(rho * PD) @ dO.abs()), _heads_merge(T(PD) @ dO.abs()), Sq)

    def bound(self, name, out_dtype, mfma, store=True):
        """(reference, bound) of out / dq / dk / dv; ``mfma``: P D and dS were rounded to bf16 operands"""
        ref, base, mag, n = self.terms[name]
        bound = base + ((U_BF16 if mfma else 0.0) + self.c * (n + 35) * U32) * mag
        if store and out_dtype == torch.bfloat16:
            bound = bound + U_BF16 * ref.abs()
        elif out_dtype not in (torch.bfloat16, torch.float32):
            raise TypeError("attention bound: fp32 or bf16 outputs, got %s" % out_dtype)
        return ref, bound

    def bias_bound(self, name, mfma):
        """(reference, bound) [B, H] of the per-sample column sums of dq / dk / dv (the fp32 bias-gradient partials)"""
        ref, bound = self.bound(name, torch.float32, mfma, store=False)
        S = ref.shape[0] // self.B
        col = lambda t: t.reshape(self.B, S, -1).sum(1)
        return col(ref), col(bound) + (S + 3) * U32 * col(ref.abs())


def attn_fwd_excess(out, R, out_dtype, mfma):
    """|out - ref| / bound per element of the context [B*Sq, H] against the AttnRef ``R`` (fp64, CPU)"""
    ref, bound = R.bound("out", out_dtype, mfma)
    return bound_excess(out.detach().double().cpu(), ref, bound)


def attn_bwd_excess(dq, dk, dv, R, out_dtype, mfma):
    """{"dq" | "dk" | "dv": |g - ref| / bound per element} against the AttnRef ``R`` (built with d_out)"""
    out = {}
    for name, g in (("dq", dq), ("dk", dk), ("dv", dv)):
        ref, bound = R.bound(name, out_dtype, mfma)
        out[name] = bound_excess(g.detach().double().cpu(), ref, bound)
    return out


# ---- element-wise row-kernel bounds --------------------------------------------------------------------------------
# The row kernels (csrc/rowops.hip: the LayerNorm family, the two embeddings, the column sums) are compared element by
# element with an fp64 reference of the SAME stored operands.  As above, every term follows from the arithmetic and none
# is fitted to a kernel's result.  u = 2^-24, UB = 2^-8, c = 2 the margin for an unknown summation order (lanes, wave
# shuffles, LDS and workspace stages), H the row width, M the number of rows.
#   z              e_z = (n + 3) u S        S = (sum |in slab| + |bias|) keep_pre + |residual|: n - 1 slab additions (n <= 8),
#                  the bias, the keep-scale product and the residual, fp32 each; + UB |z| where z is stored as bf16.
#                  The kernel normalises the ROUNDED z it stores and so does the reference: then e_z = 0 below.
#   mean           e_mean = c (H + 3) u mean|z| + mean(e_z)           H - 1 additions in any order and the division
#   centred        e_t = e_z + e_mean + u |t|,  t = z - mean          the centred values carry the error of the mean
#   variance       e_var = mean(2 |t| e_t + e_t^2) + c (H + 3) u var  the squares of the perturbed t, the H-term sum
#   rstd           v = var + eps, e_v = e_var + 3 u v (addition, division by H, eps as fp32); the computed variance is
#                  a sum of squares, so the computed v is never below eps (1 - 2 u): lo = max(v - e_v, eps (1 - 2 u)) and
#                  rho = max(sqrt(v / lo) - 1, 1 - sqrt(v / (v + e_v))) + 4 * 2^-23      the RELATIVE error of rstd.
#                  The interval form is first order e_v / (2 v) = e_v / (2 (var + eps)) for a well-conditioned row and
#                  stays finite at var = 0.  It is MEANINGFUL (rho below bf16's round-off at H = 2048) only for rows with
#                  var >= ROW_TAU * mean|z|^2; row_cases asserts that of every input row but the one named constant-row
#                  case, which is checked for finite results and for the exact out = beta instead.
#                  4 * 2^-23: rsqrtf 2 ulp, the addition of eps and the division by H one rounding each.  The 2 ulp is a
#                  DOCUMENTED figure, not a derivation: the ROCm device library's rsqrt follows the OpenCL full-profile
#                  accuracy table (2 ulp; the native v_rsq_f32 is 1 ulp).  The HIP math API's own accuracy table was
#                  not at hand when this was written, so the count rests on that specification.
#   out            e_y = |g| (|t| rstd rho + rstd (1 + rho) e_t) + 4 u (|y| + |beta|),  y = t rstd g + beta;
#                  bound = e_y keep_post |out_scale| + 2 u |y keep_post out_scale| (+ u (|old| + |ref|) when
#                  accumulating) + UB |ref| for a bf16 store (round-to-nearest, no margin on this term)
#   ln_sum_fwd     the sum over the n <= 4 terms of their out bounds without store, n u sum|term| for the additions,
#                  then ONE store
#   ln_bwd         from the stored dy, z, stats (mean, rstd as the forward left them: operands, no error), gamma:
#                  dyn = dy keep_post out_scale (2 u), xh = (z - mean) rstd (2 u), tt = dyn g (3 u in all)
#                  s1 = mean(tt), s2 = mean(tt xh):  e_s = c (H + 3) u mean|term| + mean(term roundings)
#                  dz = rstd (tt - s1 - xh s2):  e_dz = rstd (3 u |tt| + e_s1 + |xh| e_s2 + 2 u |xh s2| + 4 u (|tt| + |s1| + |xh s2|))
#                  d_res = dz (+ old: one more rounding, u (|old| + |ref|)) + store
#                  d_in = dz keep_pre gelu'(aux):  e_dz keep |gelu'| + |dz| keep 4 u (1 + |gelu'|) (the fp32 evaluation of
#                  gelu_grad_f, as gemm_excess's `extra` takes it) + 2 u |d_in| + store
#   column sums    dgamma = sum_m dyn xh (5 u per term), dbeta = sum_m dyn (2 u), dbias = sum_m d_in (UNROUNDED: the d_in
#                  bound without store), the ten vectors of visn_embed_bwd, colsum, the embedding scatter:
#                  sum_m (per-row bound) + c (M + 3) u sum_m |term| + u (|old| + |ref|) for the `+=` into the gradient
# A zero bound admits only the exact value; a non-finite result has excess +inf (bound_excess).
ROW_TAU = 2.0 ** -8
ROW_RSQRT_ULPS = 4


def store_term(ref, dtype):
    if dtype == torch.bfloat16:
        return U_BF16 * ref.abs()
    if dtype != torch.float32:
        raise TypeError("row bound: fp32 or bf16 storage, got %s" % dtype)
    return torch.zeros_like(ref)


def row_z_bound(S, n_slabs, dtype, ref):
    """bound of the stored pre-normalisation sum against the unrounded fp64 sum ``ref``; S as in the block above"""
    return (max(n_slabs, 1) + 3) * U32 * S + store_term(ref, dtype)


def ln_terms(z, gamma, beta, eps, e_z=None, c=2.0):
    """fp64 LayerNorm of the rows z [M, H] (as the kernel normalises them) and the error terms of the block above:
    dict(mean, rstd, t, y, e_mean, rho, e_t, e_y, var)"""
    H = z.shape[-1]
    ez = torch.zeros_like(z) if e_z is None else e_z
    mean = z.mean(-1, keepdim=True)
    t = z - mean
    var = (t * t).mean(-1, keepdim=True)
    e_mean = c * (H + 3) * U32 * z.abs().mean(-1, keepdim=True) + ez.mean(-1, keepdim=True)
    e_t = ez + e_mean + U32 * t.abs()
    e_var = (2 * t.abs() * e_t + e_t * e_t).mean(-1, keepdim=True) + c * (H + 3) * U32 * var
    v = var + eps
    e_v = e_var + 3 * U32 * v
    lo = torch.maximum(v - e_v, torch.full_like(v, eps * (1 - 2 * U32)))
    rho = torch.maximum(torch.sqrt(v / lo) - 1, 1 - torch.sqrt(v / (v + e_v))) + ROW_RSQRT_ULPS * 2.0 ** -23
    rstd = v.rsqrt()
    y = t * rstd * gamma + beta
    e_y = gamma.abs() * (t.abs() * rstd * rho + rstd * (1 + rho) * e_t) + 4 * U32 * (y.abs() + beta.abs())
    return dict(mean=mean, rstd=rstd, t=t, y=y, var=var, e_mean=e_mean, rho=rho, e_t=e_t, e_y=e_y)


def ln_out_bound(L, keep_post, out_scale, old, dtype, store=True):
    """(reference, bound) of out = [old +] out_scale keep_post y from ln_terms' dict ``L``"""
    f = keep_post * abs(out_scale)
    ref = L["y"] * keep_post * out_scale
    bound = L["e_y"] * f + 2 * U32 * ref.abs()
    if old is not None:
        ref = ref + old
        bound = bound + U32 * (old.abs() + ref.abs())
    return ref, bound + (store_term(ref, dtype) if store else 0.0)


def ln_bwd_terms(dy, z, mean, rstd, gamma, keep_post, out_scale, keep_pre, gp, c=2.0):
    """fp64 LayerNorm backward of the stored operands and the error terms of the block above.  ``gp`` = gelu'(aux) or
    None.  dict(dz, e_dz, din, e_din, and the per-row column-sum terms tg, e_tg (dgamma), tb, e_tb (dbeta))"""
    u, H = U32, z.shape[-1]
    m = lambda x: x.mean(-1, keepdim=True)
    dyn = dy * keep_post * out_scale
    xh = (z - mean) * rstd
    tt = dyn * gamma
    s1, s2 = m(tt), m(tt * xh)
    e_s1 = c * (H + 3) * u * m(tt.abs()) + 3 * u * m(tt.abs())
    e_s2 = c * (H + 3) * u * m((tt * xh).abs()) + 6 * u * m((tt * xh).abs())
    dz = rstd * (tt - s1 - xh * s2)
    e_dz = rstd * (3 * u * tt.abs() + e_s1 + xh.abs() * e_s2 + 2 * u * (xh * s2).abs()
                   + 4 * u * (tt.abs() + s1.abs() + (xh * s2).abs()))
    din, e_din = dz * keep_pre, e_dz * keep_pre
    if gp is not None:
        e_din = e_din * gp.abs() + din.abs() * 4 * u * (1 + gp.abs())
        din = din * gp
    e_din = e_din + 2 * u * din.abs()
    return dict(dz=dz, e_dz=e_dz, din=din, e_din=e_din, tg=dyn * xh, e_tg=5 * u * (dyn * xh).abs(), tb=dyn,
                e_tb=2 * u * dyn.abs(), xh=xh, dyn=dyn)


def colsum_bound(term, e_term, old, c=2.0):
    """(reference, bound) of old + sum_m term[m, :] for fp32 additions in any order; e_term: the per-row bounds"""
    M = term.shape[0]
    ref = term.sum(0)
    bound = e_term.sum(0) + c * (M + 3) * U32 * term.abs().sum(0)
    if old is not None:
        ref = ref + old
        bound = bound + U32 * (old.abs() + ref.abs())
    return ref, bound
