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
