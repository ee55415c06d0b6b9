"""Attention-core cases with 65 .. 128 rows on a side (csrc/attention_long.hip), shared by test_attention_long_cpu.py and
test_attention_long_gpu.py.

``LongCase`` is attention_cases.Case -- NaN moats, sentinel buffers, the fp64 reference, the emulated ``scalar`` / ``mfma``
arithmetic and its planted defects, none of which assumes 64 rows -- with one change to the bound.  The reference's
relative probability error ``rho`` (helpers.AttnRef) ends in ``64 u``: the round-off of the softmax's row sum, a sum of at
most 64 non-negative terms in the 64-row kernels (each addition adds at most u relative to the running sum).  A row of
attention_long.hip has up to 128 terms, so the term is ``max(Sk, 64) u``: derived from the row length, not fitted, and equal
to the old term wherever Sk <= 64.  Nothing else of the bound knows the old limit; c = 2 stays.
"""
import torch

from attention_cases import SCALE, Case
from helpers import ATTN_D, U32, AttnRef, _heads_merge, _heads_split

# both sides of 64, of the 16- and 32-row paddings and of the 32-row query blocks of the fp32 kernels; one long side only
LONG_SHAPES = [(65, 65), (64, 65), (65, 64), (65, 1), (1, 65), (100, 20), (20, 100), (72, 36), (36, 72), (97, 113), (127, 128),
               (128, 127), (128, 128)]
# both branches of the four-key Philox call (Sk % 4 == 0: one call per four keys)
LONG_DROPOUT_SHAPES = [(65, 67), (72, 65), (100, 36), (36, 100), (97, 113), (128, 128)]
LONG_WIDE_SHAPES = [(72, 36), (128, 128)]


class LongAttnRef(AttnRef):
    """helpers.AttnRef with the row-sum term of ``rho`` taken from the row length: max(Sk, 64) u instead of 64 u.  The
    constructor repeats AttnRef's closed forms (rho enters every bound part, so it cannot be patched afterwards)."""

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
        rho = 2 * eS.max(-1, keepdim=True).values + (4 + (m - S).clamp(max=100.0)) * 2.0 ** -23 + max(Sk, 64) * u
        self.S, self.P, self.D, self.rho = S, P, D, rho
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


class LongCase(Case):
    """attention_cases.Case whose reference carries the row-sum term of its own row length"""

    def reference(self):
        if self._ref is None:
            assert (self.p > 0) == (self.keep is not None), "%s: dropout needs set_keep first" % self.name
            self._ref = LongAttnRef(self.q, self.k, self.v, self.mask, self.do, self.keep, self.B, self.heads, SCALE)
        return self._ref
