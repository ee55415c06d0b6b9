"""Attention-core cases shared by test_attention_edges_cpu.py and test_attention_edges_gpu.py.

A ``Case`` is one problem of csrc/attention.hip / attention_mfma.hip -- softmax(Q K^T / 8 + mask) -> dropout -> P V and
its backward for B samples of ``heads`` heads, Sq queries, Sk keys -- with
  * q, k, v and dO inside NaN-filled buffers (LEAD rows before, MOAT_ROWS rows after, NaN in every stride gap): a kernel
    that lets a row or column past the problem reach a product turns an output into NaN and stays inside the allocation,
  * out, dq, dk, dv, the e4m3 copy and the fp32 bias-partial workspace inside sentinel-filled buffers: after a launch every
    cell the problem does not own must still hold the sentinel's bits (stride gaps, rows before and past the end, the
    columns of a partial row that belong to a foreign head, the partial rows of a kind that was not asked for),
  * the fp64 reference and the magnitude sums of its bound (helpers.AttnRef), computed once from the stored operands and,
    with dropout, from the keep-scales handed to ``set_keep``,
  * an emulation of either arithmetic in fp32 torch on the CPU, with the defects test_attention_edges_cpu.py plants.
Layouts (row strides): ``fused`` = q a slice of one [B*Sq, 3H] buffer, k and v slices of another, dq / dk / dv slices of
fused gradient buffers, out and dO contiguous; ``wide`` = every matrix with row stride H + 8; ``odd4`` = bf16 with row
stride H + 4 and a 16-byte aligned base, which attention.hip's mfma_ok sends to the scalar kernels; ``odd12`` = the
same with H + 12, the ``wide`` layout of that path (canaries at least 8 elements from every row end).
Nothing here imports the library at module level: the CPU test drives the same cases with the emulated kernels.
"""
import ctypes
import math

import torch

from gemm_edge_cases import LEAD, SENTINEL, Guarded, _ints
from helpers import ATTN_D, AttnRef, _heads_merge, _heads_split, assert_excess, bound_excess

BF16, F32 = torch.bfloat16, torch.float32
# every border of the paddings: Sq to 16 (all products) and to 32 (reduction length of dK / dV), Sk to 16 and to 32
SHAPES = [(1, 1), (1, 7), (15, 17), (16, 16), (17, 15), (20, 36), (31, 33), (33, 31), (36, 20), (47, 49), (49, 47),
          (63, 64), (64, 63), (64, 64),
          # Sq in 33 .. 48 with Sk <= 16: the matrix-core backward's dynamic LDS alone stays under 48 KiB, with its static
          # csum it passes it (the large-LDS opt-in has to count both)
          (33, 3), (36, 12), (48, 16)]
# both branches of Drop::scale4 (Sk % 4 == 0: one Philox call per four keys) at several tile borders
DROPOUT_SHAPES = [(1, 7), (15, 17), (17, 15), (20, 36), (33, 31), (36, 12), (36, 20), (49, 47), (64, 63), (64, 64)]
WIDE_SHAPES = [(17, 15), (36, 20), (64, 64)]
SCALE = 0.125
C8_FILL = 0x55


def ids(shape):
    return "%dx%d" % shape


class Slab(Guarded):
    """a Guarded buffer in which one or more regions are owned by the problem; everything else is canary"""

    def __init__(self, rows, cols, dtype, device, fill, ld):
        super().__init__(rows, cols, dtype, device, fill, ld)
        self.owned = torch.zeros(self.buf.shape, dtype=torch.bool, device=device)

    def window(self, col0, cols, rows=None):
        """own columns [col0, col0 + cols) of the given rows (default: all) and return that view"""
        rows = slice(0, self.rows) if rows is None else rows
        self.owned[LEAD:LEAD + self.rows][rows, col0:col0 + cols] = True
        return self.buf[LEAD:LEAD + self.rows][rows, col0:col0 + cols]

    def untouched_outside(self):
        cur, pri = _ints(self.buf), _ints(self.pristine)
        return torch.equal(torch.where(self.owned, pri, cur), pri)


def mask_lens(B, Sk, masked):
    """valid keys per sample: True -> all / half / exactly one, in turn; a list is taken as it is (0 = a fully masked
    sample: every score shifted by -10000, still a proper softmax)"""
    if masked is True:
        return [(Sk, max(1, Sk // 2), 1)[b % 3] for b in range(B)]
    assert len(masked) == B
    return list(masked)


class Case:
    """one attention problem with guarded operands and outputs; see the module docstring"""

    def __init__(self, B, heads, Sq, Sk, dt, device, masked=True, p=0.0, layout="fused", seed=0, sharp=1.0, db="qkv",
                 ws_heads=None, db_bs=None, out8=False):
        """``db``: which bias partials are asked for ("qkv", "q", "kv", ""); ``ws_heads`` (>= heads): heads of the
        partial workspace's rows, the ones past ``heads`` belong to nobody; ``sharp``: factor on q"""
        assert layout in ("fused", "wide", "odd4", "odd12") and (layout[:3] != "odd" or dt == BF16) and db in ("qkv", "q", "kv", "")
        self.B, self.heads, self.Sq, self.Sk, self.dt, self.device, self.p, self.layout = B, heads, Sq, Sk, dt, device, p, layout
        H = self.H = heads * ATTN_D
        self.db = db
        self.name = "%dx%d B %d heads %d %s %s%s%s%s" % (Sq, Sk, B, heads, "bf16" if dt == BF16 else "f32", layout,
                                                      " masked" if masked else "", " p %.1f" % p if p else "",
                                                      " q x %g" % sharp if sharp != 1.0 else "")
        gen = torch.Generator().manual_seed(7919 * seed + 131 * Sq + 17 * Sk + 5 * B + heads)
        rn = lambda rows: torch.randn(rows, H, generator=gen)
        nan, f = float("nan"), "fused"
        ld = {"fused": H, "wide": H + 8, "odd4": H + 4, "odd12": H + 12}[layout]
        ld3 = 3 * H if layout == f else ld
        # operands
        self.q_slab = Slab(B * Sq, ld3 if layout == f else H, dt, device, nan, ld3)
        self.k_slab = Slab(B * Sk, ld3 if layout == f else H, dt, device, nan, ld3)
        self.v_slab = self.k_slab if layout == f else Slab(B * Sk, H, dt, device, nan, ld3)
        self.do_slab = Slab(B * Sq, H, dt, device, nan, ld)
        self.q = self.q_slab.window(0, H)
        self.k = self.k_slab.window(H if layout == f else 0, H)
        self.v = self.v_slab.window(2 * H if layout == f else 0, H)
        self.do = self.do_slab.window(0, H)
        self.q.copy_((rn(B * Sq) * sharp).to(dt))
        self.k.copy_(rn(B * Sk).to(dt))
        self.v.copy_(rn(B * Sk).to(dt))
        self.do.copy_(rn(B * Sq).to(dt))
        self.mask = None
        if masked:
            lens = torch.tensor(mask_lens(B, Sk, masked))
            self.mask = ((torch.arange(Sk)[None, :] >= lens[:, None]).float() * -10000.0).to(device)
        # outputs
        self.out_slab = Slab(B * Sq, H, dt, device, SENTINEL, ld)
        self.dq_slab = Slab(B * Sq, ld3 if layout == f else H, dt, device, SENTINEL, ld3)
        self.dk_slab = Slab(B * Sk, ld3 if layout == f else H, dt, device, SENTINEL, ld3)
        self.dv_slab = self.dk_slab if layout == f else Slab(B * Sk, H, dt, device, SENTINEL, ld3)
        self.out = self.out_slab.window(0, H)
        self.dq = self.dq_slab.window(0, H)
        self.dk = self.dk_slab.window(H if layout == f else 0, H)
        self.dv = self.dv_slab.window(2 * H if layout == f else 0, H)
        self.outputs = {"out": self.out_slab, "dq": self.dq_slab, "dk": self.dk_slab, "dv": self.dv_slab}
        # bias partials: rows (b, kind) of Hw columns; the problem owns [0, H) of the rows of the kinds asked for
        self.ws_heads = heads + 1 if ws_heads is None else ws_heads
        Hw = self.Hw = self.ws_heads * ATTN_D
        assert self.ws_heads >= heads
        self.db_bs = 3 * Hw if db_bs is None else db_bs
        assert self.db_bs == 3 * Hw or (B == 1 and self.db_bs == 0)
        self.ws = self.outputs["bias partials"] = Slab(B * 3, Hw, F32, device, SENTINEL, Hw)
        self.part = {}
        for kind, key in enumerate("qkv"):
            if key in db:
                self.part["d" + key] = self.ws.window(0, H, rows=slice(kind, B * 3, 3))
        self.out8 = None
        if out8:
            assert dt == BF16
            self.out8_slab = self.outputs["e4m3 copy"] = Slab(B * Sq, H, torch.uint8, device, C8_FILL, ld)
            self.out8 = self.out8_slab.window(0, H)
            self.q8 = torch.tensor([256.0], dtype=F32, device=device)  # calibrated: maxima beyond 0.5 * 448 / 256 are recorded
            self.amax = torch.zeros(1, dtype=F32, device=device)
        for g in set(self.outputs.values()):
            g.seal()
        self.keep = None
        self._ref = None

    # ---- launching -----------------------------------------------------------------------------------------------
    def reset(self):
        for g in set(self.outputs.values()):
            g.reset()
        if self.out8 is not None:
            self.amax.zero_()

    def problem(self, ops, sid=0):
        """the xggm_attn_problem of this case, forward and backward fields, with the raw strides of its windows"""
        from xggm_amd._lib import ptr
        pp = lambda key: ptr(self.ws.buf[LEAD + "qkv".index(key), 0:]) if key in self.db else None
        pr = ops.AttnProblem(ptr(self.q), ptr(self.k), ptr(self.v), ptr(self.mask), ptr(self.out), self.B, self.heads,
                             self.Sq, self.Sk, self.q.stride(0), self.k.stride(0), self.v.stride(0), self.out.stride(0),
                             SCALE, float(self.p), sid, ptr(self.do), ptr(self.dq), ptr(self.dk), ptr(self.dv),
                             self.dq.stride(0), self.dk.stride(0), self.dv.stride(0), pp("q"), pp("k"), pp("v"), self.db_bs)
        assert self.do.stride(0) == self.out.stride(0)
        if self.out8 is not None:
            assert self.out8.stride(0) == self.out.stride(0)
            pr.out8, pr.qscale, pr.amax, pr.amax_slots = ptr(self.out8), ptr(self.q8), ptr(self.amax), 1
        return pr

    def set_keep(self, keep):
        """the dropout keep-scales of this problem, element ((b * heads + h) * Sq + i) * Sk + j: 0 or 1 / (1 - p);
        their keep rate must agree with 1 - p within five binomial standard deviations"""
        n = self.B * self.heads * self.Sq * self.Sk
        keep = keep.detach().float().cpu().reshape(self.B, self.heads, self.Sq, self.Sk)
        assert bool(((keep == 0) | (keep == keep_scale(self.p))).all()), "%s: keep-scales other than 0 and 1 / (1 - p)" % self.name
        rate = float((keep > 0).double().mean())
        assert abs(rate - (1 - self.p)) <= 5 * math.sqrt(self.p * (1 - self.p) / n), (self.name, rate)
        self.keep, self._ref = keep, None
        return self

    def host_keep(self, seed=0):
        """a host-made keep mask (the CPU test's stand-in for ops.dropout_mask)"""
        gen = torch.Generator().manual_seed(4409 * seed + 31 * self.Sq + self.Sk)
        n = self.B * self.heads * self.Sq * self.Sk
        return self.set_keep((torch.rand(n, generator=gen) >= self.p).float() * keep_scale(self.p))

    def reference(self):
        """helpers.AttnRef of the stored operands (fp64, CPU), computed once per keep mask"""
        if self._ref is None:
            assert (self.p > 0) == (self.keep is not None), "%s: dropout needs set_keep first" % self.name
            self._ref = AttnRef(self.q, self.k, self.v, self.mask, self.do, self.keep, self.B, self.heads, SCALE)
        return self._ref

    # ---- the emulated kernels of the CPU test ---------------------------------------------------------------------
    def emulate(self, path, defect=None, at=None):
        """every output as the ``mfma`` or the ``scalar`` kernels compute it, in fp32 torch:
        mfma: scores, softmax, dP and the row sum in fp32, P D and dS rounded to bf16 before the second products, fp32
        accumulation, bf16 store;  scalar: fp32 throughout, then the store of the storage type.
        The bias partials are the column sums of the unrounded fp32 tiles.  ``defect`` plants one of the corruptions of
        test_attention_edges_cpu.py at (sample, head, query row) ``at``.  Returns {name: tensor}."""
        assert path in ("mfma", "scalar")
        B, heads, Sq, Sk = self.B, self.heads, self.Sq, self.Sk
        b0, h0, i0 = at if at is not None else (0, 0, 0)
        rb = (lambda t: t.to(BF16).float()) if path == "mfma" else (lambda t: t)
        Q, K, V, dO = (_heads_split(t.float().cpu(), B, heads) for t in (self.q, self.k, self.v, self.do))
        T = lambda t: t.transpose(-1, -2)
        S = (Q @ T(K)) * SCALE
        if self.mask is not None:
            mk = self.mask.cpu()
            if defect == "wrong_mask_row":
                mk = mk[torch.arange(B) ^ 1]
            S = S + mk[:, None, None, :]
        m = S.max(-1, keepdim=True).values
        E = torch.exp(S - m)
        P = E / E.sum(-1, keepdim=True)
        if defect == "dropped_key":  # the row is renormalised without its most probable key (never the last key)
            row = P[b0, h0, i0].clone()
            row[int(torch.argmax(row[:Sk - 1]))] = 0
            P[b0, h0, i0] = row / row.sum()
        if defect == "padding_key":  # the zero key row j = Sk (score 0, V row 0) takes part in the softmax of (b0, h0)
            s = S[b0, h0]
            m2 = torch.clamp(s.max(-1, keepdim=True).values, min=0.0)
            e = torch.exp(s - m2)
            P[b0, h0] = e / (e.sum(-1, keepdim=True) + torch.exp(-m2))
        D = torch.ones_like(P)
        if self.keep is not None:
            D = self.keep.clone()
            if defect == "shifted_keep":
                D = shifted(self.keep)
        PD = rb(P * D)
        O = PD @ V
        dP = (dO @ T(V)) * D
        rs = (P * dP).sum(-1, keepdim=True)
        dS = rb(P * (dP - rs) * SCALE)
        dQ, dK, dV = dS @ K, T(dS) @ Q, T(PD) @ dO
        if defect == "padding_query":  # the padding row i = Sq enters dK / dV as a copy of the last query row
            dK[b0, h0] += torch.outer(dS[b0, h0, Sq - 1], Q[b0, h0, Sq - 1])
            dV[b0, h0] += torch.outer(PD[b0, h0, Sq - 1], dO[b0, h0, Sq - 1])
        res = {"out": _heads_merge(O).to(self.dt), "dq": _heads_merge(dQ).to(self.dt), "dk": _heads_merge(dK).to(self.dt),
               "dv": _heads_merge(dV).to(self.dt)}
        part = {"dq": dQ.sum(2), "dk": dK.sum(2), "dv": dV.sum(2)}  # [B, heads, 64]
        if defect == "short_partial":  # the last 16-row tile of the (sample, head) is missing from the column sums
            for key, g in (("dq", dQ), ("dk", dK), ("dv", dV)):
                S_ = g.shape[2]
                part[key][b0, h0] = g[b0, h0, :16 * ((S_ - 1) // 16)].sum(0)
        if defect == "copied_row":  # the last query row of the (sample, head) holds the row before it
            cols = slice(h0 * ATTN_D, (h0 + 1) * ATTN_D)
            for key in ("out", "dq"):
                res[key][b0 * Sq + Sq - 1, cols] = res[key][b0 * Sq + Sq - 2, cols]
        for key in part:
            res["b" + key] = part[key].reshape(B, self.H)
        return res

    def store(self, res):
        """write an emulated launch through the windows, as the kernels would"""
        for key in ("out", "dq", "dk", "dv"):
            getattr(self, key).copy_(res[key])
        for key, win in self.part.items():
            win.copy_(res["b" + key])
        if self.out8 is not None:
            self.out8.copy_(e4m3_bits(self.out, float(self.q8)))
            self.amax.fill_(float(self.out.float().abs().max()))

    # ---- checks --------------------------------------------------------------------------------------------------
    def check(self, tag, path, fwd=True, bwd=True, canaries=True):
        """canaries of every output buffer, then every element of out (``fwd``) and of dq / dk / dv and the bias
        partials asked for (``bwd``) against the derived bound of ``path`` ("mfma" or "scalar"); the e4m3 copy bit for
        bit from the stored bf16 context.  Returns {what: largest |err| / bound}; the message of a failure carries the
        arg-max index."""
        assert path in ("mfma", "scalar")
        what = "%s [%s]" % (self.name, tag)
        if canaries:
            for name, g in self.outputs.items():
                assert g.untouched_outside(), "%s: cells outside the region of %s were written" % (what, name)
        R, mfma, res = self.reference(), path == "mfma", {}
        for name in (("out",) if fwd else ()) + (("dq", "dk", "dv") if bwd else ()):
            ref, bound = R.bound(name, self.dt, mfma)
            res[name] = assert_excess(bound_excess(getattr(self, name).double().cpu(), ref, bound), "%s %s" % (what, name))
        for name, win in self.part.items() if bwd else ():
            ref, bound = R.bias_bound(name, mfma)
            res["b" + name] = assert_excess(bound_excess(win.double().cpu(), ref, bound), "%s bias partial of %s" % (what, name))
        if fwd and self.out8 is not None:
            assert torch.equal(self.out8.cpu(), e4m3_bits(self.out, float(self.q8)).cpu()), \
                "%s: the e4m3 copy differs from the quantised bf16 context" % what
            assert float(self.amax) == float(self.out.float().abs().max()), "%s: amax %r" % (what, float(self.amax))
        return res

    def excess(self, name, got, path):
        """|got - ref| / bound of a candidate for out / dq / dk / dv, or (bdq / bdk / bdv) a bias partial [B, H]"""
        R, mfma = self.reference(), path == "mfma"
        ref, bound = R.bias_bound(name[1:], mfma) if name[0] == "b" else R.bound(name, self.dt, mfma)
        return bound_excess(got.double().cpu(), ref, bound)

    def snapshot(self):
        return {name: g.buf.clone() for name, g in self.outputs.items()}


def keep_scale(p):
    """1 / (1 - p) as the kernels compute it: fp32 arithmetic on the fp32 value of p"""
    one = torch.tensor(1.0, dtype=F32)
    return one / (one - torch.tensor(p, dtype=F32))


def shifted(keep):
    """the keep mask one element late (element n takes the decision of element n - 1)"""
    return torch.roll(keep.reshape(-1), 1).reshape(keep.shape)


def e4m3_bits(x, q):
    """torch's float8_e4m3fn cast of clamp(x * q, +-448), as uint8 bits"""
    return (x.float() * q).clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8)


def problem_array(ops, cases, sids):
    """(ctypes array of xggm_attn_problem, pointer for the grouped entry points)"""
    arr = (ops.AttnProblem * len(cases))(*[c.problem(ops, sid) for c, sid in zip(cases, sids)])
    return arr, ctypes.cast(arr, ctypes.c_void_p)
