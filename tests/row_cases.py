"""Row-kernel cases shared by test_row_edges_cpu.py and test_row_edges_gpu.py (csrc/rowops.hip).

A ``RowCase(kind, M, H, dt, device, ...)`` is one problem of kind ln_fwd, ln_sum, ln_bwd, embed, visn or colsum with
  * every operand a window into a NaN-filled buffer (gemm_edge_cases.Guarded: LEAD rows before, MOAT_ROWS rows after; the
    rows of a row-shaped operand are contiguous as the kernels require, so the moat is rows M.. and rows < 0; a vector
    operand gamma / beta / bias is a one-row window, so column H.. is moat): a read past row M or past column H of a
    vector reaches an output as NaN.  The clamped reads at H - 4 stay inside the row and trip nothing,
  * every output (out, z_out, stats, d_in, d_res, the fp32 gradient vectors and tables, the partial workspace) a window
    into a sentinel-filled buffer: after a launch every cell outside the window must hold the sentinel's bits.  The
    workspace window has exactly the size xggm_*_workspace_bytes reports; everything behind it is canary.  A gradient
    vector passed as null, and an e4m3 copy nobody asked for, are whole decoy buffers that must stay sentinel,
  * fp64 references in closed form (no autograd) from the operands AS STORED, and the bounds of helpers.py: the kernel
    normalises the rounded z it stores, so the reference normalises the stored z, and z itself is checked against the
    unrounded fp64 sum with a store term; the backward takes the stored (mean, rstd) as operands,
  * an emulation in fp32 torch (``emulate``) with the summation order as a parameter -- "seq", "pair" or "kernel" (lane
    partial sums over the 16-byte vectors, a butterfly over the 64 lanes; for column sums rows per wave, waves per
    workgroup, then the two-stage workspace reduction) -- and the planted DEFECTS of test_row_edges_cpu.py.
Nothing here imports the library at module level; ``launch`` takes the package's ``ops``.
"""
import ctypes
import numpy as np
import torch

from gemm_edge_cases import LEAD, MOAT_ROWS, SENTINEL, Guarded, _ints, gelu_grad64  # noqa: F401 (MOAT_ROWS: Guarded's)
from helpers import (ROW_TAU, U32, assert_excess, bound_excess, colsum_bound, ln_bwd_terms, ln_out_bound, ln_terms,
                     row_z_bound, store_term)

BF16, F32 = torch.bfloat16, torch.float32
NAN = float("nan")
LN_H = [4, 8, 252, 256, 260, 508, 512, 516, 768, 772, 1020, 1024, 1028, 1280, 1284, 1536, 1540, 1792, 2044, 2048]
LN_M = [1, 7, 8, 9, 17]
VISN_H = [4, 252, 256, 260, 512, 516, 768, 772, 1020, 1024]
VISN_M = [1, 7, 9]
EMBED_H = [4, 260, 768, 1028]
EMBED_T = [1, 20]
COLSUM_N = [1, 63, 64, 65, 200]
COLSUM_M = [1, 3, 63, 64, 65, 130]
SID_PRE, SID_POST = 5, 6
ORDERS = ("seq", "pair", "kernel")
EPS = 1e-12
GRAD_NAMES = ("dgamma", "dbeta", "dbias")
VISN_GRADS = ("dbf", "dg1", "db1", "dbb", "dg2", "db2")  # the order of the partial rows; dWb's four columns follow


# the launch variants of the issue's lists (options of RowCase)
FWD_VARIANTS = {
    "plain": {},
    "bias_res": dict(bias=True, res=True),
    "zout": dict(bias=True, res=True, zout=True),
    "dropout": dict(bias=True, res=True, zout=True, p_pre=0.1, p_post=0.5),
    "acc_scale": dict(zout=True, acc=True, out_scale=0.37),
    "slabs1": dict(slabs=1, bias=True, res=True),
    "slabs2": dict(slabs=2, bias=True, res=True),
    "slabs4": dict(slabs=4, bias=True, res=True),
    "slabs5": dict(slabs=5, bias=True, res=True),  # the kernel adds the slabs past the fourth in a loop of its own
    "slabs8": dict(slabs=8, bias=True, res=True, p_pre=0.1),
}
SUM_VARIANTS = [dict(n=n, p_post=p) for n in (1, 2, 3, 4) for p in (0.0, 0.5)]
BWD_VARIANTS = {
    "plain": {},
    "dres": dict(want_dres=True),
    "acc_dres": dict(acc_dres=True),
    "gelu": dict(gelu=True, want_dres=True),
    "dropout": dict(p_pre=0.1, p_post=0.5, want_dres=True, out_scale=0.37),
    "null_dgamma": dict(null=("dgamma",)),
    "null_dbeta": dict(null=("dbeta",)),
    "null_dbias": dict(null=("dbias",), gelu=True),
    "prefill": dict(prefill=True, acc_dres=True, gelu=True),
}


def sfx(dt):
    return "bf16" if dt == BF16 else "f32"


def padded_width(H):
    return 256 * ((H + 255) // 256)


def ln_bwd_blocks(M):
    return min((M + 7) // 8, 256)


# ---- fp32 sums in a chosen order -----------------------------------------------------------------------------------
def rowsum32(x, order):
    """sum over the last axis of fp32 x [M, W] -> [M, 1], every addition rounded to fp32, in the given order"""
    M, W = x.shape
    if order == "seq":  # numpy's accumulate is strictly sequential in the array's own type
        return torch.from_numpy(np.add.accumulate(x.contiguous().numpy(), axis=1)[:, -1:].copy())
    if order == "pair":
        n = 1 << max(0, (W - 1).bit_length())
        p = torch.zeros((M, n), dtype=F32, device=x.device)
        p[:, :W] = x
        while p.shape[1] > 1:
            p = p[:, 0::2] + p[:, 1::2]
        return p
    # kernel: lane l owns columns (v * 64 + l) * 4 + i, sums them in (v, i) order, then the 64 lanes are added pairwise
    nv = (W + 255) // 256
    p = torch.zeros((M, nv * 256), dtype=F32, device=x.device)
    p[:, :W] = x
    p = p.view(M, nv, 64, 4)
    acc = torch.zeros((M, 64), dtype=F32, device=x.device)
    for v in range(nv):
        for i in range(4):
            acc = acc + p[:, v, :, i]
    lanes = torch.arange(64, device=x.device)
    for off in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, lanes ^ off]
    return acc[:, :1]


def colsum32(x, order, W=8, cap=256, drop_last_block=False):
    """sum over the rows of fp32 x [M, N] -> [N] in the given order; "kernel": row r belongs to wave r % W of workgroup
    (r // W) % nblk, a wave adds its rows in order, a workgroup its waves in order, the blocks are added in four strided
    slices and the slices pairwise.  ``drop_last_block``: the planted defect that misses the last partial row"""
    M, N = x.shape
    nblk = min((M + W - 1) // W, cap)
    if order != "kernel" and not drop_last_block:
        return rowsum32(x.t().contiguous(), order)[:, 0]
    part = torch.zeros((nblk, W, N), dtype=F32, device=x.device)
    for r in range(M):
        b, w = (r // W) % nblk, r % W
        part[b, w] = part[b, w] + x[r]
    blk = torch.zeros((nblk, N), dtype=F32, device=x.device)
    for w in range(W):
        blk = blk + part[:, w]
    if drop_last_block:
        blk = blk[:-1]
    sl = torch.zeros((4, N), dtype=F32, device=x.device)
    for b in range(blk.shape[0]):
        sl[b % 4] = sl[b % 4] + blk[b]
    return (sl[0] + sl[1]) + (sl[2] + sl[3])


def ln32(z, g, b, eps, order, defect=None):
    """(mean, rstd, y) of the fp32 rows z as the kernels compute them"""
    M, H = z.shape
    rs = lambda x: rowsum32(x, order)
    mean = rs(z) / float(padded_width(H) if defect == "padded_mean" else H)
    t = z - mean
    sq = t * t
    if defect == "double_var":
        sq = torch.cat([sq, sq[:, H - 4:]], 1)
    rstd = torch.rsqrt(rs(sq) / float(H) + torch.tensor(eps, dtype=F32))
    if defect == "stale_stats" and M > 1:
        mean, rstd = mean.clone(), rstd.clone()
        mean[-1], rstd[-1] = mean[-2], rstd[-2]
    return mean, rstd, (z - mean) * rstd * g + b


def lnbwd32(dy, z, mean, rstd, g, kpost, scale, order, defect=None):
    """(dz, dyn * xh, dyn) of the fp32 LayerNorm backward"""
    H = z.shape[1]
    dyn = dy * kpost * scale
    xh = (z - mean) * rstd
    tt = dyn * g
    a, b = tt, tt * xh
    if defect == "double_s":
        a, b = torch.cat([a, a[:, H - 4:]], 1), torch.cat([b, b[:, H - 4:]], 1)
    s1, s2 = rowsum32(a, order) / float(H), rowsum32(b, order) / float(H)
    return rstd * (tt - s1 - xh * s2), dyn * xh, dyn


def shifted(mask):
    """the keep mask one element late (the planted defect 7)"""
    return torch.roll(mask.reshape(-1), 1).reshape(mask.shape)


def host_mask(seed):
    """mask_fn of the CPU test: keep-scales 0 or 1 / (1 - p) as fp32, one stream per sid"""
    def fn(n, p, sid):
        g = torch.Generator().manual_seed(7919 * seed + sid)
        ik = (torch.tensor(1.0, dtype=F32) / (torch.tensor(1.0, dtype=F32) - torch.tensor(p, dtype=F32)))
        return (torch.rand(n, generator=g) >= p).to(F32) * ik
    return fn


class IllConditioned(Exception):
    pass


class RowCase:
    """one guarded row-kernel problem; see the module docstring.  ``mask_fn(n, p, sid)`` -> flat fp32 keep-scales."""

    DEFAULTS = dict(bias=False, res=False, zout=False, stats=True, p_pre=0.0, p_post=0.0, acc=False, out_scale=1.0, slabs=0,
                    const=False, offset=0.5, n=1, want_dres=False, acc_dres=False, gelu=False, null=(), prefill=False,
                    defer=False, T=1, seg=True, ld=None, ws_short=0)

    def __init__(self, kind, M, H, dt, device, seed=0, mask_fn=None, **opt):
        o = dict(self.DEFAULTS)
        assert set(opt) <= set(o), opt
        o.update(opt)
        self.kind, self.M, self.H, self.dt, self.device, self.o = kind, M, H, dt, device, o
        self.name = "%s %dx%d %s %s" % (kind, M, H, sfx(dt), " ".join("%s=%s" % kv for kv in sorted(opt.items())))
        self.mask_fn = mask_fn or host_mask(seed)
        for attempt in range(32):  # inputs are CHOSEN with no (nearly) constant row: redraw until the condition holds
            self.gen = torch.Generator().manual_seed(100003 * (seed + 1000 * attempt) + 31 * M + H)
            self.ins, self.outs, self.decoys, self.ref = {}, {}, {}, {}
            try:
                getattr(self, "_build_" + kind)()
                break
            except IllConditioned:
                if attempt == 31:
                    raise
        for g in list(self.outs.values()) + list(self.decoys.values()):
            g.seal()

    # ---- construction -------------------------------------------------------------------------------------------
    def rn(self, *s):
        return torch.randn(*s, generator=self.gen)

    def _in(self, name, val, dtype=None, ld=None):
        val = val if val.dim() == 2 else val[None]
        dtype = dtype or val.dtype
        g = Guarded(val.shape[0], val.shape[1], dtype, self.device, NAN, ld=val.shape[1] if ld is None else ld)
        g.view.copy_(val)
        self.ins[name] = g
        return g.view.double()

    def _out(self, name, rows, cols, dtype, init=None, decoy=False):
        g = Guarded(rows, cols, dtype, self.device, 0x55 if dtype == torch.uint8 else SENTINEL, ld=cols)
        if init is not None:
            g.view.copy_(init.reshape(rows, cols))
        (self.decoys if decoy else self.outs)[name] = g
        return g

    def _vecs(self, *names):
        for nm in names:
            val = 1.0 + 0.5 * self.rn(self.H) if nm[0] == "g" else 0.5 * self.rn(self.H)
            self.ref[nm] = self._in(nm, val.to(F32))

    def _keep(self, p, sid):
        M, H = self.M, self.H
        if p <= 0:
            return torch.ones((M, H), dtype=torch.float64, device=self.device)
        return self.mask_fn(M * H, p, sid).to(self.device).double().view(M, H)

    def _ws(self, nfloats):
        return self._out("ws", 1, nfloats, F32)

    def _assert_conditioned(self, z, skip_row=None):
        """the input condition of the rstd bound (helpers.py): var >= ROW_TAU * mean|z|^2 in every row"""
        var = z.var(-1, unbiased=False)
        ok = var >= ROW_TAU * z.abs().mean(-1) ** 2
        if skip_row is not None:
            ok[skip_row] = True
        if not bool(ok.all()):
            raise IllConditioned("%s: an input row is (nearly) constant" % self.name)

    def _build_ln_fwd(self):
        M, H, dt, o, R = self.M, self.H, self.dt, self.o, self.ref
        S = o["slabs"]
        if S:
            x = self._in("in", ((self.rn(S, M, H) + o["offset"]) / S).reshape(S * M, H).to(F32)).view(S, M, H)
            zs, za = x.sum(0), x.abs().sum(0)
        else:
            v = self.rn(M, H) + o["offset"]
            if o["const"]:
                v[0] = 3.0  # sums of 3.0 are exact in fp32 up to H = 2048 and 3 H / H = 3: t = 0 and out = beta exactly
            zs = self._in("in", v.to(dt))
            za = zs.abs()
        self._vecs("gamma", "beta")
        if o["bias"]:
            self._vecs("bias")
            zs, za = zs + R["bias"], za + R["bias"].abs()
        R["keep_pre"], R["keep_post"] = self._keep(o["p_pre"], SID_PRE), self._keep(o["p_post"], SID_POST)
        zs, za = zs * R["keep_pre"], za * R["keep_pre"]
        if o["res"]:
            r = self._in("residual", self.rn(M, H).to(dt))
            zs, za = zs + r, za + r.abs()
        self.nops = max(S - 1, 0) + int(o["bias"]) + int(o["p_pre"] > 0) + int(o["res"])
        R["zsum"], R["zabs"] = zs, za
        self._assert_conditioned(zs, 0 if o["const"] else None)
        old = (self.rn(M, H) * 2).to(dt) if o["acc"] else None
        R["old"] = None if old is None else old.double().to(self.device)
        self._out("out", M, H, dt, old)
        if o["zout"] or S:
            self._out("z_out", M, H, dt)
        if o["stats"]:
            self._out("stats", M, 2, F32)
        if dt == F32:
            self._out("out8", M, H, torch.uint8, decoy=True)  # fp32 storage has no e4m3 copy: must stay untouched

    def _build_ln_sum(self):
        M, H, dt, o, R = self.M, self.H, self.dt, self.o, self.ref
        for k in range(o["n"]):
            R["in%d" % k] = self._in("in%d" % k, (self.rn(M, H) + o["offset"]).to(dt))
            self._assert_conditioned(R["in%d" % k])
            self._vecs("gamma%d" % k, "beta%d" % k)
            R["keep%d" % k] = self._keep(o["p_post"], SID_POST + k)
            self._out("stats%d" % k, M, 2, F32)
        self._out("out", M, H, dt)

    def _build_ln_bwd(self):
        M, H, dt, o, R = self.M, self.H, self.dt, self.o, self.ref
        R["dy"] = self._in("dy", self.rn(M, H).to(dt))
        R["z"] = self._in("z", (self.rn(M, H) + o["offset"]).to(dt))
        self._assert_conditioned(R["z"])
        one = torch.ones(1, dtype=torch.float64, device=self.device)
        L = ln_terms(R["z"], one, 0.0 * one, EPS)
        R["stats"] = self._in("stats", torch.cat([L["mean"], L["rstd"]], 1).to(F32))
        self._vecs("gamma")
        R["gp"] = None
        if o["gelu"]:
            R["gp"] = gelu_grad64(self._in("gelu_aux", self.rn(M, H).to(dt)))
        R["keep_pre"], R["keep_post"] = self._keep(o["p_pre"], SID_PRE), self._keep(o["p_post"], SID_POST)
        self._out("d_in", M, H, dt)
        R["old_dres"] = None
        if o["acc_dres"]:
            old = self.rn(M, H).to(dt)
            R["old_dres"] = old.double().to(self.device)
            self._out("d_res", M, H, dt, old)
        elif o["want_dres"]:
            self._out("d_res", M, H, dt)
        for nm in GRAD_NAMES:
            init = (self.rn(H) if o["prefill"] else torch.zeros(H)).to(F32)
            R["old_" + nm] = init.double().to(self.device)
            self._out(nm, 1, H, F32, init, decoy=nm in o["null"])
        self.nblk = ln_bwd_blocks(M)
        self._ws(self.nblk * 3 * H)

    def _build_colsum(self):
        M, N, dt, o, R = self.M, self.H, self.dt, self.o, self.ref
        R["x"] = self._in("x", self.rn(M, N).to(dt), ld=o["ld"] or N)
        init = self.rn(N).to(F32)
        R["old"] = init.double().to(self.device)
        self._out("out", 1, N, F32, init)
        self._ws((M + 63) // 64 * N)

    def _build_embed(self):
        M, H, dt, o, R = self.M, self.H, self.dt, self.o, self.ref
        T = o["T"]
        assert M % T == 0
        self.V, self.P = 11, max(T, 2)
        R["word"] = self._in("word", (self.rn(self.V, H) + o["offset"]).to(dt))
        R["pos"] = self._in("pos", self.rn(self.P, H).to(dt))
        R["type"] = self._in("type", self.rn(2, H).to(dt))
        # heavy duplicates (ids 3 and 7 carry most rows) and the padding id 0
        pool = torch.tensor([3, 3, 3, 7, 7, 0, 5, 10, 3, 0])
        self.ids = pool[torch.randint(0, len(pool), (M,), generator=self.gen)].to(self.device)
        self.seg = torch.randint(0, 2, (M,), generator=self.gen).to(self.device) if o["seg"] else None
        self._vecs("gamma", "beta")
        R["keep_post"] = self._keep(o["p_post"], SID_POST)
        R["dy"] = self._in("dy", self.rn(M, H).to(dt))
        pos = torch.arange(M, device=self.device) % T
        ti = self.seg if self.seg is not None else torch.zeros(M, dtype=torch.int64, device=self.device)
        parts = (R["word"][self.ids], R["pos"][pos], R["type"][ti])
        R["zsum"], R["zabs"] = sum(parts), sum(p.abs() for p in parts)
        self._assert_conditioned(R["zsum"])
        self.pos_idx, self.type_idx = pos, ti
        for nm, shape, dtype in (("out", (M, H), dt), ("z_out", (M, H), dt), ("stats", (M, 2), F32), ("dz", (M, H), dt)):
            self._out(nm, shape[0], shape[1], dtype)
        for nm, rows in (("dword", self.V), ("dpos", self.P), ("dtype", 2), ("dgamma", 1), ("dbeta", 1)):
            init = (0.25 * self.rn(rows, H)).to(F32)
            if nm == "dword":
                init[0] = 0.0  # the padding row: stays exactly zero
            R["old_" + nm] = init.double().to(self.device)
            self._out(nm, rows, H, F32, init)
        self.nblk = ln_bwd_blocks(M)
        self._ws(self.nblk * 3 * H)

    def _build_visn(self):
        M, H, dt, o, R = self.M, self.H, self.dt, self.o, self.ref
        R["u"] = self._in("u", (self.rn(M, H) + o["offset"]).to(dt))
        R["boxes"] = self._in("boxes", torch.rand(M, 4, generator=self.gen).to(dt))
        R["Wb"] = self._in("Wb", self.rn(H, 4).to(F32))
        self._vecs("bf", "bb", "g1", "b1", "g2", "b2")
        R["keep_post"] = self._keep(o["p_post"], SID_POST)
        R["dy"] = self._in("dy", self.rn(M, H).to(dt))
        R["z1sum"], R["z1abs"] = R["u"] + R["bf"], R["u"].abs() + R["bf"].abs()
        R["z2sum"], R["z2abs"] = R["bb"] + R["boxes"] @ R["Wb"].t(), R["bb"].abs() + R["boxes"].abs() @ R["Wb"].abs().t()
        self._assert_conditioned(R["z1sum"])
        self._assert_conditioned(R["z2sum"])
        for nm, cols, dtype in (("out", H, dt), ("z1", H, dt), ("z2", H, dt), ("stats", 4, F32), ("du", H, dt)):
            self._out(nm, M, cols, dtype)
        for nm in VISN_GRADS:
            init = (0.25 * self.rn(H)).to(F32)
            R["old_" + nm] = init.double().to(self.device)
            self._out(nm, 1, H, F32, init)
        init = (0.25 * self.rn(H, 4)).to(F32)
        R["old_dWb"] = init.double().to(self.device)
        self._out("dWb", H, 4, F32, init)
        self.nblk = min((M + 3) // 4, 512)
        self._ws(self.nblk * 10 * H)

    # ---- launching (GPU) -----------------------------------------------------------------------------------------
    def reset(self):
        for g in list(self.outs.values()) + list(self.decoys.values()):
            g.reset()

    def p(self, name):
        g = self.ins.get(name) or self.outs.get(name)
        return None if g is None else g.view.data_ptr()

    def ws_bytes(self):
        return self.outs["ws"].cols * 4 - self.o["ws_short"]

    def fwd_problem(self, ops):
        o = self.o
        q = ops.LnFwdProblem(self.p("in"), self.p("bias"), self.p("residual"), self.p("gamma"), self.p("beta"), self.p("out"),
                             self.p("z_out"), self.p("stats"), self.M, SID_PRE, SID_POST, o["slabs"])
        if "out8" in self.decoys:
            q.out8 = self.decoys["out8"].view.data_ptr()
        return q

    def bwd_problem(self, ops):
        o = self.o
        gp = lambda nm: None if (nm in o["null"] or o["defer"]) else self.p(nm)
        return ops.LnBwdProblem(self.p("dy"), self.p("z"), self.p("stats"), self.p("gamma"), self.p("d_in"), self.p("d_res"),
                                gp("dgamma"), gp("dbeta"), gp("dbias"), self.p("gelu_aux"), self.p("ws"), self.ws_bytes(),
                                self.M, SID_PRE, SID_POST, int(o["acc_dres"]))

    def reduce_deferred(self, ops):
        tg = tuple(None if nm in self.o["null"] else self.outs[nm].view[0] for nm in GRAD_NAMES)
        ops.reduce_batch([(self.outs["ws"].view[0], self.nblk, 3, self.H, tg)])

    def launch(self, ops, rng=None):
        """one launch of the case through the C ABI (ops.call) with the guarded pointers"""
        o, M, H, s = self.o, self.M, self.H, sfx(self.dt)
        st, rp = ops.stream(), None if rng is None else rng.data_ptr()
        k = self.kind
        if k == "ln_fwd":
            if o["slabs"] or "out8" in self.decoys:
                launch_fwd_group(ops, [self], rng)
            else:
                ops.call("xggm_ln_fwd_" + s, self.p("in"), self.p("bias"), self.p("residual"), self.p("gamma"), self.p("beta"),
                         self.p("out"), self.p("z_out"), self.p("stats"), M, H, EPS, o["p_pre"], o["p_post"], rp, SID_PRE,
                         SID_POST, int(o["acc"]), float(o["out_scale"]), st)
        elif k == "ln_sum":
            a = ops.LnSumArgs()
            for i in range(o["n"]):
                a.inp[i], a.gamma[i], a.beta[i] = self.p("in%d" % i), self.p("gamma%d" % i), self.p("beta%d" % i)
                a.stats[i], a.sid_post[i] = self.p("stats%d" % i), SID_POST + i
            a.out, a.n, a.M, a.H, a.eps, a.p_post, a.rng = self.p("out"), o["n"], M, H, EPS, o["p_post"], rp
            ops.call("xggm_ln_sum_fwd_" + s, ctypes.byref(a), st)
        elif k == "ln_bwd":
            q = self.bwd_problem(ops)
            ops.call("xggm_ln_bwd_" + s, q.dy, q.z, q.stats, q.gamma, q.d_in, q.d_res, q.dgamma, q.dbeta, q.dbias, M, H,
                     o["p_pre"], o["p_post"], rp, SID_PRE, SID_POST, float(o["out_scale"]), int(o["acc_dres"]), q.gelu_aux,
                     q.ws, self.ws_bytes(), st)
            if o["defer"]:
                self.reduce_deferred(ops)
        elif k == "colsum":
            ops.call("xggm_colsum_" + s, self.p("x"), self.p("out"), M, H, self.ins["x"].ld, self.p("ws"), self.ws_bytes(), st)
        elif k == "embed":
            ip = lambda t: None if t is None else t.data_ptr()
            self.launch_embed_fwd(ops, rng)
            ops.call("xggm_embed_bwd_" + s, ip(self.ids), ip(self.seg), self.p("dy"), self.p("z_out"), self.p("stats"),
                     self.p("gamma"), self.p("dz"), self.p("dword"), self.p("dpos"), self.p("dtype"), self.p("dgamma"),
                     self.p("dbeta"), M, o["T"], H, o["p_post"], rp, SID_POST, self.p("ws"), self.ws_bytes(), st)
        elif k == "visn":
            self.launch_visn_fwd(ops, rng)
            self.launch_visn_bwd(ops, rng)

    def launch_embed_fwd(self, ops, rng=None):
        ip = lambda t: None if t is None else t.data_ptr()
        ops.call("xggm_embed_fwd_" + sfx(self.dt), ip(self.ids), ip(self.seg), self.p("word"), self.p("pos"), self.p("type"),
                 self.p("gamma"), self.p("beta"), self.p("out"), self.p("z_out"), self.p("stats"), self.M, self.o["T"], self.H,
                 EPS, self.o["p_post"], None if rng is None else rng.data_ptr(), SID_POST, None, None, None, 0, ops.stream())

    def launch_visn_fwd(self, ops, rng=None):
        ops.call("xggm_visn_embed_fwd_" + sfx(self.dt), self.p("u"), self.p("bf"), self.p("boxes"), self.p("Wb"), self.p("bb"),
                 self.p("g1"), self.p("b1"), self.p("g2"), self.p("b2"), self.p("out"), self.p("z1"), self.p("z2"),
                 self.p("stats"), self.M, self.H, EPS, self.o["p_post"], None if rng is None else rng.data_ptr(), SID_POST,
                 None, None, None, 0, ops.stream())

    def launch_visn_bwd(self, ops, rng=None):
        ops.call("xggm_visn_embed_bwd_" + sfx(self.dt), self.p("dy"), self.p("z1"), self.p("z2"), self.p("stats"),
                 self.p("boxes"), self.p("g1"), self.p("g2"), self.p("du"), self.p("dbf"), self.p("dg1"), self.p("db1"),
                 self.p("dWb"), self.p("dbb"), self.p("dg2"), self.p("db2"), self.M, self.H, self.o["p_post"],
                 None if rng is None else rng.data_ptr(), SID_POST, self.p("ws"), self.ws_bytes(), ops.stream())

    # ---- the emulated kernels of the CPU test -------------------------------------------------------------------------
    def w(self, name, val):
        g = self.outs[name]
        g.view.copy_(val.reshape(g.rows, g.cols).to(g.view.dtype))

    def f(self, name):
        return self.ins[name].view.float()

    def emulate(self, order="kernel", defect=None):
        """every output of the case in fp32 torch, written through the windows; ``defect``: one of the planted ones"""
        getattr(self, "_emulate_" + self.kind)(order, defect)

    def _k32(self, name, defect):
        k = self.ref[name].float()
        return shifted(k) if defect == "shifted_keep" else k

    def _emulate_ln_fwd(self, order, defect):
        o, M, H, dt = self.o, self.M, self.H, self.dt
        if o["slabs"]:
            x = self.f("in").view(o["slabs"], M, H)
            z = x[0]
            for s in range(1, o["slabs"] - (1 if defect == "dropped_slab" else 0)):
                z = z + x[s]
        else:
            z = self.f("in")
        if o["bias"]:
            z = z + self.f("bias")
        if o["p_pre"] > 0:
            z = z * self._k32("keep_pre", defect)
        if o["res"]:
            z = z + self.f("residual")
        if "z_out" in self.outs:
            z = z.to(dt).float()
            self.w("z_out", z)
        mean, rstd, y = ln32(z, self.f("gamma"), self.f("beta"), EPS, order, defect)
        if "stats" in self.outs:
            self.w("stats", torch.cat([mean, rstd], 1))
        if o["p_post"] > 0:
            y = y * self._k32("keep_post", defect)
        y = y * torch.tensor(o["out_scale"], dtype=F32)
        if o["acc"]:
            y = y + self.outs["out"].view.float()
        self.w("out", y)

    def _emulate_ln_sum(self, order, defect):
        acc = torch.zeros((self.M, self.H), dtype=F32)
        for k in range(self.o["n"]):
            mean, rstd, y = ln32(self.f("in%d" % k), self.f("gamma%d" % k), self.f("beta%d" % k), EPS, order, defect)
            self.w("stats%d" % k, torch.cat([mean, rstd], 1))
            acc = acc + y * self._k32("keep%d" % k, defect)
        self.w("out", acc)

    def _emulate_ln_bwd(self, order, defect):
        o, M, H = self.o, self.M, self.H
        st = self.f("stats")
        dz, tg, tb = lnbwd32(self.f("dy"), self.f("z"), st[:, :1], st[:, 1:], self.f("gamma"), self._k32("keep_post", defect),
                             torch.tensor(o["out_scale"], dtype=F32), order, defect)
        if "d_res" in self.outs:
            self.w("d_res", dz + self.outs["d_res"].view.float() if (o["acc_dres"] and defect != "dres_overwritten") else dz)
        din = dz * self._k32("keep_pre", defect)
        tbias = din
        if o["gelu"]:
            din = din * self.ref["gp"].float()
            tbias = tbias if defect == "dbias_before_gelu" else din
        self.w("d_in", din)
        part = torch.zeros((self.nblk, 3, H), dtype=F32)
        for r in range(M):  # the partial rows of the workspace: waves added in order inside a workgroup
            part[(r // 8) % self.nblk] += torch.stack([tg[r], tb[r], tbias[r]])
        self.w("ws", part)
        for nm, term in zip(GRAD_NAMES, (tg, tb, tbias)):
            if nm not in o["null"]:
                s = colsum32(term, order, 8, 256, drop_last_block=(defect == "short_dgamma" and nm == "dgamma"))
                self.w(nm, self.outs[nm].view[0].float() + s)

    def _emulate_colsum(self, order, defect):
        self.w("out", self.outs["out"].view[0].float() + colsum32(self.f("x"), order, 4, 1 << 30))
        self.w("ws", torch.zeros(self.outs["ws"].cols))

    def _emulate_embed(self, order, defect):
        M, H, dt = self.M, self.H, self.dt
        ids, pos, ti = self.ids.cpu(), self.pos_idx.cpu(), self.type_idx.cpu()
        z = ((self.f("word")[ids] + self.f("pos")[pos]) + self.f("type")[ti]).to(dt).float()
        self.w("z_out", z)
        mean, rstd, y = ln32(z, self.f("gamma"), self.f("beta"), EPS, order, defect)
        self.w("stats", torch.cat([mean, rstd], 1))
        kp = self._k32("keep_post", defect)
        self.w("out", y * kp)
        dz, tg, tb = lnbwd32(self.f("dy"), z, mean, rstd, self.f("gamma"), kp, torch.tensor(1.0), order, defect)
        self.w("dz", dz)
        dzs = self.outs["dz"].view.float()
        self.w("ws", torch.zeros(self.outs["ws"].cols))
        for nm, term in (("dgamma", tg), ("dbeta", tb)):
            self.w(nm, self.outs[nm].view[0].float() + colsum32(term, order, 8, 256))
        for nm, key in (("dword", ids), ("dpos", pos), ("dtype", ti)):
            g = self.outs[nm].view.float().clone()
            for k in sorted(set(key.tolist())):
                if k == 0 or (nm == "dtype" and self.seg is None):
                    continue  # row 0 is every table's padding_idx; without segment ids the type table receives nothing
                g[k] = g[k] + colsum32(dzs[key == k], "seq" if order == "kernel" else order)
            self.w(nm, g)

    def _emulate_visn(self, order, defect):
        M, H, dt = self.M, self.H, self.dt
        bx, Wb = self.f("boxes"), self.f("Wb")
        z1 = (self.f("u") + self.f("bf")).to(dt).float()
        acc = self.f("bb") + Wb[:, 0] * bx[:, 0:1]
        for j in range(1, 4):
            acc = acc + Wb[:, j] * bx[:, j:j + 1]
        z2 = acc.to(dt).float()
        self.w("z1", z1), self.w("z2", z2)
        m1, r1, y1 = ln32(z1, self.f("g1"), self.f("b1"), EPS, order, defect)
        m2, r2, y2 = ln32(z2, self.f("g2"), self.f("b2"), EPS, order, defect)
        self.w("stats", torch.cat([m1, r1, m2, r2], 1))
        kp = self._k32("keep_post", defect)
        self.w("out", 0.5 * (y1 + y2) * kp)
        half = torch.tensor(0.5)
        d1, tg1, tb1 = lnbwd32(self.f("dy"), z1, m1, r1, self.f("g1"), kp, half, order, defect)
        d2, tg2, tb2 = lnbwd32(self.f("dy"), z2, m2, r2, self.f("g2"), kp, half, order, defect)
        self.w("du", d1)
        self.w("ws", torch.zeros(self.outs["ws"].cols))
        for nm, term in zip(VISN_GRADS, (d1, tg1, tb1, d2, tg2, tb2)):
            self.w(nm, self.outs[nm].view[0].float() + colsum32(term, order, 4, 512))
        gw = self.outs["dWb"].view.float().clone()
        for j in range(4):
            gw[:, j] = gw[:, j] + colsum32(d2 * bx[:, j:j + 1], order, 4, 512)
        self.w("dWb", gw)

    # ---- checks ---------------------------------------------------------------------------------------------------
    def canaries(self, what):
        def outside_ok(g):  # ld == cols here: the outside is the rows before and behind the window, compared in place
            if g.ld != g.cols:
                return g.untouched_outside()
            a, b, e = _ints(g.buf), _ints(g.pristine), LEAD + g.rows
            return torch.equal(a[:LEAD], b[:LEAD]) and torch.equal(a[e:], b[e:])
        for name, g in self.outs.items():
            assert outside_ok(g), "%s: cells outside the [%d, %d] window of %s were written" % (what, g.rows, g.cols, name)
        for name, g in self.decoys.items():
            assert torch.equal(_ints(g.buf), _ints(g.pristine)), "%s: %s was not asked for and was written" % (what, name)

    def untouched(self):
        """every output and decoy still as sealed, windows included (a refused launch writes nothing)"""
        return all(torch.equal(_ints(g.buf), _ints(g.pristine)) for g in list(self.outs.values()) + list(self.decoys.values()))

    def got(self, name):
        return self.outs[name].view.double()

    def excesses(self, canaries=True, tag=""):
        """{output: |err| / bound per element} of everything the case owns (nothing excluded)"""
        if canaries:
            self.canaries("%s [%s]" % (self.name, tag))
        return getattr(self, "_check_" + self.kind)()

    def check(self, tag, canaries=True):
        """canaries first, then assert_excess on every output; returns {output: largest |err| / bound}"""
        what = "%s [%s]" % (self.name, tag)
        return {k: assert_excess(e, what + " " + k) for k, e in self.excesses(canaries, tag).items()}

    def _ex(self, name, ref, bound, got=None):
        g = self.got(name) if got is None else got
        return bound_excess(g.reshape(ref.shape), ref, bound)

    def _stats_ex(self, L, got_mean, got_rstd):
        return torch.cat([bound_excess(got_mean, L["mean"], L["e_mean"]),
                          bound_excess(got_rstd, L["rstd"], L["rho"] * L["rstd"])], 1)

    def _check_ln_fwd(self):
        o, R, dt = self.o, self.ref, self.dt
        out = {}
        if "z_out" in self.outs:
            zst = self.got("z_out")
            out["z"] = self._ex("z_out", R["zsum"], row_z_bound(R["zabs"], o["slabs"], dt, R["zsum"]) if self.nops or dt == BF16
                                else torch.zeros_like(R["zsum"]))
            L = ln_terms(zst, R["gamma"], R["beta"], EPS)
        else:
            e_z = row_z_bound(R["zabs"], o["slabs"], F32, R["zsum"]) if self.nops else None
            L = ln_terms(R["zsum"], R["gamma"], R["beta"], EPS, e_z)
        if "stats" in self.outs:
            st = self.got("stats")
            out["stats"] = self._stats_ex(L, st[:, :1], st[:, 1:])
        ref, bound = ln_out_bound(L, R["keep_post"], o["out_scale"], R["old"], dt)
        out["out"] = self._ex("out", ref, bound)
        return out

    def _check_ln_sum(self):
        o, R = self.o, self.ref
        out, ref, bound, mag = {}, 0.0, 0.0, 0.0
        for k in range(o["n"]):
            if "L%d" % k not in R:  # the terms are inputs: computed once
                R["L%d" % k] = ln_terms(R["in%d" % k], R["gamma%d" % k], R["beta%d" % k], EPS)
            L = R["L%d" % k]
            st = self.got("stats%d" % k)
            out["stats%d" % k] = self._stats_ex(L, st[:, :1], st[:, 1:])
            r, b = ln_out_bound(L, R["keep%d" % k], 1.0, None, self.dt, store=False)
            ref, bound, mag = ref + r, bound + b, mag + r.abs()
        out["out"] = self._ex("out", ref, bound + o["n"] * U32 * mag + store_term(ref, self.dt))
        return out

    def _check_ln_bwd(self):
        o, R, dt = self.o, self.ref, self.dt
        st = R["stats"]
        if "B" not in R:  # every operand is an input: computed once, shared by every launch of the case
            R["B"] = ln_bwd_terms(R["dy"], R["z"], st[:, :1], st[:, 1:], R["gamma"], R["keep_post"], o["out_scale"],
                                  R["keep_pre"], R["gp"])
        B = R["B"]
        out = {"d_in": self._ex("d_in", B["din"], B["e_din"] + store_term(B["din"], dt))}
        if "d_res" in self.outs:
            ref, bound = B["dz"], B["e_dz"]
            if R["old_dres"] is not None:
                ref = ref + R["old_dres"]
                bound = bound + U32 * (R["old_dres"].abs() + ref.abs())
            out["d_res"] = self._ex("d_res", ref, bound + store_term(ref, dt))
        for nm, t, e in (("dgamma", B["tg"], B["e_tg"]), ("dbeta", B["tb"], B["e_tb"]), ("dbias", B["din"], B["e_din"])):
            if nm in self.outs:
                ref, bound = colsum_bound(t, e, R["old_" + nm])
                out[nm] = self._ex(nm, ref, bound)
        return out

    def _check_colsum(self):
        R = self.ref
        ref, bound = colsum_bound(R["x"], torch.zeros_like(R["x"]), R["old"])
        return {"out": self._ex("out", ref, bound)}

    def _scatter_ref(self, dz, key, rows, old, skip0=True):
        ref, bound = old.clone(), torch.zeros_like(old)
        for k in range(rows):
            sel = dz[key == k]
            if (k == 0 and skip0) or sel.shape[0] == 0:
                continue
            ref[k], bound[k] = colsum_bound(sel, torch.zeros_like(sel), old[k])
        return ref, bound

    def _check_embed(self):
        R, dt = self.ref, self.dt
        out = {"z": self._ex("z_out", R["zsum"], row_z_bound(R["zabs"], 0, dt, R["zsum"]))}
        z = self.got("z_out")
        L = ln_terms(z, R["gamma"], R["beta"], EPS)
        st = self.got("stats")
        out["stats"] = self._stats_ex(L, st[:, :1], st[:, 1:])
        ref, bound = ln_out_bound(L, R["keep_post"], 1.0, None, dt)
        out["out"] = self._ex("out", ref, bound)
        one = torch.ones_like(z)
        B = ln_bwd_terms(R["dy"], z, st[:, :1], st[:, 1:], R["gamma"], R["keep_post"], 1.0, one, None)
        out["dz"] = self._ex("dz", B["din"], B["e_din"] + store_term(B["din"], dt))
        for nm, t, e in (("dgamma", B["tg"], B["e_tg"]), ("dbeta", B["tb"], B["e_tb"])):
            ref, bound = colsum_bound(t, e, R["old_" + nm][0])
            out[nm] = self._ex(nm, ref, bound)
        dz = self.got("dz")  # the scatter reads the stored rows
        for nm, key, rows in (("dword", self.ids, self.V), ("dpos", self.pos_idx, self.P), ("dtype", self.type_idx, 2)):
            if nm == "dtype" and self.seg is None:
                ref, bound = R["old_dtype"], torch.zeros_like(R["old_dtype"])
            else:
                ref, bound = self._scatter_ref(dz, key, rows, R["old_" + nm])
            out[nm] = self._ex(nm, ref, bound)
        assert bool((self.got("dword")[0] == 0).all()), "%s: the padding row of the word table received gradient" % self.name
        return out

    def _check_visn(self):
        R, dt = self.ref, self.dt
        out = {"z1": self._ex("z1", R["z1sum"], row_z_bound(R["z1abs"], 0, dt, R["z1sum"])),
               "z2": self._ex("z2", R["z2sum"], 2.0 * row_z_bound(R["z2abs"], 4, dt, R["z2sum"]) - store_term(R["z2sum"], dt))}
        z1, z2, st = self.got("z1"), self.got("z2"), self.got("stats")
        L1, L2 = ln_terms(z1, R["g1"], R["b1"], EPS), ln_terms(z2, R["g2"], R["b2"], EPS)
        out["stats"] = torch.cat([self._stats_ex(L1, st[:, 0:1], st[:, 1:2]), self._stats_ex(L2, st[:, 2:3], st[:, 3:4])], 1)
        (r1, e1), (r2, e2) = (ln_out_bound(L, 1.0, 1.0, None, dt, store=False) for L in (L1, L2))
        ref = 0.5 * (r1 + r2) * R["keep_post"]
        out["out"] = self._ex("out", ref, 0.5 * (e1 + e2 + U32 * (r1.abs() + r2.abs())) * R["keep_post"] + 3 * U32 * ref.abs()
                              + store_term(ref, dt))
        one = torch.ones_like(z1)
        B1 = ln_bwd_terms(R["dy"], z1, st[:, 0:1], st[:, 1:2], R["g1"], R["keep_post"], 0.5, one, None)
        B2 = ln_bwd_terms(R["dy"], z2, st[:, 2:3], st[:, 3:4], R["g2"], R["keep_post"], 0.5, one, None)
        out["du"] = self._ex("du", B1["din"], B1["e_din"] + store_term(B1["din"], dt))
        for nm, t, e in zip(VISN_GRADS, (B1["din"], B1["tg"], B1["tb"], B2["din"], B2["tg"], B2["tb"]),
                            (B1["e_din"], B1["e_tg"], B1["e_tb"], B2["e_din"], B2["e_tg"], B2["e_tb"])):
            ref, bound = colsum_bound(t, e, R["old_" + nm])
            out[nm] = self._ex(nm, ref, bound)
        refs, bounds = [], []
        for j in range(4):  # the stride-4 columns of box_fc.weight's gradient
            bx = R["boxes"][:, j:j + 1]
            t = B2["din"] * bx
            r, b = colsum_bound(t, B2["e_din"] * bx.abs() + U32 * t.abs(), R["old_dWb"][:, j])
            refs.append(r), bounds.append(b)
        out["dWb"] = self._ex("dWb", torch.stack(refs, 1), torch.stack(bounds, 1))
        return out


def launch_fwd_group(ops, cases, rng=None):
    """several ln_fwd cases of one H, type and dropout setting in ONE grouped launch"""
    c0 = cases[0]
    arr = (ops.LnFwdProblem * len(cases))(*[c.fwd_problem(ops) for c in cases])
    ops.call("xggm_ln_fwd_grouped_" + sfx(c0.dt), ctypes.cast(arr, ctypes.c_void_p), len(cases), c0.H, EPS, c0.o["p_pre"],
             c0.o["p_post"], None if rng is None else rng.data_ptr(), int(c0.o["acc"]), float(c0.o["out_scale"]), None,
             ops.stream())


def launch_bwd_group(ops, cases, rng=None):
    c0 = cases[0]
    arr = (ops.LnBwdProblem * len(cases))(*[c.bwd_problem(ops) for c in cases])
    ops.call("xggm_ln_bwd_grouped_" + sfx(c0.dt), ctypes.cast(arr, ctypes.c_void_p), len(cases), c0.H, c0.o["p_pre"],
             c0.o["p_post"], None if rng is None else rng.data_ptr(), float(c0.o["out_scale"]), None, ops.stream())


def snapshot(case):
    return {k: g.view.clone() for k, g in case.outs.items() if k != "ws"}
