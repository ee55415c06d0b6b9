"""Edge-tile GEMM cases shared by test_gemm_edges_cpu.py and test_gemm_edges_gpu.py.

A ``Case`` is one product C[M, N] = epilogue(A[M, K] . B[N, K]^T) with
  * its operands laid out as the kernels' operand forms want them (``form`` = a_mode b_mode of gemm.hip's pick_mode:
    1 = the reduction index is contiguous, 0 = the row index is contiguous; forward "11", dgrad "10", wgrad "00", "01"),
  * every operand a window into a larger buffer filled with NaN (LEAD rows before, MOAT_ROWS rows after, the row stride
    padded): a kernel that loads past M, N or K without masking turns an output into NaN and stays inside the
    allocation while doing it,
  * every output (C, pre-activation, column-sum partials and their target, norm slots, e4m3 copy) a window into a buffer
    filled with a finite sentinel: after a launch every cell outside the window must hold the sentinel's bits,
  * fp64 references computed ONCE from the already-rounded inputs, with the magnitude sums gemm_excess needs.
Nothing here imports the library: the CPU test drives the same cases with an emulated kernel.
"""
import math

import torch

from helpers import U32, U_BF16, assert_excess, gemm_excess

# (M, N, K): one row / column past the 64 and the 128 tile edges, partial 32-row column-sum blocks, partial 64 x 64 norm
# blocks, both k-loops (K % 64 == 0: LDS-DMA; K in {72, 200}: the register-staged loop)
SHAPES = [(1, 8, 64), (65, 72, 64), (129, 136, 128), (63, 200, 192), (100, 264, 72), (180, 136, 200)]
FORMS = ("11", "10", "00", "01")
LEAD, MOAT_ROWS = 8, 128
SENTINEL = -1234.0
ACT_NONE, ACT_GELU, ACT_SIGMOID, ACT_TANH, ACT_GELU_GRAD = 0, 1, 2, 3, 4
BF16, F32 = torch.bfloat16, torch.float32

# epilogues; which value of gemm.hip's epilogue_kind() each reaches on the tuned kernels (N % 4 == 0, ldc % 4 == 0):
#   kind 0 (register epilogue, C = acc + bias):       plain, bias, f32, bias_f32, f32_sqsum
#   kind 1 (register epilogue, GELU + preact):        gelu_pre, gelu_pre_c8
#   kind 2 (staged walk):                             everything with a residual, `accumulate`, column sums, sigmoid,
#                                                     tanh, GELU_GRAD or an e4m3 copy without GELU -- and every
#                                                     epilogue at N = 50 (N % 4 != 0), where the staged walk also
#                                                     leaves its 16-byte stores for the scalar ones (vec_ok == false)
EPILOGUES = {
    "plain": {},
    "bias": dict(bias=True),
    "bias_f32": dict(bias=True, f32=True),
    "bias_res": dict(bias=True, res=True),
    "bias_c8": dict(bias=True, c8=True),
    "gelu_pre": dict(bias=True, act=ACT_GELU, pre=True),
    "gelu_pre_c8": dict(bias=True, act=ACT_GELU, pre=True, c8=True),
    "sigmoid_f32": dict(bias=True, act=ACT_SIGMOID, f32=True),
    "tanh": dict(bias=True, act=ACT_TANH),
    "res": dict(res=True),
    "acc": dict(acc=True),
    "gelugrad_colsum": dict(act=ACT_GELU_GRAD, colsum=True),
    "gelugrad_colsum_f32": dict(act=ACT_GELU_GRAD, colsum=True, f32=True),
    "f32": dict(f32=True),
    "f32_acc": dict(f32=True, acc=True),
    "f32_sqsum": dict(f32=True, sqsum=True),
    "f32_acc_sqsum": dict(f32=True, acc=True, sqsum=True),
}
# what each operand form carries in the training step (plus "01", which only ops._problem builds)
FORM_EPILOGUES = {
    "11": ("bias", "gelu_pre", "gelu_pre_c8", "bias_c8", "sigmoid_f32", "tanh", "bias_res"),
    "10": ("plain", "res", "acc", "gelugrad_colsum", "gelugrad_colsum_f32"),
    "00": ("f32", "f32_acc", "f32_sqsum", "f32_acc_sqsum", "plain"),
    "01": ("plain", "bias_f32", "f32_acc_sqsum"),
}
# Lipschitz constants of the activations (in front of the accumulation term)
LIPSCHITZ = {ACT_GELU: 1.13, ACT_SIGMOID: 0.25, ACT_TANH: 1.0}
C8_QSCALE = 4.0


def up(n, m):
    return (n + m - 1) // m * m


def _ints(t):
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def gelu64(x):
    return x * 0.5 * (1 + torch.erf(x / math.sqrt(2)))


def gelu_grad64(x):
    return 0.5 * (1 + torch.erf(x / math.sqrt(2))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2 * math.pi)


def act64(act, x):
    return {ACT_GELU: gelu64, ACT_SIGMOID: torch.sigmoid, ACT_TANH: torch.tanh}[act](x)


class Guarded:
    """a [rows, cols] window into a buffer of LEAD + rows + MOAT_ROWS rows of ``ld`` columns filled with ``fill``"""

    def __init__(self, rows, cols, dtype, device, fill, ld=None):
        self.rows, self.cols = rows, cols
        self.ld = up(cols, 8) + 8 if ld is None else ld
        assert self.ld >= cols
        self.buf = torch.full((LEAD + rows + MOAT_ROWS, self.ld), fill, dtype=dtype, device=device)
        self.view = self.buf[LEAD:LEAD + rows, :cols]
        assert self.view.data_ptr() % 16 == 0
        self.pristine = None

    def seal(self):
        """remember the buffer as it is before any launch (the window's initial contents included)"""
        self.pristine = self.buf.clone()
        return self

    def reset(self):
        self.buf.copy_(self.pristine)

    def untouched_outside(self):
        cur = self.buf.clone()
        cur[LEAD:LEAD + self.rows, :self.cols] = self.pristine[LEAD:LEAD + self.rows, :self.cols]
        return torch.equal(_ints(cur), _ints(self.pristine))


def _nan_fill(dtype):
    return 0x7F if dtype == torch.uint8 else float("nan")  # 0x7f: the NaN of e4m3fn


def _operand(val, kmajor, device, ld=None):
    """[R, K] values -> (Guarded, row stride, reduction stride) in the k-contiguous or the row-contiguous layout"""
    R, K = val.shape
    if kmajor:
        g = Guarded(R, K, val.dtype, device, _nan_fill(val.dtype), ld)
        g.view.copy_(val)
        return g, g.ld, 1
    g = Guarded(K, R, val.dtype, device, _nan_fill(val.dtype), ld)
    g.view.copy_(val.t())
    return g, 1, g.ld


class Case:
    """one product with guarded operands and outputs and its fp64 references; see the module docstring"""

    def __init__(self, M, N, K, form, epi, device, dt=BF16, seed=0, ldc=None, a_ld=None, b_ld=None, fp8=False):
        self.M, self.N, self.K, self.form, self.epi, self.dt, self.fp8, self.device = M, N, K, form, epi, dt, fp8, device
        e = dict(bias=False, res=False, acc=False, f32=False, act=ACT_NONE, pre=False, colsum=False, sqsum=False, c8=False)
        e.update(EPILOGUES[epi])
        self.e = e
        self.name = "%dx%dx%d form %s %s%s" % (M, N, K, form, epi, " e4m3" if fp8 else "")
        gen = torch.Generator().manual_seed(1000 * seed + 17 * M + 3 * N + K)
        rn = lambda *s: torch.randn(*s, generator=gen)
        self.out_dtype = F32 if e["f32"] else dt
        sdt = dt  # storage type of residual / preact / aux
        if fp8:
            assert form == "11" and dt == BF16
            a8, b8 = rn(M, K).to(torch.float8_e4m3fn), (rn(N, K) * 2).to(torch.float8_e4m3fn)
            A64, B64 = a8.float().double(), b8.float().double()
            a, b = a8.view(torch.uint8), b8.view(torch.uint8)
            a_ld = up(K, 16) + 16 if a_ld is None else a_ld
            b_ld = up(K, 16) + 16 if b_ld is None else b_ld
            self.sx = torch.tensor([0.75 / math.sqrt(K)], dtype=F32, device=device)
            self.sw = torch.tensor([1.5], dtype=F32, device=device)
            deq = float(self.sx.double().cpu() * self.sw.double().cpu())
        else:
            a, b = rn(M, K).to(dt), (rn(N, K) * (1.5 / math.sqrt(K))).to(dt)
            A64, B64, deq = a.double(), b.double(), 1.0
        self.A, self.a_rs, self.a_ks = _operand(a, form[0] == "1", device, a_ld)
        self.B, self.b_ns, self.b_ks = _operand(b, form[1] == "1", device, b_ld)
        P, SP = (A64 @ B64.t()) * deq, (A64.abs() @ B64.abs().t()) * deq
        self.bias = None
        if e["bias"]:
            bv = rn(N)
            self.bias = Guarded(1, N, F32, device, float("nan"), ld=N)
            self.bias.view.copy_(bv[None])
            P, SP = P + bv.double(), SP + bv.double().abs()
        # outputs: sentinel everywhere, then the window's initial contents, then sealed
        self.C = Guarded(M, N, self.out_dtype, device, SENTINEL, ldc)
        ldc = self.C.ld
        self.outputs = {"C": self.C}
        self.pre = self.res = self.aux = self.part = self.colsum = self.sq = self.c8 = None
        self.pre_ref = self.pre_S = None
        if e["pre"]:
            self.pre = self.outputs["preact"] = Guarded(M, N, sdt, device, SENTINEL, ldc)
            self.pre_ref, self.pre_S = P.to(device), SP.to(device)
        # C reference: v = f(P) (+ residual) (+ old C).  With a stored pre-activation the kernel applies f to the value AS
        # STORED, so the reference does too (self.dynamic) and no accumulation term remains for that part.
        self.dynamic = e["act"] in LIPSCHITZ and e["pre"]
        extra = torch.zeros_like(P)
        if e["act"] == ACT_GELU_GRAD:
            u = rn(M, N).to(sdt)
            self.aux = Guarded(M, N, sdt, device, float("nan"), ldc)
            self.aux.view.copy_(u)
            gp = gelu_grad64(u.double())
            # C = acc * gelu'(aux): |gelu'(aux)| in front of the accumulation term; the fp32 evaluation of the function,
            # 4 u (1 + |gelu'|), reaches C multiplied by |acc|; 4 u (1 + |C|) for the product itself
            extra = 4 * U32 * (1 + gp.abs()) * P.abs()
            P, SP = P * gp, SP * gp.abs()
            extra = extra + 4 * U32 * (1 + P.abs())
        elif self.dynamic:
            P, SP = torch.zeros_like(P), torch.zeros_like(SP)
        elif e["act"] in LIPSCHITZ:
            P, SP = act64(e["act"], P), SP * LIPSCHITZ[e["act"]]
            extra = 4 * U32 * (1 + P.abs())
        if e["res"]:
            r = rn(M, N).to(sdt)
            self.res = Guarded(M, N, sdt, device, float("nan"), ldc)
            self.res.view.copy_(r)
            P, SP = P + r.double(), SP + r.double().abs()
        if e["acc"]:
            old = (rn(M, N) * 2).to(self.out_dtype)
            self.C.view.copy_(old)
            P, SP = P + old.double(), SP + old.double().abs()
        self.ref, self.S, self.extra = P.to(device), SP.to(device), extra.to(device)
        if e["colsum"]:
            nblk = (M + 31) // 32
            self.part = self.outputs["colsum partials"] = Guarded(nblk, N, F32, device, SENTINEL, ld=N)
            if N % 4 == 0:  # the second stage (xggm_partial_reduce_batch) takes widths that are multiples of 4
                self.colsum = self.outputs["colsum"] = Guarded(1, N, F32, device, SENTINEL, ld=N)
                self.colsum.view.fill_(2.0)
        if e["sqsum"]:
            self.nr, self.nc = (M + 63) // 64, (N + 63) // 64
            self.sq = self.outputs["norm slots"] = Guarded(1, self.nr * self.nc, F32, device, SENTINEL, ld=self.nr * self.nc)
        if e["c8"]:
            self.c8 = self.outputs["e4m3 copy"] = Guarded(M, N, torch.uint8, device, 0x55, ldc)
            self.q8 = torch.tensor([C8_QSCALE], dtype=F32, device=device)
        for g in self.outputs.values():
            g.seal()

    # ---- launching -------------------------------------------------------------------------------------------
    def reset(self):
        for g in self.outputs.values():
            g.reset()

    def problem(self, ops):
        """the xggm_gemm_problem of this case (ops._problem: raw strides, so every operand form can be built)"""
        from xggm_amd._lib import ptr
        v = lambda g: None if g is None else g.view
        e = self.e
        p = ops._problem(self.A.view, self.B.view, self.C.view, self.M, self.N, self.K, self.a_rs, self.a_ks, self.b_ns,
                         self.b_ks, self.C.ld, bias=None if self.bias is None else self.bias.view[0], residual=v(self.res),
                         preact=v(self.pre), aux=v(self.aux), act=e["act"], c_f32=e["f32"], accumulate=e["acc"],
                         colsum=v(self.part))
        if self.sq is not None:
            p.sqsum = ptr(self.sq.view)
        if self.c8 is not None:
            p.c8, p.c8_qscale = ptr(self.c8.view), ptr(self.q8)
        if self.fp8:
            p.scale_a, p.scale_b = ptr(self.sx), ptr(self.sw)
        p.keep = p.keep + (self,)
        return p

    def reduce_colsum(self, ops):
        """second stage of the bias gradient: the partial rows are added onto the running column sums"""
        if self.colsum is not None:
            ops.reduce_batch([(self.part.view, self.part.rows, 1, self.N, (self.colsum.view[0],))])

    # ---- the emulated kernel of the CPU test ---------------------------------------------------------------------
    def logical(self):
        """(A [M, K], B [N, K]) as fp32, read through the windows only"""
        a = self.A.view if self.form[0] == "1" else self.A.view.t()
        b = self.B.view if self.form[1] == "1" else self.B.view.t()
        if self.fp8:
            a, b = a.view(torch.float8_e4m3fn), b.view(torch.float8_e4m3fn)
        return a.float(), b.float()

    def emulate_f32(self):
        """the bf16 linear as an fp32 product (plus bias) of the bf16 inputs, before the store's rounding"""
        a, b = self.logical()
        y = a @ b.t()
        if self.fp8:
            y = y * (float(self.sx) * float(self.sw))
        return y + self.bias.view[0] if self.bias is not None else y

    def emulate_launch(self):
        """every output of the case as the kernels define them (xggm.h: epilogue), in fp32 torch, written through the
        windows: what the CPU test feeds to check()"""
        e, M, N = self.e, self.M, self.N
        v = self.emulate_f32()
        if self.pre is not None:
            self.pre.view.copy_(v.to(self.dt))
            v = self.pre.view.float()
        if e["act"] == ACT_GELU_GRAD:
            v = v * gelu_grad64(self.aux.view.double()).float()
        elif e["act"] != ACT_NONE:
            v = act64(e["act"], v.double()).float()
        if self.res is not None:
            v = v + self.res.view.float()
        if self.part is not None:
            pad = torch.zeros((self.part.rows * 32, N))
            pad[:M] = v
            self.part.view.copy_(pad.view(-1, 32, N).sum(1))
            if self.colsum is not None:
                self.colsum.view[0] += self.part.view.sum(0)
        if self.c8 is not None:
            self.c8.view.copy_((v * C8_QSCALE).to(torch.float8_e4m3fn).view(torch.uint8))
        if e["acc"]:
            v = v + self.C.view.float()
        self.C.view.copy_(v.to(self.out_dtype))
        if self.sq is not None:
            pad = torch.zeros((self.nr * 64, self.nc * 64))
            pad[:M, :N] = self.C.view
            self.sq.view.copy_((pad * pad).view(self.nr, 64, self.nc, 64).sum((1, 3)).view(1, -1))

    # ---- checks -----------------------------------------------------------------------------------------------
    def c_reference(self):
        if not self.dynamic:
            return self.ref, self.S, self.extra
        f = act64(self.e["act"], self.pre.view.double())
        return f + self.ref, self.S, 4 * U32 * (1 + f.abs())

    def check(self, tag, canaries=True):
        """canaries, element-wise bounds of C and the pre-activation, column sums and norm slots against the launch's
        own stored output.  Returns {what: largest |err| / bound}."""
        what = "%s [%s]" % (self.name, tag)
        M, N, K = self.M, self.N, self.K
        if canaries:
            for name, g in self.outputs.items():
                assert g.untouched_outside(), "%s: cells outside the [%d, %d] window of %s were written" % (what, g.rows, g.cols, name)
        out = {}
        if self.pre is not None:
            out["preact"] = assert_excess(gemm_excess(self.pre.view, self.pre_ref, self.pre_S, K, self.dt), what + " preact")
        ref, S, extra = self.c_reference()
        out["C"] = assert_excess(gemm_excess(self.C.view, ref, S, K, self.out_dtype, extra), what + " C")
        stored = self.C.view.double()
        if self.part is not None:
            # Partial row r = the sum of the values of output rows 32 r .. 32 r + 31 (< M), fp32 additions: the fp32
            # summation bound with K = 32.  The kernel sums the fp32 values it is about to store; where C is bf16 the
            # stored value differs from each by the store's rounding, at most 2^-8 |v| <= 2^-8 (1 + 2^-7) |stored|.
            nblk = self.part.rows
            pad = torch.zeros((nblk * 32, N), dtype=torch.float64, device=stored.device)
            pad[:M] = stored
            blk, ablk = pad.view(nblk, 32, N).sum(1), pad.abs().view(nblk, 32, N).sum(1)
            rnd = (U_BF16 * (1 + 2.0 ** -7)) if self.out_dtype == BF16 else 0.0
            out["colsum partials"] = assert_excess(gemm_excess(self.part.view, blk, ablk, 32, F32, rnd * ablk),
                                                   what + " colsum partials")
        if self.colsum is not None:
            out["colsum"] = assert_excess(gemm_excess(self.colsum.view[0], 2.0 + stored.sum(0), 2.0 + stored.abs().sum(0), M,
                                                      F32, rnd * stored.abs().sum(0)), what + " colsum")
        if self.sq is not None:
            # slot (r, c) = the sum of squares of the stored fp32 block, clipped to the matrix: K = 4096 additions
            pad = torch.zeros((self.nr * 64, self.nc * 64), dtype=torch.float64, device=stored.device)
            pad[:M, :N] = stored
            sq = (pad * pad).view(self.nr, 64, self.nc, 64).sum((1, 3))
            out["norm slots"] = assert_excess(gemm_excess(self.sq.view.view(self.nr, self.nc), sq, sq, 4096, F32),
                                              what + " norm slots")
        if self.c8 is not None:
            # e4m3 copy of q * v: round-to-nearest of 3 mantissa bits (2^-4 |x|, 2^-10 below the normal range) on the fp32
            # value, which the stored bf16 value brackets within 2^-8
            x = stored * C8_QSCALE
            deq = self.c8.view.view(torch.float8_e4m3fn).float().double()
            bound = (2.0 ** -4 + 2.0 ** -8) * (1 + 2.0 ** -7) * x.abs() + 2.0 ** -10
            exc = (deq - x).abs() / bound
            out["e4m3 copy"] = assert_excess(torch.where(torch.isfinite(deq), exc, torch.full_like(exc, float("inf"))),
                                             what + " e4m3 copy")
        return out

    def snapshot(self):
        """bits of every output window (bit-identity across tiles); the norm slots separately (tile-dependent order)"""
        snap = {k: g.view.clone() for k, g in self.outputs.items() if k != "norm slots"}
        return snap, None if self.sq is None else self.sq.view.clone()


def matrix_cases(device, shapes=SHAPES, forms=FORMS, epilogues=None, seed=0):
    """every (shape, operand form, epilogue of that form)"""
    return [Case(M, N, K, form, epi, device, seed=seed)
            for (M, N, K) in shapes for form in forms for epi in (epilogues or FORM_EPILOGUES[form])]


def padded_cases(device, seed=0):
    """the padded-edge operands of pick_mode and the outputs that fail vec_ok:
    K = 100 with a row stride of 104 (`tail`: the chunk straddling K is zeroed on the way to LDS);
    N = 50 with ldc = 56 and with ldc = 50 (scalar stores inside the tuned kernels; ldc = 50 leaves room for rows only)"""
    cs = []
    for form, epi in (("11", "bias"), ("11", "gelu_pre"), ("10", "res"), ("01", "plain")):
        cs.append(Case(129, 136, 100, form, epi, device, seed=seed, a_ld=104 if form[0] == "1" else None,
                       b_ld=104 if form[1] == "1" else None))
    for ldc in (56, 50):
        for form, epi in (("11", "bias"), ("11", "gelu_pre"), ("11", "bias_res"), ("10", "acc"), ("00", "f32_acc_sqsum"),
                          ("11", "sigmoid_f32")):
            cs.append(Case(65, 50, 64, form, epi, device, seed=seed, ldc=ldc))
        cs.append(Case(129, 50, 100, "11", "tanh", device, seed=seed, ldc=ldc, a_ld=104, b_ld=104))
    return cs


E4M3_SHAPES = [(65, 72, 128), (129, 136, 256), (100, 264, 144)]  # K = 144: no whole 128-element k-tile, the register loop
E4M3_EPILOGUES = ("bias", "gelu_pre", "gelu_pre_c8", "bias_res", "bias_f32")


def e4m3_cases(device, epilogues=E4M3_EPILOGUES, seed=0):
    return [Case(M, N, K, "11", epi, device, seed=seed, fp8=True) for (M, N, K) in E4M3_SHAPES for epi in epilogues]
