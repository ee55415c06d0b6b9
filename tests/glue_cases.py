"""Shapes, inputs, fp64 references and per-element bounds of the element-wise glue kernels (csrc/elementwise.hip, the
element-wise ends of csrc/gat.hip, xggm_cast_f32_to_bf16 / xggm_dropout_mask of csrc/loss_optim.hip).

Importable without a GPU.  As in helpers.py / gemm_edge_cases.py every reference is an fp64 evaluation of the operands AS
STORED (bf16 inputs are rounded first and the reference consumes the rounded values), and every bound follows from the
arithmetic the kernel does -- u = 2^-24 per fp32 rounding, 2^-8 |ref| for a bf16 store and nothing else for it -- and is never
fitted to what a kernel returns.  ``R3`` = (1 + u)^3 - 1 and ``R2`` = (1 + u)^2 - 1 are the exact relative errors of three / two
chained roundings.  The fills and the casts are exact: their references are bit patterns.
"""
import numpy as np
import torch

from helpers import U32, U_BF16, bound_excess

F32, BF16 = torch.float32, torch.bfloat16
R2 = (1.0 + U32) ** 2 - 1.0
R3 = (1.0 + U32) ** 3 - 1.0

NT = 256
CAP, CAP_BIG = 2048 * NT, 4096 * NT               # threads of a capped grid: grid1d() / zero_ranges and cast_f32_to_bf16
FLAT_NS = (1, 3, 255, 257, 1027)                  # below a wave, one workgroup minus / plus one, four workgroups and a rest
N_PAST_CAP = CAP + 259                            # the second trip of the grid-stride loop, odd remainder
N_PAST_CAP_BIG = CAP_BIG + 259
N_CAST_FROM = tuple(4 * (CAP + 37) + r for r in range(4))   # float4 stride loop past the cap x every tail lane count
ELU_SHAPES = ((7, 5, 13, 3), (51, 24, 48, 24), (144, 32, 64, 32), (8200, 64, 128, 64))  # (M, D, ld, col0); the last: past the cap
ZERO_DIAG_B, ZERO_DIAG_NS = 3, (1, 4, 36, 100)
DROPOUT_PS = (0.5, 0.1)


def _store(bound, ref, dt):
    """+ 2^-8 |ref| for a bf16 store (round to nearest, no margin), nothing for fp32"""
    if dt == BF16:
        return bound + U_BF16 * ref.abs()
    if dt != F32:
        raise TypeError("glue bound: fp32 or bf16 outputs, got %s" % dt)
    return bound


def excess(got, ref, bound):
    """|got - ref| / bound per element on the CPU in fp64 (helpers.bound_excess: a zero bound admits only the exact value)"""
    return bound_excess(got.detach().double().cpu().reshape(ref.shape), ref, bound)


def bits(t):
    """the bit patterns of a tensor as integers (CPU)"""
    t = t.detach().cpu().contiguous()
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def same_bits(a, b):
    """equal bit patterns; two NaNs count as equal whatever their payload (no format fixes the payload of a NaN made by
    a conversion)"""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    ok = bits(a) == bits(b)
    if a.is_floating_point():
        ok = ok | (torch.isnan(a.detach().cpu()) & torch.isnan(b.detach().cpu()))
    return bool(ok.all())


def randn(n, seed, dt=F32, scale=1.0):
    """values as stored (CPU, ``dt``)"""
    return (torch.randn(n, generator=torch.Generator().manual_seed(seed)) * scale).to(dt)


def _plant(x, values):
    """``values`` at the front and, when there is room, again at the very end (the last lanes of the last trip)"""
    v = torch.tensor(values, dtype=torch.float64).to(x.dtype)
    k = min(len(v), x.numel())
    x.reshape(-1)[:k] = v[:k]
    if x.numel() >= 2 * len(v):
        x.reshape(-1)[-len(v):] = v
    return x


# ---------------------------------------------------------------------------------------------------- scale
# kernel: t = fl(1 + e); s' = fl(s * t); out = fl(s' * x): three fp32 roundings, each relative to its exact-operand
# result, so |out - s (1 + e) x| <= ((1 + u)^3 - 1) |ref| (one rounding without scale_ptr: covered).
def scale_ref(x, s, e, dt):
    """(ref, bound): ``s`` a python float exactly representable in fp32, ``e`` the fp32 device scalar's value or None"""
    assert float(np.float32(s)) == float(s)
    ref = float(s) * (1.0 + (0.0 if e is None else float(np.float32(e)))) * x.double()
    return ref, _store(R3 * ref.abs(), ref, dt)


# ---------------------------------------------------------------------------------------------------- sigmoid_bwd
# kernel: fl(fl(dy * y) * fl(1 - y)) on fp32 operands: three roundings, each relative (y is the exact operand of 1 - y,
# so the subtraction's error is u |1 - y| however close y is to 1).
SIGMOID_Y = (0.0, 1.0, 0.5, 2.0 ** -24, 1.0 - 2.0 ** -24, 0.996)


def sigmoid_inputs(n, seed):
    dy = randn(n, seed)
    y = _plant(torch.sigmoid(randn(n, seed + 1, scale=4.0)), SIGMOID_Y)
    return dy, y


def sigmoid_bwd_ref(dy, y, dt):
    d, s = dy.double(), y.double()
    ref = d * s * (1.0 - s)
    return ref, _store(R3 * ref.abs(), ref, dt)


# ---------------------------------------------------------------------------------------------------- tanh_bwd
# kernel: q = fl(t * t) (error u t^2); c = fl(1 - q) (error u |1 - q|); out = fl(dy * c).  The error of q passes through
# the subtraction UNCHANGED while 1 - t^2 shrinks: an absolute term |dy| u t^2 that no multiple of |ref| covers near
# |t| = 1.  |out - ref| <= (|dy| u t^2 + 2 u |ref|) (1 + 4 u).  (A fused 1 - t * t rounds once: smaller.)
TANH_T = (0.996, -0.996, 1.0 - 2.0 ** -8, -(1.0 - 2.0 ** -8), 1.0, -1.0, 0.0, 0.5)


def tanh_inputs(n, seed, dt):
    dy = randn(n, seed, dt)
    t = _plant(torch.tanh(randn(n, seed + 1, scale=2.0)).to(dt), TANH_T)
    return dy, t


def tanh_bwd_ref(dy, t, dt):
    d, s = dy.double(), t.double()
    ref = d * (1.0 - s * s)
    return ref, _store((d.abs() * U32 * s * s + 2.0 * U32 * ref.abs()) * (1.0 + 4.0 * U32), ref, dt)


# ---------------------------------------------------------------------------------------------------- elu
# forward: x if x > 0 (a copy: exact) else expm1f(x): the term helpers.py gives an activation evaluated in fp32,
# 4 * 2^-24 * (1 + |f|).  backward, written in the OUTPUT y: g if y > 0 (exact) else fl(g * fl(y + 1)): two roundings.
ELU_EDGES = (0.0, -2.0 ** -126, -2.0 ** -30, -1.0 + 2.0 ** -8, 2.0 ** -30, -20.0, 3.0)  # exactly 0; just below; y + 1 = 2^-8


def elu_inputs(M, D, seed, dt):
    return _plant(randn(M * D, seed, dt, scale=2.0), ELU_EDGES).view(M, D)


def elu_fwd_ref(x, dt):
    v = x.double()
    ref = torch.where(v > 0, v, torch.expm1(v))
    return ref, _store(torch.where(v > 0, torch.zeros_like(v), 4.0 * U32 * (1.0 + ref.abs())), ref, dt)


def elu_bwd_ref(g, y, dt):
    d, v = g.double(), y.double()
    ref = torch.where(v > 0, d, d * (v + 1.0))
    return ref, _store(torch.where(v > 0, torch.zeros_like(v), R2 * ref.abs()), ref, dt)


# ---------------------------------------------------------------------------------------------------- dropout
# mask: philox_uniform(seed, offset, sid, i) >= p ? 1 / (1 - p) : 0 with p and the quotient in fp32 -- exact, bit patterns.
# product: fl(x * keep), one rounding against the fp32 keep; against the reference's 1 / (1 - p) the keep itself carries
# two more (fl(1 - p), fl(1 / .)): three in all.  p = 0.5 makes keep = 2 and everything exact.
def dropout_mask_host(n, p, seed, offset, sid):
    """the fp32 mask [n] (CPU) by the host restatement of common.h's generator"""
    from pretrain_mask_ref import philox_uniform
    p32 = np.float32(p)
    ik = np.float32(1.0) / (np.float32(1.0) - p32)
    u = philox_uniform(int(seed), int(offset), int(sid), int(n))
    return torch.from_numpy(np.where(u >= p32, ik, np.float32(0.0)).astype(np.float32))


def dropout_ref(x, mask, p, dt):
    """(ref, bound): ``mask`` the fp32 host mask; the reference scales the kept elements by the real 1 / (1 - p)"""
    keep = (mask != 0).double() / (1.0 - float(np.float32(p)))
    ref = x.double() * keep
    return ref, _store(R3 * ref.abs(), ref, dt)


# ---------------------------------------------------------------------------------------------------- exact: fills
def fill_pattern(n):
    """n non-zero, pairwise different fp32 values (a fill that moves data instead of zeroing it is seen too)"""
    return torch.arange(1, n + 1, dtype=torch.float64).mul_(0.25).to(F32)


def zero_ranges_ref(buf, ranges):
    out = buf.clone()
    for s, e in ranges:
        out[s:e] = 0.0
    return out


def zero_ranges_rows_ref(buf, ranges, t0, R, H, ids, n):
    """ranges as above plus rows ids[:min(n, len(ids))] of the [R, H] table at element ``t0``; ids outside [0, R) skipped"""
    out = zero_ranges_ref(buf, ranges)
    for r in ids[:max(0, min(int(n), len(ids)))]:
        r = int(r)
        if 0 <= r < R:
            out[t0 + r * H:t0 + (r + 1) * H] = 0.0
    return out


def range_cases():
    """name -> (buffer length, [(start, end)]) of the small xggm_zero_ranges_f32 cases (the wrapper drops empty ranges)"""
    def run(k):
        rs, o = [], 4
        for i in range(k):
            ln = 4 * (1 + i % 3)
            rs.append((o, o + ln))
            o += ln + 4                   # a gap of four floats that must survive
        return o + 4, rs
    return {"one4": (24, [(8, 12)]), "sixteen": run(16), "seventeen": run(17)}


BIG_RANGE = 4 * (CAP_BIG + 37)            # floats of the one range past the cap (16.8 MB)
ROWS_R, ROWS_H, ROWS_H_WIDE, ROWS_CAP = 37, 12, 1028, 64


def row_ids(R, cap, seed):
    """[cap] ids with duplicates, -1 and R among them; entries 40.. name rows 30..R-1 ONLY (a kernel that ignores the
    count zeroes those rows), entries below 40 never do"""
    g = torch.Generator().manual_seed(seed)
    hi = min(30, R)
    ids = torch.randint(0, hi, (cap,), generator=g, dtype=torch.int64)
    ids[1], ids[2], ids[5], ids[7] = ids[0], -1, R, ids[0]
    if R > 30:
        ids[40:] = torch.randint(30, R, (cap - 40,), generator=g, dtype=torch.int64)
    return ids


# ---------------------------------------------------------------------------------------------------- exact: zero_diag, masks, sums
def zero_diag_input(B, N, seed):
    """[B, N, N] fp32 whose DIAGONAL ONLY holds NaN and +-inf (in turn): they must not survive or spread"""
    a = randn(B * N * N, seed).view(B, N, N).clone()
    bad = torch.tensor([float("nan"), float("inf"), -float("inf")])
    for b in range(B):
        for i in range(N):
            a[b, i, i] = bad[(b + i) % 3]
    return a


def zero_diag_ref(adj):
    out = adj.clone()
    for i in range(adj.shape[-1]):
        out[:, i, i] = 0.0
    return out


def additive_mask_ref(mask):
    """fp32, as the kernel: (1 - (float) m) * -10000"""
    m = mask.numpy().astype(np.float32)
    return torch.from_numpy(((np.float32(1.0) - m) * np.float32(-10000.0)).astype(np.float32))


def add_scalars_ref(vals):
    """fp32 sum left to right"""
    acc = np.float32(vals[0])
    for v in vals[1:]:
        acc = np.float32(acc + np.float32(v))
    return acc


SCALAR_TERMS = (1.0e8, 1.0, -1.0e8, 0.5)  # left to right in fp32: 0.5; any other order or a wider accumulator: 1.5


# ---------------------------------------------------------------------------------------------------- exact: casts
# the patterns of tests/test_resident_gpu.py::_tables, plus -inf and the canonical NaN
CAST_SPECIAL = np.array([0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000,  # ties: to even (down), to even (up), negative
                         0x3F808001, 0x3F807FFF,                          # just above / below a tie
                         0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F8000, 0x7F7F7FFF,  # round up to +-inf; the tie; the largest survivor
                         0x7F800000, 0xFF800000, 0x7FC00000,              # +-inf, NaN
                         0x00000001, 0x80000001, 0x00008000, 0x00018000, 0x007FFFFF, 0x807FFFFF,  # denormals
                         0x00000000, 0x80000000], dtype=np.uint32)


def cast_input(n, seed):
    """[n] fp32 with the special patterns at the front and (n permitting) in the last elements: the tail lanes"""
    x = randn(n, seed).numpy().copy()
    sp = CAST_SPECIAL.view(np.float32)
    k = min(len(sp), n)
    x[:k] = sp[:k]
    if n >= 2 * len(sp):
        x[-len(sp):] = sp
    elif n > 4:
        x[-4:] = sp[:4]  # ties in the tail of a short input
    return torch.from_numpy(x)


def bf16_rne_ref(x):
    """fp32 -> bf16 by round to nearest even on the bit pattern, independent of torch's conversion (NaN -> 0x7FC0)"""
    u = x.detach().cpu().contiguous().numpy().view(np.uint32).astype(np.uint64)
    r = ((u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)) & np.uint64(0xFFFF)
    nan = ((u & np.uint64(0x7F800000)) == np.uint64(0x7F800000)) & ((u & np.uint64(0x007FFFFF)) != 0)
    r = np.where(nan, np.uint64(0x7FC0), r).astype(np.uint16)
    return torch.from_numpy(r.view(np.int16).copy()).view(BF16).reshape(x.shape)
