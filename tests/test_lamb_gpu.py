"""``BertLamb`` on the device: ``ops.lamb_multi`` against an fp64 restatement of the step, bit equalities, the golden
trajectory, and the optimiser over the tiny 2/2/1 model.

Every kernel-level case runs on a ``Bed``: flat buffers whose spans lie between NaN moats (nothing outside a span may be
written, and nothing read from there may reach a result) and whose alignment gaps between tensors hold a sentinel band in
m and v -- the update owns the tensors' elements and nothing else.

Bounds.  p, m, v: with ``ref64`` / ``ref32`` the restatement below stepping in fp64 / fp32 on the same clipped gradients,
max|x_gpu - ref64| <= 4 * max|ref32 - ref64| + ulp32(max|x|), the bound of test_optim_gpu.test_rule_matches_torch_over_*.
The restatement works on the kernel's INPUTS: fp32 weights and gradients, and b1, b2, eps, weight_decay as the floats of
``xggm_adam_args`` hold them (1 - 0.999f is 1.3e-5 below 0.001; BertAdam's rule has always formed it so, and a ratio of 1
has to give BertAdam's bits).
Trust ratios: 1e-6 relative against the fp64 restatement -- every u is within two fp32 ulp (1.2e-7) of the restatement's
and the double sums add nothing of that order.  Nothing is calibrated on the code under test."""
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from xggm_amd import synth  # noqa: E402,F401
from test_optim_gpu import MAX_NORM, clip_coef, ratio_of, _tiny, _batch, _backward, _arena_equal  # noqa: E402

DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
CH = 2048  # XGGM_LAMB_CHUNK: what one workgroup sums
HP = dict(lr=1e-2, b1=0.9, b2=0.999, e=1e-6, weight_decay=0.01)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lamb.npz")

# 1, 7, 8, 9, 24: the n & 3 tail alone, a float4 and a tail, two float4, two and a tail, six; exactly a chunk and a chunk
# plus one element; 2 * 2048 + 9 elements from an offset that is no multiple of 2048: three chunks over four workgroups'
# ranges; an all-zero tensor; a tensor that is not adapted; a last short one
LENGTHS = [1, 7, 8, 9, 24, CH + 1, CH, 2 * CH + 9, 300, 130, 5]
ZERO, PLAIN = 8, 9
SPANS9 = [[0, 1], [2], [3], [4], [5], [6], [7], [8, 9], [10]]  # nine spans: one launch takes 8


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


# ------------------------------------------------------------------------------------------------------------------ the bed
class Bed:
    """tensors at 8-aligned offsets, grouped into spans; NaN moats in front of, between and behind the spans"""
    MOAT, BAND = 72, 7.0

    def __init__(self, lengths, spans=None, gdtype=F32, adapted=None, band=True, first=None):
        self.lengths = list(lengths)
        spans = spans or [list(range(len(lengths)))]
        self.off, self.span = [0] * len(lengths), []
        o = self.MOAT if first is None else first
        for members in spans:
            s0 = o
            for i in members:
                self.off[i] = o
                o = (o + lengths[i] + 7) // 8 * 8
                if lengths[i] % 8 == 0:
                    o += 8  # a gap behind every tensor
            self.span.append((s0, o))
            o += 16
        self.total = o + self.MOAT
        nan = float("nan")
        self.p = torch.full((self.total,), nan, device=DEV)
        self.m = torch.full((self.total,), nan, device=DEV)
        self.v = torch.full((self.total,), nan, device=DEV)
        self.g = torch.full((self.total,), nan, device=DEV, dtype=gdtype)
        self.shadow = torch.full((self.total,), nan, device=DEV, dtype=BF16)
        for a, b in self.span:  # inside a span: zeros, as an arena holds them -- with a band in the gaps' moments
            for buf in (self.p, self.g, self.shadow):
                buf[a:b] = 0
            self.m[a:b] = self.BAND if band else 0.0
            self.v[a:b] = self.BAND if band else 0.0
        for buf in (self.m, self.v):
            for x in self.views(buf):
                x.zero_()
        self.adapted = [True] * len(lengths) if adapted is None else list(adapted)
        order = sorted(range(len(lengths)), key=lambda i: self.off[i])
        self.row = {i: r for r, i in enumerate(order)}
        self.table = torch.tensor([[self.off[i], lengths[i], int(self.adapted[i])] for i in order], dtype=torch.int64, device=DEV)
        self.ratios = torch.full((len(lengths),), -1.0, device=DEV)
        from xggm_amd import ops
        self.ws = ops.lamb_workspace(self.total, len(lengths), DEV)
        self.ws.fill_(nan)
        self.steps = torch.zeros(1, device=DEV, dtype=torch.int64)
        self.lr_scale = torch.ones(1, device=DEV)
        self.sq = torch.zeros(1, device=DEV)
        self.outside = torch.ones(self.total, dtype=torch.bool, device=DEV)
        for o_, n in zip(self.off, self.lengths):
            self.outside[o_:o_ + n] = False
        self.frozen = None

    def views(self, buf):
        return [buf[o:o + n] for o, n in zip(self.off, self.lengths)]

    def fill(self, buf, tensors):
        for x, t in zip(self.views(buf), tensors):
            x.copy_(t)

    def jobs(self, hp, clip, g_scale, lr_dev=None):
        out = []
        for a, b in self.span:
            sl = slice(a, b)
            out.append(((self.p[sl], self.g[sl], self.m[sl], self.v[sl], self.shadow[sl], self.sq if clip else None, MAX_NORM,
                         hp["lr"], self.lr_scale, hp["b1"], hp["b2"], hp["e"], hp["weight_decay"]),
                        dict(elem0=a, g_scale=g_scale, lr_dev=lr_dev), {}))
        return out

    def snapshot_outside(self):
        self.frozen = [buf.clone() for buf in (self.p, self.m, self.v, self.shadow)]

    def check_outside(self):
        """moats, gaps and bands: every bit that belongs to no tensor is the bit it was"""
        for buf, old in zip((self.p, self.m, self.v, self.shadow), self.frozen):
            w = torch.int32 if buf.dtype == F32 else torch.int16
            assert torch.equal(buf.view(w)[self.outside], old.view(w)[self.outside])

    def step(self, hp=HP, clip=True, g_scale=1.0, hyper_map=None, t_total=-1, warmup=0.0, lr_dev=None):
        from xggm_amd import ops
        if self.frozen is None:
            self.snapshot_outside()
        ops.sched_step_ex(self.steps, self.lr_scale, None, [(0, t_total, warmup, "warmup_linear", 0.0, 0.0)])
        ops.lamb_multi(self.jobs(hp, clip, g_scale, lr_dev), self.table, self.ratios, self.ws, hyper_map=hyper_map)
        self.check_outside()

    def ratio_list(self):
        r = self.ratios.tolist()
        return [r[self.row[i]] for i in range(len(self.lengths))]

    def id_map(self, ids):
        """uint8 per 8 elements: ``ids[i]`` over tensor i and the gap behind it, 0 elsewhere"""
        m = torch.zeros((self.total + 7) // 8, dtype=torch.uint8)
        for o, n, i in zip(self.off, self.lengths, ids):
            m[o // 8:(o + n + 7) // 8] = i
        return m.to(DEV)


def grads_of(lengths, step, bf16_exact=False, seed=1000):
    """N(0, 1) with a sprinkling of exact zeros; the odd steps scaled so that the clip at 5 is not active"""
    gen = torch.Generator().manual_seed(seed + step)
    out = []
    for n in lengths:
        g = torch.randn(n, generator=gen)
        g[torch.rand(n, generator=gen) < 0.05] = 0.0
        if step % 2:
            g *= 0.01
        out.append(g.to(BF16).float() if bf16_exact else g)
    return out


def start_of(lengths, seed=7):
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn(n, generator=gen) for n in lengths]


def restate(dt, p, g, m, v, lr, wd, adapted, hp=HP):
    """the issue's step of one tensor, in torch on the CPU in ``dt`` -> (p, m, v, ratio): the reference of the bounds.  In
    fp64 the norms are plain fp64 norms; in fp32 everything, the norms too, is torch's fp32."""
    f32 = lambda x: float(np.float32(x))  # noqa: E731
    b1, b2, e, wd = f32(hp["b1"]), f32(hp["b2"]), f32(hp["e"]), f32(wd)  # the values the C ABI's floats hold, taken exactly
    g = g.to(dt)
    m = m * b1 + (1 - b1) * g
    v = v * b2 + (1 - b2) * g * g
    u = m / (v.sqrt() + e)
    if wd > 0.0:
        u = u + wd * p
    np_, nu = float(torch.linalg.vector_norm(p)), float(torch.linalg.vector_norm(u))
    r = np_ / nu if (adapted and np_ > 0.0 and nu > 0.0) else 1.0
    return p - (lr * r) * u, m, v, r


class Refs:
    """the fp64 and the fp32 restatement side by side over all tensors of a bed"""

    def __init__(self, p0, lrs, wds, adapted):
        self.lrs, self.wds, self.adapted = lrs, wds, adapted
        self.state = {dt: ([t.to(dt).clone() for t in p0], [torch.zeros_like(t, dtype=dt) for t in p0],
                           [torch.zeros_like(t, dtype=dt) for t in p0]) for dt in (torch.float64, F32)}
        self.r = []

    def step(self, gs, coef, lr_scale=1.0, skip=()):
        self.r = [1.0] * len(gs)
        for dt, (P, M, V) in self.state.items():
            for i, g in enumerate(gs):
                if i in skip:
                    continue
                gk = (g * float(coef)).to(F32)  # the fp32 product the kernel forms, for both references
                P[i], M[i], V[i], r = restate(dt, P[i], gk, M[i], V[i], self.lrs[i] * lr_scale, self.wds[i], self.adapted[i])
                if dt == torch.float64:
                    self.r[i] = r

    def check(self, bed, tag, skip=()):
        keep = [i for i in range(len(bed.lengths)) if i not in skip]
        rs = {}
        for k, name in enumerate(("p", "m", "v")):
            x = [bed.views(getattr(bed, name))[i] for i in keep]
            rs[name] = ratio_of(x, [self.state[torch.float64][k][i] for i in keep], [self.state[F32][k][i] for i in keep])
        got = bed.ratio_list()
        worst = max(abs(got[i] - self.r[i]) / self.r[i] for i in keep)
        print("%s: error / bound %s; trust ratios: worst relative error %.2e" % (tag, {k: round(v, 3) for k, v in rs.items()}, worst))
        assert all(v <= 1.0 for v in rs.values()), (tag, rs)
        assert worst <= 1e-6, (tag, worst, got, self.r)
        assert torch.equal(bed.shadow[~bed.outside], bed.p[~bed.outside].to(BF16))  # the shadow is the bf16 of the new masters


def clip_of(gs):
    sq = np.float32(sum(float(g.double().pow(2).sum()) for g in gs))
    return float(sq), clip_coef(sq)


# ---------------------------------------------------------------------------------------------------- against the restatement
@pytest.mark.parametrize("gdtype", [F32, BF16], ids=["g32", "g16"])
@pytest.mark.parametrize("mapped", [False, True], ids=["nomap", "map"])
def test_nine_spans_match_the_restatement(gdtype, mapped):
    """every tensor length of the list, nine spans (two launches of each phase), six steps with the clip active on the even
    ones, g_scale = 1/2 with bf16 gradients; with the map: two param_groups {lr, wd} / {lr / 2, 0} per tensor, one tensor
    in no group (every bit of it stays), and an id the table does not hold"""
    n = len(LENGTHS)
    adapted = [i != PLAIN for i in range(n)]
    bed = Bed(LENGTHS, SPANS9, gdtype=gdtype, adapted=adapted)
    p0 = start_of(LENGTHS)
    p0[ZERO].zero_()
    bed.fill(bed.p, p0)
    bed.fill(bed.shadow, [t.to(BF16) for t in p0])
    g_scale = 0.5 if gdtype == BF16 else 1.0
    ids = [1, 2, 1, 2, 1, 1, 2, 1, 1, 2, 3] if mapped else [1] * n
    out = 2  # with the map: the 8-element tensor is in no param_group -> id 0; the last tensor's id 3 is not in the table
    hyper_map, skip = None, ()
    if mapped:
        ids[out] = 0
        table = torch.tensor([[0.0, 0.0], [HP["lr"], HP["weight_decay"]], [0.5 * HP["lr"], 0.0]], device=DEV)
        hyper_map, skip = (bed.id_map(ids), table), (out, n - 1)
        for k in skip:  # sentinels in what must not be touched
            bed.views(bed.m)[k].fill_(3.0)
            bed.views(bed.v)[k].fill_(4.0)
    lrs = [HP["lr"] * (0.5 if i == 2 else 1.0) for i in ids]
    wds = [0.0 if i == 2 else HP["weight_decay"] for i in ids]
    refs = Refs(p0, lrs, wds, adapted)
    hp = dict(HP, lr=123.0, weight_decay=55.0) if mapped else HP  # (with a map the spans' own are not read)
    for s in range(6):
        gs = grads_of(LENGTHS, s, bf16_exact=gdtype == BF16)
        gs[ZERO].zero_()
        sq, coef = clip_of(gs)
        assert (coef < 1.0) == (s % 2 == 0)
        bed.sq.fill_(sq)
        bed.fill(bed.g, gs)
        bed.step(hp, clip=True, g_scale=g_scale, hyper_map=hyper_map)
        refs.step(gs, np.float32(coef) * np.float32(g_scale), skip=skip)
        refs.check(bed, "step %d" % s, skip=skip)
        got = bed.ratio_list()
        assert got[ZERO] == 1.0 and got[PLAIN] == 1.0
        assert float(bed.views(bed.p)[ZERO].abs().max()) == 0.0 and float(bed.views(bed.m)[ZERO].abs().max()) == 0.0
        if mapped:
            for k in skip:
                assert got[k] == 1.0 and torch.equal(bed.views(bed.p)[k], p0[k].to(DEV))
                assert bool((bed.views(bed.m)[k] == 3.0).all()) and bool((bed.views(bed.v)[k] == 4.0).all())
                assert torch.equal(bed.views(bed.shadow)[k], p0[k].to(BF16).to(DEV))
    live = [r for i, r in enumerate(bed.ratio_list()) if i not in (ZERO, PLAIN) + tuple(skip)]
    assert all(abs(r - 1.0) > 1e-3 for r in live)  # the ratios are no accident of 1
    assert int(bed.steps[0]) == 6


def test_clip_inactive_without_a_norm_and_lr_from_the_device():
    """no sqnorm pointer (no clip), lr from a device scalar, a warm-up schedule value: one step against the restatement"""
    lengths = [9, CH + 1, 24]
    bed = Bed(lengths)
    p0 = start_of(lengths)
    bed.fill(bed.p, p0)
    gs = grads_of(lengths, 0)
    bed.fill(bed.g, gs)
    lr_dev = torch.tensor([HP["lr"]], device=DEV)
    bed.steps.fill_(3)
    bed.step(dict(HP, lr=99.0), clip=False, lr_dev=lr_dev, t_total=10, warmup=0.5)  # schedule value 0.3 / 0.5
    assert abs(float(bed.lr_scale[0]) - 0.6) < 1e-6
    refs = Refs(p0, [HP["lr"]] * 3, [HP["weight_decay"]] * 3, [True] * 3)
    refs.step(gs, 1.0, lr_scale=0.6)
    refs.check(bed, "no clip")


# -------------------------------------------------------------------------------------------------------- degenerate ratios
def test_degenerate_ratios():
    """an all-zero tensor: r = 1, every value stays +0.  A zero gradient at the first step with weight_decay 0: u = 0,
    r = 1, p keeps its bits, m and v stay 0.  A tensor that is not adapted between adapted ones: r = 1 for it alone, and its
    bits are BertAdam's."""
    from xggm_amd import ops
    lengths = [300, CH + 9, 40, 130, 24]
    bed = Bed(lengths, adapted=[True, True, True, False, True], band=False)
    twin = Bed(lengths, band=False)  # BertAdam on the same values (gaps hold zeros there, as in an arena)
    p0 = start_of(lengths)
    p0[0].zero_()
    gs = grads_of(lengths, 1)
    gs[0].zero_()
    gs[2].zero_()
    ids = bed.id_map([1, 1, 2, 1, 1])
    table = torch.tensor([[0.0, 0.0], [HP["lr"], HP["weight_decay"]], [HP["lr"], 0.0]], device=DEV)
    for b in (bed, twin):
        b.fill(b.p, p0)
        b.fill(b.g, gs)
    bed.step(clip=False, hyper_map=(ids, table))
    ops.optim_multi("bertadam", twin.jobs(HP, False, 1.0), hyper_map=(ids, table))
    r = bed.ratio_list()
    assert r[0] == 1.0 and r[2] == 1.0 and r[3] == 1.0 and abs(r[1] - 1.0) > 1e-3 and abs(r[4] - 1.0) > 1e-3
    for name in ("p", "m", "v", "shadow"):
        x = bed.views(getattr(bed, name))
        w = torch.int32 if x[0].dtype == F32 else torch.int16
        assert int(x[0].view(w).abs().max()) == 0, name  # +0 everywhere: not even a sign bit
        assert torch.equal(x[3], twin.views(getattr(twin, name))[3]), name
    assert torch.equal(bed.views(bed.p)[2], p0[2].to(DEV))
    assert float(bed.views(bed.m)[2].abs().max()) == 0.0 and float(bed.views(bed.v)[2].abs().max()) == 0.0
    assert not torch.equal(bed.views(bed.p)[1], twin.views(twin.p)[1])  # an adapted neighbour does move differently


# ------------------------------------------------------------------------------------------------------------- bit equality
@pytest.mark.parametrize("gdtype", [F32, BF16], ids=["g32", "g16"])
@pytest.mark.parametrize("mapped", [False, True], ids=["nomap", "map"])
def test_nothing_adapted_is_bertadam_bit_for_bit(gdtype, mapped):
    """every tensor not adapted: p, m, v and the shadow are those of xggm_optim_multi's BertAdam rule over the same spans,
    three steps, with the clip, g_scale and a schedule value -- moats and (zero) gaps included"""
    from xggm_amd import ops
    n = len(LENGTHS)
    beds = [Bed(LENGTHS, SPANS9, gdtype=gdtype, adapted=[False] * n, band=False) for _ in range(2)]
    p0 = start_of(LENGTHS)
    hyper_map = None
    if mapped:
        ids = [1, 2, 0, 2, 1, 1, 2, 1, 1, 2, 1]
        table = torch.tensor([[0.0, 0.0], [HP["lr"], HP["weight_decay"]], [0.5 * HP["lr"], 0.0]], device=DEV)
        hyper_map = (beds[0].id_map(ids), table)
    for b in beds:
        b.fill(b.p, p0)
        b.fill(b.shadow, [t.to(BF16) for t in p0])
    for s in range(3):
        gs = grads_of(LENGTHS, s, bf16_exact=gdtype == BF16)
        sq, _ = clip_of(gs)
        for b in beds:
            b.sq.fill_(sq)
            b.fill(b.g, gs)
        beds[0].step(clip=True, g_scale=0.5, hyper_map=hyper_map, t_total=10, warmup=0.3)
        ops.sched_step_ex(beds[1].steps, beds[1].lr_scale, None, [(0, 10, 0.3, "warmup_linear", 0.0, 0.0)])
        ops.optim_multi("bertadam", beds[1].jobs(HP, True, 0.5), hyper_map=hyper_map)
        for name in ("p", "m", "v", "shadow"):
            x, y = getattr(beds[0], name), getattr(beds[1], name)
            w = torch.int32 if x.dtype == F32 else torch.int16
            assert torch.equal(x.view(w), y.view(w)), (s, name)
        assert all(r == 1.0 for r in beds[0].ratio_list())
    assert float(beds[0].lr_scale[0]) > 0 and not torch.equal(beds[0].views(beds[0].p)[5], p0[5].to(DEV))


def test_two_launches_give_the_same_bits():
    beds = [Bed(LENGTHS, SPANS9) for _ in range(2)]
    p0 = start_of(LENGTHS)
    for s in range(2):
        gs = grads_of(LENGTHS, s)
        sq, _ = clip_of(gs)
        for b in beds:
            if s == 0:
                b.fill(b.p, p0)
            b.sq.fill_(sq)
            b.fill(b.g, gs)
            b.step()
    for name in ("p", "m", "v", "shadow", "ratios"):
        x, y = getattr(beds[0], name), getattr(beds[1], name)
        w = torch.int16 if x.dtype == BF16 else torch.int32
        assert torch.equal(x.view(w), y.view(w)), name


def test_a_ratio_depends_on_its_tensor_alone():
    """the same tensors (values and lengths) (a) all in one pass, (b) with their neighbours in no param_group, (c) alone in
    spans of their own at other offsets -- other ranges, other workgroups, other slots: the ratios of the tensors that take
    part are the same bits, and so are their p, m, v"""
    lengths = [2 * CH + 9, 24, CH + 1, 7]
    p0, gs = start_of(lengths), grads_of(lengths, 1)
    table = torch.tensor([[0.0, 0.0], [HP["lr"], HP["weight_decay"]]], device=DEV)
    a = Bed(lengths)
    b = Bed(lengths)
    c = Bed(lengths, [[3], [2], [1], [0]], first=8 * 131)
    runs = []
    for bed, ids in ((a, [1, 1, 1, 1]), (b, [1, 0, 1, 0]), (c, [1, 1, 1, 1])):
        bed.fill(bed.p, p0)
        bed.fill(bed.g, gs)
        bed.step(clip=False, hyper_map=(bed.id_map(ids), table))
        runs.append((bed.ratios.clone(), bed))
    assert a.off != c.off
    for k in (0, 2):
        ra, rb, rc = (float(bed.ratio_list()[k]) for _, bed in runs)
        assert ra == rb == rc and abs(ra - 1.0) > 1e-3, (k, ra, rb, rc)
        for name in ("p", "m", "v"):
            assert torch.equal(a.views(getattr(a, name))[k], b.views(getattr(b, name))[k])
            assert torch.equal(a.views(getattr(a, name))[k], c.views(getattr(c, name))[k])
    assert a.ratio_list()[1] == c.ratio_list()[1] and b.ratio_list()[1] == 1.0


# ---------------------------------------------------------------------------------------------------------- golden trajectory
def test_golden_trajectory():
    """the six steps of tests/golden/lamb.npz (the reference's defaults and warm-up schedule, fp64) through the kernels: a
    mapped launch, the not-adapted tensor in a param_group without weight decay.  The first step has lr 0: p keeps its bits."""
    g = np.load(GOLDEN)
    lengths = g["lengths"].tolist()
    off = np.concatenate([[0], np.cumsum(lengths)])
    cut = lambda x: [torch.from_numpy(np.ascontiguousarray(x[a:b])) for a, b in zip(off[:-1], off[1:])]  # noqa: E731
    lr0, b1, b2, e, warmup, t_total = g["hyper"].tolist()
    hp = dict(lr=lr0, b1=b1, b2=b2, e=e, weight_decay=0.01)
    adapted, wds = g["adapted"].tolist(), g["weight_decay"].tolist()
    bed = Bed(lengths, [[0, 1, 2, 3, 4], [5, 6, 7, 8]], adapted=adapted)
    p0 = cut(g["p0"])
    bed.fill(bed.p, p0)
    table = torch.tensor([[0.0, 0.0], [lr0, max(wds)], [lr0, 0.0]], device=DEV)
    hyper_map = (bed.id_map([2 if w == 0.0 else 1 for w in wds]), table)
    ref32 = ([t.clone() for t in p0], [torch.zeros_like(t) for t in p0], [torch.zeros_like(t) for t in p0])
    from xggm_amd.lxrt.optimization import SCHEDULES
    for s in range(g["grads"].shape[0]):
        gs = cut(g["grads"][s])
        bed.fill(bed.g, gs)
        bed.step(hp, clip=False, hyper_map=hyper_map, t_total=int(t_total), warmup=warmup)
        lr = lr0 * SCHEDULES["warmup_linear"](s / t_total, warmup)
        for i, gi in enumerate(gs):
            ref32[0][i], ref32[1][i], ref32[2][i], _ = restate(F32, ref32[0][i], gi, ref32[1][i], ref32[2][i], lr, wds[i],
                                                               adapted[i], hp)
        got = np.array(bed.ratio_list())
        worst = float(np.abs(got / g["ratios"][s] - 1.0).max())
        print("golden step %d: trust ratios, worst relative error %.2e" % (s, worst))
        assert worst <= 1e-6, (s, got, g["ratios"][s])
        if s == 0:
            assert all(torch.equal(x.cpu(), t) for x, t in zip(bed.views(bed.p), p0))
            assert ratio_of(bed.views(bed.m), cut(g["m_first"]), ref32[1]) <= 1.0
    rs = {k: ratio_of(bed.views(getattr(bed, k)), cut(g[k + "_last"]), ref32[j]) for j, k in enumerate(("p", "m", "v"))}
    print("golden, after six steps: error / bound %s" % {k: round(v, 3) for k, v in rs.items()})
    assert all(v <= 1.0 for v in rs.values()), rs


# ---------------------------------------------------------------------------------------------------------------- model level
def _lamb(m, lr=1e-3, **kw):
    """the BERT recipe over the tiny model: biases and LayerNorm weights neither decayed nor adapted"""
    from xggm_amd.lxrt.optimization import BertLamb
    from xggm_amd.vqa.vqacpv2 import NO_DECAY
    nd = lambda n: any(s in n for s in NO_DECAY)  # noqa: E731
    groups = [{"params": [p for n, p in m.named_parameters() if not nd(n)]},
              {"params": [p for n, p in m.named_parameters() if nd(n)], "weight_decay": 0.0, "layer_adaptation": False}]
    return BertLamb(groups, lr=lr, split_groups=True, **kw)


def _iteration(m, o, b, kinds=("plain", "rel")):
    from xggm_amd.runtime import runtime_of
    from xggm_amd.vqa.vqacpv2 import plain_pass, ggm_pass, BCEWithLogitsLoss
    sent = (b["input_ids"], b["input_mask"], b["segment_ids"])
    rt, bce, out = runtime_of(m), BCEWithLogitsLoss(), []
    for kind in kinds:
        if kind == "plain":
            out.append(plain_pass(m, o, bce, b["feats"], b["boxes"], sent, b["target"])[0])
        else:
            out.append(ggm_pass(m, o, bce, b["feats"], b["boxes"], sent, b["target"], b["adj_true"], kind, 1.0, 8.0)[0])
        rt.advance()
    return [float(x) for x in out]


def test_captured_equals_eager_bf16():
    """four iterations under CapturedTrainer (the constructor's eager warm-up one and three replays) equal four eager ones:
    parameters, moments, shadows, step counters and the ratio table, bit for bit"""
    from xggm_amd.engine import CapturedTrainer
    from xggm_amd.runtime import runtime_of
    from xggm_amd.vqa.vqacpv2 import NO_DECAY, make_optimizer
    mk = lambda mm: make_optimizer(mm, 1e-3, 40, optim="bertlamb", no_decay=NO_DECAY)  # noqa: E731
    cfg, m1, o1 = _tiny(5, 11, mk)
    _, m2, o2 = _tiny(5, 11, mk)
    assert type(o1).__name__ == "BertLamb"
    batches = [_batch(cfg, s) for s in (3, 4)]
    branches = ["rel", "node", "rel"]
    tr = CapturedTrainer(m1, o1, batches[0], sigma=1.0, warmup_iters=1)
    for i, br in enumerate(branches):
        tr.load_batch(batches[i % 2])
        tr.iteration(br)
    m2.train()
    _iteration(m2, o2, batches[0], ("plain", "rel", "node"))  # the constructor's warm-up iteration
    for i, br in enumerate(branches):
        _iteration(m2, o2, batches[i % 2], ("plain", br))
    _arena_equal(m1, m2)
    r1, r2 = o1.trust_ratios(), o2.trust_ratios()
    assert r1 == r2 and len(r1) == len(list(m1.parameters()))
    assert all(r == 1.0 for n, r in r1.items() if any(s in n for s in NO_DECAY))
    moving = [r for n, r in r1.items() if n.endswith("dense.weight")]
    assert moving and all(math.isfinite(r) and r > 0 and r != 1.0 for r in moving)
    assert min(runtime_of(m1).arena.steps.tolist()) >= 2


def test_step_over_the_models_gradients_matches_the_restatement():
    """one backward on the GPU; from ITS gradients (read back) the restatement gives every tensor's new weights and ratio:
    BertLamb.step agrees within the bound of the module docstring, tensor by tensor"""
    from xggm_amd.lxrt.optimization import clip_grad_norm_
    from xggm_amd.runtime import runtime_of
    cfg, m, o = _tiny(5, 11, _lamb, dt=F32)
    b = _batch(cfg)
    m.eval()
    _backward(m, b, "rel")
    arena = runtime_of(m).arena
    before = {n: (p.detach().cpu().clone(), p.grad.detach().cpu().clone()) for n, p in m.named_parameters() if p.grad is not None}
    clip_grad_norm_(m.parameters(), MAX_NORM, tail=(o, None))
    coef = clip_coef(np.float32(arena.sqnorm.item()))
    o.step()
    ratios = o.trust_ratios()
    plain = {id(p) for p in o.param_groups[1]["params"]}
    worst_p = worst_r = 0.0
    for n, p in m.named_parameters():
        if n not in before:
            continue
        p_old, g = before[n]
        wd, ad = (0.0, False) if id(p) in plain else (0.01, True)
        gk = (g * float(coef)).to(F32).reshape(-1)
        z64, z32 = torch.zeros(gk.numel(), dtype=torch.float64), torch.zeros(gk.numel())
        p64, _, _, r = restate(torch.float64, p_old.double().reshape(-1), gk, z64, z64, 1e-3, wd, ad)
        p32, _, _, _ = restate(F32, p_old.reshape(-1), gk, z32, z32, 1e-3, wd, ad)
        worst_p = max(worst_p, ratio_of([p.detach().reshape(-1)], [p64], [p32]))
        worst_r = max(worst_r, abs(ratios[n] - r) / r)
        assert (ratios[n] == 1.0) == (not ad or float(p_old.abs().max()) == 0.0), n
    print("model step: p error / bound %.3f over %d tensors; trust ratios: worst relative error %.2e" % (worst_p, len(before), worst_r))
    assert len(before) > 50 and worst_p <= 1.0 and worst_r <= 1e-6


def test_training_state_round_trip(tmp_path):
    """save_training_state after two iterations, load_training_state into a fresh model and a fresh BertLamb: the third
    iteration equals the straight run bit for bit, and the file holds BertAdam's layout"""
    from xggm_amd.vqa.vqacpv2 import save_training_state, load_training_state
    cfg, ma, oa = _tiny(5, 11, _lamb)
    _, mb, ob = _tiny(77, 99, _lamb)
    b = _batch(cfg)
    for _ in range(2):
        _iteration(ma, oa, b)
    path = str(tmp_path / "state.pth")
    save_training_state(path, ma, oa, step=2)
    sd = oa.state_dict()
    assert set(sd["state"][0]) == {"step", "next_m", "next_v"} and [g["layer_adaptation"] for g in sd["param_groups"]] == [True, False]
    _iteration(mb, ob, b)  # a history of its own
    assert load_training_state(path, mb, ob) == {"step": 2}
    la, lb = _iteration(ma, oa, b), _iteration(mb, ob, b)
    assert la == lb
    _arena_equal(ma, mb)
    assert oa.trust_ratios() == ob.trust_ratios()


def test_refusals():
    from xggm_amd.fp8 import enable_fp8
    from xggm_amd.vqa.vqacpv2 import enable_data_parallel
    cfg, m, o = _tiny(5, 11, _lamb)
    enable_data_parallel(m, wire_dtype=BF16, zero1=True)
    with pytest.raises(RuntimeError, match="zero1.*norm would cross"):
        o.step()
    _, m2, o2 = _tiny(5, 11, _lamb)
    enable_fp8(m2)
    with pytest.raises(RuntimeError, match="fp8 forward"):
        o2.step()
