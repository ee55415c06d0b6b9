"""The reference's ``--optim`` choices (src/param.py:9-31) on the fused device update, against ``torch.optim`` on the CPU.

The bound of every numerical comparison: with ``ref64`` / ``ref32`` the same-named torch class stepping on the same clipped
gradients in fp64 / fp32,  max|x_gpu - ref64| <= 4 * max|ref32 - ref64| + ulp32(max|x|).  The spread ref32 - ref64 is
torch's own rounding on these inputs, the factor 4 covers a different but fixed operation order; nothing is calibrated
on the code under test."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from xggm_amd import synth  # noqa: E402
from helpers import batch_tensors  # noqa: E402

DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
MAX_NORM = 5.0


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


# ---------------------------------------------------------------------------------------------------------------- helpers
def ratio_of(x_gpu, r64, r32):
    """max|x_gpu - ref64| / (4 max|ref32 - ref64| + ulp32(max|x|)) over a list of tensors: <= 1 is the bound"""
    err = max(float((x.detach().double().cpu() - a).abs().max()) for x, a in zip(x_gpu, r64))
    spread = max(float((b.double() - a).abs().max()) for a, b in zip(r64, r32))
    top = max(float(a.abs().max()) for a in r64)
    return err / (4.0 * spread + float(np.spacing(np.float32(top))))


def clip_coef(sq):
    """the kernel's clip scale from the fp32 sum of squares, in fp32: min(max_norm / (sqrt(sq) + 1e-6), 1)"""
    total = np.sqrt(np.float32(sq))
    return np.float32(min(np.float32(MAX_NORM) / (total + np.float32(1e-6)), np.float32(1.0)))


RULES = {
    "adam": ("adam", torch.optim.Adam, dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.1), ("exp_avg", "exp_avg_sq")),
    "adamw": ("adamw", torch.optim.AdamW, dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.1), ("exp_avg", "exp_avg_sq")),
    "adamax": ("adamax", torch.optim.Adamax, dict(lr=2e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.1), ("exp_avg", "exp_inf")),
    "sgd0": ("sgd", torch.optim.SGD, dict(lr=1e-2, momentum=0.0, weight_decay=0.1), (None, None)),
    "sgdm": ("sgd", torch.optim.SGD, dict(lr=1e-2, momentum=0.9, dampening=0.1, weight_decay=0.1), ("momentum_buffer", None)),
    "sgdn": ("sgd", torch.optim.SGD, dict(lr=1e-2, momentum=0.9, nesterov=True, weight_decay=0.1), ("momentum_buffer", None)),
    "rms0": ("rmsprop", torch.optim.RMSprop, dict(lr=1e-2, alpha=0.99, eps=1e-8, weight_decay=0.1), (None, "square_avg")),
    "rmsm": ("rmsprop", torch.optim.RMSprop, dict(lr=1e-2, alpha=0.99, eps=1e-8, weight_decay=0.1, momentum=0.9),
             ("momentum_buffer", "square_avg")),
}
SIZES4 = [3, 4, 1027, 70001]  # tail only, exactly one vector, an odd tail, more than one unrolled stride of the grid
SIZES9 = [3, 4, 1027, 70001, 5, 260, 1, 2049, 8]  # past ADAM_MULTI = 8 spans: two launches


class Flat:
    """spans of one 'arena group' in flat device buffers (starts 64-element aligned), one step counter"""

    def __init__(self, sizes, gdtype=F32, sentinel=0.0):
        self.sizes = sizes
        self.off, o = [], 0
        for n in sizes:
            self.off.append(o)
            o = (o + n + 63) // 64 * 64
        self.total = o
        self.p = torch.zeros(o, device=DEV)
        self.g = torch.zeros(o, device=DEV, dtype=gdtype)
        self.m = torch.full((o,), sentinel, device=DEV)
        self.v = torch.full((o,), sentinel, device=DEV)
        self.shadow = torch.zeros(o, device=DEV, dtype=BF16)
        self.steps = torch.zeros(1, device=DEV, dtype=torch.int64)
        self.lr_scale = torch.ones(1, device=DEV)
        self.hs = torch.zeros(4, device=DEV)
        self.sq = torch.zeros(1, device=DEV)

    def views(self, buf):
        return [buf[o:o + n] for o, n in zip(self.off, self.sizes)]

    def step(self, rule, hp, clip=True):
        from xggm_amd import ops
        b1, b2 = hp.get("betas", (0.0, 0.0))
        ops.sched_step_ex(self.steps, self.lr_scale, self.hs, [(0, -1, 0.0, "warmup_linear", b1, b2)])
        jobs = []
        for o, n in zip(self.off, self.sizes):
            sl = slice(o, o + n)
            jobs.append(((self.p[sl], self.g[sl], self.m[sl], self.v[sl], self.shadow[sl], self.sq if clip else None, MAX_NORM,
                          hp["lr"], self.lr_scale, 0.0, 0.0, hp.get("eps", 0.0), hp["weight_decay"]), {},
                         dict(step_scalars=self.hs, b1=b1, b2=b2, momentum=hp.get("momentum", 0.0),
                              dampening=hp.get("dampening", 0.0), alpha=hp.get("alpha", 0.0), nesterov=hp.get("nesterov", False))))
        ops.optim_multi(rule, jobs)


def seeded_grads(sizes, step, bf16_exact=False):
    """N(0, 1) with a sprinkling of exact zeros; every other step scaled so that the clip at 5 is not active"""
    gen = torch.Generator().manual_seed(1000 + step)
    out = []
    for n in sizes:
        g = torch.randn(n, generator=gen)
        g[torch.rand(n, generator=gen) < 0.05] = 0.0
        if step % 2:
            g *= 0.01 if sum(sizes) > 10000 else 1.0
        out.append(g.to(BF16).float() if bf16_exact else g)
    if step % 2 and sum(sizes) > 10000:
        assert math.sqrt(sum(float(g.double().pow(2).sum()) for g in out)) < MAX_NORM
    return out


def run_against_torch(key, sizes, n_steps=6):
    rule, tcls, hp, (mn, vn) = RULES[key]
    f = Flat(sizes)
    gen = torch.Generator().manual_seed(7)
    p0 = [torch.randn(n, generator=gen) for n in sizes]
    for x, t in zip(f.views(f.p), p0):
        x.copy_(t)
    refs = []
    for dt in (torch.float64, torch.float32):
        ps = [torch.nn.Parameter(t.to(dt).clone()) for t in p0]
        refs.append((ps, tcls(ps, **hp)))
    if not mn:
        f.m.fill_(7.0)  # a buffer the rule does not have is neither read nor written
    if not vn:
        f.v.fill_(7.0)
    worst = 0.0
    for s in range(n_steps):
        gs = seeded_grads(sizes, s)
        sq = np.float32(sum(float(g.double().pow(2).sum()) for g in gs))
        f.sq.fill_(float(sq))
        coef = clip_coef(sq)
        assert (coef < 1.0) == (s % 2 == 0)  # the clip is active on the even steps only
        for x, g in zip(f.views(f.g), gs):
            x.copy_(g)
        f.step(rule, hp)
        for ps, opt in refs:
            for p, g in zip(ps, gs):
                p.grad = (g * float(coef)).to(F32).to(p.dtype)  # the fp32 product the kernel forms, for both references
            opt.step()
        (p64, o64), (p32, o32) = refs
        rs = {"p": ratio_of(f.views(f.p), [p.detach() for p in p64], [p.detach() for p in p32])}
        for buf, name in ((f.m, mn), (f.v, vn)):
            if name:
                rs[name] = ratio_of(f.views(buf), [o64.state[p][name] for p in p64], [o32.state[p][name] for p in p32])
            else:
                assert bool((buf == 7.0).all())
        print("%s spans=%d step %d (t=%d): error / bound %s" % (key, len(sizes), s, s + 1,
                                                                 {k: round(v, 3) for k, v in rs.items()}))
        assert all(v <= 1.0 for v in rs.values()), (key, s, rs)
        assert torch.equal(f.shadow, f.p.to(BF16))  # the shadow is the bf16 of the new masters, every step
        worst = max(worst, max(rs.values()))
    assert int(f.steps[0]) == n_steps
    return worst


# ------------------------------------------------------------------------------------------------------- kernel vs torch
@pytest.mark.parametrize("key", list(RULES))
def test_rule_matches_torch_over_four_spans(key):
    """6 steps, clip active on steps 0, 2, 4; weight decay on; step 0 is the t = 1, b2 = 0.999 case an fp32 1 - b^t fails"""
    w = run_against_torch(key, SIZES4)
    print("largest error / bound of %s: %.3f" % (key, w))


@pytest.mark.parametrize("key", list(RULES))
def test_rule_matches_torch_over_nine_spans(key):
    run_against_torch(key, SIZES9)


def _fp32_bias_correction(rule, hp, grads, coefs):
    """torch's Adam / AdamW formula in fp64 with ONLY the bias corrections 1 - b^t taken in fp32: what a kernel that
    computed them per element in fp32 would give, everything else being exact"""
    (b1, b2), lr, wd, eps = hp["betas"], hp["lr"], hp["weight_decay"], hp["eps"]
    P = [torch.zeros(g.shape, dtype=torch.float64) for g in grads[0]]
    M, V = [torch.zeros_like(x) for x in P], [torch.zeros_like(x) for x in P]
    for t, (gs, coef) in enumerate(zip(grads, coefs), 1):
        bc1 = float(np.float32(1) - np.power(np.float32(b1), np.float32(t)))
        bc2 = float(np.float32(1) - np.power(np.float32(b2), np.float32(t)))
        for p, m, v, g in zip(P, M, V, gs):
            g = (g * float(coef)).to(F32).double()
            if rule == "adamw":
                p.mul_(1 - lr * wd)
            else:
                g = g + wd * p
            m.lerp_(g, 1 - b1)
            v.mul_(b2).addcmul_(g, g, value=1 - b2)
            p.addcdiv_(m, v.sqrt() / math.sqrt(bc2) + eps, value=-lr / bc1)
    return P


@pytest.mark.parametrize("key,wd", [("adam", 0.0), ("adamw", 0.01), ("adamax", 0.0)])
def test_bias_correction_where_the_update_dominates(key, wd):
    """b2 = 0.999 from t = 1 on, with p0 = 0 and no (AdamW: a tiny decoupled) weight decay: |p| is lr after the first
    step, so ulp32(max|p|) is 1e-9 and the bound is torch's own rounding of the UPDATE -- a bias correction off by 1e-5
    relative cannot hide behind the rounding of p ~ 1 as in the cases above.  The same six steps as there.
    For Adam and AdamW the case is shown to discriminate: the fp64 formula with only 1 - b^t taken in fp32
    (1.f - 0.999f is 1.3e-5 below 0.001) has to EXCEED the bound at t = 1 (it does by a factor near 5)."""
    rule, tcls, hp, (mn, vn) = RULES[key]
    hp = dict(hp, weight_decay=wd)
    f = Flat(SIZES4)
    refs = []
    for dt in (torch.float64, torch.float32):
        ps = [torch.nn.Parameter(torch.zeros(n, dtype=dt)) for n in SIZES4]
        refs.append((ps, tcls(ps, **hp)))
    grads, coefs = [], []
    for s in range(6):
        gs = seeded_grads(SIZES4, s)
        sq = np.float32(sum(float(g.double().pow(2).sum()) for g in gs))
        f.sq.fill_(float(sq))
        coef = clip_coef(sq)
        grads.append(gs)
        coefs.append(coef)
        for x, g in zip(f.views(f.g), gs):
            x.copy_(g)
        f.step(rule, hp)
        for ps, opt in refs:
            for p, g in zip(ps, gs):
                p.grad = (g * float(coef)).to(F32).to(p.dtype)
            opt.step()
        (p64, o64), (p32, o32) = refs
        r64, r32 = [p.detach() for p in p64], [p.detach() for p in p32]
        rs = {"p": ratio_of(f.views(f.p), r64, r32)}
        for buf, name in ((f.m, mn), (f.v, vn)):
            rs[name] = ratio_of(f.views(buf), [o64.state[p][name] for p in p64], [o32.state[p][name] for p in p32])
        line = "%s p0=0 step %d (t=%d): error / bound %s" % (key, s, s + 1, {k: round(v, 3) for k, v in rs.items()})
        if key != "adamax":
            bad = ratio_of(_fp32_bias_correction(rule, hp, grads, coefs), r64, r32)
            line += "; fp32 1 - b^t: %.2f" % bad
        print(line)
        assert all(v <= 1.0 for v in rs.values()), (key, s, rs)
        if key != "adamax" and s == 0:
            assert bad > 1.0, bad  # the case tells an fp32 bias correction from a double one
        assert torch.equal(f.shadow, f.p.to(BF16))


@pytest.mark.parametrize("key", list(RULES))
def test_fp32_and_bf16_gradient_instantiations_agree(key):
    rule, _, hp, _ = RULES[key]
    fs = [Flat(SIZES4, gdtype=dt) for dt in (F32, BF16)]
    gen = torch.Generator().manual_seed(3)
    p0 = torch.randn(fs[0].total, generator=gen).to(DEV)
    for f in fs:
        f.p.copy_(p0)
    for s in range(3):
        gs = seeded_grads(SIZES4, s, bf16_exact=True)
        sq = float(np.float32(sum(float(g.double().pow(2).sum()) for g in gs)))
        for f in fs:
            f.sq.fill_(sq)
            for x, g in zip(f.views(f.g), gs):
                x.copy_(g)
            f.step(rule, hp)
    a, b = fs
    for k in ("p", "m", "v", "shadow"):
        assert torch.equal(getattr(a, k), getattr(b, k)), (key, k)


@pytest.mark.parametrize("name", ["adam", "adamw", "adamax", "sgd", "rmsprop"])
def test_zeros_stay_zeros(name):
    """default hyper-parameters, weight decay on: p = g = m = v = 0 stays exactly 0 for 6 steps (the arena's alignment
    gaps and the norm rely on it).  Adamax's exp_inf is max(b2 u, |g| + eps) = eps by torch's definition: p, its
    shadow and exp_avg stay 0 there."""
    from xggm_amd import optim as xo
    cls = {"adam": xo.Adam, "adamw": xo.AdamW, "adamax": xo.Adamax, "sgd": xo.SGD, "rmsprop": xo.RMSprop}[name]
    hp = dict(cls([torch.nn.Parameter(torch.zeros(1))]).defaults, weight_decay=0.01)
    variants = [hp] if name in ("adam", "adamw", "adamax") else [hp, dict(hp, momentum=0.9)]
    for h in variants:
        f = Flat(SIZES4)
        f.sq.fill_(1.0)
        for _ in range(6):
            f.step(name, h)
        zero = torch.zeros_like(f.p)
        assert torch.equal(f.p, zero) and torch.equal(f.shadow, zero.to(BF16)) and torch.equal(f.m, zero)
        if name != "adamax":
            assert torch.equal(f.v, zero)


# ------------------------------------------------------------------------------------------- bits of a recorded commit
def _golden():
    import importlib.util
    import json
    import os
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    spec = importlib.util.spec_from_file_location("make_optim_update_golden", os.path.join(here, "make_optim_update_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    with open(os.path.join(here, "optim_update_bits.json")) as f:
        return gen, json.load(f)


GOLDEN_GEN, GOLDEN = _golden()


@pytest.mark.parametrize("case", GOLDEN_GEN.cases(), ids=lambda c: c[0])
def test_update_bits_equal_the_recorded_commit(case):
    """three steps over nine spans (two launches) per rule, gradient type, with and without a hyper map, BertAdam also with
    the e4m3 copy + lr_dev + g_scale: SHA-256 of p, m, v, the bf16 shadow, the e4m3 copy and the amax table after every
    step equal the digests tests/golden/make_optim_update_golden.py recorded with the library of GOLDEN["commit"]"""
    from xggm_amd import ops
    cid, key, gdt, mapped, extra = case
    assert sorted(GOLDEN["cases"]) == sorted(c[0] for c in GOLDEN_GEN.cases())
    got = GOLDEN_GEN.run_case(ops, key, gdt, mapped, extra)
    assert got == GOLDEN["cases"][cid], (cid, [k for k in got if got[k] != GOLDEN["cases"][cid][k]])


# ------------------------------------------------------------------------------------------------------------- schedules
@pytest.mark.parametrize("warmup", [0.1, 0.35])
@pytest.mark.parametrize("kind", ["warmup_cosine", "warmup_constant", "warmup_linear"])
def test_schedule_on_the_device(kind, warmup):
    from xggm_amd import ops
    from xggm_amd.lxrt.optimization import SCHEDULES
    steps = torch.zeros(2, device=DEV, dtype=torch.int64)
    sc = torch.zeros(2, device=DEV)
    for s in range(13):
        ops.sched_step_ex(steps, sc, None, [(1, 10, warmup, kind, 0.0, 0.0)])
        want = SCHEDULES[kind](s / 10, warmup)
        assert abs(float(sc[1]) - want) <= 1e-6, (kind, warmup, s, float(sc[1]), want)
        assert steps.tolist() == [0, s + 1]


def _tiny(seed_w, seed_rt, make_opt, dt=BF16, layers=(2, 2, 1)):
    from oracle import shapes
    from test_model_gpu import build_model
    cfg = dict(shapes.TINY, l_layers=layers[0], x_layers=layers[1], r_layers=layers[2])
    m = build_model(cfg, 29, seed=seed_w, dt=dt)
    m.seed = seed_rt
    return cfg, m, make_opt(m)


def _batch(cfg, seed=3, B=4, A=29):
    return batch_tensors(synth.vqa_batch(B, A=A, F=cfg["feat_dim"], vocab=cfg["vocab"], seed=seed), DEV)


def _backward(m, b, kind):
    from xggm_amd.vqa.vqacpv2 import forward_backward_plain, forward_backward_ggm, BCEWithLogitsLoss
    sent = (b["input_ids"], b["input_mask"], b["segment_ids"])
    if kind == "plain":
        forward_backward_plain(m, BCEWithLogitsLoss(), b["feats"], b["boxes"], sent, b["target"])
    else:
        forward_backward_ggm(m, BCEWithLogitsLoss(), b["feats"], b["boxes"], sent, b["target"], b["adj_true"], kind, 1.0, 8.0)


def _bertadam_passes(kind, n_steps=6):
    """plain passes of BertAdam(schedule=kind, t_total=10, warmup=0.35) over the answer head in fp32 execution; yields per
    step (s, the optimiser, the arena, the head's last weight, its gradient, the clip coefficient, the Python schedule)"""
    from xggm_amd.lxrt.optimization import BertAdam, SCHEDULES, clip_grad_norm_
    from xggm_amd.runtime import runtime_of
    lr, wu, tt = 1e-3, 0.35, 10
    cfg, m, opt = _tiny(5, 11, lambda mm: BertAdam(mm.logit_fc.parameters(), lr=lr, warmup=wu, t_total=tt, schedule=kind),
                        dt=F32)  # (the head alone: get_lr() is [0] while a parameter of the optimiser has never been stepped)
    b = _batch(cfg)
    m.eval()
    w = m.logit_fc[3].weight
    yield w.detach().cpu().clone()
    for s in range(n_steps):
        _backward(m, b, "plain")
        g = w.grad.detach().cpu().clone()
        arena = runtime_of(m).arena
        clip_grad_norm_(m.parameters(), MAX_NORM, tail=(opt, None))
        assert not getattr(arena, "sched_done", False)  # a non-linear kind does not ride on the norm's launch
        coef = clip_coef(np.float32(arena.sqnorm.item()))
        opt.step()
        opt.zero_grad()
        yield s, opt, arena, w, g, coef, SCHEDULES[kind](s / tt, wu)


@pytest.mark.parametrize("kind", ["warmup_cosine", "warmup_constant"])
def test_bertadam_nonlinear_schedule_reaches_the_update_and_get_lr(kind):
    """the device's lr_scale of the pass and ``get_lr()`` agree with the Python schedule (src/lxrt/optimization.py:27-39)"""
    from xggm_amd.lxrt.optimization import SCHEDULES
    it = _bertadam_passes(kind)
    next(it)
    for s, opt, arena, w, g, coef, sched in it:
        assert abs(float(arena.lr_scale[arena.group_index[w._xg[3]]]) - sched) <= 1e-6
        got = opt.get_lr()
        assert len(got) == len(opt.param_groups[0]['params']) and abs(got[0] - 1e-3 * SCHEDULES[kind]((s + 1) / 10, 0.35)) < 1e-12


# ----------------------------------------------------------------------------------------------------------- model level
@pytest.mark.parametrize("name", ["adamax", "sgd"])
def test_model_level_passes_match_a_torch_twin(name):
    """tiny 2/2/1 H128 model, B = 4, fp32 execution, plain -> rel -> node -> plain: after each backward the parameters,
    gradients and the norm are copied, a torch.optim twin steps on the clipped gradients, and the pass's update is
    compared under the bound.  Groups a pass does not touch keep their parameters and step counts bit for bit."""
    from xggm_amd import optim as xo
    from xggm_amd.lxrt.optimization import clip_grad_norm_
    from xggm_amd.runtime import runtime_of
    cls, tcls, hp = {"adamax": (xo.Adamax, torch.optim.Adamax, dict(lr=1e-3, weight_decay=0.01)),
                     "sgd": (xo.SGD, torch.optim.SGD, dict(lr=1e-3, momentum=0.9, weight_decay=0.01))}[name]
    snames = {"adamax": ("exp_avg", "exp_inf"), "sgd": ("momentum_buffer", None)}[name]
    cfg, m, opt = _tiny(5, 11, lambda mm: cls(mm.parameters(), **hp), dt=F32)
    b = _batch(cfg)
    names = [n for n, _ in m.named_parameters()]
    params = [p for _, p in m.named_parameters()]
    twins = {}
    for dt in (torch.float64, torch.float32):
        ps = [torch.nn.Parameter(p.detach().cpu().to(dt)) for p in params]
        twins[dt] = (ps, tcls(ps, **hp))
    for i, kind in enumerate(["plain", "rel", "node", "plain"]):
        _backward(m, b, kind)
        arena = runtime_of(m).arena
        before = [p.detach().clone() for p in params]
        steps0 = arena.steps.tolist()
        grads = [None if p.grad is None else p.grad.detach().cpu().clone() for p in params]
        total = clip_grad_norm_(m.parameters(), MAX_NORM, tail=(opt, None))
        coef = clip_coef(np.float32(arena.sqnorm.item()))
        assert abs(float(total) - math.sqrt(float(arena.sqnorm.item()))) <= 1e-5 * float(total)
        opt.step()
        opt.zero_grad()
        touched = [g is not None for g in grads]
        for dt, (ps, topt) in twins.items():
            with torch.no_grad():
                for q, p0 in zip(ps, before):
                    q.copy_(p0.cpu().to(dt))
            for q, g in zip(ps, grads):
                q.grad = None if g is None else (g * float(coef)).to(F32).to(dt)
            topt.step()
        idx = [j for j, t in enumerate(touched) if t]
        r = ratio_of([params[j] for j in idx], [twins[torch.float64][0][j].detach() for j in idx],
                     [twins[torch.float32][0][j].detach() for j in idx])
        print("%s pass %d (%s): error / bound %.3f, clip coef %.4f" % (name, i, kind, r, float(coef)))
        assert r <= 1.0
        # ... and the state the twin carries across the passes (exp_avg / exp_inf, momentum_buffer), same bound
        for buf, key in ((arena.m, snames[0]), (arena.v, snames[1])):
            if key:
                views = [buf[params[j]._xg[1]:params[j]._xg[1] + params[j]._xg[2]].view(params[j].shape) for j in idx]
                rb = ratio_of(views, *[[twins[dt][1].state[twins[dt][0][j]][key] for j in idx]
                                       for dt in (torch.float64, torch.float32)])
                print("%s pass %d (%s): %s error / bound %.3f" % (name, i, kind, key, rb))
                assert rb <= 1.0
        # untouched groups: parameters and step counts exactly as before
        steps1 = arena.steps.tolist()
        for j, t in enumerate(touched):
            gi = arena.group_index[params[j]._xg[3]]
            if t:
                assert steps1[gi] == steps0[gi] + 1
            else:
                assert torch.equal(params[j].detach(), before[j]) and steps1[gi] == steps0[gi], names[j]
        if kind == "plain":
            idle = {n.split(".")[0] for n, t in zip(names, touched) if not t}
            assert {"generator", "encoder_adj", "node_fc", "fusion_fc"} <= idle, idle


def _arena_equal(m1, m2):
    from xggm_amd.runtime import runtime_of
    a1, a2 = runtime_of(m1).arena, runtime_of(m2).arena
    bad = [k for k in ("params", "m", "v", "shadow") if not torch.equal(getattr(a1, k), getattr(a2, k))]
    assert not bad, bad
    assert a1.steps.tolist() == a2.steps.tolist()


@pytest.mark.parametrize("name", ["Adamax", "AdamW"])
def test_captured_equals_eager_bf16(name):
    from xggm_amd import optim as xo
    from xggm_amd.engine import CapturedTrainer
    from xggm_amd.runtime import runtime_of
    from xggm_amd.vqa.vqacpv2 import plain_pass, ggm_pass, BCEWithLogitsLoss
    mk = lambda mm: getattr(xo, name)(mm.parameters(), lr=1e-4)  # noqa: E731
    cfg, m1, o1 = _tiny(5, 11, mk)
    _, m2, o2 = _tiny(5, 11, mk)
    batches = [_batch(cfg, s) for s in (3, 4)]
    branches = ["rel", "node", "rel"]
    tr = CapturedTrainer(m1, o1, batches[0], sigma=1.0, warmup_iters=1)
    for i, br in enumerate(branches):
        tr.load_batch(batches[i % 2])
        tr.iteration(br)
    bce, rt2 = BCEWithLogitsLoss(), runtime_of(m2)
    m2.train()

    def run(kind, b):
        sent = (b["input_ids"], b["input_mask"], b["segment_ids"])
        if kind == "plain":
            plain_pass(m2, o2, bce, b["feats"], b["boxes"], sent, b["target"])
        else:
            ggm_pass(m2, o2, bce, b["feats"], b["boxes"], sent, b["target"], b["adj_true"], kind, 1.0, 8.0)
        rt2.advance()

    for kind in ("plain", "rel", "node"):  # the constructor's warm-up iteration
        run(kind, batches[0])
    for i, br in enumerate(branches):
        run("plain", batches[i % 2])
        run(br, batches[i % 2])
    _arena_equal(m1, m2)
    assert float(runtime_of(m1).arena.m.abs().max()) > 0 and min(runtime_of(m1).arena.steps.tolist()) >= 2


# ------------------------------------------------------------------------------------------------- state-dict interchange
def test_state_dict_moves_to_torch_and_back_under_live_graphs():
    from xggm_amd import optim as xo
    from xggm_amd.engine import CapturedTrainer
    from xggm_amd.runtime import runtime_of
    mk = lambda mm: xo.Adamax(mm.parameters(), lr=1e-4, weight_decay=0.01)  # noqa: E731
    cfg, ma, oa = _tiny(5, 11, mk)
    _, mb, ob = _tiny(77, 99, mk)
    batch = _batch(cfg)
    ta = CapturedTrainer(ma, oa, batch, warmup_iters=1)
    tb = CapturedTrainer(mb, ob, batch, warmup_iters=1)
    for br in ("rel", "node"):
        ta.iteration(br)
    sd = oa.state_dict()
    # into torch.optim.Adamax over CPU clones of the parameters
    clones = [torch.nn.Parameter(p.detach().cpu().clone()) for p in ma.parameters()]
    twin = torch.optim.Adamax(clones, lr=1e-4, weight_decay=0.01)
    twin.load_state_dict(sd)
    assert len(sd["state"]) == len(clones)
    for i, q in enumerate(clones):
        st = twin.state[q]
        assert float(st["step"]) == float(sd["state"][i]["step"]) and float(st["step"]) >= 2
        for k in ("exp_avg", "exp_inf"):
            assert st[k].device.type == "cpu" and torch.equal(st[k], sd["state"][i][k].cpu())
    twin.step()  # (no gradients: a no-op, but the loaded state has to be what torch's own step accepts)
    # a torch-made state into a fresh optimiser whose graphs are captured already
    made = twin.state_dict()
    mb.load_state_dict(ma.state_dict())
    rtb = runtime_of(mb)
    rtb.rng.copy_(runtime_of(ma).rng)
    ob.load_state_dict(made)
    ta.iteration("rel")
    tb.iteration("rel")
    # the load is exact (fp32 buffers, integer steps) and replays are deterministic: the continuation is bit-identical,
    # which is within the bound
    _arena_equal(ma, mb)


def test_training_state_round_trip_with_adam(tmp_path):
    from xggm_amd import optim as xo
    from xggm_amd.engine import CapturedTrainer
    from xggm_amd.vqa.vqacpv2 import save_training_state, load_training_state
    mk = lambda mm: xo.Adam(mm.parameters(), lr=1e-4)  # noqa: E731
    cfg, ma, oa = _tiny(5, 11, mk)
    _, mb, ob = _tiny(77, 99, mk)
    batch = _batch(cfg)
    ta = CapturedTrainer(ma, oa, batch, warmup_iters=1)
    tb = CapturedTrainer(mb, ob, batch, warmup_iters=1)
    tb.iteration("rel")
    for br in ("rel", "node"):
        ta.iteration(br)
    path = str(tmp_path / "state.pth")
    save_training_state(path, ma, oa, iteration=2)
    (lp_a, _, _), (lg_a, _, _) = ta.iteration("rel")
    assert load_training_state(path, mb, ob) == {"iteration": 2}
    (lp_b, _, _), (lg_b, _, _) = tb.iteration("rel")
    assert [float(lp_b), float(lg_b)] == [float(lp_a), float(lg_a)]
    _arena_equal(ma, mb)


# --------------------------------------------------------------------------------------------------------------- refusals
def test_refusals():
    from xggm_amd import optim as xo
    from xggm_amd.vqa.vqacpv2 import clip_and_step, plain_pass, enable_data_parallel, BCEWithLogitsLoss
    cfg, m, _ = _tiny(5, 11, lambda mm: None)
    b = _batch(cfg)
    sent = (b["input_ids"], b["input_mask"], b["segment_ids"])
    _backward(m, b, "plain")
    w0 = m.logit_fc[3].weight.detach().clone()
    with pytest.raises(TypeError, match="xggm_amd.optim"):
        clip_and_step(m, torch.optim.Adamax(m.parameters()))
    assert torch.equal(m.logit_fc[3].weight.detach(), w0)
    m.zero_grad()
    decay = [p for n, p in m.named_parameters() if not n.endswith("bias")]
    no_decay = [p for n, p in m.named_parameters() if n.endswith("bias")]
    bad = xo.Adamax([{"params": decay}, {"params": no_decay, "weight_decay": 0.0}], lr=1e-3)
    with pytest.raises(ValueError, match="param_groups"):
        plain_pass(m, bad, BCEWithLogitsLoss(), b["feats"], b["boxes"], sent, b["target"])
    _, m2, o2 = _tiny(5, 11, lambda mm: xo.Adamax(mm.parameters(), lr=1e-3))
    enable_data_parallel(m2, wire_dtype=BF16, zero1=True)
    with pytest.raises(RuntimeError, match="BertAdam"):
        o2.step()


# ------------------------------------------------------------------------- BertAdam trajectory under the new schedules
@pytest.mark.parametrize("kind", ["warmup_cosine", "warmup_constant"])
def test_bertadam_schedule_trajectory(kind):
    """6 plain passes of BertAdam(schedule=kind, t_total=10, warmup=0.35, lr 1e-3, weight decay 0.01) over the answer
    head in fp32 execution: its last weight against the reference formula (src/lxrt/optimization.py:159-193) evaluated on
    the CPU in fp64 (ref64) and fp32 (ref32) on the same clipped gradients and Python schedule values, under the bound, at
    every step.  A second figure is printed per step and not asserted: the distance to the same fp32 formula with the
    complements 1 - b1, 1 - b2 taken in fp32, as the kernel's pinned ``adam_update`` takes them."""
    lr, wd = 1e-3, 0.01
    it = _bertadam_passes(kind)
    w0 = next(it)
    c_exact = (1 - 0.9, 1 - 0.999)
    c_kernel = (float(np.float32(1) - np.float32(0.9)), float(np.float32(1) - np.float32(0.999)))
    ref = {k: [w0.to(dt), torch.zeros(w0.shape, dtype=dt), torch.zeros(w0.shape, dtype=dt)]
           for k, dt in (("ref64", torch.float64), ("ref32", torch.float32), ("kernel32", torch.float32))}
    ratios = []
    for s, opt, arena, w, g, coef, sched in it:
        for k, (p, mm, vv) in ref.items():
            c1, c2 = c_kernel if k == "kernel32" else c_exact
            gc = (g * float(coef)).to(F32).to(p.dtype)
            mm.mul_(0.9).add_(gc, alpha=c1)
            vv.mul_(0.999).addcmul_(gc, gc, value=c2)
            p.add_(mm / (vv.sqrt() + 1e-6) + wd * p, alpha=-lr * sched)
        r = ratio_of([w], [ref["ref64"][0]], [ref["ref32"][0]])
        ulp = float(np.spacing(np.float32(ref["ref64"][0].abs().max())))
        k_ulps = float((w.detach().cpu() - ref["kernel32"][0]).abs().max()) / ulp
        print("BertAdam %s step %d: error / bound %.3f; against the formula with fp32 complements: %.2f ulp32(max|p|)"
              % (kind, s, r, k_ulps))
        ratios.append(r)
    assert all(r <= 1.0 for r in ratios), ratios
