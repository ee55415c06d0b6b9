"""``split_groups``: lr and weight decay per tensor from a device map, on the fused update.

Kernel level: ONE mapped launch over a flat range of eight tensors (three param_groups round-robin, one tensor in none)
against per-tensor launches of the unmapped entry points -- bit for bit -- and against ``torch.optim`` with two groups on
the CPU.  The bound of the numerical comparison is the one of test_optim_gpu.py, restated: with ``ref64`` / ``ref32`` the
same-named torch class stepping on the same clipped gradients in fp64 / fp32,
max|x_gpu - ref64| <= 4 * max|ref32 - ref64| + ulp32(max|x|).  The spread ref32 - ref64 is torch's own rounding on these
inputs, the factor 4 covers a different but fixed operation order; nothing is calibrated on the code under test.

Model level: the tiny 2/2/1 model of test_optim_gpu.py, B = 4, A = 29, plain + rel + node passes."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from test_optim_gpu import RULES, MAX_NORM, clip_coef, seeded_grads, _tiny, _batch, _backward, _arena_equal  # noqa: E402

DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def ratio_of(x_gpu, r64, r32):
    """max|x_gpu - ref64| / (4 max|ref32 - ref64| + ulp32(max|x|)) over a list of tensors: <= 1 is the bound"""
    err = max(float((x.detach().double().cpu() - a).abs().max()) for x, a in zip(x_gpu, r64))
    spread = max(float((b.double() - a).abs().max()) for a, b in zip(r64, r32))
    top = max(float(a.abs().max()) for a in r64)
    return err / (4.0 * spread + float(np.spacing(np.float32(top))))


# ------------------------------------------------------------------------------------------------------------ flat buffers
SIZES = [3, 4, 8, 12, 260, 512, 1027, 70001]
OFFS = [8, 16, 24, 32, 48, 512, 1032, 2064]  # 8-aligned, not 64-aligned -- but the 512 on a 256-element boundary
OWNER = [1, 2, 3, 0, 1, 2, 3, 1]             # three param_groups round-robin; the tensor of 12 is in none
END = OFFS[-1] + SIZES[-1]                   # 72065: the whole range [8, END) has n % 4 == 1 -- the scalar tail runs too
TOTAL = (END + 255) // 256 * 256
LRS = {1: 1e-2, 2: 3e-3, 3: 2.5e-2}
WDS = {1: 0.1, 2: 0.0, 3: 0.03}
BERT = ("bertadam", None, dict(b1=0.9, b2=0.999, eps=1e-6), (True, True))


def _id_map(owner=OWNER):
    from xggm_amd import arena
    info = {"t%d" % i: (o, n, "g", True) for i, (o, n) in enumerate(zip(OFFS, SIZES))}
    ids = arena.hyper_id_map(info, {"t%d" % i: w for i, w in enumerate(owner)}, TOTAL)
    assert ids.nbytes == TOTAL // 8
    return torch.from_numpy(ids).to(DEV)


def _table(lrs=LRS, wds=WDS):
    return torch.tensor([[0.0, 0.0]] + [[lrs[i], wds[i]] for i in (1, 2, 3)], dtype=F32, device=DEV)


class Flat:
    """one 'arena group' in flat device buffers with the layout above"""

    def __init__(self, gdtype, p0, uses):
        self.p = p0.to(DEV).clone()
        self.g = torch.zeros(TOTAL, device=DEV, dtype=gdtype)
        self.m = torch.zeros(TOTAL, device=DEV)
        self.v = torch.zeros(TOTAL, device=DEV)
        for buf, used in zip((self.m, self.v), uses):
            if not used:
                buf.fill_(7.0)  # a buffer the rule does not have is neither read nor written
        self.m[OFFS[3]:OFFS[3] + SIZES[3]] = 7.0  # the tensor in no param_group: a sentinel in its moments
        self.v[OFFS[3]:OFFS[3] + SIZES[3]] = 7.0
        self.shadow = self.p.to(BF16)
        self.steps = torch.zeros(1, device=DEV, dtype=torch.int64)
        self.lr_scale = torch.ones(1, device=DEV)
        self.hs = torch.zeros(4, device=DEV)
        self.sq = torch.zeros(1, device=DEV)

    def views(self, buf, which=None):
        return [buf[o:o + n] for i, (o, n) in enumerate(zip(OFFS, SIZES)) if which is None or i in which]

    def load(self, gs, sq):
        self.sq.fill_(float(sq))
        for x, g in zip(self.views(self.g), gs):
            x.copy_(g)

    def sched(self, hp):
        from xggm_amd import ops
        b1, b2 = hp.get("betas", (0.0, 0.0))
        ops.sched_step_ex(self.steps, self.lr_scale, self.hs, [(0, -1, 0.0, "warmup_linear", b1, b2)])
        if "b1" in hp:
            self.lr_scale.fill_(0.7)  # BertAdam: a schedule value that is not 1

    def job(self, a, b, hp, lr, wd, clip=True):
        sl = slice(a, b)
        b1, b2 = hp.get("betas", (0.0, 0.0))
        args = (self.p[sl], self.g[sl], self.m[sl], self.v[sl], self.shadow[sl], self.sq if clip else None, MAX_NORM, lr,
                self.lr_scale, hp.get("b1", 0.0), hp.get("b2", 0.0), hp.get("eps", 0.0), wd)
        rule = dict(step_scalars=self.hs, b1=b1, b2=b2, momentum=hp.get("momentum", 0.0), dampening=hp.get("dampening", 0.0),
                    alpha=hp.get("alpha", 0.0), nesterov=hp.get("nesterov", False))
        return args, dict(elem0=a), rule

    def launch(self, rule, jobs, hyper_map=None):
        from xggm_amd import ops
        ops.optim_multi(rule, jobs, hyper_map=hyper_map)


def _start(seed=7):
    gen = torch.Generator().manual_seed(seed)
    p0 = torch.zeros(TOTAL)
    for o, n in zip(OFFS, SIZES):
        p0[o:o + n] = torch.randn(n, generator=gen)
    return p0


def _grads(step, bf16_exact):
    gs = seeded_grads(SIZES, step, bf16_exact=bf16_exact)
    sq = np.float32(sum(float(g.double().pow(2).sum()) for g in gs))
    assert (clip_coef(sq) < 1.0) == (step % 2 == 0)  # the clip is active on the even steps only
    return gs, sq


CASES = dict(RULES, bertadam=BERT)


@pytest.mark.parametrize("gdtype", [F32, BF16], ids=["g32", "g16"])
@pytest.mark.parametrize("key", list(CASES))
def test_one_mapped_launch_equals_per_tensor_launches(key, gdtype):
    """3 steps (clip active, inactive, active): the mapped launch over [8, END) against one unmapped launch per tensor
    with that tensor's lr and weight decay -- the parent's code -- on p, m, v and the shadow, bit for bit; the tensor in
    no param_group, the sentinel in its moments and the gap behind it are untouched."""
    rule, _, hp, uses = CASES[key]
    p0 = _start()
    fa, fb = Flat(gdtype, p0, uses), Flat(gdtype, p0, uses)
    ids, table = _id_map(), _table()
    owned = [i for i, w in enumerate(OWNER) if w]
    for s in range(3):
        gs, sq = _grads(s, bf16_exact=True)
        for f in (fa, fb):
            f.load(gs, sq)
            f.sched(hp)
        fa.launch(rule, [fa.job(OFFS[0], END, hp, 123.0, 456.0)], hyper_map=(ids, table))  # (the span's own lr / wd: not read)
        for i in owned:
            fb.launch(rule, [fb.job(OFFS[i], OFFS[i] + SIZES[i], hp, LRS[OWNER[i]], WDS[OWNER[i]])])
        for k in ("p", "m", "v", "shadow"):
            for i, (x, y) in zip(owned, zip(fa.views(getattr(fa, k), owned), fb.views(getattr(fb, k), owned))):
                assert torch.equal(x, y), (key, k, "step %d" % s, "tensor %d (%d elements)" % (i, SIZES[i]))
        lo, hi = OFFS[3], OFFS[4]  # the tensor of 12 and the 4 elements of gap behind it
        assert torch.equal(fa.p[lo:hi].cpu(), p0[lo:hi]) and torch.equal(fa.shadow[lo:hi].cpu(), p0[lo:hi].to(BF16))
        assert bool((fa.m[lo:lo + 12] == 7.0).all()) and bool((fa.v[lo:lo + 12] == 7.0).all())
        assert torch.equal(fa.p[:8].cpu(), p0[:8]) and torch.equal(fa.p[END:].cpu(), p0[END:])  # nothing outside the span
    moved = [not torch.equal(x.cpu(), p0[o:o + n]) for x, o, n in zip(fa.views(fa.p, owned), [OFFS[i] for i in owned],
                                                                      [SIZES[i] for i in owned])]
    assert all(moved)


@pytest.mark.parametrize("key", list(CASES))
def test_uniform_table_equals_the_unmapped_multi_span_launch(key):
    """every id with the same lr / weight decay: the mapped launch of the eight spans equals the unmapped one, whole
    buffers, bit for bit (bf16 gradients, clip active then inactive)"""
    rule, _, hp, uses = CASES[key]
    p0 = _start(8)
    fa, fb = Flat(BF16, p0, uses), Flat(BF16, p0, uses)
    owner = [1, 2, 3, 1, 2, 3, 1, 2]
    ids = _id_map(owner)
    table = _table({i: LRS[1] for i in LRS}, {i: WDS[1] for i in WDS})
    for s in range(2):
        gs, sq = _grads(s, bf16_exact=True)
        for f, hm in ((fa, (ids, table)), (fb, None)):
            f.load(gs, sq)
            f.sched(hp)
            f.launch(rule, [f.job(o, o + n, hp, LRS[1], WDS[1]) for o, n in zip(OFFS, SIZES)], hyper_map=hm)
    for k in ("p", "m", "v", "shadow"):
        assert torch.equal(getattr(fa, k), getattr(fb, k)), (key, k)
    assert not torch.equal(fa.p.cpu(), p0)


@pytest.mark.parametrize("key", list(RULES))
def test_mapped_launch_matches_a_two_group_torch_optimiser(key):
    """torch.optim with two param_groups (weight decay 0.1 / 0.0, two learning rates) on the CPU in fp64 and fp32, on the
    same clipped gradients, 4 steps: p and the rule's state under the bound of the module docstring"""
    rule, tcls, hp, (mn, vn) = RULES[key]
    owner = [1, 2, 1, 2, 1, 2, 1, 2]
    lrs, wds = {1: hp["lr"], 2: 0.3 * hp["lr"], 3: 0.0}, {1: 0.1, 2: 0.0, 3: 0.0}
    p0 = _start(9)
    f = Flat(F32, p0, (bool(mn), bool(vn)))
    f.m[OFFS[3]:OFFS[3] + SIZES[3]] = 7.0 if not mn else 0.0  # (every tensor is owned here: no sentinel)
    f.v[OFFS[3]:OFFS[3] + SIZES[3]] = 7.0 if not vn else 0.0
    ids, table = _id_map(owner), _table(lrs, wds)
    refs = []
    for dt in (torch.float64, torch.float32):
        ps = [torch.nn.Parameter(p0[o:o + n].to(dt).clone()) for o, n in zip(OFFS, SIZES)]
        common = {k: v for k, v in hp.items() if k not in ("lr", "weight_decay")}
        groups = [dict(params=[p for p, w in zip(ps, owner) if w == i], lr=lrs[i], weight_decay=wds[i]) for i in (1, 2)]
        refs.append((ps, tcls(groups, **common)))
    for s in range(4):
        gs = seeded_grads(SIZES, s)
        sq = np.float32(sum(float(g.double().pow(2).sum()) for g in gs))
        coef = clip_coef(sq)
        f.load(gs, sq)
        f.sched(hp)
        f.launch(rule, [f.job(OFFS[0], END, hp, 0.0, 0.0)], hyper_map=(ids, table))
        for ps, opt in refs:
            for p, g in zip(ps, gs):
                p.grad = (g * float(coef)).to(F32).to(p.dtype)  # the fp32 product the kernel forms, for both references
            opt.step()
        (p64, o64), (p32, o32) = refs
        rs = {"p": ratio_of(f.views(f.p), [p.detach() for p in p64], [p.detach() for p in p32])}
        for buf, name in ((f.m, mn), (f.v, vn)):
            if name:
                rs[name] = ratio_of(f.views(buf), [o64.state[p][name] for p in p64], [o32.state[p][name] for p in p32])
        print("%s step %d: error / bound %s" % (key, s, {k: round(v, 3) for k, v in rs.items()}))
        assert all(v <= 1.0 for v in rs.values()), (key, s, rs)
        assert torch.equal(f.shadow[OFFS[0]:END], f.p[OFFS[0]:END].to(BF16))


# ------------------------------------------------------------------------------------------------------------- model level
def _is_no_decay(n):
    from xggm_amd.vqa.vqacpv2 import NO_DECAY
    return any(s in n for s in NO_DECAY)


def _two_groups(m, second=None):
    """decay / no-decay: a split that cuts through every arena group"""
    decay = [p for n, p in m.named_parameters() if not _is_no_decay(n)]
    no_decay = [p for n, p in m.named_parameters() if _is_no_decay(n)]
    assert decay and no_decay
    return [{"params": decay}, dict({"params": no_decay}, **(second or {}))]


def _bertadam(groups, **kw):
    from xggm_amd.lxrt.optimization import BertAdam
    return BertAdam(groups, lr=1e-3, **kw)  # (no t_total: the schedule value is 1 from the first step on)


def _iteration(m, o, b, kinds=("plain", "rel", "node")):
    """eager passes as the engine runs them; -> the losses"""
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


@pytest.mark.parametrize("name", ["BertAdam", "AdamW"])
def test_equal_hyper_parameters_equal_the_unsplit_update(name):
    """decay / no-decay groups with the SAME hyper-parameters under split_groups=True against a twin under today's
    unsplit optimiser: parameters, moments and bf16 shadows after 3 iterations, bit for bit"""
    from xggm_amd import optim as xo
    if name == "BertAdam":
        mk1 = lambda mm: _bertadam(mm.parameters())  # noqa: E731
        mk2 = lambda mm: _bertadam(_two_groups(mm), split_groups=True)  # noqa: E731
    else:
        mk1 = lambda mm: xo.AdamW(mm.parameters(), lr=1e-3)  # noqa: E731
        mk2 = lambda mm: xo.AdamW(_two_groups(mm), lr=1e-3, split_groups=True)  # noqa: E731
    cfg, m1, o1 = _tiny(5, 11, mk1)
    _, m2, o2 = _tiny(5, 11, mk2)
    b = _batch(cfg)
    for _ in range(3):
        l1, l2 = _iteration(m1, o1, b), _iteration(m2, o2, b)
        assert l1 == l2 and all(math.isfinite(x) for x in l1)
    _arena_equal(m1, m2)
    from xggm_amd.runtime import runtime_of
    a = runtime_of(m2).arena
    assert float(a.m.abs().max()) > 0 and min(a.steps.tolist()) >= 3
    assert o2._split_state["ids"].numel() * 8 == a.total and len(o1.param_groups) == 1 and not hasattr(o1, "_split_state")


def test_frozen_bias_group_and_sync_hyper_eager_and_captured():
    """weight_decay 0 and lr 0 on the no-decay group: biases and LayerNorm weights stay bit-identical over an iteration
    while the matrices move; restoring the lr through sync_hyper() moves them again -- eagerly and under CapturedTrainer
    replays, the two bit for bit"""
    from xggm_amd.engine import CapturedTrainer
    mk = lambda mm: _bertadam(_two_groups(mm, dict(weight_decay=0.0)), split_groups=True)  # noqa: E731
    cfg, m1, o1 = _tiny(5, 11, mk)
    _, m2, o2 = _tiny(5, 11, mk)
    b = _batch(cfg)
    tr = CapturedTrainer(m1, o1, b, sigma=1.0, warmup_iters=1)
    m2.train()
    _iteration(m2, o2, b)  # the constructor's warm-up iteration
    frozen = {n: p for n, p in m1.named_parameters() if _is_no_decay(n)}
    w = m1.logit_fc[3].weight
    for lr in (0.0, 1e-3):
        for o in (o1, o2):
            o.param_groups[1]["lr"] = lr
            o.sync_hyper()
        before = {n: p.detach().clone() for n, p in frozen.items()}
        w0 = w.detach().clone()
        tr.iteration("rel")
        _iteration(m2, o2, b, ("plain", "rel"))
        same = [torch.equal(p.detach(), before[n]) for n, p in frozen.items()]
        assert not torch.equal(w.detach(), w0)
        if lr == 0.0:
            assert all(same)
        else:
            assert not torch.equal(frozen["logit_fc.3.bias"].detach(), before["logit_fc.3.bias"])
            assert not torch.equal(frozen["logit_fc.2.weight"].detach(), before["logit_fc.2.weight"])
        _arena_equal(m1, m2)
    assert o1._split_state["table"][2].tolist() == [float(np.float32(1e-3)), 0.0]


def _grad_norm64(arena):
    act = [arena.groups[g] for g in arena.active_groups()]
    return math.sqrt(sum(float((arena.grads[G.start:G.end].double() ** 2).sum()) for G in act))


def _step_by_hand(m, o, b, kind):
    """backward, the norm, the update; -> (reported norm, fp64 norm of the gradient buffer)"""
    from xggm_amd.lxrt.optimization import clip_grad_norm_
    from xggm_amd.runtime import runtime_of
    _backward(m, b, kind)
    arena = runtime_of(m).arena
    want = _grad_norm64(arena)
    total = float(clip_grad_norm_(m.parameters(), MAX_NORM, tail=(o, None)))
    o.step()
    o.zero_grad()
    m.zero_grad()  # (the parameters the optimiser was not given: torch would go on accumulating their gradients too)
    runtime_of(m).advance()
    return total, want


def test_heads_only_optimiser_leaves_the_encoder_alone():
    """only logit_fc + generator + encoder_adj + node_fc + fusion_fc in the optimiser: every encoder parameter, moment and
    shadow is bit-unchanged after an iteration, and the reported clip norm is the norm of the WHOLE gradient buffer (fp64,
    relative 1e-4: the tolerance of test_engine_gpu.test_full_size_iteration_properties)"""
    from xggm_amd.runtime import runtime_of
    heads = ("logit_fc", "generator", "encoder_adj", "node_fc", "fusion_fc")
    mk = lambda mm: _bertadam([p for n, p in mm.named_parameters() if n.split(".")[0] in heads], split_groups=True)  # noqa: E731
    cfg, m, o = _tiny(5, 11, mk)
    assert {n.split(".")[0] for n, _ in m.named_parameters()} == set(heads) | {"lxrt_encoder"}
    b = _batch(cfg)
    arena = runtime_of(m).arena
    enc = [(G.start, G.end) for g, G in arena.groups.items() if g.startswith("enc_")]
    snap = {k: getattr(arena, k).clone() for k in ("params", "m", "v", "shadow")}
    for kind in ("plain", "rel", "node"):
        total, want = _step_by_hand(m, o, b, kind)
        assert abs(total - want) < 1e-4 * want, (kind, total, want)
    for k, old in snap.items():
        for a, e in enc:
            assert torch.equal(getattr(arena, k)[a:e], old[a:e]), k
    for h in heads:
        G = arena.groups[h]
        assert not torch.equal(arena.params[G.start:G.end], snap["params"][G.start:G.end]), h
    assert float(arena.m[enc[0][0]:enc[0][1]].abs().max()) == 0.0


def test_tensors_left_out_inside_an_arena_group_keep_their_bits():
    """the encoder's LayerNorm parameters and logit_fc.3.weight in no param_group: they, their moments and their shadows
    stay as they are while their arena-group siblings move, and their gradient still counts in the norm"""
    from xggm_amd.runtime import runtime_of
    out = lambda n: ("LayerNorm" in n and n.startswith("lxrt_encoder.")) or n == "logit_fc.3.weight"  # noqa: E731
    mk = lambda mm: _bertadam([p for n, p in mm.named_parameters() if not out(n)], split_groups=True)  # noqa: E731
    cfg, m, o = _tiny(5, 11, mk)
    b = _batch(cfg)
    arena = runtime_of(m).arena
    snap = {k: getattr(arena, k).clone() for k in ("params", "m", "v", "shadow")}
    for kind in ("plain", "rel"):
        total, want = _step_by_hand(m, o, b, kind)
        assert abs(total - want) < 1e-4 * want, (kind, total, want)
    n_out = n_moved = 0
    for n, (off, k, g, _) in arena.info.items():
        same = [torch.equal(getattr(arena, key)[off:off + k], snap[key][off:off + k]) for key in snap]
        if out(n):
            n_out += 1
            assert all(same), n
        elif g in ("enc_main", "logit_fc") and n.endswith("dense.weight") or n.startswith("logit_fc.0."):
            n_moved += 1
            assert not any(same), n  # a sibling in the same arena group: parameter, moments and shadow all moved
    assert n_out > 10 and n_moved > 10


def test_make_optimizer_with_no_decay_and_layer_decay():
    from oracle import shapes
    from xggm_amd.vqa.vqacpv2 import NO_DECAY, make_optimizer, split_param_names
    lr, d = 1e-3, 0.9
    cfg, m, o = _tiny(5, 11, lambda mm: make_optimizer(mm, lr, 40, no_decay=NO_DECAY, layer_decay=d))
    assert o.split_groups and type(o).__name__ == "BertAdam"
    names = [n for n, _ in m.named_parameters()]
    assert set(names) == set(shapes.model_shapes(cfg, 29))
    want = split_param_names(names, lr, NO_DECAY, d, 2, 2, 1)
    assert [len(g["names"]) for g in want] == [len(pg["params"]) for pg in o.param_groups]
    b = _batch(cfg)
    losses = _iteration(m, o, b) + _iteration(m, o, b)
    assert all(math.isfinite(x) and x > 0 for x in losses)
    table = o._split_state["table"].cpu()
    assert table.shape == (len(o.param_groups) + 1, 2) and table[0].tolist() == [0.0, 0.0]
    D = 2 + 2 + 1
    by_name = {n: i for i, g in enumerate(want) for n in g["names"]}
    for n, base, depth, wd in (("logit_fc.3.weight", 4 * lr, D, 0.01), ("logit_fc.2.weight", 4 * lr, D, 0.0),
                               ("lxrt_encoder.model.bert.pooler.dense.weight", lr, D, 0.01),
                               ("lxrt_encoder.model.bert.encoder.x_layers.1.visn_output.dense.bias", lr, 4, 0.0),
                               ("lxrt_encoder.model.bert.encoder.x_layers.0.lang_inter.dense.weight", lr, 3, 0.01),
                               ("lxrt_encoder.model.bert.encoder.layer.1.output.LayerNorm.weight", lr, 2, 0.0),
                               ("lxrt_encoder.model.bert.encoder.r_layers.0.output.dense.weight", lr, 2, 0.01),
                               ("lxrt_encoder.model.bert.encoder.layer.0.intermediate.dense.weight", lr, 1, 0.01),
                               ("lxrt_encoder.model.bert.embeddings.word_embeddings.weight", lr, 0, 0.01),
                               ("lxrt_encoder.model.bert.encoder.visn_fc.box_layer_norm.weight", lr, 0, 0.0)):
        row = table[by_name[n] + 1].tolist()
        assert row == [float(np.float32(base * d ** (D - depth))), float(np.float32(wd))], (n, row)
    # with both None the optimiser is the one of today: two groups, no split
    o0 = make_optimizer(m, lr, 40)
    assert not o0.split_groups and [pg["lr"] for pg in o0.param_groups] == [4 * lr, lr]


@pytest.mark.parametrize("name", ["BertAdam", "AdamW"])
def test_state_dict_round_trip(name):
    """save after 2 iterations, load into a fresh optimiser with the same groups on a twin restored with load_state_dict:
    the third iteration equals the straight run bit for bit.  The xggm_amd.optim.AdamW dict goes through a two-group
    torch.optim.AdamW on the CPU and back."""
    from xggm_amd import optim as xo
    from xggm_amd.runtime import runtime_of
    hp2 = dict(weight_decay=0.0, lr=3e-4)
    if name == "BertAdam":
        mk = lambda mm: _bertadam(_two_groups(mm, hp2), split_groups=True)  # noqa: E731
    else:
        mk = lambda mm: xo.AdamW(_two_groups(mm, hp2), lr=1e-3, split_groups=True)  # noqa: E731
    cfg, ma, oa = _tiny(5, 11, mk)
    _, mb, ob = _tiny(77, 99, mk)
    b = _batch(cfg)
    for _ in range(2):
        _iteration(ma, oa, b)
    sd = oa.state_dict()
    assert len(sd["param_groups"]) == 2 and len(sd["state"]) == len(list(ma.parameters()))
    if name == "AdamW":
        groups = [[torch.nn.Parameter(p.detach().cpu().clone()) for p in pg["params"]] for pg in oa.param_groups]
        twin = torch.optim.AdamW([{"params": groups[0]}, dict({"params": groups[1]}, **hp2)], lr=1e-3)
        twin.load_state_dict(sd)
        flat = groups[0] + groups[1]
        for i, q in enumerate(flat):
            st = twin.state[q]
            assert float(st["step"]) == float(sd["state"][i]["step"]) >= 2
            for k in ("exp_avg", "exp_avg_sq"):
                assert st[k].device.type == "cpu" and torch.equal(st[k], sd["state"][i][k].cpu())
        assert [g["weight_decay"] for g in twin.param_groups] == [0.01, 0.0]
        twin.step()  # (no gradients: a no-op, but the loaded state has to be what torch's own step accepts)
        sd = twin.state_dict()
    mb.load_state_dict(ma.state_dict())
    runtime_of(mb).rng.copy_(runtime_of(ma).rng)
    ob.load_state_dict(sd)
    la, lb = _iteration(ma, oa, b), _iteration(mb, ob, b)
    assert la == lb
    _arena_equal(ma, mb)


def test_fp8_forward_with_split_groups():
    """enable_fp8 + split_groups=True runs, and with equal hyper-parameters equals the unsplit fp8 run bit for bit --
    the e4m3 weight copies and their scales included"""
    from xggm_amd.fp8 import enable_fp8
    from xggm_amd.runtime import runtime_of
    cfg, m1, o1 = _tiny(5, 11, lambda mm: _bertadam(mm.parameters()))
    _, m2, o2 = _tiny(5, 11, lambda mm: _bertadam(_two_groups(mm), split_groups=True))
    b = _batch(cfg)
    sent = (b["input_ids"], b["input_mask"], b["segment_ids"])
    for m in (m1, m2):
        enable_fp8(m)
        with torch.no_grad():
            m(b["feats"], b["boxes"], sent)  # calibration forward
        runtime_of(m).advance()
        assert runtime_of(m).arena.fp8.active
    for _ in range(2):
        l1, l2 = _iteration(m1, o1, b), _iteration(m2, o2, b)
        assert l1 == l2 and all(math.isfinite(x) for x in l1)
    _arena_equal(m1, m2)
    f1, f2 = runtime_of(m1).arena.fp8, runtime_of(m2).arena.fp8
    assert torch.equal(f1.shadow8, f2.shadow8) and torch.equal(f1.qscale, f2.qscale) and torch.equal(f1.amax, f2.amax)
    assert int((f2.shadow8 != 0).sum()) > 0


def test_refusals():
    from xggm_amd import optim as xo
    from xggm_amd.lxrt.optimization import BertAdam
    from xggm_amd.vqa.vqacpv2 import enable_data_parallel
    # a split in a key other than lr / weight_decay inside an arena group: named
    cfg, m, o = _tiny(5, 11, lambda mm: xo.Adam(_two_groups(mm, dict(betas=(0.8, 0.999))), lr=1e-3, split_groups=True))
    b = _batch(cfg)
    p0 = m.logit_fc[3].weight.detach().clone()
    with pytest.raises(ValueError, match="betas"):
        _iteration(m, o, b, ("plain",))
    assert torch.equal(m.logit_fc[3].weight.detach(), p0)
    m.zero_grad()
    o = BertAdam(_two_groups(m, dict(t_total=80)), lr=1e-3, warmup=0.1, t_total=40, split_groups=True)
    with pytest.raises(ValueError, match="t_total"):
        _iteration(m, o, b, ("plain",))
    m.zero_grad()
    # without the keyword a split is refused as before
    o = BertAdam(_two_groups(m, dict(weight_decay=0.0)), lr=1e-3)
    with pytest.raises(ValueError, match="param_groups"):
        _iteration(m, o, b, ("plain",))
    # the sharded update
    _, m2, o2 = _tiny(5, 11, lambda mm: _bertadam(_two_groups(mm), split_groups=True))
    enable_data_parallel(m2, wire_dtype=BF16, zero1=True)
    with pytest.raises(RuntimeError, match="split_groups"):
        o2.step()
