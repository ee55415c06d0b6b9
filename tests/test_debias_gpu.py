"""The debias answer losses on the GPU: parity of the fused kernels with the reference's float64 results
(tests/golden/debias.npz), ``bias_index`` against an expanded bias, ``Plain`` against the existing head loss, bit-equality
across runs, and the model level -- eager passes, ``CapturedTrainer``, state_dict, weight-decay groups, refusals and
replicated data parallelism.

Tolerances are the project's (``test_kernels_gpu.tol``: 2e-5 in fp32, 1.2e-2 in bf16) on ``rel_err``; the loss to 1e-5
relative; the two scalar gradients (bias_lin.bias, smooth_param: cancelling sums over B x A terms) to tol x the stored sum of
the absolute values of their terms."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from xggm_amd import synth  # noqa: E402
from helpers import batch_tensors, load_golden, rel_err  # noqa: E402
from test_kernels_gpu import tol  # noqa: E402

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, BF16 = torch.float32, torch.bfloat16


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def golden():
    g = load_golden("debias")
    return g, json.loads(str(g["meta_json"]))


def _kind(name):
    from xggm_amd import ops
    return dict(LearnedMixin=ops.DEBIAS_LEARNED_MIXIN, BiasProduct=ops.DEBIAS_BIAS_PRODUCT,
                ReweightByInvBias=ops.DEBIAS_REWEIGHT)[name]


def _inputs(c, dt):
    """device tensors of golden case ``c`` (meta entry); bf16: hidden and bias_lin rounded to bf16 first, as the golden's"""
    x = synth.debias_case(c["B"], c["A"], c["Hd"], c["seed"], c["bias_max"])
    t = {k: torch.from_numpy(v).to(DEV) for k, v in x.items()}
    if c["Hd"]:
        if dt == BF16:
            t["lin_w"], t["lin_b"] = t["lin_w"].to(BF16).float(), t["lin_b"].to(BF16).float()
        t["hidden"] = t["hidden"].to(dt)
    kw = c["kwargs"]
    smooth = c["kind"] != "ReweightByInvBias" and kw.get("smooth", True)
    t["smooth_param"] = torch.full((1,), float(kw.get("smooth_init", -1)), device=DEV) if smooth else None
    return t


def _run(c, t, dlogit_dtype=None, bias=None, bias_index=None, save=None):
    from xggm_amd import ops
    kw = c["kwargs"]
    loss, pr = ops.debias_fwd(_kind(c["kind"]), t["logits"], t["labels"], t["bias"] if bias is None else bias, bias_index,
                              t.get("hidden"), t.get("lin_w"), t.get("lin_b"), t["smooth_param"],
                              kw.get("constant_smooth", 0.0), kw.get("w", 0.0), save=save)
    return (loss,) + ops.debias_bwd(pr, dlogit_dtype=dlogit_dtype)


NAMES = ("loss", "d_logit", "d_hidden", "d_lin_w", "d_lin_b", "d_smooth")


@pytest.mark.parametrize("name,dt", [(n, F32) for n in "abcdefgh"] + [(n, BF16) for n in "acd"],
                         ids=lambda v: v if isinstance(v, str) else str(v).split(".")[-1])
def test_parity_with_the_reference(golden, name, dt):
    g, meta = golden
    c = meta["cases"][name]
    tag = name + (".bf16" if dt == BF16 else "")
    out = dict(zip(NAMES, _run(c, _inputs(c, dt))))
    torch.cuda.synchronize()
    t = tol(dt)
    loss, want = float(out["loss"]), float(g[tag + ".loss"])
    print("%s loss %.9g (reference %.9g, rel %.2e)" % (tag, loss, want, abs(loss - want) / abs(want)))
    figures = {}
    dl = out["d_logit"].float().cpu()
    assert out["d_logit"].dtype == (dt if c["Hd"] else F32)
    if c["whole"]:
        figures["d_logit"] = rel_err(dl, torch.from_numpy(g[tag + ".d_logit"]))
    else:
        figures["d_logit[::97]"] = rel_err(dl.reshape(-1)[::meta["stride"]], torch.from_numpy(g[tag + ".d_logit_every97"]))
        rs = (dl.double().sum(1) - torch.from_numpy(g[tag + ".d_logit_rowsum"])).abs() / torch.from_numpy(g[tag + ".d_logit_rowabs"])
        figures["d_logit row sums / abs-sums"] = float(rs.max())
    if c["Hd"]:
        assert out["d_hidden"].dtype == dt
        figures["d_hidden"] = rel_err(out["d_hidden"], torch.from_numpy(g[tag + ".d_hidden"]))
        figures["d_lin_w"] = rel_err(out["d_lin_w"], torch.from_numpy(g[tag + ".d_lin_w"]).reshape(-1))
        figures["d_lin_b / abs-sum"] = abs(float(out["d_lin_b"]) - float(g[tag + ".d_lin_b"][0])) / float(g[tag + ".d_lin_b_abs"])
    else:
        assert out["d_hidden"] is None and out["d_lin_w"] is None and out["d_lin_b"] is None
    if (tag + ".d_smooth") in g.files:
        figures["d_smooth / abs-sum"] = abs(float(out["d_smooth"]) - float(g[tag + ".d_smooth"][0])) / float(g[tag + ".d_smooth_abs"])
    else:
        assert out["d_smooth"] is None
    for k, v in figures.items():
        print("%s %s: %.3e (bound %.1e)" % (tag, k, v, t))
    assert abs(loss - want) <= 1e-5 * abs(want)
    for k, v in figures.items():
        assert v < t, (tag, k, v)


def _equal(a, b):
    assert len(a) == len(b)
    for name, x, y in zip(NAMES, a, b):
        assert (x is None) == (y is None), name
        if x is not None:
            assert x.dtype == y.dtype and torch.equal(x, y), name


@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
def test_bias_index_equals_an_expanded_bias(golden, dt):
    """case (a) through a [4, A] table plus an index: the same bits as the gathered [B, A] bias (which is case (a)'s own);
    d_logit in fp32 under either suffix, as the answer head takes it"""
    g, meta = golden
    c = meta["cases"]["a"]
    t = _inputs(c, dt)
    extra = torch.from_numpy(synth.debias_case(1, c["A"], 0, 99)["bias"]).to(DEV)
    table = torch.cat([t["bias"][2:3], extra, t["bias"][0:1], t["bias"][1:2]])
    idx = torch.tensor([2, 3, 0], device=DEV)
    assert torch.equal(table[idx], t["bias"])
    direct = _run(c, t, dlogit_dtype=F32)
    via = _run(c, t, dlogit_dtype=F32, bias=table, bias_index=idx)
    torch.cuda.synchronize()
    assert via[1].dtype == F32
    _equal(direct, via)
    assert abs(float(via[0]) - float(g["a" + (".bf16" if dt == BF16 else "") + ".loss"])) <= 1e-5 * float(via[0])
    # an index outside the table is clamped into it (no read leaves the table): row 3 for 7, row 0 for -2
    far = _run(c, t, dlogit_dtype=F32, bias=table, bias_index=torch.tensor([2, 7, -2], device=DEV))
    near = _run(c, t, dlogit_dtype=F32, bias=table, bias_index=torch.tensor([2, 3, 0], device=DEV))
    _equal(far, near)


def test_plain_equals_the_existing_head_loss():
    from xggm_amd.module.vqa_debias_loss_functions import Plain
    from xggm_amd.vqa.vqacpv2 import BCEWithLogitsLoss
    x = synth.debias_case(3, 3129, 0, 21)
    res = []
    for fn in (lambda z, y: Plain()(None, z, None, y), lambda z, y: BCEWithLogitsLoss()(z, y, scale=y.size(1))):
        z = torch.from_numpy(x["logits"]).to(DEV).requires_grad_(True)
        loss = fn(z, torch.from_numpy(x["labels"]).to(DEV))
        loss.backward()
        res.append((loss.detach(), z.grad))
    torch.cuda.synchronize()
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    ref = torch.nn.functional.binary_cross_entropy_with_logits(torch.from_numpy(x["logits"]).double(),
                                                               torch.from_numpy(x["labels"]).double()) * 3129
    assert abs(float(res[0][0]) - float(ref)) <= 1e-5 * float(ref)


@pytest.mark.parametrize("name", ["d", "e", "g"])
def test_same_bits_across_runs_beside_other_work_and_on_poisoned_buffers(golden, name, monkeypatch):
    g, meta = golden
    c = meta["cases"][name]
    t = _inputs(c, BF16 if c["Hd"] else F32)
    first = _run(c, t)
    second = _run(c, t)
    big = torch.empty(32 << 20, dtype=F32, device=DEV)  # 128 MB: copies that are still busy while the loss runs
    big2 = torch.empty_like(big)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for _ in range(4):
            big2.copy_(big)
    beside = _run(c, t)
    torch.cuda.synchronize()
    # every buffer the kernels are handed (save, d_*, the backward's scratch) full of NaN: they write all they read
    real_empty, real_like = torch.empty, torch.empty_like

    def poisoned(fn):
        def wrapper(*a, **k):
            x = fn(*a, **k)
            return x.fill_(float("nan")) if x.is_floating_point() else x
        return wrapper

    monkeypatch.setattr(torch, "empty", poisoned(real_empty))
    monkeypatch.setattr(torch, "empty_like", poisoned(real_like))
    save = torch.full((2 * c["B"],), float("nan"), device=DEV)
    poison = _run(c, t, save=save)
    monkeypatch.undo()
    torch.cuda.synchronize()
    for other in (second, beside, poison):
        _equal(first, other)
    for x in first:
        assert x is None or bool(torch.isfinite(x.float()).all())


def test_the_loss_classes_run_the_fused_kernels_stand_alone(golden):
    """the public classes outside a model: autograd hands the parameter gradients out; the same bits as the ops level"""
    from xggm_amd.module.vqa_debias_loss_functions import LearnedMixin, BiasProduct, ReweightByInvBias
    g, meta = golden
    for name, cls in (("c", LearnedMixin), ("e", BiasProduct), ("h", ReweightByInvBias)):
        c = meta["cases"][name]
        t = _inputs(c, F32)
        m = cls(**c["kwargs"], **(dict(hidden_dim=c["Hd"]) if c["Hd"] else {})).to(DEV)
        if c["Hd"]:
            m.load_state_dict(dict(m.state_dict(), **{"bias_lin.weight": t["lin_w"], "bias_lin.bias": t["lin_b"]}))
        z = t["logits"].clone().requires_grad_(True)
        h = t["hidden"].clone().requires_grad_(True) if c["Hd"] else None
        loss = m(h, z, t["bias"], t["labels"])
        loss.backward()
        want = _run(c, t, dlogit_dtype=F32)
        torch.cuda.synchronize()
        got = (loss.detach(), z.grad, None if h is None else h.grad,
               m.bias_lin.weight.grad.reshape(-1) if c["Hd"] else None, m.bias_lin.bias.grad if c["Hd"] else None,
               m.smooth_param.grad if getattr(m, "smooth_param", None) is not None else None)
        _equal(want, got)
    with pytest.raises(ValueError):
        LearnedMixin(0.3, hidden_dim=16).to(DEV)(torch.zeros(2, 8, device=DEV), torch.zeros(2, 4, device=DEV),
                                                 torch.zeros(2, 4, device=DEV), torch.zeros(2, 4, device=DEV))


# ----------------------------------------------------------------------------- the model level (tiny configuration)
B, A, T_TOTAL = 4, 29, 40
BRANCHES = ("rel", "node", "rel")
DEBIAS = ("debias_loss.bias_lin.weight", "debias_loss.bias_lin.bias", "debias_loss.smooth_param")


def _tiny(dtype, loss="mixin", no_decay=None, attach=True):
    from oracle import shapes
    from xggm_amd import param
    from xggm_amd.lxrt.modeling import BertConfig, VISUAL_CONFIG
    from xggm_amd.module.vqa_debias_loss_functions import LearnedMixin
    from xggm_amd.vqa.vqacpv2 import attach_debias_loss, make_optimizer
    from xggm_amd.vqa.vqacpv2_model import VQAModel
    cfg = dict(shapes.TINY, l_layers=2, x_layers=2, r_layers=1)  # H = 128
    VISUAL_CONFIG.set_visual_dims(cfg["feat_dim"], 4)
    a = param.parse_args(["--llayers", "2", "--xlayers", "2", "--rlayers", "1"])
    bc = BertConfig(cfg["vocab"], hidden_size=cfg["hidden"], num_attention_heads=cfg["heads"],
                    intermediate_size=cfg["inter"], max_position_embeddings=cfg["max_pos"])
    m = VQAModel(A, gnn="GCN", n_layers=2, args=a, config=bc, compute_dtype=dtype)
    m.load_state_dict({k: torch.from_numpy(synth.seeded_param(k, v.shape, 5)) for k, v in m.state_dict().items()})
    m = m.to(DEV)
    m.seed = 11
    dl = LearnedMixin(0.36, hidden_dim=cfg["hidden"])
    dl.load_state_dict({k: torch.from_numpy(synth.seeded_param("debias_loss." + k, v.shape, 5)) for k, v in dl.state_dict().items()})
    dl.set_bias_table(synth.debias_case(3, A, 0, 31)["bias"])
    if attach:
        attach_debias_loss(m, dl)
    return cfg, m, make_optimizer(m, 1e-4, T_TOTAL, no_decay=no_decay), dl


def _batches(cfg, key):
    out = []
    for s in (3, 4, 5, 6):
        b = batch_tensors(synth.vqa_batch(B, A=A, F=cfg["feat_dim"], vocab=cfg["vocab"], seed=s), DEV)
        if key == "bias":
            b["bias"] = torch.from_numpy(synth.debias_case(B, A, 0, 40 + s)["bias"]).to(DEV)
        else:
            b["bias_index"] = torch.tensor([(s + i) % 3 for i in range(B)], device=DEV)
        out.append(b)
    return out


def _state(m):
    from xggm_amd.runtime import runtime_of
    rt = runtime_of(m)
    arena = rt.arena
    st = {k: getattr(arena, k).clone() for k in ("params", "m", "v", "shadow") if getattr(arena, k) is not None}
    st["steps"], st["lr_scale"], st["rng"] = arena.steps.clone(), arena.lr_scale.clone(), rt.rng.clone()
    return st


def _eager_batch(x):
    return dict(x, sent=(x["input_ids"], x["input_mask"], x["segment_ids"]))


@pytest.fixture(scope="module")
def trained():
    """bf16: three iterations (rel, node, rel) on three batches with ``bias_index`` and a TrainLog, once replayed from
    ``CapturedTrainer`` graphs and once through the eager ``train_iteration`` (behind the trainer's warm-up passes, run by
    hand).  fp32: three eager iterations with a ``bias`` key."""
    from xggm_amd.engine import CapturedTrainer, TrainLog
    from xggm_amd.vqa.vqacpv2 import train_iteration
    out = {}
    for name in ("captured", "eager"):
        cfg, m, o, dl = _tiny(BF16)
        b = _batches(cfg, "bias_index")
        before = {k: v.detach().clone() for k, v in m.state_dict().items()}
        log = TrainLog(8, DEV)
        t = CapturedTrainer(m, o, b[0], sigma=1.0, warmup_iters=1, use_graph=name == "captured",
                            train_log=log if name == "captured" else None)
        if name == "eager":
            for kind in ("plain", "rel", "node"):  # the constructor's warm-up passes, by hand
                t._eager_pass(kind)
        for i, br in enumerate(BRANCHES):
            if name == "captured":
                t.load_batch(b[i + 1])
                t.iteration(br)
            else:
                train_iteration(m, o, t.bce, _eager_batch(b[i + 1]), sigma=1.0, order="vqa", branch=br, clip=5.0, train_log=log)
        torch.cuda.synchronize()
        out[name] = dict(model=m, optim=o, loss=dl, log=log, state=_state(m), before=before, trainer=t)
    from xggm_amd.vqa.vqacpv2 import BCEWithLogitsLoss
    cfg, m, o, dl = _tiny(F32)
    before = {k: v.detach().clone() for k, v in m.state_dict().items()}
    losses = []
    for x, br in zip(_batches(cfg, "bias")[1:], BRANCHES):
        r = train_iteration(m, o, BCEWithLogitsLoss(), _eager_batch(x), sigma=1.0, branch=br)
        losses.append((r["loss_plain"], r["loss_ggm"]))
    torch.cuda.synchronize()
    out["fp32"] = dict(model=m, before=before, losses=losses)
    return out


@pytest.mark.parametrize("run", ["eager", "captured", "fp32"])
def test_the_loss_parameters_are_trained(trained, run):
    r = trained[run]
    sd = r["model"].state_dict()
    assert [k for k in sd if k.startswith("debias_loss.")] == ["debias_loss.smooth_param", "debias_loss.bias_table",
                                                                "debias_loss.bias_lin.weight", "debias_loss.bias_lin.bias"]
    for k in DEBIAS:
        assert bool(torch.isfinite(sd[k]).all()) and not torch.equal(sd[k], r["before"][k]), k
    assert torch.equal(sd["debias_loss.bias_table"], r["before"]["debias_loss.bias_table"])
    arena = r["model"].arena()
    for k in DEBIAS:  # vector class, in a group of their own, views of the arena
        o, n, group, atomic = arena.info[k]
        assert group == "debias_loss" and atomic
        assert sd[k].data_ptr() == arena.params[o:o + n].data_ptr()
    if run == "fp32":
        assert all(bool(torch.isfinite(a)) and bool(torch.isfinite(b)) for a, b in r["losses"])


def test_captured_replay_equals_eager_iterations(trained):
    cap, eag = trained["captured"], trained["eager"]
    assert sorted(cap["state"]) == sorted(eag["state"])
    for k in cap["state"]:  # parameters, moments, bf16 weights, step counters, schedule values, the RNG words
        assert torch.equal(cap["state"][k], eag["state"][k]), k
    assert torch.equal(cap["log"].buf, eag["log"].buf)
    rec = cap["log"].read()
    assert int(rec["cursor"]) == 6 and int(rec["first_bad"]) == -1
    from xggm_amd.engine import TrainLog as L
    v = rec["values"].numpy()
    assert (v[:, L.BCE] > 0).all() and np.isfinite(v).all()
    plain = rec["kinds"].numpy() == L.PLAIN
    assert np.array_equal(v[plain, L.BCE], v[plain, L.LOSS])  # the plain pass's loss IS the debias loss


def test_state_dict_round_trip_keeps_the_loss(trained):
    m = trained["eager"]["model"]
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    assert all(k in sd for k in DEBIAS)
    _, m2, _, _ = _tiny(BF16)
    m2.load_state_dict(sd)
    sd2 = m2.state_dict()
    assert list(sd2) == list(sd)
    for k in sd:
        assert torch.equal(sd2[k], sd[k]), k


def test_no_decay_puts_the_loss_parameters_in_the_undecayed_group():
    from xggm_amd.vqa.vqacpv2 import NO_DECAY, train_iteration, BCEWithLogitsLoss
    cfg, m, o, _ = _tiny(BF16, no_decay=NO_DECAY)
    named = dict(m.named_parameters())
    for k in DEBIAS:
        groups = [g for g in o.param_groups if any(p is named[k] for p in g["params"])]
        assert len(groups) == 1 and groups[0].get("weight_decay") == 0.0, k
    before = {k: named[k].detach().clone() for k in DEBIAS}
    for x, br in zip(_batches(cfg, "bias")[1:3], BRANCHES):
        train_iteration(m, o, BCEWithLogitsLoss(), _eager_batch(x), sigma=1.0, branch=br)
    torch.cuda.synchronize()
    for k in DEBIAS:
        assert bool(torch.isfinite(named[k]).all()) and not torch.equal(named[k].detach(), before[k]), k


def test_refusals():
    from xggm_amd.engine import CapturedTrainer
    from xggm_amd.tools.data_loader import DataLoaderX  # noqa: F401  (the packed hand-over exists)
    from xggm_amd.vqa.vqacpv2 import (attach_debias_loss, enable_data_parallel, train_iteration, plain_pass, BCEWithLogitsLoss)
    # attaching after the first forward
    cfg, m, o, dl = _tiny(BF16, attach=False)
    b = _batches(cfg, "bias")[0]
    sent = (b["input_ids"], b["input_mask"], b["segment_ids"])
    with pytest.raises(TypeError):
        attach_debias_loss(m, torch.nn.BCEWithLogitsLoss())
    m(b["feats"], b["boxes"], sent)
    with pytest.raises(RuntimeError, match="before the first forward"):
        attach_debias_loss(m, dl)
    # a batch without bias
    cfg, m, o, dl = _tiny(BF16)
    bare = {k: v for k, v in b.items() if k != "bias"}
    with pytest.raises(ValueError, match="bias"):
        train_iteration(m, o, BCEWithLogitsLoss(), _eager_batch(bare), branch="rel")
    with pytest.raises(ValueError, match="bias"):
        plain_pass(m, o, BCEWithLogitsLoss(), b["feats"], b["boxes"], sent, b["target"])
    with pytest.raises(ValueError, match="bias"):
        CapturedTrainer(m, o, bare, use_graph=False)._eager_pass("plain")
    # the packed hand-over and the sharded update
    with pytest.raises(ValueError, match="packed_spec"):
        CapturedTrainer(m, o, b, packed_spec=object(), use_graph=False)
    with pytest.raises(RuntimeError, match="zero1"):
        enable_data_parallel(m, wire_dtype=BF16, zero1=True)


# ----------------------------------------------------------------------------- replicated data parallelism (two gloo ranks, one GPU)
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_data_parallel_replicas_train_the_loss_identically():
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", XGGM_DIST_BACKEND="gloo", XGGM_SHARE_GPU="1")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
                        os.path.join(ROOT, "tools", "dp_debias_rehearsal.py")], capture_output=True, text=True, timeout=300,
                       env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    for k in DEBIAS:
        assert "%s: moved True equal True" % k in r.stdout, r.stdout[-3000:]
    assert "replicas equal True" in r.stdout
