"""The softmax answer losses on the GPU: parity of the fused kernels with the reference's float64 results
(tests/golden/softmax_loss.npz: the reference's ``Focal``, torch's ``CrossEntropyLoss(ignore_index=-1)``), ``bias_index``
against an expanded bias, soft targets against class indices, bit-equality across runs, and the model level -- eager passes,
``CapturedTrainer``, the training log, the packed hand-over.

Tolerances are the project's (``test_kernels_gpu.tol``: 2e-5 in fp32, 1.2e-2 in bf16): the loss relative, ``rel_err`` on
d_logit.  The golden's generator admits a case only if the reference's own float32 run meets half of the fp32 bar."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from xggm_amd import synth  # noqa: E402
from helpers import batch_tensors, load_golden, rel_err  # noqa: E402
from test_kernels_gpu import tol  # noqa: E402

DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
IGNORE = -1


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def golden():
    g = load_golden("softmax_loss")
    return g, json.loads(str(g["meta_json"]))


def _inputs(golden, name):
    """device tensors of golden case ``name``: logits, labels, bias (and label_index for the index variant)"""
    g, meta = golden
    c = meta["cases"][name]
    x = synth.debias_case(c["B"], c["A"], 0, c["seed"])
    if c["variant"] == "all_ignored":
        x["labels"] = np.zeros_like(x["labels"])
    t = {k: torch.from_numpy(v).to(DEV) for k, v in x.items()}
    t["label_index"] = torch.from_numpy(g[name + ".label_index"]).to(DEV) if c["variant"] == "label_index" else None
    return t


def _kind(kind):
    from xggm_amd import ops
    return dict(focal=ops.SOFTMAX_FOCAL, ce=ops.SOFTMAX_CE)[kind]


def _one():
    return torch.ones((), device=DEV)


def _run(kind, t, bias=None, bias_index=None, label_index=None, labels=True, scale=1.0, save=None, gout=None, d_logit=None):
    """-> (loss, d_logit, labels int32, problem)"""
    from xggm_amd import ops
    li = t.get("label_index") if label_index is None else label_index
    loss, pr = ops.softmax_loss_fwd(_kind(kind), t["logits"], t["labels"] if labels else None, li if kind == "ce" else None,
                                    (t["bias"] if bias is None else bias) if kind == "focal" else None, bias_index,
                                    ignore_index=IGNORE, scale=scale, save=save)
    d = ops.softmax_loss_bwd(pr, _one() if gout is None else gout, d_logit=d_logit)
    return loss, d, pr.labels_int32(), pr


CASES = [(n, k) for n in "abcdefg" for k in ("focal", "ce")] + [("h", "ce"), ("i", "ce")]


@pytest.mark.parametrize("name,kind", CASES)
def test_parity_with_the_reference(golden, name, kind):
    g, meta = golden
    c = meta["cases"][name]
    assert kind in c["kinds"]
    tag = "%s.%s" % (name, kind)
    loss, d, labels, _ = _run(kind, _inputs(golden, name))
    torch.cuda.synchronize()
    loss, want = float(loss), float(g[tag + ".loss"])
    want_d = torch.from_numpy(g[tag + ".d_logit"])
    assert d.dtype == F32 and tuple(d.shape) == (c["B"], c["A"])
    if kind == "ce":
        print("%s labels %s (recorded %s)" % (tag, labels.cpu().tolist()[:8], g[tag + ".labels"].tolist()[:8]))
        assert labels.dtype == torch.int32 and np.array_equal(labels.cpu().numpy().astype(np.int64), g[tag + ".labels"])
        ignored = torch.from_numpy(g[tag + ".labels"] == IGNORE)
        assert not d.cpu()[ignored].any()  # exactly zero, not small
    if c["variant"] == "all_ignored":
        # what torch did when the golden was recorded: a NaN loss, an all-zero gradient
        print("%s loss %r (recorded %r), |d_logit| max %g" % (tag, loss, want, float(d.abs().max())))
        assert np.isnan(want) == np.isnan(loss) and np.isnan(loss)
        assert torch.equal(d.cpu(), want_d) and not want_d.any()
        return
    err_loss = abs(loss - want) / abs(want) if want != 0.0 else abs(loss)
    err_d = rel_err(d, want_d)
    print("%s loss %.9g (reference %.9g, rel %.2e)   d_logit rel_err %.3e   (bound %.1e; the reference's own float32 run: "
          "%.2e, %.2e)" % (tag, loss, want, err_loss, err_d, tol(F32), c["gate"][kind]["loss"], c["gate"][kind]["d_logit"]))
    assert bool(torch.isfinite(d).all())
    assert err_loss <= tol(F32)
    assert err_d <= tol(F32)


def _equal(a, b):
    for x, y in zip(a[:3], b[:3]):
        assert x.dtype == y.dtype and torch.equal(x, y)


def test_bias_index_equals_an_expanded_bias(golden):
    """Focal, case (d) through a [4, A] table plus an index: the same bits as the gathered [B, A] bias (case (d)'s own)"""
    g, _ = golden
    t = _inputs(golden, "d")
    A = t["logits"].shape[1]
    extra = torch.from_numpy(synth.debias_case(1, A, 0, 99)["bias"]).to(DEV)
    table = torch.cat([t["bias"][2:3], extra, t["bias"][0:1], t["bias"][1:2]])
    idx = torch.tensor([2, 3, 0], device=DEV)
    assert torch.equal(table[idx], t["bias"])
    direct = _run("focal", t)
    via = _run("focal", t, bias=table, bias_index=idx)
    # a table whose rows are wider than A (a view): the row stride is honoured
    wide = torch.cat([table, table.new_full((4, 3), 7.0)], 1)[:, :A]
    assert wide.stride(0) == A + 3
    strided = _run("focal", t, bias=wide, bias_index=idx)
    # an index outside the table is clamped into it (no read leaves the table): row 3 for 7, row 0 for -2
    far = _run("focal", t, bias=table, bias_index=torch.tensor([2, 7, -2], device=DEV))
    torch.cuda.synchronize()
    for other in (via, strided, far):
        _equal(direct, other)
    assert abs(float(via[0]) - float(g["d.focal.loss"])) <= tol(F32) * float(g["d.focal.loss"])


@pytest.mark.parametrize("name", ["b", "d", "f", "g"])
def test_soft_targets_equal_the_same_labels_as_an_index(golden, name):
    g, _ = golden
    t = _inputs(golden, name)
    soft = _run("ce", t, scale=1.75)
    index = _run("ce", t, label_index=torch.from_numpy(g[name + ".ce.labels"]).to(DEV), scale=1.75)
    only = _run("ce", t, label_index=torch.from_numpy(g[name + ".ce.labels"]).to(DEV), labels=False, scale=1.75)
    unit = _run("ce", t)
    torch.cuda.synchronize()
    _equal(soft, index)
    _equal(soft, only)
    assert abs(float(soft[0]) - 1.75 * float(unit[0])) <= 1e-6 * abs(float(soft[0]))
    assert rel_err(soft[1], 1.75 * unit[1]) <= 1e-6
    # an index outside [0, A) that is not ignore_index: the row is ignored, nothing is read outside the row
    bad = torch.from_numpy(g[name + ".ce.labels"]).clone()
    valid = np.nonzero(g[name + ".ce.labels"] >= 0)[0]
    bad[valid[0]] = t["logits"].shape[1]
    out = _run("ce", t, label_index=bad.to(DEV))
    torch.cuda.synchronize()
    assert int(out[2][valid[0]]) == IGNORE and not out[1][valid[0]].any()


@pytest.mark.parametrize("name,kind", [("g", "focal"), ("g", "ce"), ("d", "focal"), ("d", "ce"), ("f", "focal"), ("f", "ce")])
def test_same_bits_across_runs_beside_other_work_and_on_poisoned_buffers(golden, name, kind, monkeypatch):
    t = _inputs(golden, name)
    B = t["logits"].shape[0]
    first = _run(kind, t)
    second = _run(kind, t)
    big = torch.empty(32 << 20, dtype=F32, device=DEV)  # 128 MB: copies that are still busy while the loss runs
    big2 = torch.empty_like(big)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for _ in range(4):
            big2.copy_(big)
    beside = _run(kind, t)
    torch.cuda.synchronize()
    # every buffer the kernels are handed (save, d_logit) full of NaN: they write all they read
    real_empty = torch.empty

    def poisoned(*a, **k):
        x = real_empty(*a, **k)
        return x.fill_(float("nan")) if x.is_floating_point() else x

    monkeypatch.setattr(torch, "empty", poisoned)
    poison = _run(kind, t, save=torch.full((5 * B + 1,), float("nan"), device=DEV))
    monkeypatch.undo()
    torch.cuda.synchronize()
    for other in (second, beside, poison):
        _equal(first, other)
    assert bool(torch.isfinite(first[0])) and bool(torch.isfinite(first[1]).all())
    # accumulate: the gradient is ADDED to an existing one (rows cross-entropy ignores stay as they were), scaled by *gout
    base = torch.from_numpy(synth.debias_case(B, t["logits"].shape[1], 0, 77)["logits"]).to(DEV)
    gout = torch.full((), 0.5, device=DEV)
    half = _run(kind, t, gout=gout)
    added = _run(kind, t, gout=gout, d_logit=base.clone())
    torch.cuda.synchronize()
    assert torch.equal(added[1], base + half[1])
    assert rel_err(half[1], 0.5 * first[1]) <= 1e-6


def test_the_loss_classes_run_the_fused_kernels_stand_alone(golden):
    """the public classes outside a model, through autograd: the same bits as the ops level"""
    from xggm_amd.module.answer_losses import CrossEntropy
    from xggm_amd.module.answer_losses import Focal
    g, _ = golden
    t = _inputs(golden, "e")
    classes = torch.from_numpy(g["e.ce.labels"]).to(DEV)
    table = torch.cat([t["bias"][3:], t["bias"][:3]])
    idx = torch.tensor([2, 3, 4, 0, 1], device=DEV)
    runs = [
        (lambda z: Focal()(None, z, t["bias"], t["labels"]), _run("focal", t)),
        (lambda z: Focal().set_bias_table(table.cpu()).to(DEV)(None, z, None, t["labels"], bias_index=idx), _run("focal", t)),
        (lambda z: CrossEntropy()(None, z, None, t["labels"]), _run("ce", t)),
        (lambda z: CrossEntropy(scale=3.0)(None, z, None, classes), _run("ce", t, scale=3.0)),
    ]
    for fn, want in runs:
        z = t["logits"].clone().requires_grad_(True)
        loss = fn(z)
        assert loss.dim() == 0
        loss.backward()
        torch.cuda.synchronize()
        assert torch.equal(loss.detach(), want[0]) and torch.equal(z.grad, want[1])
    with pytest.raises(ValueError, match="no bias given"):
        Focal()(None, t["logits"], None, t["labels"])
    with pytest.raises(ValueError):
        CrossEntropy()(None, t["logits"], None, classes[:3])


# ----------------------------------------------------------------------------- the model level (tiny configuration)
B, A, T_TOTAL = 4, 29, 40


def _loss(kind):
    from xggm_amd.module.answer_losses import CrossEntropy
    from xggm_amd.module.answer_losses import Focal
    if kind == "ce":
        return CrossEntropy()
    return Focal().set_bias_table(synth.debias_case(3, A, 0, 31)["bias"])


def _tiny(dtype, kind):
    """the ``_tiny`` recipe of tests/test_debias_gpu.py with ``kind`` in ("ce", "focal", None) attached"""
    from oracle import shapes
    from xggm_amd import param
    from xggm_amd.lxrt.modeling import BertConfig, VISUAL_CONFIG
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
    if kind is not None:
        attach_debias_loss(m, _loss(kind))
    return cfg, m, make_optimizer(m, 1e-4, T_TOTAL)


def _batches(cfg, kind):
    out = []
    for s in (3, 4, 5, 6):
        b = batch_tensors(synth.vqa_batch(B, A=A, F=cfg["feat_dim"], vocab=cfg["vocab"], seed=s), DEV)
        if kind == "focal":
            b["bias_index"] = torch.tensor([(s + i) % 3 for i in range(B)], device=DEV)
        out.append(b)
    out[1]["target"][1].zero_()  # a question whose answer is outside the vocabulary: cross-entropy ignores the row
    return out


def _eager_batch(x):
    return dict(x, sent=(x["input_ids"], x["input_mask"], x["segment_ids"]))


def _cpu_dlogit(kind, logit, batch, table):
    """d loss / d logits by torch on the CPU in float64, from the pass's own logits"""
    z = logit.detach().double().cpu().requires_grad_(True)
    y = batch["target"].double().cpu()
    if kind == "ce":
        mx, arg = y.max(1)
        loss = torch.nn.functional.cross_entropy(z, torch.where(mx > 0, arg, torch.full_like(arg, IGNORE)), ignore_index=IGNORE)
    else:
        b = table.double().cpu()[batch["bias_index"].cpu()]
        f = torch.log(torch.softmax(z, 1) + 1e-5) * (1 - torch.softmax(b, 1)) ** 2
        loss = torch.nn.functional.binary_cross_entropy_with_logits(f, y) * y.size(1)
    loss.backward()
    return loss.detach(), z.grad


@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("kind", ["ce", "focal"])
def test_an_eager_plain_pass_feeds_the_head_with_the_loss_gradient(kind, dt):
    """wiring and scale: after one plain pass ``logit_fc.3.bias.grad`` is the column sum of d loss / d logits, which torch
    computes on the CPU from the logits the pass returned.  Bound: the project's bar of the compute dtype -- the kernel's
    d_logit meets the fp32 bar (parity test), the sum over B = 4 rows adds a few ulp, and a bf16 model rounds the gradient
    that enters the head's backward to bf16 (2^-9 per element)."""
    from xggm_amd.vqa.vqacpv2 import BCEWithLogitsLoss, forward_backward_plain
    cfg, m, _ = _tiny(dt, kind)
    m.eval()  # dropout off: the returned logits are those the loss saw either way; this keeps the pass reproducible
    b = _batches(cfg, kind)[1]
    loss, logit = forward_backward_plain(m, BCEWithLogitsLoss(), b["feats"], b["boxes"],
                                         (b["input_ids"], b["input_mask"], b["segment_ids"]), b["target"],
                                         bias_index=b.get("bias_index"))
    torch.cuda.synchronize()
    assert logit.dtype == F32 and tuple(logit.shape) == (B, A)
    want_loss, d = _cpu_dlogit(kind, logit, b, getattr(m.debias_loss, "bias_table", None))
    if kind == "ce":
        assert not d[1].any() and d[0].any()
    got = dict(m.named_parameters())["logit_fc.3.bias"].grad
    err_loss, err = abs(float(loss) - float(want_loss)) / abs(float(want_loss)), rel_err(got, d.sum(0))
    print("%s %s: loss %.9g (torch %.9g, rel %.2e), logit_fc.3.bias.grad rel_err %.3e (bound %.1e)"
          % (kind, dt, float(loss), float(want_loss), err_loss, err, tol(dt)))
    assert err_loss <= tol(F32)  # the loss kernel reads fp32 logits under either compute dtype
    assert err <= tol(dt)


def _state(m):
    from xggm_amd.runtime import runtime_of
    rt = runtime_of(m)
    arena = rt.arena
    st = {k: getattr(arena, k).clone() for k in ("params", "m", "v", "shadow") if getattr(arena, k) is not None}
    st["steps"], st["lr_scale"], st["rng"] = arena.steps.clone(), arena.lr_scale.clone(), rt.rng.clone()
    return st


BRANCHES = ("rel", "node")


@pytest.mark.parametrize("kind,order", [("ce", "gqa"), ("ce", "vqa"), ("focal", "vqa"), ("focal", "gqa")])
def test_captured_replay_equals_eager_iterations(kind, order):
    """bf16, two iterations (rel, node) with a TrainLog: replayed from ``CapturedTrainer`` graphs and through the eager
    ``train_iteration`` (behind the trainer's warm-up passes, run by hand) -- the same bits in the losses, the weights, the
    moments and the log; the log's BCE column is the attached loss (the whole loss of a plain pass)."""
    from xggm_amd.engine import CapturedTrainer, TrainLog
    from xggm_amd.vqa.vqacpv2 import train_iteration
    runs = {}
    for name in ("captured", "eager"):
        cfg, m, o = _tiny(BF16, kind)
        assert [k for k in m.state_dict() if k.startswith("debias_loss.")] == (["debias_loss.bias_table"] if kind == "focal" else [])
        b = _batches(cfg, kind)
        log = TrainLog(8, DEV)
        t = CapturedTrainer(m, o, b[0], sigma=1.0, order=order, warmup_iters=1, use_graph=name == "captured",
                            train_log=log if name == "captured" else None)
        if name == "eager":
            for p in ("plain", "rel", "node"):  # the constructor's warm-up passes, by hand
                t._eager_pass(p)
        losses = []
        for i, br in enumerate(BRANCHES):
            if name == "captured":
                t.load_batch(b[i + 1])
                (lp, _, _), (lg, _, _) = t.iteration(br)
                losses.append((float(lp), float(lg)))
            else:
                r = train_iteration(m, o, t.bce, _eager_batch(b[i + 1]), sigma=1.0, order=order, branch=br, clip=5.0, train_log=log)
                losses.append((float(r["loss_plain"]), float(r["loss_ggm"])))
        torch.cuda.synchronize()
        assert "debias_loss" not in m.arena().group_index  # no parameters: no arena group
        runs[name] = dict(state=_state(m), log=log, losses=losses)
    cap, eag = runs["captured"], runs["eager"]
    assert cap["losses"] == eag["losses"] and all(np.isfinite(x) for pair in cap["losses"] for x in pair), (cap["losses"], eag["losses"])
    assert sorted(cap["state"]) == sorted(eag["state"])
    for k in cap["state"]:
        assert torch.equal(cap["state"][k], eag["state"][k]), k
    assert torch.equal(cap["log"].buf, eag["log"].buf)
    rec = cap["log"].read()
    assert int(rec["cursor"]) == 4 and int(rec["first_bad"]) == -1
    v, kinds = rec["values"].numpy(), rec["kinds"].numpy()
    assert (v[:, TrainLog.BCE] > 0).all() and np.isfinite(v).all()
    plain = kinds == TrainLog.PLAIN
    assert list(plain) == ([True, False] * 2 if order == "vqa" else [False, True] * 2)
    assert np.array_equal(v[plain, TrainLog.BCE], v[plain, TrainLog.LOSS])  # the plain pass's loss IS the attached loss
    assert [float(x) for x in v[plain, TrainLog.LOSS]] == [lp for lp, _ in cap["losses"]]
    assert [float(x) for x in v[~plain, TrainLog.LOSS]] == [lg for _, lg in cap["losses"]]
    assert (v[~plain, TrainLog.BCE] < v[~plain, TrainLog.LOSS]).all()


@pytest.mark.parametrize("kind", ["ce", "focal"])
def test_the_bce_column_is_the_loss_term_the_pass_returns(kind):
    from xggm_amd.engine import TrainLog
    from xggm_amd.vqa.vqacpv2 import BCEWithLogitsLoss, ggm_pass
    cfg, m, o = _tiny(BF16, kind)
    b = _batches(cfg, kind)[2]
    log = TrainLog(4, DEV)
    loss, _, terms = ggm_pass(m, o, BCEWithLogitsLoss(), b["feats"], b["boxes"], (b["input_ids"], b["input_mask"], b["segment_ids"]),
                              b["target"], b["adj_true"], "rel", train_log=log, bias_index=b.get("bias_index"))
    rec = log.read()
    v = rec["values"].numpy()
    assert int(rec["cursor"]) == 1
    assert float(v[0, TrainLog.BCE]) == float(terms["bce"]) == float(terms["bce"].t) and float(v[0, TrainLog.LOSS]) == float(loss)
    assert 0 < float(v[0, TrainLog.BCE]) < float(loss)


def _calls_of_a_pass(kind, attach):
    """the C-ABI calls of one eager plain pass and one eager relation pass of the tiny model, in order"""
    from xggm_amd import ops
    from xggm_amd.engine import CapturedTrainer
    cfg, m, o = _tiny(BF16, attach)
    t = CapturedTrainer(m, o, _batches(cfg, attach)[0], sigma=1.0, use_graph=False)
    t.iteration("rel")  # first use: workspaces, caches
    seen, real = [], ops.call

    def spy(fn, *a):
        seen.append(fn)
        return real(fn, *a)

    ops.call = spy
    try:
        t._eager_pass(kind)
    finally:
        ops.call = real
    torch.cuda.synchronize()
    return seen


@pytest.mark.parametrize("kind", ["plain", "rel"])
def test_nothing_attached_launches_what_it_did_and_an_attached_loss_only_swaps_the_pair(kind):
    """With nothing attached a pass makes no call of the new entry points: its head loss is the BCE pair, one call each.
    The passes' own code has no branch on the new classes, so the call sequence with ``CrossEntropy`` / ``Focal`` attached
    is the unattached one with exactly that pair replaced -- nothing is added before, between or behind."""
    bare = _calls_of_a_pass(kind, None)
    assert not [c for c in bare if "softmax_loss" in c or "debias" in c]
    assert bare.count("xggm_bce_fwd") == 1 and bare.count("xggm_bce_bwd_f32") == 1
    swap = {"xggm_bce_fwd": "xggm_softmax_loss_fwd_f32", "xggm_bce_bwd_f32": "xggm_softmax_loss_bwd_f32"}
    for attach in ("ce", "focal"):
        got = _calls_of_a_pass(kind, attach)
        assert got == [swap.get(c, c) for c in bare], attach


@pytest.mark.parametrize("kind", ["ce", "focal"])
def test_no_framework_kernel_inside_a_training_pass(kind):
    """as tests/test_engine_gpu.py::test_no_framework_kernel_inside_a_training_pass, with the loss attached: every device
    kernel of the plain, the relation and the node pass is one of the package's own"""
    if os.environ.get("XGGM_POISON_EMPTY"):
        pytest.skip("the poisoned torch.empty of conftest.py fills every buffer with a framework kernel")
    from torch.profiler import ProfilerActivity, profile
    from xggm_amd import ops
    from xggm_amd.engine import CapturedTrainer
    cfg, m, o = _tiny(BF16, kind)
    tr = CapturedTrainer(m, o, _batches(cfg, kind)[0], sigma=1.0, order="vqa", use_graph=False)
    tr.iteration("rel")
    tr.iteration("node")
    torch.cuda.synchronize()
    seen, real = [], ops.call

    def spy(fn, *a):
        seen.append(fn)
        return real(fn, *a)

    ops.call = spy
    try:
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA], record_shapes=True) as prof:
            tr.iteration("rel")
            tr.iteration("node")
            torch.cuda.synchronize()
    finally:
        ops.call = real
    bad = []
    for ev in prof.events():
        if ev.name.startswith("aten::") and any(k.name for k in ev.kernels):
            bad.append((ev.name, str(ev.input_shapes)[:60], [k.name[:50] for k in ev.kernels][:2]))
    assert not bad, bad[:8]
    # four passes, each with the attached loss's forward and backward and no BCE pair
    assert seen.count("xggm_softmax_loss_fwd_f32") == 4 and seen.count("xggm_softmax_loss_bwd_f32") == 4
    assert not [c for c in seen if c.startswith("xggm_bce")]


def test_the_packed_hand_over_takes_cross_entropy_and_refuses_focal():
    from xggm_amd.engine import CapturedTrainer
    for kind in ("ce", "focal"):
        cfg, m, o = _tiny(BF16, kind)
        b = _batches(cfg, kind)[0]
        spec = dict(feats=(tuple(b["feats"].shape), b["feats"].dtype), boxes=(tuple(b["boxes"].shape), b["boxes"].dtype),
                    ids=((3,) + tuple(b["input_ids"].shape), b["input_ids"].dtype),
                    target=(tuple(b["target"].shape), b["target"].dtype), adj=(tuple(b["adj_true"].shape), b["adj_true"].dtype))
        if kind == "focal":
            with pytest.raises(ValueError, match="packed_spec carries no bias"):
                CapturedTrainer(m, o, b, packed_spec=spec, use_graph=False)
            continue
        t = CapturedTrainer(m, o, b, packed_spec=spec, use_graph=False)
        assert t.static_flat is not None and torch.equal(t.static["target"], b["target"])
        loss, logit, total = t._eager_pass("plain")
        torch.cuda.synchronize()
        assert bool(torch.isfinite(loss)) and float(total) > 0
