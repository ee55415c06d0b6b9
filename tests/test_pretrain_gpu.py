"""The pre-training losses on the GPU: ``mlm_select`` against ``torch.nonzero``, the vocabulary cross-entropy and the
object losses against the float64 restatement of tests/pretrain_ref.py (itself pinned to the reference's recorded results by
tests/test_pretrain_cpu.py), exact zeros where the contract promises them, bit-equality across runs.

Tolerances are the project's (``test_kernels_gpu.tol``: 2e-5 in fp32, 1.2e-2 in bf16): a loss relative to its value,
``rel_err`` on a gradient.  bf16 inputs reach the restatement as the bf16 values the kernel reads."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import rel_err  # noqa: E402
from test_kernels_gpu import tol  # noqa: E402
import pretrain_ref as R  # noqa: E402

DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from xggm_amd import ops as o
    return o


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _i32(v):
    return torch.tensor([v], dtype=torch.int32, device=DEV)


def _one(v=1.0):
    return torch.full((), v, device=DEV)


def _loss_err(got, want):
    return abs(got - want) / abs(want) if want != 0.0 else abs(got)


# ------------------------------------------------------------------------------------------------ mlm_select
V_SEL = 50
SELECT_CASES = {
    "one_row_unlabelled": (1, [], 4),
    "one_row_labelled": (1, [0], 4),
    "across_a_scan_chunk": (257, [0, 255, 256], 8),
    "all_rows": (70, list(range(70)), 70),
    "no_rows": (300, [], 5),
    "n_equals_cap": (600, [1, 63, 64, 255, 256, 511, 599], 7),
    "n_is_cap_plus_one": (600, [1, 63, 64, 255, 256, 511, 598, 599], 7),
}


def _select_inputs(M, rows, dt, seed=3):
    labels = torch.full((M,), -1, dtype=torch.int64)
    for i, r in enumerate(rows):
        labels[r] = (0, V_SEL - 1)[i % 2] if i < 2 else (7 * r + 3) % V_SEL
    x = torch.randn((M, 8), generator=_gen(seed)).to(dt)
    return labels, x


@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("name", list(SELECT_CASES))
def test_mlm_select(ops, name, dt):
    M, rows, cap = SELECT_CASES[name]
    labels, x = _select_inputs(M, rows, dt)
    want = R.mlm_select(labels, x, cap, V_SEL)
    nz = torch.nonzero(labels != -1).reshape(-1)
    assert want["row_index"][:want["n"]].tolist() == nz[:cap].tolist()  # the restatement is torch.nonzero's order
    runs = []
    for _ in range(2):
        sel = ops.mlm_select(labels.to(DEV), x.to(DEV), cap, V_SEL)
        runs.append([t.cpu() for t in (sel.row_index, sel.label, sel.n, sel.overflow, sel.x)])
    torch.cuda.synchronize()
    ri, lab, n, over, out = runs[0]
    print("%s %s: n %d (want %d) overflow %d (want %d) rows %s" % (name, dt, int(n), want["n"], int(over), want["overflow"],
                                                                  ri.tolist()[:8]))
    assert int(n) == want["n"] and int(over) == want["overflow"]
    assert torch.equal(ri, want["row_index"]) and torch.equal(lab, want["label"])
    assert torch.equal(out, want["x"])                 # the rows themselves, bit for bit
    assert not out[int(n):].any()                      # and an exactly zero tail
    for a, b in zip(runs[0], runs[1]):
        assert torch.equal(a, b)
    # the gather's backward puts the rows back and zeroes the rest
    back = ops.mlm_scatter(sel, sel.x).cpu()
    ref = torch.zeros_like(x)
    ref[ri[:int(n)].long()] = x[ri[:int(n)].long()]
    assert torch.equal(back, ref)


def test_mlm_select_ignores_labels_outside_the_vocabulary(ops):
    """the rule of XGGM_SOFTMAX_CE: a label that is neither ignore_index nor in [0, V) cannot be refused from the host; the
    row does not count"""
    labels = torch.tensor([-1, 3, V_SEL, -7, V_SEL - 1, 10 ** 12], dtype=torch.int64)
    x = torch.randn((6, 8), generator=_gen(1))
    sel = ops.mlm_select(labels.to(DEV), x.to(DEV), 6, V_SEL)
    assert int(sel.n) == 2 and sel.row_index.tolist()[:2] == [1, 4] and sel.label.tolist()[:2] == [3, V_SEL - 1]


def test_overflow_turns_the_loss_into_nan(ops):
    M, rows, cap = SELECT_CASES["n_is_cap_plus_one"]
    labels, x = _select_inputs(M, rows, F32)
    sel = ops.mlm_select(labels.to(DEV), x.to(DEV), cap, V_SEL)
    ld = ops.vocab_ld(V_SEL, F32)
    z = torch.randn((cap, ld), generator=_gen(5)).to(DEV)
    loss, pr = ops.vocab_ce_fwd(z, sel.label, sel.n, V_SEL, overflow=sel.overflow)
    assert int(sel.overflow) == 1 and int(sel.n) == cap and math.isnan(float(loss))
    # the same list without the flag is a finite loss over the first cap rows
    loss2, _ = ops.vocab_ce_fwd(z, sel.label, sel.n, V_SEL)
    want, _ = R.vocab_ce(z[:, :V_SEL], sel.label, cap)
    assert _loss_err(float(loss2), want) <= tol(F32)


# ------------------------------------------------------------------------------------------------ vocab_ce
def _vocab_case(ops, V, cap, dt, seed):
    """padded logits (NaN in the padding columns: never read), labels that include 0 and V - 1"""
    ld = ops.vocab_ld(V, dt)
    z = (torch.randn((cap, ld), generator=_gen(seed)) * 3.0).to(dt)
    z[:, V:] = float("nan")
    label = torch.randint(0, V, (cap,), generator=_gen(seed + 1)).to(torch.int32)
    label[0] = 0
    label[-1] = V - 1
    if cap > 2:
        label[1] = V - 1
    return z, label, ld


def _check_vocab(ops, V, cap, ns, dt, seed):
    z, label, ld = _vocab_case(ops, V, cap, dt, seed)
    for n in ns:
        outs = []
        for _ in range(2):
            zd = z.to(DEV)
            loss, pr = ops.vocab_ce_fwd(zd, label.to(DEV), _i32(n), V)
            d = ops.vocab_ce_bwd(pr, _one(0.75))
            assert d.data_ptr() == zd.data_ptr() and d.dtype == dt  # in place, in the logits' type
            outs.append((loss.cpu(), d.cpu()))
        torch.cuda.synchronize()
        (loss, d), (loss_b, d_b) = outs
        want, want_d = R.vocab_ce(z[:, :V], label, n, gout=0.75)
        assert torch.equal(d, d_b) and (torch.equal(loss, loss_b) or n == 0)
        assert not d[n:].any() and not d[:, V:].any()  # exact zeros: rows >= n, padding columns
        if n == 0:
            print("V=%d cap=%d n=0 %s: loss %r" % (V, cap, dt, float(loss)))
            assert math.isnan(float(loss)) and not d.any()
            continue
        e_loss, e_d = _loss_err(float(loss), want), rel_err(d[:, :V], want_d)
        print("V=%d cap=%d n=%d %s: loss %.9g (restatement %.9g, rel %.2e)  d rel_err %.3e  (bound %.1e)"
              % (V, cap, n, dt, float(loss), want, e_loss, e_d, tol(dt)))
        assert bool(torch.isfinite(d).all())
        assert e_loss <= tol(dt)
        assert e_d <= tol(dt)


@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("V", [1, 5, 263, 4097, 30522, 32768, 32769])
def test_vocab_ce_widths(ops, V, dt):
    """three rows of every width class: one partial chunk, the tiny golden vocabulary, past one pass of the workgroup,
    BERT's vocabulary, the register-resident limit and the first width that is folded online"""
    assert ops.VOCAB_CE_REG_MAX == 32768
    _check_vocab(ops, V, 3, (0, 2, 3), dt, seed=V)


@pytest.mark.parametrize("dt", [F32, BF16])
def test_vocab_ce_many_rows(ops, dt):
    _check_vocab(ops, 64, 130, (130, 77), dt, seed=11)


def test_vocab_ce_walks_rows_past_its_grid(ops):
    """more rows than the forward has workgroups (1024) and the backward (2048): a workgroup's rows add up in row order"""
    _check_vocab(ops, 12, max(ops.VOCAB_CE_FWD_GRID, ops.VOCAB_CE_BWD_GRID) + 3, (max(ops.VOCAB_CE_FWD_GRID, ops.VOCAB_CE_BWD_GRID) + 3,), F32, seed=13)


# ------------------------------------------------------------------------------------------------ visual_loss
def _visual_jobs(R_, widths, dt, seed, conf_zero=False):
    """(kind, scores, label, conf, weight) per width: 'ce' for all but 2048 / 7-wide 'l2' jobs named by a leading 'l'"""
    jobs = []
    for q, (kind, W) in enumerate(widths):
        g = _gen(seed + q)
        s = (torch.randn((R_, W), generator=g) * 2.0).to(dt)
        conf = torch.rand((R_,), generator=g)
        if R_ > 1:
            conf[R_ // 2] = 0.0
        if conf_zero:
            conf.zero_()
        if kind == "ce":
            label = torch.randint(0, W, (R_,), generator=g)
            label[0] = W - 1
            if R_ > 1:
                label[1] = -1  # ignored, its confidence is positive
        else:
            d = torch.randn((R_, W), generator=g) * 1.5
            edge = torch.tensor([0.5, -0.5, 1.0, -1.0, 1.5, -2.0, 0.0])
            d[0, :min(W, 7)] = edge[:min(W, 7)]
            label = (s.float() - d).contiguous()
            label[0, :min(W, 7)] = s[0, :min(W, 7)].float() - edge[:min(W, 7)]
        jobs.append((kind, s, label, conf, 1.0 / 0.15 if q != 1 else 0.5))
    return jobs


def _check_visual(ops, R_, widths, dt, seed, conf_zero=False):
    jobs = _visual_jobs(R_, widths, dt, seed, conf_zero)
    kinds = dict(ce=ops.VISUAL_CE, l2=ops.VISUAL_L2)
    dev_jobs = [(kinds[k], s.to(DEV), lab.to(DEV), c.to(DEV), w) for k, s, lab, c, w in jobs]
    outs = []
    for _ in range(2):
        losses, pr = ops.visual_loss_fwd(dev_jobs)
        ds = ops.visual_loss_bwd(pr, _one(1.25))
        outs.append((losses.cpu(), [d.cpu() for d in ds]))
    torch.cuda.synchronize()
    want, want_d = R.visual_losses(jobs, gout=1.25)
    (losses, ds), (losses_b, ds_b) = outs
    assert torch.equal(losses, losses_b) and all(torch.equal(a, b) for a, b in zip(ds, ds_b))
    for q, (kind, s, lab, conf, w) in enumerate(jobs):
        assert ds[q].dtype == dt and ds[q].shape == s.shape
        dead = conf == 0
        if kind == "ce":
            dead = dead | (lab == -1)
        assert not ds[q][dead].any()  # exactly zero, not small
        e_loss, e_d = _loss_err(float(losses[q]), want[q]), rel_err(ds[q], want_d[q])
        print("R=%d %s W=%d %s: loss %.9g (restatement %.9g, rel %.2e)  d rel_err %.3e  (bound %.1e)"
              % (R_, kind, s.shape[1], dt, float(losses[q]), want[q], e_loss, e_d, tol(dt)))
        assert bool(torch.isfinite(ds[q]).all())
        if conf_zero:
            assert float(losses[q]) == 0.0 and want[q] == 0.0 and not ds[q].any()
            continue
        assert e_loss <= tol(dt)
        assert e_d <= tol(dt)


PRETRAIN_WIDTHS = [("ce", 1600), ("ce", 400), ("l2", 2048)]


@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("R_", [1, 2, 37])
def test_visual_loss_pretraining_widths(ops, R_, dt):
    _check_visual(ops, R_, PRETRAIN_WIDTHS, dt, seed=100 + R_)


@pytest.mark.parametrize("dt", [F32, BF16])
def test_visual_loss_rows_past_the_ticket_grid(ops, dt):
    """width 7 (no vector access, one partial chunk) on more rows than workgroups"""
    _check_visual(ops, ops.VISUAL_LOSS_GRID + 1, [("ce", 7), ("l2", 7)], dt, seed=7)


@pytest.mark.parametrize("widths", [[("l2", 2048)], [("ce", 1600), ("l2", 2048)], [("ce", 400)]])
def test_visual_loss_subsets(ops, widths):
    """--visualLosses may name any subset: one-job and two-job launches"""
    _check_visual(ops, 5, widths, F32, seed=21)


@pytest.mark.parametrize("dt", [F32, BF16])
def test_visual_loss_all_confidences_zero(ops, dt):
    _check_visual(ops, 9, PRETRAIN_WIDTHS, dt, seed=31, conf_zero=True)


def test_visual_loss_smooth_l1_on_both_sides_of_one(ops):
    """|d| = 0.5, 1 exactly, 1.5 and 2 in one row: the quadratic branch below 1, the linear one from 1 on; d_score is
    clamp(d, -1, 1) scaled"""
    s = torch.zeros((1, 8))
    y = -torch.tensor([[0.5, -0.5, 1.0, -1.0, 1.5, -2.0, 0.0, 0.999]])
    conf = torch.ones(1)
    losses, pr = ops.visual_loss_fwd([(ops.VISUAL_L2, s.to(DEV), y.to(DEV), conf.to(DEV), 1.0)])
    (d,) = ops.visual_loss_bwd(pr, _one())
    want = (0.125 + 0.125 + 0.5 + 0.5 + 1.0 + 1.5 + 0.0 + 0.5 * 0.999 ** 2) / 8
    assert abs(float(losses[0]) - want) <= tol(F32) * want
    want_d = torch.tensor([[0.5, -0.5, 1.0, -1.0, 1.0, -1.0, 0.0, 0.999]]) / 8
    assert rel_err(d, want_d) <= tol(F32)


# ------------------------------------------------------------------------------------------------ the decoder path
def _decoder_case(M, H, V, rows, dt, seed):
    g = _gen(seed)
    labels = torch.full((M,), -1, dtype=torch.int64)
    for i, r in enumerate(rows):
        labels[r] = (0, V - 1)[i % 2] if i < 2 else (5 * r + 1) % V
    x = torch.randn((M, H), generator=g).to(dt)
    w = (torch.randn((V, H), generator=g) * 0.3).to(dt)
    bias = torch.randn((V,), generator=g) * 0.1
    return labels, x, w, bias


def _decoder_ref(labels, x, w, bias, gout):
    """float64: logits of ALL rows, torch's CrossEntropyLoss(ignore_index=-1), gradients by autograd"""
    import torch.nn.functional as F
    xd, wd, bd = (t.double().clone().requires_grad_(True) for t in (x, w, bias))
    loss = F.cross_entropy(xd @ wd.t() + bd, labels, ignore_index=-1)
    gx, gw, gb = torch.autograd.grad(loss * gout, [xd, wd, bd])
    return float(loss.detach()), gx, gw, gb


def _decoder_run(ops, labels, x, w, bias, capacity, gout):
    from xggm_amd import pretrain_heads as PH
    M, H = x.shape
    V = w.shape[0]
    cap = PH.mlm_capacity(M, capacity)
    sel = ops.mlm_select(labels.to(DEV), x.to(DEV), cap, V)
    loss, st = PH.mlm_decoder_fwd(sel, sel.x, w.to(DEV), bias.to(DEV))
    g_table = torch.empty((V, H), device=DEV)
    g_bias = torch.zeros(V, device=DEV)
    d_t = PH.mlm_decoder_bwd(st, _one(gout), g_table, False, g_bias)
    d_x = ops.mlm_scatter(sel, d_t)
    assert st.logits.shape == (cap, ops.vocab_ld(V, x.dtype)) and st.logits.dtype == x.dtype
    return loss.cpu(), d_x.cpu(), g_table.cpu(), g_bias.cpu(), sel


@pytest.mark.parametrize("dt", [F32, BF16])
def test_masked_lm_decoder_path(ops, dt):
    """select -> tied decoder -> cross-entropy -> dgrad / wgrad / bias gradient -> scatter, against torch's loss over ALL
    rows in float64: a sample without a masked token, labels 0 and V - 1, capacity None and a tight one bit-identical"""
    M, H, V = 24, 128, 263
    rows = [1, 6, 9, 10, 23]  # rows 16 ... 22 (a whole sample of 8) carry no label
    labels, x, w, bias = _decoder_case(M, H, V, rows, dt, seed=17)
    want, gx, gw, gb = _decoder_ref(labels, x, w, bias, 0.5)
    full = _decoder_run(ops, labels, x, w, bias, None, 0.5)
    tight = _decoder_run(ops, labels, x, w, bias, len(rows), 0.5)
    again = _decoder_run(ops, labels, x, w, bias, len(rows), 0.5)
    torch.cuda.synchronize()
    loss, d_x, g_table, g_bias, sel = full
    errs = (_loss_err(float(loss), want), rel_err(d_x, gx), rel_err(g_table, gw), rel_err(g_bias, gb))
    print("decoder path %s: loss %.9g (float64 %.9g, rel %.2e)  d_x %.3e  d_table %.3e  d_bias %.3e  (bound %.1e)"
          % ((dt, float(loss), want) + errs + (tol(dt),)))
    assert int(sel.overflow) == 0 and int(sel.n) == len(rows)
    assert all(e <= tol(dt) for e in errs)
    keep = torch.zeros(M, dtype=torch.bool)
    keep[rows] = True
    assert not d_x[~keep].any()  # rows without a label get exact zeros
    for a, b in zip(full[:4], tight[:4]):
        assert torch.equal(a, b)  # the capacity changes the row count of the products, not one bit of the result
    for a, b in zip(tight[:4], again[:4]):
        assert torch.equal(a, b)
    # one slot too few: the flag is up and the loss is NaN
    short = _decoder_run(ops, labels, x, w, bias, len(rows) - 1, 0.5)
    assert int(short[4].overflow) == 1 and math.isnan(float(short[0]))


# ------------------------------------------------------------------------------------------------ the reference's own numbers
@pytest.mark.parametrize("case", ["full", "noqa"])
def test_kernels_against_the_reference_recorded_losses(ops, case):
    """tests/golden/pretrain.npz (the reference's LXRTPretraining in float64): the head transforms run in float64 on the
    host (tests/pretrain_ref.py) from the recorded encoder outputs, the decoder product and every loss kernel on the GPU in
    fp32.  Compared with what the reference recorded: the masked-LM loss and the gradient of cls.predictions.bias (the
    column sums of the in-place logit gradient), each object loss and the gradient of its decoder weight (d_score^T h)."""
    import json
    import os
    from helpers import GOLDEN, load_golden
    from xggm_amd import pretrain_heads as PH, synth
    g = load_golden("pretrain")
    meta = json.loads(str(g["meta_json"]))
    cfg, c = meta["cfg"], meta["cases"][case]
    x = synth.pretrain_case(cfg["B"], cfg["T"], cfg["O"], cfg["F"], cfg["vocab"], cfg["n_obj"], cfg["n_attr"], cfg["n_ans"],
                            seed=meta["seed"])
    names = json.load(open(os.path.join(GOLDEN, "pretrain_state_dict.json")))[case]
    tied = "bert.embeddings.word_embeddings.weight"
    P = {k: torch.from_numpy(synth.seeded_param(tied if k == "cls.predictions.decoder.weight" else k, shp, meta["seed"])).double()
         for k, shp in names.items() if not k.startswith("bert.")}
    want = g[case + ".losses"]
    H, V = cfg["hidden"], cfg["vocab"]
    # masked-LM: select on the device, transform of the selected rows on the host, decoder + loss + gradients on the device
    lang = torch.from_numpy(g[case + ".lang_output"]).reshape(-1, H)
    labels = torch.from_numpy(x["masked_lm_labels"]).reshape(-1)
    sel = ops.mlm_select(labels.to(DEV), lang.float().to(DEV), PH.mlm_capacity(lang.shape[0], 6), V)
    t = R.transform(sel.x.cpu().double(), P, "cls.predictions.transform.").float().to(DEV)
    loss, st = PH.mlm_decoder_fwd(sel, t, P["cls.predictions.decoder.weight"].float().to(DEV), P["cls.predictions.bias"].float().to(DEV))
    g_table, g_bias = torch.empty((V, H), device=DEV), torch.zeros(V, device=DEV)
    PH.mlm_decoder_bwd(st, _one(), g_table, False, g_bias)
    errs = {"masked_lm": _loss_err(float(loss), float(want[0])),
            "grad.cls.predictions.bias": rel_err(g_bias, torch.from_numpy(g[case + ".grad.cls.predictions.bias"]))}
    assert int(sel.n) == int((labels != -1).sum()) <= 6 and int(sel.overflow) == 0
    # object losses: scores on the host, the losses and d_score on the device
    keys = c["visual_losses"].split(",")
    h = R.transform(torch.from_numpy(g[case + ".visn_output"]).reshape(-1, H), P, "obj_predict_head.transform.")
    kinds = dict(obj=ops.VISUAL_CE, attr=ops.VISUAL_CE, feat=ops.VISUAL_L2)
    jobs = []
    for k in keys:
        s = h @ P["obj_predict_head.decoder_dict.%s.weight" % k].t() + P["obj_predict_head.decoder_dict.%s.bias" % k]
        lab = torch.from_numpy(x[k + "_label"])
        lab = lab.reshape(-1) if k != "feat" else lab.reshape(-1, cfg["F"]).contiguous()
        jobs.append((kinds[k], s.float().to(DEV), lab.to(DEV), torch.from_numpy(x[k + "_conf"]).reshape(-1).to(DEV), 1 / 0.15))
    losses, pr = ops.visual_loss_fwd(jobs)
    ds = ops.visual_loss_bwd(pr, _one())
    torch.cuda.synchronize()
    for q, k in enumerate(keys):
        errs[k] = _loss_err(float(losses[q]), float(want[2 + q]))
        name = "obj_predict_head.decoder_dict.%s.weight" % k
        errs["grad." + name] = rel_err(ds[q].cpu().double().t() @ h, torch.from_numpy(g["%s.grad.%s" % (case, name)]))
    print(case, {k: "%.1e" % v for k, v in errs.items()}, "(bound %.1e)" % tol(F32))
    assert max(errs.values()) <= tol(F32), errs
