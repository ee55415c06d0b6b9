"""Float64 restatement of the pre-training heads and losses of LXRTPretraining (src/lxrt/modeling.py:623-715, :1009-1061):
tensors in, losses and gradients out, all on the CPU through torch autograd.  tests/test_pretrain_cpu.py pins it to what the
reference itself recorded (tests/golden/pretrain.npz); the GPU tests compare kernels at sizes no fixture stores with it."""
import math

import torch
import torch.nn.functional as F

IGNORE = -1


def mlm_select(labels, x, cap, V, ignore_index=IGNORE):
    """-> dict(row_index, label (int32 [cap], -1 behind n), n, overflow, x [cap, H] zero-filled behind n)"""
    labels = labels.reshape(-1).cpu()
    keep = (labels != ignore_index) & (labels >= 0) & (labels < V)
    rows = torch.nonzero(keep).reshape(-1)
    n = min(int(rows.numel()), cap)
    row_index = torch.full((cap,), -1, dtype=torch.int32)
    label = torch.full((cap,), -1, dtype=torch.int32)
    row_index[:n] = rows[:n].to(torch.int32)
    label[:n] = labels[rows[:n]].to(torch.int32)
    out = torch.zeros((cap, x.shape[1]), dtype=x.dtype)
    out[:n] = x.cpu()[rows[:n]]
    return dict(row_index=row_index, label=label, n=n, overflow=int(rows.numel() > cap), x=out)


def vocab_ce(logits, label, n, gout=1.0):
    """logits [cap, V] (any float dtype, taken as float64), label [cap], n rows count -> (loss, d_logits [cap, V]) with
    loss = sum_{r<n} (logsumexp(z_r) - z_r[label_r]) / n; n == 0: NaN and an all-zero gradient (torch's mean over nothing)"""
    z = logits.detach().double().cpu().clone().requires_grad_(True)
    d = torch.zeros_like(z)
    if n == 0:
        return float("nan"), d
    lab = label[:n].long().cpu()
    loss = F.cross_entropy(z[:n], lab, reduction="sum") / n
    (g,) = torch.autograd.grad(loss * gout, z)
    return float(loss.detach()), g.detach()


def smooth_l1(d):
    a = d.abs()
    return torch.where(a < 1.0, 0.5 * d * d, a - 0.5)


def visual_losses(jobs, gout=1.0, ignore_index=IGNORE):
    """jobs: (kind 'ce' | 'l2', scores [R, W], label, mask_conf [R], weight) -> ([loss], [d_scores]): per-row loss (0 on
    an ignored label) times the confidence, mean over ALL rows, times the weight (modeling.py:1036-1044)"""
    losses, grads = [], []
    for kind, scores, label, conf, weight in jobs:
        s = scores.detach().double().cpu().clone().requires_grad_(True)
        c = conf.detach().double().cpu().reshape(-1)
        if kind == "ce":
            row = F.cross_entropy(s, label.cpu().long().reshape(-1), ignore_index=ignore_index, reduction="none")
        else:
            row = smooth_l1(s - label.detach().double().cpu().reshape(s.shape)).mean(1)
        loss = (row * c).mean() * weight
        (g,) = torch.autograd.grad(loss * gout, s)
        losses.append(float(loss.detach()))
        grads.append(g.detach())
    return losses, grads


def gelu(x):
    return x * 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0)))


def layer_norm(x, w, b, eps=1e-12):
    u = x.mean(-1, keepdim=True)
    s = (x - u).pow(2).mean(-1, keepdim=True)
    return w * ((x - u) / torch.sqrt(s + eps)) + b


def transform(x, P, prefix):
    """BertPredictionHeadTransform: dense, GELU, LayerNorm(eps 1e-12)"""
    h = gelu(x @ P[prefix + "dense.weight"].t() + P[prefix + "dense.bias"])
    return layer_norm(h, P[prefix + "LayerNorm.weight"], P[prefix + "LayerNorm.bias"])


HEAD_INPUTS = ("lang_output", "visn_output", "pooled_output")


def heads(P, t, task_mask_lm=True, task_matched=True, task_obj_predict=True, task_qa=True, visual_losses_on=("obj", "attr", "feat"),
          visual_loss_config=None):
    """The heads and losses on top of the encoder's outputs.  ``P``: parameters by their state_dict names
    (``cls.predictions.decoder.weight`` is the tied word table); ``t``: lang_output [B, T, H], visn_output [B, O, H],
    pooled_output [B, H], masked_lm_labels [B, T], matched_label [B], ans [B], and per visual loss ``<key>_label`` and
    ``<key>_conf``.  -> dict(total, losses [k] in the reference's order, answer_score, grads {name: d total / d tensor} for
    every parameter used and for the three encoder outputs)."""
    P = {k: v.detach().double().clone().requires_grad_(True) for k, v in P.items()}
    x = {k: t[k].detach().double().clone().requires_grad_(True) for k in HEAD_INPUTS}
    lang, visn, pooled = x["lang_output"], x["visn_output"], x["pooled_output"]
    total, losses = 0.0, []
    answer_score = None
    if task_qa:
        h = gelu(pooled @ P["answer_head.logit_fc.0.weight"].t() + P["answer_head.logit_fc.0.bias"])
        h = layer_norm(h, P["answer_head.logit_fc.2.weight"], P["answer_head.logit_fc.2.bias"])
        answer_score = h @ P["answer_head.logit_fc.3.weight"].t() + P["answer_head.logit_fc.3.bias"]
    if t.get("masked_lm_labels") is not None and task_mask_lm:
        h = transform(lang, P, "cls.predictions.transform.")
        z = h @ P["cls.predictions.decoder.weight"].t() + P["cls.predictions.bias"]
        l = F.cross_entropy(z.reshape(-1, z.shape[-1]), t["masked_lm_labels"].reshape(-1).long(), ignore_index=IGNORE)
        total, losses = total + l, losses + [l.detach()]
    if t.get("matched_label") is not None and task_matched:
        z = pooled @ P["cls.seq_relationship.weight"].t() + P["cls.seq_relationship.bias"]
        l = F.cross_entropy(z, t["matched_label"].reshape(-1).long(), ignore_index=IGNORE)
        total, losses = total + l, losses + [l.detach()]
    if task_obj_predict and any((k + "_label") in t for k in visual_losses_on):
        h = transform(visn, P, "obj_predict_head.transform.")
        for key in visual_losses_on:
            W, kind, _, weight = visual_loss_config[key]
            s = h @ P["obj_predict_head.decoder_dict.%s.weight" % key].t() + P["obj_predict_head.decoder_dict.%s.bias" % key]
            s = s.reshape(-1, W)
            conf = t[key + "_conf"].double().reshape(-1)
            if kind == "ce":
                row = F.cross_entropy(s, t[key + "_label"].reshape(-1).long(), ignore_index=IGNORE, reduction="none")
            else:
                row = smooth_l1(s - t[key + "_label"].double().reshape(-1, W)).mean(1)
            l = (row * conf).mean() * weight
            total, losses = total + l, losses + [l.detach()]
    if t.get("ans") is not None and task_qa:
        l = F.cross_entropy(answer_score, t["ans"].reshape(-1).long(), ignore_index=IGNORE)
        total, losses = total + l, losses + [l.detach()]
    leaves = dict(P)
    leaves.update(x)
    names = list(leaves)
    gs = torch.autograd.grad(total, [leaves[k] for k in names], allow_unused=True)
    grads = {k: g.detach() for k, g in zip(names, gs) if g is not None}
    return dict(total=float(total.detach()), losses=[float(l) for l in losses],
                answer_score=(answer_score.detach() if task_qa else pooled.detach()[0][0]), grads=grads)
