"""The VQA-CP v2 training iteration (src/vqa/vqacpv2.py:164-254) on the HIP blocks.

``loss_func`` / ``compute_kl_loss`` keep the reference names and signatures
(src/vqa/vqacpv2.py:48-61).  ``plain_pass`` / ``ggm_pass`` are the two optimiser passes of
one iteration; ``train_iteration`` strings them together in the VQA order (plain first) or
the GQA order (GGM first, src/gqa/gqa_ood.py:165-292).  The only PyTorch arithmetic left is
scalar glue on 0-dim loss tensors and the removal of the adjacency diagonal of the INPUT.
"""
import random

import torch
import torch.nn as nn

from .. import functional as XF
from ..lxrt.optimization import clip_grad_norm_, require_arena_aware
from ..runtime import runtime_of


# ``scale`` (not in the reference signatures, default 1): a constant factor folded into the loss kernel and its
# backward.  The training passes use it for the loss weights (x num_answers, x 6 (8 KL + DSM), ...): every
# ``scalar * loss`` written in torch is a kernel of its own in forward and another one in backward, ~5 us each for
# one float.
# ``slot``: a zeroed 1-element fp32 tensor the kernel accumulates into (Runtime.scalar_slot: the loss terms of a pass
# share one buffer zeroed by one launch); None = the op zeroes its own.
def loss_func(score, grad_log_q_noise, sigma=0.2, scale=1.0, slot=None):
    """0.5 sigma^2 mean_b sum_ij (score - g)^2 / (d1 d2).  ref: src/vqa/vqacpv2.py:48-51"""
    return XF.DSMFn.apply(score, grad_log_q_noise, sigma, scale, slot)


def compute_kl_loss(x, y, scale=1.0, slot=None):
    """symmetric KL of the last-dim softmaxes, mean over all elements.
    ref: src/vqa/vqacpv2.py:54-61"""
    if x.dtype != y.dtype:
        x, y = x.float(), y.float()
    return XF.SymKLFn.apply(x, y, scale, slot)


class BCEWithLogitsLoss(nn.Module):
    """nn.BCEWithLogitsLoss() of src/vqa/vqacpv2.py:131 on fp32 logits."""

    def forward(self, logit, target, scale=1.0, slot=None):
        return XF.BCEFn.apply(logit.float(), target.float(), scale, slot)


class _Scaled:
    """a loss term that was computed with its weight folded in; ``float()`` gives the unweighted value"""

    def __init__(self, t, c):
        self.t, self.c = t.detach(), float(c)

    def __float__(self):
        return float(self.t) / self.c

    def detach(self):
        return self


def remove_diagonal(adj_true):
    """adj_true.triu(1) + adj_true.tril(-1)   (src/vqa/vqacpv2.py:188): input preparation"""
    from .. import ops
    return ops.zero_diag(adj_true.float().contiguous())


def enable_data_parallel(model, group=None, wire_dtype=None, overlap=None, zero1=False, check_every=None,
                         check_level="weights"):
    """one process per GPU: average the flat gradient arena over ``group`` between backward and
    the fused clip + BertAdam of every pass (xggm_amd.dist.GradSync); replicas start equal.
    ``overlap`` (default on; XGGM_DP_OVERLAP=0 turns it off): cut the backward between the single-modality
    and the cross-modality layers so the all-reduce of the upper 60 % of the gradients runs under the
    backward of the lower layers (engine.CapturedTrainer).  ``zero1``: shard the update (dist.ShardedUpdate:
    reduce-scatter of the matrix gradients, BertAdam on this rank's 1/world of every matrix range, all-gather
    of the bf16 weights the GEMMs read).
    Every rank draws its OWN dropout masks and denoising noise (the Philox seed is folded with the rank): the
    averaged gradient is then that of one batch of world x B samples with independent noise; only the host-side
    branch decision is shared (``pick_branch``).
    ``check_every`` (default None: off, nothing is launched or exchanged): every so many iterations the ranks compare
    fingerprints of what ``check_level`` names ("weights" or "state", dist.ReplicaGuard) and ALL raise
    ``dist.ReplicaDrift`` when their replicas have come apart; ``save_training_state`` then checks before it writes and
    is a collective call under either update mode: make it on EVERY rank (``path=None`` where no file is wanted)."""
    import os
    import torch.distributed as dist
    from ..dist import GradSync, broadcast_params
    if zero1 and getattr(model, "debias_loss", None) is not None:
        raise RuntimeError("the sharded update (zero1=True) does not support an attached debias loss; use the replicated "
                           "update")
    rt = runtime_of(model)
    broadcast_params(rt.arena, group)
    rank = dist.get_rank(group) if dist.is_initialized() else 0
    if rank:
        # seed word of the device-resident {seed, offset} pair; saved / restored with the training state
        rt.rng[0] = (int(rt.rng[0].item()) + rank * 0x9E3779B97F4A7C15) & 0x7FFFFFFFFFFFFFFF
    inplace = wire_dtype == torch.bfloat16 and rt.arena.shadow is not None and os.environ.get("XGGM_DP_WIRE_ARENA", "1") != "0"
    if inplace:
        # bf16 on the wire + bf16 storage: matrix gradients are BORN in the wire arena (weight-gradient GEMM epilogue),
        # reduced in place and read by the update: no cast before, no copy after the exchange
        rt.arena.enable_wire()
    if zero1 and not inplace:
        raise RuntimeError("the sharded update needs the bf16 wire arena (bf16 storage, wire_dtype=torch.bfloat16)")
    if zero1:
        from ..dist import ShardedUpdate
        gs = rt.arena.zero1 = ShardedUpdate(rt.arena, group)
    else:
        gs = GradSync(rt.arena.grads, group, wire_dtype, arena=rt.arena if inplace else None)
    if inplace and os.environ.get("XGGM_DP_SPARSE_EMB", "1") != "0":
        # the word-embedding gradient: exchange the rows of this step's tokens, not the 30522-row table
        wt = model.lxrt_encoder.model.bert.embeddings.word_embeddings.weight
        xg = getattr(wt, "_xg", None)
        if xg is not None and xg[0] is rt.arena:
            gs.set_sparse_table(xg[1], wt.shape[0], wt.shape[1], lambda: rt.emb_ids)
    object.__setattr__(model, "_grad_sync", gs)
    rt.arena.sq_enabled = False  # the clip norm is that of the AVERAGED gradients: read them after the exchange
    rt.arena.row_list_enabled = False  # ... and the word table's gradient holds the OTHER ranks' rows too
    if overlap is None:
        overlap = os.environ.get("XGGM_DP_OVERLAP", "1") != "0"
    rt.cut_enabled = bool(overlap)
    if check_every is not None:
        from ..dist import ReplicaGuard
        object.__setattr__(model, "_replica_guard", ReplicaGuard(rt.arena, group, every=check_every, level=check_level))
    return model


def _tick_guard(model):
    """end of a training iteration: the replica drift guard (when ``enable_data_parallel`` made one) counts it"""
    guard = getattr(model, "_replica_guard", None)
    if guard is not None:
        guard.tick()


def _sync_grads(model):
    gs = getattr(model, "_grad_sync", None)
    if gs is not None:
        from ..dist import active_ranges
        gs.sync(active_ranges(runtime_of(model).arena))


def attach_debias_loss(model, loss):
    """train ``model`` (a VQAModel / GQAModel) with a debias answer loss -- a ``module.vqa_debias_loss_functions``
    instance (Plain, ReweightByInvBias, BiasProduct, LearnedMixin) or one of ``module.answer_losses`` (Focal; CrossEntropy,
    the reference's --mceLoss, ``make_answer_loss``) -- in place of BCEWithLogits x answers: sets
    ``model.debias_loss = loss``.  Every pass (``forward_backward_plain`` / ``_ggm``, ``plain_pass``, ``ggm_pass``,
    ``train_iteration``, ``engine.CapturedTrainer``) then hands the loss the tensor that enters ``logit_fc`` as ``hidden``,
    the logits, the target and the batch's ``"bias"`` ([B, A] fp32) or ``"bias_index"`` ([B] int64 rows of
    ``loss.bias_table``, see ``answer_prior_table`` / ``set_bias_table``).
    Call it BEFORE the first forward (and before the optimiser is made): the loss's parameters (bias_lin.weight,
    bias_lin.bias, smooth_param) then join the parameter arena as the group ``debias_loss`` -- vector-class members: fp32
    gradient, no bf16 shadow read -- and the fused update trains them.  Afterwards the arena's layout is fixed:
    RuntimeError.  Under ``make_optimizer(..., no_decay=NO_DECAY)`` all three names contain "bias" (de-bias-loss) and land
    in the undecayed group: intended, they are a bias, a gate and a scalar.
    Not supported together with the sharded update (``enable_data_parallel(zero1=True)``); ``CapturedTrainer(packed_spec=)``
    takes the losses that read no bias (Plain, CrossEntropy) only; replicated data parallelism works."""
    from ..module.vqa_debias_loss_functions import DebiasLossFn
    from ..runtime import root_of
    if not isinstance(loss, DebiasLossFn):
        raise TypeError("attach_debias_loss: expected a module.vqa_debias_loss_functions loss, got %s" % type(loss).__name__)
    root = root_of(model)
    if getattr(root, "_xg_rt", None) is not None:
        raise RuntimeError("attach_debias_loss must run before the first forward: the parameter arena has been laid out "
                           "and the loss's parameters can no longer join it")
    p = next(model.parameters(), None)
    if p is not None:
        loss.to(p.device)
    model.debias_loss = loss
    return model


def make_answer_loss(args):
    """the loss to attach for the parsed flags ``args`` (``param.parse_args``): ``CrossEntropy()`` -- the reference's
    nn.CrossEntropyLoss(ignore_index=-1), src/gqa/gqa_ood.py:116 -- under ``--mceLoss``, else None (BCEWithLogits x answers)"""
    if getattr(args, "mce_loss", False):
        from ..module.answer_losses import CrossEntropy
        return CrossEntropy()
    return None


def _head_loss(model, bce_loss, hidden, logit, target, bias, bias_index, **slot):
    """the answer-head loss of a pass at the scale BCE x answers: the attached debias loss, else ``bce_loss``"""
    dl = getattr(model, "debias_loss", None)
    if dl is None:
        return bce_loss(logit, target, scale=target.size(1), **slot)
    if dl.needs_bias and bias is None and bias_index is None:
        raise ValueError("the model has a %s attached: the batch needs \"bias\" ([B, A] fp32) or \"bias_index\" ([B] int64)"
                         % type(dl).__name__)
    return dl(hidden, logit, bias, target, bias_index=bias_index, **slot)


def _head_inputs(model, x):
    """(input of ``logit_fc``, ``hidden`` of the attached loss): two consumers of one tensor go through ``XF.fan_out``"""
    dl = getattr(model, "debias_loss", None)
    if dl is not None and dl.needs_hidden:
        return XF.fan_out(x, 2)
    return x, None


def forward_backward_plain(model, bce_loss, feats, boxes, sent, target, between=None, bias=None, bias_index=None):
    """step A up to backward: src/vqa/vqacpv2.py:170-174.  ``between``: callback between the two backward
    stages when the runtime cuts the graph (Runtime.backward).  ``bias`` / ``bias_index``: for an attached debias loss
    (``attach_debias_loss``)."""
    model.zero_grad()
    rt = runtime_of(model)
    _, _, x = model(feats, boxes, sent)
    x, hidden = _head_inputs(model, x)
    logit = model.logit_fc(x)
    loss = _head_loss(model, bce_loss, hidden, logit, target, bias, bias_index)
    rt.backward(loss, between)
    return loss.detach(), logit.detach()


def forward_backward_ggm(model, bce_loss, feats, boxes, sent, target, adj_true, branch, sigma=1.0, kl_weight=8.0,
                         randn=None, between=None, bias=None, bias_index=None):
    """step B up to backward: relation generation (branch 'rel', src/vqa/vqacpv2.py:195-222) or
    representation generation ('node', :228-251).  ``randn`` injects the Gaussian draw
    (parity tests); None = in-kernel Philox."""
    model.zero_grad()
    rt = runtime_of(model)
    feat_seq, _, x = model(feats, boxes, sent)
    adj_true = remove_diagonal(adj_true)
    N = feat_seq[1].shape[1]
    A = target.size(1)
    rt.begin_losses(4)  # the three loss kernels accumulate into slots of one buffer zeroed by one launch
    # tensors the reference uses more than once go through XF.fan_out: same values, same gradients, but the sum of
    # the consumers' gradients is one launch of ours instead of the autograd engine's at::add per extra consumer
    x, x_fuse = XF.fan_out(x, 2)
    if branch == "rel":
        e = model.encoder_adj(x)
        adj_noise, grad_log_noise = XF.AdjInitFn.apply(e, N, sigma, randn, None if randn is not None else rt.rng, 9001,
                                                       rt.long_graph)
        node_feats, adj_noise = model.generator(feat_seq[1], adj_noise)
        adj_noise, adj_kl = XF.fan_out(adj_noise, 2)
        # loss = bce * A + 6 * (kl_weight * (kl * A) + dsm), the weights folded into the loss kernels
        w_kl, w_dsm = 6.0 * kl_weight * A, 6.0
        loss_grad = loss_func(adj_noise, grad_log_noise, sigma=sigma, scale=w_dsm, slot=rt.scalar_slot())
        d_loss = compute_kl_loss(adj_true, adj_kl, scale=w_kl, slot=rt.scalar_slot())
    elif branch == "node":
        node_feats = XF.BcastRowsFn.apply(model.node_fc(x), N)  # == node_fc(x.unsqueeze(1).repeat(1, N, 1))
        node_feats, feat_grad = XF.FeatureNoiseFn.apply(node_feats, sigma, randn,
                                                        None if randn is not None else rt.rng, 9002)
        node_feats, _ = model.generator(node_feats, adj_true)
        node_feats, node_kl, node_dsm = XF.fan_out(node_feats, 3)
        # loss = bce * A + 1.1 * (0.15 * (kl * A) + 6 * dsm)
        w_kl, w_dsm = 1.1 * 0.15 * A, 1.1 * 6.0
        d_loss = compute_kl_loss(node_kl, feat_seq[1], scale=w_kl, slot=rt.scalar_slot())
        loss_grad = loss_func(node_dsm, feat_grad, sigma=sigma, scale=w_dsm, slot=rt.scalar_slot())
    else:
        raise ValueError(branch)
    x_gen, hidden = _head_inputs(model, model.fusion_fc(XF.PoolConcatFn.apply(x_fuse, node_feats)))
    logit = model.logit_fc(x_gen)
    bce = _head_loss(model, bce_loss, hidden, logit, target, bias, bias_index, slot=rt.scalar_slot())
    loss = XF.LossSumFn.apply(bce, d_loss, loss_grad)
    rt.backward(loss, between)
    # reported as the reference logs them: bce = BCE * A, d_loss = KL * A, loss_grad = the unweighted DSM term
    return loss.detach(), logit.detach(), dict(d_loss=_Scaled(d_loss, w_kl / A), loss_grad=_Scaled(loss_grad, w_dsm),
                                               bce=_Scaled(bce, 1.0))


def clip_and_step(model, optim, clip=5.0, advance=False):
    """nn.utils.clip_grad_norm_(params, 5.) + optim.step() + optim.zero_grad()
    (src/vqa/vqacpv2.py:175-177), fused: one norm reduction, one update pass.  ``advance``: also end the pass
    (Runtime.advance: new dropout masks / noise for the next one) -- the RNG step then rides on the norm's last launch."""
    require_arena_aware(optim)  # a torch.optim class here would train nothing, silently (TypeError)
    rt = runtime_of(model)
    total = clip_grad_norm_(model.parameters(), clip, tail=(optim, rt if advance else None))
    optim.step()
    z = rt.arena.zero1
    if z is not None:
        z.gather()  # sharded update: the other ranks' slices of the bf16 weights
    optim.zero_grad()
    if advance:
        rt.advance()
    return total


def log_pass(train_log, model, optim, kind, loss, total, terms=None):
    """one ``ops.train_log_append`` behind the update of a pass (``plain_pass`` / ``ggm_pass`` here,
    ``engine.CapturedTrainer(train_log=)``): the same call with the same operands wherever the pass runs, hence the same
    bits.  ``train_log``: an ``engine.TrainLog``; ``loss`` / ``total``: the pass's total loss and pre-clip norm (device
    scalars); ``terms``: the third value of ``forward_backward_ggm`` (the loss-kernel slots and the weights ``_Scaled``
    divides by), None for the plain pass, whose loss IS its BCE term.  The recorded terms are the un-weighted ones the
    reference logs: BCE x answers, KL x answers, the DSM term.

    LR_SCALE and the record's step come from the arena group of the answer head ``model.logit_fc`` -- part of
    ``optim.param_groups[0]`` under ``make_optimizer``, and the one group of it that EVERY pass updates (a group that only
    the GGM passes touch would leave stale values in the plain records).  The schedule step of a pass runs BEFORE its update (on the norm's finishing
    launch, ``clip_grad_norm_``; else at the top of ``BertAdam.step``): it writes lr_scale = warmup_linear(s / t_total,
    warmup) from the counter s it finds and leaves s + 1.  The append is issued behind the update, so it reads the
    value THIS pass's update multiplied its lr by, together with the counter the pass left: a record with step k holds
    warmup_linear((k - 1) / t_total, warmup)."""
    from .. import ops, trainlog as T
    arena = runtime_of(model).arena
    xg = getattr(next(model.logit_fc.parameters()), "_xg", None)
    gi = arena.group_index[xg[3]] if xg is not None and xg[0] is arena else None
    cols, mul = [None] * 6, [1.0] * 6
    cols[T.LOSS] = loss
    if terms is None:
        cols[T.BCE] = loss
    else:
        for c, key in ((T.BCE, "bce"), (T.KL, "d_loss"), (T.DSM, "loss_grad")):
            cols[c], mul[c] = terms[key].t, 1.0 / terms[key].c
    cols[T.GRAD_NORM] = total
    if gi is not None:
        cols[T.LR_SCALE] = arena.lr_scale[gi:gi + 1]
    ops.train_log_append(train_log, T.KIND_OF[kind], cols, mul, step=None if gi is None else arena.steps[gi:gi + 1])


def plain_pass(model, optim, bce_loss, feats, boxes, sent, target, clip=5.0, advance=False, train_log=None, bias=None,
               bias_index=None):
    """``train_log`` = an ``engine.TrainLog``: the pass ends with one ``log_pass`` behind its update (None: no launch)"""
    out = forward_backward_plain(model, bce_loss, feats, boxes, sent, target, bias=bias, bias_index=bias_index)
    _sync_grads(model)
    total = clip_and_step(model, optim, clip, advance)
    if train_log is not None:
        log_pass(train_log, model, optim, "plain", out[0], total)
    return out


def ggm_pass(model, optim, bce_loss, feats, boxes, sent, target, adj_true, branch, sigma=1.0, kl_weight=8.0,
             randn=None, clip=5.0, advance=False, train_log=None, bias=None, bias_index=None):
    out = forward_backward_ggm(model, bce_loss, feats, boxes, sent, target, adj_true, branch, sigma, kl_weight, randn,
                               bias=bias, bias_index=bias_index)
    _sync_grads(model)
    total = clip_and_step(model, optim, clip, advance)
    if train_log is not None:
        log_pass(train_log, model, optim, branch, out[0], total, out[2])
    return out


def pick_branch(delta, rng=random, model=None):
    """random.randint(1, 10) <= args.delta -> relation generation (src/vqa/vqacpv2.py:192-193).  With data
    parallelism (``model`` carries a gradient exchange) every rank takes RANK 0's draw: ranks on different
    branches would exchange different parameter ranges (encoder_adj vs node_fc) and hang or mix gradients."""
    rel = rng.randint(1, 10) <= delta
    gs = getattr(model, "_grad_sync", None) if model is not None else None
    if gs is not None and gs.world > 1:
        from ..dist import sync_branch
        rel = sync_branch(rel, gs.g.device, gs.group)
    return "rel" if rel else "node"


def train_iteration(model, optim, bce_loss, batch, delta=5, sigma=1.0, order="vqa", branch=None, clip=5.0, train_log=None):
    """one iteration = two fwd+bwd+clip+BertAdam passes.  ``batch``: dict with feats, boxes,
    sent, target, adj_true (device tensors).  order 'vqa': plain then GGM (KL weight 8);
    'gqa': GGM then plain (KL weight 12, src/gqa/gqa_ood.py:197).  ``train_log`` = an ``engine.TrainLog``: every pass
    appends its record to it on the device (``log_pass``) -- the scalars of src/vqa/vqacpv2.py:179 and :256-270 without a
    read per iteration."""
    rt = runtime_of(model)
    model.train()
    if branch is None:
        branch = pick_branch(delta, model=model)
    args = (batch["feats"], batch["boxes"], batch["sent"], batch["target"])
    kw = dict(clip=clip, advance=True, train_log=train_log)
    if getattr(model, "debias_loss", None) is not None:  # the bias of the attached loss travels in the batch
        kw.update(bias=batch.get("bias"), bias_index=batch.get("bias_index"))
    out = {}
    if order == "vqa":
        out["loss_plain"], out["logit"] = plain_pass(model, optim, bce_loss, *args, **kw)
        out["loss_ggm"], _, ex = ggm_pass(model, optim, bce_loss, *args, batch["adj_true"], branch, sigma, 8.0, **kw)
    else:
        out["loss_ggm"], _, ex = ggm_pass(model, optim, bce_loss, *args, batch["adj_true"], branch, sigma, 12.0, **kw)
        out["loss_plain"], out["logit"] = plain_pass(model, optim, bce_loss, *args, **kw)
    out.update((k, v) for k, v in ex.items() if k != "bce")  # the BCE slot is ``log_pass``'s: the keys stay the reference's
    out["branch"] = branch
    _tick_guard(model)
    return out


ENCODER_PREFIX = "lxrt_encoder."
# name substrings of the parameters that usually go without weight decay: biases and LayerNorm weights.  The encoder's
# LayerNorms are attributes called LayerNorm / *_layer_norm; the heads (logit_fc, node_fc, fusion_fc) and the generators'
# MLPs are Sequential(Linear, GeLU, LayerNorm), whose LayerNorm weight is item "2.weight".
NO_DECAY = ("bias", "LayerNorm.weight", "layer_norm.weight", ".2.weight")


def param_depth(name, llayers, xlayers, rlayers):
    """depth of a parameter for layer-wise learning-rate decay: 0 for the embeddings and visn_fc, the two towers END level
    (with L = max(llayers, rlayers): ``encoder.layer.i`` -> i + 1 + (L - llayers), ``encoder.r_layers.i`` -> i + 1 +
    (L - rlayers)), ``encoder.x_layers.j`` -> L + 1 + j, and D = L + xlayers + 1 for the pooler and everything outside
    the encoder."""
    import re
    L = max(llayers, rlayers)
    D = L + xlayers + 1
    if not name.startswith(ENCODER_PREFIX):
        return D
    m = re.search(r"\.encoder\.(layer|r_layers|x_layers)\.(\d+)\.", name)
    if m:
        i = int(m.group(2))
        return {"layer": i + 1 + (L - llayers), "r_layers": i + 1 + (L - rlayers), "x_layers": L + 1 + i}[m.group(1)]
    if ".embeddings." in name or ".encoder.visn_fc." in name:
        return 0
    return D  # the pooler


def split_param_names(names, lr, no_decay=None, layer_decay=None, llayers=9, xlayers=5, rlayers=5, head_lr_mult=4.0):
    """The param_groups of ``make_optimizer(..., no_decay, layer_decay)`` over parameter NAMES (``named_parameters()``
    order is kept inside a group): [{"names": [...], "lr": ..., ("weight_decay": 0.0)}].
    Base lr: ``lr`` for the encoder, ``head_lr_mult * lr`` for the rest (the reference's two groups,
    src/vqa/vqacpv2.py:113-128).  ``layer_decay`` = d: a parameter's lr is its base lr times d ** (D - depth)
    (``param_depth``).  ``no_decay``: name substrings (``NO_DECAY``); a matching parameter goes to a twin group with
    ``weight_decay`` 0.0, the others keep the optimiser's default.  Every name lands in exactly one group; groups come
    in the order head, then encoder by falling depth, decay before no-decay.  With both None: the reference's two."""
    D = max(llayers, rlayers) + xlayers + 1
    groups = {}
    for n in names:
        enc = n.startswith(ENCODER_PREFIX)
        depth = param_depth(n, llayers, xlayers, rlayers) if layer_decay is not None else D
        nd = no_decay is not None and any(s in n for s in no_decay)
        groups.setdefault((enc, -depth, nd), []).append(n)
    out = []
    for (enc, mdepth, nd) in sorted(groups):
        g = {"names": groups[(enc, mdepth, nd)], "lr": (lr if enc else lr * head_lr_mult)}
        if layer_decay is not None:
            g["lr"] = g["lr"] * float(layer_decay) ** (D + mdepth)
        if nd:
            g["weight_decay"] = 0.0
        out.append(g)
    return out


def answer_prior_table(targets, group_ids, n_groups):
    """the usual bias of the ensemble losses: per group (question type) the mean target score of every answer over the
    group's training samples.  ``targets``: [n, A] soft scores, ``group_ids``: [n] ints in [0, n_groups) -> fp32
    [n_groups, A]; a group without samples gets zeros.  Host side, numpy: run once over the training set, hand the table
    to ``loss.set_bias_table`` and put each sample's group id into the batch as ``"bias_index"``."""
    import numpy as np
    targets = np.asarray(targets, dtype=np.float64)
    group_ids = np.asarray(group_ids, dtype=np.int64).reshape(-1)
    if targets.ndim != 2 or group_ids.shape[0] != targets.shape[0]:
        raise ValueError("answer_prior_table: targets %s and group_ids %s do not match" % (targets.shape, group_ids.shape))
    if group_ids.size and (group_ids.min() < 0 or group_ids.max() >= n_groups):
        raise ValueError("answer_prior_table: group ids must lie in [0, %d)" % n_groups)
    sums = np.zeros((int(n_groups), targets.shape[1]), dtype=np.float64)
    np.add.at(sums, group_ids, targets)
    counts = np.bincount(group_ids, minlength=int(n_groups)).astype(np.float64)
    return (sums / np.maximum(counts, 1.0)[:, None]).astype(np.float32)


def make_optimizer(model, lr, t_total, warmup=0.1, optim='bert', no_decay=None, layer_decay=None):
    """the two parameter groups of src/vqa/vqacpv2.py:113-128: heads/generator at 4*lr,
    encoder at lr; BertAdam(warmup=0.1, t_total=2*iters).  ``optim``: another ``--optim`` name of the reference
    (rms, adam, adamw, adamax, sgd) or what ``param.get_optimizer`` returned for it builds the else-branch
    (src/vqa/vqacpv2.py:141): one group, all parameters, ``lr`` -- the arena-aware class of ``xggm_amd.optim``.
    ``no_decay`` (name substrings, e.g. ``NO_DECAY``) and / or ``layer_decay`` (a factor d per layer of depth, see
    ``split_param_names``) build finer param_groups and turn ``split_groups`` on, so that groups which cut through the
    arena's ranges are honoured; the else-branch's base lr is ``lr`` for every parameter, as without them.
    ``optim='bertlamb'``: ``BertLamb`` in BertAdam's place (layer-wise trust ratios, for large global batches); with
    ``no_decay`` the no-decay groups also get ``layer_adaptation=False``."""
    lamb = isinstance(optim, str) and 'lamb' in optim  # 'bertlamb': param.get_optimizer answers 'bert' for it, as for any bert*
    if isinstance(optim, str):
        from ..param import get_optimizer
        optim = get_optimizer(optim)
    split = no_decay is not None or layer_decay is not None
    if split:
        enc = model.lxrt_encoder.model.bert.encoder
        named = dict(model.named_parameters())
        specs = split_param_names(list(named), lr, no_decay, layer_decay, len(enc.layer), len(enc.x_layers), len(enc.r_layers),
                                  head_lr_mult=4.0 if optim == 'bert' else 1.0)
        groups = [dict({k: v for k, v in g.items() if k != "names"}, params=[named[n] for n in g["names"]]) for g in specs]
    if optim != 'bert':
        return optim(groups, lr, split_groups=True) if split else optim(model.parameters(), lr)
    from ..lxrt.optimization import BertAdam
    if lamb:
        # the BERT recipe: with ``no_decay`` the biases and LayerNorm weights (the groups split_param_names gave
        # weight_decay 0.0) are not adapted either
        from ..lxrt.optimization import BertLamb as BertAdam
        if split:
            for g in groups:
                if g.get("weight_decay") == 0.0:
                    g["layer_adaptation"] = False
    if split:
        return BertAdam(groups, lr=lr, warmup=warmup, t_total=t_total, split_groups=True)
    lxrt_ids = set(map(id, model.lxrt_encoder.parameters()))
    base_params = [p for p in model.parameters() if id(p) not in lxrt_ids]
    groups = [{"params": base_params, "lr": lr * 4}, {"params": list(model.lxrt_encoder.parameters())}]
    return BertAdam(groups, lr=lr, warmup=warmup, t_total=t_total)


def predict(model, eval_tuple, dump=None, predictor=None, resident=None):
    """``VQA.predict`` (src/vqa/vqacpv2.py:315-339; GQA twin src/gqa/gqa_ood.py:379-403): eval mode, encoder ->
    ``logit_fc`` -> arg-max -> ``{question_id: answer}``.  ``eval_tuple`` = (dset, loader, evaluator) as in the
    reference; only the first four fields of a loader item are looked at (never the ground truth).  ``predictor``:
    an ``engine.CapturedPredictor`` to replay one captured forward per batch instead of launching eagerly.  When the
    predictor carries an ``engine.AnswerLog`` the answers stay on the device for the whole sweep: every batch is only
    queued (``push``), the question ids are kept on the host in call order, and the log is read ONCE behind the loop --
    no host synchronisation between the first and the last batch (the per-batch ``.cpu()`` of :333 is gone).
    ``resident``: a ``tools.resident.ResidentDataset`` of the split: the sweep then goes over the store's samples in data
    set order, ``predictor.push_resident`` gathers every batch on the device (the last one ragged) and the loader is not
    iterated; needs a ``predictor``.  Same ``{question_id: answer}`` as the loader path."""
    dset, loader, evaluator = eval_tuple
    dev = next(model.parameters()).device
    was_training = model.training
    model.eval()
    quesid2ans = {}
    try:
        if resident is not None:
            if predictor is None:
                raise ValueError("predict: a resident store is swept through a CapturedPredictor (predictor=...)")
            from ..answers import to_quesid2ans
            log, n, B = getattr(predictor, "log", None), len(resident), predictor.B
            ques_ids = resident.ques_ids(resident.order(0, shuffle=False, drop_last=False))
            labels = []
            if log is not None:
                log.reset()
            for start in range(0, n, B):
                b = predictor.push_resident(resident, start, min(B, n - start))
                if log is None:
                    labels.append(predictor.label[:b].cpu())  # a view of a static buffer: consumed before the next push
            labels = log.read()[0] if log is not None else torch.cat(labels)
            quesid2ans = to_quesid2ans(ques_ids, labels, dset.label2ans)
        elif predictor is not None and getattr(predictor, "log", None) is not None:
            from ..answers import to_quesid2ans
            log, ques_ids = predictor.log, []
            log.reset()
            for datum_tuple in loader:
                ques_id, feats, boxes, sent = datum_tuple[:4]
                predictor.push(feats.to(dev, non_blocking=True), boxes.to(dev, non_blocking=True), sent)
                ques_ids.extend(ques_id.tolist() if torch.is_tensor(ques_id) else ques_id)
            labels = log.read()[0]
            quesid2ans = to_quesid2ans(ques_ids, labels, dset.label2ans)
        else:
            for datum_tuple in loader:
                ques_id, feats, boxes, sent = datum_tuple[:4]
                feats, boxes = feats.to(dev, non_blocking=True), boxes.to(dev, non_blocking=True)
                if predictor is not None:
                    label, _ = predictor(feats, boxes, sent)
                else:
                    with torch.no_grad():
                        _, _, x = model(feats, boxes, sent)
                        label = model.logit_fc(x).max(1)[1]
                for qid, l in zip(ques_id, label.cpu().numpy()):
                    quesid2ans[qid.item() if hasattr(qid, "item") else qid] = dset.label2ans[l]
    finally:
        model.train(was_training)
    if dump is not None:
        evaluator.dump_result(quesid2ans, dump)
    return quesid2ans


def evaluate(model, eval_tuple, dump=None, predictor=None, resident=None):
    """``VQA.evaluate`` (src/vqa/vqacpv2.py:341-344)"""
    return eval_tuple[2].evaluate(predict(model, eval_tuple, dump, predictor, resident))


def val_schedule(n_batches):
    """the iterations after which the reference validates inside an epoch of ``n_batches`` iterations
    (``val_in_epoch``, src/vqa/vqacpv2.py:157; the last bin edge is the epoch's own validation)"""
    import numpy as np
    return np.linspace(0, n_batches, 5, dtype=int)[1:-1]


def global_steps(n, batch_size, world=1):
    """iterations of a training epoch over ``n`` samples at ``batch_size`` rows PER RANK: whole global steps of ``world x
    batch_size`` samples (a ragged global step cannot be split into equal ranks and is dropped).  Under data parallelism
    ``t_total`` (times the epochs) and ``val_schedule`` count these, so a run on ``world`` ranks validates and decays its
    learning rate where a single-process run at ``world x batch_size`` would."""
    return int(n) // (int(batch_size) * int(world))


def _tuple(t):
    """(dataset, loader, evaluator) of a DataTuple-like object or a plain 3-tuple"""
    if hasattr(t, "dataset"):
        return t.dataset, t.loader, t.evaluator
    return t[0], t[1], t[2]


def _is_store(loader):
    from ..tools.resident import ResidentDataset
    return isinstance(loader, ResidentDataset)


class FineTuner:
    """What ``class VQA`` (src/vqa/vqacpv2.py:70-368) and ``class GQA`` (src/gqa/gqa_ood.py:70-431) share -- the names,
    signatures, printed lines and ``log.log`` lines are the reference's, the code is ours and runs on the pieces of this
    module and of ``engine``: an iteration is ``CapturedTrainer.load_resident`` + ``iteration(pick_branch(...))``, a
    validation sweep one ``CapturedPredictor`` with an ``AnswerLog``, and every score one ``AnswerLog.score_store`` launch
    with a read-back of a few words.  Nothing is read from the device per iteration: the losses come from a ``TrainLog``
    once per epoch (``log_every=N``: once per N iterations) and ahead of every validation sweep, so that a ``writer`` sees
    the reference's sequence of scalars.

    ``model``: a ``VQAModel`` / ``GQAModel`` on the GPU, snapshots loaded (the reference builds it inside the class; here
    the caller does, as for ``pretrain.lxmert_pretrain.LXMERT``); a model prepared with ``enable_data_parallel`` is refused
    unless ``data_parallel=True`` is given (below).
    ``train_tuple`` / ``valid_tuple``: ``(dataset, loader, evaluator)``.  A loader is a ``tools.resident.ResidentDataset``
    -- the device path: per-epoch order from ``store.order(epoch, shuffle=True, seed=args.seed, drop_last=True)``, batches
    gathered in HBM, scores computed against the store's own tables with the keep mask that gives a ``quesid2ans`` dict's
    semantics (a question that occurs twice counts once, with its last answer) -- or a ``DataLoaderX`` (the host path:
    ``load_batch``, the module's ``predict`` and the evaluator's dict walk).  ``args``: the flag namespace
    (``param.parse_args``: ``batch_size``, ``epochs``, ``lr``, ``optim``, ``delta``, ``sigma``, ``seed``, ``output``).
    ``valid_batch_size``: rows of the captured validation forward (default ``valid_factor * args.batch_size``).
    ``writer``: anything with ``add_scalar(tag, value, step)`` (the reference's ``--tf_writer``); None: nothing is written.

    The training engine is captured on the first batch of the first epoch; ``CapturedTrainer`` warms up with eager passes
    on that batch (optimiser steps at the head of the warm-up schedule), as it does for every caller.

    ``data_parallel=True`` (the reference's ``--multiGPU``, src/vqa/vqacpv2.py:106-107) with a model prepared by
    ``enable_data_parallel`` in a group of several ranks: ``train``, ``evaluate`` and ``predict`` are then COLLECTIVE calls, made
    on every rank, and both loaders must be resident stores (a host loader is a ValueError).  ``args.batch_size`` is per rank;
    an epoch has ``n // (B * world)`` GLOBAL steps, which ``t_total`` and ``val_schedule`` count; rank r takes its ``B`` rows of
    every global step (``store.order(..., rank=, world=)``); rank 0's branch draws for the epoch travel in one broadcast
    (``dist.sync_branches``); the losses are read through ``TrainLog.fold`` (the mean over the ranks); the epoch's answers are
    merged with ``AnswerLog.fold`` (interleaved back into the global order) and scored on every rank.  A validation sweep
    gives rank r the slice ``dist.shard_range(n, r, world)`` of the data set order, with no collective inside, and merges the
    logs in rank order before ONE ``score_store`` with the global keep mask.  Every rank keeps the same ``history``,
    ``valid_scores`` and best score; rank 0 alone prints, writes ``log.log`` and ``dump``, calls the ``writer`` and saves.
    Without the keyword, with a model that was not prepared, or in a one-rank group nothing changes."""

    order = "vqa"        # pass order and KL weight of ``CapturedTrainer``
    valid_factor = 1     # validation batch size over the training one (src/gqa/gqa_ood.py:82: 2)
    extra_tags = ()      # writer tags beyond the common ones, written with the value the reference leaves in them

    def __init__(self, model, train_tuple, valid_tuple=None, args=None, use_graph=True, valid_batch_size=None, log_every=None,
                 writer=None, data_parallel=False):
        import os
        from .. import param
        from ..dist import rank0_printer
        if getattr(model, "_grad_sync", None) is not None and not data_parallel:
            raise NotImplementedError("%s: a model prepared with enable_data_parallel is not supported by this driver (every "
                                      "rank would need its own epoch order and the ranks' scores would need combining); "
                                      "drive CapturedTrainer directly" % type(self).__name__)
        self.model, self.args = model, (param.args if args is None else args)
        self.data_parallel = bool(data_parallel)
        self.train_tuple, self.valid_tuple = train_tuple, valid_tuple
        self.use_graph, self.log_every, self.writer = use_graph, log_every, writer
        dp = self._dp()
        if dp is not None and dp[0] != 0:
            self.writer = None  # rank 0 alone calls the writer
        self.device = next(model.parameters()).device
        self.B = int(self.args.batch_size)  # data parallel: per rank
        self.valid_B = int(valid_batch_size) if valid_batch_size else self.valid_factor * self.B
        self.bce_loss = BCEWithLogitsLoss()
        batch_per_epoch = self._n_batches(_tuple(train_tuple)[1])  # data parallel: GLOBAL steps of world x B samples
        t_total = int(batch_per_epoch * self.args.epochs)
        if 'bert' in self.args.optim:
            rank0_printer(dp)(self._total_iters_line(t_total))
        self.optim = make_optimizer(model, self.args.lr, 2 * t_total, optim=self.args.optim)
        self.output = self.args.output
        os.makedirs(self.output, exist_ok=True)
        self.trainer, self.predictor = None, None
        self.sweeps = 0          # validation sweeps made so far (``predict`` calls)
        self.total_loss = 0.0    # the reference's running ``total_loss`` (never reset between epochs)
        self.history = []        # per epoch of ``train``: the unrounded numbers behind the lines of log.log
        self.valid_scores = []   # every validation score of ``train``, in the order the sweeps ran
        self.best_valid = 0.     # the best of them in the last ``train`` call

    # ------------------------------------------------------------------ what the two classes differ in
    def _total_iters_line(self, t_total):
        return f"BertAdam Total Iters: {t_total}\n{'*' * 80}"

    def _loss_divisor(self, trainer):
        """``total_loss += loss / logit.size(0)`` (src/vqa/vqacpv2.py:179)"""
        return trainer.static["target"].shape[0]

    def _epoch_lines(self, epoch, train_score, valid_score, best_valid):
        s = f"\nEpoch {epoch}: Train {train_score:.2f}\n"
        if valid_score is not None:
            s += f"\nEpoch {epoch}: Valid {valid_score * 100.:.2f}\n" + f"Epoch {epoch}: Best {best_valid * 100.:.2f}\n"
        return s

    def _print_lr(self):
        print(f"lr: {self.optim.state_dict()['param_groups'][0]['lr']}")  # src/vqa/vqacpv2.py:289

    # ------------------------------------------------------------------ engines
    def _dp(self):
        """(rank, world, group) when the driver was built with ``data_parallel=True`` on a model prepared by
        ``enable_data_parallel`` and the group has several ranks, else None: everything then runs as it always did"""
        gs = getattr(self.model, "_grad_sync", None)
        if not self.data_parallel or gs is None or gs.world <= 1:
            return None
        import torch.distributed as dist
        return dist.get_rank(gs.group), gs.world, gs.group

    def _n_batches(self, loader):
        """iterations of a training epoch; data parallel: GLOBAL steps of world x B samples"""
        dp = self._dp()
        if dp is not None:
            self._need_store(loader)
            return global_steps(len(loader), self.B, dp[1])
        return len(loader) // self.B if _is_store(loader) else len(loader)

    def _need_store(self, loader):
        if not _is_store(loader):
            raise ValueError("%s: under data parallelism the loader must be a ResidentDataset (its order is sharded over the "
                             "ranks); a host loader would have to be sharded by the caller" % type(self).__name__)

    def _engine(self, make_batch, B, n_batches):
        """the captured iteration at ``B`` rows with an answer log for a whole epoch and a training log for ``log_every``
        iterations (default: an epoch); built on ``make_batch()`` when there is none that fits"""
        from ..engine import AnswerLog, CapturedTrainer, TrainLog
        window = self.window = min(int(self.log_every), n_batches) if self.log_every else n_batches
        tr = self.trainer
        if tr is None or tr.static["target"].shape[0] != B or tr.answer_log.capacity < n_batches * B or tr.window < window:
            tr = CapturedTrainer(self.model, self.optim, make_batch(), sigma=self.args.sigma, order=self.order,
                                 use_graph=self.use_graph, answer_log=AnswerLog(n_batches * B, self.device),
                                 train_log=TrainLog(2 * window, self.device))
            tr.window = window
            self.trainer = tr
        return tr

    def _store_batch(self, store, samples):
        """the samples ``samples`` of a resident store as device tensors under the trainer's names, features in the store's
        own type: the batch the engine is captured on"""
        host = store.host_batch(samples, out_f32=store.tables["feats"].dtype == torch.float32)
        with_bias = getattr(self.model, "debias_loss", None) is not None
        return {k: v.to(self.device) for k, v in host.items() if k != "sample" and (k != "bias_index" or with_bias)}

    def _predictor(self, loader):
        """ONE captured validation forward with an answer log for the whole sweep, reused across sweeps"""
        from ..engine import AnswerLog, CapturedPredictor
        n = len(loader) if _is_store(loader) else len(loader.ds)
        N = loader.N if _is_store(loader) else loader.ds.shard.N
        B = self.valid_B if _is_store(loader) else max(self.valid_B, loader.B)
        p = self.predictor
        if p is None or p.log.capacity < n or p.B < B or p.static["feats"].shape[1] != N:
            p = self.predictor = CapturedPredictor(self.model, B, n_objects=N, use_graph=self.use_graph,
                                                   log=AnswerLog(n, self.device, with_scores=False))
        return p

    def _device_batch(self, item):
        """a loader item (ques_id, feats, boxes, sent, target, adj) as the trainer's static fields"""
        _, feats, boxes, sent, target, adj = item[:6]
        if not torch.is_tensor(sent) and not (len(sent) == 3 and torch.is_tensor(sent[0])):
            sent = self.model.lxrt_encoder.batcher.host_batch(list(sent)).clone()  # strings: tokenised here
        to = lambda t: (torch.from_numpy(t) if not torch.is_tensor(t) else t).to(self.device)  # noqa: E731
        return dict(feats=to(feats), boxes=to(boxes), input_ids=to(sent[0]), input_mask=to(sent[1]), segment_ids=to(sent[2]),
                    target=to(target), adj_true=to(adj))

    # ------------------------------------------------------------------ the reference's methods
    def _flush_losses(self, state):
        """ONE read of the training log: the scalars of the iterations since the last flush, to ``total_loss`` and the writer"""
        tr = self.trainer
        if tr is None or state["pending"] == 0:
            return
        from ..engine import TrainLog
        dp = self._dp()
        m = 2 * state["pending"]
        # data parallel (a COLLECTIVE read: every rank flushes after the same iterations): the mean of the ranks' records
        rec = tr.train_log.read() if dp is None else tr.train_log.fold(m, dp[2])
        tr.train_log.reset()
        values, kinds = rec["values"][-m:], rec["kinds"][-m:]
        if int(rec["cursor"]) != m or values.shape[0] != m:
            raise RuntimeError("%s: the training log holds %d records, %d were expected" % (type(self).__name__, int(rec["cursor"]), m))
        div = float(self._loss_divisor(tr))
        lr = self.optim.state_dict()['param_groups'][0]['lr']
        for k in range(state["pending"]):
            pair = range(2 * k, 2 * k + 2)
            plain = [j for j in pair if int(kinds[j]) == TrainLog.PLAIN]
            if len(plain) != 1:
                raise RuntimeError("%s: iteration without exactly one plain pass in the training log" % type(self).__name__)
            self.total_loss += float(values[plain[0], TrainLog.LOSS]) / div
            if self.writer is not None:
                it = state["train_iter"]
                # ``loss`` as the iteration leaves it: the SECOND pass's (VQA: the GGM pass, GQA: the plain pass)
                self.writer.add_scalar('Train/batch_loss', float(values[2 * k + 1, TrainLog.LOSS]), it)
                self.writer.add_scalar('Train/average_loss', self.total_loss / (it + 1), it)
                self.writer.add_scalar('lr', lr, it)
                for tag in self.extra_tags:
                    self.writer.add_scalar(tag, 0., it)
                state["train_iter"] += 1
        state["pending"] = 0

    def train(self, train_tuple, eval_tuple):
        from ..answers import to_quesid2ans
        dset, loader, evaluator = _tuple(train_tuple)
        resident = _is_store(loader)
        from ..dist import rank0_printer
        dp = self._dp()
        print = rank0_printer(dp)  # data parallel: rank 0 alone prints, writes log.log, calls the writer and saves
        n_batches = self._n_batches(loader)
        val_in_epoch = set(int(v) for v in val_schedule(n_batches))
        seed = int(getattr(self.args, "seed", 0) or 0)
        best_valid = 0.
        state = dict(pending=0, train_iter=0)

        def validate(epoch):
            nonlocal best_valid
            self._flush_losses(state)
            valid_score = self.evaluate(eval_tuple)
            self.valid_scores.append(valid_score)
            if valid_score > best_valid:
                best_valid = valid_score
                self.save("BEST")
            self.best_valid = best_valid
            return valid_score

        for epoch in range(self.args.epochs):
            branches = None
            if dp is not None:
                from ..dist import sync_branches
                # the epoch's samples in GLOBAL order, perm[:steps * B * world] (the train score is taken over it), then this
                # rank's B rows of every global step: the second call leaves ITS order in the store's device buffer
                global_order = loader.order(epoch, shuffle=True, seed=seed, drop_last=True, batch_size=self.B * dp[1])
                order = loader.order(epoch, shuffle=True, seed=seed, rank=dp[0], world=dp[1], drop_last=True, batch_size=self.B)
                batches = range(n_batches)
                # rank 0's draws for the whole epoch, ONE broadcast: ranks on different branches would exchange different ranges
                branches = sync_branches(n_batches, self.device, dp[2], delta=self.args.delta)
            elif resident:
                order = loader.order(epoch, shuffle=True, seed=seed, drop_last=True, batch_size=self.B)
                batches = range(n_batches)
            else:
                batches, ques_ids = loader, []
            for i, item in enumerate(batches):
                if resident:
                    tr = self._engine(lambda: self._store_batch(loader, order[:self.B]), self.B, n_batches)
                    tr.load_resident(loader, i * self.B)
                else:
                    batch = self._device_batch(item)
                    tr = self._engine(lambda: batch, batch["target"].shape[0], n_batches)
                    tr.load_batch(batch)
                    ques_ids.extend(item[0].tolist() if torch.is_tensor(item[0]) else item[0])
                if i == 0:
                    tr.answer_log.reset()  # nothing has been logged in this epoch: the plain pass below is its first append
                tr.iteration(pick_branch(self.args.delta, model=self.model) if branches is None else
                             ("rel" if branches[i] else "node"))
                state["pending"] += 1
                if state["pending"] == self.window:
                    self._flush_losses(state)
                if i in val_in_epoch and eval_tuple is not None:
                    valid_score = validate(epoch)
                    if self.writer is not None:
                        self.writer.add_scalar('Val/acc', valid_score, epoch)
                    print(f"\nEpoch {epoch}: Iter {i}: "
                          f"Valid {valid_score * 100.:.2f}\n"
                          f"Epoch {epoch}: Iter {i}: "
                          f"Best {best_valid * 100.:.2f}\n")
            self._flush_losses(state)
            # *compute train score*
            log = self.trainer.answer_log
            if dp is not None:
                # a COLLECTIVE merge: the ranks' logs interleaved back into the global order, scored on EVERY rank -- same bits
                from ..ops import FOLD_INTERLEAVE
                merged = log.fold(FOLD_INTERLEAVE, [n_batches * self.B] * dp[1], block=self.B, group=dp[2])
                train_score = merged.score_store(loader, order=global_order, keep=loader.keep_mask(global_order))["score"] * 100.
            elif resident:
                train_score = log.score_store(loader, order=loader._order, keep=loader.keep_mask(order))["score"] * 100.
            else:
                train_score = evaluator.evaluate(to_quesid2ans(ques_ids, log.read()[0], dset.label2ans)) * 100.
            valid_score = None
            if self.writer is not None:
                self._print_lr()
                self.writer.add_scalar('Train/acc', train_score, epoch)
            # *Do Validation*
            if eval_tuple is not None:
                valid_score = validate(epoch)
                self.save(f"BEST_{epoch}")
                if self.writer is not None:
                    self.writer.add_scalar('Val/acc', valid_score, epoch)
            self.history.append(dict(epoch=epoch, train=train_score, valid=valid_score, best=best_valid))
            log_str = self._epoch_lines(epoch, train_score, valid_score, best_valid)
            print(log_str, end='')
            if dp is None or dp[0] == 0:
                with open(self.output + "/log.log", 'a') as f:
                    f.write(log_str)
                    f.flush()
        if self.writer is not None and hasattr(self.writer, "close"):
            self.writer.close()

    def predict(self, eval_tuple, dump=None):
        """``{question_id: answer}`` of a split (src/vqa/vqacpv2.py:315-339): the module's ``predict`` through this driver's
        one captured predictor and its answer log"""
        dset, loader, evaluator = _tuple(eval_tuple)
        self.sweeps += 1
        dp = self._dp()
        if dp is not None:
            # a COLLECTIVE call: the dict is built from the merged log, the same on every rank; rank 0 alone writes ``dump``
            from ..answers import to_quesid2ans
            labels = self._sweep_ranks(loader, dp).read()[0]
            quesid2ans = to_quesid2ans(loader.ques_ids(range(len(loader))), labels, dset.label2ans)
            if dump is not None and dp[0] == 0:
                evaluator.dump_result(quesid2ans, dump)
            return quesid2ans
        return predict(self.model, (dset, loader, evaluator), dump, predictor=self._predictor(loader),
                       resident=loader if _is_store(loader) else None)

    def _sweep_ranks(self, loader, dp):
        """the data-parallel validation sweep (a COLLECTIVE call): rank r pushes the positions ``shard_range(n, r, world)`` of
        the data set order through its own predictor -- no collective inside the sweep, so the slices may be uneven; a rank
        with an empty slice pushes nothing -- and the ranks' logs are then concatenated in rank order (``AnswerLog.fold``)
        -> the merged log of all ``n`` answers in data set order, on every rank"""
        from ..dist import shard_range
        from ..ops import FOLD_CONCAT
        self._need_store(loader)
        rank, world, group = dp
        pred = self._predictor(loader)
        n = len(loader)
        mine = shard_range(n, rank, world)
        loader.order(0, shuffle=False, drop_last=False)
        pred.log.reset()
        for start in range(mine.start, mine.stop, pred.B):
            pred.push_resident(loader, start, min(pred.B, mine.stop - start))
        return pred.log.fold(FOLD_CONCAT, [len(shard_range(n, r, world)) for r in range(world)], group=group)

    def evaluate(self, eval_tuple, dump=None, by_group=False):
        """the evaluator's score of a split as a float (src/vqa/vqacpv2.py:341-344).  With a resident store and no ``dump``
        the sweep's answers never leave the device: ``score_store`` scores the log against the store's tables with the keep
        mask of its data set order.  ``by_group``: ``{"all": score, name: accuracy, ...}`` over the store's groups (no entry
        for a group without samples); the host path has no groups."""
        dset, loader, evaluator = _tuple(eval_tuple)
        if not _is_store(loader) or dump is not None:
            if by_group:
                raise ValueError("%s.evaluate: by_group needs a resident store with groups and no dump" % type(self).__name__)
            return evaluator.evaluate(self.predict(eval_tuple, dump))
        dp = self._dp()
        self.sweeps += 1
        if dp is not None:
            # every rank scores the merged log with the GLOBAL keep mask: a question id on both sides of a rank boundary
            # counts once, with its last answer, and every rank holds the same bits
            log = self._sweep_ranks(loader, dp)
        else:
            pred = self._predictor(loader)
            n = len(loader)
            loader.order(0, shuffle=False, drop_last=False)
            pred.log.reset()
            for start in range(0, n, pred.B):
                pred.push_resident(loader, start, min(pred.B, n - start))
            log = pred.log
        res = log.score_store(loader, keep=loader.keep_mask(), by_group=by_group)
        return dict(res["by_group"], all=res["score"]) if by_group else res["score"]

    def oracle_score(self, data_tuple):
        """the score of always answering a target's arg-max (src/vqa/vqacpv2.py:346-359): the target rows are gathered on
        the device and ``ops.answer_pick`` takes them as if they were logits"""
        from .. import ops
        from ..answers import to_quesid2ans
        dset, loader, evaluator = _tuple(data_tuple)
        pred = self._predictor(loader)
        log = pred.log
        log.reset()
        if _is_store(loader):
            n, s = len(loader), pred.static
            tgt = torch.zeros(pred.B, loader.A, device=self.device)
            loader.order(0, shuffle=False, drop_last=False)
            for start in range(0, n, pred.B):
                b = min(pred.B, n - start)
                loader.fill(dict(feats=s["feats"], boxes=s["boxes"], input_ids=s["ids"][0], input_mask=s["ids"][1],
                                 segment_ids=s["ids"][2], target=tgt), start, b)
                log.note(b)
                ops.answer_pick(tgt[:b], log)
            return log.score_store(loader, keep=loader.keep_mask())["score"]
        ques_ids = []
        for item in loader:
            target = item[4].to(self.device).float().contiguous()
            log.note(target.shape[0])
            ops.answer_pick(target, log)
            ques_ids.extend(item[0].tolist() if torch.is_tensor(item[0]) else item[0])
        return evaluator.evaluate(to_quesid2ans(ques_ids, log.read()[0], dset.label2ans))

    def save(self, name):
        """data parallel: rank 0 writes (the replicas are equal), the other ranks write nothing"""
        import os
        dp = self._dp()
        state = self.model.state_dict()  # under the sharded update a collective (the masters are gathered): on every rank
        if dp is not None and dp[0] != 0:
            return
        torch.save(state, os.path.join(self.output, "%s.pth" % name))

    def load(self, path):
        print("Load model from %s" % path)
        state_dict = torch.load("%s.pth" % path, map_location="cpu", weights_only=True)
        self.model.load_state_dict(state_dict)


class VQA(FineTuner):
    """``class VQA`` of src/vqa/vqacpv2.py:70-368: plain pass first, KL weight 8, ``total_loss`` over the batch size"""


def save_training_state(path, model, optim, **extra):
    """everything an exact resume needs, which ``VQA.save`` (src/vqa/vqacpv2.py:361-363, model weights only) leaves
    out: BertAdam moments and step counters (reference state layout), the dropout / noise Philox state, the host
    branch-choice generator, and whatever the caller adds (epoch, iteration, best score)."""
    rt = runtime_of(model)
    # under the sharded update (ZeRO-1) this is a collective: every rank calls it (they all hold the gathered state
    # afterwards; let one of them pass a real ``path`` and the others ``None`` to write a single file)
    rt.arena.gather_sharded_state()
    guard = getattr(model, "_replica_guard", None)
    if guard is not None:
        # everything is comparable now (masters and moments are whole): a drifted run leaves no checkpoint behind.
        # With a guard this is a COLLECTIVE under the replicated update too: EVERY rank calls save_training_state (path
        # None where nothing is to be written); a rank that comes alone gets a RuntimeError after
        # XGGM_COLLECTIVE_TIMEOUT seconds (dist._meet), not a hung group
        guard.check("checkpoint", level="state", rendezvous=True)
    ck = {"model": model.state_dict(), "optimizer": optim.state_dict(), "rng": rt.rng.cpu(),
          "python_random": random.getstate(), "extra": extra}
    if path is not None:
        torch.save(ck, path)
    return ck


def load_training_state(path, model, optim):
    """restores what ``save_training_state`` wrote, in place (captured graphs stay valid); returns ``extra``"""
    ck = torch.load(path, map_location="cpu", weights_only=True)
    model.load_state_dict(ck["model"])
    rt = runtime_of(model)  # creates the arena if this model has not run yet, refreshes the bf16 shadows
    optim.load_state_dict(ck["optimizer"])
    rt.rng.copy_(ck["rng"])
    st = ck["python_random"]
    random.setstate((st[0], tuple(st[1]), st[2]))
    return ck["extra"]
