"""From a loader batch to the arguments of ``LXRTPretraining.forward`` on the device.

The reference makes a pre-training batch on the host, one example at a time (src/pretrain/lxmert_pretrain.py:76-215:
``random_word`` per token, ``random_feat`` per object with a copy of the example's features, the QA answer draw), and uploads
both ``feat`` and ``masked_feat`` (:258-306).  ``DeviceFeatures`` takes the UNCORRUPTED batch that is already on the device and
produces the same arguments with one HIP launch (``ops.pretrain_corrupt``, contract: xggm_pretrain_corrupt_* in
include/xggm.h): only the clean features cross the host link, once.

Draws: five Philox streams ``sid_base + 0..4`` (``ops.PRETRAIN_DRAWS``: u_word, u_word_pick [B, T]; u_obj, u_obj_pick [B, O];
u_ans [B]) at the state ``rng``; the caller advances ``rng`` (``ops.rng_advance``) between batches.  ``draws`` replaces any of
them by explicit buffers (tests pin the kernel to the reference's functions that way).

Deviations from the reference, both documented in INTEGRATION.md:
  * the random replacement row comes from ``pool`` [P, F] (default: the batch's own clean features as [B O, F]) instead of
    ``torchdset.random_feat()``, a random object of a random datum of the whole data set; a loader can pass a larger pool,
    and a resident corpus (``pretrain.resident.ResidentPretrainSet``) passes every object of every image;
  * an example with several answer keys draws by inverse CDF on one uniform instead of ``np.random.multinomial``: the same
    distribution, not the same stream.

The matched-sentence swap of src/pretrain/lxmert_data.py:173-183 is opt-in (``DeviceFeatures(match_rate=0.5)``): one more
launch (``ops.pretrain_swap``, contract: xggm_pretrain_swap in include/xggm.h) AHEAD of the corruption, which then reads the
swapped ids and the new ``is_matched`` -- the reference's order (the data set swaps, ``convert_example_to_features`` masks).
Its two deviations (a bounded number of candidates, ``randint`` as floor(u n)) are written down in INTEGRATION.md as well.

The driver loop is at the bottom: ``InputExample``, ``collate_examples`` and ``LXMERT``, our own code behind the names and
signatures of ``class LXMERT`` (src/pretrain/lxmert_pretrain.py:221-409), running on ``engine.CapturedPretrainer``.

The batch itself can come from the device: ``pretrain.resident.ResidentPretrainSet`` keeps a corpus of ``InputExample``s in
HBM and one launch gathers a clean batch with the swap fused in -- drawn from EVERY sample, as the reference draws -- in
place of ``collate_examples`` and thirteen copies; ``LXMERT(resident=True)`` takes such a store as the loader of a tuple.

The feature files have a reader of their own: ``tools.tsv.load_obj_tsv_device`` decodes a bottom-up TSV on the device into
an ``ObjTable``, which ``pretrain.resident.pretrain_tables(..., images=table)`` hands to the store without a copy
(``utils.load_obj_tsv`` is the host path).  Out of scope here: the json annotation readers and the evaluator of
src/pretrain/lxmert_data.py (``LXMERTDataset``, ``LXMERTTorchDataset``, ``LXMERTEvaluator``; any ``(dataset, loader,
evaluator)`` whose loader yields lists of ``InputExample`` or is a ``ResidentPretrainSet`` serves), the packed loader ring
of the fine-tuning side, and fusing the masking into the visual-embedding product's input read.

Data parallel (the reference's ``--multiGPU``, :255-256): ``enable_data_parallel`` prepares the model, the captured step
exchanges the gradients between its two graphs (``engine.CapturedPretrainer``) and ``LXMERT`` shards a resident store over
the ranks; the sharded update, the staged exchange and sharding a host loader are out of scope."""
import os

import numpy as np
import torch

from .. import ops
from ..dist import rank0_printer as _printer, shard_range  # noqa: F401  (shared with the fine-tuning drivers)
from ..trainlog import LOSSES_NAME  # src/pretrain/lxmert_pretrain.py:218

SID_BASE = 0x70726500  # far from the module streams (16 * (i + 1) + k) and the graph streams


def pack_labels(labels, K):
    """``example.label`` dicts (answer id -> score, insertion order; ``None`` or empty: no label) of one batch ->
    (label_ids int64 [B, K] padded with -1, label_scores float32 [B, K]) on the host.  More than K keys raises."""
    K = int(K)
    if K <= 0:
        raise ValueError("pack_labels: K=%d must be positive" % K)
    ids = np.full((len(labels), K), -1, dtype=np.int64)
    scores = np.zeros((len(labels), K), dtype=np.float32)
    for b, lab in enumerate(labels):
        if not lab:
            continue
        if len(lab) > K:
            raise ValueError("pack_labels: example %d has %d answer keys, at most %d fit" % (b, len(lab), K))
        for j, (k, v) in enumerate(lab.items()):
            if int(k) < 0:
                raise ValueError("pack_labels: example %d has the negative answer id %d" % (b, int(k)))
            ids[b, j], scores[b, j] = int(k), v
    return torch.from_numpy(ids), torch.from_numpy(scores)


class DeviceFeatures:
    """``convert_example_to_features`` (src/pretrain/lxmert_pretrain.py:139-215) for a whole batch on the device.

    ``__call__`` returns the positional arguments of ``LXRTPretraining.forward`` in the reference's order (:302-305):
    ``input_ids, segment_ids, input_mask, lm_labels, masked_feat, pos, obj_labels, matched_labels, ans`` with
    ``obj_labels = {'obj': (obj_labels, obj_confs), 'attr': (attr_labels, attr_confs), 'feat': (feat, feat_mask)}``.
    The five output buffers are allocated once per (shape, dtype, device) and reused -- a call allocates nothing after the
    first and can be captured; a consumer that keeps a result across calls has to copy it.

    ``match_rate`` (None: no swap, nothing more is launched): the share of matched examples whose sentence is replaced by one
    of another image (the reference fixes 0.5, src/pretrain/lxmert_data.py:178).  The swap runs first, from ``img_ids`` [B]
    (an integer per image) and ``sent_pool`` = (pool_ids, pool_mask, pool_img) or None (the batch's own sentences); the
    corruption reads the swapped ids, ``input_mask`` and ``matched_labels`` of the result are the swapped ones, and an
    unmatched row gets ``ans = -1``.  ``swap_exhausted`` (int32 [1] on the device) counts the rows that found no other image
    among their ``ops.PRETRAIN_SWAP_TRIES`` candidates and stayed matched."""

    def __init__(self, word_mask_rate=0.15, obj_mask_rate=0.15, vocab_size=30522, mask_id=103, sid_base=SID_BASE, max_labels=4,
                 match_rate=None):
        self.word_mask_rate, self.obj_mask_rate = float(word_mask_rate), float(obj_mask_rate)
        self.vocab_size, self.mask_id, self.sid_base, self.max_labels = int(vocab_size), int(mask_id), int(sid_base), int(max_labels)
        self.match_rate = None if match_rate is None else float(match_rate)
        if self.match_rate is not None and not 0.0 <= self.match_rate <= 1.0:
            raise ValueError("DeviceFeatures: match_rate %r outside [0, 1]" % (match_rate,))
        self.swap_exhausted = None
        self._out, self._swap = {}, {}

    @classmethod
    def from_args(cls, args, swap=False, **kw):
        """rates from a flag namespace (``--wordMaskRate`` / ``--objMaskRate``, src/param.py:102-105); ``swap=True``: the
        sentence swap follows ``--taskMatched`` (rate 0.5 when the flag is set, as src/pretrain/lxmert_data.py:177-178)"""
        if swap and "match_rate" not in kw:
            kw["match_rate"] = 0.5 if getattr(args, "task_matched", False) else None
        return cls(word_mask_rate=args.word_mask_rate, obj_mask_rate=args.obj_mask_rate, **kw)

    def _swap_buffers(self, input_ids):
        key = (tuple(input_ids.shape), input_ids.device)
        out = self._swap.get(key)
        if out is None:
            dev = input_ids.device
            if self.swap_exhausted is None or self.swap_exhausted.device != dev:
                self.swap_exhausted = torch.zeros(1, device=dev, dtype=torch.int32)
            out = dict(input_ids=torch.empty_like(input_ids), input_mask=torch.empty_like(input_ids),
                       is_matched=torch.empty(input_ids.shape[0], device=dev, dtype=torch.int64), exhausted=self.swap_exhausted)
            self._swap[key] = out
        return out

    def _buffers(self, input_ids, feats):
        B, T = input_ids.shape
        key = (tuple(feats.shape), T, feats.dtype, feats.device)
        out = self._out.get(key)
        if out is None:
            dev = feats.device
            out = dict(input_ids=torch.empty((B, T), device=dev, dtype=torch.int64),
                       masked_lm_labels=torch.empty((B, T), device=dev, dtype=torch.int64),
                       masked_feat=torch.empty_like(feats),
                       feat_mask=torch.empty(feats.shape[:2], device=dev, dtype=torch.float32),
                       ans=torch.empty(B, device=dev, dtype=torch.int64))
            self._out[key] = out
        return out

    def __call__(self, input_ids, input_mask, segment_ids, feats, boxes, obj_labels, obj_confs, attr_labels, attr_confs,
                 is_matched, label_ids, label_scores, rng, pool=None, draws=None, img_ids=None, sent_pool=None):
        if label_ids.dim() != 2 or label_ids.shape[1] != self.max_labels:
            raise ValueError("DeviceFeatures: label_ids %s, [B, %d] expected (pack_labels(labels, %d))"
                             % (tuple(label_ids.shape), self.max_labels, self.max_labels))
        draws = dict(draws or {})
        swap_draws = {k: draws.pop(k) for k in ops.PRETRAIN_SWAP_DRAWS if k in draws}
        if self.match_rate is not None:
            if img_ids is None:
                raise ValueError("DeviceFeatures: match_rate needs img_ids [B] (an integer per image)")
            sw = ops.pretrain_swap(input_ids, input_mask, img_ids, self.match_rate, matched_in=is_matched, pool=sent_pool,
                                   rng=rng, sid_base=self.sid_base, draws=swap_draws, out=self._swap_buffers(input_ids))
            input_ids, input_mask, is_matched = sw["input_ids"], sw["input_mask"], sw["is_matched"]
        elif swap_draws:
            raise ValueError("DeviceFeatures: swap draws %s without a match_rate" % sorted(swap_draws))
        out = ops.pretrain_corrupt(input_ids, input_mask, feats, is_matched, label_ids, label_scores, self.word_mask_rate,
                                   self.obj_mask_rate, self.vocab_size, self.mask_id, rng=rng, sid_base=self.sid_base,
                                   pool=pool, draws=draws, out=self._buffers(input_ids, feats))
        visn = {'obj': (obj_labels, obj_confs), 'attr': (attr_labels, attr_confs), 'feat': (feats, out["feat_mask"])}
        return (out["input_ids"], segment_ids, input_mask, out["masked_lm_labels"], out["masked_feat"], boxes, visn,
                is_matched, out["ans"])


# ----------------------------------------------------------------------------------------------- data parallelism


def enable_data_parallel(model, group=None, wire_dtype=None, check_every=None, check_level="weights", overlap=False,
                         zero1=False):
    """one process per GPU for an ``LXRTPretraining`` (the reference's ``--multiGPU``, src/pretrain/lxmert_pretrain.py:255-256):
    what ``vqa.vqacpv2.enable_data_parallel`` does for a ``VQAModel``.  Rank 0's parameters go to everyone; the rank is
    folded into the Philox seed (same constant), so every rank draws its OWN masks, swaps, dropout and noise; a
    ``dist.GradSync`` averages the flat gradient arena between the backward and the fused clip + update of every step
    (``engine.CapturedPretrainer``: two graphs with the exchange between them) -- over ``rt.arena.grads``, or IN PLACE on the
    bf16 wire arena when the storage is bf16 and ``wire_dtype=torch.bfloat16``; the clip norm is read after the exchange
    (``arena.sq_enabled = False``, ``row_list_enabled = False``).  ``check_every`` / ``check_level``: a
    ``dist.ReplicaGuard`` that ``CapturedPretrainer.step`` ticks.

    The word table: the tied decoder of the masked-LM head gives EVERY row of the vocab x H table a gradient, so with
    ``task_mask_lm`` the table is exchanged densely; only with the masked-LM task off are the rows of the step's tokens all
    there is, and ``GradSync.set_sparse_table`` is used (wire arena only, as in fine-tuning).

    Scope: the replicated update with a plain exchange.  ``zero1=True`` (the sharded update) and ``overlap=True`` (the
    exchange staged under the backward) raise ``NotImplementedError`` before anything is touched; ``rt.cut_enabled`` is
    False."""
    if zero1:
        raise NotImplementedError("pretrain.lxmert_pretrain.enable_data_parallel: the sharded update (zero1=True) is not "
                                  "built for pre-training; the update is replicated")
    if overlap:
        raise NotImplementedError("pretrain.lxmert_pretrain.enable_data_parallel: the overlapped, staged exchange "
                                  "(overlap=True) is not built for pre-training; the exchange runs between the two graphs")
    import torch.distributed as dist
    from ..dist import GradSync, broadcast_params
    from ..runtime import runtime_of
    rt = runtime_of(model)
    broadcast_params(rt.arena, group)
    rank = dist.get_rank(group) if dist.is_initialized() else 0
    if rank:
        # seed word of the device-resident {seed, offset} pair; saved / restored with the training state
        rt.rng[0] = (int(rt.rng[0].item()) + rank * 0x9E3779B97F4A7C15) & 0x7FFFFFFFFFFFFFFF
    inplace = wire_dtype == torch.bfloat16 and rt.arena.shadow is not None and os.environ.get("XGGM_DP_WIRE_ARENA", "1") != "0"
    if inplace:
        rt.arena.enable_wire()  # matrix gradients are born in the wire arena, reduced in place and read by the update
    gs = GradSync(rt.arena.grads, group, wire_dtype, arena=rt.arena if inplace else None)
    if inplace and not model.task_mask_lm and os.environ.get("XGGM_DP_SPARSE_EMB", "1") != "0":
        wt = model.bert.embeddings.word_embeddings.weight
        xg = getattr(wt, "_xg", None)
        if xg is not None and xg[0] is rt.arena:
            gs.set_sparse_table(xg[1], wt.shape[0], wt.shape[1], lambda: rt.emb_ids)
    object.__setattr__(model, "_grad_sync", gs)
    rt.arena.sq_enabled = False  # the clip norm is that of the AVERAGED gradients: read them after the exchange
    rt.arena.row_list_enabled = False  # ... and the word table's gradient holds the OTHER ranks' rows too
    rt.cut_enabled = False
    if check_every is not None:
        from ..dist import ReplicaGuard
        object.__setattr__(model, "_replica_guard", ReplicaGuard(rt.arena, group, every=check_every, level=check_level))
    return model


def combine_sums(sums, steps, group=None):
    """the data-parallel validation sweep's loss sums, combined once after the sweep: every rank hands in its fp64 host
    sums ``sums`` (any number of values, the same number on every rank) and its step count; they are all-gathered and
    added in RANK ORDER in fp64 -> (numpy fp64 array of the totals, total steps): the same bits on every rank.  The sums
    are sums of per-step means, so total / steps is the mean of the per-step means the reference prints.  Without a
    process group (or on one rank): the input."""
    import torch.distributed as dist
    mine = np.asarray(list(sums) + [float(steps)], dtype=np.float64)
    if not dist.is_initialized() or dist.get_world_size(group) == 1:
        return mine[:-1].copy(), int(steps)
    world = dist.get_world_size(group)
    t = torch.from_numpy(mine)
    if dist.get_backend(group) == "nccl":
        t = t.cuda()
    parts = [torch.empty_like(t) for _ in range(world)]
    dist.all_gather(parts, t, group=group)
    return combine_sums_host([p.cpu().numpy()[:-1] for p in parts], [p.cpu().numpy()[-1] for p in parts])


def combine_sums_host(per_rank_sums, per_rank_steps):
    """``combine_sums`` restated without a process group: lists over the ranks -> (totals, steps), added in rank order"""
    total = np.zeros(len(per_rank_sums[0]), dtype=np.float64)
    steps = 0
    for s, k in zip(per_rank_sums, per_rank_steps):
        total = total + np.asarray(s, dtype=np.float64)
        steps += int(k)
    return total, steps


# ----------------------------------------------------------------------------------------------- the driver loop


class InputExample(object):
    """one example as the data set hands it over (src/pretrain/lxmert_data.py:26-38): ``visual_feats`` = (feats [O, F],
    boxes [O, 4]), ``obj_labels`` / ``attr_labels`` = (ids [O], confidences [O]), ``label`` = {answer id: score} or None"""

    def __init__(self, uid, sent, visual_feats=None, obj_labels=None, attr_labels=None, is_matched=None, label=None):
        self.uid, self.sent, self.visual_feats = uid, sent, visual_feats
        self.obj_labels, self.attr_labels, self.is_matched, self.label = obj_labels, attr_labels, is_matched, label


def image_id(example):
    """the image id of an example as a string: ``example.img_id`` when the example carries one, else the head of the
    reference's uid ``"<img_id>_<dset>_<idx>"`` (src/pretrain/lxmert_data.py:80-81, which returns it as a 1-tuple)"""
    img = getattr(example, "img_id", None)
    if img is None:
        uid = example.uid[0] if isinstance(example.uid, (tuple, list)) else example.uid
        parts = str(uid).rsplit("_", 2)
        img = parts[0] if len(parts) == 3 else str(uid)
    return str(img)


def image_key(example):
    """a stable non-negative integer per distinct image id (``image_id``): the same in every batch and every process, so
    that a sentence pool may span batches"""
    import hashlib
    return int.from_bytes(hashlib.blake2b(image_id(example).encode("utf-8"), digest_size=8).digest(), "little") >> 1


def collate_examples(examples, tokenizer, max_seq_length, max_labels):
    """a list of ``InputExample`` -> the CLEAN host batch ``engine.CapturedPretrainer`` takes (dict of CPU tensors): each
    sentence as ``[CLS] tokens[:max_seq_length - 2] [SEP]`` zero-padded with segment ids 0 (the layout of
    src/pretrain/lxmert_pretrain.py:146-183 without its masking), the stacked visual arrays, ``pack_labels`` and
    ``img_ids`` (``image_key``).  No masking and no swap: both happen on the device (``DeviceFeatures``)."""
    B, T = len(examples), int(max_seq_length)
    if B == 0 or T < 2:
        raise ValueError("collate_examples: %d examples, max_seq_length %d" % (B, T))
    ids = np.zeros((B, T), dtype=np.int64)
    mask = np.zeros((B, T), dtype=np.int64)
    for b, ex in enumerate(examples):
        tokens = ["[CLS]"] + tokenizer.tokenize(ex.sent.strip())[:T - 2] + ["[SEP]"]
        w = tokenizer.convert_tokens_to_ids(tokens)
        ids[b, :len(w)], mask[b, :len(w)] = w, 1
    stack = lambda f, dt: torch.from_numpy(np.stack([np.asarray(f(ex)) for ex in examples]).astype(dt, copy=False))
    label_ids, label_scores = pack_labels([ex.label for ex in examples], max_labels)
    return dict(input_ids=torch.from_numpy(ids), input_mask=torch.from_numpy(mask), segment_ids=torch.zeros((B, T), dtype=torch.int64),
                feats=stack(lambda e: e.visual_feats[0], np.float32), boxes=stack(lambda e: e.visual_feats[1], np.float32),
                obj_labels=stack(lambda e: e.obj_labels[0], np.int64), obj_confs=stack(lambda e: e.obj_labels[1], np.float32),
                attr_labels=stack(lambda e: e.attr_labels[0], np.int64), attr_confs=stack(lambda e: e.attr_labels[1], np.float32),
                is_matched=torch.tensor([int(ex.is_matched) for ex in examples], dtype=torch.int64),
                label_ids=label_ids, label_scores=label_scores,
                img_ids=torch.tensor([image_key(ex) for ex in examples], dtype=torch.int64))


class LXMERT:
    """``class LXMERT`` of src/pretrain/lxmert_pretrain.py:221-409 -- the names, signatures, return contracts and printed
    lines are the reference's, the code is ours and runs on ``engine.CapturedPretrainer``: batches are collated CLEAN on the
    host, swapped and masked on the device, and a step is one graph replay.

    ``model``: an ``LXRTPretraining`` on the GPU (the reference builds it from the downloaded BERT weights; offline the
    caller builds it); ``tokenizer``: anything with ``tokenize`` / ``convert_tokens_to_ids``; ``args``: the flag namespace
    (``param.parse_args``: task flags, rates, ``epochs``, ``lr``, ``output``).  ``--taskMatched`` switches the device swap on
    (rate 0.5): examples arrive with ``is_matched = 1`` and their own sentence.

    ``train_batch`` / ``valid_batch`` keep the reference's return contract ``(loss.item(), losses numpy [1, n],
    ans_logit)`` at ONE read per call, for callers that keep the reference's outer loop; ``forward`` is one eager pass with
    the reference's ``(loss, losses on the host, ans_logit)``.  ``train`` /
    ``evaluate_epoch`` read nothing per step: the losses come from the ``TrainLog`` and the answers from the ``AnswerLog``
    once per epoch -- with ``log_every=N`` once per N steps (the logs then hold N steps instead of an epoch) -- together
    with ``CapturedPretrainer.check()``; ``uid2ans`` is built from the answer log and the uids kept on the host in call
    order.

    Two engines, each captured at the size of the first batch it sees: ``engine`` (training; it also holds a forward-only
    graph at the training batch size) and, when validation comes with a batch size of its own -- the reference validates at
    512 or 2048 against ``--bs`` (src/pretrain/lxmert_pretrain.py:50-52) -- or before any training, ``valid_engine``, a
    validation-only ``CapturedPretrainer(optim=None)`` at THAT size: validation is a replayed graph too and never takes an
    optimiser step.  Only a ragged last batch (fewer rows than the engine's) runs EAGERLY (the same calls on the batch as it
    is: padding it would change its mean losses); its answers land in the same log.  An answer log holds ``steps x batch
    size`` SAMPLES of its own engine and is read back early when the next batch would not fit.

    A tuple's loader may be a ``pretrain.resident.ResidentPretrainSet`` (build ``LXMERT(resident=True)``: the store's gather
    launch swaps, ``features`` does not): the per-epoch order comes from the store (training shuffles with ``args.seed`` and
    drops the ragged tail, as the reference's train loader does), a step is ``load_resident`` + ``step()``, validation runs a
    short last batch eagerly through buffers of its own size, and ``uid2ans`` pairs the answer log with ``store.uids(order)``.
    ``train_batch(optim, (store, start[, rows]))`` / ``valid_batch((store, start[, rows]))`` take rows of the order the store
    currently holds.

    Data parallel (``enable_data_parallel(model)`` before the driver is built, one process per GPU; the reference's
    ``--multiGPU``, :255-256, with its ``loss.mean()`` over the replicas, :311-313): the loader must be a store.  ``train`` and
    ``evaluate_epoch`` are then COLLECTIVE calls, made on every rank.  Training: every rank takes its ``B`` rows of each
    global step of ``world x B`` (``store.order(..., rank=, world=)``), ``t_total`` counts global steps, and the printed losses
    come from the logs FOLDED over the ranks (``TrainLog.fold``: the mean of the ranks' values per step).  Validation: rank r
    walks the slice ``shard_range(n, r, world)`` of the sweep with no collective inside, so ranks may take different numbers
    of steps (none included); after the sweep the fp64 sums are combined in rank order (``combine_sums``: weighted by steps,
    the printed mean is that of the per-step means) and the ``uid2ans`` dicts merged in rank order.  Rank 0 alone prints,
    calls the evaluator and writes snapshots (``save`` is a no-op elsewhere); every rank returns the same numbers.

    The printed per-term line names the terms that are on; the reference zips LOSSES_NAME with however many terms there
    are, which mislabels them as soon as a task is off (:366, :402) -- with all tasks on the lines are the same."""

    def __init__(self, max_seq_length, model, tokenizer, args=None, use_graph=True, log_every=None, max_labels=4,
                 vocab_size=None, mask_id=None, resident=False):
        from .. import param
        from ..lxrt.modeling import check_sequence_limits
        check_sequence_limits("LXMERT", max_seq_length, config=getattr(model, "config", None))
        self.max_seq_length, self.model, self.tokenizer = max_seq_length, model, tokenizer
        self.args = param.args if args is None else args
        self.use_graph, self.log_every, self.max_labels = use_graph, log_every, int(max_labels)
        vocab = getattr(tokenizer, "vocab", None)
        vocab_size = vocab_size if vocab_size is not None else (len(vocab) if vocab is not None else model.config.vocab_size)
        mask_id = mask_id if mask_id is not None else (vocab["[MASK]"] if vocab is not None else 103)
        # with a resident store the swap is fused into its gather launch: ``features`` must not swap a second time
        self.features = DeviceFeatures.from_args(self.args, swap=not resident, vocab_size=vocab_size, mask_id=mask_id, max_labels=max_labels)
        self.device = next(model.parameters()).device
        self.engine, self._optim = None, None  # the training engine and the optimiser it was captured with
        self.valid_engine = None               # validation at another batch size, or before any training

    # ------------------------------------------------------------------ batches and the engines
    def _device_batch(self, examples):
        host = collate_examples(examples, self.tokenizer, self.max_seq_length, self.max_labels)
        return {k: v.to(self.device, non_blocking=True) for k, v in host.items()}

    @staticmethod
    def _is_store(loader):
        from .resident import ResidentPretrainSet
        return isinstance(loader, ResidentPretrainSet)

    def resident_order(self, store, kind, epoch=0):
        """the order of one sweep over a store: training shuffles with ``args.seed`` and drops the ragged tail (the reference's
        train loader: shuffle, drop_last), validation walks every sample in the store's own order"""
        train = kind == "train"
        if store.batch_size is None:
            raise ValueError("LXMERT: a ResidentPretrainSet loader needs its batch_size")
        dp = self._dp()
        if dp is not None and train:
            # global step s covers perm[s B world : (s + 1) B world], this rank takes its B of it: B is per rank
            return store.order(epoch, shuffle=True, seed=int(getattr(self.args, "seed", 0) or 0), rank=dp[0], world=dp[1],
                               drop_last=True, batch_size=store.batch_size)
        return store.order(epoch, shuffle=train, seed=int(getattr(self.args, "seed", 0) or 0), drop_last=train,
                           batch_size=store.batch_size)

    def _dp(self):
        """(rank, world, group) when the model was prepared by ``enable_data_parallel`` and the group has several ranks, else
        None: everything below then runs as it always did"""
        gs = getattr(self.model, "_grad_sync", None)
        if gs is None or gs.world <= 1:
            return None
        import torch.distributed as dist
        return dist.get_rank(gs.group), gs.world, gs.group

    def _n_batches(self, loader, kind):
        """steps of one sweep: GLOBAL steps of a training epoch, THIS rank's steps of a validation sweep"""
        dp = self._dp()
        if not self._is_store(loader):
            if dp is not None:
                raise ValueError("LXMERT: under data parallelism the loader must be a ResidentPretrainSet (its order is "
                                 "sharded over the ranks); a host loader would have to be sharded by the caller")
            return len(loader)
        B = loader.batch_size
        if kind == "train":
            return len(loader) // (B * (dp[1] if dp is not None else 1))
        n = len(loader) if dp is None else len(shard_range(len(loader), dp[0], dp[1]))
        return -(-n // B)

    def _resident_batch(self, store, start, rows, like=None):
        """buffers of ``rows`` rows filled from the store, swap included: the first batch an engine is built on (``like`` None:
        a clean gather, nothing is drawn) or a ragged last batch that runs eagerly through buffers of its own size"""
        from ..runtime import runtime_of
        bufs = store.buffers(rows)
        if like is None:
            return store.fill(bufs, start, rows, swap=False)
        store.fill(bufs, start, rows, rng=runtime_of(self.model).rng, sid_base=self.features.sid_base)
        if "feat_pool" in like.static:
            bufs["feat_pool"] = like.static["feat_pool"]
        return bufs

    def _build(self, optim, batch, window, resident=None):
        from ..engine import AnswerLog, CapturedPretrainer, TrainLog
        B = batch["input_ids"].shape[0]
        e = CapturedPretrainer(self.model, optim, batch, self.features, clip=1.0, use_graph=self.use_graph, resident=resident,
                               train_log=TrainLog(window, self.device) if optim is not None else None,
                               valid_log=TrainLog(window, self.device),
                               answer_log=AnswerLog(window * B, self.device, with_scores=False) if self.model.task_qa else None)
        e.window = window
        return e

    def _train_engine(self, optim, batch, window, resident=None):
        """the captured step for ``optim``, built at the first training batch (its size is the static one) with logs of
        ``window`` steps; rebuilt when the caller comes with another optimiser or a longer window"""
        if self.engine is None or optim is not self._optim or window > self.engine.window:
            self.engine, self._optim = self._build(optim, batch, window, resident), optim
        return self.engine

    def _valid_engine(self, batch, window, resident=None):
        """the forward-only graph for batches of this size: the training engine's when the size is its own, else a
        validation-only engine captured at this size (rebuilt for a longer window or a larger batch)"""
        B = batch["input_ids"].shape[0]
        e = self.engine
        if e is not None and e.B == B and window <= e.window:
            return e
        e = self.valid_engine
        if e is None or window > e.window or B > e.B:
            self.valid_engine = e = self._build(None, batch, window, resident)
        return e

    @staticmethod
    def _read(out):
        flat = torch.cat([out[0].reshape(1), out[1].reshape(-1)]).cpu()  # the ONE read of the call
        return float(flat[0]), flat[1:].reshape(1, -1).numpy(), out[2]

    def _reset_logs(self, e):
        for log in (e.train_log, e.valid_log, e.answer_log):
            if log is not None:
                log.reset()

    def forward(self, examples):
        """src/pretrain/lxmert_pretrain.py:258-306 -> (loss, losses [1, n] on the host, ans_logit): ONE eager, uncaptured pass
        in the model's current mode -- collate, swap and mask on the device, ``model(...)``.  ``loss`` carries its autograd
        graph in training mode; a caller that goes on by hand ends the pass with ``runtime.backward(loss)`` and
        ``clip_and_step(model, optim, 1.0, advance=True)`` (the draws of the next pass come with that advance).
        ``train_batch`` / ``valid_batch`` do not come through here: they are one captured step each."""
        from ..runtime import runtime_of
        b = self._device_batch(examples)
        from ..engine import CapturedPretrainer
        args = self.features(*[b[k] for k in CapturedPretrainer.KEYS], runtime_of(self.model).rng, img_ids=b["img_ids"])
        loss, losses, ans_logit = self.model(*args)
        return loss, losses.detach().cpu(), ans_logit

    def train_batch(self, optim, batch):
        """src/pretrain/lxmert_pretrain.py:308-318 -> (loss.item(), losses numpy [1, n], ans_logit)"""
        if self._is_store(batch[0]):
            return self._resident_call("train", optim, *batch)
        dev_batch = self._device_batch(batch)
        e = self._train_engine(optim, dev_batch, 1)
        self._reset_logs(e)  # a caller of the per-batch interface reads per batch: the logs never hold more than this step
        return self._read(e.step(dev_batch))

    def valid_batch(self, batch):
        """src/pretrain/lxmert_pretrain.py:320-326 -> (loss.item(), losses numpy [1, n], ans_logit)"""
        if self._is_store(batch[0]):
            return self._resident_call("valid", None, *batch)
        dev_batch = self._device_batch(batch)
        e = self._valid_engine(dev_batch, 1)
        self._reset_logs(e)
        return self._read(e.valid_step(dev_batch))

    def _resident_step(self, e, kind, store, start, rows):
        """rows ``start .. start + rows`` of the store's current order through engine ``e``: ``load_resident`` + the replayed
        step, or -- a ragged last batch -- the same calls eagerly on buffers of its own size"""
        run = e.step if kind == "train" else e.valid_step
        if rows == e.B:
            e.load_resident(store, start)
            return run()
        if store.match_rate is not None and self.features.match_rate is not None:
            raise ValueError("LXMERT: the store swaps and so does features; build LXMERT(resident=True)")
        return run(self._resident_batch(store, start, rows, like=e))

    def _resident_call(self, kind, optim, store, start, rows=None):
        """``train_batch(optim, (store, start[, rows]))`` / ``valid_batch((store, start[, rows]))``: the batch is rows
        ``start .. start + rows`` (default: the store's batch size) of the order the store currently holds"""
        rows = int(rows if rows is not None else store.batch_size)
        first = lambda: self._resident_batch(store, start, rows)
        e = self.engine if self.engine is not None and (kind == "valid" or optim is self._optim) and self.engine.B == rows else None
        if e is None:
            e = self._train_engine(optim, first(), 1, store) if kind == "train" else self._valid_engine(first(), 1, store)
        self._reset_logs(e)
        return self._read(self._resident_step(e, kind, store, start, rows))

    # ------------------------------------------------------------------ epochs
    def _steps(self, loader, kind, epoch):
        """one sweep as (feed, rows, uids) per step; feed: the device batch of a list loader, or (store, start) of a store"""
        dp = self._dp()
        if not self._is_store(loader):
            if dp is not None:
                raise ValueError("LXMERT: under data parallelism the loader must be a ResidentPretrainSet (its order is "
                                 "sharded over the ranks); a host loader would have to be sharded by the caller")
            for batch in loader:
                yield self._device_batch(batch), len(batch), [datum.uid for datum in batch]
            return
        order, B = self.resident_order(loader, kind, epoch), loader.batch_size
        lo, hi = 0, len(order)
        if dp is not None and kind != "train":
            # validation: a contiguous slice of the sweep per rank, its ragged tail eagerly; no collective in here, so the
            # ranks may take different numbers of steps (none at all included)
            mine = shard_range(len(order), dp[0], dp[1])
            lo, hi = mine.start, mine.stop
        for start in range(lo, hi, B):
            rows = min(B, hi - start)
            yield (loader, start), rows, loader.uids(order[start:start + rows])

    def _sweep(self, loader, optim, kind, table, iters=-1, epoch=0):
        """one pass over ``loader`` with no per-step read -> (sum of losses, {name: sum of term}, steps, uid2ans); the logs
        are read once at its end, or once per ``log_every`` steps (earlier when the answer log could not take the next batch)"""
        from .. import trainlog as T
        n_batches = self._n_batches(loader, kind)
        window = max(1, min(self.log_every or n_batches, n_batches))
        total, terms, steps, uids, uid2ans = 0.0, {}, 0, [], {}
        e = None
        dp = self._dp()
        self._deferred = None  # data-parallel validation: an overflow of THIS rank, raised on every rank after the sweep

        def read_back():
            nonlocal total, steps, uids
            log = e.train_log if kind == "train" else e.valid_log
            if dp is not None and kind == "train":
                # every rank is here after the same number of steps: the overflow flag is agreed on (all raise or none),
                # then the ranks' logs are folded into their mean -- one collective each per read-back, none per step
                e.check()
                rec = log.fold(pending, dp[2])
            elif dp is not None:
                try:
                    e.check(collective=False)
                except RuntimeError as err:
                    self._deferred = self._deferred or err
                rec = log.read()
            else:
                e.check()
                rec = log.read()
            mean, named, n = T.pretrain_means(rec)
            total, steps = total + mean * n, steps + n
            for name, v in named:
                terms[name] = terms.get(name, 0.0) + v * n
            if e.answer_log is not None:
                labels, _, _, m = e.answer_log.read()
                assert m == len(uids), (m, len(uids))
                id2ans = table.id2ans
                for uid, l in zip(uids, labels.tolist()):
                    uid2ans[uid] = id2ans(l) if callable(id2ans) else id2ans[l]
            uids = []
            self._reset_logs(e)

        pending = 0
        store = loader if self._is_store(loader) else None
        for i, (feed, rows, step_uids) in enumerate(self._steps(loader, kind, epoch)):
            if e is None:
                # a store's engine is built on a clean gather of the sweep's first rows, with the store's table as its pool
                first = feed if store is None else self._resident_batch(store, feed[1], rows)
                e = (self._train_engine(optim, first, window, store) if kind == "train"
                     else self._valid_engine(first, window, store))
                self._reset_logs(e)
            if pending and e.answer_log is not None and e.answer_log.count + rows > e.answer_log.capacity:
                read_back()
                pending = 0
            if store is not None:
                self._resident_step(e, kind, store, feed[1], rows)
            elif kind == "train":
                e.step(feed)
            else:
                e.valid_step(feed)
            uids.extend(step_uids)
            pending += 1
            if pending == window:
                read_back()
                pending = 0
            if i == iters:
                break
        if pending:
            read_back()
        return total, terms, steps, uid2ans

    def _merge_ranks(self, uid2ans):
        """data parallel, once after a sweep (a COLLECTIVE call): the ranks' ``uid2ans`` merged in rank order with one
        ``all_gather_object``; an overflow a rank met in its validation slice travels with it and is raised on EVERY rank"""
        dp = self._dp()
        err, self._deferred = getattr(self, "_deferred", None), None
        if dp is None:
            if err is not None:
                raise err
            return uid2ans
        import torch.distributed as dist
        parts = [None] * dp[1]
        dist.all_gather_object(parts, (uid2ans, None if err is None else str(err)), group=dp[2])
        merged = {}
        for u, _ in parts:
            merged.update(u)
        for r, (_, msg) in enumerate(parts):
            if msg is not None:
                raise RuntimeError("rank %d: %s" % (r, msg))
        return merged

    @staticmethod
    def _losses_line(terms, denom):
        s = "The losses are "
        for name in LOSSES_NAME:
            if name in terms:
                s += "%s: %0.4f " % (name, terms[name] / denom)
        return s

    def train(self, train_tuple, eval_tuple):
        """src/pretrain/lxmert_pretrain.py:328-379; ``*_tuple`` = (dataset, loader, evaluator) or anything with those
        attributes"""
        from ..lxrt.optimization import BertAdam
        args = self.args
        dataset, train_ld, evaluator = _tuple(train_tuple)
        dp = self._dp()
        print = _printer(dp)  # data parallel: rank 0 alone prints, evaluates and writes
        batch_per_epoch = self._n_batches(train_ld, "train")  # data parallel: GLOBAL steps of world x B samples
        t_total = int(batch_per_epoch * args.epochs)
        warmup_ratio = 0.05
        warmup_iters = int(t_total * warmup_ratio)
        print("Batch per epoch: %d" % batch_per_epoch)
        print("Total Iters: %d" % t_total)
        print("Warm up Iters: %d" % warmup_iters)
        if 'lamb' in str(getattr(args, 'optim', 'bert')):  # --optim bertlamb: layer-wise trust ratios for large global batches
            from ..lxrt.optimization import BertLamb as BertAdam
        optim = BertAdam(list(self.model.parameters()), lr=args.lr, warmup=warmup_ratio, t_total=t_total)
        best_eval_loss = 9595.
        for epoch in range(args.epochs):
            self.model.train()
            total_loss, terms, _, uid2ans = self._sweep(train_ld, optim, "train", dataset.answer_table, epoch=epoch)
            uid2ans = self._merge_ranks(uid2ans)
            print("The training loss for Epoch %d is %0.4f" % (epoch, total_loss / batch_per_epoch))
            print(self._losses_line(terms, batch_per_epoch))
            if self.model.task_qa and (dp is None or dp[0] == 0):
                evaluator.evaluate(uid2ans, pprint=True)
            avg_eval_loss = self.evaluate_epoch(eval_tuple, iters=-1)
            if avg_eval_loss < best_eval_loss:
                best_eval_loss = avg_eval_loss
                self.save("BEST_EVAL_LOSS")
            self.save("Epoch%02d" % (epoch + 1))

    def evaluate_epoch(self, eval_tuple, iters=-1):
        """src/pretrain/lxmert_pretrain.py:381-409 (the answers are decoded with the evaluated data set's own table)"""
        dataset, eval_ld, evaluator = _tuple(eval_tuple)
        was_training = self.model.training
        self.model.eval()
        total_loss, terms, steps, uid2ans = self._sweep(eval_ld, None, "valid", dataset.answer_table, iters)
        self.model.train(was_training)
        n_eval = self._n_batches(eval_ld, "valid")
        dp = self._dp()
        print = _printer(dp)  # data parallel: rank 0 alone prints and evaluates
        if dp is not None:
            # the ranks' sums of per-step means, combined once: fp64, rank order, weighted by steps -- the printed mean is
            # that of the per-step means of the whole sweep, the same bits on every rank
            uid2ans = self._merge_ranks(uid2ans)
            named = list(LOSSES_NAME)
            sums = [total_loss] + [terms.get(n, 0.0) for n in named] + [float(n in terms) for n in named]
            tot, n_eval = combine_sums(sums, steps, dp[2])
            if n_eval == 0:
                raise ValueError("LXMERT.evaluate_epoch: no rank took a validation step")
            total_loss = float(tot[0])
            terms = {n: float(tot[1 + i]) for i, n in enumerate(named) if tot[1 + len(named) + i] > 0}
        print("The valid loss is %0.4f" % (total_loss / n_eval))
        print(self._losses_line(terms, n_eval))
        if self.model.task_qa and (dp is None or dp[0] == 0):
            evaluator.evaluate(uid2ans, pprint=True)
        return total_loss / n_eval

    # ------------------------------------------------------------------ snapshots, the reference's file names
    def save(self, name):
        """data parallel: rank 0 writes (the replicas are equal), on the other ranks a no-op"""
        dp = self._dp()
        if dp is not None and dp[0] != 0:
            return
        os.makedirs(self.args.output, exist_ok=True)
        torch.save(self.model.state_dict(), os.path.join(self.args.output, "%s_LXRT.pth" % name))

    def load(self, path):
        print("Load BERT extractor from %s" % path)
        self.model.load_state_dict(torch.load("%s_LXRT.pth" % path, map_location="cpu", weights_only=True))

    def load_lxmert(self, path):
        """every weight of the snapshot but the answer head (src/pretrain/lxmert_pretrain.py:420-448); a ``module.``
        prefix (a snapshot of a DataParallel model) is dropped, names without it are kept"""
        print("Load LXMERT model from %s" % path)
        sd = torch.load("%s_LXRT.pth" % path, map_location="cpu", weights_only=True)
        sd = {(k[len("module."):] if k.startswith("module.") else k): v for k, v in sd.items() if "answer" not in k}
        load_keys, model_keys = set(sd), set(self.model.state_dict())
        print()
        print("Keys in loaded but not in model:")
        for key in sorted(load_keys.difference(model_keys)):
            print(key)
        print()
        print("Keys in model but not in loaded:")
        for key in sorted(model_keys.difference(load_keys)):
            print(key)
        print()
        self.model.load_state_dict(sd, strict=False)


def _tuple(t):
    """(dataset, loader, evaluator) of a DataTuple-like object or a plain 3-tuple"""
    if hasattr(t, "dataset"):
        return t.dataset, t.loader, t.evaluator
    return t[0], t[1], t[2]
