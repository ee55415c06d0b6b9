"""Graph-captured training iteration.

Eager execution of one pass issues ~700 kernel launches through Python; at 32 samples per GPU
each kernel runs for microseconds, so the host would be the bottleneck.  ``CapturedTrainer``
records each pass ONCE into a hipGraph (torch.cuda.CUDAGraph: every kernel here is launched on
torch's current stream, so stream capture sees them all, forward, backward, clip and BertAdam
alike) and replays it per step -- "HIP graphs instead of a tracing compiler".  Everything a
replay needs to differ from the previous one lives in device memory: the batch (static input
buffers), the Philox offset, the per-group step counters and schedule values.

With data parallelism each pass is captured as two graphs (forward+backward | clip+update)
and the gradient all-reduce runs between them on the live RCCL communicator; with the overlap
option (default) the backward is cut below the cross-modality layers into a third graph, and the
gradients above the cut are already on the wire while the lower backward graph replays.
With the sharded update (ZeRO-1) on top of the overlap the FORWARD is cut at the same places: the
all-gather of the bf16 weights that follows the update is queued stage by stage in forward order
on the communication stream, forward graph i waits only for batch i, and the gather of stage
i + 1 runs under the forward of stage i (dist.ShardedUpdate.gather_begin).
"""
import gc

import torch

from . import ops

from .runtime import runtime_of
from .vqa.vqacpv2 import (forward_backward_plain, forward_backward_ggm, clip_and_step, _sync_grads,
                          BCEWithLogitsLoss, log_pass)


class _quiet_gc:
    """no garbage collection while a stream is being captured: a finalizer that runs in the middle of a capture
    (on whatever thread allocates next, the autograd thread included) may free pinned host memory or destroy
    events -- the caching host allocator then queries an event, which HIP refuses during a global-mode capture,
    and the process aborts.  Collect first, then keep the collector off until the capture has ended."""

    def __enter__(self):
        gc.collect()
        self.was = gc.isenabled()
        gc.disable()

    def __exit__(self, *a):
        if self.was:
            gc.enable()


class AnswerLog:
    """Device-resident log of chosen answers (``ops.answer_pick`` / xggm_answer_pick_f32): every call appends the
    arg-max of its batch -- with a target also the soft scores and their running fp64 sum -- and the host reads the
    log ONCE per sweep or epoch instead of once per batch (the reference: ``logit.max(1)[1].cpu()``,
    src/vqa/vqacpv2.py:180-181 and :333-334).

        log = AnswerLog(len(dset), dev, with_scores=False)
        pred = CapturedPredictor(model, 512, log=log)
        log.reset()
        for ques_id, feats, boxes, sent in loader: pred.push(feats, boxes, sent)   # no host synchronisation
        labels, _, _, n = log.read()                                              # the one read-back

    Everything lives in one int64 device buffer -- [cursor, score sum (fp64), flags, labels, scores] -- so that
    ``read`` is one transfer into one pinned host buffer.  An append that does not fit stores nothing and raises the
    overflow flag; ``read`` then raises.  Calls that share a log must be ordered against each other (one stream)."""

    def __init__(self, capacity, device, with_scores=True):
        capacity = int(capacity)
        if capacity <= 0:
            raise ValueError("AnswerLog: capacity must be positive")
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("xggm_amd: the answer log must live on the GPU (no CPU fallback)")
        self.capacity, self.with_scores = capacity, bool(with_scores)
        words = 3 + capacity + ((capacity + 1) // 2 if with_scores else 0)
        self.buf = torch.zeros(words, dtype=torch.int64, device=device)
        self.host = torch.zeros(words, dtype=torch.int64).pin_memory()
        self.cursor = self.buf[0:1]
        self.score_sum = self.buf[1:2].view(torch.float64) if with_scores else None
        self.flags = self.buf[2:3].view(torch.int32)[0:1]
        self.labels = self.buf[3:3 + capacity]
        self.scores = self.buf[3 + capacity:].view(torch.float32)[:capacity] if with_scores else None
        # the kept rows of a padded short batch: a device word the captured launch reads, fed from ONE pinned slot
        self.rows = torch.zeros(1, dtype=torch.int32, device=device)
        self._rows_host = torch.zeros(1, dtype=torch.int32).pin_memory()
        self._rows_sent = None   # value the device word holds (after the copies queued so far)
        self._rows_copied = None  # event behind the last copy out of the pinned slot
        self.count = 0  # host mirror of the cursor: samples handed to the log since reset()
        self._score = None  # buffers of ``score_store``, made on its first call

    def set_rows(self, n):
        """queue ``rows = n`` in stream order (nothing is queued while the value does not change: full batches).  The
        pinned slot is rewritten only once the previous copy out of it has run -- it was queued batches ago; should it
        still be pending, the new value goes through a fresh slot instead of waiting"""
        n = int(n)
        if n == self._rows_sent:
            return
        if self._rows_copied is not None and not self._rows_copied.query():
            self._rows_host = torch.zeros(1, dtype=torch.int32).pin_memory()
        self._rows_host[0] = n
        self.rows.copy_(self._rows_host, non_blocking=True)
        self._rows_copied = torch.cuda.Event()
        self._rows_copied.record()
        self._rows_sent = n

    def note(self, n):
        """host bookkeeping of an append of ``n`` samples that has been queued (a graph replay runs no Python): an
        append past the capacity is refused here already, before anything is queued"""
        if self.count + n > self.capacity:
            raise RuntimeError("answer log overflow: capacity %d, %d samples logged, %d more do not fit"
                               % (self.capacity, self.count, n))
        self.count += n

    def reset(self):
        """cursor, score sum and flags back to zero, in stream order (no synchronisation)"""
        self.buf[:3].zero_()
        self.count = 0

    def read(self):
        """-> (labels [n] int64, scores [n] fp32 or None, score_sum float, n) as CPU tensors / numbers: ONE
        device-to-host transfer and one wait for it.  RuntimeError when an append was refused."""
        from .answers import decode_packed
        self.host.copy_(self.buf, non_blocking=True)
        torch.cuda.current_stream(self.buf.device).synchronize()
        return decode_packed(self.host, self.capacity, self.with_scores)

    def fold(self, layout, expect, block=None, group=None):
        """COLLECTIVE merge under data parallelism (every rank of ``group`` calls it with the same arguments): the ranks'
        packed logs -- the same capacity on every rank -- are all-gathered, ONE collective per sweep or epoch and never per
        step, and one launch (``ops.answer_log_fold``) merges them in sweep order into a log of capacity >= ``sum(expect)``
        that is made once and reused.  ``expect[r]``: the answers rank r must hold; ``layout``: ``ops.FOLD_CONCAT`` (a sweep cut
        into contiguous slices, counts may differ or be 0) or ``ops.FOLD_INTERLEAVE`` (a training epoch: global step s holds
        the ranks' ``block`` answers in rank order).  -> the merged ``AnswerLog`` with ``count = sum(expect)``: ``read`` and
        ``score_store`` work on it as on any log, and give the same bits on every rank.  RuntimeError on every rank (the
        flag is computed from the same gathered words) when a rank's cursor is not its ``expect[r]`` or its log refused an
        append.  A one-rank group: ``self``, without a launch."""
        import torch.distributed as dist
        from .answers import fold_flag_message
        world = dist.get_world_size(group) if dist.is_initialized() else 1
        if world == 1:
            return self
        expect = [int(e) for e in expect]
        total = sum(expect)
        if len(expect) != world or total < 1 or any(not 0 <= e <= self.capacity for e in expect):
            raise ValueError("AnswerLog.fold: expect = %s for %d ranks of capacity %d" % (expect, world, self.capacity))
        dev, W = self.buf.device, self.buf.numel()
        if getattr(self, "_gathered", None) is None or self._gathered.shape[0] != world:
            self._gathered = torch.zeros((world, W), dtype=torch.int64, device=dev)
            self._flag = torch.zeros(1, dtype=torch.int64, device=dev)
            self._flag_host = torch.zeros(1, dtype=torch.int64).pin_memory()
        if getattr(self, "_merged", None) is None or self._merged.capacity < total:
            self._merged = AnswerLog(total, dev, with_scores=self.with_scores)  # a sweep's total does not change
        if dist.get_backend(group) == "nccl":
            dist.all_gather_into_tensor(self._gathered, self.buf, group=group)
        else:  # gloo, the test transport: through the host
            self.host.copy_(self.buf, non_blocking=True)
            torch.cuda.current_stream(dev).synchronize()
            parts = [torch.empty(W, dtype=torch.int64) for _ in range(world)]
            dist.all_gather(parts, self.host.clone(), group=group)
            self._gathered.copy_(torch.stack(parts))
        out = self._merged
        ops.answer_log_fold(self._gathered, out, self._flag, self.capacity, self.with_scores, layout, expect,
                            block=1 if block is None else block)
        out.count = total
        self._flag_host.copy_(self._flag, non_blocking=True)
        torch.cuda.current_stream(dev).synchronize()
        flag = int(self._flag_host[0])
        if flag:
            raise RuntimeError(fold_flag_message(flag) + " (expected per rank: %s)" % expect)
        return out

    def score(self):
        """mean soft score of the logged samples (the reference's per-epoch train score, src/vqa/vqacpv2.py:285, as a
        fraction; the evaluator's sum, src/vqa/vqacpv2_data.py:134-142, over the count)"""
        if not self.with_scores:
            raise RuntimeError("AnswerLog.score: the log was built without scores")
        _, _, total, n = self.read()
        return total / n if n else 0.0

    def score_store(self, store, order=None, keep=None, by_group=False):
        """what ``evaluator.evaluate`` makes of the log's first ``count`` answers, computed where they lie: ONE launch
        (``ops.answer_score``) scores them against the ground truth of ``store`` (a ``tools.resident.ResidentDataset``: its
        q_label / q_score tables) and ONE read-back of a few words follows -- no labels cross the host link, no dict is built.
        ``order``: the sample of every logged answer, a device int64 tensor or a host array of at least ``count`` entries
        (None: answer i belongs to sample i, a sweep in data set order); ``keep``: 0 / 1 per answer, device uint8 tensor or
        host array (None: all count) -- ``answers.last_occurrence_mask`` of the question ids gives the reference's dict
        semantics, where a question that occurs twice counts once.  ``by_group``: also per group of the store (``ResidentDataset(groups=)``).
        -> the dict of ``answers.decode_score``; RuntimeError when the cursor is not ``count`` or an index was out of range."""
        from .answers import decode_score
        n, dev = self.count, self.buf.device
        if n < 1:
            raise RuntimeError("AnswerLog.score_store: the log is empty")
        G = 0
        if by_group:
            if "q_group" not in store.tables:
                raise ValueError("AnswerLog.score_store: the store was built without groups")
            G = store.G
        if self._score is None:  # out words, their pinned mirror and the workspace: sized once, for every later call
            self._score = (torch.zeros(3 + 2 * ops.SCORE_MAX_GROUPS, dtype=torch.int64, device=dev),
                           torch.zeros(3 + 2 * ops.SCORE_MAX_GROUPS, dtype=torch.int64).pin_memory(),
                           ops.answer_score_workspace(self.capacity, ops.SCORE_MAX_GROUPS, dev))
        out, host, ws = self._score
        order = order if order is None or torch.is_tensor(order) else torch.as_tensor(order, dtype=torch.int64).to(dev)
        keep = keep if keep is None or torch.is_tensor(keep) else torch.as_tensor(keep, dtype=torch.uint8).to(dev)
        W = 3 + 2 * G
        ops.answer_score(self.labels, store.tables["q_label"], store.tables["q_score"], n, order=order, keep=keep,
                         q_group=store.tables["q_group"] if G else None, G=G, cursor=self.cursor, out=out, ws=ws)
        host[:W].copy_(out[:W], non_blocking=True)
        torch.cuda.current_stream(dev).synchronize()
        return decode_score(host[:W], G, store.group_names if G else None)


class TrainLog:
    """Device-resident log of the scalars of every optimiser pass (``ops.train_log_append`` / xggm_train_log_append):
    the loss and its terms, the pre-clip gradient norm and the schedule value are appended to a ring of ``capacity``
    records, with running fp64 sums per pass kind and the index of the first record that holds an inf or a NaN.  The
    host reads it ONCE per N iterations or per epoch instead of calling ``float()`` on a device scalar in every pass
    (the reference: ``total_loss += loss.detach() / logit.size(0)``, src/vqa/vqacpv2.py:179, and the tensorboard scalars
    Train/batch_loss, Train/average_loss and lr, :256-270).

        log = TrainLog(2 * iters_per_epoch, dev)
        trainer = CapturedTrainer(model, optim, batch, train_log=log)
        for ...: trainer.iteration(branch)                       # no host synchronisation
        rec = log.read()                                         # the one read-back
        rec["values"][rec["kinds"] == TrainLog.PLAIN, TrainLog.LOSS] / batch_size   # Train/batch_loss of every iteration
        log.average_loss(batch_size, rec)                        # Train/average_loss, from the same read-back

    Everything lives in one int64 device buffer (layout: ``trainlog.words``), so that ``read`` is one transfer into one
    pinned host buffer.  The ring keeps the last ``capacity`` records; the sums, the counts and ``first_bad`` cover every
    record since ``reset()``.  Calls that share a log must be ordered against each other (one stream)."""

    LOSS, BCE, KL, DSM, GRAD_NORM, LR_SCALE = range(6)  # columns (trainlog.py); 6 and 7 are spare
    PLAIN, REL, NODE = 0, 1, 2                          # kinds

    def __init__(self, capacity, device):
        from . import trainlog
        capacity = int(capacity)
        if capacity <= 0:
            raise ValueError("TrainLog: capacity must be positive")
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("xggm_amd: the training log must live on the GPU (no CPU fallback)")
        self.capacity = capacity
        C, K, H = trainlog.COLS, trainlog.KINDS, trainlog.HEADER
        n = trainlog.words(capacity)
        self.buf = torch.zeros(n, dtype=torch.int64, device=device)
        self.host = torch.zeros(n, dtype=torch.int64).pin_memory()
        self.cursor = self.buf[0:1]
        self.first_bad_word = self.buf[1:2]
        self.counts = self.buf[2:2 + K]
        self.sums = self.buf[2 + K:H].view(torch.float64).view(K, C)
        self.steps = self.buf[H:H + capacity]
        o = H + capacity
        self.values = self.buf[o:o + capacity * C // 2].view(torch.float32).view(capacity, C)
        self.kinds = self.buf[o + capacity * C // 2:].view(torch.int32)[:capacity]
        self.reset()

    def reset(self):
        """an empty log (ring, sums, counts and cursor zero, ``first_bad`` -1), in stream order: no synchronisation"""
        self.buf.zero_()
        self.first_bad_word.fill_(-1)

    def read(self):
        """-> dict of CPU tensors: values [m, COLS] fp32, steps [m] int64, kinds [m] int64, present [m, COLS] bool,
        cursor, sums [KINDS, COLS] fp64, counts [KINDS] int64, first_bad -- the records are the last m = min(cursor,
        capacity), oldest first.  ONE device-to-host transfer and one wait for it."""
        from .trainlog import decode_packed
        self.host.copy_(self.buf, non_blocking=True)
        torch.cuda.current_stream(self.buf.device).synchronize()
        return decode_packed(self.host, self.capacity)

    def fold(self, n, group=None):
        """COLLECTIVE read-back under data parallelism (every rank of ``group`` calls it with the same ``n``): the ranks'
        rings are all-gathered -- ONE collective per read-back, never per step --, one launch (``ops.train_log_fold``) replaces
        this rank's ``n`` records, all of them since ``reset()``, by their mean over the ranks (the reference's
        ``loss.mean()`` / ``losses.mean(0)`` over its replicas, src/pretrain/lxmert_pretrain.py:311-313), and the log is
        read as ``read()`` reads it: the same bits on every rank.  RuntimeError (on every rank: the flag is computed from
        the same gathered words) when the ranks disagree on the kind, the present columns or the step of a record or have
        not logged ``n`` records each -- replicas that have come apart.  A one-rank group: ``read()``."""
        import torch.distributed as dist
        from . import trainlog as T
        world = dist.get_world_size(group) if dist.is_initialized() else 1
        n = int(n)
        if world == 1:
            return self.read()
        if not 1 <= n <= self.capacity:
            raise ValueError("TrainLog.fold: %d records, the log holds 1 .. %d" % (n, self.capacity))
        dev, W = self.buf.device, self.buf.numel()
        if getattr(self, "_gathered", None) is None or self._gathered.shape[0] != world:
            self._gathered = torch.zeros((world, W), dtype=torch.int64, device=dev)
            self._flag = torch.zeros(1, dtype=torch.int64, device=dev)
            self._flag_host = torch.zeros(1, dtype=torch.int64).pin_memory()
        if dist.get_backend(group) == "nccl":
            dist.all_gather_into_tensor(self._gathered, self.buf, group=group)
        else:  # gloo, the test transport: through the host
            self.host.copy_(self.buf, non_blocking=True)
            torch.cuda.current_stream(dev).synchronize()
            parts = [torch.empty(W, dtype=torch.int64) for _ in range(world)]
            dist.all_gather(parts, self.host.clone(), group=group)
            self._gathered.copy_(torch.stack(parts))
        flat, C, cap = self._gathered.view(-1), T.COLS, self.capacity
        o = T.HEADER + cap
        ops.train_log_fold(self, flat[o:].view(torch.float32), flat[o + cap * C // 2:].view(torch.int32), world, n, self._flag,
                           steps=flat[T.HEADER:], cursors=flat, strides=(2 * W, 2 * W, W, W))
        self._flag_host.copy_(self._flag, non_blocking=True)
        rec = self.read()  # one wait for both transfers
        flag = int(self._flag_host[0])
        if flag >= 0:
            raise RuntimeError("training log fold: " + ("a rank has not logged %d records" % n if flag == n else
                               "the ranks disagree on record %d (its kind, its present columns or its optimiser step)" % flag)
                               + " -- the data-parallel replicas have come apart")
        return rec

    def average_loss(self, batch_size, rec=None):
        """the reference's Train/average_loss (src/vqa/vqacpv2.py:179, :262): the sum of the plain passes' losses since
        ``reset()``, each divided by the batch size, over their count -- sums[PLAIN][LOSS] / batch_size / counts[PLAIN].
        ``rec``: what ``read()`` returned (no further transfer); None reads the log"""
        rec = self.read() if rec is None else rec
        n = int(rec["counts"][self.PLAIN])
        return float(rec["sums"][self.PLAIN, self.LOSS]) / batch_size / n if n else 0.0

    def first_bad(self, rec=None):
        """-1, or the index (counted from ``reset()``) of the first record with an inf or a NaN in a present column;
        ``rec`` as in ``average_loss``"""
        return int((self.read() if rec is None else rec)["first_bad"])


class CapturedTrainer:
    def __init__(self, model, optim, batch, sigma=1.0, order="vqa", clip=5.0, use_graph=True, warmup_iters=2,
                 packed_spec=None, answer_log=None, train_log=None):
        """``batch``: dict of DEVICE tensors feats, boxes, input_ids, input_mask, segment_ids,
        target, adj_true; they become the static input buffers (``load_batch`` copies into them).
        ``packed_spec`` = ``DataLoaderX.spec`` of a loader with ``handover="inline"``: the static buffers are then
        views of ONE flat device buffer laid out like the loader's pinned slots, and ``load_packed`` hands a batch over
        with a single host-to-device copy on the compute stream.
        ``answer_log`` = an ``AnswerLog`` with scores: the PLAIN pass (whose answers the reference logs,
        src/vqa/vqacpv2.py:180-181) then ends with one ``ops.answer_pick`` on its logits and the static target, inside
        the captured graph; ``train_score()`` / ``answers()`` read it back.  It observes only: nothing of the step
        depends on it.  Under data parallelism each rank logs its own samples -- the caller averages the ranks'
        ``train_score()`` (weighted by their counts); no collective is added.  None (default): no launch is added.
        ``train_log`` = a ``TrainLog``: EVERY pass then ends with one ``ops.train_log_append`` (``vqa.vqacpv2.log_pass``)
        behind its update -- inside the captured graph, under data parallelism inside the update graph's capture -- that
        records the pass's total loss, its un-weighted terms, the pre-clip norm and the schedule value of the update
        (which value: ``log_pass``).  It reads device scalars the pass leaves anyway and observes only.  Each rank logs
        its own values; no collective is added.  None (default): no launch is added."""
        self.model, self.optim = model, optim
        self.answer_log = answer_log
        self.train_log = train_log
        self._pass = None  # (kind, loss, terms) of the running pass, for the record its update appends
        if answer_log is not None and not answer_log.with_scores:
            raise ValueError("CapturedTrainer: answer_log needs scores (AnswerLog(with_scores=True))")
        self.rt = runtime_of(model)
        self.static_flat = None
        # (a loss that reads no bias -- Plain, CrossEntropy -- needs nothing beyond the loader's fields)
        if packed_spec is not None and getattr(getattr(model, "debias_loss", None), "needs_bias", False):
            raise ValueError("CapturedTrainer: packed_spec carries no bias for the attached debias loss; hand batches over "
                             "with load_batch")
        if packed_spec is not None:
            from .tools.data_loader import packed_like
            dev = next(model.parameters()).device
            self.static_flat, v = packed_like(packed_spec, dev)
            self.static = dict(feats=v["feats"], boxes=v["boxes"], input_ids=v["ids"][0], input_mask=v["ids"][1],
                               segment_ids=v["ids"][2], target=v["target"], adj_true=v["adj"])
            for k, t in self.static.items():
                if tuple(t.shape) != tuple(batch[k].shape) or t.dtype != batch[k].dtype:
                    raise ValueError("packed_spec field %s is %s %s, the batch has %s %s"
                                     % (k, tuple(t.shape), t.dtype, tuple(batch[k].shape), batch[k].dtype))
                t.copy_(batch[k])
        else:
            self.static = {k: v.clone() for k, v in batch.items() if torch.is_tensor(v)}
        self.sigma, self.clip = sigma, clip
        self.kl_weight = 8.0 if order == "vqa" else 12.0
        self.order = order
        self.bce = BCEWithLogitsLoss()
        self.use_graph = use_graph
        self.graphs = {}
        self.outputs = {}
        self.split = getattr(model, "_grad_sync", None) is not None
        self._comm = None
        # With a process group alive its watchdog thread polls events at any time; under the default "global"
        # capture mode HIP rejects that ("operation not permitted when stream is capturing") and the process
        # aborts.  "thread_local" only polices the capturing thread.
        self.capture_mode = "thread_local" if self.split else "global"
        model.train()
        if use_graph:
            self._capture(warmup_iters)
        if answer_log is not None:
            answer_log.reset()  # what the warm-up passes logged
        if train_log is not None:
            train_log.reset()  # the records of the warm-up and capture passes

    # ------------------------------------------------------------------ the two halves of a pass
    def _fwd_bwd(self, kind, between=None):
        s = self.static
        sent = (s["input_ids"], s["input_mask"], s["segment_ids"])
        # an attached debias loss (vqa.vqacpv2.attach_debias_loss) reads its bias from the static batch like everything else
        kw = dict(bias=s.get("bias"), bias_index=s.get("bias_index")) if getattr(self.model, "debias_loss", None) is not None else {}
        if kind == "plain":
            loss, logit = forward_backward_plain(self.model, self.bce, s["feats"], s["boxes"], sent, s["target"],
                                                 between=between, **kw)
            if self.answer_log is not None:
                # reads the logits and the target only: behind the backward it costs one short launch at the tail of the
                # (last backward) graph and nothing waits for it
                ops.answer_pick(logit, self.answer_log, target=s["target"])
            terms = None
        else:
            loss, logit, terms = forward_backward_ggm(self.model, self.bce, s["feats"], s["boxes"], sent, s["target"],
                                                      s["adj_true"], kind, self.sigma, self.kl_weight, between=between, **kw)
        if self.train_log is not None:
            self._pass = (kind, loss, terms)  # the loss-kernel slots stay alive until the update has appended them
        return loss, logit

    def _update(self):
        total = clip_and_step(self.model, self.optim, self.clip, advance=True)
        self._log_pass(total)
        return total

    def _log_pass(self, total):
        """the training log's record of the running pass, issued (or captured) behind its update"""
        if self.train_log is not None:
            kind, loss, terms = self._pass
            self._pass = None
            log_pass(self.train_log, self.model, self.optim, kind, loss, total, terms)

    # the update as graphs: one, or -- sharded update -- two with the norm's scalar all-reduce between them and the
    # all-gather of the weights behind them (collectives run on the live communicator, never inside a capture)
    def _capture_update(self, pool):
        z = self.rt.arena.zero1
        if z is None:
            gu = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gu, pool=pool, capture_error_mode=self.capture_mode):
                total = self._update()
            return (gu,), total
        from .lxrt.optimization import clip_norm_local, clip_norm_finish
        arena = self.rt.arena
        g1, g2 = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
        with torch.cuda.graph(g1, pool=pool, capture_error_mode=self.capture_mode):
            clip_norm_local(arena)
        z.exchange_norm(arena.sqnorm)
        with torch.cuda.graph(g2, pool=pool, capture_error_mode=self.capture_mode):
            total = clip_norm_finish(arena, self.clip, tail=(self.optim, None))  # (the schedule step rides on the finish)
            self.optim.step()
            self._log_pass(total)
        z.gather()
        self.optim.zero_grad()
        # Runtime.advance (new dropout masks for the next pass) is NOT run here: a capture executes nothing, and the
        # replay issues it eagerly behind the gather (_replay_update) -- exactly once per trained pass
        return (g1, g2), total

    def _replay_update(self, gus, staged_gather=False):
        if len(gus) == 1:
            gus[0].replay()
            return
        z = self.rt.arena.zero1
        gus[0].replay()
        z.exchange_norm(self.rt.arena.sqnorm)
        gus[1].replay()
        if staged_gather:
            # the bf16 weights come back stage by stage beside the NEXT pass's forward graphs (run_pass waits per stage)
            z.gather_begin(self._comm_stream())
        else:
            z.gather()
        self.rt.advance()

    def _comm_stream(self):
        if self._comm is None:
            self._comm = torch.cuda.Stream()
        return self._comm

    def _stage_ranges(self):
        from .dist import active_ranges, stage_ranges
        return stage_ranges(self.rt.arena, active_ranges(self.rt.arena), self.rt.cut_layout, self.rt.n_stages)

    def _eager_pass(self, kind):
        if self.split and self.rt.cut_enabled:
            gs, handles = self.model._grad_sync, []

            def between(k):  # gradients above cut k are final: put them on the wire
                handles.append(gs.begin(self._stage_ranges()[k], slot=k))

            loss, logit = self._fwd_bwd(kind, between)
            gs.sync(self._stage_ranges()[-1])
            for h in handles:
                gs.finish(h)
        else:
            loss, logit = self._fwd_bwd(kind)
            _sync_grads(self.model)
        total = self._update()
        return loss, logit, total

    # ------------------------------------------------------------------ capture
    def _capture(self, warmup_iters):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(warmup_iters):
                for kind in ("plain", "rel", "node"):
                    self._eager_pass(kind)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        if self.split:
            # nothing of the eager warm-up exchanges may still be in flight (or polled) while graphs are captured
            import torch.distributed as dist
            dist.barrier()
            torch.cuda.synchronize()
        with _quiet_gc():
            self._capture_kinds()
        torch.cuda.synchronize()

    def _capture_kinds(self):
        for kind in ("plain", "rel", "node"):
            # one memory pool per pass kind (shared by the graphs of that kind only): with a pool shared across kinds
            # the outputs of one kind (loss, logits, norm) can land where an earlier-captured kind keeps its
            # intermediates, and replaying that kind then overwrites them before the caller has read them
            pool = None
            if not self.split:
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, pool=pool, capture_error_mode=self.capture_mode):
                    out = self._eager_pass(kind)
                pool = g.pool()
                self.graphs[kind] = (g,)
                self.outputs[kind] = out
            elif not self.rt.cut_enabled:
                g1 = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g1, pool=pool, capture_error_mode=self.capture_mode):
                    loss, logit = self._fwd_bwd(kind)
                pool = g1.pool()
                ranges = None
                from .dist import active_ranges
                ranges = active_ranges(self.rt.arena)
                if self.rt.arena.zero1 is not None:
                    # the sharded update records its runs at the exchange: run the one of this pass kind (on whatever the
                    # buffers hold -- the captured kernels have not run; every rank does the same)
                    self.rt.arena.zero1.reset()
                    self.model._grad_sync.sync(ranges)
                gus, total = self._capture_update(pool)
                self.graphs[kind] = (g1, gus, ranges)
                self.outputs[kind] = (loss, logit, total)
            else:
                # one graph per backward stage: forward + stage 0 | stage 1 | ... | clip + update.  The capture is
                # switched from one graph to the next inside Runtime.backward (the ``between`` callback).
                graphs, early = [torch.cuda.CUDAGraph()], []
                n_fwd = [0]  # forward cuts passed = forward graphs in front of the one that also holds backward stage 0

                def switch(k):
                    graphs[-1].capture_end()
                    early.append(self._stage_ranges()[k])
                    graphs.append(torch.cuda.CUDAGraph())
                    graphs[-1].capture_begin(pool=graphs[0].pool(), capture_error_mode=self.capture_mode)

                def fwd_switch(i):  # sharded update: one graph per forward stage (see the module docstring)
                    graphs[-1].capture_end()
                    graphs.append(torch.cuda.CUDAGraph())
                    graphs[-1].capture_begin(pool=graphs[0].pool(), capture_error_mode=self.capture_mode)
                    n_fwd[0] += 1

                torch.cuda.synchronize()
                gc.collect()
                torch.cuda.empty_cache()
                cap = torch.cuda.Stream()
                cap.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(cap):
                    if pool is None:
                        graphs[0].capture_begin(capture_error_mode=self.capture_mode)
                    else:
                        graphs[0].capture_begin(pool=pool, capture_error_mode=self.capture_mode)
                    self.rt.fwd_hook = fwd_switch if self.rt.arena.zero1 is not None else None
                    try:
                        loss, logit = self._fwd_bwd(kind, switch)
                    finally:
                        self.rt.fwd_hook = None
                    graphs[-1].capture_end()
                torch.cuda.current_stream().wait_stream(cap)
                pool = graphs[0].pool()
                final = self._stage_ranges()[-1] if early else None
                if final is None:
                    from .dist import active_ranges
                    final = active_ranges(self.rt.arena)
                if self.rt.arena.zero1 is not None:
                    # the runs of this pass kind, recorded as the real exchange would record them
                    self.rt.arena.zero1.reset()
                    for rs in early + [final]:
                        self.model._grad_sync.sync(rs)
                gus, total = self._capture_update(pool)
                self.graphs[kind] = ("staged", graphs, early, final, gus, n_fwd[0])
                self.outputs[kind] = (loss, logit, total)
        torch.cuda.synchronize()

    # ------------------------------------------------------------------ run
    def load_batch(self, batch):
        for k, v in batch.items():
            if k in self.static:
                self.static[k].copy_(v, non_blocking=True)

    def load_packed(self, it):
        """hand over the batch the loader iterator ``it`` (DataLoaderX(handover="inline")) has just yielded: ONE copy of
        the slot's pinned flat buffer into the static inputs, in stream order on the compute stream (it runs between
        the previous iteration's graphs and the next one's: no second stream, no event the graphs wait for, no
        device-to-device copies), then the slot is marked so that the producer does not rewrite it under the copy"""
        if self.static_flat is None:
            raise RuntimeError("load_packed needs CapturedTrainer(packed_spec=loader.spec)")
        if it.flat is None or it.flat.numel() != self.static_flat.numel():
            raise ValueError("the iterator's slot does not have this trainer's layout (handover='inline', same batch size)")
        rows = getattr(it, "rows", None)
        if rows is not None and rows != self.static["feats"].shape[0]:
            # a short (last) batch fills only the head of the slot: the captured step would train on its rows PLUS the
            # stale tail of an older batch (the ring path fails on the shape in copy_; this one has to say so itself)
            raise ValueError("load_packed: the batch holds %d samples, the captured step %d -- iterate the loader with "
                             "drop_last=True (or run the short batch through an eager pass)" % (rows, self.static["feats"].shape[0]))
        self.static_flat.copy_(it.flat, non_blocking=True)
        it.mark_copied()

    def load_resident(self, store, start):
        """hand over rows ``start .. start + B`` of the epoch order of ``store`` (tools.resident.ResidentDataset): ONE
        gather launch out of the device-resident tables into the static inputs, eagerly and in stream order between the
        replays, where ``load_packed`` queues its copy -- nothing crosses PCIe and no graph is captured again.  An attached
        debias loss that selects its prior by ``bias_index`` is fed from the store's; one that reads the dense ``bias`` of a
        batch cannot be (the store holds no [B, A] bias): hand such batches over with ``load_batch``."""
        s = self.static
        if getattr(getattr(self.model, "debias_loss", None), "needs_bias", False):
            if "bias_index" not in s:
                raise ValueError("CapturedTrainer: a resident store carries no dense bias for the attached debias loss; "
                                 "build the trainer on a batch with bias_index (loss.set_bias_table) or use load_batch")
            if "q_bias_index" not in store.tables:
                raise ValueError("CapturedTrainer: the attached debias loss reads bias_index, the store was built without one")
        skip = ("sample",) if "q_bias_index" in store.tables else ("sample", "bias_index")
        store.fill({k: v for k, v in s.items() if k not in skip}, start, s["feats"].shape[0])

    def train_score(self):
        """mean soft score of the plain pass's answers since the log's last ``reset()`` (the reference's per-epoch train
        score, src/vqa/vqacpv2.py:285, as a fraction): one read-back"""
        return self._log().score()

    def answers(self):
        """-> (labels [n] int64, scores [n] fp32) of the plain passes since the log's last ``reset()``, CPU tensors"""
        labels, scores, _, _ = self._log().read()
        return labels, scores

    def _log(self):
        if self.answer_log is None:
            raise RuntimeError("CapturedTrainer was built without answer_log")
        return self.answer_log

    def run_pass(self, kind):
        if kind == "plain" and self.answer_log is not None:
            self.answer_log.note(self.static["target"].shape[0])
        if not self.use_graph:
            return self._eager_pass(kind)
        gs = self.graphs[kind]
        arena = self.rt.arena
        # host-side bookkeeping a replay relies on but never runs (the Python of a pass executes at CAPTURE time only):
        # the sparse exchange of the word table gathers the rows of THIS trainer's ids, looked up once per pass -- an eval
        # forward or a second trainer's capture in between would otherwise leave another batch's ids or a count != 1 behind
        self.rt.emb_ids = self.static["input_ids"]
        arena.emb_uses = 1
        rl = arena.row_list
        if rl is not None and not rl.clean and arena.row_list_enabled:
            # an eager pass in between left rows of the word table's gradient the device-side list does not name (two
            # look-ups, accumulation): the captured clear only knows the list -- clear the whole table once
            ops.zero_ranges(arena.grads, [(rl.o, rl.o + rl.R * rl.H)])
            rl.clean = True
        if arena.zero1 is not None:
            arena.zero1.reset()  # the runs of this pass are recorded again by its exchanges
        if len(gs) == 1:
            gs[0].replay()
        elif gs[0] != "staged":
            gs[0].replay()
            self.model._grad_sync.sync(gs[2])
            self._replay_update(gs[1])
        else:
            # the exchange of stage k (cast to the wire type, all-reduce, copy back) is queued on a side stream
            # right behind graph k and runs under graph k + 1; the update waits for all of it
            _, graphs, early, final, gus, n_fwd = gs
            sync = self.model._grad_sync
            main = torch.cuda.current_stream()
            comm = self._comm_stream()
            z = self.rt.arena.zero1
            # all-gathers of the previous pass's update that are still running: pend[i] covers what forward graph i reads
            pend = z.take_pending() if z is not None else []

            def exchange(k, after):
                comm.wait_event(after)
                with torch.cuda.stream(comm):
                    if k < len(early):
                        sync.finish(sync.begin(early[k], slot=k))
                    else:
                        sync.sync(final)

            # graph k + 1 is handed to the GPU BEFORE the host enqueues the (eager) exchange of stage k: those dozens
            # of small launches take the host longer than the GPU needs to get to the end of graph k
            prev = None
            for i, g in enumerate(graphs):
                if i < len(pend):
                    main.wait_event(pend[i])
                if i == n_fwd:  # the last forward graph (it also holds backward stage 0): nothing may be left running
                    for ev in pend[i + 1:]:
                        main.wait_event(ev)
                g.replay()
                k = i - n_fwd  # backward stage this graph ends with (negative: a forward-only graph)
                if k < 0:
                    continue
                ev = torch.cuda.Event()
                ev.record(main)
                if prev is not None:
                    exchange(k - 1, prev)
                prev = ev
            exchange(len(graphs) - 1 - n_fwd, prev)
            main.wait_stream(comm)
            self._replay_update(gus, staged_gather=z is not None and n_fwd > 0)
        return self.outputs[kind]

    def iteration(self, branch):
        """one training iteration: VQA order = plain then GGM; GQA order = GGM then plain."""
        if self.order == "vqa":
            a = self.run_pass("plain")
            b = self.run_pass(branch)
        else:
            b = self.run_pass(branch)
            a = self.run_pass("plain")
        guard = getattr(self.model, "_replica_guard", None)
        if guard is not None:
            # eager work between two replays, never part of a graph (the check is a collective); what the staged
            # exchange left on the communication stream is waited for first
            if self._comm is not None and all(self._comm is not s for s in guard.wait_streams):
                guard.wait_streams.append(self._comm)
            guard.tick()
        return a, b


class CapturedPredictor:
    """The validation sweep of the reference (``VQA.predict``, src/vqa/vqacpv2.py:315-339; GQA twin
    src/gqa/gqa_ood.py:379-403): eval mode, no autograd, encoder -> ``logit_fc`` -> arg-max; the generator is
    not on this path.  The forward of one full batch is captured once and replayed; a short last batch is
    padded (its padding rows are computed and dropped: samples are independent, so the kept rows do not change).
    The logits are fp32 and the arg-max is torch's (first maximal index), as in ``logit.max(1)``.
    ``log`` = an ``AnswerLog``: the forward then ends in ``ops.answer_pick`` instead (same indices), which appends the
    kept rows' answers to the log on the device; ``push`` queues a batch without handing anything back, and the sweep
    reads the log once at its end (``vqa.vqacpv2.predict`` does so when the predictor carries a log)."""

    def __init__(self, model, batch_size, n_objects=36, feat_dim=None, max_seq_length=None, use_graph=True, log=None):
        self.model = model
        self.log = log
        dev = next(model.parameters()).device
        enc = model.lxrt_encoder
        T = max_seq_length or enc.max_seq_length
        F = feat_dim or enc.model.bert.encoder.visn_fc.visn_fc.in_features
        self.B = batch_size
        self.static = dict(feats=torch.zeros(batch_size, n_objects, F, device=dev),
                           boxes=torch.zeros(batch_size, n_objects, 4, device=dev),
                           ids=torch.zeros(3, batch_size, T, dtype=torch.long, device=dev))
        self.static["ids"][1, :, 0] = 1  # a valid mask for the rows nobody has filled yet
        self.graph, self.logit, self.label = None, None, None
        self.use_graph = use_graph
        if use_graph:
            was_training = model.training
            model.eval()
            if log is not None:
                log.set_rows(batch_size)
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                self._forward()
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            self.graph = torch.cuda.CUDAGraph()
            with _quiet_gc(), torch.cuda.graph(self.graph):
                self.logit, self.label = self._forward()
            model.train(was_training)
            if log is not None:
                log.reset()  # what the warm-up forward logged

    def _forward(self):
        s = self.static
        with torch.no_grad():
            _, _, x = self.model(s["feats"], s["boxes"], (s["ids"][0], s["ids"][1], s["ids"][2]))
            logit = self.model.logit_fc(x)
            if self.log is not None:
                ops.answer_pick(logit, self.log, rows=self.log.rows)
                return logit, None
            return logit, logit.max(1)[1]

    def __call__(self, feats, boxes, sent):
        """-> (labels [b] int64, logits [b, A] fp32) for b <= batch_size samples; ``sent``: list of strings or the
        (input_ids, input_mask, segment_ids) tuple.  The returned tensors are views of static buffers: consume
        them (``.cpu()``) before the next call.  With a log the labels are views of the log's newest ``b`` entries."""
        b = self.push(feats, boxes, sent)
        if self.log is not None:
            return self.log.labels[self.log.count - b:self.log.count], self.logit[:b]
        return self.label[:b], self.logit[:b]

    def push(self, feats, boxes, sent):
        """queue the forward of one batch (b <= batch_size samples) and return b: what ``__call__`` does, without tensors
        to consume.  With a log the answers of the b kept rows are appended to it on the device -- the row count of a
        short batch travels to the device in stream order ahead of the replay, as the ids do, so the padded rows never
        enter the log -- and the host is not synchronised."""
        b = feats.shape[0]
        if b > self.B:
            raise ValueError("batch of %d exceeds the captured batch size %d" % (b, self.B))
        s = self.static
        if isinstance(sent, (tuple, list)) and len(sent) == 3 and torch.is_tensor(sent[0]):
            for i in range(3):
                s["ids"][i, :b].copy_(sent[i], non_blocking=True)
        else:
            batcher = self.model.lxrt_encoder.batcher
            s["ids"][:, :b].copy_(batcher.host_batch(list(sent)), non_blocking=True)
            batcher.record_copy()  # the pinned buffer is not rewritten before this copy has read it
        s["feats"][:b].copy_(feats, non_blocking=True)
        s["boxes"][:b].copy_(boxes, non_blocking=True)
        return self._queue(b)

    def push_resident(self, store, start, b):
        """``push`` for rows ``start .. start + b`` of the order of ``store`` (tools.resident.ResidentDataset): ONE gather
        launch out of the device-resident tables into the static buffers (fp32 features: a bf16 table is widened on the
        way) instead of the host-to-device copies; the row count travels as in ``push``."""
        if not 1 <= b <= self.B:
            raise ValueError("batch of %d outside the captured batch size %d" % (b, self.B))
        s = self.static
        store.fill(dict(feats=s["feats"], boxes=s["boxes"], input_ids=s["ids"][0], input_mask=s["ids"][1],
                        segment_ids=s["ids"][2]), start, b)
        return self._queue(b)

    def _queue(self, b):
        if self.log is not None:
            self.log.note(b)
            self.log.set_rows(b)
        if self.graph is not None:
            self.graph.replay()
        else:
            was_training = self.model.training
            self.model.eval()
            self.logit, self.label = self._forward()
            self.model.train(was_training)
        return b


class CapturedPretrainer:
    """The LXMERT pre-training step (``LXMERT.train_batch`` / ``valid_batch``, src/pretrain/lxmert_pretrain.py:308-326) as
    ONE replayed graph per step: one pass kind, one graph.  Data parallel (a model prepared by
    ``pretrain.lxmert_pretrain.enable_data_parallel``: one process per GPU, the reference's ``--multiGPU``,
    src/pretrain/lxmert_pretrain.py:255-256) the training step is TWO graphs with the gradient exchange between them:
    graph F = swap, masking, forward, backward; ``_sync_grads`` live on the communicator, never inside a capture; graph U =
    ``clip_and_step(..., advance=True)`` and the log appends -- captured with ``capture_error_mode="thread_local"``
    (``CapturedTrainer`` says why).  The eager path makes the same calls in the same order: the same bits.  ``step()``
    and ``check()`` are then COLLECTIVE calls (every rank makes them, equally often); ``valid_step()`` exchanges nothing and
    stays one graph, so ranks may validate on different numbers of batches.  Every rank logs its OWN losses;
    ``TrainLog.fold`` averages the logs over the ranks at read-back time.  The constructor is collective too (its warm-up
    steps exchange) and restores the state every rank started from, so equal replicas stay equal.  Without
    ``enable_data_parallel`` nothing of this exists: one graph, the same launches.

        feats = DeviceFeatures.from_args(args, swap=True, vocab_size=..., max_labels=K)
        tr = CapturedPretrainer(model, optim, batch, feats, train_log=TrainLog(n, dev), answer_log=AnswerLog(n * B, dev, False))
        for batch in loader: tr.load_batch(batch); tr.step()          # no host synchronisation
        tr.check(); rec = tr.train_log.read()                         # once per N steps

    ``batch``: dict of DEVICE tensors of the CLEAN batch -- input_ids, input_mask, segment_ids, feats, boxes, obj_labels,
    obj_confs, attr_labels, attr_confs, is_matched, label_ids, label_scores (``pretrain.lxmert_pretrain.pack_labels``) and,
    with a swap (``features.match_rate``), img_ids and optionally pool_ids / pool_mask / pool_img; optionally feat_pool (the
    replacement rows of the object masking).  They become the static input buffers; ``load_batch`` copies into them.
    ``resident=store`` (``pretrain.resident.ResidentPretrainSet``): ``static["feat_pool"]`` is the store's whole feature table
    by reference (not cloned; refused when its dtype is not that of ``feats``), and ``load_resident(store, start)`` fills the
    static inputs with one gather launch instead of ``load_batch``.

    ``step()`` holds, in order: the swap (when configured) and the masking (``features``: one or two launches),
    ``LXRTPretraining.forward``, ``Runtime.backward``, ``clip_and_step(model, optim, clip, advance=True)`` (the reference
    clips at 1.0, :315), the log appends.  ``features`` draws from the model's runtime state ``runtime_of(model).rng``: the
    ONE advance at the end of the step moves masks, swaps, dropout and noise together, and a restored ``rng``
    (``vqa.vqacpv2.load_training_state``) reproduces the run.  ``valid_step()`` is the forward-only twin (:320-326),
    captured under ``model.eval()``: swap, masking, forward, log appends, the rng advance -- no backward, no update.

    The warm-up steps and the capture run on the first batch like everything else here, but what they changed is put back
    before the constructor returns -- parameters, moments, step counters, ``rng``, the overflow flag and the swap's
    exhausted counter -- so a captured run, an eager run (``use_graph=False``: the same calls, not captured, no warm-up) and
    a restored run start from the same state and give the same bits.  ``warmup_iters=0``: the caller has run an eager step
    already (a capture needs every workspace to exist); nothing is snapshotted.

    ``optim=None``: a validation-only engine (an eval loader with a batch size of its own, an evaluation before any
    training).  Only the forward-only graph is warmed up and captured, no optimiser step is ever taken on the model -- not
    even one that is rolled back -- and ``step()`` raises.

    ``train_log`` / ``valid_log`` (``TrainLog``; observe only, None adds no launch): one record of kind
    ``trainlog.PRETRAIN`` per step -- LOSS, the reference's six terms at the fixed columns 1-6 (a task that is off leaves its
    column absent), the pre-clip norm in column 7 (absent in ``valid_log``); the record's step is the optimiser counter of the
    arena group that holds ``cls.predictions``.  ``answer_log`` (``AnswerLog(with_scores=False)``): every step of either
    kind ends with ``ops.answer_pick`` on the fp32 answer scores (``logit.max(1)`` of :357 / :392 without its ``.cpu()``).
    A batch of another size than the static one (the ragged last batch of an epoch) goes through ``step(batch)`` /
    ``valid_step(batch)``: the same calls run eagerly on it."""

    KEYS = ("input_ids", "input_mask", "segment_ids", "feats", "boxes", "obj_labels", "obj_confs", "attr_labels", "attr_confs",
            "is_matched", "label_ids", "label_scores")
    POOL = ("pool_ids", "pool_mask", "pool_img")

    def __init__(self, model, optim, batch, features, clip=1.0, use_graph=True, warmup_iters=2, train_log=None,
                 valid_log=None, answer_log=None, resident=None):
        from . import trainlog as T
        from .lxrt.modeling import VISUAL_CONFIG
        self.model, self.optim, self.features, self.clip = model, optim, features, clip
        self.train_log, self.valid_log, self.answer_log = train_log, valid_log, answer_log
        missing = [k for k in self.KEYS if k not in batch]
        if features.match_rate is not None and "img_ids" not in batch:
            missing.append("img_ids")
        if missing:
            raise ValueError("CapturedPretrainer: the batch lacks %s" % missing)
        if 0 < sum(k in batch for k in self.POOL) < 3:
            raise ValueError("CapturedPretrainer: a sentence pool is pool_ids, pool_mask and pool_img together")
        if answer_log is not None and (answer_log.with_scores or not model.task_qa):
            raise ValueError("CapturedPretrainer: answer_log is an AnswerLog(with_scores=False) and needs the QA task")
        if optim is None and train_log is not None:
            raise ValueError("CapturedPretrainer: a validation-only engine (optim=None) appends to no train_log")
        self.static = {k: v.clone() for k, v in batch.items() if torch.is_tensor(v)}
        self.B = self.static["input_ids"].shape[0]
        if resident is not None:
            # every object of every image of the store, by reference: the pool torchdset.random_feat() draws from
            pool = resident.feat_pool()
            if pool.dtype != self.static["feats"].dtype:
                raise ValueError("CapturedPretrainer: resident= hands the store's %s feature table to the object masking as its "
                                 "pool, the batch's feats are %s; build the batch in the store's type (store.buffers(B))"
                                 % (pool.dtype, self.static["feats"].dtype))
            self.static["feat_pool"] = pool
        self.rt = runtime_of(model)
        cols = [T.PT_MASK_LM] if model.task_mask_lm else []
        cols += [T.PT_MATCHED] if model.task_matched else []
        if model.task_obj_predict:
            cols += [dict(obj=T.PT_OBJ, attr=T.PT_ATTR, feat=T.PT_FEAT)[k] for k in VISUAL_CONFIG.visual_losses]
        cols += [T.PT_QA] if model.task_qa else []
        self.columns = cols  # column of the i-th entry of the ``losses`` the model returns
        self.use_graph = use_graph
        self.graphs, self.outputs = {}, {}
        # data parallelism (pretrain.lxmert_pretrain.enable_data_parallel): the training step is two graphs with the live
        # gradient exchange between them; a capture beside a process group polices its own thread only (CapturedTrainer)
        self.split = getattr(model, "_grad_sync", None) is not None
        self.capture_mode = "thread_local" if self.split else "global"
        self._emb_ids = None  # the ids the captured forward looks up (the sparse exchange of the word table reads them)
        self._flags = torch.zeros(1, dtype=torch.int64, device=self.static["input_ids"].device)
        self._flags_host = torch.zeros(1, dtype=torch.int64).pin_memory()
        if use_graph:
            self._capture(warmup_iters)

    # ------------------------------------------------------------------ the two passes
    def _corrupt(self, s):
        pool = tuple(s[k] for k in self.POOL) if self.POOL[0] in s else None
        return self.features(*[s[k] for k in self.KEYS], self.rt.rng, pool=s.get("feat_pool"), img_ids=s.get("img_ids"),
                             sent_pool=pool)

    def _observe(self, log, loss, losses, norm, ans):
        from . import trainlog as T
        if log is not None:
            if losses.shape[1] != len(self.columns):
                raise RuntimeError("CapturedPretrainer: the model returned %d loss terms, its tasks name %d"
                                   % (losses.shape[1], len(self.columns)))
            cols = [None] * T.COLS
            cols[T.LOSS] = loss
            for i, c in enumerate(self.columns):
                cols[c] = losses[0, i:i + 1]
            cols[T.PT_GRAD_NORM] = norm
            arena = self.rt.arena
            xg = getattr(next(self.model.cls.predictions.parameters()), "_xg", None)
            gi = arena.group_index[xg[3]] if xg is not None and xg[0] is arena else None
            ops.train_log_append(log, T.PRETRAIN, cols, step=None if gi is None else arena.steps[gi:gi + 1])
        if self.answer_log is not None:
            ops.answer_pick(ans if ans.dtype == torch.float32 else ans.float(), self.answer_log)

    def _fwd_bwd(self, s):
        """graph F of a data-parallel step: swap, masking, forward, backward"""
        self.model.train()
        if self.split:
            # the gradients are zero here (the previous update cleared them) and a validation forward in between adds to
            # none: the look-up of this forward is the ONE the sparse exchange of the word table has to cover
            self.rt.arena.emb_uses = 0
        total, losses, ans = self.model(*self._corrupt(s))
        self.rt.backward(total)
        return total.detach(), losses, ans

    def _update(self, loss, losses, ans):
        """graph U of a data-parallel step: clip, update, the rng advance, the log appends"""
        norm = clip_and_step(self.model, self.optim, self.clip, advance=True)
        self._observe(self.train_log, loss, losses, norm, ans)
        return norm

    def _train_pass(self, s):
        loss, losses, ans = self._fwd_bwd(s)
        if self.split:
            _sync_grads(self.model)  # live, never inside a capture: the ranks' gradients are averaged where they lie
        norm = self._update(loss, losses, ans)
        return loss, losses, ans, norm

    def _valid_pass(self, s):
        was_training = self.model.training
        self.model.eval()
        with torch.no_grad():
            total, losses, ans = self.model(*self._corrupt(s))
            loss = total.detach()
            self._observe(self.valid_log, loss, losses, None, ans)
            self.rt.advance()
        self.model.train(was_training)
        return loss, losses, ans, None

    def _passes(self):
        train = [("train", self._train_pass)] if self.optim is not None else []
        return train + [("valid", self._valid_pass)]

    # ------------------------------------------------------------------ capture
    def _snapshot(self):
        f = self.features
        trains = self.optim is not None  # validation passes change no weight and no moment: nothing of them to put back
        return dict(model={k: v.clone() for k, v in self.model.state_dict().items()} if trains else None,
                    optim=self.optim.state_dict() if trains else None, rng=self.rt.rng.clone(),
                    overflow=None if self.model.mlm_overflow is None else self.model.mlm_overflow.clone(),
                    exhausted=None if f.swap_exhausted is None else f.swap_exhausted.clone())

    def _restore(self, snap):
        if snap["model"] is not None:
            self.model.load_state_dict(snap["model"])
            self.rt = runtime_of(self.model)  # refreshes the bf16 shadows, outside of any capture
            self.optim.load_state_dict(snap["optim"])
        self.rt.rng.copy_(snap["rng"])
        # the two device counters: back to what they held, or to zero when the warm-up created them
        for t, was in ((self.model.mlm_overflow, snap["overflow"]), (self.features.swap_exhausted, snap["exhausted"])):
            if t is not None:
                t.copy_(was if was is not None else torch.zeros_like(t))
        for log in (self.train_log, self.valid_log, self.answer_log):
            if log is not None:
                log.reset()  # what the warm-up steps logged

    def _capture(self, warmup_iters):
        was_training = self.model.training
        snap = self._snapshot() if warmup_iters > 0 else None
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(warmup_iters):
                for _, run in self._passes():
                    run(self.static)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        mode = {}
        if self.split:
            mode = dict(capture_error_mode=self.capture_mode)
        if self.split and self.optim is not None:
            # nothing of the eager warm-up exchanges may still be in flight (or polled) while graphs are captured; every
            # rank is here: the warm-up is the same number of steps everywhere.  (A validation-only engine exchanged nothing
            # and may be built on one rank alone -- a ragged validation slice -- so it must not wait for the others.)
            import torch.distributed as dist
            dist.barrier()
            torch.cuda.synchronize()
        with _quiet_gc():
            for kind, run in self._passes():
                g = torch.cuda.CUDAGraph()  # a memory pool per graph: the outputs of one are not the other's scratch
                if kind == "train" and self.split:
                    # forward + backward | live exchange | clip + update + logs.  The two graphs share a pool: U reads what
                    # F left (loss, terms, answer scores), which stays referenced here and is therefore never handed out
                    from .dist import active_ranges
                    with torch.cuda.graph(g, **mode):
                        loss, losses, ans = self._fwd_bwd(self.static)
                    ranges, self._emb_ids = active_ranges(self.rt.arena), getattr(self.rt, "emb_ids", None)
                    gu = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(gu, pool=g.pool(), **mode):
                        norm = self._update(loss, losses, ans)
                    self.graphs[kind], self.outputs[kind] = (g, gu, ranges), (loss, losses, ans, norm)
                    continue
                with torch.cuda.graph(g, **mode):
                    out = run(self.static)
                self.graphs[kind], self.outputs[kind] = g, out
        torch.cuda.synchronize()
        if snap is not None:
            self._restore(snap)
        self.model.train(was_training)
        torch.cuda.synchronize()

    # ------------------------------------------------------------------ run
    def load_batch(self, batch):
        for k, v in batch.items():
            if k in self.static:
                self.static[k].copy_(v, non_blocking=True)

    def load_resident(self, store, start):
        """hand over rows ``start .. start + B`` of the epoch order of ``store`` (pretrain.resident.ResidentPretrainSet): ONE
        gather launch out of the device-resident tables into the static inputs (and img_ids / sample where the static batch
        has them), eagerly and in stream order between the replays, where ``load_batch`` would copy -- nothing crosses PCIe
        and no graph is captured again.  A store with a ``match_rate`` swaps in that launch, drawing from the model's
        runtime state ``rng`` at ``features.sid_base`` -- the state the step that follows masks with, so the swap moves with
        the ONE advance per step, and a captured, an eager and a restored run give the same bits.  ``features`` must then
        not swap itself."""
        if getattr(store, "match_rate", None) is not None and self.features.match_rate is not None:
            raise ValueError("CapturedPretrainer.load_resident: the store swaps (match_rate %g) and so does features (match_rate "
                             "%g): the batch would be swapped twice; build DeviceFeatures without a match_rate"
                             % (store.match_rate, self.features.match_rate))
        if "img_ids" not in self.static:  # the launch writes it; a batch without a swap of its own came without one
            self.static["img_ids"] = torch.zeros(self.B, dtype=torch.int64, device=self.static["input_ids"].device)
        store.fill(self.static, start, self.B, rng=runtime_of(self.model).rng, sid_base=self.features.sid_base)

    def _run(self, kind, batch):
        if kind == "train" and self.optim is None:
            raise RuntimeError("CapturedPretrainer.step: this engine was built without an optimiser (validation only)")
        run = self._train_pass if kind == "train" else self._valid_pass
        if batch is not None and batch["input_ids"].shape[0] != self.B:
            if self.answer_log is not None:
                self.answer_log.note(batch["input_ids"].shape[0])
            return run(batch)  # the ragged last batch: the same calls, eagerly, on the batch as it is
        if batch is not None:
            self.load_batch(batch)
        if self.answer_log is not None:
            self.answer_log.note(self.B)
        if not self.use_graph:
            return run(self.static)
        runtime_of(self.model)  # weights loaded since the last step (load_state_dict): the bf16 shadows are refreshed here
        g = self.graphs[kind]
        if isinstance(g, tuple):  # data parallel: the exchange runs live between the two graphs
            # host-side bookkeeping a replay never runs (CapturedTrainer.run_pass): the sparse exchange of the word table
            # gathers the rows of the ids THIS step's forward looks up, once
            self.rt.emb_ids = self._emb_ids
            self.rt.arena.emb_uses = 1
            g[0].replay()
            self.model._grad_sync.sync(g[2])
            g[1].replay()
        else:
            g.replay()
        return self.outputs[kind]

    def step(self, batch=None):
        """one training step -> (loss, losses [1, n], answer scores, pre-clip norm): device tensors, views of static
        buffers under a graph (consume them before the next step).  ``batch``: loaded first; another batch size than the
        static one runs eagerly.  Under data parallelism a COLLECTIVE call (every rank steps, on a batch of its own), and
        the replica guard, when there is one, counts the step"""
        out = self._run("train", batch)
        if self.split:
            guard = getattr(self.model, "_replica_guard", None)
            if guard is not None:
                guard.tick()  # eager work between two replays, never part of a graph (the check is a collective)
        return out

    def valid_step(self, batch=None):
        """the forward-only step -> (loss, losses, answer scores, None); it changes no parameter and no optimiser state"""
        return self._run("valid", batch)

    def _agree_on_overflow(self):
        """data parallel: MAX of the ranks' overflow flags into ``_flags_host``, so that either every rank raises or none
        does -- a rank that raised alone would leave the others hung in the next exchange.  The ranks first meet on the
        host with a timeout (``dist._meet``): a lone caller gets a RuntimeError, not a hung group."""
        import torch.distributed as dist
        from .dist import _meet
        gs = self.model._grad_sync
        if not dist.is_initialized() or gs.world == 1:
            return
        _meet(gs, "pretrain_check", None,
              "CapturedPretrainer.check: only %d of %d ranks reached %s (call %d) within %.0f s.  Under data parallelism "
              "check() is a COLLECTIVE call: make it on every rank, not inside `if rank == 0:`")
        t = self._flags_host.clone() if gs.backend != "nccl" else self._flags.clone()
        dist.all_reduce(t, op=dist.ReduceOp.MAX, group=gs.group)
        self._flags_host.copy_(t)

    def check(self, collective=None):
        """``collective`` (default: whether the model is data parallel): the ranks first agree on the flag (MAX), so that
        either every rank raises or none does -- then a COLLECTIVE call; False: this rank's flag alone (the driver's
        validation sweep, where the ranks take different numbers of steps, collects what it raises and agrees once, after
        the sweep).
        ONE synchronisation per read-back: the masked-LM overflow flag ``model.mlm_overflow`` (more labelled rows than
        ``mlm_capacity`` slots: the masked-LM loss of that step was NaN).  Nothing is raised while it is clear -- a NaN of
        another origin (a batch whose swap left no QA label has a NaN QA loss, as in the reference) is the log's business
        (``first_bad``), not an error here.  When it is set, the attached logs are read (the failing path alone pays that
        second transfer) and the RuntimeError names the first retained record whose Mask_LM column is NaN -- its number
        since the log's reset and the optimiser step it carries -- not merely the first non-finite record; the flag is
        cleared, so the next read-back reports the next overflow.  Called by the driver once per read-back, never per
        step."""
        from . import trainlog as T
        flag = self.model.mlm_overflow
        if flag is None:
            return
        self._flags[0:1].copy_(flag)
        self._flags_host.copy_(self._flags, non_blocking=True)
        torch.cuda.current_stream(self._flags.device).synchronize()
        if self.split if collective is None else collective:
            self._agree_on_overflow()
        if not int(self._flags_host[0]):
            return
        flag.zero_()
        where = []
        for name, log in (("training", self.train_log), ("validation", self.valid_log)):
            if log is None:
                continue
            rec = log.read()
            bad = (torch.isnan(rec["values"][:, T.PT_MASK_LM]) & rec["present"][:, T.PT_MASK_LM]).nonzero().reshape(-1)
            if bad.numel():
                row, m = int(bad[0]), rec["values"].shape[0]
                number = int(rec["cursor"]) - m + row
                where.append("the first %s record with a NaN Mask_LM is number %d since the log's reset (step %d of this "
                             "window, optimiser step %d)" % (name, number, number + 1, int(rec["steps"][row])))
        none = "no attached log of this rank retains the step (it overflowed on another rank)" if self.split \
            else "no attached log retains the step"
        raise RuntimeError("masked-LM overflow: a batch had more labelled tokens than mlm_capacity=%r slots; %s"
                           % (self.model.mlm_capacity, "; ".join(where) or none))
