"""BertAdam with the reference's constructor and semantics (src/lxrt/optimization.py:58-203)
running as ONE fused HIP pass per contiguous parameter range: clip scale, moment update,
weight decay, scheduled step and the bf16 shadow-weight write.

State lives in the model's flat arena (``next_m``/``next_v`` = arena.m / arena.v); the
per-parameter ``state['step']`` of the reference becomes one device-resident counter per
arena group (all parameters of a group always step together), from which
``warmup_linear`` is evaluated on the device -- no host synchronisation, graph replayable.
"""
import math

import torch
from torch.optim import Optimizer

from .. import ops


def warmup_cosine(x, warmup=0.002):
    if x < warmup:
        return x / warmup
    return 0.5 * (1.0 + math.cos(math.pi * x))


def warmup_constant(x, warmup=0.002):
    if x < warmup:
        return x / warmup
    return 1.0


def warmup_linear(x, warmup=0.002):
    if x < warmup:
        return x / warmup
    return max((x - 1.) / (warmup - 1.), 0)


SCHEDULES = {'warmup_cosine': warmup_cosine, 'warmup_constant': warmup_constant, 'warmup_linear': warmup_linear}


def _arena_of_params(params):
    for p in params:
        xg = getattr(p, "_xg", None)
        if xg is not None:
            return xg[0]
    return None


def clip_grad_norm_(parameters, max_norm, tail=None):
    """fused replacement of ``nn.utils.clip_grad_norm_(model.parameters(), 5.)``
    (src/vqa/vqacpv2.py:175): one sum-of-squares reduction per active arena range; the scale
    min(1, max_norm/(norm+1e-6)) is applied INSIDE the following BertAdam.step (the gradients
    in memory stay unscaled).  Returns the total norm as a device scalar.
    ``tail`` = (optimiser, runtime or None), given by ``vqa.vqacpv2.clip_and_step``: the launch that finishes the norm
    also takes the schedule step of the ``optimiser.step()`` that follows and -- with a runtime -- the RNG advance that
    ends the pass (``arena.sched_done`` / ``runtime.rng_advanced`` tell the two that their launch has been made)."""
    params = [p for p in parameters]
    arena = _arena_of_params(params)
    if arena is None:
        raise RuntimeError("clip_grad_norm_: parameters are not arena-managed; run a forward first")
    if arena.wire is not None:  # data parallel, bf16 wire arena: the (averaged) gradients live there
        if arena.zero1 is None:
            spans = [(a, b) for a, b in _active_ranges(arena) if b > a]
            if len(spans) <= ops.CLIP_NORM_MAX_SPANS and all(a % 8 == 0 for a, _ in spans):
                # replicated update: every rank sums the whole wire itself -- one pair of launches, the pass's scalar
                # bookkeeping on the finishing one (as on one GPU); |mean|^2 = |sum|^2 / world^2
                total = torch.empty(1, device=arena.grads.device, dtype=torch.float32)
                sched, rng = _tail_of(arena, tail)
                ops.clip_norm_bf16(arena.wire, spans, arena.sqnorm, total, mul=arena.grad_scale ** 2, sched=sched, rng=rng)
                arena.pending_clip = float(max_norm)
                return total.view(())
        clip_norm_local(arena)
        if arena.zero1 is not None:
            arena.zero1.exchange_norm(arena.sqnorm)
        return clip_norm_finish(arena, max_norm, tail)
    # ranges of the flat gradient buffer the norm pass has to READ: everything of the active groups except the
    # matrices whose weight-gradient GEMM already left its sum of squares in the slot table (arena.sq_target);
    # adjacent ranges are merged
    spans, slot_spans = [], []

    def add(a, b):
        if b > a:
            if spans and spans[-1][1] == a:
                spans[-1][1] = b
            else:
                spans.append([a, b])

    for g in sorted(arena.active_groups(), key=lambda n: arena.groups[n].start):
        G = arena.groups[g]
        covered = arena.sq_covered if (arena.sq_enabled and g in arena.sq_range) else ()
        if not covered:
            add(G.start, G.end)
            continue
        pos = G.start
        for o, k, n in sorted((o, k, n) for n, (o, k, g_, _) in arena.info.items() if g_ == g and n in covered):
            add(pos, o)
            pos = o + k  # alignment gaps hold zeros
        add(pos, G.end)
        slot_spans.append(arena.sq_range[g])
    # two launches for all ranges, two more for the slot table; sums in a fixed order (deterministic replicas); the
    # finish kernels seed the running sum and write the norm: no framework fill / add / sqrt kernels in the pass
    rl = arena.row_list
    if rl is not None and rl.clean and rl.listed and arena.row_list_enabled:
        # the word table's gradient: its non-zero rows are the ones the embedding backward of this pass listed, with
        # their sums of squares in the slots behind the products' -- 94 MB the norm does not read (arena.RowList)
        from ..arena import _cut
        cut = _cut([tuple(sp) for sp in spans], rl.o, rl.o + rl.R * rl.H)
        if cut != [tuple(sp) for sp in spans]:
            spans = [list(sp) for sp in cut]
            slot_spans.append((arena.row_sq0, arena.row_sq0 + rl.listed))
    total = torch.empty(1, device=arena.grads.device, dtype=torch.float32)
    if len(spans) + len(slot_spans) <= ops.CLIP_NORM_MAX_SPANS:
        # one pair of launches for the ranges AND the slot table; the finishing one carries the pass's scalar bookkeeping
        sched, rng = _tail_of(arena, tail)
        ops.clip_norm(arena.grads, spans, arena.sq_slots if slot_spans else None, slot_spans, arena.sqnorm, total, sched=sched,
                      rng=rng)
    else:
        ops.sqnorm_multi(arena.grads, spans, arena.sqnorm, None if slot_spans else total, overwrite=True)
        if slot_spans:
            ops.sqnorm_multi(arena.sq_slots, slot_spans, arena.sqnorm, total, overwrite=False, square=False)
    arena.pending_clip = float(max_norm)
    return total.view(())


def _tail_of(arena, tail):
    """(sched, rng) arguments of ops.clip_norm* for ``tail`` = (optimiser, runtime or None) of clip_grad_norm_, and the
    marks that tell ``optimiser.step()`` / ``runtime.advance()`` that their launch has been made"""
    sched = rng = None
    if tail is not None:
        optim, rt = tail
        require_arena_aware(optim)
        # the optimiser says what its schedule step is; None: the norm's finishing launch cannot carry it (a non-linear
        # schedule kind, or a rule with bias corrections) -- ``sched_done`` stays False and ``step()`` makes its own launch
        entries = optim._tail_entries(arena)
        if entries and len(entries) <= ops.CLIP_NORM_MAX_SCHED:
            sched = (arena.steps, arena.lr_scale, entries)
            arena.sched_done = True
        if rt is not None:
            rng = (rt.rng, 1)
            rt.rng_advanced = True
    return sched, rng


def _active_ranges(arena):
    return [(arena.groups[g].start, arena.groups[g].end)
            for g in sorted(arena.active_groups(), key=lambda n: arena.groups[n].start)]


def clip_norm_local(arena):
    """wire-arena norm, first half: seed the running sum and add what THIS rank sums alone -- everything without a
    sharded update, the own slices of the matrix runs with one (their sum is then all-reduced: ShardedUpdate)"""
    z = arena.zero1
    spans = _active_ranges(arena) if z is None else z.norm_spans(_active_ranges(arena))[0]
    spans = [(a, b) for a, b in spans if b > a]
    if len(spans) <= ops.CLIP_NORM_MAX_SPANS and all(a % 8 == 0 for a, _ in spans):
        ops.clip_norm_bf16(arena.wire, spans, arena.sqnorm)  # seeds the sum: one pair of launches for all ranges
        return
    ops.sqnorm_multi(arena.grads, [], arena.sqnorm, None, overwrite=True)
    for a, b in spans:
        ops.sqnorm_bf16(arena.wire[a:b], arena.sqnorm)


def clip_norm_finish(arena, max_norm, tail=None):
    """second half: the vector ranges every rank holds in full (sharded update only), then the norm"""
    z = arena.zero1
    spans = [(a, b) for a, b in (z.norm_spans(_active_ranges(arena))[1] if z is not None else []) if b > a]
    total = torch.empty(1, device=arena.grads.device, dtype=torch.float32)
    # the wire holds sums over the ranks: |mean|^2 = |sum|^2 / world^2
    if len(spans) <= ops.CLIP_NORM_MAX_SPANS and all(a % 8 == 0 for a, _ in spans):
        sched, rng = _tail_of(arena, tail)
        ops.clip_norm_bf16(arena.wire, spans, arena.sqnorm, total, accumulate=True, mul=arena.grad_scale ** 2, sched=sched, rng=rng)
    else:
        for a, b in spans:
            ops.sqnorm_bf16(arena.wire[a:b], arena.sqnorm)
        ops.sqnorm_multi(arena.grads, [], arena.sqnorm, total, overwrite=False, mul=arena.grad_scale ** 2)
    arena.pending_clip = float(max_norm)
    return total.view(())


def require_arena_aware(optim):
    """A ``torch.optim`` class over arena-managed parameters looks healthy and trains nothing: it updates the fp32
    masters while every product reads the bf16 shadow only the fused update writes, and it never sees the clip scale
    (``clip_grad_norm_`` applies it inside the fused update)."""
    if not isinstance(optim, ArenaOptimizer):
        raise TypeError("%s is not arena-aware: over this package's models it would update the fp32 masters only (stale "
                        "bf16 weights, unclipped gradients).  Use the class of the same name from xggm_amd.optim (Adam, "
                        "AdamW, Adamax, SGD, RMSprop) or xggm_amd.lxrt.optimization.BertAdam"
                        % (type(optim).__module__ + "." + type(optim).__name__))


class ArenaOptimizer(Optimizer):
    """What every optimiser of this package shares: state in the model's flat arena, one device-resident step counter
    per arena group, learning rates in a device table, ONE fused launch for all spans of a pass.  A subclass gives the
    rule: its kernel hyper-parameters, its schedule step and its state layout."""

    # ``split_groups=True`` (constructor keyword of every class): param_groups may cut through an arena group and differ
    # there in lr and weight_decay; the update then reads both per tensor from a device map (ops.optim_multi with
    # ``hyper_map``).  Off: one lr / weight_decay per arena group, a split is refused.
    split_groups = False
    rule = None  # key of ops.RULES
    SPLIT_KEYS = ('lr', 'weight_decay')  # what param_groups inside one arena group may differ in

    @property
    def _name(self):
        return type(self).__name__

    # ---- hooks
    def _state_into_arena(self, arena, state):
        raise NotImplementedError

    def _check_arena(self, arena):
        """refuse arena modes the rule does not support"""

    def _kernel_hyper(self, pg):
        """(b1, b2, eps, weight_decay) of ``xggm_adam_args`` for this param_group"""
        raise NotImplementedError

    def _tail_entries(self, arena):
        """[(counter, t_total, warmup)] when the schedule step of the coming ``step()`` can ride on the norm's finishing
        launch (warmup_linear semantics of ``xggm_pass_tail``), else None"""
        return None

    def _sched_launch(self, arena, todo):
        """the stand-alone schedule step: counters, ``lr_scale`` and whatever the rule needs per step"""
        raise NotImplementedError

    def _variant(self, pg):
        """(rule name of ops.RULES, anything else that selects another kernel instantiation): spans of one launch share it"""
        return (self.rule,)

    def _rule_args(self, pg):
        """the rule's keyword arguments of ops.optim_multi for this param_group (the group's step scalars are added), or
        None: the rule takes neither"""
        return None

    def _launch(self, arena, jobs, hyper_map=None):
        """``jobs``: [(positional arguments of a span of ops.optim_multi, its keyword arguments, param_group, group index)];
        ``hyper_map``: (ids, table) under split_groups"""
        by = {}
        for a, kw, pg, gi in jobs:
            r = self._rule_args(pg)
            if r is not None:
                r = dict(r, step_scalars=arena.step_scalars[4 * gi:4 * gi + 4])
            by.setdefault(self._variant(pg), []).append((a, kw, r or {}))
        for key in sorted(by):
            ops.optim_multi(key[0], by[key], hyper_map=hyper_map)

    # ---- shared plumbing
    def _arena(self):
        arena = _arena_of_params(p for pg in self.param_groups for p in pg['params'])
        pending = getattr(self, "_pending_state", None)
        if arena is not None and pending is not None:
            self._pending_state = None
            self._state_into_arena(arena, pending)
        return arena

    def _hyper_of_group(self, arena, gname):
        """the optimiser param_group that speaks for arena group ``gname`` (one contiguous range, one launch), or None
        when the optimiser holds none of its parameters.
        Default: the param_group that holds ALL parameters of the arena group.  A param_groups split that cuts through
        an arena group -- the usual BERT "no decay for bias / LayerNorm" grouping would -- cannot be honoured by a flat
        update with one lr / weight_decay and is refused instead of silently applying the first parameter's settings
        to the whole range.
        With ``split_groups=True`` the split is honoured: the param_groups that share an arena group may differ in
        ``lr`` and ``weight_decay`` (read per tensor from the hyper map, ``_hyper_map``), parameters in no param_group
        are left untouched, and the first param_group found stands for every other key -- schedule, betas, eps,
        momentum ... -- which must agree inside the arena group (step counter and schedule value stay one per arena
        group): a difference raises a ValueError that names the key."""
        cache = getattr(self, "_group_pg", None)
        if cache is None:
            cache = self._group_pg = {}
        if gname not in cache:
            owner = {}
            for i, pg in enumerate(self.param_groups):
                for p in pg['params']:
                    owner[id(p)] = i
            idx = {owner.get(id(p)) for p in arena.groups[gname].params}
            if self.split_groups:
                idx = sorted(i for i in idx if i is not None)
                first = self.param_groups[idx[0]] if idx else None
                for i in idx[1:]:
                    pg = self.param_groups[i]
                    for k in sorted(set(first) | set(pg)):
                        if k != 'params' and k not in self.SPLIT_KEYS and first.get(k) != pg.get(k):
                            raise ValueError("%s(split_groups=True): param_groups %d and %d share arena group '%s' and differ "
                                             "in '%s' (%r, %r); inside an arena group only %s may differ"
                                             % (self._name, idx[0], i, gname, k, first.get(k), pg.get(k),
                                                " and ".join(self.SPLIT_KEYS)))
                idx = {idx[0] if idx else None}
            if len(idx) > 1:
                raise ValueError("%s: the parameters of arena group '%s' are spread over optimiser param_groups %s; "
                                 "a group is updated as one range with one lr / weight_decay / schedule -- keep its "
                                 "parameters in one param_group (vqa.vqacpv2.make_optimizer does)"
                                 % (self._name, gname, sorted(idx, key=str)))
            cache[gname] = idx.pop()
        i = cache[gname]
        return None if i is None else self.param_groups[i]

    def _hyper_map(self, arena, upload=True):
        """split_groups: (ids, table) of ops.optim_multi -- the id map of this optimiser over
        ``arena`` (arena.hyper_id_map: one uint8 per 8 elements, 1 + index of the owning param_group, 0 = not ours),
        built and uploaded once, and the {lr, weight_decay} table with one row per param_group behind row 0, rewritten
        when a value changed.  Both outside of captures only."""
        st = getattr(self, "_split_state", None)
        if st is None or st['arena'] is not arena or st['n'] != len(self.param_groups):
            if not upload or torch.cuda.is_current_stream_capturing():
                raise RuntimeError("%s.step is being captured before any eager step: run one pass eagerly first "
                                   "(the hyper map is uploaded to the device outside of captures)" % self._name)
            from ..arena import hyper_id_map
            owner = {}
            for i, pg in enumerate(self.param_groups):
                for p in pg['params']:
                    xg = getattr(p, "_xg", None)
                    if xg is not None and xg[0] is arena:
                        owner[xg[5]] = i + 1
            ids = hyper_id_map(arena.info, owner, arena.total)  # (ValueError: more param_groups than the ids hold)
            st = self._split_state = dict(arena=arena, n=len(self.param_groups), host=None,
                                          ids=torch.from_numpy(ids).to(arena.device),
                                          table=torch.zeros(len(self.param_groups) + 1, 2, device=arena.device))
        if upload:
            host = [(0.0, 0.0)] + [(float(pg['lr']), float(pg['weight_decay'])) for pg in self.param_groups]
            if host != st['host']:
                if torch.cuda.is_current_stream_capturing():
                    raise RuntimeError("%s: a learning rate or weight decay changed during graph capture; call sync_hyper() "
                                       "before" % self._name)
                st['table'].copy_(torch.tensor(host, dtype=torch.float32))
                st['host'] = host
        return st['ids'], st['table']

    def sync_hyper(self):
        """push ``param_groups[i]['lr']`` -- with ``split_groups=True`` also ``['weight_decay']`` -- to the device table the
        update kernels read: call after editing one between replays of a captured pass (an eager ``step()`` does it by
        itself)"""
        arena = self._arena()
        if arena is None:
            return
        if self.split_groups:
            self._hyper_map(arena)
            return
        for g in arena.groups:
            pg = self._hyper_of_group(arena, g)
            gi = arena.group_index[g]
            if pg is not None and arena.lr_host[gi] != float(pg['lr']):
                if torch.cuda.is_current_stream_capturing():
                    raise RuntimeError("%s: a learning rate changed during graph capture; call sync_hyper() before" % self._name)
                arena.lr_table[gi] = float(pg['lr'])
                arena.lr_host[gi] = float(pg['lr'])

    def zero_grad(self, set_to_none=True):
        super().zero_grad(set_to_none=True)
        arena = self._arena()
        if arena is not None:
            arena.begin_pass()

    def _todo(self, arena):
        """(group, its param_group, its index) for every arena group that received gradients in this pass"""
        self._check_arena(arena)
        if self.split_groups and arena.zero1 is not None:
            raise RuntimeError("%s(split_groups=True) does not run under the sharded update (zero1): a rank's slices are "
                               "updated with one lr / weight_decay per arena group; build the optimiser without "
                               "split_groups, or the data parallelism without zero1" % self._name)
        todo = []
        for g in arena.active_groups():
            G = arena.groups[g]
            pg = self._hyper_of_group(arena, g)
            if pg is None:
                continue  # parameters not handed to this optimiser
            if any(p.grad is None for p in G.params):
                raise RuntimeError("arena group '%s' received gradients for only part of its parameters" % g)
            todo.append((G, pg, arena.group_index[g]))
        return todo

    @torch.no_grad()
    def step(self, closure=None):
        loss = closure() if closure is not None else None
        arena = self._arena()
        if arena is None:
            raise RuntimeError("%s.step: parameters are not arena-managed; run a forward/backward first" % self._name)
        sq = arena.sqnorm if arena.pending_clip is not None else None
        max_norm = arena.pending_clip if arena.pending_clip is not None else 0.0
        todo = self._todo(arena)
        if todo and not getattr(arena, "sched_done", False):  # schedule values and step counters of all groups: one launch
            self._sched_launch(arena, todo)
        arena.sched_done = False  # (True: clip_grad_norm_'s finishing launch has taken the step along)
        hyper_map = None
        if not torch.cuda.is_current_stream_capturing():
            self.sync_hyper()  # the kernels read lr from a device table: edits of param_groups survive graph replay
        elif not self.split_groups and any(arena.lr_host[gi] is None for _, _, gi in todo):  # (split: _hyper_map below)
            raise RuntimeError("%s.step is being captured before any eager step: run one pass eagerly first "
                               "(the learning rates are uploaded to the device outside of captures)" % self._name)
        f8 = arena.fp8
        gbuf = arena.wire if arena.wire is not None else arena.grads  # bf16 wire arena: the update reads it directly
        gscale = arena.grad_scale if arena.wire is not None else 1.0     # ... and holds sums over the ranks
        z = arena.zero1
        jobs = []  # every span of this step: ONE launch (xggm_optim_multi)
        if f8 is not None:
            # new scales of the weight operands of every group, before the update rewrites their e4m3 copies
            f8.update_weight_scales_of([G.name for G, _, _ in todo])
        for G, pg, gi in todo:
            scale_t = arena.lr_scale[gi:gi + 1]
            hyper = tuple(self._kernel_hyper(pg))
            if z is not None:
                # sharded update: this rank's slice of every matrix run of the group + the whole vector region.  With the
                # fp8 forward a slice also writes ITS part of the e4m3 weight copies (slices are whole 256-element chunks
                # of the scale-id table) under scales derived from maxima that ShardedUpdate.exchange_norm has just
                # MAX-reduced over the ranks -- identical tables on every rank; gather() brings the other slices over
                w8g = f8.adam_w8(G.name) if f8 is not None else None
                pieces = [z.own(r) + (True,) for r in z.runs if r[0] >= G.start and r[1] <= G.vec_start]
                pieces.append((G.vec_start, G.end, False))
                for a, b, is_mat in pieces:
                    if b > a:
                        sl = slice(a, b)
                        w8 = ((f8.shadow8[sl],) + w8g) if (w8g is not None and is_mat) else None
                        jobs.append(((arena.params[sl], gbuf[sl], arena.m[sl], arena.v[sl], arena.shadow[sl], sq, max_norm,
                                      pg['lr'], scale_t) + hyper,
                                     dict(lr_dev=arena.lr_table[gi:gi + 1], w8=w8, elem0=a, g_scale=gscale), pg, gi))
                continue
            sl = slice(G.start, G.end)
            w8 = f8.adam_w8(G.name) if f8 is not None else None
            if w8 is not None:
                # fp8 forward: this group's weight operands get their e4m3 copies from the same pass over p, with
                # the scales the delayed update derives from the maxima earlier steps recorded
                w8 = (f8.shadow8[sl],) + w8
            jobs.append(((arena.params[sl], gbuf[sl], arena.m[sl], arena.v[sl],
                          None if arena.shadow is None else arena.shadow[sl], sq, max_norm, pg['lr'], scale_t) + hyper,
                         dict(lr_dev=arena.lr_table[gi:gi + 1], w8=w8, elem0=G.start, g_scale=gscale), pg, gi))
        if self.split_groups and jobs:
            hyper_map = self._hyper_map(arena, upload=False)
        self._launch(arena, jobs, hyper_map)
        arena.pending_clip = None
        return loss


class BertAdam(ArenaOptimizer):
    """ref: src/lxrt/optimization.py:58-203 (no bias correction; decoupled weight decay on
    every parameter; gradient clipping is done outside, as LXMERT does)."""
    rule = "bertadam"

    def __init__(self, params, lr, warmup=-1, t_total=-1, schedule='warmup_linear', b1=0.9, b2=0.999, e=1e-6,
                 weight_decay=0.01, max_grad_norm=1.0, split_groups=False):
        if lr < 0.0:
            raise ValueError("Invalid learning rate: {} - should be >= 0.0".format(lr))
        if schedule not in SCHEDULES:
            raise ValueError("Invalid schedule parameter: {}".format(schedule))
        if not 0.0 <= warmup < 1.0 and not warmup == -1:
            raise ValueError("Invalid warmup: {} - should be in [0.0, 1.0[ or -1".format(warmup))
        if not 0.0 <= b1 < 1.0:
            raise ValueError("Invalid b1 parameter: {} - should be in [0.0, 1.0[".format(b1))
        if not 0.0 <= b2 < 1.0:
            raise ValueError("Invalid b2 parameter: {} - should be in [0.0, 1.0[".format(b2))
        if not e >= 0.0:
            raise ValueError("Invalid epsilon value: {} - should be >= 0.0".format(e))
        defaults = dict(lr=lr, schedule=schedule, warmup=warmup, t_total=t_total, b1=b1, b2=b2, e=e,
                        weight_decay=weight_decay, max_grad_norm=max_grad_norm)
        self.split_groups = bool(split_groups)
        super().__init__(params, defaults)

    # ---- checkpointing: the reference layout (src/lxrt/optimization.py:147-155 keeps per-parameter
    # state['step'], state['next_m'], state['next_v']), read from / written into the flat arena
    def state_dict(self):
        sd = super().state_dict()
        arena = self._arena()
        if arena is None:
            if getattr(self, "_pending_state", None) is not None:
                sd['state'] = self._pending_state
            return sd
        arena.gather_sharded_state()  # ZeRO-1: the moments of the other ranks' slices (collective, see dist.ShardedUpdate)
        steps = arena.steps.tolist()
        state, idx = {}, 0
        for pg in self.param_groups:
            for p in pg['params']:
                xg = getattr(p, "_xg", None)
                if xg is not None and xg[0] is arena:
                    _, o, k, gname = xg[:4]
                    state[idx] = {'step': steps[arena.group_index[gname]],
                                  'next_m': arena.m[o:o + k].view(p.shape).clone(),
                                  'next_v': arena.v[o:o + k].view(p.shape).clone()}
                idx += 1
        sd['state'] = state
        return sd

    def load_state_dict(self, state_dict):
        """hyper-parameters through torch's loader, moments and step counters IN PLACE into the arena (captured
        graphs keep pointing at the same buffers).  Before the arena exists (no forward yet) the state is kept and
        applied at the first use."""
        groups = state_dict['param_groups']
        if 'layer_adaptation' not in self.defaults:  # a BertLamb checkpoint: the moments are the same, its flag is not ours
            groups = [{k: v for k, v in g.items() if k != 'layer_adaptation'} for g in groups]
        super().load_state_dict({'state': {}, 'param_groups': groups})
        self._pending_state = dict(state_dict.get('state', {}))
        self._arena()

    @torch.no_grad()
    def _state_into_arena(self, arena, state):
        step_of, idx = {}, 0
        for pg in self.param_groups:
            for p in pg['params']:
                st = state.get(idx, state.get(str(idx)))
                idx += 1
                xg = getattr(p, "_xg", None)
                if st is None or xg is None or xg[0] is not arena:
                    continue
                _, o, k, gname = xg[:4]
                arena.m[o:o + k].view(p.shape).copy_(st['next_m'])
                arena.v[o:o + k].view(p.shape).copy_(st['next_v'])
                if step_of.setdefault(gname, int(st['step'])) != int(st['step']):
                    raise ValueError("BertAdam.load_state_dict: parameters of arena group '%s' carry different step "
                                     "counts (%d, %d); they always step together here" % (gname, step_of[gname],
                                                                                          int(st['step'])))
        for gname, s in step_of.items():
            arena.steps[arena.group_index[gname]] = s

    def get_lr(self):
        """ref :100-114: the scheduled learning rate of every parameter, in param_groups order; ``[0]`` while some
        parameter has never been stepped (the reference's empty ``state[p]``)."""
        arena = self._arena()
        if arena is None:
            return [0]
        steps = arena.steps.tolist()
        lr = []
        for pg in self.param_groups:
            for p in pg['params']:
                xg = getattr(p, "_xg", None)
                if xg is None or xg[0] is not arena:
                    return [0]
                s = steps[arena.group_index[xg[3]]]
                if s == 0:
                    return [0]
                if pg['t_total'] != -1:
                    lr.append(pg['lr'] * SCHEDULES[pg['schedule']](s / pg['t_total'], pg['warmup']))
                else:
                    lr.append(pg['lr'])
        return lr

    # ---- the rule
    def _kernel_hyper(self, pg):
        return pg['b1'], pg['b2'], pg['e'], pg['weight_decay']

    @staticmethod
    def _linear(pg):
        return pg['schedule'] == 'warmup_linear' or pg['t_total'] <= 0  # (no t_total: every kind is the constant 1)

    def _tail_entries(self, arena):
        todo = self._todo(arena)
        if not all(self._linear(pg) for _, pg, _ in todo):
            return None
        return [(gi, pg['t_total'], pg['warmup']) for _, pg, gi in todo]

    def _sched_launch(self, arena, todo):
        if all(self._linear(pg) for _, pg, _ in todo):
            ops.sched_step_multi(arena.steps, arena.lr_scale, [(gi, pg['t_total'], pg['warmup']) for _, pg, gi in todo])
        else:  # warmup_cosine / warmup_constant (ref :27-39): a schedule kind per entry
            ops.sched_step_ex(arena.steps, arena.lr_scale, None,
                              [(gi, pg['t_total'], pg['warmup'], pg['schedule'], 0.0, 0.0) for _, pg, gi in todo])


# ---------------------------------------------------------------------------------------------------------------- BertLamb
def lamb_sum_host(x):
    """the fp64 sum of a 1-D array in the order ``xggm_lamb_multi`` sums a tensor's p^2 and u^2 (include/xggm.h, "ORDER OF
    THE SUMS"): chunks of 2048 from the first element on, 256 threads with two runs of four values each, a tree inside
    every 64 threads, the four results pairwise; then the chunks' partials strided over 256 threads and the same
    reduction.  numpy, no device."""
    import numpy as np

    def reduce256(a):  # [rows, 256] -> [rows]
        a = a.reshape(-1, 4, 64).copy()
        h = 32
        while h >= 1:
            a[:, :, :h] = a[:, :, :h] + a[:, :, h:2 * h]
            h //= 2
        return (a[:, 0, 0] + a[:, 1, 0]) + (a[:, 2, 0] + a[:, 3, 0])

    x = np.asarray(x, dtype=np.float64).reshape(-1)
    chunk = ops.LAMB_CHUNK
    C = max(1, -(-x.size // chunk))
    x = np.concatenate([x, np.zeros(C * chunk - x.size)]).reshape(C, 2, 256, 4)
    a = np.zeros((C, 256))
    for u in range(2):
        for k in range(4):
            a = a + x[:, u, :, k]
    part = reduce256(a)
    R = -(-C // 256)
    part = np.concatenate([part, np.zeros(R * 256 - C)]).reshape(R, 256)
    b = np.zeros(256)
    for r in range(R):
        b = b + part[r]
    return float(reduce256(b[None])[0])


def lamb_step_host(p, g, m, v, lr, b1=0.9, b2=0.999, e=1e-6, weight_decay=0.01, adapted=True):
    """``BertLamb``'s step of ONE tensor restated in fp64 (numpy): ``g`` is the clipped gradient, ``lr`` the scheduled
    learning rate.  -> (p, m, v, ratio); the ratio is rounded to fp32 as the kernel's is."""
    import numpy as np
    p, g, m, v = (np.asarray(t, dtype=np.float64).reshape(-1) for t in (p, g, m, v))
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    u = m / (np.sqrt(v) + e)
    if weight_decay > 0.0:
        u = u + weight_decay * p
    sp, su = lamb_sum_host(p * p), lamb_sum_host(u * u)
    r = float(np.float32(math.sqrt(sp) / math.sqrt(su))) if (adapted and sp > 0.0 and su > 0.0) else 1.0
    return p - lr * r * u, m, v, r


class BertLamb(BertAdam):
    """LAMB over BertAdam: the same moments, schedules, constructor and ``state_dict`` layout (ref:
    src/lxrt/optimization.py:58-203), and the step of every parameter tensor T multiplied by the trust ratio
    ||p_T|| / ||u_T|| of that tensor (1 where a norm is zero) -- the layer-wise adaptation the BERT code base shipped for
    large batches.  One new param_group key, ``layer_adaptation`` (default True): False leaves the group's tensors at
    ratio 1, which is BertAdam bit for bit.  The update is two passes and a finish (``ops.lamb_multi``); a tensor's norms
    are summed in double in an order that depends on its length alone, so replicas that hold the same bits keep the same
    bits and nothing new is exchanged under replicated data parallelism."""
    rule = "bertlamb"
    SPLIT_KEYS = ArenaOptimizer.SPLIT_KEYS + ('layer_adaptation',)

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.defaults['layer_adaptation'] = True

    def add_param_group(self, param_group):
        param_group.setdefault('layer_adaptation', True)
        super().add_param_group(param_group)
        self._lamb = None  # (the tensor table carries the groups' flags)

    def load_state_dict(self, state_dict):
        """as BertAdam; a BertAdam checkpoint has no ``layer_adaptation``: the groups keep the flags they have"""
        flags = [pg['layer_adaptation'] for pg in self.param_groups]
        super().load_state_dict(state_dict)
        for pg, f in zip(self.param_groups, flags):
            pg.setdefault('layer_adaptation', f)

    def _check_arena(self, arena):
        if arena.zero1 is not None:
            raise RuntimeError("BertLamb does not run under the sharded update (zero1): a tensor's norm would cross the ranks' "
                               "slices; build the data parallelism without zero1 (the replicated update needs no exchange: "
                               "every rank sums the same bits in the same order)")
        if arena.fp8 is not None:
            raise RuntimeError("BertLamb does not run with the fp8 forward: the e4m3 weight copies are written by BertAdam's "
                               "one-pass update only")

    def _lamb_state(self, arena):
        """the device tensor table {elem0, n, adapted}, the ratio table and the scratch of ``ops.lamb_multi``: built and
        uploaded outside of captures, the table again when a ``layer_adaptation`` flag has changed"""
        owned = {}
        for pg in self.param_groups:
            for p in pg['params']:
                xg = getattr(p, "_xg", None)
                if xg is not None and xg[0] is arena:
                    owned[xg[5]] = bool(pg['layer_adaptation'])
        st = getattr(self, "_lamb", None)
        if st is None or st['arena'] is not arena or st['owned'] != owned:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("BertLamb.step is being captured before any eager step, or a layer_adaptation flag changed "
                                   "during graph capture: run one pass eagerly first (the tensor table is uploaded to the device "
                                   "outside of captures)")
            from ..arena import lamb_tensor_table
            table, names = lamb_tensor_table(arena.info, owned, arena.total)
            if st is not None and st['arena'] is arena:  # captured graphs keep pointing at the same buffers
                st['tensors'].copy_(torch.from_numpy(table))
                st['owned'] = owned
            else:
                st = self._lamb = dict(arena=arena, owned=owned, names=names, tensors=torch.from_numpy(table).to(arena.device),
                                       ratios=torch.ones(len(names), device=arena.device),
                                       ws=ops.lamb_workspace(arena.total, len(names), arena.device))
        return st

    def _launch(self, arena, jobs, hyper_map=None):
        if not jobs:
            return
        st = self._lamb_state(arena)
        spans = sorted(jobs, key=lambda j: j[1]['elem0'])  # arena order
        ops.lamb_multi([(a, kw, {}) for a, kw, _, _ in spans], st['tensors'], st['ratios'], st['ws'], hyper_map)

    def trust_ratios(self):
        """{parameter name: trust ratio} of the last step that updated the parameter (1.0 before its first), for the
        parameters this optimiser holds: ONE read of the device table"""
        st = getattr(self, "_lamb", None)
        if st is None:
            return {}
        r = st['ratios'].tolist()
        return {n: r[i] for i, n in enumerate(st['names']) if n in st['owned']}
