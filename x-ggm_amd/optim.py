"""``torch.optim``'s Adam, AdamW, Adamax, SGD and RMSprop -- the classes the reference's ``--optim`` flag binds
(src/param.py:9-31) and ``args.optimizer(self.model.parameters(), args.lr)`` builds (src/vqa/vqacpv2.py:141) -- on this
package's fused device update.

A ``torch.optim`` class handed ``model.parameters()`` of an arena-managed model updates the fp32 masters and nothing
else: the bf16 weights every product reads are written by the fused update only, and so is the clip scale applied.  The
classes here keep torch's constructor signatures, defaults, single-tensor arithmetic and ``state_dict`` layout, and run
as ONE launch per pass over the arena (``ops.optim_multi``): clip scale, rule, bf16 shadow.  State lives in ``arena.m`` /
``arena.v``; the step counter of a group lives on the device, and the bias corrections ``1 - beta^t`` are computed from
it once per step in double by the launch that advances it (``ops.sched_step_ex``) -- graph replayable, and as exact as
torch's Python floats.

Groups that received no gradient in a pass are not touched (no decay, no momentum, no step count): torch's
``grad is None`` skip.  ``split_groups=True`` (every constructor) honours param_groups that cut through an arena group --
a no-decay group for biases and LayerNorm, layer-wise learning rates, parameters left out: lr and weight_decay are then
read per tensor from a device map by the same single launch (``ArenaOptimizer._hyper_of_group``).  The sharded update (ZeRO-1) and the fp8 forward are BertAdam's."""
import torch

from . import ops
from .lxrt.optimization import ArenaOptimizer

__all__ = ["Adam", "AdamW", "Adamax", "SGD", "RMSprop"]


def _refuse(cls, **flags):
    """flags of the torch signature that select another implementation or another rule: only their defaults are accepted"""
    for k, (v, ok) in flags.items():
        if v not in ok:
            raise ValueError("xggm_amd.optim.%s: %s=%r is not supported (the fused device update implements torch's "
                             "default single-tensor rule; accepted: %s)" % (cls, k, v, " / ".join(repr(o) for o in ok)))


class _TorchRule(ArenaOptimizer):
    _m_name = _v_name = None  # torch's names of the buffers kept in arena.m / arena.v
    _has_step = True     # torch keeps state['step'] for this rule

    def _check_arena(self, arena):
        if arena.zero1 is not None or arena.fp8 is not None:
            raise RuntimeError("xggm_amd.optim.%s does not run under %s; BertAdam (xggm_amd.lxrt.optimization) is the "
                               "supported optimiser there" % (self._name, "the sharded update (zero1)"
                                                              if arena.zero1 is not None else "the fp8 forward"))

    def _betas(self, pg):
        return 0.0, 0.0

    def _rule_args(self, pg):
        return {}

    def _names(self, pg):
        """(name of the arena.m buffer or None, name of the arena.v buffer or None) for this param_group"""
        return self._m_name, self._v_name

    def _kernel_hyper(self, pg):
        return 0.0, 0.0, pg['eps'] if 'eps' in pg else 0.0, pg['weight_decay']

    def _sched_launch(self, arena, todo):
        ops.sched_step_ex(arena.steps, arena.lr_scale, arena.step_scalars,
                          [(gi, -1, 0.0, 'warmup_linear') + tuple(self._betas(pg)) for _, pg, gi in todo])

    # ---- checkpointing: torch's per-parameter layout, read from / written into the flat arena
    def state_dict(self):
        sd = super().state_dict()
        arena = self._arena()
        if arena is None:
            if getattr(self, "_pending_state", None) is not None:
                sd['state'] = self._pending_state
            return sd
        steps = arena.steps.tolist()
        state, idx = {}, 0
        for pg in self.param_groups:
            mn, vn = self._names(pg)
            for p in pg['params']:
                xg = getattr(p, "_xg", None)
                if xg is not None and xg[0] is arena and (mn or vn):
                    _, o, k, gname = xg[:4]
                    s = steps[arena.group_index[gname]]
                    if s > 0:  # torch has no state for a parameter that has never been stepped
                        st = {}
                        if self._has_step:
                            st['step'] = torch.tensor(float(s))
                        if mn:
                            st[mn] = arena.m[o:o + k].view(p.shape).clone()
                        if vn:
                            st[vn] = arena.v[o:o + k].view(p.shape).clone()
                        state[idx] = st
                idx += 1
        sd['state'] = state
        return sd

    def load_state_dict(self, state_dict):
        """hyper-parameters through torch's loader, buffers and step counters IN PLACE into the arena (captured graphs
        keep pointing at the same buffers).  Before the arena exists the state is kept and applied at the first use."""
        super().load_state_dict({'state': {}, 'param_groups': state_dict['param_groups']})
        self._group_pg = None
        self._pending_state = dict(state_dict.get('state', {}))
        self._arena()

    @torch.no_grad()
    def _state_into_arena(self, arena, state):
        step_of, idx = {}, 0
        have = arena.steps.tolist()
        for pg in self.param_groups:
            mn, vn = self._names(pg)
            for p in pg['params']:
                st = state.get(idx, state.get(str(idx)))
                idx += 1
                xg = getattr(p, "_xg", None)
                if not st or xg is None or xg[0] is not arena:
                    continue
                _, o, k, gname = xg[:4]
                if mn and st.get(mn) is not None:
                    arena.m[o:o + k].view(p.shape).copy_(st[mn])
                if vn and st.get(vn) is not None:
                    arena.v[o:o + k].view(p.shape).copy_(st[vn])
                # (torch's SGD keeps no step: a loaded momentum buffer only means "not the first step")
                s = int(st['step']) if 'step' in st else max(1, have[arena.group_index[gname]])
                if step_of.setdefault(gname, s) != s:
                    raise ValueError("%s.load_state_dict: parameters of arena group '%s' carry different step counts "
                                     "(%d, %d); they always step together here" % (self._name, gname, step_of[gname], s))
        for gname, s in step_of.items():
            arena.steps[arena.group_index[gname]] = s


def _check_common(lr, eps=0.0, weight_decay=0.0):
    if not 0.0 <= lr:
        raise ValueError("Invalid learning rate: {}".format(lr))
    if not 0.0 <= eps:
        raise ValueError("Invalid epsilon value: {}".format(eps))
    if not 0.0 <= weight_decay:
        raise ValueError("Invalid weight_decay value: {}".format(weight_decay))


def _check_betas(betas):
    for i, b in enumerate(betas):
        if not 0.0 <= b < 1.0:
            raise ValueError("Invalid beta parameter at index {}: {}".format(i, b))


class Adam(_TorchRule):
    """torch.optim.Adam (src/param.py:17-19)"""
    rule, _m_name, _v_name = "adam", "exp_avg", "exp_avg_sq"

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *, foreach=None,
                 maximize=False, capturable=False, differentiable=False, fused=None, decoupled_weight_decay=False,
                 split_groups=False):
        _check_common(lr, eps, weight_decay)
        _check_betas(betas)
        _refuse(self._name, amsgrad=(amsgrad, (False,)), foreach=(foreach, (None,)), maximize=(maximize, (False,)),
                capturable=(capturable, (False,)), differentiable=(differentiable, (False,)), fused=(fused, (None,)))
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize,
                        foreach=foreach, capturable=capturable, differentiable=differentiable, fused=fused,
                        decoupled_weight_decay=decoupled_weight_decay)
        self.split_groups = bool(split_groups)
        super().__init__(params, defaults)

    def _betas(self, pg):
        return pg['betas']

    def _rule_args(self, pg):
        return dict(b1=pg['betas'][0], b2=pg['betas'][1])

    def _variant(self, pg):
        # decoupled weight decay is a property of the param_group (torch.optim.AdamW is Adam with it set)
        return ("adamw" if pg.get('decoupled_weight_decay', False) else "adam",)


class AdamW(Adam):
    """torch.optim.AdamW (src/param.py:20-22): Adam with decoupled weight decay, default 0.01"""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, *, maximize=False,
                 foreach=None, capturable=False, differentiable=False, fused=None, split_groups=False):
        super().__init__(params, lr, betas, eps, weight_decay, amsgrad, foreach=foreach, maximize=maximize,
                         capturable=capturable, differentiable=differentiable, fused=fused, decoupled_weight_decay=True,
                         split_groups=split_groups)


class Adamax(_TorchRule):
    """torch.optim.Adamax (src/param.py:23-25)"""
    rule, _m_name, _v_name = "adamax", "exp_avg", "exp_inf"

    def __init__(self, params, lr=2e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, foreach=None, *, maximize=False,
                 differentiable=False, capturable=False, split_groups=False):
        _check_common(lr, eps, weight_decay)
        _check_betas(betas)
        _refuse(self._name, foreach=(foreach, (None,)), maximize=(maximize, (False,)), capturable=(capturable, (False,)),
                differentiable=(differentiable, (False,)))
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, foreach=foreach, maximize=maximize,
                        differentiable=differentiable, capturable=capturable)
        self.split_groups = bool(split_groups)
        super().__init__(params, defaults)

    def _betas(self, pg):
        return pg['betas']

    def _rule_args(self, pg):
        return dict(b1=pg['betas'][0], b2=pg['betas'][1])


class SGD(_TorchRule):
    """torch.optim.SGD (src/param.py:26-28)"""
    rule, _m_name, _v_name, _has_step = "sgd", "momentum_buffer", None, False

    def __init__(self, params, lr=1e-3, momentum=0, dampening=0, weight_decay=0, nesterov=False, *, maximize=False,
                 foreach=None, differentiable=False, fused=None, split_groups=False):
        _check_common(lr, 0.0, weight_decay)
        if momentum < 0.0:
            raise ValueError("Invalid momentum value: {}".format(momentum))
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        _refuse(self._name, foreach=(foreach, (None,)), maximize=(maximize, (False,)), differentiable=(differentiable, (False,)),
                fused=(fused, (None,)))
        defaults = dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov,
                        maximize=maximize, foreach=foreach, differentiable=differentiable, fused=fused)
        self.split_groups = bool(split_groups)
        super().__init__(params, defaults)

    def _names(self, pg):
        return ("momentum_buffer" if pg['momentum'] != 0 else None), None

    def _rule_args(self, pg):
        return dict(momentum=pg['momentum'], dampening=pg['dampening'], nesterov=pg['nesterov'])

    def _variant(self, pg):
        return self.rule, pg['momentum'] == 0  # with momentum 0 the kernel has no buffer: its own instantiation and launch


class RMSprop(_TorchRule):
    """torch.optim.RMSprop (src/param.py:14-16)"""
    rule, _m_name, _v_name = "rmsprop", "momentum_buffer", "square_avg"

    def __init__(self, params, lr=1e-2, alpha=0.99, eps=1e-8, weight_decay=0, momentum=0, centered=False, capturable=False,
                 foreach=None, maximize=False, differentiable=False, split_groups=False):
        _check_common(lr, eps, weight_decay)
        if momentum < 0.0:
            raise ValueError("Invalid momentum value: {}".format(momentum))
        if not 0.0 <= alpha:
            raise ValueError("Invalid alpha value: {}".format(alpha))
        _refuse(self._name, centered=(centered, (False,)), capturable=(capturable, (False,)), foreach=(foreach, (None,)),
                maximize=(maximize, (False,)), differentiable=(differentiable, (False,)))
        defaults = dict(lr=lr, momentum=momentum, alpha=alpha, eps=eps, centered=centered, weight_decay=weight_decay,
                        capturable=capturable, foreach=foreach, maximize=maximize, differentiable=differentiable)
        self.split_groups = bool(split_groups)
        super().__init__(params, defaults)

    def _names(self, pg):
        return ("momentum_buffer" if pg['momentum'] > 0 else None), "square_avg"

    def _rule_args(self, pg):
        return dict(momentum=pg['momentum'], alpha=pg['alpha'])

    def _variant(self, pg):
        return self.rule, pg['momentum'] == 0
