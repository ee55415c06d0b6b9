"""The ensemble ("debias") answer losses of the language-prior benchmarks, behind the reference's class names
(src/module/vqa_debias_loss_functions.py:29-207): ``Plain``, ``ReweightByInvBias``, ``BiasProduct``, ``LearnedMixin``.
Constructor signatures and defaults, ``to_json()`` and the ``state_dict`` keys (``bias_lin.weight``, ``bias_lin.bias``,
``smooth_param``) are the reference's; the arithmetic is one fused HIP forward and one fused backward
(``functional.DebiasFn`` / xggm_debias_* in xggm.h), ``Plain`` is the existing ``BCEFn`` with ``scale = A``.
``Focal`` (:74-81) needs row softmaxes, a different kernel family: it lives beside cross-entropy in ``module.answer_losses``
(a ``DebiasLossFn`` like the classes here, attached the same way).

``forward(hidden, logits, bias, labels, *, bias_index=None, slot=None)`` keeps the reference's four positional
arguments.  ``bias_index`` (int64 [B]): row of ``bias`` per sample -- ``bias`` is then a small [groups, A] prior table
(``vqa.vqacpv2.answer_prior_table``) and never exists as [B, A]; ``bias=None`` takes the module's ``bias_table`` buffer
(``set_bias_table``).  ``slot``: a zeroed accumulator of the running pass (``Runtime.scalar_slot``).

Every loss is at the scale of ``BCEWithLogits(mean) * A``: in a training pass it REPLACES ``bce_loss(logit, target,
scale=A)`` (``vqa.vqacpv2.attach_debias_loss``)."""
import inspect
from collections import OrderedDict

import numpy as np
import torch
from torch import nn

from .. import functional as XF
from .. import ops


class DebiasLossFn(nn.Module):
    """General API of the loss functions (src/module/vqa_debias_loss_functions.py:29-64)"""

    kind = None          # ops.DEBIAS_* of the fused kernel; None: not one of its kinds
    needs_bias = True    # the passes hand ``bias`` / ``bias_index`` of the batch to it
    needs_hidden = False

    def forward(self, hidden, logits, bias, labels, *, bias_index=None, slot=None):
        """hidden [B, Hd] (compute dtype), logits [B, A] fp32, bias [B, A] (or [groups, A] with ``bias_index``) in
        [0, 1], labels [B, A] soft scores -> 0-dim loss"""
        raise NotImplementedError()

    def set_bias_table(self, table):
        """register the [groups, A] prior table that ``bias_index`` selects rows of (a buffer: it moves with the module
        and is saved with it)"""
        table = torch.as_tensor(table, dtype=torch.float32)
        if table.dim() != 2:
            raise ValueError("bias_table must be [groups, A], got %s" % (tuple(table.shape),))
        if "bias_table" in self._buffers:
            table = table.to(self._buffers["bias_table"].device)
            self._buffers["bias_table"] = table.contiguous()
        else:
            p = next(self.parameters(), None)
            self.register_buffer("bias_table", table.to(p.device).contiguous() if p is not None else table.contiguous())
        return self

    def _bias(self, bias, bias_index):
        if bias is None:
            bias = getattr(self, "bias_table", None)
            if bias is None or bias_index is None:
                raise ValueError("%s: no bias given (pass bias [B, A], or bias_index with set_bias_table)" % type(self).__name__)
        return bias.float()

    def _fused(self, hidden, logits, bias, labels, bias_index, slot, lin=None, w=0.0):
        sp = getattr(self, "smooth_param", None)
        return XF.DebiasFn.apply(self.kind, logits.float(), labels.float(), self._bias(bias, bias_index), bias_index,
                                 hidden if lin is not None else None, None if lin is None else lin.weight,
                                 None if lin is None else lin.bias, sp, float(getattr(self, "constant_smooth", 0.0)), float(w),
                                 slot)

    def to_json(self):
        """a json representation: the class name and the __init__ arguments (the reference's, :44-64; keyword-only
        additions of this package are not part of it)"""
        cls = self.__class__
        out = OrderedDict()
        out["name"] = cls.__name__
        if cls.__init__ is nn.Module.__init__:
            return out  # no init args
        for name, p in inspect.signature(cls.__init__).parameters.items():
            if p.kind in (p.VAR_POSITIONAL, p.VAR_KEYWORD):
                raise NotImplementedError("varargs / keywords not supported")
            if name != "self" and p.kind != p.KEYWORD_ONLY:
                out[name] = getattr(self, name)
        return out


class Plain(DebiasLossFn):
    """F.binary_cross_entropy_with_logits(logits, labels) * A  (:67-71): the package's own head loss, bit for bit"""
    needs_bias = False

    def forward(self, hidden, logits, bias, labels, *, bias_index=None, slot=None):
        return XF.BCEFn.apply(logits.float(), labels.float(), labels.size(1), slot)


class ReweightByInvBias(DebiasLossFn):
    """sum (1 - bias) * bce_elem / sum (1 - bias)  (:84-93)"""
    kind = ops.DEBIAS_REWEIGHT

    def forward(self, hidden, logits, bias, labels, *, bias_index=None, slot=None):
        return self._fused(hidden, logits, bias, labels, bias_index, slot)


def _smooth_parameter(smooth_init):
    return torch.nn.Parameter(torch.from_numpy(np.full((1,), smooth_init, dtype=np.float32)))


class BiasProduct(DebiasLossFn):
    kind = ops.DEBIAS_BIAS_PRODUCT

    def __init__(self, smooth=True, smooth_init=-1, constant_smooth=0.0):
        """
        :param smooth: Add a learned sigmoid(a) factor to the bias to smooth it
        :param smooth_init: How to initialize `a`
        :param constant_smooth: Constant to add to the bias to smooth it
        """
        super(BiasProduct, self).__init__()
        self.constant_smooth = constant_smooth
        self.smooth_init = smooth_init
        self.smooth = smooth
        self.smooth_param = _smooth_parameter(smooth_init) if smooth else None

    def forward(self, hidden, logits, bias, labels, *, bias_index=None, slot=None):
        return self._fused(hidden, logits, bias, labels, bias_index, slot)


class LearnedMixin(DebiasLossFn):
    kind = ops.DEBIAS_LEARNED_MIXIN
    needs_hidden = True

    def __init__(self, w, smooth=True, smooth_init=-1, constant_smooth=0.0, *, hidden_dim=1024):
        """
        :param w: Weight of the entropy penalty
        :param smooth: Add a learned sigmoid(a) factor to the bias to smooth it
        :param smooth_init: How to initialize `a`
        :param constant_smooth: Constant to add to the bias to smooth it
        :param hidden_dim: width of ``hidden`` (the reference hard-codes 1024, :153; LXMERT's logit_fc input is 768)
        """
        super(LearnedMixin, self).__init__()
        self.w = w
        self.smooth_init = smooth_init
        self.constant_smooth = constant_smooth
        self.bias_lin = torch.nn.Linear(hidden_dim, 1)
        self.smooth = smooth
        self.smooth_param = _smooth_parameter(smooth_init) if smooth else None

    def forward(self, hidden, logits, bias, labels, *, bias_index=None, slot=None):
        if hidden is None or hidden.shape[-1] != self.bias_lin.in_features:
            raise ValueError("LearnedMixin(hidden_dim=%d) got hidden %s" % (self.bias_lin.in_features,
                                                                          None if hidden is None else tuple(hidden.shape)))
        return self._fused(hidden, logits, bias, labels, bias_index, slot, lin=self.bias_lin, w=self.w)
