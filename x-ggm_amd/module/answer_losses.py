"""Answer-head losses with a softmax over the answers.  They attach like the debias family
(``vqa.vqacpv2.attach_debias_loss``) and share one fused HIP forward and one backward (``functional.SoftmaxLossFn`` /
xggm_softmax_loss_* in xggm.h).

``Focal``: the fifth class of the reference's src/module/vqa_debias_loss_functions.py (:74-81), under its name, with its
(empty) constructor, ``to_json()`` and ``state_dict``.  It is defined here, next to the kernel family it runs on, and not
in ``module.vqa_debias_loss_functions``, whose classes all run the xggm_debias_* kernels.

``CrossEntropy``: the ``nn.CrossEntropyLoss(ignore_index=-1)`` the reference constructs for ``--mceLoss`` (src/param.py:78,
src/gqa/gqa_ood.py:116) -- GQA has one answer per question -- instead of framework kernels inside a pass.

``labels``: the loaders' ``target`` ([B, A] soft scores: the class of a row is the FIRST index of its maximum, torch's
``max(1)``; a row whose maximum is <= 0 -- an answer outside the vocabulary -- gets ``ignore_index``), or [B] int64
classes.  The loss is the mean over the rows that are not ignored, times ``scale``; ignored rows get an exactly zero
gradient.  With no valid row the loss is NaN and the gradient all zero, as torch's.
The reference only constructs this loss and fixes no weight for it: ``scale`` is an argument (default 1.0)."""
from .. import functional as XF
from .. import ops
from .vqa_debias_loss_functions import DebiasLossFn


class Focal(DebiasLossFn):
    """BCEWithLogits(log(softmax(logits) + 1e-5) * (1 - softmax(bias))^2, labels) * A  (:74-81); the softmaxes run over the
    answers.  No constructor arguments, no parameters; ``bias`` / ``bias_index`` / ``set_bias_table`` as for the family."""
    kind = ops.SOFTMAX_FOCAL

    def forward(self, hidden, logits, bias, labels, *, bias_index=None, slot=None):
        return XF.SoftmaxLossFn.apply(self.kind, logits.float(), labels.float(), self._bias(bias, bias_index), bias_index,
                                      -1, 1.0, slot)


class CrossEntropy(DebiasLossFn):
    kind = ops.SOFTMAX_CE
    needs_bias = False
    needs_hidden = False

    def __init__(self, ignore_index=-1, scale=1.0):
        """
        :param ignore_index: label of the rows that do not count
        :param scale: constant factor on the mean (folded into the kernel and its backward)
        """
        super(CrossEntropy, self).__init__()
        self.ignore_index = int(ignore_index)
        self.scale = float(scale)

    def forward(self, hidden, logits, bias, labels, *, bias_index=None, slot=None):
        if labels.dim() == 2:
            labels = labels.float()
        return XF.SoftmaxLossFn.apply(self.kind, logits.float(), labels, None, None, self.ignore_index, self.scale, slot)
