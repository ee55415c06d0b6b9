"""The masked-LM loss of LXMERT pre-training on the device, from the language stream's rows to the gradients of the tied
word table (``BertLMPredictionHead.decoder`` + ``CrossEntropyLoss(ignore_index=-1)``, src/lxrt/modeling.py:642-659,
:1009-1016).

Only the rows whose label counts (about 15 %) reach the decoder: ``ops.mlm_select`` compacts them into ``cap`` slots on the
device, the decoder's product, the loss and all three backward products then run over ``cap`` rows of 30522 logits
instead of B T.  ``cap`` is ``mlm_capacity``: None = every row (can never overflow), an int = a fixed number of slots; more
labelled rows than slots set the device flag ``overflow`` and make the loss NaN -- never a silent truncation.

The word table receives its decoder gradient HERE (``accumulate`` says whether the embedding's contribution is already in
the buffer); the order a trainer must keep is written down at ``mlm_decoder_bwd``.
"""
import torch

from . import ops

F32 = torch.float32


class MlmDecoderState:
    """what ``mlm_decoder_fwd`` keeps for ``mlm_decoder_bwd``"""

    def __init__(self, sel, t, w, logits, problem):
        self.sel, self.t, self.w, self.logits, self.problem = sel, t, w, logits, problem


def mlm_capacity(M, capacity=None):
    """slots of the compacted list for ``M`` = B T rows: all of them, or the caller's fixed number.  The number is not
    rounded up to a granule of the weight-gradient product (whose reduction runs over the slots): the GEMMs mask a partial
    last K step themselves -- 5 slots give the bits of 24 in tests/test_pretrain_gpu.py -- and rounding here would make
    "one slot too few" mean something else than the caller wrote.  Capacities that matter for speed (ceil(0.25 B T) at
    batch 32 / 256: 160 / 1280) are multiples of 32 anyway."""
    cap = int(M) if capacity is None else int(capacity)
    if cap <= 0:
        raise ValueError("mlm_capacity must be positive, got %r" % (capacity,))
    return min(cap, int(M))


def mlm_decoder_fwd(sel, t, w, bias, out=None):
    """``sel``: the ``ops.MlmSelection`` of this batch; ``t`` [cap, H]: the transformed selected rows (compute dtype; rows
    behind ``sel.n`` may hold anything finite: their logits are never read); ``w`` [V, H]: the word table as the products
    read it (compute dtype); ``bias`` [V] fp32.  -> (0-dim loss, MlmDecoderState).  Logits live in the compute dtype in a
    [cap, ld] buffer whose rows start 16-byte aligned: cap * ld elements instead of B T * V floats."""
    cap, H = t.shape
    V = w.shape[0]
    if cap != sel.cap or w.shape[1] != H or w.dtype != t.dtype or not w.is_contiguous() or not t.is_contiguous():
        raise RuntimeError("mlm_decoder_fwd: rows %s, table %s/%s do not fit a selection of %d slots"
                           % (tuple(t.shape), tuple(w.shape), w.dtype, sel.cap))
    ops._c(bias, F32, "cls.predictions.bias")
    assert bias.numel() == V
    ld = ops.vocab_ld(V, t.dtype)
    buf = torch.empty((cap, ld), device=t.device, dtype=t.dtype)  # columns [V, ld): never read as values, zeroed by the backward
    ops.gemm_raw(t.dtype, t, w, buf, cap, V, H, H, 1, H, 1, ld, bias=bias)
    loss, pr = ops.vocab_ce_fwd(buf, sel.label, sel.n, V, overflow=sel.overflow, out=out)
    return loss, MlmDecoderState(sel, t, w, buf, pr)


def mlm_decoder_bwd(st, gout, g_table, accumulate, g_bias):
    """backward of ``mlm_decoder_fwd``: -> d_t [cap, H] (zero rows behind n).  The logits buffer is overwritten by their
    gradient (no second [cap, ld] tensor).  ``g_table`` [V, H] fp32 gets the decoder's weight gradient d_z^T t --
    OVERWRITTEN when ``accumulate`` is False, added otherwise; ``g_bias`` [V] fp32 is added to (a cleared vector gradient).

    Order of the two contributions to the tied table, fixed: the decoder's weight gradient is written FIRST (the heads'
    backward runs before the encoder's, accumulate=False on a table whose .grad is None), the embedding backward then ADDS
    its rows (``ParamArena.target`` semantics: a parameter that already has a gradient gets the new one added).  The
    row-sparse bookkeeping of the table's gradient does not hold for a dense decoder gradient: a model that trains this
    head sets ``arena.row_list_enabled = False``."""
    V = st.w.shape[0]
    dz = ops.vocab_ce_bwd(st.problem, gout)[:, :V]
    d_t = ops.linear_dgrad(dz, st.w)
    ops.linear_wgrad(dz, st.t, g_table, accumulate)
    ops.colsum(dz, g_bias)
    return d_t
