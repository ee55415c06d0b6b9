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
    ``torchdset.random_feat()``, a random object of a random datum of the whole data set; a loader can pass a larger pool;
  * an example with several answer keys draws by inverse CDF on one uniform instead of ``np.random.multinomial``: the same
    distribution, not the same stream.

Out of scope here: the matched-sentence swap of src/pretrain/lxmert_data.py:175-190 (string work in the data set;
``is_matched`` arrives with the batch), data-set readers, a pre-training driver loop, and fusing the masking into the
visual-embedding product's input read."""
import numpy as np
import torch

from .. import ops

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
    first and can be captured; a consumer that keeps a result across calls has to copy it."""

    def __init__(self, word_mask_rate=0.15, obj_mask_rate=0.15, vocab_size=30522, mask_id=103, sid_base=SID_BASE, max_labels=4):
        self.word_mask_rate, self.obj_mask_rate = float(word_mask_rate), float(obj_mask_rate)
        self.vocab_size, self.mask_id, self.sid_base, self.max_labels = int(vocab_size), int(mask_id), int(sid_base), int(max_labels)
        self._out = {}

    @classmethod
    def from_args(cls, args, **kw):
        """rates from a flag namespace (``--wordMaskRate`` / ``--objMaskRate``, src/param.py:102-105)"""
        return cls(word_mask_rate=args.word_mask_rate, obj_mask_rate=args.obj_mask_rate, **kw)

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
                 is_matched, label_ids, label_scores, rng, pool=None, draws=None):
        if label_ids.dim() != 2 or label_ids.shape[1] != self.max_labels:
            raise ValueError("DeviceFeatures: label_ids %s, [B, %d] expected (pack_labels(labels, %d))"
                             % (tuple(label_ids.shape), self.max_labels, self.max_labels))
        out = ops.pretrain_corrupt(input_ids, input_mask, feats, is_matched, label_ids, label_scores, self.word_mask_rate,
                                   self.obj_mask_rate, self.vocab_size, self.mask_id, rng=rng, sid_base=self.sid_base,
                                   pool=pool, draws=draws, out=self._buffers(input_ids, feats))
        visn = {'obj': (obj_labels, obj_confs), 'attr': (attr_labels, attr_confs), 'feat': (feats, out["feat_mask"])}
        return (out["input_ids"], segment_ids, input_mask, out["masked_lm_labels"], out["masked_feat"], boxes, visn,
                is_matched, out["ans"])
