"""Host side of the device-resident training log (``engine.TrainLog``, ``xggm_train_log_append``): pure Python,
importable without a GPU.  The kernel appends one record per optimiser pass -- the scalars the reference reads from the
GPU in every iteration (``total_loss += loss.detach() / logit.size(0)``, src/vqa/vqacpv2.py:179; the tensorboard scalars
of :256-270) -- to a ring on the device; what is here turns ONE read-back of that ring into host tensors."""

COLS = 8   # XGGM_TRAINLOG_COLS
KINDS = 4  # XGGM_TRAINLOG_KINDS
LOSS, BCE, KL, DSM, GRAD_NORM, LR_SCALE = range(6)  # columns of a pass record; 6 and 7 are spare
PLAIN, REL, NODE = 0, 1, 2                          # kinds
KIND_OF = {"plain": PLAIN, "rel": REL, "node": NODE}
# the spare kind: one record per pre-training step (``engine.CapturedPretrainer``).  Column 0 is LOSS as above; columns 1-6
# are the reference's six terms in the order of its LOSSES_NAME (src/pretrain/lxmert_pretrain.py:218), each at a FIXED
# column -- a task that is off leaves its column absent -- and column 7 the pre-clip gradient norm (absent in a validation
# log, which has no backward)
PRETRAIN = 3
LOSSES_NAME = ('Mask_LM', 'Matched', 'Obj', 'Attr', 'Feat', 'QA')
PT_MASK_LM, PT_MATCHED, PT_OBJ, PT_ATTR, PT_FEAT, PT_QA = range(1, 7)
PT_GRAD_NORM = 7
HEADER = 2 + KINDS + KINDS * COLS  # int64 words in front of the ring: cursor, first_bad, counts, sums (fp64 bits)


def words(capacity):
    """int64 words of the one buffer a log of ``capacity`` records lives in:
    [cursor, first_bad, counts[KINDS], sums[KINDS * COLS] (fp64), steps[capacity], values[capacity * COLS] (fp32),
    kinds[capacity] (int32)]"""
    capacity = int(capacity)
    return HEADER + capacity + capacity * COLS // 2 + (capacity + 1) // 2


def unroll(cursor, capacity):
    """row order of the retained records, oldest first: record r lives in row r % capacity and the ring keeps the last
    min(cursor, capacity) records"""
    cursor, capacity = int(cursor), int(capacity)
    if capacity <= 0 or cursor < 0:
        raise ValueError("unroll: cursor %d, capacity %d" % (cursor, capacity))
    return [r % capacity for r in range(max(cursor - capacity, 0), cursor)]


def decode_packed(w, capacity):
    """what ``TrainLog.read`` does with the int64 words of its ONE transfer (layout: ``words``) -> dict of CPU tensors /
    numbers: values [m, COLS] fp32, steps [m] int64, kinds [m] int64 (the kind alone), present [m, COLS] bool, cursor,
    sums [KINDS, COLS] fp64, counts [KINDS] int64, first_bad; the m = min(cursor, capacity) retained records oldest
    first"""
    import torch
    capacity = int(capacity)
    cursor = int(w[0])
    if cursor < 0:
        raise RuntimeError("training log: cursor %d is negative" % cursor)
    o = HEADER
    steps = w[o:o + capacity]
    o += capacity
    values = w[o:o + capacity * COLS // 2].view(torch.float32).view(capacity, COLS)
    o += capacity * COLS // 2
    packed = w[o:].view(torch.int32)[:capacity]
    order = torch.tensor(unroll(cursor, capacity), dtype=torch.int64)
    packed = packed[order].to(torch.int64)
    mask = packed >> 8
    return dict(values=values[order].clone(), steps=steps[order].clone(), kinds=packed & 0xFF,
                present=((mask[:, None] >> torch.arange(COLS)) & 1).bool(), cursor=w[0].clone(),
                sums=w[2 + KINDS:HEADER].view(torch.float64).view(KINDS, COLS).clone(), counts=w[2:2 + KINDS].clone(),
                first_bad=w[1].clone())


def pretrain_means(rec):
    """what the reference prints per epoch (src/pretrain/lxmert_pretrain.py:363-368, :400-404) from ONE decoded read-back
    ``rec`` (``decode_packed`` / ``TrainLog.read``): -> (mean loss, [(name, mean term)] for the terms that were logged, in
    the order of LOSSES_NAME, number of steps).  The means are the log's fp64 running sums of the PRETRAIN records since its
    reset over their count, so they cover every step even when the ring has wrapped; a term counts as logged when the
    newest retained PRETRAIN record holds its column (the set of tasks does not change within a run)."""
    n = int(rec["counts"][PRETRAIN])
    if n == 0:
        return 0.0, [], 0
    rows = (rec["kinds"] == PRETRAIN).nonzero().reshape(-1)
    if rows.numel() == 0:
        raise RuntimeError("pretrain_means: %d pre-training steps were logged but the ring retains none of them" % n)
    present = rec["present"][int(rows[-1])]
    sums = rec["sums"][PRETRAIN]
    terms = [(name, float(sums[c]) / n) for name, c in zip(LOSSES_NAME, range(PT_MASK_LM, PT_QA + 1)) if bool(present[c])]
    return float(sums[LOSS]) / n, terms, n


def fold_host(values, kinds, present, steps=None, cursors=None, cursor=None):
    """xggm_train_log_fold restated in numpy: the data-parallel ranks' copies of the n records of a log -> what the launch
    leaves in a rank's ring.  ``values`` [world, n, COLS] fp32, ``kinds`` [world, n] (the kind alone), ``present`` [world, n,
    COLS] bool, ``steps`` [world, n] int64 or None, ``cursors`` [world] or None, ``cursor``: this rank's (default n).
    -> dict of numpy arrays / numbers: values [n, COLS] fp32 -- per record and column the sum in rank order times the fp32
    1 / world; an absent column 0; ``world == 1``: unchanged --, kinds [n] (rank 0's), present [n, COLS] (on EVERY rank),
    sums [KINDS, COLS] fp64 and counts [KINDS] over the folded records in record order, first_bad, and ``flag``: -1, the
    first record whose kind, present columns or step differ between ranks, or n when only a cursor is not n.  The
    CPU-testable reference of the kernel (tested against it bit for bit); no fallback."""
    import numpy as np
    values = np.asarray(values, dtype=np.float32)
    kinds, present = np.asarray(kinds).astype(np.int64), np.asarray(present).astype(bool)
    world, n = kinds.shape
    if world < 1 or n < 1 or values.shape != (world, n, COLS) or present.shape != (world, n, COLS):
        raise ValueError("fold_host: values %s, kinds %s, present %s" % (values.shape, kinds.shape, present.shape))
    both = present.all(axis=0)
    with np.errstate(invalid="ignore", over="ignore"):
        acc = values[0].copy()
        for r in range(1, world):
            acc = acc + values[r]  # rank order, fp32
        out = acc if world == 1 else np.where(both, acc * (np.float32(1.0) / np.float32(world)), np.float32(0.0))
    out = out.astype(np.float32)
    differ = (kinds != kinds[0]).any(axis=0) | (present != present[0]).any(axis=(0, 2))
    if steps is not None:
        steps = np.asarray(steps).astype(np.int64)
        differ |= (steps != steps[0]).any(axis=0)
    flag = int(np.argmax(differ)) if differ.any() else -1
    if flag < 0 and cursors is not None and any(int(c) != n for c in np.asarray(cursors).reshape(-1)):
        flag = n
    sums, counts = np.zeros((KINDS, COLS), dtype=np.float64), np.zeros(KINDS, dtype=np.int64)
    for i in range(n):  # record order, fp64: what the appends would have accumulated
        k = int(kinds[0, i])
        counts[k] += 1
        for c in range(COLS):
            if both[i, c]:
                sums[k, c] = sums[k, c] + np.float64(out[i, c])
    bad = (~np.isfinite(out) & both).any(axis=1)
    first_bad = (n if cursor is None else int(cursor)) - n + int(np.argmax(bad)) if bad.any() else -1
    return dict(values=out, kinds=kinds[0].copy(), present=both, sums=sums, counts=counts, first_bad=first_bad, flag=flag)
