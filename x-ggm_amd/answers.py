"""Host side of the device-resident answer log (``engine.AnswerLog``, ``xggm_answer_pick_f32``): pure Python, importable
without a GPU.  The kernel appends the arg-max of every logit row -- what the reference takes with
``logit.max(1)[1].cpu()`` per batch (src/vqa/vqacpv2.py:180-181, :333-334; src/gqa/gqa_ood.py:379-403) -- to device
buffers; what is here turns ONE read-back of those buffers into the reference's host objects."""

FLAG_OVERFLOW = 1  # bit 0 of the log's flag word: an append did not fit; the bits above it count the refused appends


def check_flags(flags, capacity, count):
    """the flag word of a log read back: raises when an append was refused (the sweep is then incomplete)"""
    flags = int(flags)
    if flags & FLAG_OVERFLOW:
        raise RuntimeError("answer log overflow: capacity %d, %d samples logged, %d append(s) refused -- the log is "
                           "incomplete (size it for the whole sweep, or reset() it in time)"
                           % (int(capacity), int(count), flags >> 1))


def decode_packed(words, capacity, with_scores=True):
    """what ``AnswerLog.read`` does with the int64 words of its ONE transfer: ``words`` = CPU int64 tensor laid out as
    [cursor, score_sum (fp64 bits), flags, labels[0:capacity], scores (fp32 pairs)...] -> (labels [n] int64, scores [n]
    fp32 or None, score_sum float, n).  Raises RuntimeError on the overflow flag."""
    import torch
    n = int(words[0])
    check_flags(int(words[2]), capacity, n)
    if not 0 <= n <= capacity:
        raise RuntimeError("answer log: cursor %d outside [0, %d]" % (n, capacity))
    labels = words[3:3 + n].clone()
    score_sum = float(words[1:2].view(torch.float64)[0])
    scores = words[3 + capacity:].view(torch.float32)[:n].clone() if with_scores else None
    return labels, scores, score_sum, n


FOLD_MAX_RANKS = 64               # XGGM_FOLD_MAX_RANKS (include/xggm.h)
FOLD_CONCAT, FOLD_INTERLEAVE = 0, 1   # XGGM_FOLD_CONCAT, XGGM_FOLD_INTERLEAVE
FOLD_FLAG_CURSOR = 1              # bit 0 of a fold's flag: a rank's cursor is not its expected count
FOLD_FLAG_REFUSED = 2             # bit 1: a rank's log carries refused appends; bits 8..: the lowest offending rank


def packed_words(capacity, with_scores=True):
    """int64 words of a packed answer log: [cursor, score_sum, flags, labels[capacity], scores fp32 two per word]"""
    capacity = int(capacity)
    return 3 + capacity + ((capacity + 1) // 2 if with_scores else 0)


def fold_destinations(layout, expect, block=None):
    """where xggm_answer_log_fold puts the answers: a list over the ranks of int64 arrays, entry p of rank r's = the
    destination index of its position p.  ``FOLD_CONCAT``: rank r's ``expect[r]`` answers behind those of the ranks below it
    (a sweep cut into contiguous slices, ``dist.shard_range``); ``FOLD_INTERLEAVE``: global step s holds ``world`` blocks of
    ``block`` answers, rank r's the r-th -- the inverse of ``perm.reshape(steps, world, B)[:, rank]`` (``ResidentDataset.order``).
    ValueError for what the entry refuses."""
    import numpy as np
    expect = [int(e) for e in expect]
    world = len(expect)
    if not 1 <= world <= FOLD_MAX_RANKS or any(e < 0 for e in expect) or sum(expect) < 1:
        raise ValueError("fold: expect = %s (1 .. %d ranks, counts >= 0, at least one answer)" % (expect, FOLD_MAX_RANKS))
    if layout == FOLD_CONCAT:
        first = np.concatenate([[0], np.cumsum(expect)[:-1]]).astype(np.int64)
        return [first[r] + np.arange(expect[r], dtype=np.int64) for r in range(world)]
    if layout != FOLD_INTERLEAVE:
        raise ValueError("fold: unknown layout %r" % (layout,))
    if block is None or int(block) < 1 or any(e != expect[0] or e % int(block) for e in expect):
        raise ValueError("fold: interleave needs equal counts that are multiples of the block (expect = %s, block = %s)" % (expect, block))
    block = int(block)
    p = np.arange(expect[0], dtype=np.int64)
    return [((p // block) * world + r) * block + p % block for r in range(world)]


def fold_logs_host(bufs, capacity, with_scores, layout, block, expect):
    """xggm_answer_log_fold restated in numpy: ``bufs`` = [world, >= packed_words] int64 (the gathered packed logs, one row
    per rank, ``capacity`` entries each) -> dict: ``labels`` [total] int64, ``scores`` [total] fp32 or None, ``cursor`` = total,
    ``score_sum`` (the ranks' fp64 sums added in rank order to +0.0), ``flags`` = 0, ``flag`` (0, or FOLD_FLAG_* with the lowest
    offending rank from bit 8 on) and ``dest`` (``fold_destinations``).  As the kernel does, it copies ``expect[r]`` positions
    whatever the cursors say.  The CPU-testable reference of the kernel (tested against it bit for bit); no fallback."""
    import numpy as np
    bufs = np.asarray(bufs, dtype=np.int64)
    capacity = int(capacity)
    dest = fold_destinations(layout, expect, block)
    world, total = len(dest), sum(len(d) for d in dest)
    if bufs.ndim != 2 or bufs.shape[0] != world or bufs.shape[1] < packed_words(capacity, with_scores):
        raise ValueError("fold_logs_host: bufs %s for %d ranks of capacity %d" % (bufs.shape, world, capacity))
    if any(len(d) > capacity for d in dest):
        raise ValueError("fold_logs_host: expect = %s exceeds the capacity %d" % ([len(d) for d in dest], capacity))
    labels = np.zeros(total, dtype=np.int64)
    scores = np.zeros(total, dtype=np.float32) if with_scores else None
    score_sum, bits, bad = np.float64(0.0), 0, -1
    for r in range(world):
        row = np.ascontiguousarray(bufs[r])
        n = len(dest[r])
        labels[dest[r]] = row[3:3 + n]
        if with_scores:
            scores[dest[r]] = row[3 + capacity:3 + capacity + (capacity + 1) // 2].view(np.float32)[:n]
        with np.errstate(invalid="ignore", over="ignore"):
            score_sum = score_sum + row[1:2].view(np.float64)[0]
        off = (FOLD_FLAG_CURSOR if int(row[0]) != n else 0) | (FOLD_FLAG_REFUSED if int(row[2]) != 0 else 0)
        bits |= off
        if off and bad < 0:
            bad = r
    return dict(labels=labels, scores=scores, cursor=total, score_sum=float(score_sum), flags=0,
                flag=(bits | (bad << 8)) if bits else 0, dest=dest)


def fold_flag_message(flag):
    """what a non-zero flag of a fold says"""
    flag = int(flag)
    what = [s for bit, s in ((FOLD_FLAG_CURSOR, "a rank has not logged the answers expected of it"),
                             (FOLD_FLAG_REFUSED, "a rank's log refused appends (overflow)")) if flag & bit]
    return "answer log fold: %s; the lowest such rank is %d -- the merged sweep is incomplete" % (" and ".join(what), flag >> 8)


SCORE_CHUNK = 1024       # XGGM_SCORE_CHUNK (include/xggm.h)
SCORE_MAX_GROUPS = 16    # XGGM_SCORE_MAX_GROUPS
SCORE_FLAG_CURSOR = 1    # bit 0 of a score's flag word: the log's cursor was not the n the launch was given
SCORE_FLAG_RANGE = 2     # bit 1: a sample index or a group id was out of range (the position contributed nothing)


def ordered_sum(v):
    """the fp64 sum of xggm_answer_score, in ITS order (written down in xggm.h): chunks of 1024 values padded with +0.0;
    in a chunk lane t adds x[t], x[t + 256], x[t + 512], x[t + 768] to +0.0 in that order, eight halving steps a[:h] + a[h:]
    join the 256 lanes, and the chunk partials are added in chunk order to +0.0"""
    import numpy as np
    v = np.asarray(v, dtype=np.float64).reshape(-1)
    C = -(-len(v) // SCORE_CHUNK)
    x = np.zeros(C * SCORE_CHUNK, dtype=np.float64)
    x[:len(v)] = v
    x = x.reshape(C, 4, SCORE_CHUNK // 4)
    a = (((0.0 + x[:, 0]) + x[:, 1]) + x[:, 2]) + x[:, 3]
    h = a.shape[1] // 2
    while h >= 1:
        a = a[:, :h] + a[:, h:2 * h]
        h //= 2
    total = np.float64(0.0)
    for p in a[:, 0]:
        total = total + p
    return total


def score_host(labels, tables, order=None, keep=None, groups=None, G=0, n_q=None, cursor=None):
    """``ops.answer_score`` (xggm_answer_score) restated in numpy, in the kernel's order of addition: the CPU-testable
    reference of the kernel, NOT a fallback.  ``labels``: [n] ints (an ``AnswerLog``'s); ``tables``: anything with ``q_label``
    [n_q, K] and ``q_score`` [n_q, K] (numpy); ``order``: [n] sample indices or None (position i is sample i); ``keep``: [n]
    0 / 1 or None; ``groups``: [n_q] ids in [0, G) or None; ``n_q``: the number of samples the launch is TOLD of (default:
    the tables' rows); ``cursor``: the log's cursor, compared with n.  -> CPU int64 tensor of 3 + 2 G words [flags, count_all,
    count_g[0..G), sum_all, sum_g[0..G)], the sums as fp64 bit patterns -- ``decode_score`` reads them."""
    import numpy as np
    import torch
    labels = np.asarray(labels, dtype=np.int64).reshape(-1)
    n, G = len(labels), int(G)
    ql, qs = np.asarray(tables["q_label"]), np.asarray(tables["q_score"], dtype=np.float32)
    n_q = ql.shape[0] if n_q is None else int(n_q)
    if n < 1 or ql.ndim != 2 or qs.shape != ql.shape or not 0 <= G <= SCORE_MAX_GROUPS or (groups is None) != (G == 0):
        raise ValueError("score_host: n=%d, q_label %s, q_score %s, G=%d%s" % (n, ql.shape, qs.shape, G, "" if groups is None else " with groups"))
    s = np.arange(n, dtype=np.int64) if order is None else np.asarray(order, dtype=np.int64).reshape(-1)
    w = np.ones(n, dtype=bool) if keep is None else np.asarray(keep).reshape(-1) != 0
    if len(s) != n or len(w) != n:
        raise ValueError("score_host: %d labels, %d order entries, %d keep entries" % (n, len(s), len(w)))
    ok = (s >= 0) & (s < n_q)
    g = np.zeros(n, dtype=np.int64)
    if groups is not None:
        g[ok] = np.asarray(groups, dtype=np.int64).reshape(-1)[s[ok]]
        ok &= (g >= 0) & (g < G)
    cnt = ok & w
    sc = np.zeros(n, dtype=np.float64)
    idx = np.nonzero(cnt)[0]
    if len(idx):
        rows = ql[s[idx]]
        match = (rows == labels[idx][:, None]) & (rows >= 0)
        first = match.argmax(1)  # the FIRST matching slot
        sc[idx] = np.where(match.any(1), qs[s[idx], first].astype(np.float64), 0.0)
    words = np.zeros(3 + 2 * G, dtype=np.int64)
    sums = words[2 + G:].view(np.float64)
    words[0] = (SCORE_FLAG_RANGE if (~ok).any() else 0) | (SCORE_FLAG_CURSOR if cursor is not None and int(cursor) != n else 0)
    words[1], sums[0] = cnt.sum(), ordered_sum(np.where(cnt, sc, 0.0))
    for k in range(G):
        m = cnt & (g == k)
        words[2 + k], sums[1 + k] = m.sum(), ordered_sum(np.where(m, sc, 0.0))
    return torch.from_numpy(words)


def last_occurrence_mask(ids_in_order):
    """[n] uint8: 1 at the LAST position of every distinct question id of ``ids_in_order`` (ints or strings), 0 elsewhere --
    the positions whose answer a dict assignment loop ``quesid2ans[qid] = ans`` over the sweep leaves standing (the
    reference's train and validation loops; ``GQATorchDataset`` repeats a datum once per label, src/gqa/gqa_ood_data.py:88-93)"""
    import numpy as np
    ids = np.asarray(list(ids_in_order))
    keep = np.zeros(len(ids), dtype=np.uint8)
    if len(ids):
        _, first_rev = np.unique(ids[::-1], return_index=True)
        keep[len(ids) - 1 - first_rev] = 1
    return keep


def decode_score(words, G, names=None):
    """the words of ``ops.answer_score`` / ``score_host`` (CPU int64 tensor or array) -> dict: ``score`` = sum_all / count_all
    (what ``evaluator.evaluate`` returns; 0.0 for no sample), ``count``, ``sum``, ``counts`` [G], ``sums`` [G] and ``by_group``
    {name: accuracy} -- ``names[k]`` (default: k) for every group WITH samples; an empty group has no entry.  RuntimeError
    on a flagged result: the numbers would be those of another sweep or of a part of it."""
    import numpy as np
    words = np.asarray(words.numpy() if hasattr(words, "numpy") else words, dtype=np.int64).reshape(-1)
    G = int(G)
    if len(words) != 3 + 2 * G:
        raise ValueError("decode_score: %d words for G=%d (3 + 2 G expected)" % (len(words), G))
    if names is not None and len(names) != G:
        raise ValueError("decode_score: %d names for %d groups" % (len(names), G))
    flags = int(words[0])
    if flags & SCORE_FLAG_CURSOR:
        raise RuntimeError("answer score: the log's cursor is not the number of samples scored -- an append is missing or "
                           "was refused")
    if flags & SCORE_FLAG_RANGE:
        raise RuntimeError("answer score: a sample index or a group id was out of range; the position was left out")
    counts = words[1:2 + G].copy()
    sums = words[2 + G:].copy().view(np.float64)
    by_group = {}
    for k in range(G):
        if counts[1 + k]:
            by_group[names[k] if names is not None else k] = float(sums[1 + k]) / int(counts[1 + k])
    return dict(score=float(sums[0]) / int(counts[0]) if counts[0] else 0.0, count=int(counts[0]), sum=float(sums[0]),
                counts=counts[1:], sums=sums[1:], by_group=by_group)


def to_quesid2ans(ques_ids, labels, label2ans):
    """the reference's ``{question_id: answer}`` dict (src/vqa/vqacpv2.py:333-337) from the question ids kept on the host
    in call order and the labels read back from the log.  A length mismatch is refused: ids and labels would pair up
    wrongly from the first missing one on."""
    ids = [q.item() if hasattr(q, "item") else q for q in ques_ids]
    labels = labels.tolist() if hasattr(labels, "tolist") else list(labels)
    if len(ids) != len(labels):
        raise ValueError("to_quesid2ans: %d question ids, %d labels" % (len(ids), len(labels)))
    return {q: label2ans[l] for q, l in zip(ids, labels)}
