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
