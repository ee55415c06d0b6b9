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


def to_quesid2ans(ques_ids, labels, label2ans):
    """the reference's ``{question_id: answer}`` dict (src/vqa/vqacpv2.py:333-337) from the question ids kept on the host
    in call order and the labels read back from the log.  A length mismatch is refused: ids and labels would pair up
    wrongly from the first missing one on."""
    ids = [q.item() if hasattr(q, "item") else q for q in ques_ids]
    labels = labels.tolist() if hasattr(labels, "tolist") else list(labels)
    if len(ids) != len(labels):
        raise ValueError("to_quesid2ans: %d question ids, %d labels" % (len(ids), len(labels)))
    return {q: label2ans[l] for q, l in zip(ids, labels)}
