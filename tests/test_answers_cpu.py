"""Host side of the device-resident answer log (xggm_answer_pick_f32, engine.AnswerLog): the boundary and the pure
helpers.  No kernel runs here."""
import ctypes
import json
import os
import re

import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_entry_point_is_exported_and_declared():
    from xggm_amd import _lib
    assert "xggm_answer_pick_f32" in _lib.parse_header()
    assert hasattr(_lib.lib, "xggm_answer_pick_f32")
    src = open(_lib.HEADER_PATH).read()
    # the reference lines the log replaces
    for cite in ("src/vqa/vqacpv2.py:180-181", "src/vqa/vqacpv2.py:333-334", "src/vqa/vqacpv2_data.py:134-142",
                 "src/gqa/gqa_ood.py:379-403"):
        assert cite in src, cite
    # the descriptor of the header and its ctypes mirror name the same fields in the same order
    from xggm_amd import ops
    m = re.search(r"typedef struct xggm_answer_log \{(.*?)\} xggm_answer_log;", src, flags=re.S)
    body = re.sub(r"/\*.*?\*/", " ", m.group(1), flags=re.S)
    fields = [f.split()[-1].lstrip("*") for f in body.split(";") if f.strip()]
    assert fields == [n for n, _ in ops.AnswerLogDesc._fields_]


def test_bad_arguments_are_refused_before_any_launch():
    """null pointers, empty shapes, a row stride below A, a target without scores: an error code and a message, and
    nothing is enqueued (the pointers below are never dereferenced: no GPU is needed to be refused)"""
    from xggm_amd import _lib, ops
    L = _lib.lib
    fake = 0x1000  # aligned, never touched
    d = ops.AnswerLogDesc()
    d.labels, d.scores, d.cursor, d.score_sum, d.flags, d.capacity = fake, fake, fake, fake, fake, 8
    D = ctypes.addressof(d)

    def refused(*args):
        rc = L.xggm_answer_pick_f32(*args)
        assert rc != 0 and b"xggm_answer_pick_f32" in L.xggm_last_error(), args
        return L.xggm_last_error()

    refused(None, 8, None, 0, 2, 8, None, D, fake, None)  # logits
    refused(fake, 8, None, 0, 2, 8, None, None, fake, None)  # log
    refused(fake, 8, None, 0, 2, 8, None, D, None, None)  # workspace
    assert b"B = 0" in refused(fake, 8, None, 0, 0, 8, None, D, fake, None)
    assert b"A = 0" in refused(fake, 8, None, 0, 2, 0, None, D, fake, None)
    assert b"A = -3" in refused(fake, 8, None, 0, 2, -3, None, D, fake, None)
    assert b"row_stride" in refused(fake, 7, None, 0, 2, 8, None, D, fake, None)
    assert b"target_stride" in refused(fake, 8, fake, 7, 2, 8, None, D, fake, None)
    for field in ("labels", "cursor", "flags"):
        e = ops.AnswerLogDesc.from_buffer_copy(d)
        setattr(e, field, None)
        refused(fake, 8, None, 0, 2, 8, None, ctypes.addressof(e), fake, None)
    e = ops.AnswerLogDesc.from_buffer_copy(d)
    e.scores = None
    assert b"scores" in refused(fake, 8, fake, 8, 2, 8, None, ctypes.addressof(e), fake, None)
    e = ops.AnswerLogDesc.from_buffer_copy(d)
    e.labels = fake + 4
    assert b"aligned" in refused(fake, 8, None, 0, 2, 8, None, ctypes.addressof(e), fake, None)


def test_wrapper_rejects_cpu_tensors_and_mismatched_targets():
    from xggm_amd import ops

    class Log:
        capacity = 4
        labels, cursor = torch.zeros(4, dtype=torch.int64), torch.zeros(1, dtype=torch.int64)
        scores, score_sum, flags = None, None, torch.zeros(1, dtype=torch.int32)

    with pytest.raises(RuntimeError, match="GPU"):
        ops.answer_pick(torch.zeros(2, 3), Log)
    with pytest.raises(RuntimeError, match="GPU"):
        from xggm_amd.engine import AnswerLog
        AnswerLog(4, "cpu")


def test_quesid2ans_on_the_dataset_golden():
    """the reference's ``{question_id: answer}`` dict from ids in call order + labels read back"""
    from xggm_amd.answers import to_quesid2ans
    g = json.load(open(os.path.join(GOLDEN, "dataset.json")))
    label2ans = g["label2ans"]
    ans2label = {a: i for i, a in enumerate(label2ans)}
    qids = [d["question_id"] for d in g["vqa"]]
    labels = torch.tensor([ans2label[g["pred_vqa"][str(q)]] for q in qids])
    want = {q: g["pred_vqa"][str(q)] for q in qids}
    assert to_quesid2ans(qids, labels, label2ans) == want
    # ids as the loader hands them out (tensor elements), labels as a list; GQA's string ids
    assert to_quesid2ans(list(torch.tensor(qids)), labels.tolist(), label2ans) == want
    gq = [d["question_id"] for d in g["gqa"]]
    gl = [ans2label[g["pred_gqa"][q]] for q in gq]
    assert to_quesid2ans(gq, gl, label2ans) == g["pred_gqa"]
    for bad in (labels[:-1], torch.cat([labels, labels[:1]])):
        with pytest.raises(ValueError, match="14 question ids"):
            to_quesid2ans(qids, bad, label2ans)


def test_decode_of_a_read_back_log():
    """the int64 words of ``AnswerLog.read``'s one transfer: [cursor, score sum (fp64 bits), flags, labels, scores];
    an overflowed log raises and says how much was refused"""
    from xggm_amd.answers import decode_packed
    cap = 5
    w = torch.zeros(3 + cap + 3, dtype=torch.int64)
    w[0] = 3
    w[1:2].view(torch.float64)[0] = 1.25
    w[3:3 + cap] = torch.tensor([7, 0, 28, -1, -1])
    w[3 + cap:].view(torch.float32)[:3] = torch.tensor([1.0, 0.0, 0.25])
    labels, scores, total, n = decode_packed(w, cap)
    assert n == 3 and labels.tolist() == [7, 0, 28] and scores.tolist() == [1.0, 0.0, 0.25] and total == 1.25
    assert labels.dtype == torch.int64 and scores.dtype == torch.float32
    labels2, scores2, _, _ = decode_packed(w[:3 + cap], cap, with_scores=False)
    assert labels2.tolist() == [7, 0, 28] and scores2 is None
    w[2:3].view(torch.int32)[0] = 1 + 2 * 2  # overflow bit, two refused appends
    with pytest.raises(RuntimeError, match=r"capacity 5, 3 samples logged, 2 append\(s\) refused"):
        decode_packed(w, cap)
    w[2:3].view(torch.int32)[0] = 0
    w[0] = cap + 1
    with pytest.raises(RuntimeError, match="cursor"):
        decode_packed(w, cap)
