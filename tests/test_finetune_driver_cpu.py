"""Host side of the fine-tuning drivers (``vqa.vqacpv2.VQA``, ``gqa.gqa_ood.GQA``): the validation schedule, the group ids and
the store's group / question-id tables, the reference's log lines and the refusal of a data-parallel model.  No kernel runs
here."""
import numpy as np
import pytest

from test_resident_cpu import _store, _ts


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 7, 100])
def test_validation_schedule_is_the_references_linspace(n):
    from xggm_amd.vqa.vqacpv2 import val_schedule
    want = np.linspace(0, n, 5, dtype=int)[1:-1]  # src/vqa/vqacpv2.py:157 (np.int is gone from numpy)
    got = val_schedule(n)
    assert len(got) == 3 and got.tolist() == want.tolist()
    assert got.tolist() == [int(n * k / 4) for k in (1, 2, 3)]


def test_group_ids_by_field_and_by_callable():
    from xggm_amd.tools.resident import group_ids
    data = [dict(question_id=q, answer_type=t) for q, t in enumerate(["yes/no", "other", "number", "other", "yes/no", "other"])]
    ids, names = group_ids(data, "answer_type")
    assert names == ["number", "other", "yes/no"] and ids.dtype == np.int32 and ids.tolist() == [2, 1, 0, 1, 2, 1]
    ids2, names2 = group_ids(data[::-1], "answer_type")  # sorted names: the ids do not depend on the order of the data
    assert names2 == names and ids2.tolist() == ids.tolist()[::-1]
    head, tail = {0, 3}, {4}
    ids, names = group_ids(data, lambda d: "head" if d["question_id"] in head else "tail" if d["question_id"] in tail else "neither")
    assert names == ["head", "neither", "tail"] and ids.tolist() == [0, 1, 1, 0, 2, 1]


def test_store_groups_question_index_and_keep_mask(tmp_path):
    """``ResidentDataset(groups=)`` uploads ``q_group`` (int32) and keeps the names; bad ids are refused; ``qid_index`` gives
    equal ints to equal question ids (GQA: a datum per label, string ids) and ``keep_mask`` marks their last visit"""
    from xggm_amd.tools.resident import group_ids
    ts = _ts(tmp_path, "gqa")
    pair = group_ids(ts.data, lambda d: "long" if len(d["sent"].split()) > 6 else "short")
    store = _store(ts, groups=pair)
    assert store.G == len(pair[1]) and store.group_names == pair[1]
    assert store.tables["q_group"].dtype.is_floating_point is False and store.tables["q_group"].tolist() == pair[0].tolist()
    assert store.host["q_group"].dtype == np.int32
    plain = _store(ts)
    assert "q_group" not in plain.tables and plain.G == 0
    named = _store(ts, groups=pair[0], group_names=["a", "b"])
    assert named.group_names == ["a", "b"]
    for bad in (np.full(len(ts), 16), np.full(len(ts), -1), np.zeros(len(ts) - 1, dtype=int)):
        with pytest.raises(ValueError, match="group"):
            _store(ts, groups=bad)
    qids = store.ques_ids(np.arange(len(store)))
    assert len(set(qids)) < len(qids) and isinstance(qids[0], str)
    idx = store.qid_index
    assert idx.dtype == np.int64 and len(idx) == len(qids)
    assert all((idx[i] == idx[j]) == (qids[i] == qids[j]) for i in range(len(qids)) for j in range(len(qids)))
    last = {}
    for pos, q in enumerate(qids):
        last[q] = pos
    keep = store.keep_mask()
    assert keep.dtype.is_floating_point is False and sorted(np.nonzero(keep.numpy())[0].tolist()) == sorted(last.values())
    assert store.keep_mask() is keep  # computed once
    order = np.random.default_rng(0).permutation(len(qids))[:7]
    last = {}
    for pos, s in enumerate(order):
        last[qids[s]] = pos
    assert sorted(np.nonzero(store.keep_mask(order).numpy())[0].tolist()) == sorted(last.values())


def test_log_lines_are_the_references():
    """character for character: src/vqa/vqacpv2.py:286-305 and src/gqa/gqa_ood.py:353-369 (the GQA twin has no blank line in
    front of its Valid line)"""
    from xggm_amd.gqa.gqa_ood import GQA
    from xggm_amd.vqa.vqacpv2 import VQA
    epoch, train_score, valid_score, best_valid = 3, 61.23456, 0.56789, 0.6
    assert VQA._epoch_lines(None, epoch, train_score, None, best_valid) == "\nEpoch 3: Train 61.23\n"
    assert VQA._epoch_lines(None, epoch, train_score, valid_score, best_valid) == \
        "\nEpoch 3: Train 61.23\n\nEpoch 3: Valid 56.79\nEpoch 3: Best 60.00\n"
    assert GQA._epoch_lines(None, epoch, train_score, None, best_valid) == "\nEpoch 3: Train 61.23\n"
    assert GQA._epoch_lines(None, epoch, train_score, valid_score, best_valid) == \
        "\nEpoch 3: Train 61.23\nEpoch 3: Valid 56.79\nEpoch 3: Best 60.00\n"
    assert VQA._total_iters_line(None, 12) == "BertAdam Total Iters: 12\n" + "*" * 80
    assert GQA._total_iters_line(None, 12) == "Total Iters: 12"
    assert VQA.order == "vqa" and GQA.order == "gqa" and GQA.valid_factor == 2 and len(GQA.extra_tags) == 6


@pytest.mark.parametrize("kind", ["VQA", "GQA"])
def test_data_parallel_models_are_refused(kind):
    """before anything is built: the ranks would need their own epoch orders and their scores would need combining"""
    from xggm_amd.gqa.gqa_ood import GQA
    from xggm_amd.vqa.vqacpv2 import VQA

    class Model:
        _grad_sync = object()

    with pytest.raises(NotImplementedError, match="enable_data_parallel"):
        {"VQA": VQA, "GQA": GQA}[kind](Model(), (None, None, None))
