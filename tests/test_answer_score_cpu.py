"""Host side of the sweep score (xggm_answer_score): its numpy restatement ``answers.score_host`` against the evaluators on the
golden fixture, the keep mask against a literal dict loop, the decoding of the words, the declarations and the refusals the
entry point makes before any launch.  No kernel runs here."""
import ctypes
import os

import numpy as np
import pytest
import torch

from helpers import load_golden
from test_data_cpu import _records
from test_resident_cpu import _store, _ts

TOL = 2.0 ** -24  # one fp32 rounding of a score <= 1: the store holds fp32, the evaluator adds Python doubles


def _fixture(tmp_path, kind):
    from xggm_amd.vqa.vqacpv2_data import VQAEvaluator
    from xggm_amd.gqa.gqa_ood_data import GQAEvaluator
    meta, _ = _records()
    ts = _ts(tmp_path, kind)
    store = _store(ts)
    a2l = ts.raw_dataset.ans2label
    if kind == "vqa":
        pred = {int(k): v for k, v in meta["pred_vqa"].items()}
        ev = VQAEvaluator(ts.raw_dataset)
    else:
        pred = dict(meta["pred_gqa"])
        ev = GQAEvaluator(ts.raw_dataset)
    qids = store.ques_ids(np.arange(len(store)))
    labels = np.asarray([a2l[pred[q]] for q in qids], dtype=np.int64)
    return meta, ts, store, pred, ev, qids, labels


@pytest.mark.parametrize("kind", ["vqa", "gqa"])
def test_score_host_equals_the_evaluators_on_the_golden_fixture(tmp_path, kind):
    """the fixture's predictions scored against the store's own tables == ``evaluator.evaluate`` of the dict == the score the
    reference's evaluator recorded, to within 2^-24; the GQA store repeats a question once per label, so the keep mask is
    what makes the count ``len(quesid2ans)``.  Also over a shuffled order with repeated positions, against the dict a loop
    over that order leaves."""
    from xggm_amd.answers import decode_score, last_occurrence_mask, score_host
    meta, ts, store, pred, ev, qids, labels = _fixture(tmp_path, kind)
    g = load_golden("dataset")
    n = len(store)
    if kind == "gqa":
        assert len(set(qids)) < n  # repeats: without the mask the divisor would be n
    keep = last_occurrence_mask(store.qid_index)
    res = decode_score(score_host(labels, store.host, keep=keep), 0)
    assert res["count"] == len(set(qids)) == len(pred)
    want = ev.evaluate(pred)
    print(kind, "score_host", res["score"], "evaluator", want, "recorded", float(g["score_" + kind]))
    assert abs(res["score"] - want) <= TOL
    assert abs(res["score"] - float(g["score_" + kind])) <= TOL
    # a sweep in another order, samples visited twice with DIFFERENT answers: the last one stands, as in the dict
    rng = np.random.default_rng(3)
    order = rng.integers(0, n, 2 * n)
    l2a = ts.raw_dataset.label2ans
    answers = rng.integers(0, len(l2a), 2 * n)
    answers[::2] = labels[order[::2]]
    d = {}
    for s, a in zip(order, answers):
        d[qids[s]] = l2a[a]
    res = decode_score(score_host(answers, store.host, order=order, keep=last_occurrence_mask(store.qid_index[order])), 0)
    assert res["count"] == len(d) and abs(res["score"] - ev.evaluate(d)) <= TOL


def test_score_host_by_group_and_the_order_of_addition(tmp_path):
    """per-group counts and sums add up to the total's samples; ``ordered_sum`` is the written-down order: lanes of four, a
    halving tree, chunks in sequence -- NOT a left-to-right sum, which differs in the last bits on wide-ranged values"""
    from xggm_amd.answers import decode_score, ordered_sum, score_host
    from xggm_amd.tools.resident import group_ids
    meta, ts, store, pred, ev, qids, labels = _fixture(tmp_path, "vqa")
    ids, names = group_ids(ts.data, lambda d: "q%d" % (d["question_id"] % 3))
    res = decode_score(score_host(labels, store.host, groups=ids, G=len(names)), len(names), names)
    assert int(res["counts"].sum()) == res["count"] == len(store)
    for k, name in enumerate(names):
        sub = {q: pred[q] for q, i in zip(qids, ids) if i == k}
        assert abs(res["by_group"][name] - ev.evaluate(sub)) <= TOL
    rng = np.random.default_rng(0)
    v = (rng.random(3 * 1024 + 17) + 1.0) * 2.0 ** rng.integers(-40, 11, 3 * 1024 + 17)
    v = v.astype(np.float32).astype(np.float64)
    x = np.zeros(4 * 1024)
    x[:len(v)] = v
    want = 0.0
    for c in range(4):  # the header's formula, element by element
        a = [(((0.0 + x[c * 1024 + t]) + x[c * 1024 + t + 256]) + x[c * 1024 + t + 512]) + x[c * 1024 + t + 768] for t in range(256)]
        h = 128
        while h >= 1:
            a = [a[t] + a[t + h] for t in range(h)]
            h //= 2
        want = want + a[0]
    assert float(ordered_sum(v)) == want
    naive = 0.0
    for e in v:
        naive += e
    assert naive != want  # the inputs DO tell the two orders apart


def test_last_occurrence_mask_is_what_a_dict_loop_leaves():
    from xggm_amd.answers import last_occurrence_mask
    rng = np.random.default_rng(1)
    for trial in range(20):
        n = int(rng.integers(1, 60))
        ids = rng.integers(0, max(1, n // 2), n)
        ids = ["q%d" % i for i in ids] if trial % 2 else ids.tolist()
        last = {}
        for pos, q in enumerate(ids):
            last[q] = pos
        want = np.zeros(n, dtype=np.uint8)
        want[list(last.values())] = 1
        got = last_occurrence_mask(ids)
        assert got.dtype == np.uint8 and got.tolist() == want.tolist()
    assert last_occurrence_mask([]).tolist() == []


def test_decode_score_reads_the_words_and_refuses_flagged_ones():
    from xggm_amd.answers import decode_score
    G = 3
    words = np.zeros(3 + 2 * G, dtype=np.int64)
    words[1:2 + G] = (10, 4, 0, 6)
    words[2 + G:] = np.array([6.5, 3.0, 0.0, 3.5]).view(np.int64)
    res = decode_score(torch.from_numpy(words), G, ["number", "other", "yes/no"])
    assert res["score"] == 0.65 and res["count"] == 10 and res["sum"] == 6.5
    assert res["by_group"] == {"number": 0.75, "yes/no": 3.5 / 6}  # the empty group has no entry
    assert decode_score(words, G)["by_group"] == {0: 0.75, 2: 3.5 / 6}
    assert decode_score(np.zeros(3, dtype=np.int64), 0)["score"] == 0.0
    for flag, what in ((1, "cursor"), (2, "out of range"), (3, "cursor")):
        bad = words.copy()
        bad[0] = flag
        with pytest.raises(RuntimeError, match=what):
            decode_score(bad, G)
    with pytest.raises(ValueError):
        decode_score(words, G + 1)
    with pytest.raises(ValueError):
        decode_score(words, G, ["a"])


def test_header_makefile_and_bindings_know_the_new_entry_points():
    from xggm_amd import _lib
    decl = _lib.parse_header()
    assert "xggm_answer_score" in decl and "xggm_answer_score_workspace_bytes" in decl
    assert len(decl["xggm_answer_score"]) == 15 and decl["xggm_answer_score_workspace_bytes"] == [ctypes.c_int64, ctypes.c_int]
    assert _lib.RESTYPE["xggm_answer_score_workspace_bytes"] is ctypes.c_size_t
    mk = open(os.path.join(os.path.dirname(_lib.LIB_PATH), "Makefile")).read()
    assert "answer_score.hip" in [w for line in mk.splitlines() if line.startswith("SRCS") for w in line.split()]
    src = open(_lib.HEADER_PATH).read()
    for cite in ("src/vqa/vqacpv2_data.py:134-142", "XGGM_SCORE_MAX_GROUPS 16", "XGGM_SCORE_CHUNK 1024"):
        assert cite in src, cite
    assert _lib.lib.xggm_version() == 100
    L = _lib.lib
    assert L.xggm_answer_score_workspace_bytes(1, 0) == 8 * (2 + 3)
    assert L.xggm_answer_score_workspace_bytes(1024, 0) == 8 * (2 + 3)
    assert L.xggm_answer_score_workspace_bytes(1025, 16) == 8 * (2 + 2 * 35)
    assert L.xggm_answer_score_workspace_bytes(0, 0) == 0 and L.xggm_answer_score_workspace_bytes(5, 17) == 0


def test_answer_score_refuses_bad_arguments_before_any_launch():
    """every refusal of the contract comes back as an error code with a message, with no GPU present: the pointers are
    made-up addresses that nothing dereferences, and every call breaks exactly one rule"""
    from xggm_amd import _lib
    L = _lib.lib
    P = 1 << 20  # an aligned made-up address
    good = dict(labels=P, order=None, keep=None, q_label=P, q_score=P, q_group=None, n=5, n_q=5, K=3, G=0, cursor=None, out=P,
                ws=P, ws_bytes=1 << 16)
    names = list(good)

    def call(**kw):
        a = dict(good, **kw)
        return L.xggm_answer_score(*[a[k] for k in names], None)

    cases = [(dict(labels=None), b"null"), (dict(q_label=None), b"null"), (dict(q_score=None), b"null"), (dict(out=None), b"null"),
             (dict(ws=None), b"null"), (dict(n=0), b"n = 0"), (dict(n=1 << 31), b"n = "), (dict(n_q=0), b"n_q"),
             (dict(K=0), b"K = 0"), (dict(G=17, q_group=P), b"G = 17"), (dict(G=-1), b"G = -1"),
             (dict(q_group=P), b"q_group without G"), (dict(G=2), b"without q_group"),
             (dict(labels=P + 4), b"8-byte"), (dict(order=P + 4), b"8-byte"), (dict(cursor=P + 4), b"8-byte"),
             (dict(out=P + 4), b"8-byte"), (dict(ws=P + 4), b"8-byte"),
             (dict(q_label=P + 2), b"4-byte"), (dict(q_score=P + 2), b"4-byte"), (dict(q_group=P + 2, G=2), b"4-byte"),
             (dict(ws_bytes=8 * (2 + 3) - 1), b"workspace holds")]
    for kw, msg in cases:
        rc = call(**kw)
        assert rc != 0 and msg in L.xggm_last_error(), (kw, L.xggm_last_error())
        assert b"xggm_answer_score" in L.xggm_last_error()
