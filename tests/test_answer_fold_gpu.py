"""The answer-log fold on the GPU: the kernel (xggm_answer_log_fold / ``ops.answer_log_fold``) against its numpy restatement
(``answers.fold_logs_host``) bit for bit, with every buffer between sentinel bands -- nothing outside ``labels[0, total)``,
``scores[0, total)``, cursor, score_sum, flags and the flag may change, whatever the device cursors say --, replayed from a
captured graph, and ``AnswerLog.fold`` in a one-rank group."""
import types

import numpy as np
import pytest
import torch

from answer_fold_cases import CASES, expect_of, packed_logs
from test_pretrain_dp_gpu import PAD, SENTINEL, _banded

pytestmark = pytest.mark.gpu

DEV = "cuda"
VARIANTS = ("clean", "cursor_off_by_one", "refused_on_rank_1", "cursors_far_above_capacity")
PARAMS = [(c, ws, v) for c in CASES for ws in (True, False) for v in VARIANTS
          if not (v == "refused_on_rank_1" and len(c["expect"]) < 2)]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _dst(capacity, with_scores, odd_scores):
    """a destination laid out as ``engine.AnswerLog`` lays its own out, between two sentinel bands; ``odd_scores``: the scores
    start one float behind a word boundary -- a region that is only 4-byte aligned"""
    words = 3 + capacity + ((capacity + 2) // 2 if with_scores else 0)
    raw, buf = _banded(words)
    o = 1 if odd_scores else 0
    log = types.SimpleNamespace(capacity=capacity, buf=buf, cursor=buf[0:1], flags=buf[2:3].view(torch.int32)[0:1],
                                score_sum=buf[1:2].view(torch.float64) if with_scores else None, labels=buf[3:3 + capacity],
                                scores=buf[3 + capacity:].view(torch.float32)[o:o + capacity] if with_scores else None)
    return raw, log


def _setup(case, with_scores, variant, extra_stride=2):
    from xggm_amd import answers as A
    expect = expect_of(case)
    world, total, cap = len(expect), sum(expect), int(case["capacity"])
    bufs, _, _ = packed_logs(case, with_scores)
    if variant == "cursor_off_by_one":
        bufs[-1, 0] += 1
    elif variant == "refused_on_rank_1":
        bufs[1, 2] = 3
    elif variant == "cursors_far_above_capacity":
        bufs[:, 0] = 1 << 40
    want = A.fold_logs_host(bufs, cap, with_scores, case["layout"], case.get("block"), expect)
    words = bufs.shape[1]
    stride = words + extra_stride  # the words between two ranks' logs stay sentinels
    raw_g, g = _banded(world * stride)
    g.view(world, stride)[:, :words].copy_(torch.from_numpy(bufs))
    raw_d, dst = _dst(total + 3, with_scores, odd_scores=total % 2 == 1)
    raw_f, flag = _banded(1)
    expected = raw_d.clone()
    e = expected[PAD:PAD + dst.buf.numel()]
    e[0] = total
    e[2:3].view(torch.int32)[0] = 0
    e[3:3 + total].copy_(torch.from_numpy(want["labels"]))
    if with_scores:
        e[1:2].view(torch.float64)[0] = want["score_sum"]
        o = 1 if total % 2 == 1 else 0
        e[3 + dst.capacity:].view(torch.float32)[o:o + total].copy_(torch.from_numpy(want["scores"]))
    return dict(g=g.view(world, stride), raw_g=raw_g, dst=dst, raw_d=raw_d, flag=flag, raw_f=raw_f, expected=expected, want=want,
                cap=cap, expect=expect, stride=stride)


def _launch(s, case, with_scores):
    from xggm_amd import ops
    ops.answer_log_fold(s["g"], s["dst"], s["flag"], s["cap"], with_scores, case["layout"], s["expect"], block=case.get("block", 1),
                        log_stride=s["stride"])


@pytest.mark.parametrize("case,with_scores,variant", PARAMS, ids=lambda p: p["id"] if isinstance(p, dict) else str(p))
def test_fold_equals_the_restatement_and_writes_nothing_else(case, with_scores, variant):
    from xggm_amd import answers as A
    s = _setup(case, with_scores, variant)
    before = s["raw_g"].clone()
    _launch(s, case, with_scores)
    torch.cuda.synchronize()
    want, world = s["want"], len(s["expect"])
    if variant == "clean":
        assert want["flag"] == 0
    elif variant == "cursor_off_by_one":
        assert want["flag"] == A.FOLD_FLAG_CURSOR | ((world - 1) << 8)
    elif variant == "refused_on_rank_1":
        assert want["flag"] == A.FOLD_FLAG_REFUSED | (1 << 8)
    else:
        assert want["flag"] == A.FOLD_FLAG_CURSOR
    assert int(s["flag"][0]) == want["flag"]
    band = torch.full((PAD,), SENTINEL, dtype=torch.int64, device=DEV)
    assert torch.equal(s["raw_f"][:PAD], band) and torch.equal(s["raw_f"][PAD + 1:], band)
    assert torch.equal(s["raw_g"], before)  # the gathered logs are only read
    # every word of the destination: the copy is carried out whatever the variant, and nothing else moves -- the tail of
    # labels and scores behind ``total``, the upper half of the flags word, the float in front of an odd scores region, the bands
    assert torch.equal(s["raw_d"], s["expected"])
    assert int(s["dst"].cursor[0]) == sum(s["expect"])


def test_a_destination_with_scores_keeps_them_when_the_sources_have_none():
    case = CASES[0]
    s = _setup(case, False, "clean")
    raw_d, dst = _dst(sum(s["expect"]) + 3, True, odd_scores=True)
    s["dst"] = dst
    expected = raw_d.clone()
    e = expected[PAD:PAD + dst.buf.numel()]
    e[0], e[1] = sum(s["expect"]), 0  # the sum of the ranks' (zero) sum words
    e[2:3].view(torch.int32)[0] = 0
    e[3:3 + 9].copy_(torch.from_numpy(s["want"]["labels"]))
    _launch(s, case, False)
    torch.cuda.synchronize()
    assert torch.equal(raw_d, expected) and int(s["flag"][0]) == 0


@pytest.mark.parametrize("case", [CASES[2], CASES[-1]], ids=lambda c: c["id"])
def test_fold_replayed_from_a_graph_equals_the_eager_one(case):
    s = _setup(case, True, "clean")
    _launch(s, case, True)
    torch.cuda.synchronize()
    eager, eager_flag = s["raw_d"].clone(), s["raw_f"].clone()
    assert torch.equal(eager, s["expected"])
    s["raw_d"].fill_(SENTINEL)
    s["raw_f"].fill_(SENTINEL)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            _launch(s, case, True)  # no allocation, no host synchronisation: legal in a capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for _ in range(2):
        s["raw_d"].fill_(SENTINEL)
        s["raw_f"].fill_(SENTINEL)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(s["raw_d"], eager) and torch.equal(s["raw_f"], eager_flag)


def test_wrapper_refuses_what_would_read_past_the_gathered_buffer():
    from xggm_amd import ops
    case = CASES[0]
    s = _setup(case, True, "clean", extra_stride=0)
    flat = s["g"].reshape(-1)
    with pytest.raises(ValueError, match="logs holds"):
        ops.answer_log_fold(flat[:-1], s["dst"], s["flag"], s["cap"], True, case["layout"], s["expect"])
    with pytest.raises(ValueError, match="logs holds"):
        ops.answer_log_fold(flat, s["dst"], s["flag"], s["cap"], True, case["layout"], s["expect"], log_stride=s["stride"] - 1)
    with pytest.raises(ValueError, match="with_scores"):
        ops.answer_log_fold(flat, types.SimpleNamespace(**dict(vars(s["dst"]), scores=None)), s["flag"], s["cap"], True,
                            case["layout"], s["expect"])
    with pytest.raises(RuntimeError, match="overlap"):
        ops.answer_log_fold(s["dst"].buf, s["dst"], s["flag"], 1, False, case["layout"], [1], log_stride=4)
    with pytest.raises(TypeError):
        ops.answer_log_fold(flat.int(), s["dst"], s["flag"], s["cap"], True, case["layout"], s["expect"])
    torch.cuda.synchronize()
    assert torch.equal(s["raw_d"][PAD:PAD + s["dst"].buf.numel()], torch.full_like(s["dst"].buf, SENTINEL))  # nothing ran


def test_fold_in_a_one_rank_group_returns_the_log_itself():
    from xggm_amd import ops
    from xggm_amd.engine import AnswerLog
    log = AnswerLog(4, DEV)
    assert log.fold(ops.FOLD_CONCAT, [4]) is log
    assert log.fold(ops.FOLD_INTERLEAVE, [4], block=2) is log
    assert getattr(log, "_merged", None) is None  # no launch, nothing was made
