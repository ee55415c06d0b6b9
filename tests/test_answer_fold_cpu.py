"""The answer-log fold without a GPU: ``answers.fold_logs_host`` (the numpy restatement of xggm_answer_log_fold) against the
orders it has to invert -- ``ResidentDataset.order(rank=, world=)`` and ``dist.shard_range`` --, the score of a folded sweep
against the score of the same sweep in one log, every refusal of the entry through the loaded library (nothing is launched),
``dist.sync_branches`` without a process group and the global step count of the data-parallel drivers."""
import ctypes
import random

import numpy as np
import pytest

from answer_fold_cases import CASES, expect_of, packed_logs

CONCAT, INTERLEAVE = 0, 1


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["id"])
def test_destinations_are_a_bijection(case):
    """every destination index in [0, total) is hit exactly once, and the restatement's copy puts every rank's labels and
    scores there"""
    from xggm_amd import answers as A
    expect = expect_of(case)
    dest = A.fold_destinations(case["layout"], expect, case.get("block"))
    total = sum(expect)
    assert [len(d) for d in dest] == expect
    assert sorted(np.concatenate(dest).tolist()) == list(range(total))
    for ws in (True, False):
        bufs, labels, scores = packed_logs(case, ws)
        got = A.fold_logs_host(bufs, case["capacity"], ws, case["layout"], case.get("block"), expect)
        assert got["cursor"] == total and got["flags"] == 0 and got["flag"] == 0
        for r, d in enumerate(dest):
            assert np.array_equal(got["labels"][d], labels[r][:expect[r]])
            if ws:
                assert np.array_equal(got["scores"][d], scores[r][:expect[r]])
        assert (got["scores"] is None) == (not ws)
        s = np.float64(0.0)
        for r in range(len(expect)):
            s = s + bufs[r, 1:2].view(np.float64)[0]
        assert got["score_sum"] == float(s)


def test_interleave_inverts_the_stores_rank_order(tmp_path):
    """the ranks' slices of an epoch (``ResidentDataset.order(rank=, world=)``), folded with INTERLEAVE and block B, are
    ``perm[:steps * B * world]`` again"""
    from test_resident_cpu import _store, _ts
    from xggm_amd import answers as A
    store = _store(_ts(tmp_path))
    n, seed, epoch = len(store), 3, 5
    perm = np.random.default_rng([seed, epoch]).permutation(n)
    for world, B in ((2, 3), (3, 2), (2, 1), (1, 4)):
        steps = n // (B * world)
        assert steps >= 1
        slices = [store.order(epoch, seed=seed, rank=r, world=world, batch_size=B) for r in range(world)]
        if world == 1:
            slices = [slices[0][:steps * B]]
        cap = steps * B + 1
        bufs = np.zeros((world, A.packed_words(cap, False)), dtype=np.int64)
        for r in range(world):
            bufs[r, 0] = steps * B
            bufs[r, 3:3 + steps * B] = slices[r]
        got = A.fold_logs_host(bufs, cap, False, INTERLEAVE, B, [steps * B] * world)
        assert got["flag"] == 0 and got["labels"].tolist() == perm[:steps * B * world].tolist(), (world, B)
        # the global order the drivers score against: one rank at the global batch size
        assert store.order(epoch, seed=seed, drop_last=True, batch_size=B * world).tolist() == perm[:steps * B * world].tolist()


@pytest.mark.parametrize("n,world", [(9, 2), (7, 3), (2, 3), (1, 4), (64, 64), (5, 1)])
def test_concat_over_shard_ranges_is_the_unsharded_sweep(n, world):
    from xggm_amd import answers as A
    from xggm_amd.dist import shard_range
    from xggm_amd.pretrain import lxmert_pretrain
    assert lxmert_pretrain.shard_range is shard_range  # one definition
    sweep = np.random.default_rng([n, world]).integers(0, 3000, n)
    cap = n
    bufs = np.zeros((world, A.packed_words(cap, False)), dtype=np.int64)
    counts = []
    for r in range(world):
        mine = shard_range(n, r, world)
        counts.append(len(mine))
        bufs[r, 0] = len(mine)
        bufs[r, 3:3 + len(mine)] = sweep[mine.start:mine.stop]
    if n < world:
        assert 0 in counts
    got = A.fold_logs_host(bufs, cap, False, CONCAT, None, counts)
    assert got["flag"] == 0 and got["cursor"] == n and np.array_equal(got["labels"], sweep)


def test_score_is_unchanged_by_sharding():
    """``score_host`` over a folded sweep == ``score_host`` over the same labels in one log, bit for bit; question id 7 occurs
    on both sides of the rank boundary and counts once, with its last answer (``last_occurrence_mask`` of the global order)"""
    from xggm_amd import answers as A
    from xggm_amd.dist import shard_range
    rng = np.random.default_rng(12)
    n, K, world = 9, 3, 2
    tables = dict(q_label=rng.integers(0, 6, (n, K)).astype(np.int32), q_score=rng.choice([0.3, 0.6, 0.9, 1.0], (n, K)).astype(np.float32))
    tables["q_label"][:, 0] = np.arange(n) % 6  # slot 0 matches the label chosen below for most samples
    qids = np.array([1, 2, 3, 7, 5, 7, 6, 8, 9])  # positions 3 (rank 0's slice 0..5) and 5 (rank 1's) share an id
    labels = (np.arange(n) % 6).astype(np.int64)
    labels[3] = 5  # ... with different answers
    keep = A.last_occurrence_mask(qids)
    assert keep.tolist() == [1, 1, 1, 0, 1, 1, 1, 1, 1]
    whole = A.score_host(labels, tables, keep=keep, cursor=n)
    bufs = np.zeros((world, A.packed_words(n, False)), dtype=np.int64)
    counts = []
    for r in range(world):
        mine = shard_range(n, r, world)
        counts.append(len(mine))
        bufs[r, 0], bufs[r, 3:3 + len(mine)] = len(mine), labels[mine.start:mine.stop]
    assert counts == [5, 4]
    f = A.fold_logs_host(bufs, n, False, CONCAT, None, counts)
    folded = A.score_host(f["labels"], tables, keep=keep, cursor=f["cursor"])
    assert np.array_equal(folded.numpy(), whole.numpy())
    res = A.decode_score(folded, 0)
    assert res["count"] == 8 and res["score"] > 0
    # a per-rank mask would count the id twice
    per_rank = np.concatenate([A.last_occurrence_mask(qids[:5]), A.last_occurrence_mask(qids[5:])])
    assert int(per_rank.sum()) == 9


def test_flag_of_the_restatement():
    from xggm_amd import answers as A
    bufs = np.zeros((3, A.packed_words(4, True)), dtype=np.int64)
    bufs[:, 0] = (2, 3, 1)
    assert A.fold_logs_host(bufs, 4, True, CONCAT, None, (2, 3, 1))["flag"] == 0
    bufs[2, 0] = 2
    assert A.fold_logs_host(bufs, 4, True, CONCAT, None, (2, 3, 1))["flag"] == A.FOLD_FLAG_CURSOR | (2 << 8)
    bufs[1, 2] = 3
    assert A.fold_logs_host(bufs, 4, True, CONCAT, None, (2, 3, 1))["flag"] == (A.FOLD_FLAG_CURSOR | A.FOLD_FLAG_REFUSED | (1 << 8))
    assert "rank is 1" in A.fold_flag_message(3 | (1 << 8))
    for bad in (dict(layout=2), dict(expect=(2, 3, -1)), dict(expect=(0, 0, 0)), dict(layout=INTERLEAVE, block=2, expect=(2, 2, 4)),
                dict(layout=INTERLEAVE, block=3, expect=(2, 2, 2)), dict(layout=INTERLEAVE, block=0, expect=(2, 2, 2)),
                dict(expect=(5, 0, 0))):
        kw = dict(dict(layout=CONCAT, block=None, expect=(2, 3, 1)), **bad)
        with pytest.raises(ValueError):
            A.fold_logs_host(bufs, 4, True, kw["layout"], kw["block"], kw["expect"])


def test_entry_refuses_before_any_launch():
    """every refusal of xggm_answer_log_fold, through the loaded library: the pointers are never dereferenced (no GPU here)"""
    from xggm_amd import _lib, ops
    L = _lib.lib
    P, FAR = 1 << 20, 1 << 30  # the gathered logs at P; the destination far behind them

    def run(logs=P, log_stride=16, src_capacity=8, with_scores=1, world=2, layout=CONCAT, block=1, expect=(5, 4), flag=FAR + 4096,
            dst=True, **d):
        desc = ops.AnswerLogDesc(FAR, FAR + 1024, FAR + 2048, FAR + 2056, FAR + 2064, 16)
        for k, v in d.items():
            setattr(desc, k, v)
        exp = None if expect is None else ctypes.cast((ctypes.c_int64 * len(expect))(*expect), ctypes.c_void_p)
        rc = L.xggm_answer_log_fold(logs, log_stride, src_capacity, with_scores, world, layout, block, exp,
                                    ctypes.addressof(desc) if dst else None, flag, None)
        return rc, L.xggm_last_error()

    cases = [(dict(logs=None), b"null"), (dict(expect=None), b"null"), (dict(dst=False), b"null"), (dict(flag=None), b"null"),
             (dict(labels=None), b"labels, cursor and flags"), (dict(cursor=None), b"labels, cursor and flags"),
             (dict(flags=None), b"labels, cursor and flags"),
             (dict(world=0), b"world = 0"), (dict(world=65, expect=(1,) * 65), b"world = 65"),
             (dict(expect=(5, -1)), b"expect[1] = -1"), (dict(expect=(9, 1)), b"expect[0] = 9"),
             (dict(expect=(0, 0)), b"0 answers in all"), (dict(expect=(8, 8), capacity=15), b"16 answers in all"),
             (dict(layout=2), b"unknown layout 2"), (dict(layout=-1), b"unknown layout -1"),
             (dict(layout=INTERLEAVE, expect=(4, 2), block=2), b"equal counts"),
             (dict(layout=INTERLEAVE, expect=(4, 4), block=0), b"block = 0"),
             (dict(layout=INTERLEAVE, expect=(4, 4), block=3), b"multiples of block 3"),
             (dict(scores=None), b"with_scores needs dst->scores"),
             (dict(log_stride=14), b"shorter than one packed log of 15 words"), (dict(log_stride=10, with_scores=0), b"of 11 words"),
             (dict(labels=P + 8 * 20), b"overlap"), (dict(scores=P), b"overlap"), (dict(cursor=P + 8 * 30), b"overlap"),
             (dict(score_sum=P + 8), b"overlap"), (dict(flags=P + 16), b"overlap"), (dict(flag=P - 8 + 8 * 31), b"overlap"),
             (dict(logs=P + 4), b"8-byte"), (dict(labels=FAR + 4), b"8-byte"), (dict(cursor=FAR + 2052), b"8-byte"),
             (dict(score_sum=FAR + 2060), b"8-byte"), (dict(flag=FAR + 4100), b"8-byte"), (dict(scores=FAR + 1026), b"4-byte"),
             (dict(flags=FAR + 2066), b"4-byte")]
    for kw, msg in cases:
        rc, err = run(**kw)
        assert rc != 0 and b"xggm_answer_log_fold" in err and msg in err, (kw, err)


def test_sync_branches_without_a_group_is_the_per_iteration_sequence():
    from xggm_amd.dist import sync_branches
    from xggm_amd.vqa.vqacpv2 import pick_branch
    for delta in (0, 3, 5, 10):
        random.seed(17)
        one_by_one = [pick_branch(delta) for _ in range(23)]
        after = random.random()
        random.seed(17)
        got = sync_branches(23, "cpu", delta=delta)
        assert ["rel" if b else "node" for b in got] == one_by_one and random.random() == after
    assert sync_branches(0, "cpu") == []


def test_global_step_count():
    """``t_total`` and ``val_schedule`` count GLOBAL steps: ``world`` ranks at ``B`` per rank == one rank at ``world x B``"""
    from xggm_amd.vqa.vqacpv2 import global_steps, val_schedule
    assert global_steps(24, 4) == 6 and global_steps(24, 4, 2) == 3 and global_steps(27, 4, 2) == 3 and global_steps(7, 4, 2) == 0
    for n, B, world in ((24, 4, 2), (219928, 32, 8), (1000, 7, 3)):
        assert global_steps(n, B, world) == global_steps(n, B * world, 1) == n // (B * world)
        assert val_schedule(global_steps(n, B, world)).tolist() == val_schedule(n // (B * world)).tolist()
    assert [int(v) for v in val_schedule(global_steps(24, 4, 2))] == [0, 1, 2]
    epochs = 3
    assert int(global_steps(24, 4, 2) * epochs) == 9  # t_total; BertAdam is handed 2 * t_total (two passes per iteration)
