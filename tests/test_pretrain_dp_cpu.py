"""Host side of data-parallel pre-training (``pretrain.lxmert_pretrain.enable_data_parallel``, ``shard_range``,
``combine_sums``; ``trainlog.fold_host``, xggm_train_log_fold): the pure helpers, the fold's numpy restatement, the C
boundary's refusals (nothing is launched: no GPU is needed to be refused) and the validation-sum combination over a
world-size-2 gloo group of CPU tensors."""
import ctypes
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp


# ------------------------------------------------------------------------------------------------ shard_range
@pytest.mark.parametrize("world", [1, 2, 3])
@pytest.mark.parametrize("n", [0, 1, 7, 8, 9, 35])
def test_shard_range_slices_are_disjoint_contiguous_and_cover_everything(n, world):
    from xggm_amd.pretrain.lxmert_pretrain import shard_range
    parts = [shard_range(n, r, world) for r in range(world)]
    assert all(isinstance(p, range) and p.step == 1 for p in parts)
    assert parts[0].start == 0 and parts[-1].stop == n
    for a, b in zip(parts, parts[1:]):
        assert a.stop == b.start  # contiguous, in rank order, disjoint
    assert [i for p in parts for i in p] == list(range(n))  # the union, every sample exactly once
    assert max(len(p) for p in parts) - min(len(p) for p in parts) <= 1
    for bad in ((n, -1, world), (n, world, world), (-1, 0, world), (n, 0, 0)):
        with pytest.raises(ValueError):
            shard_range(*bad)


# ------------------------------------------------------------------------------------------------ the fold's restatement
def _case(world, n, seed=0):
    from xggm_amd import trainlog as T
    rng = np.random.default_rng([seed, world, n])
    values = rng.standard_normal((world, n, T.COLS)).astype(np.float32)
    kinds = np.tile(rng.integers(0, T.KINDS, n), (world, 1))
    present = np.tile(rng.random((n, T.COLS)) < 0.8, (world, 1, 1))
    present[:, :, 0] = True
    values[~present] = 0.0  # an append leaves 0 in an absent column
    steps = np.tile(np.arange(1, n + 1, dtype=np.int64), (world, 1))
    return values, kinds, present, steps


def test_fold_mean_is_taken_in_rank_order_and_scaled_once():
    from xggm_amd import trainlog as T
    # three values whose fp32 sum depends on the order: (1e8 + 1) - 1e8 = 0 in fp32 but 1e8 + (1 - 1e8) = 0 too; use a
    # case where the orders differ: (a + b) + c with a = 1e8, b = -1e8, c = 1 -> 1; a + (b + c) -> 0
    values = np.zeros((3, 1, T.COLS), dtype=np.float32)
    values[:, 0, 0] = [1e8, -1e8, 1.0]
    values[:, 0, 1] = [1.0, 1e8, -1e8]  # rank order: (1 + 1e8) - 1e8 = 0
    kinds, present = np.full((3, 1), T.PRETRAIN), np.ones((3, 1, T.COLS), dtype=bool)
    out = T.fold_host(values, kinds, present)
    third = np.float32(1.0) / np.float32(3.0)
    assert out["values"].dtype == np.float32
    assert out["values"][0, 0] == np.float32(1.0) * third and out["values"][0, 1] == np.float32(0.0)
    assert out["flag"] == -1 and out["first_bad"] == -1
    # a generic case against the definition, element by element
    values, kinds, present, steps = _case(3, 5)
    out = T.fold_host(values, kinds, present, steps)
    want = ((values[0] + values[1]) + values[2]) * third
    want[~present.all(0)] = 0.0
    assert np.array_equal(out["values"], want) and out["flag"] == -1
    # the sums are those of appends of the folded records: fp64, record order, present columns only
    sums = np.zeros((T.KINDS, T.COLS))
    for i in range(5):
        for c in range(T.COLS):
            if present[0, i, c]:
                sums[kinds[0, i], c] += float(want[i, c])
    assert np.array_equal(out["sums"], sums) and out["counts"].tolist() == np.bincount(kinds[0], minlength=T.KINDS).tolist()


def test_fold_nan_propagates_and_present_is_the_intersection():
    from xggm_amd import trainlog as T
    values, kinds, present, steps = _case(2, 5, seed=1)
    values[1, 3, 0] = np.nan
    out = T.fold_host(values, kinds, present, steps, cursor=5)
    assert np.isnan(out["values"][3, 0]) and out["first_bad"] == 3 and np.isnan(out["sums"][kinds[0, 3], 0])
    assert np.isfinite(np.delete(out["values"], 3, axis=0)).all()
    # a column absent on ONE rank is absent in the result (and the mismatch is reported: next test)
    present[1, 2, 0] = False
    out = T.fold_host(values, kinds, present, steps)
    assert not out["present"][2, 0] and out["values"][2, 0] == 0.0 and out["present"][1, 0]
    assert np.array_equal(out["present"], present.all(0))


def test_fold_reports_the_first_record_the_ranks_disagree_on():
    from xggm_amd import trainlog as T
    for what in ("step", "kind", "present"):
        for where in (0, 4):
            values, kinds, present, steps = _case(3, 5, seed=2)
            if what == "step":
                steps[2, where] += 1
            elif what == "kind":
                kinds[1, where] = (kinds[1, where] + 1) % T.KINDS
            else:
                present[1, where, 0] = False
            assert T.fold_host(values, kinds, present, steps)["flag"] == where, (what, where)
    values, kinds, present, steps = _case(3, 5, seed=2)
    steps[1, 3] += 1
    kinds[2, 1] = (kinds[2, 1] + 1) % T.KINDS
    assert T.fold_host(values, kinds, present, steps)["flag"] == 1  # the FIRST
    assert T.fold_host(*_case(3, 5), cursors=[5, 5, 4])["flag"] == 5  # a cursor alone: n
    assert T.fold_host(*_case(3, 5), cursors=[5, 5, 5])["flag"] == -1


def test_fold_of_one_rank_is_the_identity():
    from xggm_amd import trainlog as T
    values, kinds, present, steps = _case(1, 5, seed=3)
    values[0, 1, 7] = 42.0  # even where a column is absent: nothing is touched
    present[0, 1, 7] = False
    out = T.fold_host(values, kinds, present, steps)
    assert np.array_equal(out["values"], values[0]) and np.array_equal(out["present"], present[0])
    assert np.array_equal(out["kinds"], kinds[0]) and out["flag"] == -1


# ------------------------------------------------------------------------------------------------ the C boundary
def test_fold_entry_point_is_exported_and_refuses_bad_arguments_before_any_launch():
    from xggm_amd import _lib, ops
    assert "xggm_train_log_fold" in _lib.parse_header() and len(_lib.parse_header()["xggm_train_log_fold"]) == 13
    assert hasattr(_lib.lib, "xggm_train_log_fold")
    L = _lib.lib
    fake = 0x1000  # aligned, never touched
    d = ops.TrainLogDesc(fake, fake, fake, fake, fake, fake, fake, 8)
    D = ctypes.addressof(d)

    def refused(*args):
        rc = L.xggm_train_log_fold(*args)
        assert rc != 0 and b"xggm_train_log_fold" in L.xggm_last_error(), args
        return L.xggm_last_error()

    good = [fake, fake, fake, fake, 64, 8, 8, 1, 2, 4, D, fake, None]

    def but(**kw):
        names = ["vals", "kinds", "steps", "cursors", "sv", "sk", "ss", "sc", "world", "n", "log", "flag", "stream"]
        a = list(good)
        for k, v in kw.items():
            a[names.index(k)] = v
        return a

    assert b"world = 0" in refused(*but(world=0))
    assert b"world = -2" in refused(*but(world=-2))
    assert b"null log" in refused(*but(log=None))
    for field in ("values", "kinds", "cursor", "sums", "counts", "first_bad"):  # a null ring
        e = ops.TrainLogDesc.from_buffer_copy(d)
        setattr(e, field, None)
        assert b"ring" in refused(*but(log=ctypes.addressof(e))), field
    refused(*but(vals=None))
    refused(*but(kinds=None))
    refused(*but(flag=None))
    assert b"n = 0" in refused(*but(n=0))
    assert b"n = 9" in refused(*but(n=9))  # more than the capacity
    assert b"stride" in refused(*but(sv=31))
    assert b"stride" in refused(*but(sk=3))
    assert b"aligned" in refused(*but(steps=fake + 4))
    assert b"aligned" in refused(*but(cursors=fake + 4))
    assert b"aligned" in refused(*but(flag=fake + 4))
    assert b"aligned" in refused(*but(vals=fake + 2))
    assert b"aligned" in refused(*but(kinds=fake + 1))
    e = ops.TrainLogDesc.from_buffer_copy(d)
    e.sums = fake + 4
    assert b"aligned" in refused(*but(log=ctypes.addressof(e)))
    e = ops.TrainLogDesc.from_buffer_copy(d)
    e.capacity = 0
    assert b"capacity = 0" in refused(*but(log=ctypes.addressof(e)))


def test_fold_wrapper_refuses_cpu_tensors_and_short_buffers():
    from xggm_amd import ops

    class Log:
        capacity = 4

    with pytest.raises(ValueError, match="world"):
        ops.train_log_fold(Log, None, None, 0, 2, None)
    with pytest.raises(ValueError, match="records"):
        ops.train_log_fold(Log, None, None, 2, 5, None)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.train_log_fold(Log, torch.zeros(64), torch.zeros(8, dtype=torch.int32), 2, 4, torch.zeros(1, dtype=torch.int64))


# ------------------------------------------------------------------------------------------------ scope cuts
@pytest.mark.parametrize("kw", [dict(zero1=True), dict(overlap=True)])
def test_scope_cuts_are_refused_before_anything_is_touched(kw, monkeypatch):
    """the sharded update and the staged exchange are not built for pre-training: NotImplementedError that names the
    function, raised before a process group (or the model) is asked anything"""
    from xggm_amd.pretrain import lxmert_pretrain as P

    def touched(*a, **k):
        raise AssertionError("a process group was touched")

    for name in ("is_initialized", "get_rank", "get_world_size", "broadcast"):
        monkeypatch.setattr(dist, name, touched)
    with pytest.raises(NotImplementedError, match="pretrain.lxmert_pretrain.enable_data_parallel"):
        P.enable_data_parallel(object(), **kw)


# ------------------------------------------------------------------------------------------------ gloo, world size 2
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_sums(rank):
    """13 fp64 sums and a step count per rank whose total depends on the order of the adds in the last bits"""
    rng = np.random.default_rng(100 + rank)
    return (rng.standard_normal(13) * 10.0 ** rng.integers(-8, 8, 13)).tolist(), 3 - rank


def _combine_worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from xggm_amd.pretrain.lxmert_pretrain import combine_sums
        sums, steps = _rank_sums(rank)
        total, n = combine_sums(sums, steps)
        empty, n0 = combine_sums([0.0] * 13 if rank else sums, 0 if rank else steps)  # a rank that took no step
        q.put((rank, total.tobytes(), n, empty.tobytes(), n0))
    finally:
        dist.destroy_process_group()


def test_validation_sums_combine_to_the_same_bits_on_both_ranks():
    from xggm_amd.pretrain.lxmert_pretrain import combine_sums, combine_sums_host
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_combine_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=120) for _ in range(world))
    for p in procs:
        p.join(60)
    (_, t0, n0, e0, m0), (_, t1, n1, e1, m1) = res
    assert t0 == t1 and n0 == n1 == 5 and e0 == e1 and m0 == m1 == 3  # the same bits on both ranks
    # ... and those of the numpy restatement: fp64, added in rank order, starting from zero
    per = [_rank_sums(r) for r in range(world)]
    want = np.zeros(13)
    for s, _ in per:
        want = want + np.asarray(s, dtype=np.float64)
    assert t0 == want.tobytes()
    total, n = combine_sums_host([s for s, _ in per], [k for _, k in per])
    assert total.tobytes() == t0 and n == 5
    assert e0 == (np.zeros(13) + np.asarray(per[0][0]) + np.zeros(13)).tobytes()
    # without a process group: the input
    alone, k = combine_sums(per[0][0], 3)
    assert alone.tolist() == per[0][0] and k == 3
