"""The replica drift guard without a GPU: the numpy restatement of the fingerprint against a word-by-word loop of the
contract (include/xggm.h, xggm_fingerprint_spans), the certainty of single-word detection, the argument validation of the
C entry point, and ``dist.ReplicaGuard`` over gloo on a toy arena of CPU tensors (world size 2 and 4)."""
import ctypes
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

M32, M64 = 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF


def scalar_fingerprint(words, salt):
    """the contract, one word at a time, in Python integers"""
    acc = 0
    for i, w in enumerate(words):
        k = (i * 0x9E3779B9 + salt) & M32
        x = ((int(w) ^ k) * 0x7FEB352D) & M32
        x ^= x >> 15
        acc = (acc + x * (2 * (i & 0x7FFFFFFF) + 1)) & M64
    return acc


@pytest.mark.parametrize("n", [0, 1, 3, 1025])
@pytest.mark.parametrize("salt", [0, 1, 0x73686477, 0xFFFFFFFF])
def test_host_restatement_equals_the_scalar_definition(n, salt):
    from xggm_amd.fingerprint import fingerprint_host
    w = np.random.default_rng(1000 * n + (salt & 0xFF)).integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    want = scalar_fingerprint(w.tolist(), salt)
    assert fingerprint_host(w, salt) == want
    assert fingerprint_host(w.view(np.uint8), salt) == want and fingerprint_host(torch.from_numpy(w.view(np.int32)), salt) == want
    if n == 0:
        assert want == 0
    if n % 2 == 0:
        assert fingerprint_host(torch.from_numpy(w.view(np.int16)).view(torch.bfloat16), salt) == want


def test_host_restatement_is_fast_and_wraps_the_index():
    """a few million words in well under a second; chunked evaluation equals the one-piece definition"""
    import time
    from xggm_amd import fingerprint as F
    w = np.random.default_rng(7).integers(0, 1 << 32, size=(1 << 22) + 4099, dtype=np.uint64).astype(np.uint32)
    t0 = time.time()
    got = F.fingerprint_host(w, 5)
    assert time.time() - t0 < 1.0
    i = np.arange(w.size, dtype=np.uint64)
    x = ((w.astype(np.uint64) ^ ((i * np.uint64(0x9E3779B9) + np.uint64(5)) & np.uint64(M32))) * np.uint64(0x7FEB352D)) & np.uint64(M32)
    x ^= x >> np.uint64(15)
    assert got == int(np.sum(x * (np.uint64(2) * i + np.uint64(1)), dtype=np.uint64))


def test_single_word_changes_are_detected_with_certainty():
    from xggm_amd.fingerprint import fingerprint_host, fingerprint
    rng = np.random.default_rng(11)
    w = rng.integers(0, 1 << 32, size=4099, dtype=np.uint64).astype(np.uint32)
    w[17] = 0
    w[18] = M32
    base = fingerprint_host(w, 3)
    for pos in (0, 1, 17, 18, 255, 256, 1024, 4097, 4098):
        for bit in range(32):
            v = w.copy()
            v[pos] ^= np.uint32(1 << bit)
            assert fingerprint_host(v, 3) != base, (pos, bit)
    # exchanging two unequal words (seeded cases, neighbours and far apart, equal words skipped by construction)
    for a, b in [(0, 1), (5, 6), (17, 18), (0, 4098), (100, 3000), (1023, 1024)] + \
            [tuple(int(x) for x in rng.choice(w.size, 2, replace=False)) for _ in range(64)]:
        assert w[a] != w[b]
        v = w.copy()
        v[a], v[b] = w[b], w[a]
        assert fingerprint_host(v, 3) != base, (a, b)
    # position in memory does not enter: the same bytes at another offset of a larger buffer (also a misaligned one)
    big = np.zeros(3 * w.size + 8, dtype=np.uint32)
    for off in (1, 2, 7, w.size + 3):
        big[:] = rng.integers(0, 1 << 32, size=big.size, dtype=np.uint64).astype(np.uint32)
        big[off:off + w.size] = w
        assert fingerprint_host(big[off:off + w.size], 3) == base
        t = torch.from_numpy(big.view(np.int32))
        assert int(fingerprint(t, [(off, off + w.size)], 3)[0]) & M64 == base
    # salts separate buffers, also all-zero ones
    assert len({fingerprint_host(w, s) for s in (0, 1, 2, 3, 0x80000000)}) == 5
    z = np.zeros(64, dtype=np.uint32)
    assert len({fingerprint_host(z, s) for s in (0x70617261, 0x6D6F6D31, 0x6D6F6D32, 0x73686477)}) == 4
    # element ranges of bf16 / uint8 tensors, an empty one in the middle; the int64 word carries the uint64 bits
    h = torch.from_numpy(w.view(np.int16)).view(torch.bfloat16)
    got = fingerprint(h, [(0, 8), (8, 8), (8, 2 * 1025)], 9)
    assert got.dtype == torch.int64 and [int(x) & M64 for x in got] == [
        scalar_fingerprint(w[:4].tolist(), 9), 0, scalar_fingerprint(w[4:1025].tolist(), 9)]
    with pytest.raises(ValueError):
        fingerprint(h, [(0, 3)])
    with pytest.raises(ValueError):
        fingerprint(torch.zeros(16, dtype=torch.uint8), [(2, 6)])


def test_fingerprint_entry_point_validates_before_launch():
    """in the style of test_argument_validation_fails_before_launch: rejected on the host, nothing is enqueued"""
    from xggm_amd import _lib, ops
    L = _lib.lib
    nb = L.xggm_fingerprint_workspace_bytes(1, 0)
    assert nb >= 8 * 2048 and L.xggm_fingerprint_workspace_bytes(28, 7) >= 8 * (7 + 28)
    assert L.xggm_fingerprint_workspace_bytes(1, 7) < nb

    def launch(p, nbytes, ws_bytes=nb, n=1, out=4096, ws=8192, wgs=0):
        sp = (ops.FpSpan * 1)()
        sp[0].ptr, sp[0].bytes, sp[0].salt = p, nbytes, 1
        return L.xggm_fingerprint_spans(ctypes.addressof(sp), n, out, ws, ws_bytes, wgs, None)

    for args, word in (((4096 + 2, 64), b"4-byte aligned"), ((4096, 66), b"multiple of 4"), ((4096, -4), b"multiple of 4"),
                       ((None, 64), b"null pointer"), ((4096, 64, nb - 8), b"workspace")):
        assert launch(*args) != 0
        err = L.xggm_last_error()
        assert b"xggm_fingerprint_spans" in err and word in err, (args, err)
    assert launch(4096, 64, n=-1) != 0 and b"xggm_fingerprint_spans" in L.xggm_last_error()
    assert launch(4096, 64, wgs=-1) != 0 and b"xggm_fingerprint_spans" in L.xggm_last_error()
    assert launch(4096, 64, out=None) != 0 and b"xggm_fingerprint_spans" in L.xggm_last_error()
    assert launch(4096, 64, ws=None) != 0 and b"xggm_fingerprint_spans" in L.xggm_last_error()
    assert L.xggm_fingerprint_spans(None, 0, None, None, 0, 0, None) == 0  # no ranges: nothing to do, nothing launched
    from xggm_amd import _lib as lib2
    src = open(lib2.HEADER_PATH).read()
    assert "src/lxrt/entry.py:183-184" in src and L.xggm_version() == 100


# ---------------------------------------------------------------------------------------------- the guard over gloo
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


class _Grp:
    def __init__(self, start, vec_start, end):
        self.start, self.vec_start, self.end = start, vec_start, end


class _Arena:
    pass


def _toy_arena():
    """two groups, matrix + vector regions, as tests/test_dist_cpu.py::_sharded_worker builds it (CPU tensors)"""
    a = _Arena()
    a.groups = {"g0": _Grp(0, 1024, 1200), "g1": _Grp(1280, 1792, 1800)}
    a.info = {"g0.w0": (0, 512, "g0", False), "g0.w1": (512, 512, "g0", False), "g0.b": (1024, 176, "g0", True),
              "g1.w": (1280, 512, "g1", False), "g1.b": (1792, 8, "g1", True)}
    n = a.total = 2048
    g = torch.Generator().manual_seed(5)
    a.params = torch.randn(n, generator=g)
    a.m = torch.randn(n, generator=g)
    a.v = torch.rand(n, generator=g)
    a.shadow = a.params.to(torch.bfloat16)
    a.grads = torch.zeros(n)
    a.wire = torch.zeros(n, dtype=torch.bfloat16)
    a.zero1 = None
    return a


def _expect_drift(guard, level, buffer, group, element, ranks, param):
    from xggm_amd.dist import ReplicaDrift
    try:
        guard.check("test", level=level)
    except ReplicaDrift as e:
        return (e.buffer == buffer and e.group == group and e.elements[0] <= element < e.elements[1]
                and e.elements[1] - e.elements[0] <= 256 and e.ranks == ranks and e.param == param and param in str(e)
                and e.iteration == guard.iteration and "test" in str(e))
    return False


def _guard_worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from xggm_amd.dist import ReplicaGuard, ShardedUpdate
        calls = [0]
        plain_all_reduce = dist.all_reduce

        def counted(*a, **k):
            calls[0] += 1
            return plain_all_reduce(*a, **k)

        dist.all_reduce = counted
        a = _toy_arena()
        last = world - 1
        ok = True
        g = ReplicaGuard(a, level="weights")
        vec = (1200 - 1024) + (1800 - 1792)
        mat = 1024 + 512
        # identical replicas pass; the count is in 32-bit words: bf16 shadow of both groups + fp32 params of the vectors
        ok &= g.check() == (mat + vec) // 2 + vec
        ok &= g.check(level="state") == (mat + vec) // 2 + 3 * (mat + vec)
        ok &= calls[0] == 2 and g.checks == 2  # ONE collective per clean check
        # one bf16 element of the shadow, lowest mantissa bit, on the last rank only
        if rank == last:
            a.shadow.view(torch.int16)[700] ^= 1
        ok &= _expect_drift(g, "weights", "shadow", "g0", 700, [last], "g0.w1")
        ok &= _expect_drift(g, "state", "shadow", "g0", 700, [last], "g0.w1")
        if rank == last:
            a.shadow.view(torch.int16)[700] ^= 1
        ok &= g.check() > 0
        # one fp32 word of v on rank 0 only: every OTHER rank then disagrees with rank 0; level "weights" does not look
        if rank == 0:
            a.v.view(torch.int32)[1500] ^= 1
        ok &= g.check(level="weights") > 0
        ok &= _expect_drift(g, "state", "v", "g1", 1500, list(range(1, world)), "g1.w")
        if rank == 0:
            a.v.view(torch.int32)[1500] ^= 1
        ok &= g.check(level="state") > 0
        # sharded update with stale slices: matrix ranges of params / m / v differ by design and are not reported ...
        z = a.zero1 = ShardedUpdate(a)
        z.stale = True
        for buf in (a.params, a.m, a.v):
            buf[0:1024] += float(rank + 1)
            buf[1280:1792] -= float(rank + 1)
        ok &= g.check(level="state") == (mat + vec) // 2 + 3 * vec
        ok &= g.check(level="weights") == (mat + vec) // 2 + vec
        # ... differing vector regions are
        if rank == last:
            a.m.view(torch.int32)[1795] ^= 1 << 20
        ok &= _expect_drift(g, "state", "m", "g1", 1795, [last], "g1.b")
        if rank == last:
            a.m.view(torch.int32)[1795] ^= 1 << 20
            a.params.view(torch.int32)[1100] ^= 1
        ok &= _expect_drift(g, "weights", "params", "g0", 1100, [last], "g0.b")
        if rank == last:
            a.params.view(torch.int32)[1100] ^= 1
        # once the state has been gathered the matrix ranges count again
        z.stale = False
        ok &= _expect_drift(g, "state", "params", "g0", 0, list(range(1, world)), "g0.w0")
        a.zero1 = None
        a2 = _toy_arena()
        # every = 3: checks on iterations 3, 6, ...; every = None: no collective at all
        g3 = ReplicaGuard(a2, every=3)
        calls[0] = 0
        seen = []
        for it in range(1, 8):
            r = g3.tick()
            seen.append(r is not None)
        ok &= seen == [False, False, True, False, False, True, False] and calls[0] == 2 and g3.checks == 2 and g3.iteration == 7
        g0 = ReplicaGuard(a2)
        calls[0] = 0
        for it in range(5):
            ok &= g0.tick() is None
        ok &= calls[0] == 0 and g0.checks == 0
        # the alarm carries the iteration it was raised in
        if rank == last:
            a2.shadow.view(torch.int16)[1300] ^= 1
        g1 = ReplicaGuard(a2, every=2)
        ok &= g1.tick() is None
        try:
            g1.tick()
            ok = False
        except Exception as e:
            ok &= type(e).__name__ == "ReplicaDrift" and e.iteration == 2 and "iteration 2" in str(e) and e.param == "g1.w"
        dist.barrier()
        # a check that user code might reach on one rank only (save_training_state under ``if rank == 0:``) goes through a
        # rendezvous first: the lone rank gets an error that says what to do, the group is not hung, the next call works
        g5 = ReplicaGuard(_toy_arena(), level="state")
        if rank == 0:
            os.environ["XGGM_COLLECTIVE_TIMEOUT"] = "1.5"
            try:
                g5.check("checkpoint", rendezvous=True)
                ok = False
            except RuntimeError as e:
                ok &= "COLLECTIVE" in str(e) and "1 of %d ranks" % world in str(e) and "save_training_state" in str(e)
            os.environ.pop("XGGM_COLLECTIVE_TIMEOUT")
        else:
            g5._calls = 1  # (the call rank 0 made alone)
        dist.barrier()
        ok &= g5.check("checkpoint", rendezvous=True) > 0 and g5.checks == 1
        q.put((rank, bool(ok)))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 4])
def test_replica_guard_over_gloo(world):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_guard_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        res = [q.get(timeout=180) for _ in range(world)]  # a rank left alone in a collective would end here
    finally:
        for p in procs:
            p.join(60)
            if p.is_alive():
                p.terminate()
    assert sorted(res) == [(r, True) for r in range(world)]


def test_guard_without_a_process_group_compares_nothing():
    from xggm_amd.dist import ReplicaGuard
    g = ReplicaGuard(_toy_arena(), every=1, level="state")
    assert g.world == 1 and g.tick() == 0 and g.checks == 0
    with pytest.raises(ValueError):
        ReplicaGuard(_toy_arena(), level="everything")
    with pytest.raises(ValueError):
        ReplicaGuard(_toy_arena(), every=0)
