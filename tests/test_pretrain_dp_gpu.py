"""Data-parallel pre-training on the GPU: the log fold kernel (xggm_train_log_fold / ``ops.train_log_fold``) against its
numpy restatement (``trainlog.fold_host``) inside sentinel bands, and the two-rank rehearsal of the captured step, the
folded log and the driver (tools/dp_pretrain_rehearsal.py: two ranks share cuda:0 over gloo)."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENTINEL = 0x5A5A5A5A5A5A5A5A
PAD = 64  # int64 words of sentinel on either side of every buffer the launch is handed


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _banded(words):
    raw = torch.full((PAD + words + PAD,), SENTINEL, dtype=torch.int64, device=DEV)
    return raw, raw[PAD:PAD + words]


def _ring(cap):
    """a log laid out as ``engine.TrainLog`` lays it out (``trainlog.words``), between two sentinel bands"""
    from xggm_amd import trainlog as T
    raw, buf = _banded(T.words(cap))
    C, K, H = T.COLS, T.KINDS, T.HEADER
    o = H + cap
    log = types.SimpleNamespace(capacity=cap, buf=buf, cursor=buf[0:1], first_bad_word=buf[1:2], counts=buf[2:2 + K],
                                sums=buf[2 + K:H].view(torch.float64).view(K, C), steps=buf[H:H + cap],
                                values=buf[o:o + cap * C // 2].view(torch.float32).view(cap, C),
                                kinds=buf[o + cap * C // 2:].view(torch.int32)[:cap])
    return raw, log


def _case(world, n, seed):
    """the ranks' copies of n records: every kind, some columns absent everywhere, all values order-sensitive in fp32"""
    from xggm_amd import trainlog as T
    rng = np.random.default_rng([seed, world, n])
    values = (rng.standard_normal((world, n, T.COLS)) * 10.0 ** rng.integers(-3, 4, (world, n, T.COLS))).astype(np.float32)
    kinds = np.tile(rng.integers(0, T.KINDS, n), (world, 1))
    present = np.tile(rng.random((n, T.COLS)) < 0.8, (world, 1, 1))
    present[:, :, 0] = True
    values[~present] = 0.0
    steps = np.tile(np.arange(11, 11 + n, dtype=np.int64), (world, 1))
    return values, kinds, present, steps


def _denan(t):
    """NaNs -> one marker, in place: that a value is NaN is the contract, which NaN is not"""
    t.copy_(torch.where(torch.isnan(t), torch.full_like(t, 12345.0), t))


VARIANTS = ("absent_and_nan", "step_first", "step_last")


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("world", [1, 2, 3])
def test_fold_equals_the_restatement_and_writes_nothing_else(world, n, variant):
    """the mean in rank order, a column absent on one rank, a NaN on one rank, a step mismatch planted at record 0 or at the
    last record: the ring rows, the recomputed sums / counts / first_bad and the flag equal ``trainlog.fold_host`` bit for
    bit, and no word outside rows [0, n) of values / kinds, the sums, the counts, first_bad and the flag changes -- the
    sentinel bands, the rest of the ring, its steps and cursor, the gathered buffers"""
    from xggm_amd import ops, trainlog as T
    cap, me = n + 2, world - 1  # this rank is the last: the ring holds ITS records before the fold
    values, kinds, present, steps = _case(world, n, 7)
    last = n - 1
    if variant == "absent_and_nan":
        values[me, last, 1] = np.nan
        present[:, last, 1] = True
        if world > 1:
            present[0, 0, 0] = False  # absent on ONE rank: absent in the result, and reported
            values[0, 0, 0] = 0.0
    elif world > 1:
        steps[0 if world == 2 else 1, 0 if variant == "step_first" else last] += 5
    want = T.fold_host(values, kinds, present, steps, cursors=[n] * world, cursor=n)
    if world == 1:
        assert want["flag"] == -1
    elif variant == "absent_and_nan":
        assert want["flag"] == 0 and not want["present"][0, 0]
    else:
        assert want["flag"] == (0 if variant == "step_first" else last)
    packed = (kinds | ((present * (1 << np.arange(T.COLS))).sum(-1) << 8)).astype(np.int32)
    # the gathered buffers, dense, each between sentinel bands
    raw_v, g_v = _banded(world * n * T.COLS // 2)
    raw_k, g_k = _banded((world * n + 1) // 2)
    raw_s, g_s = _banded(world * n)
    raw_c, g_c = _banded(world)
    raw_f, flag = _banded(1)
    g_v.view(torch.float32).copy_(torch.from_numpy(values.reshape(-1)))
    g_k.view(torch.int32)[:world * n].copy_(torch.from_numpy(packed.reshape(-1)))
    g_s.copy_(torch.from_numpy(steps.reshape(-1)))
    g_c.fill_(n)
    # the ring: this rank's own records in rows [0, n), sentinels behind them
    raw, log = _ring(cap)
    log.buf[:T.HEADER].zero_()
    log.cursor.fill_(n)
    log.first_bad_word.fill_(-1)
    log.values[:n].copy_(torch.from_numpy(values[me]))
    log.kinds[:n].copy_(torch.from_numpy(packed[me]))
    log.steps[:n].copy_(torch.from_numpy(steps[me]))
    before = [t.clone() for t in (raw_v, raw_k, raw_s, raw_c)]
    expect = raw.clone()
    e = expect[PAD:PAD + T.words(cap)]
    o = T.HEADER + cap
    e[o:o + cap * T.COLS // 2].view(torch.float32).view(cap, T.COLS)[:n].copy_(torch.from_numpy(want["values"]))
    want_packed = (want["kinds"] | ((want["present"] * (1 << np.arange(T.COLS))).sum(-1) << 8)).astype(np.int32)
    e[o + cap * T.COLS // 2:].view(torch.int32)[:n].copy_(torch.from_numpy(want_packed))
    e[2 + T.KINDS:T.HEADER].view(torch.float64).copy_(torch.from_numpy(want["sums"].reshape(-1)))
    e[2:2 + T.KINDS].copy_(torch.from_numpy(want["counts"]))
    e[1] = want["first_bad"]
    ops.train_log_fold(log, g_v.view(torch.float32), g_k.view(torch.int32), world, n, flag, steps=g_s, cursors=g_c)
    torch.cuda.synchronize()
    assert int(flag[0]) == want["flag"]
    assert torch.equal(raw_f[:PAD], torch.full_like(raw_f[:PAD], SENTINEL)) and torch.equal(raw_f[PAD + 1:], raw_f[:PAD])
    for got, was in zip((raw_v, raw_k, raw_s, raw_c), before):
        assert torch.equal(got, was)  # read only
    got_nan = torch.isnan(log.values[:n]).cpu().numpy()
    assert np.array_equal(got_nan, np.isnan(want["values"]))
    if variant == "absent_and_nan":
        assert got_nan[last, 1] and int(log.first_bad_word) == last  # a NaN on one rank is a NaN in the mean
    for buf in (raw, expect):
        b = buf[PAD:PAD + T.words(cap)]
        _denan(b[o:o + cap * T.COLS // 2].view(torch.float32)[:n * T.COLS])
        _denan(b[2 + T.KINDS:T.HEADER].view(torch.float64))
    assert torch.equal(raw, expect)  # every word: the folded rows, the header, and everything that must not move
    if world == 1:  # the identity
        assert torch.equal(log.values[:n].cpu().nan_to_num(nan=12345.0), torch.from_numpy(values[0]).nan_to_num(nan=12345.0))
        assert torch.equal(log.kinds[:n].cpu(), torch.from_numpy(packed[0]))


def test_fold_wrapper_refuses_what_would_read_past_a_buffer():
    from xggm_amd import ops
    raw, log = _ring(4)
    flag = torch.zeros(1, dtype=torch.int64, device=DEV)
    vals, kinds = torch.zeros(2 * 3 * 8, device=DEV), torch.zeros(2 * 3, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match="vals holds"):
        ops.train_log_fold(log, vals[:-1], kinds, 2, 3, flag)
    with pytest.raises(ValueError, match="kinds holds"):
        ops.train_log_fold(log, vals, kinds[:-1], 2, 3, flag)
    with pytest.raises(ValueError, match="steps holds"):
        ops.train_log_fold(log, vals, kinds, 2, 3, flag, steps=torch.zeros(5, dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError, match="records"):
        ops.train_log_fold(log, vals, kinds, 2, 5, flag)
    with pytest.raises(ValueError, match="stride"):
        ops.train_log_fold(log, vals, kinds, 2, 3, flag, strides=(23, 3, 3, 1))
    with pytest.raises(TypeError):
        ops.train_log_fold(log, vals.double(), kinds, 2, 3, flag)
    torch.cuda.synchronize()
    assert torch.equal(raw[:PAD], torch.full_like(raw[:PAD], SENTINEL))


def _free_port():
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_data_parallel_ranks_pretrain_on_one_gpu():
    """data-parallel pre-training end to end, as far as one GPU allows: two ranks (gloo rendezvous on 127.0.0.1, both on
    cuda:0, DIFFERENT halves of every global batch) on the TINY model with one layer of each kind, all four tasks on, 4
    samples per rank out of a resident store of 24.  ``tools/dp_pretrain_rehearsal.py`` asserts and prints, in order: the
    replicas are identical after 3 captured steps; captured == eager; ONE step == the single-process emulation (each rank's
    half batch run eagerly with that rank's seed, the two gradient arenas added, halved, clipped and stepped) -- which is
    what shows that the exchange happens and averages --; the folded log == the restatement over the two rings; an epoch
    of ``LXMERT.train`` and a ragged, uneven validation sweep; an overflow on rank 1 alone raises on both ranks; the
    replicas stay identical on the bf16 wire."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
                        os.path.join(root, "tools", "dp_pretrain_rehearsal.py")], capture_output=True, text=True, timeout=600,
                       env=env, cwd=root)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    out = r.stdout
    for line in ("1. replicas identical after 3 captured steps (weights, moments, step counters): True",
                 "2. captured == eager under data parallelism, bit for bit: True",
                 "3. one data-parallel step == the single-process emulation (halves differ: True), bit for bit: True",
                 "4. folded training log == the restatement over the two rings, on both ranks: True",
                 "5. LXMERT.train: rank 0's loss line == the mean of the per-rank step means: True",
                 "5. snapshots written once, by rank 0: True",
                 "5. evaluate_epoch over 9 samples (5 + 4, ragged): every uid scored exactly once: True",
                 "6. an overflow on rank 1 alone raises on both ranks at the same check(): True",
                 "7. bf16 storage, bf16 wire: replicas identical after 3 steps: True",
                 "process group shut down cleanly"):
        assert line in out, (line, out[-3000:])
    assert ": False" not in out
