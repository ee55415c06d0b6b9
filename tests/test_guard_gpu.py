"""The replica drift guard end to end, as far as one GPU allows: ``tools/dp_drift_rehearsal.py`` under
``torch.distributed.run`` with two ranks on cuda:0 (gloo), the tiny model, different batches per rank; the eager loop
(``vqacpv2.train_iteration``) and the captured engine (``CapturedTrainer.iteration``), replicated and sharded update, four
iterations each with ``check_every=1``; and the guard in ``save_training_state``."""
import os
import re
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = ["engine=%s update=%s" % (e, u) for e in ("eager", "captured") for u in ("replicated", "sharded")]


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _rehearse(*args):
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    return subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
                           os.path.join(ROOT, "tools", "dp_drift_rehearsal.py")] + list(args), capture_output=True, text=True,
                          timeout=600, env=env, cwd=ROOT)


def _digests(out):
    return sorted(re.findall(r"rank \d (engine=\S+ update=\S+): digest (.*)", out))


def test_data_parallel_replicas_pass_the_guard():
    """no alarm on healthy replicas, and the guard really ran: 4 checks per configuration on both ranks, one
    fingerprint launch per check"""
    r = _rehearse("--drift", "none", "--check-every", "1")
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "ReplicaDrift" not in r.stdout
    for rank in (0, 1):
        for c in CONFIGS:
            assert "rank %d %s: no alarm, 4 checks, 4 fingerprint launches while training" % (rank, c) in r.stdout, (rank, c)
    d = _digests(r.stdout)
    assert len(d) == 8 and all(d[2 * i] == d[2 * i + 1] for i in range(4))  # both ranks print the same weights


def test_data_parallel_drift_raises_on_every_rank():
    """Rank 1 changes one element of a named encoder tensor between iterations 2 and 3 with a plain indexed write; BOTH
    ranks must end iteration 3 with ReplicaDrift naming that tensor, in all four configurations, and the launcher must
    come back (nobody is left alone in a collective) with a non-zero status.

    What is written is the element's fp32 MASTER, not its bf16 shadow, and under the sharded update a LayerNorm weight
    instead of a matrix.  A write to the shadow alone does not survive until the check: the update of iteration 3 rewrites
    every shadow element from its master, and the masters stay identical because the gradients are summed over the ranks
    before anybody uses them -- so when the iteration's check runs the replicas are equal again and there is nothing to
    report (``test_data_parallel_shadow_write_heals_before_the_check`` shows exactly that).  Under the sharded update a
    matrix element has one owner whose result every rank receives through the all-gather, whichever rank was written to;
    only the vector regions are updated by every rank on its own and can stay apart."""
    r = _rehearse("--drift", "master", "--check-every", "1")
    out = r.stdout
    assert r.returncode != 0, out[-3000:] + r.stderr[-3000:]
    names = {"replicated": "layer.0.attention.self.query.weight", "sharded": "layer.0.attention.output.LayerNorm.weight"}
    for rank in (0, 1):
        for c in CONFIGS:
            line = [l for l in out.splitlines() if l.startswith("rank %d %s: ReplicaDrift:" % (rank, c))]
            assert len(line) == 1, (rank, c, out[-3000:] + r.stderr[-3000:])
            assert "iteration 3" in line[0] and names[c.split("update=")[1]] in line[0] and "rank(s) 1 disagree" in line[0], line[0]
        assert "rank %d: alarm alarm alarm alarm" % rank in out
    assert "no alarm" not in out


def test_data_parallel_shadow_write_heals_before_the_check():
    """the same write to the bf16 shadow element alone (lowest mantissa bit): the next update rewrites it from identical
    masters, the checks of iterations 3 and 4 find equal replicas -- on both ranks, which trained the same bits"""
    r = _rehearse("--drift", "shadow", "--check-every", "1")
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "ReplicaDrift" not in r.stdout and r.stdout.count("no alarm, 4 checks") == 8
    d = _digests(r.stdout)
    assert len(d) == 8 and all(d[2 * i] == d[2 * i + 1] for i in range(4))


def test_data_parallel_guard_is_off_by_default():
    """check_every=None: no fingerprint launch, no check, and the trained weights equal bit for bit those of a run that
    calls enable_data_parallel without the new arguments"""
    runs = {k: _rehearse("--drift", "none", "--check-every", k) for k in ("none", "absent")}
    for k, r in runs.items():
        assert r.returncode == 0, (k, r.stdout[-3000:] + r.stderr[-3000:])
        assert r.stdout.count("no alarm, 0 checks, 0 fingerprint launches while training") == 8, (k, r.stdout[-3000:])
    d_none, d_absent = _digests(runs["none"].stdout), _digests(runs["absent"].stdout)
    assert len(d_none) == 8 and d_none == d_absent


def test_data_parallel_checkpoint_is_guarded(tmp_path):
    """``save_training_state`` with a guard whose ``check_every`` (1000) never let a tick fire: healthy replicas write the
    file (every rank calls, rank 0 passes the path); after rank 1's write to an fp32 master both ranks raise ReplicaDrift
    carrying "(checkpoint)" and the parameter's name, and no file appears -- under the replicated and the sharded update"""
    r = _rehearse("--checkpoint", str(tmp_path))
    out = r.stdout
    assert r.returncode == 0, out[-3000:] + r.stderr[-3000:]
    names = {"replicated": "layer.0.attention.self.query.weight", "sharded": "layer.0.attention.output.LayerNorm.weight"}
    for mode, name in names.items():
        for rank in (0, 1):
            line = [l for l in out.splitlines() if l.startswith("rank %d checkpoint update=%s: ReplicaDrift:" % (rank, mode))]
            assert len(line) == 1 and "(checkpoint)" in line[0] and name in line[0] and "rank(s) 1 disagree" in line[0], (mode, rank, out[-3000:])
            assert "rank %d checkpoint update=%s: files written: clean True, drift False" % (rank, mode) in out
        assert (tmp_path / ("clean_%s.pt" % mode)).exists() and not (tmp_path / ("drift_%s.pt" % mode)).exists()
    assert out.count("checkpoint guard ok") == 2 and "went through" not in out
