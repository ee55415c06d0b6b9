"""The data-parallel fine-tuning drivers on the GPU: the two-rank rehearsal of ``VQA`` / ``GQA`` with ``data_parallel=True``
(tools/dp_finetune_rehearsal.py: two ranks share cuda:0 over gloo)."""
import os
import subprocess
import sys

import pytest
import torch

from test_pretrain_dp_gpu import _free_port

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def test_two_data_parallel_ranks_fine_tune_on_one_gpu():
    """the drivers end to end under data parallelism, as far as one GPU allows: two ranks (gloo rendezvous on 127.0.0.1, both
    on cuda:0) on the tiny model, a resident store of 24 training samples at 4 per rank (3 global steps, each rank its own
    rows), 9 validation samples cut 5 + 4 with one question id on both sides of the cut.  ``tools/dp_finetune_rehearsal.py``
    asserts and prints, in order, the lines below; without the feature it ends with the drivers' NotImplementedError."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
                        os.path.join(root, "tools", "dp_finetune_rehearsal.py")], capture_output=True, text=True, timeout=600,
                       env=env, cwd=root)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    out = r.stdout
    at = -1
    for line in ("1. replicas identical after one epoch of VQA.train (the ranks' rows differ: True): True",
                 "2. history, valid_scores and best_valid equal on both ranks: True",
                 "3. log.log and the BEST*.pth files written once, by rank 0: True",
                 "4. total_loss == the value rebuilt from the two rings with trainlog.fold_host: True",
                 "5. train score bit-equal to score_host over the merged labels, within 2^-24 of the evaluator: True",
                 "6. validation (5 + 4): every question scored once, merged labels == the ranks' own in slice order, the score "
                 "bit-equal on both ranks: True",
                 "7. predict(dump=) writes one file, the same dict on both ranks: True",
                 "8. a refused-append flag on rank 1 alone raises on both ranks at the same fold: True",
                 "9. the GQA driver (GGM pass first, valid_factor 2) completes one epoch with equal replicas: True",
                 "10. without data_parallel=True the prepared model is still refused: True",
                 "process group shut down cleanly"):
        assert line in out, (line, out[-3000:])
        assert out.index(line) > at, line  # in order
        at = out.index(line)
    assert ": False" not in out
