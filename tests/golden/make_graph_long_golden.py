"""Generator fixtures with more than 64 objects, from the reference's own generator classes.

Runs only where the reference is importable (make_golden.py, imported below, stops with its own message where it is
not; the GPU box has none).  ``generator_case`` of make_golden.py is reused by import: same seeded parameters
(``synth.seeded_param``), same inputs (``synth.generator_inputs``), same probes and gradient summary as the 36- and
64-object fixtures, so tests/test_graph_long_cpu.py and tests/test_graph_long_gpu.py read them exactly as
test_oracle_golden.py / test_model_gpu.py read those.  Only the recorded arrays are committed:

    gen_gcn100.npz   GCN, H 128, N 100, B 2, 2 layers   (the 100-box features: 7 row tiles of 16, a ragged second half)
    gen_gin72.npz    GIN, H 128, N 72,  B 2, 2 layers   (8 neighbours beyond the first 64)
    gen_gat128.npz   GAT, H 64,  N 128, B 2, 1 layer    (the largest graph; two full halves)

    python tests/golden/make_graph_long_golden.py
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import make_golden as MG  # noqa: E402  (imports the reference; SystemExit where it cannot)

CASES = (("gen_gcn100", "GCN", 128, 100, 2, 2, 21),
         ("gen_gin72", "GIN", 128, 72, 2, 2, 22),
         ("gen_gat128", "GAT", 64, 128, 2, 1, 23))

if __name__ == "__main__":
    MG.torch.manual_seed(0)
    limit = os.path.getsize(os.path.join(MG.HERE, "gen_gat36.npz"))  # the largest fixture so far
    for case in CASES:
        MG.generator_case(*case)
        size = os.path.getsize(os.path.join(MG.HERE, case[0] + ".npz"))
        assert size < limit, "%s.npz: %d bytes, not below gen_gat36.npz (%d)" % (case[0], size, limit)
        print(case[0], size, "bytes")
