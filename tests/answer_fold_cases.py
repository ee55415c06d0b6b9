"""The cases the answer-log fold is tested on (tests/test_answer_fold_cpu.py, tests/test_answer_fold_gpu.py): worlds 1, 2
and 3; INTERLEAVE with block 1 and block 4 at 1 step and at 3 steps; CONCAT with uneven counts, an empty rank, a rank of
300 answers (more than one workgroup of 256 destinations) and odd totals and capacities, behind which a scores region is
only 4-byte aligned."""
import numpy as np

CONCAT, INTERLEAVE = 0, 1


def _il(world, block, steps):
    return dict(id="interleave_w%d_b%d_s%d" % (world, block, steps), layout=INTERLEAVE, block=block, expect=(block * steps,) * world,
                capacity=block * steps + (1 if world == 2 else 0))


CASES = [dict(id="concat_5_4", layout=CONCAT, expect=(5, 4), capacity=5),             # total 9: odd
         dict(id="concat_0_3_2", layout=CONCAT, expect=(0, 3, 2), capacity=4),
         dict(id="concat_300_1", layout=CONCAT, expect=(300, 1), capacity=300),       # two workgroups; total 301
         dict(id="concat_odd_capacity", layout=CONCAT, expect=(2, 4, 1), capacity=7),  # total 7, source scores at an odd word
         dict(id="concat_w1", layout=CONCAT, expect=(6,), capacity=9),
         dict(id="concat_3_0_0", layout=CONCAT, expect=(3, 0, 0), capacity=3)]
CASES += [_il(w, b, s) for w in (1, 2, 3) for b in (1, 4) for s in (1, 3)]


def expect_of(case):
    return [int(e) for e in case["expect"]]


def packed_logs(case, with_scores, seed=0):
    """the ranks' packed logs as ``engine.AnswerLog`` lays them out -- [cursor, score_sum, flags, labels[capacity], scores] --
    with EVERY slot of every rank filled (the ones behind a rank's count too: they must not travel) -> (bufs [world, words]
    int64, labels per rank [capacity], scores per rank [capacity])"""
    from xggm_amd.answers import packed_words
    expect, cap = expect_of(case), int(case["capacity"])
    rng = np.random.default_rng([seed, len(expect), cap, int(with_scores)])
    bufs = np.zeros((len(expect), packed_words(cap, with_scores)), dtype=np.int64)
    labels, scores = [], []
    for r, n in enumerate(expect):
        lab = rng.integers(0, 3129, cap) + 10000 * (r + 1)  # a rank's labels are recognisable
        labels.append(lab)
        bufs[r, 0] = n
        bufs[r, 3:3 + cap] = lab
        sc = None
        if with_scores:
            sc = rng.choice(np.array([0.0, 0.3, 0.6, 0.9, 1.0], dtype=np.float32), cap)
            bufs[r, 3 + cap:].view(np.float32)[:cap] = sc
            # what the appends would have accumulated: fp64, row order, order-sensitive across the ranks
            bufs[r, 1:2].view(np.float64)[0] = np.cumsum(sc[:n].astype(np.float64))[-1] * (1.0 + 2.0 ** -40 * r) if n else 0.0
        scores.append(sc)
    return bufs, labels, scores
