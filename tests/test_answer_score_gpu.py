"""The sweep score on the GPU: ``ops.answer_score`` (xggm_answer_score) against its numpy restatement ``answers.score_host``
(which tests/test_answer_score_cpu.py holds to the evaluators) -- the int64 words bit for bit --, inside canary buffers, and
the flags."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
CHUNK = 1024  # XGGM_SCORE_CHUNK
A = 29
SENTINEL = 0x5A5A5A5A5A5A5A5A


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _case(n, K, G, seed=0, extra=5):
    """tables of n + extra samples (so that the identity order fits) and a sweep of n positions.  Scores: random mantissas at
    exponents 2^-40 .. 2^10, so that another order of addition shows in the bits of the fp64 sums (soft scores 0.3 / 0.6 /
    0.9 / 1 would add exactly at these sizes).  Row 0 has no label at all; about half the logged labels match a slot of
    their sample, the others are arbitrary answers (some match by chance, most match nothing)."""
    rng = np.random.default_rng([seed, n, K, G])
    n_q = n + extra
    q_label = np.full((n_q, K), -1, dtype=np.int32)
    for s in range(1, n_q):
        used = int(rng.integers(0, K + 1)) if s > 1 else K
        q_label[s, :used] = rng.choice(A, size=used, replace=False)
    q_score = ((rng.random((n_q, K)) + 1.0) * 2.0 ** rng.integers(-40, 11, (n_q, K))).astype(np.float32)
    order = rng.integers(0, n_q, n).astype(np.int64)  # samples repeat
    order[0] = 0
    keep = (rng.random(n) < 0.7).astype(np.uint8)
    groups = rng.integers(0, max(G, 1), n_q).astype(np.int32)
    labels = {}
    for name, smp in (("order", order), ("identity", np.arange(n))):
        lab = rng.integers(0, A, n).astype(np.int64)
        for i in range(0, n, 2):
            row = q_label[smp[i]]
            if (row >= 0).any():
                lab[i] = rng.choice(row[row >= 0])
        labels[name] = lab
    return dict(q_label=q_label, q_score=q_score, order=order, keep=keep, groups=groups, labels=labels, n_q=n_q)


def _dev(c):
    return {k: torch.from_numpy(v).to(DEV) for k, v in c.items() if isinstance(v, np.ndarray)}


@pytest.mark.parametrize("n", [1, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 17])
def test_answer_score_equals_the_host_restatement(n):
    """``torch.equal`` on the words for K in {1, 3, 10}, G in {none, 1, 3, 16}, with and without ``order`` (repeats) and
    ``keep``: counts, flags and the bit patterns of the fp64 sums -- the sums' order is the one xggm.h writes down"""
    from xggm_amd import ops
    from xggm_amd.answers import score_host
    differs = 0
    for K in (1, 3, 10):
        for G in (0, 1, 3, 16):
            c = _case(n, K, G)
            d = _dev(c)
            ws = ops.answer_score_workspace(n, G, DEV)
            for use_order in (False, True):
                lab = c["labels"]["order" if use_order else "identity"]
                d_lab = torch.from_numpy(lab).to(DEV)
                for use_keep in (False, True):
                    got = ops.answer_score(d_lab, d["q_label"], d["q_score"], order=d["order"] if use_order else None,
                                           keep=d["keep"] if use_keep else None, q_group=d["groups"] if G else None, G=G, ws=ws)
                    want = score_host(lab, c, order=c["order"] if use_order else None, keep=c["keep"] if use_keep else None,
                                      groups=c["groups"] if G else None, G=G)
                    assert got.shape == (3 + 2 * G,) and torch.equal(got.cpu(), want), (n, K, G, use_order, use_keep, got.cpu(), want)
                    assert int(want[0]) == 0 and int(want[1]) == (int(c["keep"].sum()) if use_keep else n)
                    if G:
                        assert int(want[2:2 + G].sum()) == int(want[1])
                    if n > 64 and not use_keep:  # the inputs tell the orders of addition apart (not a vacuous comparison)
                        smp = c["order"] if use_order else np.arange(n)
                        m = (c["q_label"][smp] == lab[:, None]) & (c["q_label"][smp] >= 0)
                        v = np.where(m.any(1), c["q_score"][smp, m.argmax(1)], 0).astype(np.float64)
                        naive = 0.0
                        for e in v:
                            naive += e
                        differs += naive != float(want[2 + G:3 + G].view(torch.float64)[0])
    assert n <= 64 or differs > 0


def test_answer_score_writes_only_its_words_and_leaves_the_workspace_ready():
    """the output words and the workspace sit inside larger sentinel-filled allocations: nothing outside the declared sizes
    changes; labels, order, keep and the tables are unchanged; two calls in a row on the same workspace give the same words"""
    from xggm_amd import _lib, ops
    from xggm_amd.answers import score_host
    n, K, G = 2 * CHUNK + 300, 3, 3
    c = _case(n, K, G, seed=1)
    d = _dev(c)
    d_lab = torch.from_numpy(c["labels"]["order"]).to(DEV)
    inputs = dict(d, labels=d_lab)
    before = {k: v.clone() for k, v in inputs.items()}
    words = _lib.lib.xggm_answer_score_workspace_bytes(n, G) // 8
    assert words == 2 + 3 * (3 + 2 * G)
    W, lead = 3 + 2 * G, 3
    out_big = torch.full((lead + W + 4,), SENTINEL, dtype=torch.int64, device=DEV)
    ws_big = torch.full((lead + words + 4,), SENTINEL, dtype=torch.int64, device=DEV)
    ws = ws_big[lead:lead + words]
    ws[0] = 0  # the one word the contract wants zero at the first launch
    want = score_host(c["labels"]["order"], c, order=c["order"], keep=c["keep"], groups=c["groups"], G=G)
    for call in range(2):
        out_big[lead:lead + W] = SENTINEL
        got = ops.answer_score(d_lab, d["q_label"], d["q_score"], order=d["order"], keep=d["keep"], q_group=d["groups"], G=G,
                               out=out_big[lead:lead + W], ws=ws)
        assert torch.equal(got.cpu(), want), call
        assert int(ws[0]) == 0
        for big, size in ((out_big, W), (ws_big, words)):
            assert bool((big[:lead] == SENTINEL).all()) and bool((big[lead + size:] == SENTINEL).all())
    for k, v in inputs.items():
        assert torch.equal(v, before[k]), k
    with pytest.raises(RuntimeError, match="workspace holds"):
        ops.answer_score(d_lab, d["q_label"], d["q_score"], ws=ws[:4])
    for bad in (dict(G=3), dict(q_group=d["groups"]), dict(G=17, q_group=d["groups"]), dict(n=0), dict(n=n + 1), dict(n_q=c["n_q"] + 1),
                dict(order=d["order"][:n - 1]), dict(keep=d["keep"].to(torch.int32))):
        with pytest.raises((ValueError, TypeError)):
            ops.answer_score(d_lab, d["q_label"], d["q_score"], **bad)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.answer_score(d_lab.cpu(), d["q_label"], d["q_score"])


def test_answer_score_flags():
    """a cursor that is not n raises bit 0; sample indices and group ids beyond what the launch is TOLD of -- the tables are
    larger than declared, so a kernel without the check would read valid memory and give another sum -- raise bit 1 and
    contribute nothing; ``decode_score`` refuses both"""
    from xggm_amd import ops
    from xggm_amd.answers import decode_score, score_host
    n, K, G = CHUNK + 200, 3, 5
    c = _case(n, K, G, seed=2)
    d = _dev(c)
    lab = c["labels"]["order"]
    d_lab = torch.from_numpy(lab).to(DEV)
    cursor = torch.tensor([n], dtype=torch.int64, device=DEV)
    kw = dict(order=d["order"], q_group=d["groups"], G=G)
    ok = ops.answer_score(d_lab, d["q_label"], d["q_score"], cursor=cursor, **kw).cpu()
    assert int(ok[0]) == 0 and torch.equal(ok, score_host(lab, c, order=c["order"], groups=c["groups"], G=G, cursor=n))
    cursor.fill_(n - 1)
    off = ops.answer_score(d_lab, d["q_label"], d["q_score"], cursor=cursor, **kw).cpu()
    assert int(off[0]) == 1 and torch.equal(off[1:], ok[1:])
    with pytest.raises(RuntimeError, match="cursor"):
        decode_score(off, G)
    # fewer samples than the tables hold
    n_q = c["n_q"] // 2
    inside = c["order"] < n_q
    assert 0 < inside.sum() < n
    got = ops.answer_score(d_lab, d["q_label"], d["q_score"], n_q=n_q, **kw).cpu()
    assert int(got[0]) == 2 and int(got[1]) == int(inside.sum())
    assert torch.equal(got, score_host(lab, c, order=c["order"], groups=c["groups"], G=G, n_q=n_q))
    clean = score_host(lab[inside], c, order=c["order"][inside], groups=c["groups"], G=G)  # the same sweep without the offenders
    assert torch.equal(got[1:2 + G], clean[1:2 + G])
    # fewer groups than the table holds
    G2 = 3
    inside = c["groups"][c["order"]] < G2
    assert 0 < inside.sum() < n
    got = ops.answer_score(d_lab, d["q_label"], d["q_score"], order=d["order"], q_group=d["groups"], G=G2).cpu()
    assert int(got[0]) == 2 and int(got[1]) == int(inside.sum())
    assert torch.equal(got, score_host(lab, c, order=c["order"], groups=c["groups"], G=G2))
    with pytest.raises(RuntimeError, match="out of range"):
        decode_score(got, G2)
    # a negative sample index
    neg = c["order"].copy()
    neg[5] = -1
    got = ops.answer_score(d_lab, d["q_label"], d["q_score"], order=torch.from_numpy(neg).to(DEV)).cpu()
    assert int(got[0]) == 2 and int(got[1]) == n - 1 and torch.equal(got, score_host(lab, c, order=neg))
