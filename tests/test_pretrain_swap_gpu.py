"""The matched-sentence swap on the GPU (xggm_pretrain_swap, ``ops.pretrain_swap``, ``DeviceFeatures(match_rate=)``): the
reference's own decisions on recorded draws (tests/golden/pretrain_swap.npz), the numpy rule at the shapes where the kernel
changes path, the degenerate pool, pass-through rows, the NULL pool, the Philox path against the exported draws and under
graph replay, and the distribution of what it draws.  Every comparison of outputs is ``torch.equal``: the kernel decides
in the reference's arithmetic and moves rows, it rounds nothing."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import pretrain_mask_ref as R  # noqa: E402
from helpers import load_golden  # noqa: E402
from test_pretrain_swap_cpu import DIST_B, DIST_SEED, SID, TRIES, dist_case, swap_rule  # noqa: E402

DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def sentences(n, T, seed):
    """n distinct rows of ids and masks: [CLS] words [SEP] of seeded lengths, the row number in position 1"""
    r = np.random.default_rng(seed)
    ids, mask = np.zeros((n, T), dtype=np.int64), np.zeros((n, T), dtype=np.int64)
    for j in range(n):
        L = int(r.integers(3, T + 1))
        ids[j, :L], mask[j, :L] = r.integers(5, 263, size=L), 1
        ids[j, 0], ids[j, 1], ids[j, L - 1] = 2, 1000 + j, 3
    return ids, mask


def check(out, idx, matched, exhausted, pool_ids, pool_mask, ids, mask):
    torch.cuda.synchronize()
    swapped = matched == 0
    want_ids = np.where(swapped[:, None], pool_ids[idx], ids)
    want_mask = np.where(swapped[:, None], pool_mask[idx], mask)
    assert out["input_ids"].dtype == out["input_mask"].dtype == out["is_matched"].dtype == torch.int64
    assert torch.equal(out["input_ids"], dev(want_ids)) and torch.equal(out["input_mask"], dev(want_mask))
    assert torch.equal(out["is_matched"], dev(matched))
    assert out["exhausted"].dtype == torch.int32 and int(out["exhausted"]) == exhausted


def test_golden_draws_give_the_reference():
    """LXMERTTorchDataset.__getitem__ on the recorded stream: which sentence each example came back with, and is_matched"""
    from xggm_amd import ops
    g = load_golden("pretrain_swap")
    B = int(g["cfg"][0])
    ids, mask, img = g["pool_ids"][:B], g["pool_mask"][:B], g["pool_img"][:B]
    out = ops.pretrain_swap(dev(ids), dev(mask), dev(img), float(g["rate"][0]),
                            pool=(dev(g["pool_ids"]), dev(g["pool_mask"]), dev(g["pool_img"])),
                            draws=dict(u_swap=dev(g["u_swap"]), u_pick=dev(g["u_pick"])))
    check(out, g["sent_index"], g["is_matched"], 0, g["pool_ids"], g["pool_mask"], ids, mask)
    assert g["is_matched"].tolist() == [1, 0, 0, 0, 1, 0]


@pytest.mark.parametrize("T,shift", [(7, 0), (8, 0), (8, 1)])
def test_element_and_vector_paths_against_the_rule(T, shift):
    """B = 9 rows (three workgroups of four waves, the last one partly empty) over 4 images, a pool of 13: T = 7 moves
    elements, T = 8 moves 16-byte vectors, T = 8 in buffers shifted by one int64 moves elements again; the outputs sit in
    sentinel-filled, over-allocated buffers and ``matched_in`` holds a 0 and a 2"""
    from xggm_amd import ops
    B, Pn, PAD, seed = 9, 13, 16, 31
    r = np.random.default_rng(seed)
    pool_ids, pool_mask = sentences(Pn, T, seed)
    ids, mask = sentences(B, T, seed + 1)
    ids[:, 1] += 500
    pool_img, img = r.integers(0, 4, size=Pn).astype(np.int64), r.integers(0, 4, size=B).astype(np.int64)
    matched_in = np.ones(B, dtype=np.int64)
    matched_in[2], matched_in[5] = 0, 2
    u_swap, u_pick = r.random(B, dtype=np.float32), r.random((B, TRIES), dtype=np.float32)
    u_swap[[2, 5]] = 0.0  # would swap if the row were looked at
    idx, matched, exhausted = swap_rule(u_swap, u_pick, img, pool_img, matched_in)
    assert 2 <= int((matched == 0).sum()) <= B - 3 and matched[2] == 0 and idx[2] == 2 and matched[5] == 2

    def shifted(x):  # a copy of x that starts ``shift`` int64 behind a 16-byte boundary
        big = torch.empty(x.size + 2, dtype=torch.int64, device=DEV)
        big[shift:shift + x.size] = dev(x).reshape(-1)
        return big[shift:shift + x.size].view(x.shape)

    big = {k: torch.full((B * T + 2 * PAD,), -7777, dtype=torch.int64, device=DEV) for k in ("input_ids", "input_mask")}
    out = {k: v[PAD + shift:PAD + shift + B * T].view(B, T) for k, v in big.items()}
    out["is_matched"] = torch.full((B + 2,), -7777, dtype=torch.int64, device=DEV)[1:B + 1]
    out["exhausted"] = torch.zeros(1, dtype=torch.int32, device=DEV)
    got = ops.pretrain_swap(shifted(ids), shifted(mask), dev(img), 0.5, matched_in=dev(matched_in),
                            pool=(shifted(pool_ids), shifted(pool_mask), dev(pool_img)), draws=dict(u_swap=dev(u_swap), u_pick=dev(u_pick)),
                            out=out)
    want_matched = matched.copy()
    torch.cuda.synchronize()
    swapped = (matched == 0) & (matched_in == 1)
    assert torch.equal(got["input_ids"], dev(np.where(swapped[:, None], pool_ids[idx], ids)))
    assert torch.equal(got["input_mask"], dev(np.where(swapped[:, None], pool_mask[idx], mask)))
    assert torch.equal(got["is_matched"], dev(want_matched)) and int(got["exhausted"]) == exhausted
    for k, v in big.items():  # nothing outside the outputs was written
        assert bool((v[:PAD + shift] == -7777).all()) and bool((v[PAD + shift + B * T:] == -7777).all()), k


def test_pool_of_one_image_is_counted_not_hung():
    """P = 1 and the pool's image is the row's own: all eight candidates fail, the row stays, is_matched = 1, exhausted == 1;
    a second call adds to the counter (it only ever grows)"""
    from xggm_amd import ops
    ids, mask = sentences(1, 7, 3)
    pool_ids, pool_mask = sentences(1, 7, 4)
    img = dev(np.array([5], dtype=np.int64))
    draws = dict(u_swap=torch.zeros(1, device=DEV), u_pick=torch.rand(1, TRIES, device=DEV))
    out = ops.pretrain_swap(dev(ids), dev(mask), img, 0.5, pool=(dev(pool_ids), dev(pool_mask), img.clone()), draws=draws)
    check(out, np.zeros(1, dtype=np.int64), np.ones(1, dtype=np.int64), 1, pool_ids, pool_mask, ids, mask)
    ops.pretrain_swap(dev(ids), dev(mask), img, 0.5, pool=(dev(pool_ids), dev(pool_mask), img.clone()), draws=draws, out=out)
    torch.cuda.synchronize()
    assert int(out["exhausted"]) == 2


def test_unmatched_rows_pass_through():
    from xggm_amd import ops
    B, T = 5, 8
    ids, mask = sentences(B, T, 9)
    img = np.arange(B, dtype=np.int64)
    out = ops.pretrain_swap(dev(ids), dev(mask), dev(img), 1.0, matched_in=torch.zeros(B, dtype=torch.int64, device=DEV),
                            draws=dict(u_swap=torch.zeros(B, device=DEV), u_pick=torch.rand(B, TRIES, device=DEV)))
    check(out, np.arange(B), np.zeros(B, dtype=np.int64), 0, ids, mask, ids, mask)
    assert torch.equal(out["input_ids"], dev(ids))


def test_null_pool_is_the_batch():
    from xggm_amd import ops
    B, T, seed = 12, 8, 17
    ids, mask = sentences(B, T, seed)
    img = dev(np.random.default_rng(seed).integers(0, 3, size=B).astype(np.int64))
    rng = ops.make_rng(seed, DEV)
    a = ops.pretrain_swap(dev(ids), dev(mask), img, 0.5, rng=rng, sid_base=SID)
    b = ops.pretrain_swap(dev(ids), dev(mask), img, 0.5, rng=rng, sid_base=SID, pool=(dev(ids), dev(mask), img.clone()))
    torch.cuda.synchronize()
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert 0 < int((a["is_matched"] == 0).sum()) < B


def test_philox_path_and_graph_replay():
    """draws=None draws streams sid_base + 5 / + 6 of ``rng`` -- the draws ``ops.uniform`` exports and the host restatement
    computes; ``rng`` is only read; a captured ``DeviceFeatures(match_rate=0.5)`` replays with the draws of the rng state at
    replay time, the corruption reads the swapped ids and unmatched rows get ans = -1"""
    from xggm_amd import ops
    from xggm_amd.pretrain.lxmert_pretrain import DeviceFeatures
    B, T, O, F, V, seed = 8, 8, 4, 8, 263, 77
    ids, mask = sentences(B, T, seed)
    ids[:, 1] = 5 + np.arange(B)  # inside the vocabulary
    img_np = (np.arange(B) % 3).astype(np.int64)
    b = dict(ids=dev(ids), mask=dev(mask), img=dev(img_np))
    rng = ops.make_rng(seed, DEV)
    state0 = rng.clone()

    def explicit():
        d = dict(u_swap=ops.uniform(B, rng, SID + 5), u_pick=ops.uniform(B * TRIES, rng, SID + 6))
        return ops.pretrain_swap(b["ids"], b["mask"], b["img"], 0.5, draws=d), d

    first = ops.pretrain_swap(b["ids"], b["mask"], b["img"], 0.5, rng=rng, sid_base=SID)
    e0, d0 = explicit()
    torch.cuda.synchronize()
    assert torch.equal(rng, state0)
    assert torch.equal(d0["u_swap"].cpu(), torch.from_numpy(R.philox_uniform(seed, 0, SID + 5, B)))
    assert torch.equal(d0["u_pick"].cpu(), torch.from_numpy(R.philox_uniform(seed, 0, SID + 6, B * TRIES)))
    for k in first:
        assert torch.equal(first[k], e0[k]), k
    idx, matched, exhausted = swap_rule(d0["u_swap"].cpu().numpy(), d0["u_pick"].cpu().numpy(), img_np, img_np)
    check(first, idx, matched, exhausted, ids, mask, ids, mask)

    feat = DeviceFeatures(vocab_size=V, mask_id=4, sid_base=SID, max_labels=2, match_rate=0.5)
    seg = torch.zeros_like(b["ids"])
    feats = torch.randn(B, O, F, device=DEV)
    extra = [torch.zeros(B, O, 4, device=DEV)] + [torch.zeros(B, O, device=DEV)] * 4
    ones = torch.ones(B, dtype=torch.int64, device=DEV)
    lab, sc = torch.full((B, 2), 3, dtype=torch.int64, device=DEV), torch.ones(B, 2, device=DEV)
    lab[:, 1] = -1

    def call(f):
        a = f(b["ids"], b["mask"], seg, feats, *extra, ones, lab, sc, rng, img_ids=b["img"])
        return dict(input_ids=a[0], input_mask=a[2], lm=a[3], matched=a[7], ans=a[8])

    def expect(state):
        """swap with the draws of ``state``, then the corruption of the swapped batch at the same state"""
        sw = ops.pretrain_swap(b["ids"], b["mask"], b["img"], 0.5, rng=state, sid_base=SID)
        co = ops.pretrain_corrupt(sw["input_ids"], sw["input_mask"], feats, sw["is_matched"], lab, sc, 0.15, 0.15, V, 4, rng=state,
                                  sid_base=SID)
        return dict(input_ids=co["input_ids"], input_mask=sw["input_mask"], lm=co["masked_lm_labels"], matched=sw["is_matched"],
                    ans=co["ans"])

    eager = {k: v.clone() for k, v in call(feat).items()}
    want0 = expect(rng)
    for k in eager:
        assert torch.equal(eager[k], want0[k]), k
    assert torch.equal(eager["matched"], first["is_matched"]) and bool((eager["matched"] == 0).any())
    assert bool((eager["ans"][eager["matched"] == 0] == -1).all()) and bool((eager["ans"][eager["matched"] == 1] == 3).all())
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = call(feat)
    graph.replay()
    for k in eager:
        assert torch.equal(captured[k], eager[k]), k
    ops.rng_advance(rng)
    graph.replay()
    r1 = {k: v.clone() for k, v in captured.items()}
    want1 = expect(rng)
    torch.cuda.synchronize()
    assert int(rng[1]) == 1
    for k in r1:
        assert torch.equal(r1[k], want1[k]), k
    assert not torch.equal(r1["matched"], eager["matched"])
    assert int(feat.swap_exhausted) == 0


def test_distribution():
    """B = 4096 rows over 64 images, the batch as its own pool, seed DIST_SEED (its conditions are verified on the host in
    tests/test_pretrain_swap_cpu.py): the share of swapped rows lies within 4 binomial standard deviations of 0.5 (4 sqrt(0.25
    / 4096) = 0.03125 <= 0.032), no row is exhausted (a row fails with probability about (1/64)^8), every swapped row shows
    another image -- and the kernel's decisions are the host restatement's"""
    from xggm_amd import ops
    T = 8
    img_np, u_swap, u_pick = dist_case()
    ids, mask = sentences(DIST_B, T, DIST_SEED)
    out = ops.pretrain_swap(dev(ids), dev(mask), dev(img_np), 0.5, rng=ops.make_rng(DIST_SEED, DEV), sid_base=SID)
    torch.cuda.synchronize()
    matched = out["is_matched"].cpu().numpy()
    share = float((matched == 0).mean())
    bound = 4 * math.sqrt(0.25 / DIST_B)
    print("swapped share %.4f (0.5 +- %.4f)" % (share, bound))
    assert abs(share - 0.5) <= bound <= 0.032
    assert int(out["exhausted"]) == 0
    src = out["input_ids"][:, 1].cpu().numpy() - 1000  # the row each output row came from
    assert (img_np[src[matched == 0]] != img_np[matched == 0]).all() and (src[matched == 1] == np.arange(DIST_B)[matched == 1]).all()
    idx, want, exhausted = swap_rule(u_swap, u_pick, img_np, img_np)
    check(out, idx, want, exhausted, ids, mask, ids, mask)
