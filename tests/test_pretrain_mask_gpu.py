"""Pre-training batch masking on the GPU (xggm_pretrain_corrupt_*, ``ops.pretrain_corrupt``, ``DeviceFeatures``): the
reference's own outputs on recorded draws (tests/golden/pretrain_mask.npz), the float64 restatement
(tests/pretrain_mask_ref.py) at the shapes where the kernel changes path, the Philox path against the exported draws and
under graph replay, the distribution of what it draws, and LXRTPretraining fed by it.  Every comparison of outputs is
``torch.equal``: the kernel decides in the reference's arithmetic and moves rows, it rounds nothing."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import pretrain_mask_ref as R  # noqa: E402
from helpers import load_golden  # noqa: E402
from test_pretrain_mask_cpu import DRAWS, OUT, golden_case  # noqa: E402

DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
SID = 0x70726500
CLS, SEP, MASK = 2, 3, 4


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def make_batch(B, T, O, F, seed, V=263, K=3, n_ans=19, lengths=None):
    """a clean batch in numpy: [CLS] words [SEP] padded to T with the lengths T, 2, 3 first (then seeded), normal features,
    every answer case (several keys, one, none, unmatched with a label, then seeded)"""
    r = np.random.default_rng(seed)
    L = list(lengths) if lengths is not None else [T, 2, 3][:B] + [int(x) for x in r.integers(2, T + 1, size=max(B - 3, 0))]
    ids, mask = np.zeros((B, T), dtype=np.int64), np.zeros((B, T), dtype=np.int64)
    for b in range(B):
        ids[b, 0], ids[b, L[b] - 1], mask[b, :L[b]] = CLS, SEP, 1
        ids[b, 1:L[b] - 1] = r.integers(5, V, size=L[b] - 2)
    feats = r.standard_normal((B, O, F), dtype=np.float32)
    matched = r.integers(0, 2, size=B).astype(np.int64)
    lab = np.full((B, K), -1, dtype=np.int64)
    sc = np.zeros((B, K), dtype=np.float32)
    for b in range(B):
        n = (K, 1, 0, 1)[b] if b < 4 else int(r.integers(0, K + 1))
        lab[b, :n] = r.choice(n_ans, size=n, replace=False)
        sc[b, :n] = r.random(n, dtype=np.float32) + np.float32(0.1)
    matched[:3] = 1
    if B > 3:
        matched[3] = 0
    return dict(input_ids=ids, input_mask=mask, feats=feats, is_matched=matched, label_ids=lab, label_scores=sc)


def host_draws(seed, offset, B, T, O, sid=SID):
    n = dict(u_word=B * T, u_word_pick=B * T, u_obj=B * O, u_obj_pick=B * O, u_ans=B)
    return {k: R.philox_uniform(seed, offset, sid + i, n[k]) for i, k in enumerate(DRAWS)}


def dev(x, dt=None):
    t = torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    return t.to(dt) if dt is not None and t.is_floating_point() else t


def corrupt(ops, b, feats, rates, V, **kw):
    return ops.pretrain_corrupt(b["input_ids"], b["input_mask"], feats, b["is_matched"], b["label_ids"], b["label_scores"],
                                rates[0], rates[1], V, MASK, **kw)


def check(got, want, dt, tag=""):
    for k in OUT:
        w = dev(want[k], dt if k == "masked_feat" else None)
        assert got[k].dtype == w.dtype and got[k].shape == w.shape, (tag, k)
        assert torch.equal(got[k], w), (tag, k)


@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("c", [0, 1])
def test_golden_draws_give_the_reference(c, dt):
    """the reference's random_word / random_feat / convert_example_to_features on the recorded draws, thresholds included;
    bf16: the features of the bf16-rounded inputs (a moved row is rounded before or after the move alike)"""
    from xggm_amd import ops
    g = load_golden("pretrain_mask")
    (ids, mask, feats, matched, lab, sc, d), kw, want = golden_case(g, c)
    out = ops.pretrain_corrupt(dev(ids), dev(mask), dev(feats, dt), dev(matched), dev(lab), dev(sc), kw["word_mask_rate"],
                               kw["obj_mask_rate"], kw["vocab_size"], kw["mask_id"], pool=dev(kw["pool"], dt),
                               draws={k: dev(v) for k, v in d.items()})
    torch.cuda.synchronize()
    check(out, want, dt, "golden %d" % c)


SHAPES = [(2048, 0), (24, 0), (24, 1), (10, 0)]  # (F, elements the feature buffers are shifted by): F=10 and a shifted base take the scalar path


@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("F,shift", SHAPES)
def test_shape_edges_against_the_restatement(F, shift, dt):
    """B = 2, T = 20, O = 36: 72 rows (more than one workgroup), two 16-byte vectors per thread (F = 2048 fp32), fewer vectors
    than threads (F = 24), no whole vector (F = 10) and a base that is not 16-byte aligned; rates of 0.5 so that 72 rows and
    ~20 words show every outcome; outputs inside sentinel-filled, over-allocated buffers"""
    from xggm_amd import ops
    B, T, O, V, rates, PAD = 2, 20, 36, 263, (0.5, 0.5), 64
    seed = {2048: 2079, 24: 58, 10: 41}[F]  # seeds at which the ~20 words show every outcome (asserted below)
    nb = make_batch(B, T, O, F, seed, V, lengths=[T, 3 if F != 24 else 2])
    rng = ops.make_rng(seed, DEV)
    d = {k: ops.uniform(n, rng, SID + i) for i, (k, n) in enumerate(zip(DRAWS, (B * T, B * T, B * O, B * O, B)))}
    hd = host_draws(seed, 0, B, T, O)
    for k in DRAWS:
        assert torch.equal(d[k].cpu(), torch.from_numpy(hd[k])), k  # xggm_uniform IS philox_uniform of common.h
    feats = dev(nb["feats"], dt)
    src = torch.empty(feats.numel() + PAD, device=DEV, dtype=dt)
    src[shift:shift + feats.numel()] = feats.reshape(-1)
    feats_in = src[shift:shift + feats.numel()].view(B, O, F)
    want = R.corrupt(nb["input_ids"], nb["input_mask"], feats.float().cpu().numpy(), nb["is_matched"], nb["label_ids"],
                     nb["label_scores"], hd, rates[0], rates[1], V, MASK)
    assert set(want["obj_kind"].reshape(-1).tolist()) == {0, 1, 2, 3}
    assert set(want["word_kind"][want["word_kind"] >= 0].tolist()) == {0, 1, 2, 3}
    sentinel = dict(input_ids=-7777, masked_lm_labels=-7777, masked_feat=123.25, feat_mask=123.25, ans=-7777)
    sizes = dict(input_ids=B * T, masked_lm_labels=B * T, masked_feat=B * O * F, feat_mask=B * O, ans=B)
    dts = dict(input_ids=torch.int64, masked_lm_labels=torch.int64, masked_feat=dt, feat_mask=F32, ans=torch.int64)
    big = {k: torch.full((sizes[k] + 2 * PAD,), sentinel[k], device=DEV, dtype=dts[k]) for k in OUT}
    off = {k: PAD + (shift if k == "masked_feat" else 0) for k in OUT}
    out = {k: big[k][off[k]:off[k] + sizes[k]] for k in OUT}
    out["masked_feat"] = out["masked_feat"].view(B, O, F)
    b = {k: dev(v) for k, v in nb.items()}
    got = corrupt(ops, b, feats_in, rates, V, draws=d, out=out)
    torch.cuda.synchronize()
    check({k: got[k].reshape(want[k].shape) for k in OUT}, want, dt, "F=%d" % F)
    for k in OUT:  # nothing outside the outputs was written
        assert bool((big[k][:off[k]] == sentinel[k]).all()) and bool((big[k][off[k] + sizes[k]:] == sentinel[k]).all()), k
    zero = torch.from_numpy(want["obj_kind"] == 1).to(DEV)
    raw = got["masked_feat"].view(torch.int32 if dt == F32 else torch.int16)
    assert bool(zero.any()) and bool((raw[zero] == 0).all())  # zeroed rows are +0 bits, not -0 and not small numbers
    assert torch.equal(src[shift:shift + feats.numel()], feats.reshape(-1))  # the clean features are only read


def test_philox_path_and_graph_replay():
    """draws=None draws stream sid_base + k of ``rng`` -- the draws ``ops.uniform`` exports; the kernel does not advance
    ``rng``; a captured call replays with the draws of the rng state at replay time"""
    from xggm_amd import ops
    from xggm_amd.pretrain.lxmert_pretrain import DeviceFeatures
    B, T, O, F, V, seed = 4, 20, 36, 24, 263, 77
    nb = make_batch(B, T, O, F, seed, V)
    b = {k: dev(v) for k, v in nb.items()}
    seg = torch.zeros_like(b["input_ids"])
    extra = [torch.zeros(B, O, 4, device=DEV)] + [torch.zeros(B, O, device=DEV)] * 4  # boxes, obj / attr labels and confidences
    rng = ops.make_rng(seed, DEV)
    feat = DeviceFeatures(vocab_size=V, mask_id=MASK, sid_base=SID, max_labels=3)

    def call(f):
        a = f(b["input_ids"], b["input_mask"], seg, b["feats"], *extra, b["is_matched"], b["label_ids"], b["label_scores"], rng)
        assert len(a) == 9 and a[1] is seg and a[2] is b["input_mask"] and a[5] is extra[0] and a[7] is b["is_matched"]
        assert a[6]["feat"][0] is b["feats"] and a[6]["obj"][0] is extra[1] and a[6]["attr"][1] is extra[4] and sorted(a[6]) == ["attr", "feat", "obj"]
        return dict(input_ids=a[0], masked_lm_labels=a[3], masked_feat=a[4], feat_mask=a[6]["feat"][1], ans=a[8])

    def snap(o):
        return {k: v.clone() for k, v in o.items()}

    def explicit():
        d = {k: ops.uniform(n, rng, SID + i) for i, (k, n) in enumerate(zip(DRAWS, (B * T, B * T, B * O, B * O, B)))}
        return corrupt(ops, b, b["feats"], (0.15, 0.15), V, draws=d)

    state0 = rng.clone()
    first = call(feat)
    e0 = explicit()
    assert torch.equal(rng, state0)
    for k in OUT:
        assert torch.equal(first[k], e0[k]), k
    want = R.corrupt(*[nb[k] for k in ("input_ids", "input_mask", "feats", "is_matched", "label_ids", "label_scores")],
                     host_draws(seed, 0, B, T, O), 0.15, 0.15, V, MASK)
    check(first, want, F32, "philox")
    again = call(feat)
    assert all(again[k].data_ptr() == first[k].data_ptr() for k in OUT)  # buffers are reused: capturable
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = call(feat)
    graph.replay()
    r0 = snap(captured)
    for k in OUT:
        assert torch.equal(r0[k], e0[k]), k
    ops.rng_advance(rng)
    graph.replay()
    r1 = snap(captured)
    eager = call(DeviceFeatures(vocab_size=V, mask_id=MASK, sid_base=SID, max_labels=3))
    e1 = explicit()
    torch.cuda.synchronize()
    assert int(rng[1]) == 1
    for k in OUT:
        assert torch.equal(r1[k], eager[k]) and torch.equal(r1[k], e1[k]), k
    assert not torch.equal(r1["masked_lm_labels"], r0["masked_lm_labels"]) and not torch.equal(r1["feat_mask"], r0["feat_mask"])


def test_distribution():
    """B = 512, T = 20, K = 3, seeded: every share within 5 sqrt(p (1 - p) / N) of p (N: the trials the share is taken over).
    Outcomes are read off the outputs; a replacement that draws the original id or [MASK] (2 / V per replaced word) or a
    pool row equal to its own (1 / (B O) per replaced row) would be counted as another outcome: an expected 0.01 events,
    far inside the bounds."""
    from xggm_amd import ops
    B, T, O, F, V, K, seed, rate = 512, 20, 36, 8, 30522, 3, 2024, 0.15
    nb = make_batch(B, T, O, F, seed, V, K)
    p_ans = np.array([0.2, 0.3, 0.5], dtype=np.float32)
    nb["label_ids"][:] = np.array([4, 9, 1])
    nb["label_scores"][:] = 2 * p_ans
    nb["is_matched"][:] = 1
    b = {k: dev(v) for k, v in nb.items()}
    out = corrupt(ops, b, b["feats"], (rate, rate), V, rng=ops.make_rng(seed, DEV), sid_base=SID)
    torch.cuda.synchronize()
    o = {k: v.cpu().numpy() for k, v in out.items()}
    ids, mask = nb["input_ids"], nb["input_mask"]
    eligible = np.zeros((B, T), dtype=bool)
    eligible[:, 1:T - 1] = (mask[:, 1:T - 1] == 1) & (mask[:, 2:] == 1)
    assert (ids[~eligible & (mask == 1)] <= SEP).all() and (ids[eligible] > MASK).all()  # [CLS] / [SEP] are exactly the others
    assert (o["masked_lm_labels"][~eligible] == -1).all() and (o["input_ids"][~eligible] == ids[~eligible]).all()

    def within(share, p, n, what):
        bound = 5 * math.sqrt(p * (1 - p) / n)
        print("%s: %.4f for %.2f over %d trials (bound %.4f)" % (what, share, p, n, bound))
        assert abs(share - p) <= bound, what

    lab = o["masked_lm_labels"] != -1
    assert (o["masked_lm_labels"][lab] == ids[lab]).all() and (o["input_ids"][~lab] == ids[~lab]).all()
    n_el, n_lab = int(eligible.sum()), int(lab.sum())
    within(n_lab / n_el, rate, n_el, "labelled words")
    is_mask, kept = lab & (o["input_ids"] == MASK), lab & (o["input_ids"] == ids)
    within(is_mask.sum() / n_lab, 0.8, n_lab, "words -> [MASK]")
    within(kept.sum() / n_lab, 0.1, n_lab, "words kept")
    within((lab & ~is_mask & ~kept).sum() / n_lab, 0.1, n_lab, "words replaced")
    assert o["input_ids"].min() >= 0 and o["input_ids"].max() < V
    fm = o["feat_mask"] == 1
    assert ((o["feat_mask"] == 0) | fm).all() and (o["masked_feat"][~fm] == nb["feats"][~fm]).all()
    n_obj, n_m = B * O, int(fm.sum())
    within(n_m / n_obj, rate, n_obj, "masked objects")
    zero, same = fm & (o["masked_feat"] == 0).all(-1), fm & (o["masked_feat"] == nb["feats"]).all(-1)
    within(zero.sum() / n_m, 0.8, n_m, "rows zeroed")
    within(same.sum() / n_m, 0.1, n_m, "rows kept")
    within((fm & ~zero & ~same).sum() / n_m, 0.1, n_m, "rows replaced")
    pool = {row.tobytes() for row in nb["feats"].reshape(-1, F)}
    assert all(row.tobytes() in pool for row in o["masked_feat"][fm & ~zero & ~same])  # replaced rows come from the pool
    for k, key in enumerate((4, 9, 1)):
        within((o["ans"] == key).mean(), float(p_ans[k]), B, "answer %d" % key)


@pytest.mark.parametrize("dt", [F32, BF16])
def test_model_fed_by_device_features(dt):
    """the 2-head tiny LXRTPretraining of tests/test_pretrain_model_gpu.py: forward(*DeviceFeatures(...)) gives the losses,
    bit for bit, of the same model fed the restatement's arrays; word rate 0.5 so that the 3 x 8 tokens carry labels"""
    from xggm_amd import ops, synth
    from xggm_amd.pretrain.lxmert_pretrain import DeviceFeatures, pack_labels
    from xggm_amd.runtime import runtime_of
    from test_pretrain_cpu import _tiny_model, _restore_visual_config
    model, _, meta, _, saved = _tiny_model("full", compute_dtype=dt, mlm_capacity=None)
    try:
        model = model.to(DEV).eval()
        c, seed = meta["cfg"], 5
        x = synth.pretrain_case(c["B"], c["T"], c["O"], c["F"], c["vocab"], c["n_obj"], c["n_attr"], c["n_ans"], seed=meta["seed"])
        t = {k: dev(v) for k, v in x.items()}
        lab, sc = pack_labels([{3: 0.3, 7: 0.6, 11: 1.0}, {5: 1.0}, None], 3)
        t["matched_label"][0] = 1  # the several-keys example draws
        x["matched_label"][0] = 1
        rng = ops.make_rng(seed, DEV)
        feat = DeviceFeatures(word_mask_rate=0.5, obj_mask_rate=0.15, vocab_size=c["vocab"], mask_id=103, sid_base=SID, max_labels=3)
        args = feat(t["input_ids"], t["input_mask"], t["segment_ids"], t["feats"], t["boxes"], t["obj_label"], t["obj_conf"],
                    t["attr_label"], t["attr_conf"], t["matched_label"], lab.to(DEV), sc.to(DEV), rng)

        def run(a):
            total, losses, _ = model(*a)
            runtime_of(model).backward(total)
            torch.cuda.synchronize()
            assert int(model.mlm_overflow) == 0
            return total.detach().clone(), losses.clone()

        got = run(args)
        want = R.corrupt(x["input_ids"], x["input_mask"], x["feats"], x["matched_label"], lab.numpy(), sc.numpy(),
                         host_draws(seed, 0, c["B"], c["T"], c["O"]), 0.5, 0.15, c["vocab"], 103)
        assert (want["masked_lm_labels"] != -1).sum() >= 2 and want["feat_mask"].sum() >= 1 and want["ans"][0] >= 0
        w = {k: dev(v) for k, v in want.items()}
        visn = {'obj': (t["obj_label"], t["obj_conf"]), 'attr': (t["attr_label"], t["attr_conf"]), 'feat': (t["feats"], w["feat_mask"])}
        ref = run((w["input_ids"], t["segment_ids"], t["input_mask"], w["masked_lm_labels"], w["masked_feat"], t["boxes"], visn,
                   t["matched_label"], w["ans"]))
        print("losses", got[1].tolist())
        assert got[1].numel() == 6 and bool(torch.isfinite(got[1]).all())
        assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])
    finally:
        _restore_visual_config(saved)
