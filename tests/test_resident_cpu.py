"""Host side of the device-resident data set (xggm_amd.tools.resident): the per-sample tables, the numpy restatement of the
gather (``host_batch``, the reference the kernel is held to in tests/test_resident_gpu.py) against the loader's own
collation, the epoch order against ``DataLoaderX``, and the refusals.  No kernel runs here."""
import os

import numpy as np
import pytest
import torch

from helpers import GOLDEN
from test_data_cpu import _records, _write_shard


def _tok():
    from xggm_amd.lxrt.tokenization import BertTokenizer
    return BertTokenizer(os.path.join(GOLDEN, "vocab_small.txt"), do_lower_case=True)


def _ts(tmp_path, kind="vqa", feat_dtype="bf16", data=None):
    from xggm_amd.vqa.vqacpv2_data import VQADataset, VQATorchDataset
    from xggm_amd.gqa.gqa_ood_data import GQADataset, GQATorchDataset
    meta, raw = _records()
    path = _write_shard(str(tmp_path / ("train_%s_%s.xgs" % (kind, feat_dtype))), meta, raw, feat_dtype=feat_dtype)
    a2l = {a: i for i, a in enumerate(meta["label2ans"])}
    DS, TS = (VQADataset, VQATorchDataset) if kind == "vqa" else (GQADataset, GQATorchDataset)
    return TS(DS("train", data=data if data is not None else meta[kind], ans2label=a2l, label2ans=meta["label2ans"]), shard=path)


def _store(ts, **kw):
    from xggm_amd.tools.resident import ResidentDataset
    from xggm_amd.lxrt.entry import SentenceBatcher
    return ResidentDataset(ts, SentenceBatcher(_tok(), 20), "cpu", **kw)


@pytest.mark.parametrize("kind", ["vqa", "gqa"])
@pytest.mark.parametrize("feat_dtype", ["bf16", "float32"])
@pytest.mark.parametrize("out_f32", [False, True])
def test_host_batch_equals_the_loaders_collation(tmp_path, kind, feat_dtype, out_f32):
    """``host_batch(indices)`` == ``VQATorchDataset.collate`` + ``SentenceBatcher.host_batch``, field by field and bit
    for bit, for bf16 and float32 shards into bf16 and fp32 feature buffers, and for the GQA twin.  (The loader has no
    bf16-shard-into-fp32-buffer path; widening bf16 is exact, so its bf16 batch as fp32 is the reference there.)"""
    from xggm_amd.lxrt.entry import SentenceBatcher
    ts = _ts(tmp_path, kind, feat_dtype)
    store = _store(ts)
    n = len(ts)
    assert len(store) == n and store.tables["feats"].shape[0] == 6 < n  # an image is stored once
    assert store.tables["feats"].dtype == (torch.bfloat16 if feat_dtype == "bf16" else torch.float32)
    batcher = SentenceBatcher(_tok(), 20)
    for items in ([0], [3, 1, 1, 7, n - 1], list(range(n))[::-1]):
        out = ts.alloc(len(items), False)
        if out_f32 and feat_dtype == "float32":
            out["feats"] = torch.zeros(out["feats"].shape, dtype=torch.float32)
        qids, sents, B = ts.collate(items, out)
        if out_f32 and feat_dtype == "bf16":
            out["feats"] = out["feats"].float()
        sent = batcher.host_batch(sents)
        got = store.host_batch(items, out_f32=out_f32)
        assert B == len(items) and got["feats"].dtype == (torch.float32 if out_f32 else torch.bfloat16)
        want = dict(feats=out["feats"], boxes=out["boxes"], adj_true=out["adj"], target=out["target"], input_ids=sent[0],
                    input_mask=sent[1], segment_ids=sent[2], sample=torch.tensor(items, dtype=torch.int64))
        assert sorted(got) == sorted(want)
        for k, v in want.items():
            assert got[k].dtype == v.dtype and torch.equal(got[k], v), k
        assert store.ques_ids(items) == qids


def test_table_edge_cases(tmp_path):
    """a repeated label keeps its LAST score (the host's sequential assignment), a datum without labels gives a zero
    target row, two questions of one image share one feature row, K is the largest number of distinct labels"""
    meta, _ = _records()
    data = [dict(d) for d in meta["vqa"]]
    data[1] = dict(data[1], label=[8, 3, 8], score=[0.3, 0.6, 0.9])
    del data[2]["label"], data[2]["score"]
    ts = _ts(tmp_path, data=data)
    store = _store(ts)
    h = store.host
    assert h["q_label"].shape == (len(data), 3) and store.K == 3
    assert h["q_label"][1].tolist() == [8, 3, -1] and h["q_score"][1].tolist() == [np.float32(0.9), np.float32(0.6), 0.0]
    assert h["q_label"][2].tolist() == [-1, -1, -1]
    hb = store.host_batch([1, 2, 0])
    want = torch.zeros(3, 17)
    want[0, 8], want[0, 3] = 0.9, 0.6
    ts.fill_target(data[0], want[2].numpy())
    assert torch.equal(hb["target"], want) and not hb["target"][1].any()
    assert data[0]["image_id"] == data[6]["image_id"] and h["q_row"][0] == h["q_row"][6]
    assert store.tables["feats"].shape[0] == len(ts.shard) == 6
    assert torch.equal(store.host_batch([0])["feats"], store.host_batch([6])["feats"])
    # the tables the kernel trusts are in range
    assert h["q_row"].dtype == np.int32 and 0 <= h["q_row"].min() and h["q_row"].max() < 6
    assert (h["q_len"] >= 2).all() and (h["q_len"] <= 20).all() and h["q_label"].max() < 17


def test_order_is_the_loaders_epoch_order(tmp_path):
    """``order(e, seed=s)`` visits the samples ``DataLoaderX(ts, B, shuffle=True, seed=s, drop_last=True)`` yields in its
    epoch e; the world = 2 slices are disjoint and cover every step's 2 B samples"""
    from xggm_amd.tools.data_loader import DataLoaderX
    ts = _ts(tmp_path)
    store = _store(ts)
    B, seed, n = 4, 3, len(ts)
    by_epoch = [q for b in DataLoaderX(ts, B, shuffle=True, seed=seed, drop_last=True, epochs=3) for q in b[0]]
    per = n // B * B
    assert len(by_epoch) == 3 * per
    for e in range(3):
        o = store.order(e, seed=seed, batch_size=B)
        assert o.dtype == np.int64 and len(o) == per
        assert store.ques_ids(o) == by_epoch[e * per:(e + 1) * per]
        assert torch.equal(store._order, torch.from_numpy(o))
    assert store.ques_ids(store.order(1, seed=seed)) [:per] == by_epoch[per:2 * per]  # no batch size: nothing is cut
    assert len(store.order(1, seed=seed)) == n
    assert store.order(0, shuffle=False, drop_last=False).tolist() == list(range(n))
    B = 3
    perm = np.random.default_rng([seed, 5]).permutation(n)
    r = [store.order(5, seed=seed, rank=k, world=2, batch_size=B) for k in range(2)]
    steps = n // (2 * B)
    assert steps == 2 and len(r[0]) == len(r[1]) == steps * B and not set(r[0]) & set(r[1])
    for s in range(steps):
        both = np.concatenate([r[0][s * B:(s + 1) * B], r[1][s * B:(s + 1) * B]])
        assert both.tolist() == perm[s * 2 * B:(s + 1) * 2 * B].tolist()
    with pytest.raises(ValueError, match="batch size"):
        store.order(0, world=2)
    assert _store(ts, batch_size=3).order(5, seed=seed, rank=1, world=2).tolist() == r[1].tolist()


def test_launch_function_refuses_before_any_launch():
    """the host-side checks of ``xggm_batch_gather`` run before the launch (nothing is enqueued here: no GPU): a null
    struct, B < 1, a size < 1, F % 8, rows outside the order, null and misaligned pointers, a stride below its row"""
    import ctypes
    from xggm_amd import _lib, ops

    def args(**kw):
        a = ops.BatchGatherArgs()
        for k in ("feats", "boxes", "adj", "q_row", "q_ids", "q_len", "q_label", "q_score", "q_bias_index", "order", "out_feats",
                  "out_boxes", "out_adj", "input_ids", "input_mask", "segment_ids", "target", "bias_index", "sample"):
            setattr(a, k, 4096)  # never dereferenced: every case below is refused on the host
        a.n, a.start, a.B, a.T, a.K, a.A, a.N, a.F = 20, 16, 4, 20, 3, 29, 5, 8
        a.out_feats_stride, a.target_stride = 40, 29
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    L = _lib.lib
    assert L.xggm_batch_gather(None, None) != 0 and b"null argument struct" in L.xggm_last_error()
    for kw, msg in ((dict(B=0), b"B=0"), (dict(T=0), b"T=0"), (dict(K=0), b"K=0"), (dict(A=0), b"A=0"), (dict(N=0), b"N=0"),
                    (dict(F=0), b"F=0"), (dict(F=12), b"multiple of 8"), (dict(start=17), b"leave order"),
                    (dict(start=-1), b"leave order"), (dict(feats=None), b"null table"), (dict(order=None), b"null order"),
                    (dict(input_mask=None), b"null output"), (dict(adj=None), b"adjacency table"),
                    (dict(q_label=None), b"q_label"), (dict(q_bias_index=None), b"q_bias_index"),
                    (dict(out_feats=4096 + 8), b"16-byte"), (dict(boxes=4096 + 4), b"16-byte"),
                    (dict(target=4096 + 2), b"4-byte"), (dict(order=4096 + 4), b"8-byte"),
                    (dict(out_feats_stride=36), b"row stride"), (dict(out_feats_stride=44), b"row stride"),
                    (dict(target_stride=28), b"target row stride")):
        a = args(**kw)
        assert L.xggm_batch_gather(ctypes.addressof(a), None) != 0, kw
        assert msg in L.xggm_last_error(), (kw, L.xggm_last_error())


def test_refusals(tmp_path):
    from xggm_amd import ops
    meta, _ = _records()
    data = [dict(d) for d in meta["vqa"]]
    data[5] = dict(data[5], label=[2, 17], score=[0.3, 0.6])  # the answer table has 17 entries
    with pytest.raises(ValueError, match="5005"):
        _store(_ts(tmp_path, data=data))
    data[5] = dict(data[5], label=[-1], score=[0.3])  # numpy would wrap it around to the last answer
    with pytest.raises(ValueError, match="5005"):
        _store(_ts(tmp_path, data=data))
    ts = _ts(tmp_path)
    with pytest.raises(ValueError, match=r"needs \d+ bytes"):
        _store(ts, max_bytes=1 << 12)  # the features alone are 6 * 36 * 64 * 2 bytes
    assert _store(ts, max_bytes=1 << 20).nbytes > 6 * 36 * 64 * 2
    with pytest.raises(ValueError, match="bias_index"):
        _store(ts, bias_index=[0, 1])
    store = _store(ts, bias_index=np.arange(len(ts)) % 3)
    assert store.host_batch([4, 2])["bias_index"].tolist() == [1, 2]
    out = store.host_batch([0, 1, 2])
    del out["sample"]
    with pytest.raises(RuntimeError, match="GPU"):  # the numpy restatement is a reference, not a fallback
        store.fill(out, 0, 3)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.batch_gather(store.tables, store._order, 0, 3, out)
    bad = dict(out, target=torch.zeros(3, 16))
    with pytest.raises(ValueError, match="A=17"):
        store.fill(bad, 0, 3)
