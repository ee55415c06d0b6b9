"""Host side of the label adjacency (csrc/label_adjacency.hip, preprocess/label_embeddings.py, the label-fed batch
gather): the C ABI's refusals, the checkpoint loader, a numpy restatement of the label adjacency against the fixture the
reference's own ``compute_cosin_sim_v2`` produced, and the stores adopting a table that keeps no [n, N, N] adjacency.  No
kernel runs here: every ABI call below is refused before a launch."""
import ctypes
import re
import subprocess

import numpy as np
import pytest
import torch

import label_adjacency_cases as C
import tsv_cases as TC
from helpers import load_golden
from xggm_amd import synth

P16 = 1 << 20  # a pointer-like value, 16-byte aligned; never dereferenced (every call is refused on the host)


# ----------------------------------------------------------------------------- the C ABI
def test_new_symbols_are_declared_exported_and_cite_the_reference():
    from xggm_amd import _lib
    decl = _lib.parse_header()
    for name, nargs in (("xggm_label_cosine_table_f32", 8), ("xggm_label_adjacency_f32", 9), ("xggm_batch_gather_labels", 3)):
        assert name in decl and len(decl[name]) == nargs and hasattr(_lib.lib, name), name
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert {"xggm_label_cosine_table_f32", "xggm_label_adjacency_f32", "xggm_batch_gather_labels"} <= set(re.findall(r" T (xggm_\w+)", out))
    src = open(_lib.HEADER_PATH).read()
    for sym in ("xggm_label_cosine_table_f32", "xggm_label_adjacency_f32", "xggm_batch_gather_labels"):
        at = src.index("int " + sym)
        start = src.rindex(sym, 0, at)  # the contract comment names the symbol
        comment = src[src.rindex("/*", 0, start):at]
        assert "data/preprocess/vqa/compute_adjacency.py:38-45" in comment and ":75-90" in comment, sym


def test_pair_table_entry_refuses_bad_arguments_before_any_launch():
    from xggm_amd import _lib
    L = _lib.lib
    f = L.xggm_label_cosine_table_f32
    cases = [((None, P16, P16, 7, 5, 8), b"null"), ((P16, None, P16, 7, 5, 8), b"null"), ((P16, P16, None, 7, 5, 8), b"null"),
             ((P16, P16, P16, 0, 5, 8), b"Vc=0"), ((P16, P16, P16, 7, -1, 8), b"Va=-1"),
             ((P16, P16, P16, 7, 5, 6), b"multiple of 4"), ((P16, P16, P16, 7, 5, 0), b"multiple of 4"),
             ((P16 + 4, P16, P16, 7, 5, 8), b"16-byte aligned"), ((P16, P16 + 8, P16, 7, 5, 8), b"16-byte aligned"),
             ((P16, P16, P16 + 2, 7, 5, 8), b"4-byte aligned")]
    for args, msg in cases:
        assert f(*args, 1e-6, None) == 1, args
        assert msg in L.xggm_last_error() and b"xggm_label_cosine_table_f32" in L.xggm_last_error(), (args, L.xggm_last_error())


def test_label_adjacency_entry_refuses_bad_arguments_before_any_launch():
    from xggm_amd import _lib
    L = _lib.lib
    f = L.xggm_label_adjacency_f32
    ok = dict(table=P16, Vc=7, Va=5, obj=P16, att=P16, adj=P16, n=3, N=36)
    cases = [(dict(table=None), b"null"), (dict(obj=None), b"null"), (dict(att=None), b"null"), (dict(adj=None), b"null"),
             (dict(N=0), b"N = 0"), (dict(N=129), b"N = 129"), (dict(N=-1), b"N = -1"), (dict(Vc=0), b"Vc=0"), (dict(Va=0), b"Va=0"),
             (dict(Va=-3), b"Va=-3"), (dict(n=0), b"n=0"), (dict(table=P16 + 2), b"misaligned"), (dict(obj=P16 + 1), b"misaligned"),
             (dict(att=P16 + 3), b"misaligned"), (dict(adj=P16 + 2), b"misaligned")]
    for change, msg in cases:
        a = dict(ok, **change)
        assert f(a["table"], a["Vc"], a["Va"], a["obj"], a["att"], a["adj"], a["n"], a["N"], None) == 1, change
        assert msg in L.xggm_last_error() and b"xggm_label_adjacency_f32" in L.xggm_last_error(), (change, L.xggm_last_error())


def _gather_args(ops, N=36):
    a = ops.BatchGatherArgs()
    for k in ("feats", "boxes", "q_row", "q_ids", "q_len", "q_label", "q_score", "order", "out_feats", "out_boxes", "out_adj",
              "input_ids", "input_mask", "segment_ids", "target"):
        setattr(a, k, P16)
    a.n, a.start, a.B, a.T, a.K, a.A, a.N, a.F = 8, 0, 4, 20, 2, 29, N, 64
    a.out_feats_stride, a.target_stride = N * 64, 29
    return a


def _label_args(ops, **change):
    l = ops.LabelAdjArgs()
    l.table, l.obj_labels, l.attr_labels, l.Vc, l.Va = P16, P16, P16, 7, 5
    for k, v in change.items():
        setattr(l, k, v)
    return l


def test_label_gather_entry_refuses_bad_arguments_before_any_launch():
    """the second gather entry keeps xggm_batch_gather's refusals and adds its own; the struct of the first is unchanged"""
    from xggm_amd import _lib, ops
    L = _lib.lib
    f, who = L.xggm_batch_gather_labels, b"xggm_batch_gather_labels"
    ref = lambda s: ctypes.addressof(s)  # noqa: E731
    good = _label_args(ops)
    assert f(None, ref(good), None) == 1 and b"null argument struct" in L.xggm_last_error()
    assert f(ref(_gather_args(ops)), None, None) == 1 and b"null label struct" in L.xggm_last_error()
    both = _gather_args(ops)
    both.adj = P16
    assert f(ref(both), ref(good), None) == 1 and b"one source of adj_true" in L.xggm_last_error() and who in L.xggm_last_error()
    for change, msg in ((dict(table=None), b"null label table"), (dict(obj_labels=None), b"null label table"),
                        (dict(attr_labels=None), b"null label table"), (dict(Vc=0), b"Vc=0"), (dict(Va=-2), b"Va=-2"),
                        (dict(table=P16 + 2), b"misaligned"), (dict(attr_labels=P16 + 1), b"misaligned")):
        assert f(ref(_gather_args(ops)), ref(_label_args(ops, **change)), None) == 1, change
        assert msg in L.xggm_last_error() and who in L.xggm_last_error(), (change, L.xggm_last_error())
    assert f(ref(_gather_args(ops, N=129)), ref(good), None) == 1 and b"N = 129" in L.xggm_last_error()
    bad = _gather_args(ops)
    bad.F = 12  # a rule of the first entry, under the second entry's name
    assert f(ref(bad), ref(good), None) == 1 and b"multiple of 8" in L.xggm_last_error() and who in L.xggm_last_error()
    # the first entry: still refuses an adjacency output without a table, and still has its 31 fields
    assert L.xggm_batch_gather(ref(_gather_args(ops)), None) == 1 and b"needs the adjacency table" in L.xggm_last_error()
    assert len(ops.BatchGatherArgs._fields_) == 31 and ctypes.sizeof(ops.BatchGatherArgs) == 23 * 8 + 8 * 4
    assert ctypes.sizeof(ops.LabelAdjArgs) == 3 * 8 + 2 * 4


# ----------------------------------------------------------------------------- the checkpoint loader
def _tiny_state():
    from xggm_amd.preprocess.label_embeddings import LabelEncoder
    shapes = {k: tuple(v.shape) for k, v in LabelEncoder(C.tiny_config()).state_dict().items()}
    return shapes, C.tiny_bert_state(shapes)


def test_label_encoder_has_the_key_names_of_a_bert_checkpoint():
    shapes, _ = _tiny_state()
    per_layer = ["attention.self.query", "attention.self.key", "attention.self.value", "attention.output.dense",
                 "attention.output.LayerNorm", "intermediate.dense", "output.dense", "output.LayerNorm"]
    want = ["embeddings.word_embeddings.weight", "embeddings.position_embeddings.weight", "embeddings.token_type_embeddings.weight",
            "embeddings.LayerNorm.weight", "embeddings.LayerNorm.bias", "pooler.dense.weight", "pooler.dense.bias"]
    want += ["encoder.layer.%d.%s.%s" % (i, m, p) for i in range(C.TINY["layers"]) for m in per_layer for p in ("weight", "bias")]
    assert sorted(shapes) == sorted(want)
    assert shapes["embeddings.word_embeddings.weight"] == (81, 128) and shapes["embeddings.position_embeddings.weight"] == (32, 128)
    assert shapes["encoder.layer.1.intermediate.dense.weight"] == (256, 128)


def test_loader_takes_prefixes_old_layernorm_names_and_ignores_heads(tmp_path):
    from xggm_amd.preprocess.label_embeddings import load_label_encoder
    cfg = C.tiny_config()
    shapes, sd = _tiny_state()
    plain = load_label_encoder(cfg, sd, device="cpu")
    assert not plain.training
    for k, v in plain.state_dict().items():
        assert torch.equal(v, sd[k]), k
    old = {}
    for k, v in sd.items():  # a BertForPreTraining checkpoint of the old spelling
        k = k.replace("LayerNorm.weight", "LayerNorm.gamma").replace("LayerNorm.bias", "LayerNorm.beta")
        old["bert." + k] = v
    assert any(k.endswith("gamma") for k in old) and any(k.endswith("beta") for k in old)
    old["cls.predictions.bias"] = torch.zeros(81)
    old["cls.predictions.transform.LayerNorm.gamma"] = torch.zeros(128)
    old["cls.seq_relationship.weight"] = torch.zeros(2, 128)
    old["bert.embeddings.position_ids"] = torch.arange(32).unsqueeze(0)
    torch.save(old, str(tmp_path / "pytorch_model.bin"))
    for src in (old, str(tmp_path / "pytorch_model.bin"), str(tmp_path)):
        m = load_label_encoder(cfg, src, device="cpu")
        for k, v in m.state_dict().items():
            assert torch.equal(v, sd[k]), k
    # a missing body tensor is refused BY NAME, with and without the prefix
    for victim in ("encoder.layer.1.output.dense.weight", "pooler.dense.bias", "embeddings.LayerNorm.weight"):
        short = {k: v for k, v in sd.items() if k != victim}
        with pytest.raises(KeyError, match=re.escape(victim)):
            load_label_encoder(cfg, short, device="cpu")
    short = {k: v for k, v in old.items() if k != "bert.encoder.layer.0.attention.output.LayerNorm.gamma"}
    with pytest.raises(KeyError, match=r"encoder\.layer\.0\.attention\.output\.LayerNorm\.weight"):
        load_label_encoder(cfg, short, device="cpu")
    wrong = dict(sd, **{"pooler.dense.weight": torch.zeros(64, 128)})
    with pytest.raises(ValueError, match="pooler.dense.weight"):
        load_label_encoder(cfg, wrong, device="cpu")
    # nothing is looked up by name
    with pytest.raises(FileNotFoundError, match="offline"):
        load_label_encoder(cfg, "bert-base-uncased", device="cpu")
    with pytest.raises(FileNotFoundError):
        load_label_encoder(cfg, str(tmp_path / "absent"), device="cpu")


def test_labels_tokens_and_limits(tmp_path):
    """``read_labels`` strips the line end only; a label is ``[CLS] pieces [SEP]``; the fixture's ids are the package
    tokenizer's; too long a label and a CPU encoder are refused"""
    from xggm_amd.lxrt.modeling import BertConfig
    from xggm_amd.preprocess.label_embeddings import LabelEncoder, embed_labels, label_ids, read_labels
    f = tmp_path / "objects_vocab.txt"
    f.write_text("yolk\n traffic light \nstop sign,stopsign\n\ndog")
    assert read_labels(str(f)) == ["yolk", " traffic light ", "stop sign,stopsign", "", "dog"]
    tok = C.tokenizer()
    assert label_ids(tok, "catlike dogs") == [2, 21, 22, 20, 12, 3]
    assert label_ids(tok, "") == [2, 3]
    g = load_golden("bert_tiny")
    assert [str(s) for s in g["labels"]] == C.LABELS and int(g["seed"]) == C.SEED
    ids, mask, pieces = C.padded_rows(tok, C.LABELS)
    assert np.array_equal(ids, g["input_ids"]) and np.array_equal(mask, g["input_mask"])
    assert sorted(set(pieces)) == [1, 2, 3, 4, 5] and g["pooled"].shape == (24, 128)
    enc = LabelEncoder(C.tiny_config())
    with pytest.raises(RuntimeError, match="GPU"):
        embed_labels(enc, tok, ["dog"])
    with pytest.raises(ValueError, match="no labels"):
        embed_labels(enc, tok, [])
    with pytest.raises(ValueError, match="position table"):
        enc(torch.zeros(1, 33, dtype=torch.int64))
    with pytest.raises(ValueError, match="attention core"):
        LabelEncoder(BertConfig(81, hidden_size=128, num_hidden_layers=1, num_attention_heads=2, intermediate_size=256,
                                max_position_embeddings=512))(torch.zeros(1, 129, dtype=torch.int64))


# ----------------------------------------------------------------------------- the arithmetic, restated
def test_numpy_restatement_matches_the_reference_golden():
    """look-ups in a Vc x Va cosine table, c + c^T, / max -- against what the reference's compute_cosin_sim_v2 + / max made
    of the gathered embeddings (tests/golden/adjacency.npz), at that fixture's bound; the package's own host restatement
    (what ``ResidentDataset.host_batch`` uses) is the same function"""
    from xggm_amd.preprocess.compute_adjacency import label_adjacency_host
    g = load_golden("adjacency")
    seed, D = int(g["seed"]), int(g["D"])
    cls = synth._rng(seed, "adj_class_table").standard_normal((60, D), dtype=np.float32)
    att = synth._rng(seed, "adj_attr_table").standard_normal((45, D), dtype=np.float32)
    att[7] = 0.0
    att[8] = cls[8]
    table = C.cosine_table_numpy(cls, att).astype(np.float32)
    assert table.shape == (60, 45) and not table[:, 7].any() and abs(table[8, 8] - 1.0) < 1e-6
    adj = C.label_adjacency_numpy(table, g["objects_id"], g["attrs_id"])
    assert adj.dtype == np.float32 and adj.shape == g["adj"].shape == (4, 36, 36)
    assert float(np.abs(adj - g["adj"]).max()) < 5e-6
    assert float(adj.max()) == 1.0 and np.array_equal(adj, adj.transpose(0, 2, 1))
    assert np.array_equal(label_adjacency_host(table, g["objects_id"], g["attrs_id"]), adj)


# ----------------------------------------------------------------------------- the stores
def _datasets(tmp_path, recs, tables):
    from xggm_amd.vqa.vqacpv2_data import VQADataset, VQATorchDataset
    import pretrain_resident_cases as P
    rng = np.random.default_rng(3)
    data = [dict(question_id=100 + q, image_id=recs[i]["img_id"], question=" ".join(rng.choice(P.words(), size=4)), label=[q % 7],
                 score=[0.5]) for q, i in enumerate([0, 3, 1, 1, 2, 0])]
    l2a = ["a%d" % i for i in range(7)]
    return [VQATorchDataset(VQADataset("train", data=data, ans2label={a: i for i, a in enumerate(l2a)}, label2ans=l2a), shard=t)
            for t in tables]


def test_stores_adopt_a_table_without_a_materialised_adjacency(tmp_path):
    from xggm_amd import utils
    from xggm_amd.lxrt.entry import SentenceBatcher
    from xggm_amd.tools import tsv
    from xggm_amd.tools.resident import ResidentDataset
    import pretrain_resident_cases as P
    recs = utils.load_obj_tsv(TC.tsv_file(tmp_path, 5, 24, 4, plain_ids=True)[0])
    pair = torch.from_numpy(np.random.default_rng(5).random((1600, 400), dtype=np.float32) + 0.25)
    oid, aid = np.stack([r["objects_id"] for r in recs]), np.stack([r["attrs_id"] for r in recs])
    want = C.label_adjacency_numpy(pair.numpy(), oid, aid)
    table = tsv.ObjTable.from_records(recs, "cpu")
    bare = table.nbytes
    assert table.set_label_adjacency(pair) is table and table.adj is None and table.pair_table.data_ptr() == pair.data_ptr()
    assert table.nbytes == bare + pair.numel() * 4
    twin = tsv.ObjTable.from_records(recs, "cpu").set_adjacency(torch.from_numpy(want.copy()))
    ts, ts_twin = _datasets(tmp_path, recs, (table, twin))
    batcher = SentenceBatcher(P.tok(), 10)
    mine, other = ResidentDataset(ts, batcher, "cpu"), ResidentDataset(ts_twin, batcher, "cpu")
    assert "adj" not in mine.tables
    for k in ("pair_table", "obj_labels", "attr_labels"):
        assert mine.tables[k].data_ptr() == getattr(table, k).data_ptr(), k
    # the pair table (and the label ids it is read with) in place of the [n, N, N] table
    assert mine.nbytes == other.nbytes - want.nbytes + pair.numel() * 4 + 2 * oid.size * 4
    a, b = mine.host_batch([5, 0, 2, 3]), other.host_batch([5, 0, 2, 3])
    assert a.keys() == b.keys() and "adj_true" in a
    for k in a:
        assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k
    assert np.array_equal(a["adj_true"].numpy(), want[ts.rows[[5, 0, 2, 3]]])
    with pytest.raises(RuntimeError, match="GPU"):  # an item's adjacency is made by the kernel: no CPU fallback
        ts[0]


def test_label_adjacency_refusals_of_the_stores(tmp_path):
    from xggm_amd import utils
    from xggm_amd.lxrt.entry import SentenceBatcher
    from xggm_amd.tools import tsv
    from xggm_amd.tools.resident import ResidentDataset
    import pretrain_resident_cases as P
    recs = utils.load_obj_tsv(TC.tsv_file(tmp_path, 5, 24, 4, plain_ids=True)[0])
    pair = torch.ones(1600, 400)
    adj = torch.ones(4, 5, 5)
    with pytest.raises(ValueError, match="one source"):
        tsv.ObjTable.from_records(recs, "cpu").set_label_adjacency(pair).set_adjacency(adj)
    with pytest.raises(ValueError, match="one source"):
        tsv.ObjTable.from_records(recs, "cpu").set_adjacency(adj).set_label_adjacency(pair)
    both = tsv.ObjTable.from_records(recs, "cpu").set_label_adjacency(pair)
    both.adj = adj  # behind the setters' backs: the store refuses it too
    with pytest.raises(ValueError, match="one source"):
        ResidentDataset(_datasets(tmp_path, recs, (both,))[0], SentenceBatcher(P.tok(), 10), "cpu")
    # ids outside the table: the range is named, nothing is stored
    oid = np.stack([r["objects_id"] for r in recs])
    aid = np.stack([r["attrs_id"] for r in recs])
    t = tsv.ObjTable.from_records(recs, "cpu")
    with pytest.raises(ValueError, match=r"class ids %d \.\. %d \(table: \[0, %d\)\)" % (oid.min(), oid.max(), oid.max())):
        t.set_label_adjacency(torch.ones(int(oid.max()), 400))
    with pytest.raises(ValueError, match=r"attribute ids %d \.\. %d \(table: \[0, %d\)\)" % (aid.min(), aid.max(), aid.max())):
        t.set_label_adjacency(torch.ones(1600, int(aid.max())))
    assert t.pair_table is None
    wild = utils.load_obj_tsv(TC.tsv_file(tmp_path, 5, 24, 4)[0])  # ids at +-2^31 -+ 1
    with pytest.raises(ValueError, match=r"class ids \d+ \.\. 2147483647 \(table: \[0, 1600\)\), attribute ids -2147483648 \.\. \d+"):
        tsv.ObjTable.from_records(wild, "cpu").set_label_adjacency(pair)
    for bad in (torch.ones(1600), torch.ones(1600, 400, dtype=torch.float64)):
        with pytest.raises(ValueError, match="float32"):
            t.set_label_adjacency(bad)
