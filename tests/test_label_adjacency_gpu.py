"""adj_true from detector labels on the GPU: the pair-table and label-adjacency kernels (csrc/label_adjacency.hip) against
the per-image cosine kernels they restate -- BIT for bit --, against the reference's fixture, inside guard bands and with ids
outside the table; the batch gather that makes ``adj_true`` from labels against a twin store that holds the materialised
table; and the label encoder against a ``transformers`` BertModel's pooled outputs (tests/golden/bert_tiny.npz)."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import label_adjacency_cases as C  # noqa: E402
from graph_long_cases import banded, moated  # noqa: E402
from helpers import load_golden  # noqa: E402
from xggm_amd import synth  # noqa: E402

DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _case(N, D, Vc=7, Va=5, n=5, seed=0):
    """seeded embeddings and ids: attribute row 2 is zero (under the eps clamp), attribute row 1 equals class row 3, and
    image 0 has that pair on its diagonal (the doubled cosine of a vector with itself: the maximum)"""
    gen = torch.Generator().manual_seed(1000 * N + D + seed)
    cls, att = torch.randn(Vc, D, generator=gen), torch.randn(Va, D, generator=gen)
    att[2] = 0.0
    att[1] = cls[3]
    ref = C.cosine_table_numpy(cls.numpy(), att.numpy())
    while True:
        oid, aid = torch.randint(0, Vc, (n, N), generator=gen), torch.randint(0, Va, (n, N), generator=gen)
        oid[0, 0], aid[0, 0] = 3, 1
        # an image whose maximum is the zero row's 0 (every other pair negative) is x / 0 on every path: inf and NaN, which
        # torch.equal never calls equal.  Such ids are drawn again -- a property of the INPUT, decided in fp64 on the host.
        c = np.triu(ref[oid.numpy()[:, :, None], aid.numpy()[:, None, :]])
        if ((c + c.transpose(0, 2, 1)).max(axis=(1, 2)) != 0.0).all():
            return cls.to(DEV), att.to(DEV), oid, aid


# ----------------------------------------------------------------------------- 1. the same bits as the per-image kernels
@pytest.mark.parametrize("D", [8, 68, 768])
@pytest.mark.parametrize("N", [1, 4, 36, 37, 64, 65, 100, 128])
def test_label_path_equals_the_embedding_path_bit_for_bit(N, D):
    """``build_adjacency_from_labels(label_pair_table(...))`` is ``torch.equal`` to ``build_adjacency`` -- both short
    templates (N <= 36, <= 64) and the long kernel, widths that are no multiple of either kernel's chunk, vocabularies of
    (7, 5): many duplicate labels, ties at the maximum"""
    from xggm_amd.preprocess.compute_adjacency import build_adjacency, build_adjacency_from_labels, label_pair_table
    cls, att, oid, aid = _case(N, D)
    table = label_pair_table(cls, att)
    ref = C.cosine_table_numpy(cls.cpu().numpy(), att.cpu().numpy())
    err = float(np.abs(table.cpu().numpy() - ref).max())
    print("N %d D %d: pair table against fp64 %.3e" % (N, D, err))
    assert err <= (2 * D + 8) * 2.0 ** -24  # three fp32 sums of D terms (gamma_D each, |cos| <= 1), a root, a product, a quotient
    assert not bool(table[:, 2].any())      # the zero row: 0 / (|c| eps)
    want = build_adjacency(cls, att, oid, aid)
    got = build_adjacency_from_labels(table, oid, aid)
    assert got.shape == (5, N, N) and got.dtype == F32
    assert torch.equal(got, want), "N %d D %d: %d elements differ, max %.3e" % (N, D, int((got != want).sum()), float((got - want).abs().max()))
    assert float(got.amax()) == 1.0 and float(got[0].amax()) == 1.0 and torch.equal(got, got.transpose(1, 2))
    assert float(got[0, 0, 0]) == 1.0  # the doubled diagonal of the identical pair


def test_label_path_equals_the_embedding_path_on_a_full_vocabulary():
    """1601 x 401 labels (one past the published vocabularies: ragged pair tiles on both sides), N = 36, D = 768"""
    from xggm_amd.preprocess.compute_adjacency import build_adjacency, build_adjacency_from_labels, label_pair_table
    cls, att, oid, aid = _case(36, 768, Vc=1601, Va=401)
    oid[1, :2], aid[1, :2] = torch.tensor([1600, 0]), torch.tensor([0, 400])  # the corners of the table
    table = label_pair_table(cls, att)
    assert table.shape == (1601, 401)
    assert torch.equal(build_adjacency_from_labels(table, oid, aid), build_adjacency(cls, att, oid, aid))


def test_label_path_matches_the_reference_golden():
    """the label path on the reference-made fixture, at the bound the embedding path is held to there"""
    from xggm_amd.preprocess.compute_adjacency import build_adjacency_from_labels, label_pair_table
    g = load_golden("adjacency")
    seed, D = int(g["seed"]), int(g["D"])
    cls = torch.from_numpy(synth._rng(seed, "adj_class_table").standard_normal((60, D), dtype=np.float32))
    att = torch.from_numpy(synth._rng(seed, "adj_attr_table").standard_normal((45, D), dtype=np.float32))
    att[7] = 0.0
    att[8] = cls[8]
    adj = build_adjacency_from_labels(label_pair_table(cls.to(DEV), att.to(DEV)), torch.from_numpy(g["objects_id"]),
                                      torch.from_numpy(g["attrs_id"]))
    assert adj.shape == (4, 36, 36)
    err = float((adj.cpu() - torch.from_numpy(g["adj"])).abs().max())
    print("label path against the reference fixture: %.3e" % err)
    assert err < 5e-6
    assert float(adj.max()) == 1.0 and torch.equal(adj, adj.transpose(1, 2))


# ----------------------------------------------------------------------------- 2. guard bands
def _call(name, *args):
    from xggm_amd._lib import call, stream
    call(name, *args, stream())


@pytest.mark.parametrize("n,N", [(1, 36), (1, 37), (3, 5), (2, 128), (2, 1)])
def test_label_adjacency_stays_inside_its_output(n, N):
    """inputs in moats (NaN around the table, a huge index around the ids), the output in a band of sentinels that is
    intact afterwards; n = 1, and N * N no multiple of 4"""
    from xggm_amd.preprocess.compute_adjacency import build_adjacency_from_labels, label_pair_table
    cls, att, oid, aid = _case(N, 8, n=n)
    table = label_pair_table(cls, att)
    want = build_adjacency_from_labels(table, oid, aid)
    t, o, a = moated(table.cpu(), DEV), moated(oid.to(torch.int32), DEV), moated(aid.to(torch.int32), DEV)
    out = banded((n, N, N), F32, DEV)
    _call("xggm_label_adjacency_f32", t.data_ptr(), 7, 5, o.data_ptr(), a.data_ptr(), out.view.data_ptr(), n, N)
    torch.cuda.synchronize()
    assert torch.equal(out.view, want) and out.untouched_outside()


@pytest.mark.parametrize("Vc,Va,D", [(7, 5, 8), (65, 130, 68), (64, 64, 36), (1, 1, 4)])
def test_pair_table_stays_inside_its_output(Vc, Va, D):
    """ragged pair tiles, a chunk that is cut short: embeddings in NaN moats, the table in a band of sentinels"""
    gen = torch.Generator().manual_seed(Vc + Va + D)
    cls, att = torch.randn(Vc, D, generator=gen), torch.randn(Va, D, generator=gen)
    out = banded((Vc, Va), F32, DEV)
    c, a = moated(cls, DEV), moated(att, DEV)  # named: a temporary's buffer would be handed to the next allocation
    _call("xggm_label_cosine_table_f32", c.data_ptr(), a.data_ptr(), out.view.data_ptr(), Vc, Va, D, 1e-6)
    torch.cuda.synchronize()
    err = float(np.abs(out.view.cpu().numpy() - C.cosine_table_numpy(cls.numpy(), att.numpy())).max())
    assert err <= (2 * D + 8) * 2.0 ** -24 and out.untouched_outside()


# ----------------------------------------------------------------------------- 3. ids outside the table
@pytest.mark.parametrize("N", [36, 100])
def test_ids_outside_the_table(N):
    """ids Vc, -1 and Va + 3 in one image of three: the wrapper raises before launching; the kernel (called through the
    ABI, the table in the MIDDLE of a larger allocation, so that even an unguarded look-up would read mapped memory) makes
    that image NaN and leaves its neighbours bit-equal to the clean run"""
    from xggm_amd.preprocess.compute_adjacency import build_adjacency_from_labels, label_pair_table
    Vc, Va = 7, 5
    cls, att, oid, aid = _case(N, 8, n=3)
    table = label_pair_table(cls, att)
    clean = build_adjacency_from_labels(table, oid, aid)
    for where, (obj_id, att_id) in enumerate(((Vc, 0), (-1, 0), (0, Va + 3), (0, -1))):
        bo, ba = oid.clone(), aid.clone()
        slot = (where * 7) % N
        bo[1, slot], ba[1, slot] = obj_id, att_id
        with pytest.raises(ValueError, match=r"class ids -?\d+ \.\. \d+ \(table: \[0, 7\)\), attribute ids -?\d+ \.\. \d+ \(table: \[0, 5\)\)"):
            build_adjacency_from_labels(table, bo, ba)
        room = torch.zeros(3 * Vc * Va + 64, device=DEV)
        mid = room[Vc * Va + 32:2 * Vc * Va + 32].view(Vc, Va)  # 8 * Va + 3 elements of slack on either side
        mid.copy_(table)
        o32, a32 = bo.to(torch.int32).to(DEV), ba.to(torch.int32).to(DEV)
        out = banded((3, N, N), F32, DEV)
        _call("xggm_label_adjacency_f32", mid.data_ptr(), Vc, Va, o32.data_ptr(), a32.data_ptr(), out.view.data_ptr(), 3, N)
        torch.cuda.synchronize()
        assert bool(torch.isnan(out.view[1]).all()), (where, "the image with the id is not all NaN")
        assert torch.equal(out.view[0], clean[0]) and torch.equal(out.view[2], clean[2]) and out.untouched_outside(), where


# ----------------------------------------------------------------------------- 4. the gather
def _obj_table(n_img, N, F, Vc, Va, seed):
    from xggm_amd.tools import tsv
    gen = torch.Generator().manual_seed(seed)
    t = dict(feats=torch.randn(n_img, N, F, generator=gen).to(BF16), boxes=torch.rand(n_img, N, 4, generator=gen),
             obj_labels=torch.randint(0, Vc, (n_img, N), generator=gen, dtype=torch.int32),
             attr_labels=torch.randint(0, Va, (n_img, N), generator=gen, dtype=torch.int32),
             obj_confs=torch.rand(n_img, N, generator=gen), attr_confs=torch.rand(n_img, N, generator=gen))
    t = {k: v.to(DEV) for k, v in t.items()}
    mk = lambda: tsv.ObjTable(dict(t), ["img%d" % i for i in range(n_img)], [480] * n_img, [640] * n_img)  # noqa: E731
    return mk(), mk()  # two tables over the SAME tensors


def _stores(n_img, n_q, N, F, A, seed):
    """a store whose table makes adj_true from labels and a twin that holds ``build_adjacency``'s table"""
    from xggm_amd.lxrt.entry import SentenceBatcher
    from xggm_amd.preprocess.compute_adjacency import build_adjacency, label_pair_table
    from xggm_amd.tools.resident import ResidentDataset
    from xggm_amd.vqa.vqacpv2_data import VQADataset, VQATorchDataset
    Vc, Va = 60, 45
    gen = torch.Generator().manual_seed(seed)
    cls, att = torch.randn(Vc, 64, generator=gen).to(DEV), torch.randn(Va, 64, generator=gen).to(DEV)
    lab, mat = _obj_table(n_img, N, F, Vc, Va, seed)
    pair = label_pair_table(cls, att)
    lab.set_label_adjacency(pair)
    mat.set_adjacency(build_adjacency(cls, att, mat.obj_labels, mat.attr_labels))
    assert lab.adj is None and lab.nbytes == mat.nbytes - n_img * N * N * 4 + Vc * Va * 4
    rng = np.random.default_rng(seed)
    words = [w for w in open(C.VOCAB).read().split() if w.isalpha()][:40]
    data = [dict(question_id=100 + q, image_id="img%d" % ((5 * q) % n_img), label=[int(x) for x in rng.choice(A, 1 + q % 3, replace=False)],
                 score=[float(x) for x in rng.choice([0.3, 0.6, 0.9, 1.0], 1 + q % 3)],
                 question=" ".join(rng.choice(words, size=int(rng.integers(3, 9))))) for q in range(n_q)]
    l2a = ["a%d" % k for k in range(A)]
    mk = lambda shard: VQATorchDataset(VQADataset("train", data=data, ans2label={a: k for k, a in enumerate(l2a)}, label2ans=l2a), shard=shard)  # noqa: E731
    batcher = SentenceBatcher(C.tokenizer(), 20)
    ts_lab, ts_mat = mk(lab), mk(mat)
    return ts_lab, ResidentDataset(ts_lab, batcher, DEV), ts_mat, ResidentDataset(ts_mat, batcher, DEV)


@pytest.mark.parametrize("N", [36, 37, 100])
def test_gather_makes_adj_true_from_labels(N):
    """``fill`` of the label store and of its twin: ``adj_true`` ``torch.equal`` (N = 36: the twin copies vectors; 37:
    element by element; 100: the long kernel made the twin's table), every other output identical, the adjacency output in
    a band of sentinels; the host restatement and an item read back agree with the launch"""
    B, F, A = 5, 16, 29
    ts_lab, lab, ts_mat, mat = _stores(6, 9, N, F, A, seed=N)
    assert "adj" not in lab.tables and lab.tables["pair_table"].shape == (60, 45) and "pair_table" not in mat.tables
    assert lab.nbytes == mat.nbytes - 6 * N * N * 4 + 60 * 45 * 4 + 2 * 6 * N * 4

    def outputs():
        band = banded((B, N, N), F32, DEV)
        return band, dict(feats=torch.zeros(B, N, F, dtype=BF16, device=DEV), boxes=torch.zeros(B, N, 4, device=DEV), adj_true=band.view,
                          input_ids=torch.zeros(B, 20, dtype=torch.int64, device=DEV), input_mask=torch.zeros(B, 20, dtype=torch.int64, device=DEV),
                          segment_ids=torch.ones(B, 20, dtype=torch.int64, device=DEV), target=torch.ones(B, A, device=DEV),
                          sample=torch.zeros(B, dtype=torch.int64, device=DEV))
    (band_l, out_l), (band_m, out_m) = outputs(), outputs()
    lab.fill(out_l, 3, B)
    mat.fill(out_m, 3, B)
    torch.cuda.synchronize()
    assert out_l.keys() == out_m.keys()
    for k in out_l:
        assert torch.equal(out_l[k], out_m[k]), k
    assert band_l.untouched_outside() and band_m.untouched_outside()
    assert out_l["sample"].tolist() == [3, 4, 5, 6, 7] and float(out_l["adj_true"].amax(dim=(1, 2)).min()) == 1.0
    host = lab.host_batch([3, 4, 5, 6, 7])
    for k, v in host.items():
        assert torch.equal(out_l[k].cpu(), v), k
    item, twin_item = ts_lab[4], ts_mat[4]
    assert np.array_equal(item[5], twin_item[5]) and np.array_equal(item[5], out_l["adj_true"][1].cpu().numpy())
    # a fill without the adjacency output, and a store with neither source
    lab.fill({k: v for k, v in out_l.items() if k != "adj_true"}, 0, B)
    from xggm_amd import ops
    both = dict(lab.tables, adj=mat.tables["adj"])
    with pytest.raises(ValueError, match="one source"):
        ops.batch_gather(both, lab._order, 0, B, out_l)
    torch.cuda.synchronize()


def test_label_store_feeds_the_captured_trainer():
    """a ``CapturedTrainer`` fed by the label store and a twin fed by the store that holds the table: three iterations
    (rel, node, rel), the static inputs and then the whole state (weights, gradients, moments, counters) bit-equal"""
    from test_engine_gpu import _same_state, _tiny
    from xggm_amd.engine import CapturedTrainer
    B, A = 4, 29
    (cfg, m, opt), (_, m2, opt2) = _tiny(5, 11, layers=(2, 1, 1), vocab=96), _tiny(5, 11, layers=(2, 1, 1), vocab=96)
    assert cfg["hidden"] == 128
    _, lab, _, mat = _stores(8, 12, 36, cfg["feat_dim"], A, seed=3)
    order = lab.order(0, seed=4, batch_size=B)
    assert mat.order(0, seed=4, batch_size=B).tolist() == order.tolist() and len(order) == 12
    batch0 = {k: v.to(DEV) for k, v in lab.host_batch(order[:B]).items() if k != "sample"}
    tr, tr2 = CapturedTrainer(m, opt, batch0, warmup_iters=1), CapturedTrainer(m2, opt2, batch0, warmup_iters=1)
    for k, branch in enumerate(("rel", "node", "rel")):
        tr.load_resident(lab, k * B)
        tr2.load_resident(mat, k * B)
        for kk, v in tr.static.items():
            assert torch.equal(v, tr2.static[kk]), (k, kk)
        assert torch.equal(tr.static["adj_true"].cpu(), lab.host_batch(order[k * B:(k + 1) * B])["adj_true"])
        la, lb = tr.iteration(branch), tr2.iteration(branch)
        assert [float(x[0]) for x in la] == [float(x[0]) for x in lb]
        _same_state(m, m2)
    for (k1, p1), (k2, p2) in zip(m.state_dict().items(), m2.state_dict().items()):
        assert k1 == k2 and torch.equal(p1, p2), k1
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------- 5. the label encoder
def test_label_encoder_matches_the_transformers_golden():
    """``embed_labels`` over the package's own layers, fp32, against the pooled outputs a ``transformers`` BertModel gave
    for the same seeded weights: within 1e-4 x max|golden| (the project's fp32 tensor bound), in one batch and in batches
    of 5 (other paddings); the fixture script asserts that two labels, and the unmasked run, differ by 100 x that"""
    from xggm_amd.preprocess.compute_adjacency import build_adjacency_from_labels, label_pair_table
    from xggm_amd.preprocess.label_embeddings import LabelEncoder, embed_labels, load_label_encoder
    g = load_golden("bert_tiny")
    cfg = C.tiny_config()
    shapes = {k: tuple(v.shape) for k, v in LabelEncoder(cfg).state_dict().items()}
    enc = load_label_encoder(cfg, C.tiny_bert_state(shapes, int(g["seed"])), DEV)
    labels, gold = [str(s) for s in g["labels"]], torch.from_numpy(g["pooled"])
    bound = C.REL_BOUND * float(gold.abs().max())
    one = embed_labels(enc, C.tokenizer(), labels)
    five = embed_labels(enc, C.tokenizer(), labels, batch=5)
    assert one.shape == (24, 128) and one.dtype == F32 and one.is_cuda and five.shape == one.shape
    e1, e5, e15 = (float(d.abs().max()) for d in (one.cpu().double() - gold, five.cpu().double() - gold, (one - five).cpu().double()))
    print("embed_labels against the golden: one batch %.3e, batches of 5 %.3e, between them %.3e (bound %.3e)" % (e1, e5, e15, bound))
    assert e1 <= bound and e5 <= bound and e15 <= bound
    # the whole path: labels -> tables -> pair table -> an image's adjacency
    adj = build_adjacency_from_labels(label_pair_table(one[:16], one[16:]), torch.arange(16).view(1, 16) % 16, torch.arange(16).view(1, 16) % 8)
    assert bool(torch.isfinite(adj).all()) and float(adj.max()) == 1.0 and torch.equal(adj, adj.transpose(1, 2))
