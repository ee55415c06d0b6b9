"""Device-resident data set on the GPU: ``ops.batch_gather`` against its numpy restatement (``tools.resident.gather_host``,
which tests/test_resident_cpu.py holds to the loader's collation) -- every field bit for bit, inside canary buffers -- and
the store feeding ``CapturedTrainer.load_resident`` / ``CapturedPredictor.push_resident`` / ``predict(resident=)`` against
twins fed by ``DataLoaderX``."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from xggm_amd import synth  # noqa: E402
from helpers import GOLDEN  # noqa: E402

DEV = "cuda"
BF16 = torch.bfloat16
N_IMG, N_Q, T, N_ORDER = 6, 13, 20, 20
_INT = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


# ----------------------------------------------------------------------------- 1. the kernel
class Canary:
    """``rows`` rows of ``row_shape`` at a row stride of ``stride`` elements, ``lead`` elements into a larger buffer whose
    every byte holds 0xA5: ``view`` is what the kernel writes, ``untouched(B)`` says whether every byte outside rows
    0 .. B - 1 -- in front of the first row, between two rows, behind row B - 1 -- still holds the sentinel"""

    def __init__(self, rows, row_shape, dtype, lead, stride=None):
        esz = torch.empty((), dtype=dtype).element_size()
        row = int(np.prod(row_shape)) if row_shape else 1
        self.stride, self.lead, self.row_shape = stride or row, lead, tuple(row_shape)
        self.raw = torch.full(((lead + rows * self.stride + 5) * esz,), 0xA5, dtype=torch.uint8, device=DEV)
        self.ints = self.raw.view(_INT[esz])
        self.view = self._rows(self.ints, rows).view(dtype)

    def _rows(self, base, rows):
        inner = list(np.cumprod((self.row_shape + (1,))[::-1])[::-1][1:])
        return torch.as_strided(base, (rows,) + self.row_shape, [self.stride] + [int(i) for i in inner], self.lead)

    def untouched(self, B):
        written = torch.zeros_like(self.ints)
        self._rows(written, B).fill_(-1)  # every byte of a written element
        return bool((self.raw[written.view(torch.uint8) == 0] == 0xA5).all())


def _tables(N, F, A, K, f32, seed=0):
    """host tables in the kernel's layout: 13 samples over 6 images (images repeat), label slots partly unused"""
    rng = np.random.default_rng([seed, N, F, A, K, int(f32)])
    if f32:
        feats = rng.standard_normal((N_IMG, N, F)).astype(np.float32)
        special = np.array([0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000,  # ties: to even (down), to even (up), negative
                            0x3F808001, 0x3F807FFF,                          # just above / below a tie
                            0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F8000, 0x7F7F7FFF,  # round up to +-inf; the tie; the largest survivor
                            0x7F800000, 0x00000001, 0x80000001, 0x00008000, 0x00018000, 0x007FFFFF, 0x807FFFFF,  # inf, denormals
                            0x00000000, 0x80000000], dtype=np.uint32).view(np.float32)
        feats.reshape(-1)[:len(special)] = special            # image 0
        feats[N_IMG - 1].reshape(-1)[-len(special):] = special  # the last run of the last image
    else:
        feats = rng.integers(0, 1 << 16, (N_IMG, N, F), dtype=np.uint16)
    t = dict(feats=feats, boxes=rng.random((N_IMG, N, 4), dtype=np.float32), adj=rng.random((N_IMG, N, N), dtype=np.float32))
    t["q_row"] = rng.integers(0, N_IMG, N_Q).astype(np.int32)
    t["q_row"][:2] = (0, N_IMG - 1)
    t["q_len"] = rng.integers(2, T + 1, N_Q).astype(np.int32)
    t["q_len"][:2] = (T, 2)
    t["q_ids"] = (rng.integers(1, 30000, (N_Q, T)) * (np.arange(T)[None] < t["q_len"][:, None])).astype(np.int32)
    t["q_label"] = np.full((N_Q, K), -1, dtype=np.int32)
    for s in range(N_Q):
        used = s % (K + 1) if s > 1 else K          # sample 2 (K = 1: and others) has no label at all
        t["q_label"][s, :used] = rng.choice(A, size=used, replace=False)
    t["q_label"][0, 0], t["q_label"][1, 0] = A - 1, 0  # the two ends of a target row
    if K > 1:
        t["q_label"][0, 1:], t["q_label"][1, 1:] = np.arange(1, K), np.arange(A - K, A - 1)
    t["q_score"] = rng.random((N_Q, K), dtype=np.float32)
    t["q_bias_index"] = rng.integers(0, 1 << 40, N_Q).astype(np.int64)
    return t


def _to_device(t):
    out = {}
    for k, v in t.items():
        if v.dtype == np.uint16:
            out[k] = torch.from_numpy(v.view(np.int16).copy()).view(BF16).to(DEV)
        else:
            out[k] = torch.from_numpy(v).to(DEV)
    return out


def _order(seed=0):
    o = np.random.default_rng([7, seed]).integers(0, N_Q, N_ORDER).astype(np.int64)  # samples (and so images) repeat
    o[-7:-3] = (0, 1, 2, 0)
    return o


def _bits(t):
    return t.contiguous().view(_INT[t.element_size()])


def _canaries(R, N, F, A, out_f32):
    """every output inside a sentinel buffer; leads keep feats / boxes 16-byte aligned and put target and an odd-N adj on
    4-byte boundaries only; feats and target rows are padded (stride > row)"""
    return dict(feats=Canary(R, (N, F), torch.float32 if out_f32 else BF16, lead=8, stride=N * F + 8),
                boxes=Canary(R, (N, 4), torch.float32, lead=4),
                adj_true=Canary(R, (N, N), torch.float32, lead=4 if N % 2 == 0 else 1),
                input_ids=Canary(R, (T,), torch.int64, lead=2), input_mask=Canary(R, (T,), torch.int64, lead=1),
                segment_ids=Canary(R, (T,), torch.int64, lead=3),
                target=Canary(R, (A,), torch.float32, lead=1, stride=A + 3),
                bias_index=Canary(R, (), torch.int64, lead=1), sample=Canary(R, (), torch.int64, lead=2))


def _check(c, ref, B, what):
    for k, cv in c.items():
        got = cv.view[:B].cpu()
        assert got.dtype == ref[k].dtype and got.shape == ref[k].shape, (what, k)
        assert torch.equal(_bits(got), _bits(ref[k])), (what, k)  # bits: -0.0, inf and denormals count
        assert cv.untouched(B), (what, k, "bytes outside rows 0 .. B - 1 were written")


@pytest.mark.parametrize("N,F", [(36, 64), (5, 8)])
@pytest.mark.parametrize("feats_f32,out_f32", [(False, False), (False, True), (True, False), (True, True)])
def test_batch_gather_equals_the_host_restatement(N, F, feats_f32, out_f32):
    """every field ``torch.equal`` (on the bit patterns) to ``gather_host`` for A in {29, 2274} (4-byte-aligned target
    rows), K in {1, 3}, B in {1, 4, 7} ending exactly at the end of an order with repeated samples and images; odd N gives
    100-byte adjacency rows; fp32 tables hold rounding ties, values that round up to inf and denormals.  Every output sits
    in a sentinel buffer: nothing in front of the first row, in the padding between rows or in rows b >= B is written."""
    from xggm_amd import ops
    from xggm_amd.tools.resident import gather_host
    order = _order()
    d_order = torch.from_numpy(order).to(DEV)
    for A in (29, 2274):
        for K in (1, 3):
            host = _tables(N, F, A, K, feats_f32)
            dev = _to_device(host)
            for B, start in ((1, N_ORDER - 1), (4, N_ORDER - 4), (7, N_ORDER - 7), (4, 0)):
                c = _canaries(B + 2, N, F, A, out_f32)
                ops.batch_gather(dev, d_order, start, B, {k: v.view for k, v in c.items()})
                ref = gather_host(host, order[start:start + B], A, out_f32=out_f32)
                _check(c, ref, B, (A, K, B, start))
    if feats_f32 and not out_f32:  # the planted values are in the batches above: more infinities out than went in
        last = gather_host(host, order[N_ORDER - 7:], A)["feats"]
        assert int(torch.isinf(last.float()).sum()) > int(np.isinf(host["feats"][host["q_row"][order[N_ORDER - 7:]]]).sum()) > 0


def test_batch_gather_optional_fields_and_refusals():
    """target / adj_true / bias_index / sample may be left out (the predictor has none of them); what the launch cannot
    honour is refused before it: F % 8, rows outside the order, a misaligned feature buffer, a short output"""
    from xggm_amd import ops
    from xggm_amd.tools.resident import gather_host
    N, F, A, K, B = 5, 8, 29, 3, 4
    host = _tables(N, F, A, K, False)
    dev = _to_device(host)
    order = _order()
    d_order = torch.from_numpy(order).to(DEV)
    c = _canaries(B + 1, N, F, A, True)
    few = {k: c[k] for k in ("feats", "boxes", "input_ids", "input_mask", "segment_ids")}
    no_adj = {k: v for k, v in dev.items() if k not in ("adj", "q_bias_index")}
    ops.batch_gather(no_adj, d_order, 3, B, {k: v.view for k, v in few.items()})
    _check(few, gather_host(host, order[3:3 + B], A, out_f32=True), B, "few")
    outs = {k: v.view for k, v in c.items()}
    with pytest.raises(ValueError, match="adjacency"):
        ops.batch_gather(no_adj, d_order, 0, B, outs)
    for start, b in ((N_ORDER - 3, 4), (-1, 2), (0, 0), (0, B + 2)):
        with pytest.raises(ValueError):
            ops.batch_gather(dev, d_order, start, b, outs)
    bad = dict(dev, feats=dev["feats"][:, :, :4].contiguous())
    with pytest.raises(ValueError, match="multiple of 8"):
        ops.batch_gather(bad, d_order, 0, B, dict(outs, feats=torch.zeros(B, N, 4, device=DEV)))
    off = Canary(B, (N, F), torch.float32, lead=1, stride=N * F + 8)  # 4 bytes into the buffer
    with pytest.raises(RuntimeError, match="16-byte"):
        ops.batch_gather(dev, d_order, 0, B, dict(outs, feats=off.view))
    odd = Canary(B, (N, F), torch.float32, lead=8, stride=N * F + 4)
    with pytest.raises(RuntimeError, match="multiple of 8"):
        ops.batch_gather(dev, d_order, 0, B, dict(outs, feats=odd.view))
    torch.cuda.synchronize()
    assert off.untouched(0) and odd.untouched(0)


def test_batch_gather_replays_follow_the_order():
    """captured in a graph (nothing in the call allocates, copies or synchronises) and replayed twice with ``order``
    rewritten in between: the replay reads the order it finds"""
    from xggm_amd import ops
    from xggm_amd.tools.resident import gather_host
    N, F, A, K, B, start = 36, 64, 2274, 3, 7, 5
    host = _tables(N, F, A, K, True)
    dev = _to_device(host)
    o1, o2 = _order(1), _order(2)
    assert o1[start:start + B].tolist() != o2[start:start + B].tolist()
    d_order = torch.from_numpy(o1).to(DEV)
    c = _canaries(B + 1, N, F, A, False)
    outs = {k: v.view for k, v in c.items()}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.batch_gather(dev, d_order, start, B, outs)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.batch_gather(dev, d_order, start, B, outs)
    for o in (o1, o2):
        d_order.copy_(torch.from_numpy(o))
        for cv in c.values():
            cv.raw.fill_(0xA5)
        g.replay()
        _check(c, gather_host(host, o[start:start + B], A), B, "replay")


# ----------------------------------------------------------------------------- 2. the store
def _tok():
    from xggm_amd.lxrt.tokenization import BertTokenizer
    return BertTokenizer(os.path.join(GOLDEN, "vocab_small.txt"), do_lower_case=True)


def _shard(tmp_path, n_img, n_q, F, A, vocab, seed=21):
    """a synthetic shard of ``n_img`` images and a data set of ``n_q`` questions over them (images are shared), one to
    three answers each"""
    from xggm_amd.tools.shards import ShardWriter
    from xggm_amd.vqa.vqacpv2_data import VQADataset, VQATorchDataset
    words = [w for w in open(os.path.join(GOLDEN, "vocab_small.txt")).read().split() if w.isalpha()][:40]
    rng = np.random.default_rng(0)
    w = ShardWriter(str(tmp_path / "train_obj36.xgs"), n_objects=36, feat_dim=F)
    bsrc = synth.vqa_batch(n_img, A=A, F=F, vocab=vocab, seed=seed)
    for i in range(n_img):
        w.add(i, bsrc["feats"][i], bsrc["boxes"][i] * 0.99, 1.0, 1.0, bsrc["adj_true"][i])
    data = []
    for q in range(n_q):
        k = 1 + q % 3
        data.append({"question_id": 100 + q, "image_id": int((5 * q) % n_img), "label": [int(x) for x in rng.choice(A, k, replace=False)],
                     "score": [float(x) for x in rng.choice([0.3, 0.6, 0.9, 1.0], k)],
                     "question": " ".join(rng.choice(words, size=int(rng.integers(3, 9))))})
    l2a = ["a%d" % k for k in range(A)]
    return VQATorchDataset(VQADataset("train", data=data, ans2label={a: k for k, a in enumerate(l2a)}, label2ans=l2a),
                           shard=w.close())


def _items_equal(static, ts, samples):
    """the static input buffers hold the host items of ``samples`` (features as their bf16 values)"""
    host = [ts[int(s)] for s in samples]
    assert torch.equal(static["feats"].float().cpu(), torch.from_numpy(np.stack([h[1] for h in host])))
    assert torch.equal(static["boxes"].cpu(), torch.from_numpy(np.stack([h[2] for h in host])))
    assert torch.equal(static["target"].cpu(), torch.stack([h[4] for h in host]))
    assert torch.equal(static["adj_true"].cpu(), torch.from_numpy(np.stack([h[5] for h in host])))


def _trainer_pair(tmp_path, debias):
    from test_engine_gpu import _tiny
    from test_model_gpu import build_model
    from oracle import shapes
    from xggm_amd.lxrt.entry import SentenceBatcher
    from xggm_amd.tools.resident import ResidentDataset
    from xggm_amd.vqa.vqacpv2 import attach_debias_loss, make_optimizer
    B, A, n_img, n_q = 4, 29, 8, 12
    models = []
    for _ in range(2):
        if not debias:
            cfg, m, opt = _tiny(5, 11, vocab=96)  # the test vocabulary has 81 entries: every id inside the embedding table
        else:
            from xggm_amd.module.vqa_debias_loss_functions import LearnedMixin
            cfg = dict(shapes.TINY, l_layers=2, x_layers=2, r_layers=1, vocab=96)
            m = build_model(cfg, A, seed=5, dt=BF16)
            m.seed = 11
            dl = LearnedMixin(0.36, hidden_dim=cfg["hidden"])
            dl.load_state_dict({k: torch.from_numpy(synth.seeded_param("debias_loss." + k, v.shape, 5)) for k, v in dl.state_dict().items()})
            dl.set_bias_table(synth.debias_case(3, A, 0, 31)["bias"])
            attach_debias_loss(m, dl)
            opt = make_optimizer(m, 1e-4, 40)
        models.append((m, opt))
    ts = _shard(tmp_path, n_img, n_q, cfg["feat_dim"], A, cfg["vocab"])
    batcher = SentenceBatcher(_tok(), 20)
    groups = (np.arange(n_q) * 2) % 3 if debias else None
    store = ResidentDataset(ts, batcher, DEV, bias_index=groups, chunk_bytes=1 << 16)  # several staging chunks
    assert store.tables["feats"].shape[0] == n_img and store.tables["feats"].dtype == BF16
    return B, ts, batcher, store, groups, models


def test_store_feeds_the_captured_trainer(tmp_path):
    """one engine fed by ``load_resident`` over ``order(0)``, a twin fed the same samples through ``DataLoaderX`` +
    ``load_batch``: after each of 3 iterations the losses of every pass and the whole state (weights, gradients, moments,
    counters) are equal bit for bit, and the static buffers hold the host items"""
    from test_engine_gpu import _same_state
    from xggm_amd.engine import CapturedTrainer
    from xggm_amd.tools.data_loader import DataLoaderX
    B, ts, batcher, store, _, ((m, opt), (m2, opt2)) = _trainer_pair(tmp_path, False)
    seed = 4
    order = store.order(0, seed=seed, batch_size=B)
    assert len(order) == 12 and order.tolist() != list(range(12))
    batch0 = {k: v.to(DEV) for k, v in store.host_batch(order[:B]).items() if k != "sample"}
    tr = CapturedTrainer(m, opt, batch0, warmup_iters=1)
    tr2 = CapturedTrainer(m2, opt2, batch0, warmup_iters=1)
    losses, losses2 = [], []
    loader = DataLoaderX(ts, B, shuffle=True, seed=seed, drop_last=True, device=DEV, batcher=batcher)
    for k, (qid, feats, boxes, sent, target, adj) in enumerate(loader):
        tr.load_resident(store, k * B)
        samples = order[k * B:(k + 1) * B]
        assert store.ques_ids(samples) == qid
        _items_equal(tr.static, ts, samples)
        want = store.host_batch(samples)
        for kk, v in tr.static.items():
            assert torch.equal(v.cpu(), want[kk]), kk
        tr2.load_batch(dict(feats=feats, boxes=boxes, input_ids=sent[0], input_mask=sent[1], segment_ids=sent[2], target=target,
                            adj_true=adj))
        for kk, v in tr.static.items():
            assert torch.equal(v, tr2.static[kk]), kk
        (lp, _, _), (lg, _, _) = tr.iteration("rel")
        (lp2, _, _), (lg2, _, _) = tr2.iteration("rel")
        losses.append((float(lp), float(lg)))
        losses2.append((float(lp2), float(lg2)))
        _same_state(m, m2)
    assert len(losses) == 3 and losses == losses2, (losses, losses2)
    bad = dict(tr.static, target=torch.zeros(B, 28, device=DEV))
    with pytest.raises(ValueError, match="A=29"):
        store.fill(bad, 0, B)
    with pytest.raises(ValueError):
        tr.load_resident(store, 12 - B + 1)  # the captured batch would run past the order
    torch.cuda.synchronize()


def test_store_feeds_a_bias_index_loss(tmp_path):
    """with a ``bias_index``-taking loss attached ``load_resident`` fills ``static["bias_index"]`` from the store, and one
    iteration equals the ``load_batch`` twin; a store without bias_index is refused for such a loss"""
    from test_engine_gpu import _same_state
    from xggm_amd.engine import CapturedTrainer
    from xggm_amd.lxrt.entry import SentenceBatcher
    from xggm_amd.tools.resident import ResidentDataset
    B, ts, batcher, store, groups, ((m, opt), (m2, opt2)) = _trainer_pair(tmp_path, True)
    order = store.order(0, seed=2, batch_size=B)
    first = {k: v.to(DEV) for k, v in store.host_batch(order[:B]).items() if k != "sample"}
    assert first["bias_index"].tolist() == groups[order[:B]].tolist()
    tr = CapturedTrainer(m, opt, first, warmup_iters=1)
    tr2 = CapturedTrainer(m2, opt2, first, warmup_iters=1)
    samples = order[B:2 * B]
    tr.load_resident(store, B)
    assert tr.static["bias_index"].tolist() == groups[samples].tolist()
    tr2.load_batch({k: v.to(DEV) for k, v in store.host_batch(samples).items()})
    a, b = tr.iteration("rel"), tr2.iteration("rel")
    assert float(a[0][0]) == float(b[0][0]) and float(a[1][0]) == float(b[1][0])
    _same_state(m, m2)
    bare = ResidentDataset(ts, SentenceBatcher(_tok(), 20), DEV)
    with pytest.raises(ValueError, match="bias_index"):
        tr.load_resident(bare, 0)
    torch.cuda.synchronize()


def test_predict_sweeps_the_store(tmp_path):
    """``predict(..., resident=store)`` returns the ``quesid2ans`` of the loader-fed ``predict`` on 13 samples at batch 4
    (the last batch is ragged), with a plain and with a logging predictor; the logged labels pair with ``store.ques_ids``"""
    from test_engine_gpu import _tiny
    from xggm_amd.engine import AnswerLog, CapturedPredictor
    from xggm_amd.lxrt.entry import SentenceBatcher
    from xggm_amd.tools.data_loader import DataLoaderX
    from xggm_amd.tools.resident import ResidentDataset
    from xggm_amd.vqa.vqacpv2 import predict
    B, A, n = 4, 29, 13
    cfg, m, _ = _tiny(5, 11, vocab=96)
    ts = _shard(tmp_path, 6, n, cfg["feat_dim"], A, cfg["vocab"])
    batcher = SentenceBatcher(_tok(), 20)
    store = ResidentDataset(ts, batcher, DEV)
    dset = ts.raw_dataset
    pred = CapturedPredictor(m, B)
    want = predict(m, (dset, DataLoaderX(ts, B, batcher=batcher), None), predictor=pred)
    assert sorted(want) == list(range(100, 100 + n))
    assert predict(m, (dset, None, None), predictor=pred, resident=store) == want
    # the ragged last batch (one sample) sits in row 0 of the predictor's fp32 buffers, the rows behind it are the batch before
    last, prev = store.host_batch([n - 1], out_f32=True), store.host_batch(range(n - 1 - B, n - 1), out_f32=True)
    assert torch.equal(pred.static["feats"].cpu(), torch.cat([last["feats"], prev["feats"][1:]]))
    assert torch.equal(pred.static["boxes"].cpu(), torch.cat([last["boxes"], prev["boxes"][1:]]))
    assert torch.equal(pred.static["ids"][:, 0].cpu(), torch.stack([last[k][0] for k in ("input_ids", "input_mask", "segment_ids")]))
    assert torch.equal(pred.static["ids"][0, 1:].cpu(), prev["input_ids"][1:])
    log = AnswerLog(n, DEV, with_scores=False)
    logging = CapturedPredictor(m, B, log=log)
    assert predict(m, (dset, None, None), predictor=logging, resident=store) == want
    labels, _, _, count = log.read()
    assert count == n
    assert {q: dset.label2ans[l] for q, l in zip(store.ques_ids(np.arange(n)), labels.tolist())} == want
    with pytest.raises(ValueError):
        logging.push_resident(store, 0, B + 1)
    with pytest.raises(ValueError, match="predictor"):
        predict(m, (dset, None, None), resident=store)
    torch.cuda.synchronize()
