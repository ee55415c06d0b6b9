"""The device TSV reader on the GPU: ``ops.tsv_decode`` against its numpy restatement (``tsv_decode_host``, which
tests/test_tsv_ingest_cpu.py holds to the host path) -- every table bit for bit, inside sentinel bands --, ``load_obj_tsv_device``
against the reference reader's arrays, across chunk sizes and planted faults, and the stores adopting its table."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import tsv_cases as C  # noqa: E402
from helpers import GOLDEN  # noqa: E402
from xggm_amd import utils  # noqa: E402
from xggm_amd.tools import tsv  # noqa: E402

DEV = "cuda"
BAND = 2
SENTINEL = 0x5A


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _bits(t):
    """a table tensor as the numpy array the host restatement holds (bf16: uint16 bit patterns)"""
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16).numpy().view(np.uint16) if t.dtype == torch.bfloat16 else t.numpy()


def _flags(table):
    return table.flags.cpu().numpy().view(np.uint32)


def _same_table(table, want):
    assert C.same_feats(_bits(table.feats), want["feats"])
    for k in tsv.IMAGE_TABLES[1:]:
        got = _bits(getattr(table, k))
        assert got.dtype == want[k].dtype and np.array_equal(got, want[k]), k


# ----------------------------------------------------------------------------- 1. the reference reader's arrays
def _golden_by_shape(tmp_path):
    """the golden file's lines, unchanged, one file per (O, F) (the device reader takes one box count per file), with the
    reference reader's items for them"""
    g = np.load(os.path.join(GOLDEN, "obj_tsv.npz"))
    lines = open(os.path.join(GOLDEN, "obj_tsv_small.tsv"), "rb").read().split(b"\n")[:-1]
    items = [{k: (g["%d/%s" % (i, k)] if g["%d/%s" % (i, k)].ndim else g["%d/%s" % (i, k)].item()) for k in utils.FIELDNAMES}
             for i in range(len(lines))]
    out = []
    for O, F in C.SMALL:
        sel = [i for i, it in enumerate(items) if int(it["num_boxes"]) == O]
        assert len(sel) == 2
        p = tmp_path / ("golden_%d.tsv" % O)
        p.write_bytes(b"".join(lines[i] + b"\n" for i in sel))
        recs = [dict(items[i], img_h=int(items[i]["img_h"]), img_w=int(items[i]["img_w"])) for i in sel]
        out.append((str(p), recs))
    return out


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("feats_bf16", [True, False])
def test_golden_file_equals_the_reference_readers_arrays(tmp_path, feats_bf16, normalize):
    for path, recs in _golden_by_shape(tmp_path):
        table = tsv.load_obj_tsv_device(path, DEV, feats_bf16=feats_bf16, normalize=normalize)
        assert table.last_host_rows == 0 and table.ids == [str(r["img_id"]) for r in recs]
        assert table.img_h.tolist() == [r["img_h"] for r in recs] and table.img_w.tolist() == [r["img_w"] for r in recs]
        _same_table(table, C.expected(recs, feats_bf16, normalize))


# ----------------------------------------------------------------------------- 2. every case, launched directly
CASES = [(O, F, n) for O, F in C.SHAPES[:4] for n in (1, 3, 65)] + [(O, F, n) for O, F in C.SHAPES[4:] for n in (1, 3)]
CASES += [C.MAX_BOXES + (n,) for n in (1, 3, 65)]


def _launch(data, ch, O, F, feats_bf16, normalize, row0=BAND, cap=None):
    """one direct launch into sentinel-filled tables -> (tables as numpy, flags, counts); the text allocation is the
    smallest the contract allows: the bytes rounded up to 16"""
    from xggm_amd import ops
    n = ch.n
    cap = n + 2 * BAND if cap is None else cap
    text = torch.full(((len(data) + 15) // 16 * 16,), SENTINEL, dtype=torch.uint8)
    text[:len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8)
    size = lambda dt: torch.empty(0, dtype=dt).element_size()
    fill = lambda shape, dt: torch.full(tuple(shape[:-1]) + (shape[-1] * size(dt),), SENTINEL, dtype=torch.uint8, device=DEV).view(dt)
    tb = dict(feats=fill((cap, O, F), torch.bfloat16 if feats_bf16 else torch.float32), boxes=fill((cap, O, 4), torch.float32),
              obj_labels=fill((cap, O), torch.int32), attr_labels=fill((cap, O), torch.int32),
              obj_confs=fill((cap, O), torch.float32), attr_confs=fill((cap, O), torch.float32))
    flags, counts = fill((n,), torch.int32), torch.zeros(2, dtype=torch.int32, device=DEV)
    ops.tsv_decode(text.to(DEV), len(data), torch.from_numpy(ch.desc).to(DEV), ch.desc, O, F, tb, row0, flags=flags, counts=counts,
                   normalize=normalize)
    torch.cuda.synchronize()
    return {k: _bits(v) for k, v in tb.items()}, flags.cpu().numpy().view(np.uint32), counts.cpu().numpy()


def _check_launch(got, flags, counts, want, n, row0=BAND):
    sent = {1: SENTINEL, 2: SENTINEL * 0x0101, 4: SENTINEL * 0x01010101}
    for k in tsv.IMAGE_TABLES:
        rows, w = got[k][row0:row0 + n], want[k]
        assert rows.dtype == w.dtype
        assert C.same_feats(rows, w) if k == "feats" else np.array_equal(rows.view(np.uint32), w.view(np.uint32)), k
        outside = np.delete(got[k], np.s_[row0:row0 + n], 0)
        word = outside.view(np.uint16 if outside.dtype.itemsize == 2 else np.uint32)
        assert outside.shape[0] == got[k].shape[0] - n and (word == sent[outside.dtype.itemsize]).all(), k  # the bands keep the sentinel
    assert np.array_equal(flags, want["flags"]) and not (flags == sent[4]).any()
    assert counts.tolist() == want["counts"].tolist()


@pytest.mark.parametrize("feats_bf16,normalize", [(True, True), (False, False)])
@pytest.mark.parametrize("O,F,n", CASES)
def test_direct_launch_equals_the_host_restatement(tmp_path, O, F, n, feats_bf16, normalize):
    data, ch, want = C.host_decode(tmp_path, O, F, n, feats_bf16, normalize)
    got, flags, counts = _launch(data, ch, O, F, feats_bf16, normalize)
    _check_launch(got, flags, counts, want, n)


@pytest.mark.parametrize("feats_bf16,normalize", [(True, False), (False, True)])
def test_direct_launch_other_combinations_and_row0(tmp_path, feats_bf16, normalize):
    O, F, n = 5, 24, 3
    data, ch, want = C.host_decode(tmp_path, O, F, n, feats_bf16, normalize)
    for row0, cap in ((0, n), (7, n + 7), (1, n + 4)):
        got, flags, counts = _launch(data, ch, O, F, feats_bf16, normalize, row0=row0, cap=cap)
        _check_launch(got, flags, counts, want, n, row0=row0)


def test_flags_do_not_depend_on_the_tables_asked_for(tmp_path):
    """without a feats table (or with flags alone) a bad character and a non-finite value in the features are still flagged
    and counted"""
    from xggm_amd import ops
    O, F, n = 3, 8, 5
    data, ch, _ = C.host_decode(tmp_path, O, F, n)
    t = C.field_text(data, ch, 2, 5)
    bad = C.replace_field(data, ch, 2, 5, t[:40] + b"*" + t[41:])
    want = tsv.tsv_decode_host(bad, ch.desc, O, F)
    assert want["flags"][2] & tsv.BAD_CHAR and (want["flags"] & tsv.NONFINITE).any() and want["counts"].tolist() == [1, 0]
    text = torch.zeros((len(bad) + 15) // 16 * 16, dtype=torch.uint8)
    text[:len(bad)] = torch.frombuffer(bytearray(bad), dtype=torch.uint8)
    text, desc = text.to(DEV), torch.from_numpy(ch.desc).to(DEV)
    for keys in ((), ("boxes", "obj_labels")):
        tb = {"boxes": torch.zeros((n, O, 4), device=DEV), "obj_labels": torch.zeros((n, O), dtype=torch.int32, device=DEV)}
        flags, counts = torch.full((n,), -1, dtype=torch.int32, device=DEV), torch.zeros(2, dtype=torch.int32, device=DEV)
        ops.tsv_decode(text, len(bad), desc, ch.desc, O, F, {k: tb[k] for k in keys}, 0, flags=flags, counts=counts)
        assert np.array_equal(flags.cpu().numpy().view(np.uint32), want["flags"]) and counts.tolist() == want["counts"].tolist()
        for k in keys:
            assert np.array_equal(_bits(tb[k]).view(np.uint32), want[k].view(np.uint32)), k


# ----------------------------------------------------------------------------- 3. special values
def test_special_values_bf16_as_torch_boxes_as_numpy(tmp_path):
    O, F, n = 3, 8, 20
    recs = C.records(O, F, n)
    data, ch, _ = C.host_decode(tmp_path, O, F, n)
    got, flags, _ = _launch(data, ch, O, F, True, True)
    src = torch.from_numpy(np.stack([r["features"] for r in recs]))
    assert set(C.SPECIAL_BITS.tolist()) <= set(src.view(torch.int32).numpy().view(np.uint32).reshape(-1).tolist())
    ref = src.to(torch.bfloat16)
    mine = torch.from_numpy(got["feats"][BAND:BAND + n].view(np.int16).copy()).view(torch.bfloat16)
    nan = torch.isnan(src)
    assert torch.equal(torch.isnan(mine), nan) and torch.equal(mine.view(torch.int16)[~nan], ref.view(torch.int16)[~nan])
    for i, r in enumerate(recs):
        b = np.array(r["boxes"], dtype=np.float32)
        b[:, (0, 2)] /= r["img_w"]
        b[:, (1, 3)] /= r["img_h"]
        assert np.array_equal(got["boxes"][BAND + i].view(np.uint32), b.view(np.uint32)), i
    nonfinite = np.array([not np.isfinite(r["features"]).all() for r in recs])
    assert np.array_equal(flags, np.where(nonfinite, tsv.NONFINITE, 0).astype(np.uint32)) and nonfinite.any()


# ----------------------------------------------------------------------------- 4. chunking
def test_chunk_sizes_give_identical_tables(tmp_path):
    O, F, n = 5, 24, 40
    path, data = C.tsv_file(tmp_path, O, F, n)
    want = C.expected(C.records(O, F, n))
    fixed = sum(tsv.b64_len(b) for b in tsv.field_bytes(O, F)) + 10
    longest = max(len(l) for l in data.split(b"\n")) + 1
    one_line = fixed + 64  # the smallest size the reader takes: two lines do not fit
    assert longest <= one_line < 2 * (fixed + 4)
    tables = [tsv.load_obj_tsv_device(path, DEV, chunk_bytes=c) for c in (one_line, 2 * longest + longest // 2, len(data) + 100)]
    for t in tables:
        assert (t.n, t.N, t.F, t.last_host_rows) == (n, O, F, 0) and t.ids == [C.img_id_of(i) for i in range(n)]
        _same_table(t, want)
        assert not (_flags(t) & 0xFFEF).any()
    half = tsv.load_obj_tsv_device(path, DEV, chunk_bytes=one_line, topk=7)
    assert half.n == 7 and C.same_feats(_bits(half.feats), want["feats"][:7])
    with pytest.raises(ValueError, match="at least %d" % one_line):
        tsv.load_obj_tsv_device(path, DEV, chunk_bytes=one_line - 1)
    with pytest.raises(ValueError, match="limit"):
        tsv.load_obj_tsv_device(path, DEV, max_bytes=1000)
    crlf = tmp_path / "crlf.tsv"
    crlf.write_bytes(b"\r\n" + data.replace(b"\n", b"\r\n\r\n")[:-4])  # \r\n, blank lines, no final line end
    _same_table(tsv.load_obj_tsv_device(str(crlf), DEV, chunk_bytes=2 * longest + 7), want)


# ----------------------------------------------------------------------------- 5. faults
def _faulty(tmp_path, name, line, field, edit, O=3, F=8, n=5):
    data, ch, _ = C.host_decode(tmp_path, O, F, n)
    p = tmp_path / name
    p.write_bytes(C.replace_field(data, ch, line, field, edit(C.field_text(data, ch, line, field))))
    return str(p)


def test_a_line_the_host_can_read_is_patched(tmp_path):
    O, F, n = 3, 8, 5
    want = C.expected(C.records(O, F, n))
    for field in (5, 4, 0):
        path = _faulty(tmp_path, "spaces%d.tsv" % field, 2, field, lambda t: t[:4] + b"  " + t[4:9] + b" " + t[9:])
        table = tsv.load_obj_tsv_device(path, DEV)
        assert table.last_host_rows == 1
        _same_table(table, want)
        assert not (_flags(table) & 0xFFEF).any()


def test_lines_the_host_cannot_read_raise(tmp_path):
    names = {5: "features", 4: "boxes", 2: "attrs_id", 1: "objects_conf"}
    img = C.img_id_of(3)
    for field, name in names.items():
        for kind, edit in (("star", lambda t: t[:6] + b"*" + t[7:]), ("short", lambda t: t[:-4])):
            path = _faulty(tmp_path, "%s%d.tsv" % (kind, field), 3, field, edit)
            with pytest.raises(ValueError) as e:
                tsv.load_obj_tsv_device(path, DEV)
            assert repr(img) in str(e.value) and "field %s" % name in str(e.value) and os.path.basename(path) in str(e.value)
    ids = C.records(3, 8, 5)[3]["objects_id"].copy()
    ids[2] = -(1 << 31) - 1
    path = _faulty(tmp_path, "id.tsv", 3, 0, lambda t: C.reencode(ids, np.int64))
    with pytest.raises(ValueError) as e:
        tsv.load_obj_tsv_device(path, DEV)
    assert repr(img) in str(e.value) and "field objects_id" in str(e.value) and "int32" in str(e.value)


def test_box_range_and_box_count(tmp_path):
    O, F, n = 3, 8, 5
    recs = C.records(O, F, n)
    boxes = recs[1]["boxes"].copy()
    boxes[2, 0] = np.float32(1.001) * recs[1]["img_w"]
    path = _faulty(tmp_path, "box.tsv", 1, 4, lambda t: C.reencode(boxes, np.float32))
    with pytest.raises(ValueError, match=repr(C.img_id_of(1))):
        tsv.load_obj_tsv_device(path, DEV)
    table = tsv.load_obj_tsv_device(path, DEV, check_boxes=False)
    assert (_flags(table) & tsv.BAD_BOX).tolist() == [0, tsv.BAD_BOX, 0, 0, 0] and table.last_host_rows == 0
    want = boxes.copy()
    want[:, (0, 2)] /= recs[1]["img_w"]
    want[:, (1, 3)] /= recs[1]["img_h"]
    assert np.array_equal(_bits(table.boxes)[1], want)  # the row is written all the same
    assert not (_flags(tsv.load_obj_tsv_device(path, DEV, normalize=False)) & 0xFFEF).any()  # nothing to check without normalising
    # another num_boxes than the first line's
    _, d3 = C.tsv_file(tmp_path, 3, 8, 5)
    _, d2 = C.tsv_file(tmp_path, 2, 8, 3)
    mixed = tmp_path / "mixed.tsv"
    mixed.write_bytes(d3 + d2)
    with pytest.raises(ValueError, match="num_boxes 2, the first line has 3"):
        tsv.load_obj_tsv_device(str(mixed), DEV)


def test_a_file_of_short_lines_gets_a_named_error(tmp_path):
    """lines cut short outnumber what the file's size allows for whole lines: the error names file, line, img_id and field,
    whether the host path meets the first of them or the row bound is met first"""
    O, F = 3, 8
    data, ch, _ = C.host_decode(tmp_path, O, F, 5)
    lines = data.split(b"\n")[:-1]
    cut = lines[1].split(b"\t")
    cut[9] = cut[9][:8]  # the features: 8 characters of 128
    for name, body in (("few.tsv", lines[:1] + [b"\t".join(cut)] + lines[2:]), ("many.tsv", lines[:1] + [b"\t".join(cut)] * 40)):
        p = tmp_path / name
        p.write_bytes(b"\n".join(body) + b"\n")
        with pytest.raises(ValueError) as e:
            tsv.load_obj_tsv_device(str(p), DEV)
        msg = str(e.value)
        assert name in msg and repr(C.img_id_of(1)) in msg and "field features" in msg and "line at byte %d" % (len(lines[0]) + 1) in msg, msg


# ----------------------------------------------------------------------------- 6. the stores
def _same_batch(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, k
        x, y = a[k].contiguous().view(-1), b[k].contiguous().view(-1)
        if x.dtype.is_floating_point:  # bits, except at NaN positions: the kernel's NaN is payload free, torch's keeps some
            nan = torch.isnan(y)
            assert torch.equal(torch.isnan(x), nan), k
            x, y = x[~nan], y[~nan]
        assert torch.equal(x.view(torch.uint8), y.view(torch.uint8)), k


def test_pretrain_store_adopts_the_device_table(tmp_path):
    from test_tsv_ingest_cpu import _examples
    from xggm_amd.pretrain.resident import ResidentPretrainSet, pretrain_tables
    import pretrain_resident_cases as P
    path, _ = C.tsv_file(tmp_path, 5, 24, 4)
    recs = utils.load_obj_tsv(path)
    table = tsv.load_obj_tsv_device(path, DEV, feats_bf16=True)
    tok, T, K, B = P.tok(), 12, 3, 3
    mine = ResidentPretrainSet(pretrain_tables(_examples(recs, False, True), tok, T, K, n_answers=29, images=table), DEV, match_rate=0.5)
    twin = ResidentPretrainSet(_examples(recs, True, True), DEV, tokenizer=tok, max_seq_length=T, max_labels=K, n_answers=29,
                               feats_bf16=True, match_rate=0.5)
    assert mine.tables["feats"].data_ptr() == table.feats.data_ptr() and mine.nbytes == twin.nbytes
    for k in tsv.IMAGE_TABLES:
        assert mine.tables[k].data_ptr() == getattr(table, k).data_ptr(), k
    for st in (mine, twin):
        st.order(1, shuffle=True, seed=3, drop_last=True, batch_size=B)
    for start in (0, 3, 6):
        a, b = mine.fill(mine.buffers(B), start, B, swap=False), twin.fill(twin.buffers(B), start, B, swap=False)
        torch.cuda.synchronize()
        _same_batch(a, b)
    _same_batch(mine.host_batch([8, 0, 3]), twin.host_batch([8, 0, 3]))  # adopted tables are read back on first use


@pytest.mark.parametrize("kind", ["vqa", "gqa"])
def test_finetune_store_takes_the_device_table(tmp_path, kind):
    from xggm_amd.gqa.gqa_ood_data import GQADataset, GQATorchDataset
    from xggm_amd.lxrt.entry import SentenceBatcher
    from xggm_amd.preprocess.compute_adjacency import build_adjacency
    from xggm_amd.tools.resident import ResidentDataset
    from xggm_amd.tools.shards import ShardReader, ShardWriter
    from xggm_amd.vqa.vqacpv2_data import VQADataset, VQATorchDataset
    import pretrain_resident_cases as P
    O, F, n = 5, 24, 4
    path, _ = C.tsv_file(tmp_path, O, F, n, plain_ids=True)
    recs = utils.load_obj_tsv(path)
    table = tsv.load_obj_tsv_device(path, DEV)
    rng = np.random.default_rng(8)
    cls, att = (torch.from_numpy(rng.standard_normal((v, 16)).astype(np.float32)).to(DEV) for v in (1600, 400))
    table.set_adjacency(build_adjacency(cls, att, table.obj_labels, table.attr_labels))  # int32 ids, as they stand
    twin_adj = build_adjacency(cls, att, torch.from_numpy(np.stack([r["objects_id"] for r in recs])),
                               torch.from_numpy(np.stack([r["attrs_id"] for r in recs]))).cpu().numpy()
    w = ShardWriter(str(tmp_path / ("twin_%s.xgs" % kind)), n_objects=O, feat_dim=F)
    for r, a in zip(recs, twin_adj):
        w.add(r["img_id"], r["features"], r["boxes"], r["img_w"], r["img_h"], a)
    words = P.words()
    l2a = ["a%d" % i for i in range(7)]
    a2l = {a: i for i, a in enumerate(l2a)}
    img_of = [0, 3, 1, 1, 2, 0, 2]
    if kind == "vqa":
        data = [dict(question_id=100 + q, image_id=recs[i]["img_id"], question=" ".join(rng.choice(words, size=4)), label=[q % 7],
                     score=[0.5]) for q, i in enumerate(img_of)]
        mk = lambda shard: VQATorchDataset(VQADataset("train", data=data, ans2label=a2l, label2ans=l2a), shard=shard)
    else:
        data = [dict(question_id="q%d" % q, img_id=recs[i]["img_id"], sent=" ".join(rng.choice(words, size=4)),
                     label={l2a[q % 7]: 1.0}) for q, i in enumerate(img_of)]
        mk = lambda shard: GQATorchDataset(GQADataset("train", data=data, ans2label=a2l, label2ans=l2a), shard=shard)
    ts, ts_twin = mk(table), mk(ShardReader(w.close()))
    batcher = SentenceBatcher(P.tok(), 10)
    mine, twin = ResidentDataset(ts, batcher, DEV), ResidentDataset(ts_twin, batcher, DEV)
    for k in ("feats", "boxes", "adj"):
        assert mine.tables[k].data_ptr() == getattr(table, k).data_ptr(), k
    assert mine.nbytes == twin.nbytes and len(mine) == len(twin) == len(img_of)
    B = 3
    for st in (mine, twin):
        st.order(2, shuffle=True, seed=5, drop_last=True, batch_size=B)
    proto = twin.host_batch([0, 1, 2])
    for start in (0, 3):
        a, b = ({k: torch.zeros_like(v, device=DEV) for k, v in proto.items()} for _ in range(2))
        mine.fill(a, start, B), twin.fill(b, start, B)
        torch.cuda.synchronize()
        _same_batch(a, b)
    with pytest.raises(RuntimeError, match="ResidentDataset"):
        ts.collate([0, 1], ts_twin.alloc(2, False))
    item, item_twin = ts[1], ts_twin[1]
    assert np.array_equal(item[1], item_twin[1]) and np.array_equal(item[2], item_twin[2])  # one row read back
