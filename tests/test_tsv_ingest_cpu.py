"""Host side of the device TSV reader (xggm_amd.utils, xggm_amd.tools.tsv): the host path against the reference's own
reader, the writer's round trip, the field scanner, the numpy restatement of the kernel (the reference the kernel is held to
in tests/test_tsv_ingest_gpu.py) against the host path, the entry point's refusals, and the stores adopting a table.  No
kernel runs here."""
import ctypes
import os

import numpy as np
import pytest
import torch

import tsv_cases as C
from helpers import GOLDEN
from xggm_amd import utils
from xggm_amd.tools import tsv

GOLDEN_TSV = os.path.join(GOLDEN, "obj_tsv_small.tsv")


def _same_bits(a, b):
    """equality of two tensors / arrays / scalars in dtype, shape and BITS (the features hold NaNs)"""
    if torch.is_tensor(a) or torch.is_tensor(b):
        return torch.is_tensor(a) and torch.is_tensor(b) and a.dtype == b.dtype and a.shape == b.shape and \
            torch.equal(a.contiguous().view(-1).view(torch.uint8), b.contiguous().view(-1).view(torch.uint8))
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_load_obj_tsv_equals_the_reference_reader():
    g = np.load(os.path.join(GOLDEN, "obj_tsv.npz"))
    items = utils.load_obj_tsv(GOLDEN_TSV)
    assert len(items) == 6 and len(g.files) == 6 * len(utils.FIELDNAMES)
    assert sorted({(it["num_boxes"], it["features"].shape[1]) for it in items}) == list(C.SMALL)
    for i, it in enumerate(items):
        assert list(it.keys()) == utils.FIELDNAMES
        for k in utils.FIELDNAMES:
            want, got = g["%d/%s" % (i, k)], np.asarray(it[k])
            if want.dtype.kind in "fi" and want.ndim:
                assert got.dtype == want.dtype and got.shape == want.shape, (i, k)
                assert got.tobytes() == want.tobytes(), (i, k)  # bits: the features hold NaNs
                assert not it[k].flags.writeable
            else:
                assert type(it[k]) in (int, str) and str(it[k]) == str(want), (i, k)
    assert len(utils.load_obj_tsv(GOLDEN_TSV, topk=2)) == 2


def test_load_obj_tsv_skips_blank_lines_and_names_a_short_line(tmp_path):
    data = open(GOLDEN_TSV, "rb").read()
    lines = data.split(b"\n")
    p = tmp_path / "blank.tsv"
    p.write_bytes(b"\n" + lines[0] + b"\r\n\r\n" + lines[1])  # blank lines, \r\n, no final line end
    assert [it["img_id"] for it in utils.load_obj_tsv(str(p))] == [it["img_id"] for it in utils.load_obj_tsv(GOLDEN_TSV, topk=2)]
    q = tmp_path / "short.tsv"
    q.write_bytes(lines[0] + b"\n" + lines[1].rsplit(b"\t", 1)[0] + b"\n")
    with pytest.raises(ValueError, match=r"short\.tsv, line 2"):
        utils.load_obj_tsv(str(q))


@pytest.mark.parametrize("O,F", C.SHAPES[:5])
def test_write_then_load_round_trip_is_exact(tmp_path, O, F):
    recs = C.records(O, F, 3)
    path, _ = C.tsv_file(tmp_path, O, F, 3)
    back = utils.load_obj_tsv(path)
    assert len(back) == 3
    for a, b in zip(recs, back):
        for k in utils.FIELDNAMES:
            if isinstance(a[k], np.ndarray):
                assert b[k].dtype == a[k].dtype and b[k].shape == a[k].shape and b[k].tobytes() == a[k].tobytes(), k
            else:
                assert b[k] == a[k], k


# ---------------------------------------------------------------------------------- scan_chunk
def _check_spans(data, ch, lines):
    assert ch.n == len(lines)
    for i, line in enumerate(lines):
        fields = line.split(b"\t")
        for j, f in enumerate(tsv.KERNEL_FIELDS):
            off, ln = ch.desc[i, 2 * j], ch.desc[i, 2 * j + 1]
            assert data[off:off + ln] == fields[f], (i, j)
        assert ch.ids[i] == fields[0].decode() and ch.img_h[i] == int(fields[1]) and ch.img_w[i] == int(fields[2])
        assert ch.num_boxes[i] == int(fields[7]) and (ch.desc[i, 12], ch.desc[i, 13]) == (int(fields[2]), int(fields[1]))
        assert data[ch.lines[i, 0]:ch.lines[i, 0] + ch.lines[i, 1]] == line


def test_scan_chunk_slices_the_fields_split_gives(tmp_path):
    _, data = C.tsv_file(tmp_path, 5, 24, 40)  # img_ids of 1 .. 17 characters: field starts at every residue modulo 16
    lines = data.split(b"\n")[:-1]
    ch = tsv.scan_chunk(data, len(data))
    _check_spans(data, ch, lines)
    assert ch.tail == 0 and {int(o) % 16 for o in ch.desc[:, 10]} == set(range(16))
    # \r\n, blank lines, no final line end; bytes, bytearray and numpy buffers
    messy = b"\r\n" + b"\r\n\n".join(lines)
    for buf in (messy, bytearray(messy), np.frombuffer(messy, dtype=np.uint8)):
        _check_spans(messy, tsv.scan_chunk(buf, len(messy), final=True), lines)
    part = tsv.scan_chunk(messy, len(messy))  # not final: the unfinished last line is the tail
    _check_spans(messy, part, lines[:-1])
    assert part.tail == len(lines[-1])
    few = tsv.scan_chunk(data, len(data), max_lines=3)
    assert few.n == 3 and few.tail == len(data) - sum(len(l) + 1 for l in lines[:3])
    with pytest.raises(ValueError, match="tab-separated"):
        tsv.scan_chunk(lines[0] + b"\textra\n", len(lines[0]) + 7)
    with pytest.raises(ValueError, match="tab-separated"):
        tsv.scan_chunk(lines[0].rsplit(b"\t", 1)[0] + b"\n", len(lines[0].rsplit(b"\t", 1)[0]) + 1)


def _walk(data, size):
    """the lines a reader with chunks of ``size`` bytes meets, carrying the tail over -> list of line texts"""
    out, carry, pos = [], b"", 0
    while pos < len(data) or carry:
        buf = carry + data[pos:pos + size - len(carry)]
        pos += size - len(carry)
        final = pos >= len(data)
        ch = tsv.scan_chunk(buf, len(buf), final=final)
        if ch.n == 0 and not final:
            raise ValueError("chunk shorter than a line")
        out += [buf[s:s + n] for s, n in ch.lines]
        carry = buf[len(buf) - ch.tail:] if ch.tail else b""
        if final:
            break
    return out


def test_any_chunk_size_from_one_line_upward_yields_the_same_lines(tmp_path):
    _, data = C.tsv_file(tmp_path, 3, 8, 9)
    data = data[:-1]  # no final line end
    lines = data.split(b"\n")
    longest = max(len(l) for l in lines) + 1
    for size in list(range(longest, longest + 40)) + [2 * longest + 3, len(data), len(data) + 5]:
        assert _walk(data, size) == lines, size
    with pytest.raises(ValueError, match="shorter than a line"):
        _walk(data, longest - 2)


# ---------------------------------------------------------------------------------- the kernel's restatement
@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("feats_bf16", [True, False])
@pytest.mark.parametrize("O,F,n", [(1, 8, 20), (2, 8, 20), (3, 8, 20), (5, 24, 20), (36, 2048, 2), (100, 2048, 1), C.MAX_BOXES + (3,)])
def test_decode_host_equals_the_host_path(tmp_path, O, F, n, feats_bf16, normalize):
    if (O, F) == (100, 2048):
        pads = [tsv.b64_len(b) - (4 * b + 2) // 3 for b in tsv.field_bytes(O, F)]
        assert 1 in pads and 2 in pads  # '=' and '==' at this shape
    data, ch, got = C.host_decode(tmp_path, O, F, n, feats_bf16, normalize)
    recs = utils.load_obj_tsv(C.tsv_file(tmp_path, O, F, n)[0])
    want = C.expected(recs, feats_bf16, normalize)
    assert C.same_feats(got["feats"], want["feats"])
    for k in ("boxes", "obj_labels", "attr_labels", "obj_confs", "attr_confs"):
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k
    # no fault bit anywhere; bit 4 (informational) exactly where a feature is not finite
    nonfinite = np.array([not np.isfinite(r["features"]).all() for r in recs])
    assert np.array_equal(got["flags"], np.where(nonfinite, tsv.NONFINITE, 0).astype(np.uint32)) and got["counts"].tolist() == [0, 0]


def _bf16_reference(bits):
    return torch.from_numpy(bits.view(np.float32).copy()).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


def test_special_values_round_as_torch_does(tmp_path):
    data, ch, got = C.host_decode(tmp_path, 3, 8, 20)
    src = np.stack([r["features"] for r in C.records(3, 8, 20)]).view(np.uint32)
    assert set(C.SPECIAL_BITS.tolist()) <= set(src.reshape(-1).tolist())
    assert C.same_feats(got["feats"], _bf16_reference(src))
    one = lambda b: int(_bf16_reference(np.array([b], dtype=np.uint32))[0])
    assert (one(0x3F808000), one(0x3F818000), one(0x7F7FFFFF), one(0x80000000), one(0x00008000)) == (0x3F80, 0x3F82, 0x7F80, 0x8000, 0x0000)


def test_planted_faults_give_the_stated_bits(tmp_path):
    O, F, n = 3, 8, 4
    data, ch, clean = C.host_decode(tmp_path, O, F, n)
    recs = C.records(O, F, n)

    def run(line, field, text):
        bad = C.replace_field(data, ch, line, field, text)
        return tsv.tsv_decode_host(bad, tsv.scan_chunk(bad, len(bad)).desc, O, F)

    base = clean["flags"]
    for field in range(6):
        t = C.field_text(data, ch, 1, field)
        star = run(1, field, t[:5] + b"*" + t[6:])                      # outside the alphabet
        assert star["flags"][1] & 0xFFEF == tsv.BAD_CHAR | 1 << (8 + field), field
        inner = run(1, field, t[:2] + b"=" + t[3:])                     # '=' where no padding belongs
        assert inner["flags"][1] & 0xFFEF == tsv.BAD_CHAR | 1 << (8 + field), field
        short = run(1, field, t[:-4])                                   # a quad short
        assert short["flags"][1] & 0xFFEF == tsv.BAD_LEN | 1 << (8 + field), field
        spaced = run(1, field, t[:4] + b" " + t[4:])                    # a space inside: one character long
        assert spaced["flags"][1] & 0xFFEF == tsv.BAD_LEN | 1 << (8 + field), field
        for res in (star, inner, short, spaced):
            assert res["counts"].tolist() == [1, 0]
            for k in tsv.IMAGE_TABLES:  # the other lines are untouched
                assert np.array_equal(np.delete(res[k], 1, 0).view(np.uint8), np.delete(clean[k], 1, 0).view(np.uint8)), (field, k)
        key = tsv.IMAGE_TABLES[(2, 4, 3, 5, 1, 0)[field]]
        assert not short[key][1].view(np.uint8).any() and not spaced[key][1].view(np.uint8).any()  # zeros, all of the row
    # a missing pad character where bytes % 3 calls for one (objects_conf, 12 bytes: none; objects_id, 24: none; boxes, 48:
    # none; O = 1 has them) -- covered by the shapes above; here: a data character in a pad place
    d1, c1, _ = C.host_decode(tmp_path, 1, 8, 4)
    t = C.field_text(d1, c1, 0, 0)  # 8 bytes -> 12 characters, one '='
    assert t.endswith(b"=") and not t.endswith(b"==")
    bad = C.replace_field(d1, c1, 0, 0, t[:-1] + b"A")
    assert tsv.tsv_decode_host(bad, c1.desc, 1, 8)["flags"][0] & 0xFF0F == tsv.BAD_CHAR | 1 << 8
    # an id of 2^31, a box of 1.001
    ids = recs[2]["objects_id"].copy()
    ids[1] = 1 << 31
    res = run(2, 0, C.reencode(ids, np.int64))
    assert res["flags"][2] == base[2] | tsv.BAD_ID and res["obj_labels"][2, 1] == 0 and res["counts"].tolist() == [1, 0]
    assert np.array_equal(np.delete(res["obj_labels"][2], 1), np.delete(clean["obj_labels"][2], 1))
    boxes = recs[3]["boxes"].copy()
    boxes[2, 1] = np.float32(1.001) * recs[3]["img_h"]
    res = run(3, 4, C.reencode(boxes, np.float32))
    assert res["flags"][3] == base[3] | tsv.BAD_BOX and res["counts"].tolist() == [0, 1]
    boxes[2, 1] = np.nan
    assert run(3, 4, C.reencode(boxes, np.float32))["flags"][3] == base[3] | tsv.BAD_BOX  # a NaN fails the check


# ---------------------------------------------------------------------------------- the entry point's refusals
def _args(**kw):
    """a struct that passes every check (the device pointers are never read before the launch: any aligned address)"""
    from xggm_amd.ops import TsvDecodeArgs
    O, F, n = 2, 8, 2
    desc = np.zeros((n, 14), dtype=np.int64)
    desc[:, 1::2][:, :6] = 8
    desc[:, 12:] = (640, 480)
    a = TsvDecodeArgs()
    a.text, a.n_bytes, a.alloc_bytes, a.desc, a.host_desc = 0x10000, 1000, 1008, 0x20000, desc.ctypes.data
    a.n, a.O, a.F, a.feats_bf16, a.normalize, a.row0, a.capacity = n, O, F, 1, 1, 1, 4
    a.feats, a.boxes, a.obj_labels, a.attr_labels, a.obj_confs, a.attr_confs = 0x30000, 0x40000, 0x50000, 0x60000, 0x70000, 0x80000
    a.flags, a.counts = 0x90000, 0xA0000
    for k, v in kw.items():
        setattr(a, k, v)
    return a, desc


REFUSALS = [
    (dict(text=None), "null text"), (dict(desc=None), "null text"), (dict(host_desc=None), "null text"),
    (dict(feats=None, boxes=None, obj_labels=None, attr_labels=None, obj_confs=None, attr_confs=None, flags=None, counts=None), "every output"),
    (dict(n=0), "n=0"), (dict(O=0), "O=0"), (dict(O=129), "O=129"), (dict(F=0), "F=0"), (dict(F=12), "multiple of 8"),
    (dict(row0=-1), "capacity"), (dict(row0=3), "capacity"), (dict(capacity=2), "capacity"),
    (dict(text=0x10008), "16-byte aligned"), (dict(alloc_bytes=1004), "multiple of 16"), (dict(alloc_bytes=992), "multiple of 16"),
    (dict(feats=0x30008), "feats is not 16-byte aligned"), (dict(boxes=0x40002), "4 bytes"), (dict(attr_labels=0x60001), "4 bytes"),
    (dict(flags=0x90002), "4 bytes"),
]


def test_entry_point_refuses_before_any_launch():
    from xggm_amd import _lib
    L = _lib.lib
    assert L.xggm_tsv_decode(None, None) != 0 and "xggm_tsv_decode: null argument struct" in _lib.last_error()
    for kw, word in REFUSALS:
        a, desc = _args(**kw)
        assert L.xggm_tsv_decode(ctypes.addressof(a), None) != 0, kw
        assert "xggm_tsv_decode" in _lib.last_error() and word in _lib.last_error(), (kw, _lib.last_error())
    for (i, j, v), word in [((0, 0, -1), "negative"), ((1, 3, -8), "negative"), ((1, 10, 996), "ends past n_bytes"),
                            ((0, 11, 1001), "ends past n_bytes"), ((1, 12, 0), "img_w=0"), ((0, 13, 1 << 24), "outside [1, 2^24)")]:
        a, desc = _args()
        desc[i, j] = v
        assert L.xggm_tsv_decode(ctypes.addressof(a), None) != 0, (i, j, v)
        assert "xggm_tsv_decode" in _lib.last_error() and word in _lib.last_error(), (i, j, v, _lib.last_error())


def test_wrapper_and_reader_refuse_the_cpu(tmp_path):
    from xggm_amd import ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tsv.load_obj_tsv_device(GOLDEN_TSV, "cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.tsv_decode(torch.zeros(16, dtype=torch.uint8), 0, torch.zeros((1, 14), dtype=torch.int64), np.zeros((1, 14)), 1, 8, {}, 0)


# ---------------------------------------------------------------------------------- the stores adopt a table
def _examples(recs, with_arrays, feats_bf16):
    from xggm_amd.pretrain.lxmert_pretrain import InputExample
    from xggm_amd.tools.shards import normalize_boxes
    import pretrain_resident_cases as P
    rng = np.random.default_rng(5)
    w = P.words()
    img_of = list(range(len(recs))) + [0, 2, 2, 1, 0]  # first appearances in file order: both stores have one row order
    out = []
    for q, i in enumerate(img_of):
        r = recs[i]
        sent = " ".join(rng.choice(w, size=int(rng.integers(1, 9))))
        label = {int(k): float(np.float32(rng.random())) for k in rng.choice(29, size=q % 3, replace=False)} or None
        ex = InputExample("%s_vqa_%03d" % (r["img_id"], q), sent, None, None, None, 1, label)
        if with_arrays:
            ex.visual_feats = (r["features"], normalize_boxes(r["boxes"], r["img_w"], r["img_h"]))
            ex.obj_labels, ex.attr_labels = (r["objects_id"], r["objects_conf"]), (r["attrs_id"], r["attrs_conf"])
        if q % 2:
            ex.img_id = r["img_id"]  # optional: else the uid's head
        out.append(ex)
    return out


@pytest.mark.parametrize("feats_bf16", [True, False])
def test_pretrain_store_adopts_a_cpu_table(tmp_path, feats_bf16):
    from xggm_amd.pretrain.resident import ResidentPretrainSet, pretrain_tables
    import pretrain_resident_cases as P
    recs = utils.load_obj_tsv(C.tsv_file(tmp_path, 5, 24, 4)[0])
    for r in recs:  # the image id is the uid's head "<img_id>_<dset>_<idx>": no underscore of its own
        assert "_" not in r["img_id"]
    table = tsv.ObjTable.from_records(recs, "cpu", feats_bf16=feats_bf16)
    assert (table.n, table.N, table.F) == (4, 5, 24) and table.row_of[recs[2]["img_id"]] == 2
    tok, T, K = P.tok(), 12, 3
    tabs = pretrain_tables(_examples(recs, False, feats_bf16), tok, T, K, n_answers=29, images=table)
    mine = ResidentPretrainSet(tabs, "cpu")
    twin = ResidentPretrainSet(_examples(recs, True, feats_bf16), "cpu", tokenizer=tok, max_seq_length=T, max_labels=K, n_answers=29,
                               feats_bf16=feats_bf16)
    for k in tsv.IMAGE_TABLES:
        assert mine.tables[k].data_ptr() == getattr(table, k).data_ptr(), k  # adopted, not copied
    assert mine.nbytes == twin.nbytes and (mine.n_img, mine.n, mine.O, mine.F) == (twin.n_img, twin.n, twin.O, twin.F)
    with pytest.raises(ValueError, match="limit"):
        ResidentPretrainSet(tabs, "cpu", max_bytes=mine.nbytes - 1)
    idx = [8, 0, 3, 5, 7, 1]
    a, b = mine.host_batch(idx), twin.host_batch(idx)
    assert a.keys() == b.keys()
    for k in a:
        assert _same_bits(a[k], b[k]), k
    ex = _examples(recs, False, feats_bf16)
    ex[3].uid, ex[3].img_id = "nowhere_vqa_003", None
    with pytest.raises(ValueError, match="nowhere_vqa_003"):
        pretrain_tables(ex, tok, T, K, images=table)


def test_vqa_dataset_takes_a_cpu_table(tmp_path):
    from xggm_amd.lxrt.entry import SentenceBatcher
    from xggm_amd.tools.resident import ResidentDataset
    from xggm_amd.tools.shards import ShardReader, ShardWriter
    from xggm_amd.vqa.vqacpv2_data import VQADataset, VQATorchDataset
    import pretrain_resident_cases as P
    recs = utils.load_obj_tsv(C.tsv_file(tmp_path, 5, 24, 4)[0])
    rng = np.random.default_rng(3)
    adj = rng.random((4, 5, 5), dtype=np.float32)
    table = tsv.ObjTable.from_records(recs, "cpu").set_adjacency(torch.from_numpy(adj.copy()))
    w = ShardWriter(str(tmp_path / "twin.xgs"), n_objects=5, feat_dim=24)
    for r, a in zip(recs, adj):
        w.add(r["img_id"], r["features"], r["boxes"], r["img_w"], r["img_h"], a)
    words = P.words()
    data = [dict(question_id=100 + q, image_id=recs[i]["img_id"], question=" ".join(rng.choice(words, size=4)),
                 label=[q % 7], score=[0.5]) for q, i in enumerate([0, 3, 1, 1, 2, 0, 0])]
    data[-1]["image_id"] = "absent"  # dropped by both, as the reference drops it
    l2a = ["a%d" % i for i in range(7)]
    mk = lambda shard: VQATorchDataset(VQADataset("train", data=data, ans2label={a: i for i, a in enumerate(l2a)}, label2ans=l2a), shard=shard)
    ts, ts_twin = mk(table), mk(ShardReader(w.close()))
    assert len(ts) == len(ts_twin) == 6 and ts.rows.tolist() == ts_twin.rows.tolist()
    for x, y in zip(ts[2], ts_twin[2]):  # one row read back, for inspection
        assert _same_bits(x, y)
    with pytest.raises(RuntimeError, match="ResidentDataset"):
        ts.collate([0, 1], ts_twin.alloc(2, False))
    batcher = SentenceBatcher(P.tok(), 10)
    mine, twin = ResidentDataset(ts, batcher, "cpu"), ResidentDataset(ts_twin, batcher, "cpu")
    for k in ("feats", "boxes", "adj"):
        assert mine.tables[k].data_ptr() == getattr(table, k).data_ptr(), k
    assert mine.nbytes == twin.nbytes
    a, b = mine.host_batch([5, 0, 2, 3]), twin.host_batch([5, 0, 2, 3])
    assert a.keys() == b.keys()
    for k in a:
        assert _same_bits(a[k], b[k]), k
