"""Shared cases of the feature-file tests (tests/test_tsv_ingest_cpu.py, tests/test_tsv_ingest_gpu.py): seeded records at
every (O, F) the kernel has a path for, with the values whose handling the contract spells out, the files written from
them, and the host results they are compared with -- computed once per case and shared (left unchanged by the tests)."""
import os

import numpy as np

from xggm_amd.tools import tsv
from xggm_amd.tools.shards import _bf16_bits, normalize_boxes

SEED = 20240923
# (O, F): bytes % 3 of the six fields takes 0, 1 and 2 over (1, 8), (2, 8), (3, 8); (5, 24) has a partial last unit of 64
# bytes, (36, 2048) is the published shape (3072 whole units, 12 slabs), (100, 2048) ends in a unit of 32 bytes and needs
# '=' and '==' padding
SHAPES = ((1, 8), (2, 8), (3, 8), (5, 24), (36, 2048), (100, 2048))
SMALL = SHAPES[:3]
# the largest box count the contract allows: the small fields fill their LDS regions to the last byte (ids 1024 bytes from
# 342 quads, confidences 512 from 171: the last quad of each decodes to fewer than three bytes)
MAX_BOXES = (128, 8)
# fp32 bit patterns every case carries in its first features: +-0, denormals, +-inf, NaNs, the bf16 ties 0x3F808000 (to
# even: down) and 0x3F818000 (to even: up), the largest finite value (rounds to inf), the largest bf16
SPECIAL_BITS = np.array([0x00000000, 0x80000000, 0x00000001, 0x807FFFFF, 0x00008000, 0x7F800000, 0xFF800000, 0x7FC00000,
                         0x7F800001, 0xFFFFFFFF, 0x3F808000, 0x3F818000, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F0000, 0x3F80FFFF,
                         0x00018000, 0x3F807FFF], dtype=np.uint32)
_cache = {}


def img_id_of(i):
    """img_ids of 1 .. 17 characters in rotation: field starts meet every residue modulo 16"""
    n = i % 17 + 1
    return ("%d" % (i + 1)).rjust(n, "7") if n < 13 else "COCO_%s" % ("%d" % (i + 1)).rjust(n - 5, "0")


def records(O, F, n, seed=SEED, plain_ids=False):
    """``n`` seeded records of shape (O, F): valid boxes, ids at +-2^31 -+ 1 (``plain_ids``: all inside the detector's 1600
    classes and 400 attributes, for an adjacency) and the special features (``plain_ids``: finite ones only)"""
    key = ("rec", O, F, n, seed, plain_ids)
    if key not in _cache:
        rng = np.random.default_rng([seed, O, F, n])
        out = []
        for i in range(n):
            w, h = int(rng.integers(200, 1200)), int(rng.integers(200, 1200))
            feats = (rng.standard_normal((O, F)) * np.exp(rng.uniform(-3, 3, (O, 1)))).astype(np.float32)
            flat = feats.reshape(-1).view(np.uint32)
            k = min(flat.size, SPECIAL_BITS.size)
            flat[:k] = np.roll(SPECIAL_BITS, i)[:k]
            if flat.size > 64:
                flat[-k:] = np.roll(SPECIAL_BITS, -i)[:k]  # in the last unit as well
            boxes = rng.random((O, 4), dtype=np.float32) * np.array([w, h, w, h], dtype=np.float32)
            boxes[0] = (0.0, 0.0, w, h)  # the edges of the range check
            oid, aid = rng.integers(0, 1600, O), rng.integers(0, 400, O)
            if plain_ids:
                feats = np.where(np.isfinite(feats), feats, np.float32(1.5))
            else:
                oid[i % O], aid[(i + 1) % O] = (1 << 31) - 1, -(1 << 31)
            out.append(dict(img_id=img_id_of(i), img_h=h, img_w=w, objects_id=oid.astype(np.int64),
                            objects_conf=rng.random(O, dtype=np.float32), attrs_id=aid.astype(np.int64),
                            attrs_conf=rng.random(O, dtype=np.float32), num_boxes=O, boxes=boxes, features=feats))
        _cache[key] = out
    return _cache[key]


def tsv_file(tmp_dir, O, F, n, seed=SEED, plain_ids=False):
    """the records as a file (written once) -> (path, its bytes)"""
    key = ("file", O, F, n, seed, plain_ids)
    if key not in _cache:
        path = os.path.join(str(tmp_dir), "obj_%d_%d_%d_%d_%d.tsv" % (O, F, n, seed, plain_ids))
        tsv.write_obj_tsv(path, records(O, F, n, seed, plain_ids))
        with open(path, "rb") as f:
            _cache[key] = (path, f.read())
    return _cache[key]


def expected(recs, feats_bf16=True, normalize=True):
    """the six tables of ``recs`` by the host path: ``load_obj_tsv``-style arrays + ``shards.normalize_boxes`` +
    ``shards._bf16_bits``"""
    feats = np.stack([r["features"] for r in recs])
    return dict(feats=_bf16_bits(feats) if feats_bf16 else feats,
                boxes=np.stack([normalize_boxes(r["boxes"], r["img_w"], r["img_h"]) if normalize else np.array(r["boxes"]) for r in recs]),
                obj_labels=np.stack([r["objects_id"] for r in recs]).astype(np.int32),
                attr_labels=np.stack([r["attrs_id"] for r in recs]).astype(np.int32),
                obj_confs=np.stack([r["objects_conf"] for r in recs]), attr_confs=np.stack([r["attrs_conf"] for r in recs]))


def host_decode(tmp_dir, O, F, n, feats_bf16=True, normalize=True):
    """``tsv_decode_host`` of the case's file (once per case) -> (bytes, Chunk, its result)"""
    key = ("host", O, F, n, feats_bf16, normalize)
    if key not in _cache:
        _, data = tsv_file(tmp_dir, O, F, n)
        ch = tsv.scan_chunk(data, len(data))
        _cache[key] = (data, ch, tsv.tsv_decode_host(data, ch.desc, O, F, feats_bf16=feats_bf16, normalize=normalize))
    return _cache[key]


def same_feats(got, want):
    """bit equality of two feature arrays (uint16 bf16 bits or float32) except at NaN positions, which must be NaN in both"""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    if want.dtype == np.uint16:
        nan_g, nan_w = (got & 0x7FFF) > 0x7F80, (want & 0x7FFF) > 0x7F80
    else:
        nan_g, nan_w = np.isnan(got), np.isnan(want)
        got, want = got.view(np.uint32), want.view(np.uint32)
    return bool(np.array_equal(nan_g, nan_w) and np.array_equal(got[~nan_w], want[~nan_w]))


def replace_field(data, ch, line, field, new_text):
    """``data`` with the text of kernel field ``field`` of line ``line`` replaced -> bytes"""
    off, ln = int(ch.desc[line, 2 * field]), int(ch.desc[line, 2 * field + 1])
    return data[:off] + new_text + data[off + ln:]


def field_text(data, ch, line, field):
    off, ln = int(ch.desc[line, 2 * field]), int(ch.desc[line, 2 * field + 1])
    return data[off:off + ln]


def reencode(arr, dtype):
    import base64
    return base64.b64encode(np.ascontiguousarray(arr, dtype=dtype).tobytes())

