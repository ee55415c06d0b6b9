"""Feature files: bottom-up TSVs decoded on the device, straight into the tables of the resident stores.

The features of this model family ship as TSV files (``train2014_obj36.tsv``, ``vg_gqa_obj36.tsv`` ...): one line per image,
ten tab-separated fields (``utils.FIELDNAMES``), six of them base64 text -- 393 216 characters of it per 36 x 2048 image.
The host reader (``utils.load_obj_tsv``, the reference's) decodes them in Python, and a store then stacks, rounds and
uploads the arrays: a second full copy of the file in host memory before the first byte crosses the link.
``load_obj_tsv_device`` instead moves the TEXT: ``readinto`` a pinned buffer, ``scan_chunk`` finds the fields (memchr only),
one copy carries text and descriptors over, and ONE launch per chunk (``ops.tsv_decode``, contract: xggm_tsv_decode in
include/xggm.h) decodes, converts and writes the table rows.  The result, an ``ObjTable``, is what the stores adopt without
a copy: ``pretrain.resident.pretrain_tables(..., images=table)``, ``VQATorchDataset(dataset, shard=table)``.

``tsv_decode_host`` restates the kernel in numpy, flags included -- the reference it is tested against on the CPU, NOT a
fallback: ``load_obj_tsv_device`` refuses a device without the kernel."""
import base64
import ctypes
import os

import numpy as np
import torch

from ..utils import DECODE_CONFIG, FIELDNAMES
from .shards import _bf16_bits, normalize_boxes

# xggm_tsv_decode's fields in its order, as indices into a line's ten fields, and its descriptor width
KERNEL_FIELDS = tuple(FIELDNAMES.index(k) for k, _, _ in DECODE_CONFIG)
N_DESC = 2 * len(KERNEL_FIELDS) + 2
BAD_CHAR, BAD_LEN, BAD_ID, BAD_BOX, NONFINITE = 1, 2, 4, 8, 16
HOST_BITS = BAD_CHAR | BAD_LEN | BAD_ID  # lines the host path redoes
IMAGE_TABLES = ("feats", "boxes", "obj_labels", "attr_labels", "obj_confs", "attr_confs")


def field_bytes(O, F):
    """bytes each of the kernel's six fields decodes to"""
    return (8 * O, 4 * O, 8 * O, 4 * O, 16 * O, 4 * O * F)


def b64_len(nbytes):
    return 4 * ((nbytes + 2) // 3)


# ---------------------------------------------------------------------------------- writing (tests, the benchmark)
def write_obj_tsv(path, records):
    """the inverse of ``utils.load_obj_tsv``: ``records`` (dicts under ``utils.FIELDNAMES``) -> a TSV file, one ``\\n``-ended
    line each"""
    with open(path, "wb") as f:
        for r in records:
            cols = []
            for k in FIELDNAMES:
                dt = {name: d for name, _, d in DECODE_CONFIG}.get(k)
                cols.append(str(r[k]).encode("utf-8") if dt is None else base64.b64encode(np.ascontiguousarray(r[k], dtype=dt).tobytes()))
            f.write(b"\t".join(cols) + b"\n")
    return path


# ---------------------------------------------------------------------------------- scanning
_memchr = ctypes.CDLL(None).memchr
_memchr.restype, _memchr.argtypes = ctypes.c_void_p, (ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t)


class Chunk:
    """what ``scan_chunk`` found: ``desc`` int64 [n, 14] (six (offset, length) pairs in the kernel's order, img_w, img_h),
    ``ids`` (img_id strings), ``img_h`` / ``img_w`` / ``num_boxes`` int64 [n], ``lines`` int64 [n, 2] ((start, length) of
    every kept line without its line end) and ``tail``: the bytes of the unfinished last line, to carry over"""

    def __init__(self, desc, ids, img_h, img_w, num_boxes, lines, tail):
        self.desc, self.ids, self.img_h, self.img_w, self.num_boxes, self.lines, self.tail = desc, ids, img_h, img_w, num_boxes, lines, tail
        self.n = len(ids)


def scan_chunk(buf, n_valid, final=False, max_lines=None, where="<buffer>"):
    """the descriptors of every whole line in ``buf[:n_valid]`` (``bytes``, ``bytearray`` or a C-contiguous uint8 numpy
    array, e.g. the view of a pinned staging buffer) -> ``Chunk``.  Tabs and line ends are located with memchr only: eleven
    calls per line, no per-byte Python.  Lines end with ``\\n`` or ``\\r\\n``; blank lines are skipped; ``final``: the buffer
    ends the file, so a last line without a line end counts.  ``max_lines``: stop after that many (the rest is ``tail``).
    A line without ten fields raises ValueError naming ``where`` and the line's offset."""
    if isinstance(buf, np.ndarray):
        if buf.dtype != np.uint8 or not buf.flags.c_contiguous:
            raise TypeError("scan_chunk: a numpy buffer must be C-contiguous uint8")
        keep, base = buf, buf.ctypes.data
    else:
        keep = np.frombuffer(buf, dtype=np.uint8)
        base = keep.ctypes.data
    mv = memoryview(keep)
    n_valid = int(n_valid)
    if not 0 <= n_valid <= keep.shape[0]:
        raise ValueError("scan_chunk: n_valid=%d outside the buffer's %d bytes" % (n_valid, keep.shape[0]))

    def find(c, lo, hi):
        p = _memchr(base + lo, c, hi - lo) if hi > lo else None
        return -1 if p is None else p - base

    desc, ids, hs, ws, nbs, lines = [], [], [], [], [], []
    pos = 0
    while pos < n_valid and (max_lines is None or len(ids) < max_lines):
        nl = find(10, pos, n_valid)
        if nl < 0:
            if not final:
                break
            nl = n_valid
        end = nl - 1 if nl > pos and keep[nl - 1] == 13 else nl
        start, pos = pos, min(nl + 1, n_valid)
        if end == start:
            continue
        cuts, p = [start - 1], start
        for _ in range(len(FIELDNAMES) - 1):
            t = find(9, p, end)
            if t < 0:
                break
            cuts.append(t)
            p = t + 1
        if len(cuts) != len(FIELDNAMES) or find(9, p, end) >= 0:
            raise ValueError("%s, line at byte %d: not %d tab-separated fields" % (where, start, len(FIELDNAMES)))
        cuts.append(end)
        span = lambda k: (cuts[k] + 1, cuts[k + 1] - cuts[k] - 1)
        text = lambda k: bytes(mv[cuts[k] + 1:cuts[k + 1]])
        try:
            h, w, nb = int(text(1)), int(text(2)), int(text(7))
        except ValueError:
            raise ValueError("%s, line at byte %d (img_id %r): img_h, img_w, num_boxes must be integers"
                             % (where, start, text(0))) from None
        row = []
        for k in KERNEL_FIELDS:
            row.extend(span(k))
        desc.append(row + [w, h])
        ids.append(text(0).decode("utf-8"))
        hs.append(h), ws.append(w), nbs.append(nb), lines.append((start, end - start))
    i64 = lambda v, shape: np.asarray(v, dtype=np.int64).reshape(shape)
    return Chunk(i64(desc, (-1, N_DESC)), ids, i64(hs, (-1,)), i64(ws, (-1,)), i64(nbs, (-1,)), i64(lines, (-1, 2)), n_valid - pos)


# ---------------------------------------------------------------------------------- the kernel in numpy
def _alphabet():
    t = np.full(256, 0x80, dtype=np.uint8)
    for i, c in enumerate(b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/"):
        t[c] = i
    t[ord("=")] = 0x40
    return t


_TAB = _alphabet()


def _decode_field(text, nbytes):
    """one field as xggm_tsv_decode decodes it -> (uint8 [nbytes], flag bits 0-1): a field of the wrong length is all
    zeros, a character that does not belong where it stands six zero bits"""
    quads = (nbytes + 2) // 3
    if len(text) != 4 * quads:
        return np.zeros(nbytes, dtype=np.uint8), BAD_LEN
    t = _TAB[np.frombuffer(text, dtype=np.uint8)].reshape(quads, 4)
    want = np.zeros((quads, 4), dtype=np.uint8)  # bits 6-7 every place must show: '=' in the last pad places, else none
    pad = 3 * quads - nbytes
    if pad:
        want[-1, 4 - pad:] = 0x40
    bad = bool(((t & 0xC0) != want).any())
    s = (t & 63).astype(np.uint32)
    v = s[:, 0] << 18 | s[:, 1] << 12 | s[:, 2] << 6 | s[:, 3]
    out = np.stack([v >> 16, v >> 8, v], axis=1).astype(np.uint8).reshape(-1)[:nbytes]
    return out, BAD_CHAR if bad else 0


def tsv_decode_host(buf, desc, O, F, feats_bf16=True, normalize=True):
    """xggm_tsv_decode restated in numpy: the lines ``desc`` (int64 [n, 14], as ``scan_chunk`` returns them) of the text
    ``buf`` -> dict of numpy arrays feats [n, O, F] (uint16 bf16 bit patterns, or float32), boxes, obj_labels, attr_labels,
    obj_confs, attr_confs, flags uint32 [n] and counts int32 [2].  The CPU-testable reference of the kernel; no fallback."""
    mv = memoryview(np.frombuffer(buf, dtype=np.uint8) if not isinstance(buf, np.ndarray) else buf)
    desc = np.asarray(desc, dtype=np.int64).reshape(-1, N_DESC)
    n, O, F = desc.shape[0], int(O), int(F)
    out = dict(feats=np.zeros((n, O, F), dtype=np.uint16 if feats_bf16 else np.float32), boxes=np.zeros((n, O, 4), dtype=np.float32),
               obj_labels=np.zeros((n, O), dtype=np.int32), attr_labels=np.zeros((n, O), dtype=np.int32),
               obj_confs=np.zeros((n, O), dtype=np.float32), attr_confs=np.zeros((n, O), dtype=np.float32),
               flags=np.zeros(n, dtype=np.uint32), counts=np.zeros(2, dtype=np.int32))
    for i in range(n):
        flag, raw, dead = 0, [], []
        for f, nb in enumerate(field_bytes(O, F)):
            off, ln = int(desc[i, 2 * f]), int(desc[i, 2 * f + 1])
            b, bits = _decode_field(bytes(mv[off:off + ln]), nb)
            if bits:
                flag |= bits | 1 << (8 + f)
            raw.append(b), dead.append(bits == BAD_LEN)
        for key, f in (("obj_labels", 0), ("attr_labels", 2)):
            v = raw[f].view("<i8")
            fits = (v >= -(1 << 31)) & (v < (1 << 31))
            if not fits.all():
                flag |= BAD_ID
            out[key][i] = np.where(fits, v, 0).astype(np.int32)
        out["obj_confs"][i], out["attr_confs"][i] = raw[1].view("<f4"), raw[3].view("<f4")
        b = raw[4].view("<f4").reshape(O, 4).copy()
        if normalize:
            with np.errstate(all="ignore"):
                b[:, (0, 2)] /= np.float32(desc[i, N_DESC - 2])
                b[:, (1, 3)] /= np.float32(desc[i, N_DESC - 1])
            bd = b.astype(np.float64)
            if not dead[4] and not ((bd < 1 + 1e-5) & (-bd < 1e-5)).all():  # a NaN fails
                flag |= BAD_BOX
        out["boxes"][i] = b
        feats = raw[5].view("<f4").reshape(O, F)
        if not np.isfinite(feats).all():
            flag |= NONFINITE
        out["feats"][i] = _bf16_bits(feats) if feats_bf16 else feats
        out["flags"][i] = flag
        out["counts"][0] += bool(flag & HOST_BITS)
        out["counts"][1] += bool(flag & BAD_BOX)
    return out


# ---------------------------------------------------------------------------------- the table
def _torch_feats(bits_or_f32):
    a = np.ascontiguousarray(bits_or_f32)
    return torch.from_numpy(a.view(np.int16).copy()).view(torch.bfloat16) if a.dtype == np.uint16 else torch.from_numpy(a.copy())


class ObjTable:
    """the images of one feature file as the stores' tables.  Device tensors ``feats`` [n, N, F] (bf16 or fp32), ``boxes``
    [n, N, 4], ``obj_labels`` / ``attr_labels`` [n, N] int32, ``obj_confs`` / ``attr_confs`` [n, N] fp32, ``flags`` int32 [n]
    (the bit patterns of xggm_tsv_decode's flags, or None) and, after ``set_adjacency``, ``adj`` [n, N, N] fp32 -- or, after
    ``set_label_adjacency``, ``pair_table`` [Vc, Va] fp32 and no ``adj`` at all.  Host:
    ``ids`` (the img_id strings in row order), ``row_of``, ``img_h`` / ``img_w`` int64 [n], ``n``, ``N``, ``F``.  In place of a
    ``ShardReader`` it answers ``len``, ``row_of``, ``N``, ``F``, ``adj``, ``feats_f32(row)`` and ``boxes_of(row)``."""

    def __init__(self, tensors, ids, img_h, img_w, flags=None, normalized=True):
        for k in IMAGE_TABLES:
            setattr(self, k, tensors[k])
        self.n, self.N, self.F = (int(v) for v in self.feats.shape)
        self.ids = list(ids)
        self.row_of = {i: r for r, i in enumerate(self.ids)}
        self.img_h, self.img_w = np.asarray(img_h, dtype=np.int64), np.asarray(img_w, dtype=np.int64)
        self.flags, self.adj, self.normalized, self.last_host_rows = flags, None, bool(normalized), 0
        self.pair_table = None  # set_label_adjacency: the adjacency is made from the labels, no [n, N, N] table
        self.device = self.feats.device
        want = dict(feats=(self.n, self.N, self.F), boxes=(self.n, self.N, 4), obj_labels=(self.n, self.N), attr_labels=(self.n, self.N),
                    obj_confs=(self.n, self.N), attr_confs=(self.n, self.N))
        for k, shape in want.items():
            t = getattr(self, k)
            if tuple(t.shape) != shape or t.device != self.device or not t.is_contiguous():
                raise ValueError("ObjTable: %s is %s on %s, contiguous %s on %s expected" % (k, tuple(t.shape), t.device, shape, self.device))
        if len(self.ids) != self.n or self.img_h.shape != (self.n,) or self.img_w.shape != (self.n,):
            raise ValueError("ObjTable: %d ids, img_h %s, img_w %s for %d rows" % (len(self.ids), self.img_h.shape, self.img_w.shape, self.n))

    def __len__(self):
        return self.n

    def tables(self):
        """the six image tables under the names of ``pretrain.resident.IMAGE_TABLES``"""
        return {k: getattr(self, k) for k in IMAGE_TABLES}

    @property
    def nbytes(self):
        extra = [t for t in (self.adj, self.pair_table) if t is not None]  # one of the two at most
        return sum(int(t.numel() * t.element_size()) for t in list(self.tables().values()) + extra)

    def set_adjacency(self, adj):
        """``adj`` [n, N, N] fp32 on the table's device (``preprocess.build_adjacency(class_table, attr_table,
        table.obj_labels, table.attr_labels)``), the ``adj_true`` table of ``ResidentDataset``"""
        if tuple(adj.shape) != (self.n, self.N, self.N) or adj.dtype != torch.float32 or adj.device != self.device:
            raise ValueError("ObjTable.set_adjacency: %s %s on %s, (%d, %d, %d) float32 on %s expected"
                             % (tuple(adj.shape), adj.dtype, adj.device, self.n, self.N, self.N, self.device))
        if self.pair_table is not None:
            raise ValueError("ObjTable.set_adjacency: the table makes its adjacency from labels (set_label_adjacency); one source only")
        self.adj = adj.contiguous()
        return self

    def set_label_adjacency(self, pair_table):
        """``pair_table`` [Vc, Va] fp32 on the table's device (``preprocess.compute_adjacency.label_pair_table``): ``adj``
        stays None -- no [n, N, N] table exists -- and a ``ResidentDataset`` makes ``adj_true`` from ``obj_labels`` /
        ``attr_labels`` inside the batch gather, bit-equal to the rows ``build_adjacency`` would have stored.  The ids are
        range-checked here, once (one device min/max, one read-back): ValueError naming the range."""
        from ..preprocess.compute_adjacency import check_label_range
        if pair_table.dim() != 2 or pair_table.dtype != torch.float32 or pair_table.device != self.device:
            raise ValueError("ObjTable.set_label_adjacency: %s %s on %s, [Vc, Va] float32 on %s expected"
                             % (tuple(pair_table.shape), pair_table.dtype, pair_table.device, self.device))
        if self.adj is not None:
            raise ValueError("ObjTable.set_label_adjacency: the table holds a materialised adjacency (set_adjacency); one source only")
        if not 1 <= self.N <= 128:
            raise ValueError("ObjTable.set_label_adjacency: %d objects, the label adjacency serves 1 .. 128" % self.N)
        check_label_range(pair_table, self.obj_labels, self.attr_labels, "ObjTable.set_label_adjacency")
        self.pair_table = pair_table.contiguous()
        return self

    def adj_of(self, row):
        """adjacency of one image, fp32 numpy [N, N], read back: the stored row, or the one the gather would make"""
        if self.adj is not None:
            return self.adj[row].cpu().numpy()
        if self.pair_table is None:
            raise ValueError("ObjTable: the table holds no adjacency (set_adjacency / set_label_adjacency)")
        from ..preprocess.compute_adjacency import build_adjacency_from_labels
        return build_adjacency_from_labels(self.pair_table, self.obj_labels[row:row + 1], self.attr_labels[row:row + 1], check=False)[0].cpu().numpy()

    def feats_f32(self, row):
        """features of one image as fp32 numpy (the stored values), read back: for inspection"""
        return self.feats[row].to(torch.float32).cpu().numpy()

    def boxes_of(self, row):
        return self.boxes[row].cpu().numpy()

    @classmethod
    def from_records(cls, records, device, feats_bf16=True, normalize=True):
        """the table of ``utils.load_obj_tsv`` output, built on the HOST and moved to ``device`` (``"cpu"`` too: the store
        plumbing without a GPU).  Boxes are normalised and range-checked as ``shards.normalize_boxes`` does."""
        if not records:
            raise ValueError("ObjTable.from_records: no records")
        O, F = records[0]["features"].shape
        for r in records:
            if r["features"].shape != (O, F) or r["num_boxes"] != O:
                raise ValueError("ObjTable.from_records: image %r has %d boxes / features %s, the first image has %d x %d"
                                 % (r["img_id"], r["num_boxes"], r["features"].shape, O, F))
            for k in ("objects_id", "attrs_id"):
                if r[k].size and (r[k].min() < -(1 << 31) or r[k].max() >= (1 << 31)):
                    raise ValueError("ObjTable.from_records: image %r has a value of %s outside int32" % (r["img_id"], k))
        feats = np.stack([r["features"] for r in records])
        boxes = np.stack([normalize_boxes(r["boxes"], r["img_w"], r["img_h"]) if normalize else np.array(r["boxes"]) for r in records])
        t = dict(feats=_torch_feats(_bf16_bits(feats) if feats_bf16 else feats), boxes=torch.from_numpy(boxes),
                 obj_labels=torch.from_numpy(np.stack([r["objects_id"] for r in records]).astype(np.int32)),
                 attr_labels=torch.from_numpy(np.stack([r["attrs_id"] for r in records]).astype(np.int32)),
                 obj_confs=torch.from_numpy(np.stack([r["objects_conf"] for r in records])),
                 attr_confs=torch.from_numpy(np.stack([r["attrs_conf"] for r in records])))
        return cls({k: v.to(device) for k, v in t.items()}, [str(r["img_id"]) for r in records], [r["img_h"] for r in records],
                   [r["img_w"] for r in records], normalized=normalize)


# ---------------------------------------------------------------------------------- the device reader
def _host_row(fields, O, F, where):
    """one line by the host path -> the six arrays in the kernel's order; ValueError naming ``where`` and the field when
    the host path fails as well"""
    out = []
    for f, (key, shape, dt) in zip(KERNEL_FIELDS, DECODE_CONFIG):
        try:
            raw = base64.b64decode(fields[f])
        except ValueError as e:
            raise ValueError("%s, field %s: %s" % (where, key, e)) from None
        want = field_bytes(O, F)[len(out)]
        if len(raw) != want:
            raise ValueError("%s, field %s: %d bytes after b64decode, %d expected" % (where, key, len(raw), want))
        a = np.frombuffer(raw, dtype=dt)
        if dt == np.int64:
            if a.min() < -(1 << 31) or a.max() >= (1 << 31):
                raise ValueError("%s, field %s: an id outside int32" % (where, key))
            a = a.astype(np.int32)
        out.append(a)
    return out


def load_obj_tsv_device(fname, device, topk=None, feats_bf16=True, normalize=True, check_boxes=True, chunk_bytes=64 << 20,
                        max_bytes=None):
    """a bottom-up feature TSV -> ``ObjTable`` on ``device``, decoded there.  ``f.readinto`` fills one of two pinned staging
    buffers, ``scan_chunk`` finds the fields, one asynchronous copy moves text and descriptors, one ``ops.tsv_decode`` launch
    writes the rows; a stage is rewritten only after its copy's event, so reading chunk k + 1 overlaps the copy and decode
    of chunk k.  The stages hold ``min(chunk_bytes, file size)`` of text with the chunk's descriptors right behind it, and
    only that much is copied.  O and F come from the first line; a later line with another ``num_boxes`` raises ValueError naming its
    img_id.  The tables are allocated once, at an upper bound of the row count (the file's size over the fixed part of a
    line, or ``topk``), and narrowed to n without a copy.  ``max_bytes``: refuse (ValueError naming the total) tables beyond
    it, default: the device's free memory minus 2 GiB.  After the last chunk ONE read-back of two counters; only when they
    are non-zero one of the flags: lines with bits 0-2 are redone by the host path and patched in with one small upload
    each (``table.last_host_rows``), a ValueError names file, line, img_id and field when that fails too (and when lines cut
    short outnumber the rows the file's size allows for); a box outside
    the range check raises ValueError naming the first img_id when ``check_boxes``, else stays readable in
    ``table.flags`` (bit 3).  ``feats_bf16``: bf16 features (torch's rounding), else the file's fp32."""
    from .. import ops
    who = "load_obj_tsv_device"
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("%s: device %s -- the decoder is a HIP kernel, there is no CPU fallback (utils.load_obj_tsv is the host path)" % (who, device))
    topk = None if topk is None or topk < 0 else int(topk)
    size = os.path.getsize(fname)
    with open(fname, "rb") as g:
        first = b""
        while not first.rstrip(b"\r\n"):  # geometry from the first line that is not blank
            first = g.readline()
            if not first:
                raise ValueError("%s: %s holds no line" % (who, fname))
    with open(fname, "rb", buffering=0) as f:
        head = scan_chunk(first, len(first), final=True, where=fname)
        O = int(head.num_boxes[0])
        ftext = first[int(head.desc[0, 10]):int(head.desc[0, 10] + head.desc[0, 11])]
        fbytes = len(ftext) // 4 * 3 - (len(ftext) - len(ftext.rstrip(b"=")))
        F = fbytes // (4 * O) if O >= 1 else 0
        if not 1 <= O <= 128 or F < 8 or F % 8 or fbytes != 4 * O * F:
            raise ValueError("%s: %s, first line (img_id %r): num_boxes %d, %d feature characters -- 1 .. 128 boxes of a multiple of 8 "
                             "features expected" % (who, fname, head.ids[0], O, int(head.desc[0, 11])))
        fixed = sum(b64_len(b) for b in field_bytes(O, F)) + len(FIELDNAMES)  # six fields, nine tabs, one line end
        need = fixed + 64
        if chunk_bytes < max(need, len(first)):
            raise ValueError("%s: chunk_bytes=%d is shorter than a line of %s; at least %d are needed"
                             % (who, chunk_bytes, fname, max(need, len(first))))
        cap = size // (fixed + 4) + 1  # the four small fields hold a character each at least
        if topk is not None:
            cap = min(cap, max(topk, 1))
        fdt = torch.bfloat16 if feats_bf16 else torch.float32
        total = cap * (O * F * (2 if feats_bf16 else 4) + O * (16 + 4 * 4) + 4)
        if max_bytes is None:
            max_bytes = torch.cuda.mem_get_info(device)[0] - (2 << 30)
        if total > max_bytes:
            raise ValueError("%s: the tables of %s need %d bytes on the device, the limit is %d" % (who, fname, total, max_bytes))
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=device)
        tb = dict(feats=z((cap, O, F), fdt), boxes=z((cap, O, 4), torch.float32), obj_labels=z((cap, O), torch.int32),
                  attr_labels=z((cap, O), torch.int32), obj_confs=z((cap, O), torch.float32), attr_confs=z((cap, O), torch.float32))
        flags, counts = z((cap,), torch.int32), z((2,), torch.int32)

        # a stage: [text, up to text_cap bytes | descriptors of its lines, right behind the text rounded up to 16], sized to the
        # file when that is the smaller; one device twin for both stages (copy k + 1 follows decode k on the stream)
        limit = min(int(chunk_bytes), max(size, 16))  # text bytes per chunk
        text_cap = (limit + 15) // 16 * 16
        max_lines = text_cap // (fixed + 4) + 1  # more (shorter, faulty) lines than this wait for the next chunk
        stage_bytes = text_cap + max_lines * N_DESC * 8
        stages = [torch.empty(stage_bytes, dtype=torch.uint8).pin_memory() for _ in range(1 if size <= limit else 2)]
        views = [s.numpy() for s in stages]
        events = [None] * len(stages)
        dev_stage = torch.empty(stage_bytes, dtype=torch.uint8, device=device)
        want_len = np.array([b64_len(b) for b in field_bytes(O, F)], dtype=np.int64)
        short = None  # the first line with a field of the wrong length: what an overflow of the row bound is blamed on
        stream = torch.cuda.current_stream(device)

        ids, hs, ws, where_lines = [], [], [], []  # where_lines: (file offset, length) of every row's line
        n, k, carry, file_pos, eof = 0, 0, 0, 0, False
        with torch.cuda.device(device):
            while not eof and (topk is None or n < topk):
                st = k % len(stages)
                cur = views[st]
                if events[st] is not None:
                    events[st].synchronize()  # the copy out of this stage has finished
                if carry:
                    prev = views[(k - 1) % len(stages)]
                    cur[:carry] = prev[prev_valid - carry:prev_valid]  # (numpy copies overlapping ranges correctly)
                got = carry
                while got < limit:
                    r = f.readinto(memoryview(cur)[got:limit])
                    if not r:
                        eof = True
                        break
                    got += r
                ch = scan_chunk(cur, got, final=eof, max_lines=max_lines if topk is None else min(max_lines, topk - n), where=fname)
                if ch.tail and eof:  # lines left over by max_lines: not the end yet
                    eof = False
                if ch.n == 0 and not eof:
                    raise ValueError("%s: chunk_bytes=%d holds no whole line of %s at byte %d; at least %d are needed"
                                     % (who, chunk_bytes, fname, file_pos, need))
                if ch.n:
                    wrong = np.flatnonzero(ch.num_boxes != O)
                    if wrong.size:
                        raise ValueError("%s: %s, img_id %r: num_boxes %d, the first line has %d (variable box counts are out of scope)"
                                         % (who, fname, ch.ids[wrong[0]], ch.num_boxes[wrong[0]], O))
                    if short is None:
                        bad = np.argwhere(ch.desc[:, 1:2 * len(KERNEL_FIELDS):2] != want_len)
                        if bad.size:
                            i, fld = int(bad[0, 0]), int(bad[0, 1])
                            short = (int(ch.lines[i, 0]) + file_pos - carry, ch.ids[i], DECODE_CONFIG[fld][0], int(ch.desc[i, 2 * fld + 1]))
                    if n + ch.n > cap:  # only lines shorter than a whole one can outnumber the bound from the file's size
                        if short is None:
                            raise ValueError("%s: %s holds more than the %d lines its size allows for" % (who, fname, cap))
                        raise ValueError("%s: %s, line at byte %d, img_id %r, field %s: %d characters, %d expected for %d boxes of %d features"
                                         % (who, fname, short[0], short[1], short[2], short[3],
                                            want_len[[c[0] for c in DECODE_CONFIG].index(short[2])], O, F))
                    doff = (got + 15) // 16 * 16
                    hd = cur[doff:doff + ch.n * N_DESC * 8].view(np.int64).reshape(ch.n, N_DESC)
                    hd[:] = ch.desc
                    # ONE copy: the chunk's text and, right behind it, its descriptors
                    upto = doff + ch.n * N_DESC * 8
                    dev_stage[:upto].copy_(stages[st][:upto], non_blocking=True)
                    events[st] = torch.cuda.Event()
                    events[st].record(stream)
                    ops.tsv_decode(dev_stage[:doff], got, dev_stage[doff:upto].view(torch.int64).view(ch.n, N_DESC), hd, O, F, tb, n,
                                   flags=flags[n:n + ch.n], counts=counts, normalize=normalize)
                    ids.extend(ch.ids), hs.append(ch.img_h), ws.append(ch.img_w)
                    where_lines.append(ch.lines + np.array([file_pos - carry, 0]))
                    n += ch.n
                file_pos += got - carry
                carry, prev_valid = ch.tail, got
                k += 1
            if n == 0:
                raise ValueError("%s: %s holds no line" % (who, fname))
            table = ObjTable({key: t[:n] for key, t in tb.items()}, ids, np.concatenate(hs), np.concatenate(ws), flags=flags[:n],
                             normalized=normalize)
            c = counts.cpu().numpy()  # the ONE read-back of a clean file
            if c[0] or c[1]:
                _patch(table, f, fname, np.concatenate(where_lines), bool(c[0]), check_boxes)
    return table


def _patch(table, f, fname, where_lines, redo, check_boxes):
    """after a non-zero counter: one read-back of the flags; lines with bits 0-2 by the host path, box failures reported"""
    fl = table.flags.cpu().numpy().view(np.uint32).copy()
    O, F, bf16 = table.N, table.F, table.feats.dtype == torch.bfloat16
    for r in (np.flatnonzero(fl & HOST_BITS) if redo else ()):
        f.seek(int(where_lines[r, 0]))
        fields = f.read(int(where_lines[r, 1])).split(b"\t")
        where = "%s, line at byte %d, img_id %r" % (fname, where_lines[r, 0], table.ids[r])
        oid, oc, aid, ac, bx, ft = _host_row(fields, O, F, where)
        b = np.array(bx, dtype=np.float32).reshape(O, 4)
        bit = 0
        if table.normalized:
            with np.errstate(all="ignore"):
                b[:, (0, 2)] /= np.float32(table.img_w[r])
                b[:, (1, 3)] /= np.float32(table.img_h[r])
            bd = b.astype(np.float64)
            bit = 0 if ((bd < 1 + 1e-5) & (-bd < 1e-5)).all() else BAD_BOX
        ft = ft.reshape(O, F)
        fl[r] = bit | (0 if np.isfinite(ft).all() else NONFINITE)
        parts = [(_bf16_bits(ft) if bf16 else ft), b, oid, aid, oc, ac, fl[r:r + 1]]
        blob = torch.from_numpy(np.concatenate([np.ascontiguousarray(p).reshape(-1).view(np.uint8) for p in parts])).to(table.device)
        o = 0
        for t in [getattr(table, key)[r] for key in IMAGE_TABLES] + [table.flags[r:r + 1]]:
            m = t.numel() * t.element_size()
            t.view(-1).view(torch.uint8).copy_(blob[o:o + m])
            o += m
        table.last_host_rows += 1
    bad = np.flatnonzero(fl & BAD_BOX)
    if bad.size and check_boxes:
        raise ValueError("load_obj_tsv_device: %s, img_id %r: a box outside [0, 1] after normalising by img_w=%d, img_h=%d (%d such images)"
                         % (fname, table.ids[bad[0]], table.img_w[bad[0]], table.img_h[bad[0]], bad.size))
