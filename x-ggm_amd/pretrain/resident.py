"""Device-resident pre-training set: the whole corpus uploaded to HBM once, a clean batch -- swap included -- assembled
there by ONE launch.

``collate_examples`` tokenises B sentences and stacks B x O x F fp32 features on the host every step, and thirteen tensors
cross PCIe; an image that ten sentences describe crosses ten times per epoch.  ``ResidentPretrainSet`` stores

    per image   feats [n_img, O, F] (bf16 bits or fp32), boxes [n_img, O, 4], obj_labels / attr_labels [n_img, O] int32,
                obj_confs / attr_confs [n_img, O] fp32 -- an image is stored ONCE however many sentences refer to it
    per sample  q_row [n_q] int32 (the image row), q_ids [n_q, T] int32 ([CLS] tokens[:T - 2] [SEP], zero padded: the layout
                of ``collate_examples``), q_len [n_q] int32, q_label / q_score [n_q, K] (the keys of ``example.label`` in
                insertion order, -1 padded)

and ``fill`` gathers ``order[start : start + B]`` into a trainer's static buffers with ``ops.pretrain_gather`` (contract:
xggm_pretrain_gather in include/xggm.h).  Because the device now sees the whole corpus, the two deviations of the per-batch
device path go away: the matched-sentence swap draws its other sentence from EVERY sample of the store (the reference: "a
random datum of the data set", src/pretrain/lxmert_data.py:178-183) and ``feat_pool()`` hands the object masking every
object of every image (``torchdset.random_feat()``, :140-146).

``gather_pretrain_host`` restates the kernel in numpy from the same tables -- the reference the kernel is tested against on
the CPU, NOT a fallback: ``fill`` refuses CPU tensors like every other op."""
import numpy as np
import torch

from .. import ops
from ..lxrt.tokenization import DeviceTokenizer
from ..tools.resident import ResidentDataset, adopted_to_host, host_feats, table_dtype
from ..tools.shards import _bf16_bits
from .lxmert_pretrain import SID_BASE, image_id, image_key

IMAGE_TABLES = ("feats", "boxes", "obj_labels", "attr_labels", "obj_confs", "attr_confs")
SAMPLE_TABLES = ("q_row", "q_ids", "q_len", "q_label", "q_score")
TRIES = ops.PRETRAIN_SWAP_TRIES


def pretrain_tables(examples, tokenizer, max_seq_length, max_labels, n_answers=None, vocab_size=None, feats_bf16=False, images=None):
    """a list of ``InputExample`` -> the host tables of the store (numpy arrays under the kernel's names, plus ``uids``, the
    examples' uids as a list).  Images are de-duplicated by ``image_key`` in order of first appearance, which fixes the row
    order; sentences are laid out as ``collate_examples`` lays them out.  ``feats_bf16``: store the features as bf16 bit
    patterns (uint16, torch's rounding) instead of the examples' fp32.  Everything the kernel will trust is checked here,
    once, with a ValueError naming the example: rows fit int32, token ids lie in [0, vocab) (``vocab_size``, default: the
    tokenizer's vocabulary when it has one), labels in [0, n_answers) (``n_answers`` None: only negative ids are refused), at
    most ``max_labels`` keys, one shape for the object and attribute arrays of all images, F % 8 == 0.
    ``images``: a ``tools.tsv.ObjTable`` (a feature file decoded on the device).  The examples then carry only uid, sent,
    label and optionally img_id -- their feature members may be None --, the image row of an example is
    ``images.row_of[<its image id>]`` (``image_id``; a missing image raises ValueError naming the example), and the returned
    dict carries the table's device tensors as the six image tables, in the table's row order, for the store to adopt."""
    who = "pretrain_tables"
    n_q, T, K = len(examples), int(max_seq_length), int(max_labels)
    if n_q < 1 or T < 2 or K < 1:
        raise ValueError("%s: %d examples, max_seq_length %d, max_labels %d" % (who, n_q, T, K))
    if vocab_size is None and getattr(tokenizer, "vocab", None) is not None:
        vocab_size = len(tokenizer.vocab)
    rows, per_image = {}, []
    q_row, q_len = np.zeros(n_q, dtype=np.int32), np.zeros(n_q, dtype=np.int32)
    q_ids = np.zeros((n_q, T), dtype=np.int32)
    q_label, q_score = np.full((n_q, K), -1, dtype=np.int32), np.zeros((n_q, K), dtype=np.float32)
    shape = None
    dev_ids = None
    if isinstance(tokenizer, DeviceTokenizer):  # every sentence in one launch, one read-back; the checks below stay
        dev_ids, dev_len = (t.cpu().numpy() for t in tokenizer.encode([ex.sent for ex in examples], T))
    for i, ex in enumerate(examples):
        key = image_key(ex) if images is None else image_id(ex)
        r = rows.get(key) if images is None else images.row_of.get(key)
        if r is None and images is not None:
            raise ValueError("%s: example %r refers to image %r, which the feature table does not hold" % (who, ex.uid, key))
        if r is None:
            arrs = (np.asarray(ex.visual_feats[0], dtype=np.float32), np.asarray(ex.visual_feats[1], dtype=np.float32),
                    np.asarray(ex.obj_labels[0]), np.asarray(ex.attr_labels[0]),
                    np.asarray(ex.obj_labels[1], dtype=np.float32), np.asarray(ex.attr_labels[1], dtype=np.float32))
            if arrs[0].ndim != 2:
                raise ValueError("%s: example %r has features of shape %s, [O, F] expected" % (who, ex.uid, arrs[0].shape))
            O, F = arrs[0].shape
            if F % 8:
                raise ValueError("%s: example %r has feat_dim %d, no multiple of 8 (feature rows move 16 bytes per lane)" % (who, ex.uid, F))
            if shape is None:
                shape = (O, F)
            if (O, F) != shape or arrs[1].shape != (O, 4) or any(a.shape != (O,) for a in arrs[2:]):
                raise ValueError("%s: example %r has arrays of shapes %s, the first image has O=%d F=%d"
                                 % (who, ex.uid, [a.shape for a in arrs], shape[0], shape[1]))
            for a in arrs[2:4]:
                if a.size and (a.min() < -(1 << 31) or a.max() >= (1 << 31)):
                    raise ValueError("%s: example %r has an object / attribute label outside int32" % (who, ex.uid))
            r = rows[key] = len(per_image)
            if r >= (1 << 31) - 1:
                raise ValueError("%s: example %r would be image row %d, rows must fit int32" % (who, ex.uid, r))
            per_image.append(arrs)
        q_row[i] = r
        if dev_ids is not None:
            w = dev_ids[i, :dev_len[i]].astype(np.int64)
        else:
            tokens = ["[CLS]"] + tokenizer.tokenize(ex.sent.strip())[:T - 2] + ["[SEP]"]
            w = np.asarray(tokenizer.convert_tokens_to_ids(tokens), dtype=np.int64)
        if w.min() < 0 or (vocab_size is not None and w.max() >= vocab_size) or w.max() >= (1 << 31):
            raise ValueError("%s: example %r has a token id outside [0, %s)" % (who, ex.uid, vocab_size))
        q_ids[i, :len(w)], q_len[i] = w, len(w)
        lab = ex.label or {}
        if len(lab) > K:
            raise ValueError("%s: example %r has %d answer keys, at most %d fit" % (who, ex.uid, len(lab), K))
        for j, (k, v) in enumerate(lab.items()):
            if int(k) < 0 or (n_answers is not None and int(k) >= n_answers) or int(k) >= (1 << 31):
                raise ValueError("%s: example %r has label %d outside the answer table [0, %s)" % (who, ex.uid, int(k), n_answers))
            q_label[i, j], q_score[i, j] = int(k), v
    t = dict(q_row=q_row, q_ids=q_ids, q_len=q_len, q_label=q_label, q_score=q_score)
    if images is not None:
        t.update(images.tables())
    else:
        feats = np.stack([a[0] for a in per_image])
        t.update(feats=_bf16_bits(feats) if feats_bf16 else feats, boxes=np.stack([a[1] for a in per_image]),
                 obj_labels=np.stack([a[2] for a in per_image]).astype(np.int32),
                 attr_labels=np.stack([a[3] for a in per_image]).astype(np.int32),
                 obj_confs=np.stack([a[4] for a in per_image]), attr_confs=np.stack([a[5] for a in per_image]))
    t["uids"] = [ex.uid for ex in examples]
    return t


def check_tables(t):
    """the shapes, dtypes and index ranges ``ops.pretrain_gather`` trusts, for ready-made host tables -> (n_img, n_q, O, F, T, K)"""
    who = "ResidentPretrainSet"
    missing = [k for k in IMAGE_TABLES + SAMPLE_TABLES if t.get(k) is None]
    if missing:
        raise ValueError("%s: the tables lack %s" % (who, missing))
    f = t["feats"]
    dtype_of = lambda a: table_dtype(a, feats=a is f)
    if f.ndim != 3 or dtype_of(f) not in (np.uint16, np.float32):
        raise ValueError("%s: feats %s %s, [n_img, O, F] uint16 (bf16 bits) or float32 expected" % (who, f.shape, f.dtype))
    n_img, O, F = f.shape
    n_q = t["q_row"].shape[0]
    if t["q_ids"].ndim != 2 or t["q_label"].ndim != 2:
        raise ValueError("%s: q_ids [n_q, T] and q_label [n_q, K] expected" % who)
    T, K = t["q_ids"].shape[1], t["q_label"].shape[1]
    if F % 8:
        raise ValueError("%s: feat_dim %d is no multiple of 8 (feature rows move 16 bytes per lane)" % (who, F))
    want = dict(boxes=((n_img, O, 4), np.float32), obj_labels=((n_img, O), np.int32), attr_labels=((n_img, O), np.int32),
                obj_confs=((n_img, O), np.float32), attr_confs=((n_img, O), np.float32), q_row=((n_q,), np.int32),
                q_ids=((n_q, T), np.int32), q_len=((n_q,), np.int32), q_label=((n_q, K), np.int32), q_score=((n_q, K), np.float32))
    for k, (shape, dt) in want.items():
        if tuple(t[k].shape) != shape or dtype_of(t[k]) != dt:
            raise ValueError("%s: table %s is %s %s, %s %s expected" % (who, k, tuple(t[k].shape), t[k].dtype, shape, np.dtype(dt)))
    if min(n_img, n_q, O, F, T, K) < 1:
        raise ValueError("%s: empty tables" % who)
    if t["q_row"].min() < 0 or t["q_row"].max() >= n_img:
        raise ValueError("%s: q_row outside the %d images" % (who, n_img))
    if t["q_len"].min() < 0 or t["q_len"].max() > T:
        raise ValueError("%s: q_len outside [0, %d]" % (who, T))
    if t["q_ids"].min() < 0 or t["q_label"].min() < -1:
        raise ValueError("%s: negative token id, or a label below -1" % who)
    if t.get("uids") is not None and len(t["uids"]) != n_q:
        raise ValueError("%s: %d uids for %d samples" % (who, len(t["uids"]), n_q))
    return n_img, n_q, O, F, T, K


def swap_host(q_row, samples, u_swap, u_pick, rate):
    """the fused swap of xggm_pretrain_gather in numpy and Python floats: for the batch rows of ``samples`` -> (sentence
    sample per row, is_matched, swapped_from, exhausted).  The pool is every sample of the store, the image key ``q_row``."""
    n_q, B = len(q_row), len(samples)
    u_swap, u_pick = np.asarray(u_swap, dtype=np.float32).reshape(B), np.asarray(u_pick, dtype=np.float32).reshape(B, TRIES)
    sent, matched, frm, exhausted = np.array(samples, dtype=np.int64), np.ones(B, dtype=np.int64), np.full(B, -1, dtype=np.int64), 0
    for b, s in enumerate(samples):
        if not float(u_swap[b]) < rate:
            continue
        for r in range(TRIES):
            v = float(u_pick[b, r]) * float(n_q)
            j = min(int(v) if v >= 0.0 else 0, n_q - 1)
            if q_row[j] != q_row[s]:
                sent[b], matched[b], frm[b] = j, 0, j
                break
        else:
            exhausted += 1
    return sent, matched, frm, exhausted


def gather_pretrain_host(tables, indices, draws=None, match_rate=None, out_f32=False):
    """``ops.pretrain_gather`` restated in numpy: the clean batch of the samples ``indices`` out of host ``tables`` -> dict of
    CPU tensors under the names of ``engine.CapturedPretrainer.KEYS`` plus img_ids, sample, swapped_from and exhausted
    (int32 [1]: the rows of THIS batch that found no other image).  ``match_rate`` not None: the swap, from the explicit
    ``draws`` = dict(u_swap [B], u_pick [B, 8]) (fp32).  The CPU-testable reference of the kernel; no fallback."""
    idx = np.asarray(indices, dtype=np.int64).reshape(-1)
    B, T = len(idx), tables["q_ids"].shape[1]
    rows = tables["q_row"][idx].astype(np.int64)
    sent, matched, frm, exhausted = idx, np.ones(B, dtype=np.int64), np.full(B, -1, dtype=np.int64), 0
    if match_rate is not None:
        if draws is None or "u_swap" not in draws or "u_pick" not in draws:
            raise ValueError("gather_pretrain_host: a swap needs draws = dict(u_swap, u_pick)")
        sent, matched, frm, exhausted = swap_host(tables["q_row"], idx, draws["u_swap"], draws["u_pick"], float(match_rate))
    elif draws:
        raise ValueError("gather_pretrain_host: swap draws without a match_rate")
    i64 = lambda a: torch.from_numpy(np.ascontiguousarray(a).astype(np.int64))
    f32 = lambda a: torch.from_numpy(np.array(a, dtype=np.float32))
    return dict(input_ids=i64(tables["q_ids"][sent]),
                input_mask=i64(np.arange(T)[None, :] < tables["q_len"][sent][:, None]),
                segment_ids=torch.zeros((B, T), dtype=torch.int64),
                feats=host_feats(tables["feats"][rows], out_f32), boxes=f32(tables["boxes"][rows]),
                obj_labels=i64(tables["obj_labels"][rows]), obj_confs=f32(tables["obj_confs"][rows]),
                attr_labels=i64(tables["attr_labels"][rows]), attr_confs=f32(tables["attr_confs"][rows]),
                is_matched=torch.from_numpy(matched), label_ids=i64(tables["q_label"][idx]),
                label_scores=f32(tables["q_score"][idx]), img_ids=torch.from_numpy(rows.copy()),
                sample=torch.from_numpy(idx.copy()), swapped_from=torch.from_numpy(frm),
                exhausted=torch.tensor([exhausted], dtype=torch.int32))


class ResidentPretrainSet:
    def __init__(self, source, device, tokenizer=None, max_seq_length=None, max_labels=4, n_answers=None, vocab_size=None,
                 feats_bf16=False, match_rate=None, sid_base=SID_BASE, chunk_bytes=64 << 20, max_bytes=None, batch_size=None):
        """``source``: ready host tables (a dict as ``pretrain_tables`` returns it) or a list of ``InputExample`` (then
        ``tokenizer`` and ``max_seq_length`` are needed and ``max_labels`` / ``n_answers`` / ``vocab_size`` / ``feats_bf16``
        go to ``pretrain_tables``).  An image table of ``source`` that is a tensor on ``device`` already (``pretrain_tables(...,
        images=table)``: a feature file decoded on the device) is adopted -- the same storage, no copy, counted in ``nbytes``
        like an uploaded one; ``host_batch`` reads it back on first use.  ``match_rate`` (None: no swap): the fused matched-sentence swap of ``fill``, drawn at
        Philox streams ``sid_base + 5 / 6``.  The tables are uploaded once through ONE pinned staging buffer of
        ``chunk_bytes``; ``max_bytes``: refuse (ValueError naming the total) a corpus whose tables exceed it, default: the
        device's free memory minus 2 GiB.  ``batch_size``: the default of ``order`` and of the driver loop."""
        if not isinstance(source, dict):
            if tokenizer is None or max_seq_length is None:
                raise ValueError("ResidentPretrainSet: a list of examples needs tokenizer and max_seq_length")
            source = pretrain_tables(source, tokenizer, max_seq_length, max_labels, n_answers, vocab_size, feats_bf16)
        self.n_img, self.n, self.O, self.F, self.T, self.K = check_tables(source)
        self.device, self.batch_size, self.sid_base = torch.device(device), batch_size, int(sid_base)
        self.match_rate = None if match_rate is None else float(match_rate)
        if self.match_rate is not None and not 0.0 <= self.match_rate <= 1.0:
            raise ValueError("ResidentPretrainSet: match_rate %r outside [0, 1]" % (match_rate,))
        self._uids = source.get("uids")
        # numpy arrays to upload, or (image tables) tensors that already live on the device: adopted, not copied
        self.host = {k: source[k] for k in IMAGE_TABLES + SAMPLE_TABLES}
        self.nbytes = sum(int(v.numel() * v.element_size() if torch.is_tensor(v) else v.nbytes) for v in self.host.values())
        cuda = self.device.type == "cuda"
        if max_bytes is None and cuda:
            max_bytes = torch.cuda.mem_get_info(self.device)[0] - (2 << 30)
        if max_bytes is not None and self.nbytes > max_bytes:
            raise ValueError("ResidentPretrainSet: the corpus needs %d bytes on the device, the limit is %d" % (self.nbytes, max_bytes))
        self._stage = None
        self.tables = {k: self._upload(k, v, int(chunk_bytes)) for k, v in self.host.items()}
        self._stage = None  # the pinned staging buffer is only needed for the upload
        # ONE device buffer for every epoch's order: a captured ``fill`` keeps reading the same address
        self._order_buf = torch.zeros(self.n, dtype=torch.int64, device=self.device)
        self._order, self._order_host = None, None
        self.swap_exhausted = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.order(0, shuffle=False, drop_last=False)  # identity until the loop asks for an epoch

    @classmethod
    def from_args(cls, args, source, device, **kw):
        """the swap follows ``--taskMatched`` (rate 0.5 when the flag is set, src/pretrain/lxmert_data.py:177-178), as
        ``DeviceFeatures.from_args(swap=True)`` does for the per-batch path"""
        if "match_rate" not in kw:
            kw["match_rate"] = 0.5 if getattr(args, "task_matched", False) else None
        return cls(source, device, **kw)

    def __len__(self):
        return self.n

    _upload = ResidentDataset._upload  # the same scheme: one pinned staging buffer, chunk by chunk

    def order(self, epoch, shuffle=True, seed=0, rank=0, world=1, drop_last=True, batch_size=None):
        """this rank's sample indices of epoch ``epoch`` (host int64 array), uploaded as the order ``fill`` reads: the
        semantics and the permutation of ``tools.resident.ResidentDataset.order``"""
        return ResidentDataset.order(self, epoch, shuffle=shuffle, seed=seed, rank=rank, world=world, drop_last=drop_last,
                                     batch_size=batch_size)

    # ------------------------------------------------------------------ batches
    def buffers(self, B, out_dtype=None):
        """fresh device buffers of a clean batch of ``B`` rows under the trainer's names (``ops.PRETRAIN_GATHER_OUT`` plus
        sample); feats in ``out_dtype`` (default: the table's)"""
        dev, i64, f32 = self.device, torch.int64, torch.float32
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
        return dict(input_ids=z((B, self.T), i64), input_mask=z((B, self.T), i64), segment_ids=z((B, self.T), i64),
                    feats=z((B, self.O, self.F), out_dtype or self.tables["feats"].dtype), boxes=z((B, self.O, 4), f32),
                    obj_labels=z((B, self.O), i64), obj_confs=z((B, self.O), f32), attr_labels=z((B, self.O), i64),
                    attr_confs=z((B, self.O), f32), is_matched=z((B,), i64), label_ids=z((B, self.K), i64),
                    label_scores=z((B, self.K), f32), img_ids=z((B,), i64), sample=z((B,), i64))

    def fill(self, out, start, B, rng=None, draws=None, sid_base=None, swap=True):
        """rows ``order[start : start + B]`` into the device tensors ``out`` (the trainer's names: every one of
        ``ops.PRETRAIN_GATHER_OUT`` and optionally sample, swapped_from; other keys are left alone), ONE launch on the
        current stream.  With a ``match_rate`` the swap is fused in: drawn from ``rng`` (int64 [2], the model's runtime
        state) at streams ``sid_base + 5 / 6`` (default: the store's ``sid_base``) or from the explicit ``draws``;
        ``swap=False``: a clean gather whatever the store's rate.  Exhausted rows are counted in ``swap_exhausted``."""
        for k, want in (("feats", (self.O, self.F)), ("input_ids", (self.T,)), ("label_ids", (self.K,))):
            if k in out and tuple(out[k].shape[1:]) != want:
                raise ValueError("ResidentPretrainSet.fill: out[%r] has rows of %s, the store holds O=%d F=%d T=%d K=%d"
                                 % (k, tuple(out[k].shape[1:]), self.O, self.F, self.T, self.K))
        sel = {k: out[k] for k in ops.PRETRAIN_GATHER_OUT + ("sample", "swapped_from") if k in out}
        rate = self.match_rate if swap else None
        ops.pretrain_gather(self.tables, self._order, start, B, sel, match_rate=rate, rng=rng if rate is not None else None,
                            sid_base=self.sid_base if sid_base is None else sid_base, draws=draws,
                            exhausted=self.swap_exhausted if rate is not None else None)
        return out

    def host_batch(self, indices, draws=None, out_f32=None):
        """``fill`` restated in numpy from the same tables, for the SAMPLE indices given (not positions of the order); the
        swap only from explicit ``draws``, else a clean batch.  feats in the table's type unless ``out_f32`` says otherwise.
        The CPU-testable reference of the kernel; no fallback."""
        adopted_to_host(self.host)
        if out_f32 is None:
            out_f32 = self.host["feats"].dtype == np.float32
        return gather_pretrain_host(self.host, indices, draws=draws, match_rate=self.match_rate if draws else None, out_f32=out_f32)

    def uids(self, indices):
        """uids of the samples ``indices`` (what ``fill`` leaves in ``sample``), for pairing with an ``AnswerLog``"""
        idx = np.asarray(indices).reshape(-1)
        return [int(i) for i in idx] if self._uids is None else [self._uids[int(i)] for i in idx]

    def feat_pool(self):
        """every object of every image, the feature table viewed as [n_img * O, F] (no copy): the replacement rows of the
        object masking, ``torchdset.random_feat()`` of the reference"""
        return self.tables["feats"].view(self.n_img * self.O, self.F)

    def sent_pool(self):
        """(pool_ids, pool_mask, pool_img) of ALL samples expanded to int64, the pool ``ops.pretrain_swap`` takes.  For tests
        and small stores only: it costs 16 T + 8 bytes per sample, four times the tables it is made from."""
        t = self.tables
        T = torch.arange(self.T, device=self.device)
        return (t["q_ids"].to(torch.int64), (T[None, :] < t["q_len"][:, None]).to(torch.int64), t["q_row"].to(torch.int64))
