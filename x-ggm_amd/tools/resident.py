"""Device-resident data set: a whole split uploaded to HBM once, a batch assembled there by ONE launch.

``DataLoaderX`` is as good as a host loader gets (memory-mapped bf16 shards, pinned slots, one stream-ordered copy per
batch), but every visit of a sample still carries its 147 456 B of features across PCIe -- questions that share an image
ship the image again -- and a producer thread tokenises and copies rows beside a loop whose step takes milliseconds.
The features of a split fit in HBM many times over (120 000 images: 17.7 GB of bf16), so ``ResidentDataset`` stores

    feats [n_img, N, F]   the shard's own storage type (bf16, or fp32 for a ``float32`` parity shard)
    boxes [n_img, N, 4], adj [n_img, N, N]       or, in place of adj: pair_table [Vc, Va] with obj_labels / attr_labels
                                                  [n_img, N] int32 (``ObjTable.set_label_adjacency``): ``adj_true`` is
                                                  then made in the gather launch and no per-image table exists
    q_row [n_q] int32     the image row of every sample: an image is stored ONCE however many questions refer to it
    q_ids [n_q, T] int32, q_len [n_q] int32       what ``SentenceBatcher`` would produce for the question
    q_label, q_score [n_q, K]                     the (label, score) pairs ``fill_target`` would write, -1 = unused slot
    q_bias_index [n_q] int64                      optional: the prior-table row of a debias loss

and ``fill`` gathers ``order[start : start + B]`` into the trainer's static buffers with ``ops.batch_gather``: no producer
thread, no pinned ring, no host-to-device copy, no host work per step beyond the launch.  ``host_batch`` restates the
gather in numpy from the same tables -- the reference the kernel is tested against on the CPU, NOT a fallback: ``fill``
refuses CPU tensors like every other op.  Pre-training batches have a store of their own: ``pretrain.resident.ResidentPretrainSet``.
"""
import numpy as np
import torch

from ..lxrt.tokenization import DeviceTokenizer
from .shards import _bf16_bits

FIELDS = ("feats", "boxes", "adj_true", "input_ids", "input_mask", "segment_ids", "target", "bias_index", "sample")


class _Slots:
    """what ``fill_target`` assigns, recorded instead of written: {label: score}, a repeated label keeps its LAST score (as
    the sequential assignment into a target row does) at its first position"""

    def __init__(self):
        self.d = {}

    def __setitem__(self, label, score):
        self.d[int(label)] = np.float32(score)


def sample_tables(ts, batcher, A=None):
    """the per-sample host tables of ``ts`` (VQATorchDataset / GQATorchDataset: ``rows``, ``data``, ``raw_dataset``,
    ``fill_target``) -> dict of numpy arrays q_row, q_ids, q_len, q_label, q_score.  Everything the kernel will trust is
    checked here, once: image rows fit int32, token ids fit their row, labels lie in [0, A)."""
    ds = ts.raw_dataset
    A = int(A if A is not None else ds.num_answers)
    n_q, T = len(ts.data), int(batcher.T)
    rows = np.asarray(ts.rows, dtype=np.int64)
    if n_q < 1:
        raise ValueError("ResidentDataset: the data set holds no sample")
    if rows.shape != (n_q,) or rows.min() < 0 or rows.max() >= len(ts.shard):
        raise ValueError("ResidentDataset: image rows outside the shard's %d images" % len(ts.shard))
    q_ids, q_len, pairs = np.zeros((n_q, T), dtype=np.int32), np.zeros(n_q, dtype=np.int32), []
    dev_ids = None
    if isinstance(getattr(batcher, "tok", None), DeviceTokenizer):  # every question in one launch, one read-back
        dev_ids, dev_len = (t.cpu().numpy() for t in batcher.tok.encode([d[ds.sent_key] for d in ts.data], T))
    for i, d in enumerate(ts.data):
        ids = dev_ids[i, :dev_len[i]] if dev_ids is not None else batcher.ids_of(d[ds.sent_key])
        if len(ids) > T:
            raise ValueError("ResidentDataset: question %r has %d tokens, max_seq_length is %d" % (d["question_id"], len(ids), T))
        q_ids[i, :len(ids)] = ids
        q_len[i] = len(ids)
        s = _Slots()
        if "label" in d:  # test splits carry none: all slots stay unused, the target row zero
            ts.fill_target(d, s)
        for l in s.d:
            if not 0 <= l < A:
                raise ValueError("ResidentDataset: question %r has label %d outside the answer table [0, %d)"
                                 % (d["question_id"], l, A))
        pairs.append(s.d)
    K = max(1, max(len(p) for p in pairs))
    q_label, q_score = np.full((n_q, K), -1, dtype=np.int32), np.zeros((n_q, K), dtype=np.float32)
    for i, p in enumerate(pairs):
        if p:
            q_label[i, :len(p)] = list(p.keys())
            q_score[i, :len(p)] = list(p.values())
    return dict(q_row=rows.astype(np.int32), q_ids=q_ids, q_len=q_len, q_label=q_label, q_score=q_score)


def host_feats(f, out_f32=False):
    """feature rows of a host table (uint16 bf16 bit patterns or float32) as the batch tensor the gather kernels write: same
    type copied, fp32 -> bf16 rounded as ``torch.Tensor.to(torch.bfloat16)``, bf16 -> fp32 as ``bits << 16``"""
    f = np.ascontiguousarray(f)
    if f.dtype == np.float32:
        return torch.from_numpy(f.copy()) if out_f32 else torch.from_numpy(_bf16_bits(f).view(np.int16).copy()).view(torch.bfloat16)
    if f.dtype == np.uint16:
        return (torch.from_numpy((f.astype(np.uint32) << 16).view(np.float32)) if out_f32
                else torch.from_numpy(f.view(np.int16).copy()).view(torch.bfloat16))
    raise TypeError("gather_host: feats are %s, uint16 (bf16 bits) or float32 expected" % f.dtype)


def table_dtype(a, feats=False):
    """the numpy dtype a host table would have: an array's own, a tensor's counterpart (bf16 ``feats``: uint16 bit patterns)"""
    if not torch.is_tensor(a):
        return a.dtype
    if feats and a.dtype == torch.bfloat16:
        return np.dtype(np.uint16)
    return torch.empty(0, dtype=a.dtype).numpy().dtype if a.dtype != torch.bfloat16 else None


def adopted_to_host(host):
    """``host_batch`` on a store with adopted tables: read them back ON FIRST USE, into the host dict, as the numpy arrays
    an uploaded store would have kept (bf16 features as uint16 bit patterns)"""
    for k, v in host.items():
        if torch.is_tensor(v):
            v = v.detach().cpu().contiguous()
            host[k] = v.view(torch.int16).numpy().view(np.uint16) if v.dtype == torch.bfloat16 else v.numpy()
    return host


def gather_host(tables, indices, A, out_f32=False):
    """``ops.batch_gather`` restated in numpy: the batch of the samples ``indices`` out of host ``tables`` (numpy arrays
    under the kernel's names; ``feats`` uint16 bf16 bit patterns or float32) -> dict of CPU tensors under the trainer's
    names plus ``sample``.  Same-type features are copied, fp32 -> bf16 rounds as ``torch.Tensor.to(torch.bfloat16)``,
    bf16 -> fp32 is ``bits << 16``."""
    idx = np.asarray(indices, dtype=np.int64).reshape(-1)
    rows = tables["q_row"][idx].astype(np.int64)
    feats = host_feats(tables["feats"][rows], out_f32)
    B, T = len(idx), tables["q_ids"].shape[1]
    out = dict(feats=feats, boxes=torch.from_numpy(np.array(tables["boxes"][rows], dtype=np.float32)))
    if tables.get("adj") is not None:
        out["adj_true"] = torch.from_numpy(np.array(tables["adj"][rows], dtype=np.float32))
    elif tables.get("pair_table") is not None:  # a store without an [n_img, N, N] table: the label adjacency, restated
        from ..preprocess.compute_adjacency import label_adjacency_host
        out["adj_true"] = torch.from_numpy(label_adjacency_host(tables["pair_table"], tables["obj_labels"][rows], tables["attr_labels"][rows]))
    out["input_ids"] = torch.from_numpy(tables["q_ids"][idx].astype(np.int64))
    out["input_mask"] = torch.from_numpy((np.arange(T)[None, :] < tables["q_len"][idx][:, None]).astype(np.int64))
    out["segment_ids"] = torch.zeros((B, T), dtype=torch.int64)
    tgt = np.zeros((B, int(A)), dtype=np.float32)
    for b, s in enumerate(idx):
        for l, v in zip(tables["q_label"][s], tables["q_score"][s]):
            if l >= 0:
                tgt[b, l] = v
    out["target"] = torch.from_numpy(tgt)
    if tables.get("q_bias_index") is not None:
        out["bias_index"] = torch.from_numpy(tables["q_bias_index"][idx].astype(np.int64))
    out["sample"] = torch.from_numpy(idx.copy())
    return out


MAX_GROUPS = 16  # XGGM_SCORE_MAX_GROUPS (include/xggm.h)


def group_ids(data, key):
    """group ids for the per-group scores of a sweep (``AnswerLog.score_store(by_group=True)``): ``data`` is the list of
    datums in SAMPLE order (``ts.data``), ``key`` a field name (``"answer_type"`` on VQA-CP v2) or a callable datum -> name
    (head / tail / neither from the id lists of GQA-OOD).  -> (ids int32 [n], names): the distinct names sorted (by their
    string form, so that the ids do not depend on the order of the data), ``ids[i]`` the index of datum i's name."""
    name_of = key if callable(key) else (lambda d: d[key])
    values = [name_of(d) for d in data]
    names = sorted(set(values), key=str)
    index = {v: k for k, v in enumerate(names)}
    return np.asarray([index[v] for v in values], dtype=np.int32), names


def staged_upload(arr, device, chunk_bytes=64 << 20, stage=None, bf16_bits=False):
    """a host table (numpy array, a memory map included) -> (tensor on ``device``, the pinned staging buffer): copied chunk by
    chunk through ONE pinned buffer of ``chunk_bytes`` (``stage``: the buffer of an earlier call, reused; none is made for a
    CPU device).  ``bf16_bits``: a uint16 array of bf16 bit patterns becomes a bfloat16 tensor.  How both resident stores
    upload their tables."""
    device = torch.device(device)
    dt = torch.bfloat16 if bf16_bits else torch.from_numpy(np.empty(0, dtype=arr.dtype)).dtype
    dst = torch.empty(arr.shape, dtype=dt, device=device)
    flat = dst.view(-1).view(torch.int16) if bf16_bits else dst.view(-1)
    src = np.asarray(arr).reshape(-1)
    if bf16_bits:
        src = src.view(np.int16)
    if device.type != "cuda":
        flat.numpy()[:] = src
        return dst, stage
    if stage is None:
        stage = torch.empty(max(int(chunk_bytes), 4096), dtype=torch.uint8).pin_memory()
    per = stage.numel() // src.itemsize
    view = stage[:per * src.itemsize].view(flat.dtype)
    for o in range(0, src.shape[0], per):
        m = min(per, src.shape[0] - o)
        view.numpy()[:m] = src[o:o + m]
        flat[o:o + m].copy_(view[:m], non_blocking=True)
        torch.cuda.current_stream(device).synchronize()  # the ONE staging buffer is rewritten next
    return dst, stage


class ResidentDataset:
    def __init__(self, ts, batcher, device, bias_index=None, chunk_bytes=64 << 20, max_bytes=None, batch_size=None, groups=None,
                 group_names=None):
        """``ts``: a ``VQATorchDataset`` / ``GQATorchDataset`` (anything with ``.shard``, ``.rows``, ``.data``,
        ``.raw_dataset`` and ``fill_target``); ``batcher``: the model's ``SentenceBatcher``; ``bias_index``: [n_q] ints, the
        prior-table row of every sample for a debias loss, or None.  The shard's arrays are uploaded once through ONE
        pinned staging buffer of ``chunk_bytes``.  ``max_bytes``: refuse (ValueError naming the total) a split whose tables
        exceed it; default: the device's free memory minus 2 GiB.  ``batch_size``: default of ``order`` for ``world > 1``.
        ``groups``: [n_q] ints in [0, G), G <= 16 -- the answer type, head / tail ... of every sample, uploaded as the table
        ``q_group`` for ``AnswerLog.score_store(by_group=True)`` -- or the ``(ids, names)`` pair of ``group_ids``;
        ``group_names``: G names (default: the pair's, else the ids themselves)."""
        self.ts, self.batcher, self.device = ts, batcher, torch.device(device)
        self.batch_size = batch_size
        self.G, self.group_names, self._qid_index, self._keep = 0, None, None, None
        sh = ts.shard
        self.N, self.F, self.T, self.A = int(sh.N), int(sh.F), int(batcher.T), int(ts.raw_dataset.num_answers)
        if self.F % 8:
            raise ValueError("ResidentDataset: feat_dim %d is no multiple of 8 (feature rows move 16 bytes per lane)" % self.F)
        host = sample_tables(ts, batcher, self.A)
        if bias_index is not None:
            bi = np.asarray(bias_index, dtype=np.int64).reshape(-1)
            if bi.shape[0] != len(ts.data):
                raise ValueError("ResidentDataset: bias_index has %d entries for %d samples" % (bi.shape[0], len(ts.data)))
            host["q_bias_index"] = bi
        if groups is not None:
            if isinstance(groups, tuple):
                groups, names = groups
                group_names = names if group_names is None else group_names
            gi = np.asarray(groups, dtype=np.int64).reshape(-1)
            G = len(group_names) if group_names is not None else int(gi.max()) + 1 if gi.size else 0
            if gi.shape[0] != len(ts.data):
                raise ValueError("ResidentDataset: groups has %d entries for %d samples" % (gi.shape[0], len(ts.data)))
            if not 1 <= G <= MAX_GROUPS or gi.min() < 0 or gi.max() >= G:
                raise ValueError("ResidentDataset: group ids must lie in [0, G) with 1 <= G <= %d (G = %d, ids %d .. %d)"
                                 % (MAX_GROUPS, G, gi.min(), gi.max()))
            host["q_group"] = gi.astype(np.int32)
            self.G, self.group_names = G, list(group_names) if group_names is not None else list(range(G))
        # the shard's own arrays, as mapped: nothing is read before the upload (or host_batch) touches the rows
        # (a ``tools.tsv.ObjTable`` -- a feature file decoded on the device -- hands over its tensors: adopted, not copied)
        if hasattr(sh, "feats_bits"):
            host["feats"] = sh.feats_bits if sh.feats_f is None else sh.feats_f
        else:
            host["feats"] = sh.feats
        host["boxes"] = sh.boxes
        host["adj"] = sh.adj
        if getattr(sh, "pair_table", None) is not None:  # ``ObjTable.set_label_adjacency``: adj_true made in the gather
            if sh.adj is not None:
                raise ValueError("ResidentDataset: the shard holds a materialised adjacency AND a pair table; one source of adj_true only")
            host["pair_table"], host["obj_labels"], host["attr_labels"] = sh.pair_table, sh.obj_labels, sh.attr_labels
        self.host = host
        self.n, self.K = len(ts.data), host["q_label"].shape[1]
        self.nbytes = sum(int(v.numel() * v.element_size() if torch.is_tensor(v) else v.nbytes) for v in host.values() if v is not None)
        cuda = self.device.type == "cuda"
        if max_bytes is None and cuda:
            max_bytes = torch.cuda.mem_get_info(self.device)[0] - (2 << 30)
        if max_bytes is not None and self.nbytes > max_bytes:
            raise ValueError("ResidentDataset: the split needs %d bytes on the device, the limit is %d" % (self.nbytes, max_bytes))
        self._stage = None
        self.tables = {k: self._upload(k, v, int(chunk_bytes)) for k, v in host.items() if v is not None}
        self._stage = None  # the pinned staging buffer is only needed for the upload
        # ONE device buffer for every epoch's order: a captured ``fill`` keeps reading the same address
        self._order_buf = torch.zeros(self.n, dtype=torch.int64, device=self.device)
        self._order, self._order_host = None, None
        self.order(0, shuffle=False, drop_last=False)  # identity until the loop asks for an epoch

    def __len__(self):
        return self.n

    def _upload(self, name, arr, chunk_bytes):
        if torch.is_tensor(arr):  # a table that already lives on the device is adopted: no copy, the same storage
            same = arr.device.type == self.device.type and self.device.index in (None, arr.device.index)
            if not same or not arr.is_contiguous():
                raise ValueError("%s: table %s is a %s tensor on %s; only a contiguous tensor on the store's device %s is adopted"
                                 % (type(self).__name__, name, "contiguous" if arr.is_contiguous() else "strided", arr.device, self.device))
            return arr
        dst, self._stage = staged_upload(arr, self.device, chunk_bytes, self._stage, bf16_bits=name == "feats" and arr.dtype == np.uint16)
        return dst

    # ------------------------------------------------------------------ epoch order
    def order(self, epoch, shuffle=True, seed=0, rank=0, world=1, drop_last=True, batch_size=None):
        """this rank's sample indices of epoch ``epoch`` (host int64 array), uploaded as the order ``fill`` reads.  The
        permutation is the one ``DataLoaderX._batches`` draws for its epoch ``epoch`` with the same ``seed``; with
        ``world > 1`` step s covers ``perm[s B world : (s + 1) B world]`` and rank r takes the r-th B of it (``batch_size``
        here or in the constructor).  ``drop_last``: only whole (global) batches."""
        n = self.n
        perm = np.random.default_rng([seed, epoch]).permutation(n) if shuffle else np.arange(n)
        B = batch_size if batch_size is not None else self.batch_size
        if world > 1:
            if B is None:
                raise ValueError("ResidentDataset.order: world > 1 needs the batch size")
            if not 0 <= rank < world:
                raise ValueError("ResidentDataset.order: rank %d of %d" % (rank, world))
            steps = n // (B * world)  # a ragged global step cannot be split into equal ranks: always dropped
            perm = perm[:steps * B * world].reshape(steps, world, B)[:, rank].reshape(-1)
        elif drop_last and B is not None:
            perm = perm[:n // B * B]
        perm = np.ascontiguousarray(perm, dtype=np.int64)
        if len(perm) == 0:
            raise ValueError("ResidentDataset.order: no whole batch of %s in %d samples" % (B, n))
        self._order_host = perm
        self._order = self._order_buf[:len(perm)]
        self._order.copy_(torch.from_numpy(perm))
        return perm

    # ------------------------------------------------------------------ batches
    def fill(self, out, start, B):
        """rows ``order[start : start + B]`` into the device tensors ``out`` (the trainer's names: feats, boxes, adj_true,
        input_ids, input_mask, segment_ids, target and optionally bias_index, sample; other keys are left alone), ONE
        launch on the current stream."""
        for k, want in (("feats", (self.N, self.F)), ("input_ids", (self.T,)), ("target", (self.A,))):
            if k in out and tuple(out[k].shape[1:]) != want:
                raise ValueError("ResidentDataset.fill: out[%r] has rows of %s, the store holds N=%d F=%d T=%d A=%d"
                                 % (k, tuple(out[k].shape[1:]), self.N, self.F, self.T, self.A))
        sel = {k: out[k] for k in FIELDS if k in out}
        if "adj_true" in sel and "adj" not in self.tables and "pair_table" not in self.tables:
            raise ValueError("ResidentDataset.fill: the shard holds no adjacency")
        if "bias_index" in sel and "q_bias_index" not in self.tables:
            raise ValueError("ResidentDataset.fill: the store was built without bias_index")
        from .. import ops
        ops.batch_gather(self.tables, self._order, start, B, sel)
        return out

    def host_batch(self, indices, out_f32=False):
        """``fill`` restated in numpy from the same tables, for the SAMPLE indices given (not positions of the order):
        CPU tensors under the trainer's names plus ``sample``.  The CPU-testable reference of the kernel; no fallback."""
        return gather_host(adopted_to_host(self.host), indices, self.A, out_f32)

    def ques_ids(self, indices):
        """question ids of the samples ``indices`` (what ``fill`` leaves in ``sample``), for pairing with an ``AnswerLog``"""
        return [self.ts.data[int(i)]["question_id"] for i in np.asarray(indices).reshape(-1)]

    @property
    def qid_index(self):
        """[n_q] int64: the question id of every sample as a small int -- equal ids (strings included; a GQA datum is kept
        once per label) get equal ints.  Made on first use."""
        if self._qid_index is None:
            ids = [d["question_id"] for d in self.ts.data]
            self._qid_index = np.unique(np.asarray(ids), return_inverse=True)[1].astype(np.int64).reshape(-1)
        return self._qid_index

    def keep_mask(self, order=None):
        """device uint8 [len(order)] for ``AnswerLog.score_store(keep=)``: 1 where a sweep over the samples ``order`` (host
        indices; None: every sample in data set order, computed ONCE and kept) meets a question id for the last time -- the
        answers a ``quesid2ans`` dict filled in that order would hold"""
        from ..answers import last_occurrence_mask
        if order is None:
            if self._keep is None:
                self._keep = torch.from_numpy(last_occurrence_mask(self.qid_index)).to(self.device)
            return self._keep
        return torch.from_numpy(last_occurrence_mask(self.qid_index[np.asarray(order, dtype=np.int64)])).to(self.device)
