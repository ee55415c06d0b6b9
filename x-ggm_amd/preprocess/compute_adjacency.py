"""Attribute-class cosine adjacency of the object regions (``adj_true``), on the GPU.

Reference: data/preprocess/vqa/compute_adjacency.py -- per image, BERT pooled embeddings of the 36 detected
objects' class names and attribute names (:77-85), then ``compute_cosin_sim_v2`` (:38-45: a Python double loop
of 666 ``torch.cosine_similarity`` calls filling the upper triangle incl. the diagonal, ``adj + adj^T``) and
``matrix / matrix.max()`` (:90).  The GQA twin (data/preprocess/gqa/compute_adjacency.py) is the same arithmetic.
This module takes the embeddings -- in practice a [vocabulary, 768] table per label file, gathered by the objects'
ids -- and runs the similarity for a whole split in one launch (``xggm_cosine_adjacency_f32``;
``xggm_cosine_adjacency_long_f32`` for 65..128 objects), one workgroup per image.  The tables themselves come from
``preprocess.label_embeddings``: a local ``bert-base-uncased`` checkpoint (never a hub name) and the two vocabulary
files, encoded by the package's own BERT layers.

An image's adjacency depends only on its 2 N label ids, and there are only Vc x Va distinct cosines (1600 x 400 in
the published vocabularies: 2.56 MB).  ``label_pair_table`` computes them once (``xggm_label_cosine_table_f32``, the
per-image kernels' arithmetic: the same bits) and ``build_adjacency_from_labels`` builds a split by look-ups
(``xggm_label_adjacency_f32``): no embedding gather, no chunk temporaries, bit-equal to ``build_adjacency``.  A
resident store can skip the [n_img, N, N] table altogether (``ObjTable.set_label_adjacency``): the batch gather then
makes ``adj_true`` from the labels."""
import numpy as np
import torch

from .. import _lib
from .._lib import call, ptr, stream


def compute_cosin_sim_v2(matrix1, matrix2, normalize=False):
    """matrix1 / matrix2: fp32 device tensors [N, D] (one image, the reference's signature, :38) or [n, N, D]
    (a batch) -> [N, N] / [n, N, N].  ``normalize`` also applies the ``matrix / matrix.max()`` of :90 -- the
    kernel always computes it; without it the result is scaled back."""
    single = matrix1.dim() == 2
    a = matrix1.unsqueeze(0) if single else matrix1
    b = matrix2.unsqueeze(0) if single else matrix2
    if not a.is_cuda:
        raise RuntimeError("xggm_amd: embeddings must live on the GPU (no CPU fallback)")
    a, b = a.contiguous().float(), b.contiguous().float()
    n, N, D = a.shape
    assert b.shape == a.shape
    out = torch.empty((n, N, N), device=a.device, dtype=torch.float32)
    # 65..128 objects (100-box features): the kernel laid out for them, picked by N alone -- there is no model to opt in on
    call("xggm_cosine_adjacency_long_f32" if N > 64 else "xggm_cosine_adjacency_f32", ptr(a), ptr(b), ptr(out), n, N, D,
         1e-6, stream())
    if not normalize:
        # un-normalised form: the maximum of adj + adj^T is max over (i <= j) of (1 + [i == j]) cos_ij; recover it
        # from the diagonal-doubled matrix the kernel divided by it
        an = a / a.norm(dim=-1, keepdim=True).clamp_min(1e-6)
        bn = b / b.norm(dim=-1, keepdim=True).clamp_min(1e-6)
        c = torch.einsum("nid,njd->nij", an, bn).triu()
        mx = (c + c.transpose(1, 2)).flatten(1).max(dim=1)[0]
        out = out * mx.view(n, 1, 1)
    return out[0] if single else out


def build_adjacency(class_table, attr_table, objects_id, attrs_id, chunk=4096):
    """adjacency of every image of a split.  class_table / attr_table: fp32 [vocabulary, D] pooled embeddings of the
    label strings (objects_vocab.txt / attributes_vocab.txt, :66-69); objects_id / attrs_id: int64 [n_img, N] -- the
    ``objects_id`` / ``attrs_id`` datasets of the detection h5 (:75-76).  Returns fp32 [n_img, N, N] on the device
    of the tables (what ``*_obj36_adj_v2.h5`` holds, one dataset per image)."""
    n = objects_id.shape[0]
    outs = []
    for s in range(0, n, chunk):
        oc = objects_id[s:s + chunk].to(class_table.device)
        ac = attrs_id[s:s + chunk].to(attr_table.device)
        outs.append(compute_cosin_sim_v2(class_table[oc], attr_table[ac], normalize=True))
    return torch.cat(outs)


def label_pair_table(class_table, attr_table, eps=1e-6):
    """class_table [Vc, D], attr_table [Va, D]: fp32 pooled embeddings of the label strings, on the GPU, D % 4 == 0 ->
    fp32 [Vc, Va]: the cosine of every (class, attribute) pair, with the bits the per-image kernels compute for it."""
    if not class_table.is_cuda or not attr_table.is_cuda:
        raise RuntimeError("xggm_amd: embeddings must live on the GPU (no CPU fallback)")
    if class_table.dim() != 2 or attr_table.dim() != 2 or class_table.shape[1] != attr_table.shape[1]:
        raise ValueError("label_pair_table: tables %s and %s, [Vc, D] and [Va, D] expected"
                         % (tuple(class_table.shape), tuple(attr_table.shape)))
    c, a = class_table.contiguous().float(), attr_table.contiguous().float()
    out = torch.empty((c.shape[0], a.shape[0]), device=c.device, dtype=torch.float32)
    call("xggm_label_cosine_table_f32", ptr(c), ptr(a), ptr(out), c.shape[0], a.shape[0], c.shape[1], eps, stream())
    return out


def check_label_range(pair_table, objects_id, attrs_id, who):
    """ValueError naming the offending range unless every class id lies in [0, Vc) and every attribute id in [0, Va):
    one device min/max (of ids already there) and ONE read-back"""
    Vc, Va = pair_table.shape
    if objects_id.numel() == 0:
        raise ValueError("%s: no label ids" % who)
    o, a = torch.aminmax(objects_id), torch.aminmax(attrs_id)
    lo_o, hi_o, lo_a, hi_a = torch.stack([v.to(torch.int64) for v in (*o, *a)]).tolist()
    if lo_o < 0 or hi_o >= Vc or lo_a < 0 or hi_a >= Va:
        raise ValueError("%s: class ids %d .. %d (table: [0, %d)), attribute ids %d .. %d (table: [0, %d))"
                         % (who, lo_o, hi_o, Vc, lo_a, hi_a, Va))


def build_adjacency_from_labels(pair_table, objects_id, attrs_id, check=True):
    """``build_adjacency`` without the embeddings: pair_table fp32 [Vc, Va] (``label_pair_table``) on the GPU, objects_id
    / attrs_id integer [n_img, N], 1 <= N <= 128 -> fp32 [n_img, N, N] on the table's device, bit-equal to
    ``build_adjacency(class_table, attr_table, objects_id, attrs_id)``.  An id outside the table raises ValueError before
    anything is launched (``check``: False when the caller has checked these ids already)."""
    who = "build_adjacency_from_labels"
    if not pair_table.is_cuda:
        raise RuntimeError("xggm_amd: the pair table must live on the GPU (no CPU fallback)")
    if pair_table.dim() != 2 or pair_table.dtype != torch.float32 or not pair_table.is_contiguous():
        raise ValueError("%s: pair table %s %s, contiguous float32 [Vc, Va] expected" % (who, tuple(pair_table.shape), pair_table.dtype))
    if objects_id.dim() != 2 or tuple(attrs_id.shape) != tuple(objects_id.shape):
        raise ValueError("%s: ids %s and %s, two [n_img, N] expected" % (who, tuple(objects_id.shape), tuple(attrs_id.shape)))
    n, N = objects_id.shape
    if n < 1 or not 1 <= N <= 128:
        raise ValueError("%s: %d images of %d objects (at least one image, 1..128 objects)" % (who, n, N))
    oid, aid = objects_id.to(pair_table.device), attrs_id.to(pair_table.device)
    if check:
        check_label_range(pair_table, oid, aid, who)
    oid, aid = oid.to(torch.int32).contiguous(), aid.to(torch.int32).contiguous()
    out = torch.empty((n, N, N), device=pair_table.device, dtype=torch.float32)
    call("xggm_label_adjacency_f32", ptr(pair_table), pair_table.shape[0], pair_table.shape[1], ptr(oid), ptr(aid), ptr(out), n, N,
         stream())
    return out


def label_adjacency_host(pair_table, objects_id, attrs_id):
    """``xggm_label_adjacency_f32`` restated in numpy (fp32 throughout; ids inside the table) -> float32 [n, N, N].  What
    ``ResidentDataset.host_batch`` states the gather's ``adj_true`` with; the CPU-testable reference, NOT a fallback."""
    t = np.asarray(pair_table, dtype=np.float32)
    o, a = np.asarray(objects_id, dtype=np.int64), np.asarray(attrs_id, dtype=np.int64)
    c = np.triu(t[o[:, :, None], a[:, None, :]])
    m = c + c.transpose(0, 2, 1)
    return (m / m.max(axis=(1, 2), keepdims=True)).astype(np.float32)
