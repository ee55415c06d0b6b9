"""Seeded synthetic weights and VQA batches (numpy only, platform independent).

There is no dataset, vocabulary or LXMERT snapshot offline, so every test, the golden
generator and ``bench.py`` draw inputs from this one recipe:
identical tensors here, on the GPU box and inside the reference when the goldens
were generated.
"""
import zlib

import numpy as np


def _rng(seed, name):
    return np.random.default_rng([int(seed), zlib.crc32(name.encode())])


def seeded_param(name, shape, seed=0):
    """Deterministic value for a parameter called ``name`` (reference state_dict key).

    2-D weights ~ N(0, 0.02) (0.05 for the GAT layers), 1-D ``*.weight`` (LayerNorm
    gains) ~ 1 + 0.1 N(0,1), biases ~ 0.05 N(0,1), GIN ``eps`` ~ 0.1 N(0,1).  Non-trivial
    gains/biases make the parity checks sensitive to every term.
    """
    r = _rng(seed, name)
    shape = tuple(int(s) for s in shape)
    z = r.standard_normal(shape, dtype=np.float32)
    if name.endswith("eps"):
        return 0.1 * z
    if len(shape) >= 2:
        return (0.05 if "gat_layers" in name else 0.02) * z
    if name.endswith("weight"):
        return (1.0 + 0.1 * z).astype(np.float32)
    return (0.05 * z).astype(np.float32)


def seeded_state(named_shapes, seed=0):
    """``{name: shape}`` -> ``{name: float32 ndarray}``."""
    return {k: seeded_param(k, s, seed) for k, s in named_shapes.items()}


def vqa_batch(B, A=2274, N=36, T=20, F=2048, vocab=30522, seed=0):
    """One synthetic VQA batch shaped like the reference loader's output
    (src/vqa/vqacpv2_data.py:95-127) after host tokenisation (src/lxrt/entry.py:37-72).

    feats ~ U[0,3) [B,N,F]; boxes ~ U[0,1) [B,N,4]; ``[CLS] ids [SEP]`` padded to T with
    lengths U{5..T-1}; one-hot target over A; adj_true = (triu(U)+triu(U)^T)/max,
    mirroring data/preprocess/vqa/compute_adjacency.py:38-45,90; standard-normal draws
    for the two denoising branches.
    """
    r = _rng(seed, "vqa_batch")
    feats = (3.0 * r.random((B, N, F), dtype=np.float32)).astype(np.float32)
    boxes = r.random((B, N, 4), dtype=np.float32)
    ids = np.zeros((B, T), dtype=np.int64)
    mask = np.zeros((B, T), dtype=np.int64)
    lo = min(1000, vocab // 2)
    for b in range(B):
        L = int(r.integers(5, T))  # 5..T-1 tokens incl. [CLS]/[SEP]
        body = r.integers(lo, vocab, size=L - 2)
        ids[b, 0] = min(101, vocab - 2)
        ids[b, 1:L - 1] = body
        ids[b, L - 1] = min(102, vocab - 1)
        mask[b, :L] = 1
    seg = np.zeros((B, T), dtype=np.int64)
    target = np.zeros((B, A), dtype=np.float32)
    target[np.arange(B), r.integers(0, A, size=B)] = 1.0
    u = np.triu(r.random((B, N, N), dtype=np.float32))
    a = u + np.transpose(u, (0, 2, 1))
    a = (a / a.max(axis=(1, 2), keepdims=True)).astype(np.float32)
    randn_adj = r.standard_normal((B, N, N), dtype=np.float32)
    return dict(feats=feats, boxes=boxes, input_ids=ids, input_mask=mask, segment_ids=seg,
                target=target, adj_true=a, randn_adj=randn_adj)


def randn_nodes(B, N, H, seed=0):
    """standard-normal draw for the node branch (size depends on the hidden width)."""
    return _rng(seed, "randn_node").standard_normal((B, N, H), dtype=np.float32)


def generator_inputs(tag, kind, B, N, H, seed):
    """node features ~ N(0,1) and a noisy symmetric adjacency (zero diagonal; GAT gets
    ~30% exact zeros to exercise its ``adj == 0`` mask) for the generator parity cases."""
    r = _rng(seed, "gen_case:" + tag)
    x = r.standard_normal((B, N, H), dtype=np.float32)
    u = np.triu(r.random((B, N, N), dtype=np.float32), 1)
    a = u + u.transpose(0, 2, 1) + 0.3 * np.triu(r.standard_normal((B, N, N), dtype=np.float32), 1)
    if kind == "GAT":
        a = a * (r.random((B, N, N)) > 0.3)
    return x, np.ascontiguousarray(a.astype(np.float32))


def debias_case(B, A, Hd=0, seed=0, bias_max=None):
    """Inputs of one debias-loss parity case (tests/golden/make_debias_golden.py, tests/test_debias_gpu.py):
    logits ~ 6 N(0,1) with a few entries at +-30; labels: sparse soft scores (about 1 % non-zero, values in (0, 1]);
    bias ~ U[0,1) with entries that are exactly 0 and exactly 1 (``bias_max``: clipped to it, for the reweighting loss
    whose weights 1 - bias must not all vanish); with ``Hd``: hidden ~ N(0,1) [B, Hd], bias_lin.weight ~ 0.05 N(0,1)
    [1, Hd], bias_lin.bias ~ 0.3 N(0,1) [1].  All float32."""
    r = _rng(seed, "debias_case:%d:%d:%d" % (B, A, Hd))
    n = B * A
    logits = (6.0 * r.standard_normal((B, A), dtype=np.float32)).astype(np.float32)
    flat = logits.reshape(-1)
    hot = r.choice(n, size=min(6, n), replace=False)
    flat[hot] = np.where(np.arange(hot.size) % 2 == 0, 30.0, -30.0).astype(np.float32)
    labels = np.zeros((B, A), dtype=np.float32)
    k = max(1, n // 100)
    pos = r.choice(n, size=k, replace=False)
    labels.reshape(-1)[pos] = (1.0 - r.random(k, dtype=np.float32)).astype(np.float32)  # (0, 1]
    bias = r.random((B, A), dtype=np.float32)
    e = max(1, n // 50) if n >= 2 else 0
    ends = r.choice(n, size=2 * e, replace=False) if e else np.zeros(0, dtype=np.int64)
    bias.reshape(-1)[ends[:e]] = 0.0
    bias.reshape(-1)[ends[e:]] = 1.0
    if bias_max is not None:
        bias = np.minimum(bias, np.float32(bias_max))
    out = dict(logits=logits, labels=labels, bias=np.ascontiguousarray(bias, dtype=np.float32))
    if Hd:
        out["hidden"] = r.standard_normal((B, Hd), dtype=np.float32)
        out["lin_w"] = (0.05 * r.standard_normal((1, Hd), dtype=np.float32)).astype(np.float32)
        out["lin_b"] = (0.3 * r.standard_normal((1,), dtype=np.float32)).astype(np.float32)
    return out


def pretrain_case(B, T=20, O=36, F=2048, vocab=30522, n_obj=1600, n_attr=400, n_ans=9500, seed=0, mask_rate=0.15):
    """One synthetic pre-training batch shaped like what src/pretrain/lxmert_pretrain.py:146-215 hands to
    ``LXRTPretraining.forward`` (the host-side ``random_word`` / ``random_feat`` masking is not restated: labels,
    confidences and already-masked inputs are drawn directly).  ``[CLS] ids [SEP]`` padded to T; masked_lm_labels -1
    except on about ``mask_rate`` of the real tokens; every edge the parity cases need is forced when B >= 3: sample 0
    has NO masked token, sample 1 masks position 1 and its last real token, both matched classes occur, ``ans`` holds a
    -1, one object label is -1 under a positive confidence, one object row has confidence 0 in all three losses, and
    the feature targets lie on both sides of |prediction - target| = 1 of anything near zero.  All float32 / int64.
    (The masking itself, on the device: ``xggm_amd.pretrain.lxmert_pretrain.DeviceFeatures``.)"""
    r = _rng(seed, "pretrain_case:%d:%d:%d" % (B, T, O))
    ids = np.zeros((B, T), dtype=np.int64)
    mask = np.zeros((B, T), dtype=np.int64)
    labels = np.full((B, T), -1, dtype=np.int64)
    lo = min(1000, vocab // 2)
    for b in range(B):
        L = int(r.integers(min(5, T - 1), T)) if T > 5 else T
        ids[b, 0] = min(101, vocab - 2)
        ids[b, 1:L - 1] = r.integers(lo, vocab, size=L - 2)
        ids[b, L - 1] = min(102, vocab - 1)
        mask[b, :L] = 1
        pick = r.random(L) < mask_rate
        pick[0] = False
        labels[b, :L][pick] = r.integers(0, vocab, size=int(pick.sum()))
        if b == 0:
            labels[b] = -1
        elif b == 1:
            labels[b, 1] = 0
            labels[b, L - 1] = vocab - 1
    feats = (3.0 * r.random((B, O, F), dtype=np.float32)).astype(np.float32)
    boxes = r.random((B, O, 4), dtype=np.float32)
    matched = r.integers(0, 2, size=B).astype(np.int64)
    ans = r.integers(0, n_ans, size=B).astype(np.int64)
    obj_label = r.integers(0, n_obj, size=(B, O)).astype(np.int64)
    attr_label = r.integers(0, n_attr, size=(B, O)).astype(np.int64)
    obj_conf = r.random((B, O), dtype=np.float32)
    attr_conf = r.random((B, O), dtype=np.float32)
    feat_conf = (r.random((B, O)) < 0.5).astype(np.float32)
    # regression targets around zero, where a freshly initialised head predicts: |d| on both sides of 1
    feat_label = (1.2 * r.standard_normal((B, O, F), dtype=np.float32)).astype(np.float32)
    if B >= 2:
        matched[0], matched[1] = 1, 0
        ans[1] = -1
    obj_label[0, 0] = -1
    obj_conf[0, 0] = 0.75
    attr_label[B - 1, O - 1] = -1
    attr_conf[B - 1, O - 1] = 0.5
    feat_conf[0, 0] = 1.0
    for c in (obj_conf, attr_conf, feat_conf):
        c[0, O - 1] = 0.0
    seg = np.zeros((B, T), dtype=np.int64)
    return dict(input_ids=ids, input_mask=mask, segment_ids=seg, masked_lm_labels=labels, feats=feats, boxes=boxes,
                matched_label=matched, ans=ans, obj_label=obj_label, obj_conf=obj_conf, attr_label=attr_label,
                attr_conf=attr_conf, feat_label=feat_label, feat_conf=feat_conf)
