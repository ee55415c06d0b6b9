"""float64 restatement of the pre-training batch corruption (src/pretrain/lxmert_pretrain.py:76-215: random_word,
random_feat, the QA answer draw) on position-indexed draws -- the contract of xggm_pretrain_corrupt_* in include/xggm.h,
written independently of the kernel in numpy and Python floats (IEEE double, what the reference computes with).
tests/golden/pretrain_mask.npz pins it to the reference's own functions."""
import numpy as np


def corrupt(input_ids, input_mask, feats, is_matched, label_ids, label_scores, draws, word_mask_rate=0.15, obj_mask_rate=0.15,
            vocab_size=30522, mask_id=103, pool=None):
    """numpy arrays in, dict(input_ids, masked_lm_labels, masked_feat, feat_mask, ans, word_kind, obj_kind) out.  ``draws``:
    dict of u_word, u_word_pick [B, T], u_obj, u_obj_pick [B, O], u_ans [B] (float32).  ``*_kind``: 0 untouched, 1 mask /
    zero, 2 random, 3 kept but labelled, -1 (tokens only) not eligible."""
    B, T = input_ids.shape
    _, O, F = feats.shape
    pool = feats.reshape(B * O, F) if pool is None else pool
    P = pool.shape[0]
    u_word, u_word_pick = draws["u_word"].reshape(B, T), draws["u_word_pick"].reshape(B, T)
    u_obj, u_obj_pick = draws["u_obj"].reshape(B, O), draws["u_obj_pick"].reshape(B, O)
    u_ans = draws["u_ans"].reshape(B)
    ids, labels = input_ids.copy(), np.full((B, T), -1, dtype=np.int64)
    word_kind = np.full((B, T), -1, dtype=np.int64)
    masked, feat_mask = feats.copy(), np.zeros((B, O), dtype=np.float32)
    obj_kind = np.zeros((B, O), dtype=np.int64)
    ans = np.full(B, -1, dtype=np.int64)
    for b in range(B):
        for t in range(1, T - 1):
            if input_mask[b, t] != 1 or input_mask[b, t + 1] != 1:
                continue
            word_kind[b, t] = 0
            prob = float(u_word[b, t])
            if prob < word_mask_rate:
                prob /= word_mask_rate
                labels[b, t] = input_ids[b, t]
                if prob < 0.8:
                    ids[b, t], word_kind[b, t] = mask_id, 1
                elif prob < 0.9:
                    ids[b, t], word_kind[b, t] = int(float(u_word_pick[b, t]) * vocab_size), 2
                else:
                    word_kind[b, t] = 3
        for o in range(O):
            prob = float(u_obj[b, o])
            if prob < obj_mask_rate:
                prob /= obj_mask_rate
                feat_mask[b, o] = 1.0
                if prob < 0.8:
                    masked[b, o], obj_kind[b, o] = 0, 1
                elif prob < 0.9:
                    masked[b, o], obj_kind[b, o] = pool[int(float(u_obj_pick[b, o]) * P)], 2
                else:
                    obj_kind[b, o] = 3
        keys = [(int(k), float(s)) for k, s in zip(label_ids[b], label_scores[b]) if k >= 0]
        if keys and is_matched[b] == 1:
            ans[b] = keys[-1][0]
            if len(keys) > 1:
                total = 0.0
                for _, s in keys:
                    total += s
                target, c = float(u_ans[b]) * total, 0.0
                for k, s in keys:
                    c += s
                    if target < c:
                        ans[b] = k
                        break
    return dict(input_ids=ids, masked_lm_labels=labels, masked_feat=masked, feat_mask=feat_mask, ans=ans, word_kind=word_kind,
                obj_kind=obj_kind)


def fp32_edges(cond, near):
    """(largest float32 x with cond(x), its successor) around ``near`` for a predicate that is true below a threshold"""
    x = np.float32(near)
    while not cond(float(x)):
        x = np.nextafter(x, np.float32(0))
    while cond(float(np.nextafter(x, np.float32(1)))):
        x = np.nextafter(x, np.float32(1))
    return x, np.nextafter(x, np.float32(1))


def philox_uniform(seed, offset, sid, n):
    """draws 0..n-1 of ``philox_uniform(seed, offset, sid, idx)`` (x-ggm_amd/csrc/common.h): Philox4x32-10 keyed by the seed,
    counter (idx >> 2, idx >> 34, sid, offset folded to 32 bits), word idx & 3, top 24 bits -> float32 in [0, 1)"""
    M = np.uint64(0xFFFFFFFF)
    idx = np.arange(n, dtype=np.uint64)
    c0, c1 = (idx >> np.uint64(2)) & M, (idx >> np.uint64(34)) & M
    c2 = np.full(n, sid, dtype=np.uint64) & M
    fold = ((int(offset) & 0xFFFFFFFF) ^ (((int(offset) >> 32) * 0x9E3779B9) & 0xFFFFFFFF)) & 0xFFFFFFFF
    c3 = np.full(n, fold, dtype=np.uint64)
    a, b = int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        h0, l0, h1, l1 = p0 >> np.uint64(32), p0 & M, p1 >> np.uint64(32), p1 & M
        c0, c1, c2, c3 = h1 ^ c1 ^ np.uint64(a), l1, h0 ^ c3 ^ np.uint64(b), l0
        a, b = (a + 0x9E3779B9) & 0xFFFFFFFF, (b + 0xBB67AE85) & 0xFFFFFFFF
    words = np.stack([c0, c1, c2, c3], axis=1)
    o = words[np.arange(n), (idx & np.uint64(3)).astype(np.int64)]
    return ((o >> np.uint64(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)).astype(np.float32)
