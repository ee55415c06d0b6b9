"""bert_tiny.npz: pooled outputs of a tiny seeded BERT for 24 labels, from the ``transformers`` BertModel.

What ``preprocess.label_embeddings.embed_labels`` is held to on the GPU (tests/test_label_adjacency_gpu.py).  The model is
built OFFLINE from a config -- ``BertModel(BertConfig(...))``, never a hub name -- and filled from
``label_adjacency_cases.tiny_bert_state`` (every tensor from ``synth._rng(seed, key)``), so the fixture stores the seed, the
labels, their token ids and mask and the pooled outputs, not weights.  Runs on the CPU, in fp64 (the test compares fp32
kernels at 1e-4 x max|golden|; the golden's own rounding is far below that).

The script asserts that the fixture can tell a wrong path from a right one: any two labels' pooled rows, and the masked
and the unmasked run of every padded row, differ by at least 100 x the bound the test compares at.

    python tests/golden/make_bert_tiny_golden.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))                   # tests/
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))  # the repository root

import label_adjacency_cases as C  # noqa: E402


def main():
    from transformers import BertConfig, BertModel
    t = C.TINY
    cfg = BertConfig(vocab_size=t["vocab"], hidden_size=t["hidden"], num_hidden_layers=t["layers"], num_attention_heads=t["heads"],
                     intermediate_size=t["inter"], max_position_embeddings=t["max_pos"], hidden_act="gelu", hidden_dropout_prob=0.0,
                     attention_probs_dropout_prob=0.0, layer_norm_eps=1e-12, type_vocab_size=2)
    model = BertModel(cfg).eval()
    body = {k: tuple(v.shape) for k, v in model.state_dict().items() if not k.endswith("position_ids")}
    missing, unexpected = model.load_state_dict(C.tiny_bert_state(body, C.SEED), strict=False)
    assert not unexpected and all(k.endswith("position_ids") for k in missing), (missing, unexpected)
    model = model.double()

    ids, mask, pieces = C.padded_rows(C.tokenizer(), C.LABELS)
    assert len(C.LABELS) == 24 and sorted(set(pieces)) == [1, 2, 3, 4, 5], pieces
    assert ids.shape[1] <= t["max_pos"] and ids.max() < t["vocab"]
    with torch.no_grad():
        tid, tmask = torch.from_numpy(ids), torch.from_numpy(mask)
        pooled = model(input_ids=tid, attention_mask=tmask, token_type_ids=torch.zeros_like(tid)).pooler_output.numpy()
        unmasked = model(input_ids=tid, attention_mask=torch.ones_like(tmask), token_type_ids=torch.zeros_like(tid)).pooler_output.numpy()
        # every row alone, unpadded: padding + mask must not change a row
        for v in range(len(C.LABELS)):
            n = int(mask[v].sum())
            alone = model(input_ids=tid[v:v + 1, :n], token_type_ids=torch.zeros_like(tid[v:v + 1, :n])).pooler_output.numpy()
            assert np.abs(alone[0] - pooled[v]).max() < 1e-12, v

    need = 100 * C.REL_BOUND * np.abs(pooled).max()
    diff = np.abs(pooled[:, None, :] - pooled[None, :, :]).max(axis=2)
    pair_min = diff[~np.eye(len(C.LABELS), dtype=bool)].min()
    padded = mask.sum(axis=1) < mask.shape[1]
    mask_min = np.abs(unmasked - pooled).max(axis=1)[padded].min()
    assert pair_min >= need, "two labels' pooled rows differ by %.3g only (%.3g needed): raise the scale" % (pair_min, need)
    assert mask_min >= need, "dropping the mask moves a padded row by %.3g only (%.3g needed): raise the scale" % (mask_min, need)
    cn = pooled / np.linalg.norm(pooled, axis=1, keepdims=True)
    cos = (cn @ cn.T)[~np.eye(len(C.LABELS), dtype=bool)]

    path = os.path.join(HERE, "bert_tiny.npz")
    np.savez_compressed(path, seed=np.int64(C.SEED), labels=np.array(C.LABELS), input_ids=ids, input_mask=mask, pooled=pooled)
    print("bert_tiny.npz: %d bytes; %d labels, rows of %d .. %d tokens; max|pooled| %.3f; smallest pairwise difference %.3f, "
          "smallest move without the mask %.3f (needed: %.4f); cosines %.3f .. %.3f"
          % (os.path.getsize(path), len(C.LABELS), mask.sum(1).min(), mask.sum(1).max(), np.abs(pooled).max(), pair_min, mask_min,
             need, cos.min(), cos.max()))


if __name__ == "__main__":
    main()
