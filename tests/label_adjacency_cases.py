"""Shared pieces of the label-adjacency tests (tests/test_label_adjacency_cpu.py, tests/test_label_adjacency_gpu.py) and
of the fixture script tests/golden/make_bert_tiny_golden.py.  Importable without a GPU.

The tiny BERT: vocab_small.txt (81 entries), H 128 (2 heads of 64), 2 layers, intermediate 256, 32 positions.  Its weights
are not stored anywhere: ``tiny_bert_state`` draws every tensor from ``synth._rng(seed, key)``, so fixture script and test
rebuild the same checkpoint from the seed in the fixture.  At BERT's default initialisation (std 0.02) such a model barely
looks at its input -- two labels' pooled rows differ by 0.007 and every cosine is >= 0.999, so a path that ignored the
tokens or the mask would pass.  Hence std 0.1 with LayerNorm gains and all biases perturbed by 0.1; the script ASSERTS
that any two labels, and the masked and the unmasked run, differ by at least 100 x the bound the test compares at."""
import os

import numpy as np
import torch

from xggm_amd import synth

HERE = os.path.dirname(os.path.abspath(__file__))
VOCAB = os.path.join(HERE, "golden", "vocab_small.txt")
TINY = dict(vocab=81, hidden=128, heads=2, layers=2, inter=256, max_pos=32)
SEED = 31
REL_BOUND = 1e-4  # x max|golden|: the project's fp32 tensor bound (tests/test_model_gpu.py)

# 24 labels of 1 .. 5 word pieces over vocab_small.txt ("zebra": [UNK]); with [CLS] / [SEP] rows of 3 .. 7 tokens
LABELS = ["dog", "cat", "table", "red", "umbrella", "sky", "zebra",
          "holding", "street sign", "blue bus", "skateboard", "tennis racket", "played",
          "man holding", "snowboarder", "unaffable", "red street sign",
          "catlike dogs", "woman holding umbrella", "two people playing",
          "quickly fly kites", "woman holding blue umbrella", "people on the left table", "left of the blue kite"]


def tiny_bert_param(key, shape, seed):
    """2-D tensors 0.1 N(0, 1); LayerNorm gains 1 + 0.1 N(0, 1); every bias 0.1 N(0, 1)"""
    z = synth._rng(seed, "bert_tiny:" + key).standard_normal(tuple(int(s) for s in shape), dtype=np.float32)
    if len(shape) == 1 and key.endswith("LayerNorm.weight"):
        return (1.0 + 0.1 * z).astype(np.float32)
    return (0.1 * z).astype(np.float32)


def tiny_bert_state(named_shapes, seed=SEED):
    """{key: shape} of a BERT body (``embeddings.*``, ``encoder.layer.<i>.*``, ``pooler.dense.*``) -> {key: tensor}"""
    return {k: torch.from_numpy(tiny_bert_param(k, s, seed)) for k, s in named_shapes.items()}


def tiny_config():
    from xggm_amd.lxrt.modeling import BertConfig
    return BertConfig(TINY["vocab"], hidden_size=TINY["hidden"], num_hidden_layers=TINY["layers"], num_attention_heads=TINY["heads"],
                      intermediate_size=TINY["inter"], max_position_embeddings=TINY["max_pos"])


def tokenizer():
    from xggm_amd.lxrt.tokenization import BertTokenizer
    return BertTokenizer(VOCAB, do_lower_case=True)


def padded_rows(tok, labels):
    """``[CLS] pieces [SEP]`` of every label padded to the longest -> (ids int64 [V, T], mask int64 [V, T], pieces per label)"""
    from xggm_amd.preprocess.label_embeddings import label_ids
    rows = [label_ids(tok, s) for s in labels]
    T = max(len(r) for r in rows)
    ids = np.array([r + [0] * (T - len(r)) for r in rows], dtype=np.int64)
    mask = np.array([[1] * len(r) + [0] * (T - len(r)) for r in rows], dtype=np.int64)
    return ids, mask, [len(r) - 2 for r in rows]


def label_adjacency_numpy(table, oid, aid):
    """the label adjacency restated in numpy, fp32 throughout: look-ups for j >= i, c + c^T, divided by the maximum"""
    c = np.triu(table[oid[:, :, None], aid[:, None, :]].astype(np.float32))
    m = c + c.transpose(0, 2, 1)
    return m / m.max(axis=(1, 2), keepdims=True)


def cosine_table_numpy(cls, att, eps=1e-6):
    """the pair table in fp64 from fp32 embeddings (torch.cosine_similarity: each norm clamped from below)"""
    c, a = cls.astype(np.float64), att.astype(np.float64)
    nc, na = np.maximum(np.sqrt((c * c).sum(1)), eps), np.maximum(np.sqrt((a * a).sum(1)), eps)
    return (c @ a.T) / (nc[:, None] * na[None, :])
