"""BERT pooled embeddings of the detector's label strings: the [vocabulary, H] tables ``compute_adjacency`` starts from.

Reference: data/preprocess/vqa/compute_adjacency.py:20-25 (``tokenizer.encode(sent)`` -> ``model(ids)[1]``: the pooled
output of ``bert-base-uncased`` for ``[CLS] pieces [SEP]``), called for the 36 class names and the 36 attribute names of
every image (:77-85) -- 72 forwards per image.  The names come from two vocabulary files (:66-69, ``read_txt`` of
src/utils.py:130-133), so here every distinct label is encoded ONCE, in padded batches, by a language-only encoder made of
the package's own layers (``BertEmbeddings``, ``BertLayer``, ``BertPooler``: the HIP kernels the model trains with, fp32
compute, dropout off).  The weights are read from a LOCAL checkpoint; nothing is fetched by name.  The real
``bert-base-uncased`` weights and the published vocabulary files are not part of this repository: the path is exercised
through a tiny seeded BERT (tests/golden/bert_tiny.npz)."""
import os

import torch
import torch.nn as nn

from ..lxrt.modeling import BertConfig, BertEmbeddings, BertLayer, BertPooler, check_sequence_limits
from ..runtime import bind_root

IGNORED = ("cls.",)  # the pre-training heads of a BertForPreTraining checkpoint


class _Layers(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.layer = nn.ModuleList([BertLayer(config) for _ in range(config.num_hidden_layers)])


class LabelEncoder(nn.Module):
    """embeddings -> ``num_hidden_layers`` x BertLayer -> pooler, under the key names of a BERT checkpoint
    (``embeddings.*``, ``encoder.layer.<i>.*``, ``pooler.dense.*``).  No visual stream; fp32 compute; always in eval mode
    when it encodes."""

    def __init__(self, config):
        super().__init__()
        if not isinstance(config, BertConfig):
            raise ValueError("LabelEncoder: a BertConfig is expected, got %s" % type(config).__name__)
        self.config = config
        self.embeddings = BertEmbeddings(config)
        self.encoder = _Layers(config)
        self.pooler = BertPooler(config)
        bind_root(self, compute_dtype=torch.float32)
        self.eval()

    def forward(self, input_ids, attention_mask=None):
        """input_ids int64 [B, T], attention_mask [B, T] (1: a token, 0: padding; None: all tokens) -> pooled fp32 [B, H]"""
        check_sequence_limits("LabelEncoder.forward", input_ids.shape[1], None, self.config)
        if attention_mask is None:
            attention_mask = torch.ones_like(input_ids)
        mask = (1.0 - attention_mask.unsqueeze(1).unsqueeze(2).to(torch.float32)) * -10000.0  # additive, as LXRTModel's
        h = self.embeddings(input_ids, torch.zeros_like(input_ids))
        for layer in self.encoder.layer:
            h = layer(h, mask)
        return self.pooler(h).to(torch.float32)


def _body_state(state_dict):
    """a checkpoint's keys as the encoder names them: ``gamma`` / ``beta`` -> ``weight`` / ``bias`` (the surgery of
    ``BertPreTrainedModel.from_pretrained``), a ``bert.`` prefix dropped, ``cls.*`` and ``*.position_ids`` left out"""
    out = {}
    for key, value in state_dict.items():
        k = key.replace("gamma", "weight") if "gamma" in key else key
        k = k.replace("beta", "bias") if "beta" in k else k
        if k.startswith("bert."):
            k = k[len("bert."):]
        if k.startswith(IGNORED) or k.endswith("position_ids"):
            continue
        out[k] = value
    return out


def load_label_encoder(config, checkpoint, device="cuda"):
    """``checkpoint``: a state dict, the path of a local ``pytorch_model.bin`` or of a directory that holds one ->
    ``LabelEncoder`` on ``device`` with every body tensor taken from it.  Keys may carry a ``bert.`` prefix and the old
    ``gamma`` / ``beta`` spelling of LayerNorm; ``cls.*`` and ``embeddings.position_ids`` are ignored, as is any tensor the
    encoder has no place for.  A body tensor the checkpoint lacks is refused by name (KeyError): a layer left at its random
    initialisation would give a plausible but wrong adjacency.  A name that is no local file is refused
    (FileNotFoundError): nothing is looked up on a hub."""
    if isinstance(checkpoint, (str, os.PathLike)):
        path = os.fspath(checkpoint)
        if os.path.isdir(path):
            path = os.path.join(path, "pytorch_model.bin")
        if not os.path.isfile(path):
            raise FileNotFoundError("load_label_encoder: %r is no local checkpoint file (xggm_amd runs offline: a model is never "
                                    "fetched by name)" % os.fspath(checkpoint))
        checkpoint = torch.load(path, map_location="cpu", weights_only=True)
    if not hasattr(checkpoint, "items"):
        raise TypeError("load_label_encoder: a state dict or a path is expected, got %s" % type(checkpoint).__name__)
    model = LabelEncoder(config)
    sd = _body_state(checkpoint)
    want = model.state_dict()
    missing = [k for k in want if k not in sd]
    if missing:
        raise KeyError("load_label_encoder: the checkpoint lacks %d tensor(s) of the encoder: %s" % (len(missing), ", ".join(missing)))
    for k, v in want.items():
        if tuple(sd[k].shape) != tuple(v.shape):
            raise ValueError("load_label_encoder: %s is %s in the checkpoint, the config makes it %s" % (k, tuple(sd[k].shape), tuple(v.shape)))
    model.load_state_dict({k: sd[k] for k in want}, strict=True)
    return model.to(device).eval()


def read_labels(path):
    """the lines of a vocabulary file, stripped of ``\\n`` only (``read_txt``, src/utils.py:130-133)"""
    with open(path, "r") as f:
        return [line.strip("\n") for line in f.readlines()]


def label_ids(tokenizer, label):
    """``[CLS] pieces [SEP]`` of one label as ids: what ``tokenizer.encode(sent)`` gives (compute_adjacency.py:20-25)"""
    return tokenizer.convert_tokens_to_ids(["[CLS]"] + tokenizer.tokenize(label) + ["[SEP]"])


def embed_labels(encoder, tokenizer, labels, batch=256):
    """``labels``: strings; ``tokenizer``: the package's ``BertTokenizer`` -> fp32 [V, H] on the encoder's device: row v is
    the pooled output for ``[CLS] pieces [SEP]`` of label v.  ``batch`` labels per forward, each batch padded to its
    longest row with the attention mask set.  A label with more tokens than the attention core or the position table
    takes raises ValueError (``check_sequence_limits``)."""
    if not labels:
        raise ValueError("embed_labels: no labels")
    device = next(encoder.parameters()).device
    if device.type != "cuda":
        raise RuntimeError("xggm_amd: the label encoder must live on the GPU (no CPU fallback)")
    rows = [label_ids(tokenizer, s) for s in labels]
    check_sequence_limits("embed_labels", max(len(r) for r in rows), None, encoder.config)
    encoder.eval()
    out = []
    with torch.no_grad():
        for s in range(0, len(rows), int(batch)):
            part = rows[s:s + int(batch)]
            T = max(len(r) for r in part)
            ids = torch.tensor([r + [0] * (T - len(r)) for r in part], dtype=torch.int64)
            mask = torch.tensor([[1] * len(r) + [0] * (T - len(r)) for r in part], dtype=torch.int64)
            out.append(encoder(ids.to(device), mask.to(device)))
    return torch.cat(out)


def label_tables(encoder, tokenizer, objects_vocab, attributes_vocab, batch=256):
    """the two tables of ``compute_adjacency.label_pair_table`` from ``objects_vocab.txt`` / ``attributes_vocab.txt``
    (compute_adjacency.py:66-69) -> (class_table [Vc, H], attr_table [Va, H])"""
    return (embed_labels(encoder, tokenizer, read_labels(objects_vocab), batch),
            embed_labels(encoder, tokenizer, read_labels(attributes_vocab), batch))
