"""LXMERT encoder with the reference's module tree, state_dict keys and forward signatures
(src/lxrt/modeling.py of jingjing12110/X-GGM), executed by the HIP blocks of
``xggm_amd.functional``.

The nn.Modules below only HOLD parameters under the reference's names
(``bert.encoder.layer.0.attention.self.query.weight`` ...); none of their arithmetic runs in
PyTorch.  Activations travel as 2-D [batch*seq, hidden] tensors in the compute dtype.
"""
import copy
import json
import math

import torch
import torch.nn as nn

from .. import functional as XF
from .. import ops
from ..runtime import runtime_of, bind_root

BertLayerNorm = nn.LayerNorm


class GeLU(nn.Module):
    """parameter-free marker kept so ``nn.Sequential(Linear, GeLU(), LayerNorm)`` heads have
    the reference's indices (0, 2[, 3]); the activation itself is fused into the GEMM epilogue
    (ref: src/lxrt/modeling.py:127-140)."""

    def forward(self, x):
        raise RuntimeError("GeLU is fused into the preceding Linear; call the owning head module")


class VisualConfig(object):
    """ref: src/lxrt/modeling.py:150-179"""
    VISUAL_LOSSES = ['obj', 'attr', 'feat']

    def __init__(self, l_layers=12, x_layers=5, r_layers=0):
        self.l_layers = l_layers
        self.x_layers = x_layers
        self.r_layers = r_layers
        self.visual_feat_dim = 2048
        self.visual_pos_dim = 4
        self.obj_id_num = 1600
        self.attr_id_num = 400
        self.visual_losses = self.VISUAL_LOSSES
        self.visual_loss_config = {
            'obj': (self.obj_id_num, 'ce', (-1,), 1 / 0.15),
            'attr': (self.attr_id_num, 'ce', (-1,), 1 / 0.15),
            'feat': (2048, 'l2', (-1, 2048), 1 / 0.15),
        }

    def set_visual_dims(self, feat_dim, pos_dim):
        self.visual_feat_dim = feat_dim
        self.visual_pos_dim = pos_dim


VISUAL_CONFIG = VisualConfig()


MAX_ATTENTION_ROWS = 128  # tokens of a sentence / objects of an image the attention core serves (csrc/attention_long.hip)


def check_sequence_limits(who, max_seq_length=None, n_objects=None, config=None):
    """ValueError for a sentence length or an object count the encoder cannot run: more than MAX_ATTENTION_ROWS rows on a
    side of the attention core, or more tokens than ``config``'s position table has rows.  Checked where the numbers
    become known (construction; the shapes of a forward) instead of failing inside the first launch."""
    for name, n in (("max_seq_length", max_seq_length), ("n_objects", n_objects)):
        if n is not None and not 1 <= int(n) <= MAX_ATTENTION_ROWS:
            raise ValueError("%s: %s = %d is outside 1 .. %d, the rows the attention core serves"
                             % (who, name, int(n), MAX_ATTENTION_ROWS))
    if max_seq_length is not None and config is not None and int(max_seq_length) > config.max_position_embeddings:
        raise ValueError("%s: max_seq_length = %d exceeds the position table (max_position_embeddings = %d)"
                         % (who, int(max_seq_length), config.max_position_embeddings))


class BertConfig(object):
    """ref: src/lxrt/modeling.py:182-272"""

    def __init__(self, vocab_size_or_config_json_file, hidden_size=768, num_hidden_layers=12,
                 num_attention_heads=12, intermediate_size=3072, hidden_act="gelu",
                 hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1,
                 max_position_embeddings=512, type_vocab_size=2, initializer_range=0.02):
        if isinstance(vocab_size_or_config_json_file, str):
            with open(vocab_size_or_config_json_file, "r", encoding='utf-8') as reader:
                for key, value in json.loads(reader.read()).items():
                    self.__dict__[key] = value
        elif isinstance(vocab_size_or_config_json_file, int):
            self.vocab_size = vocab_size_or_config_json_file
            self.hidden_size = hidden_size
            self.num_hidden_layers = num_hidden_layers
            self.num_attention_heads = num_attention_heads
            self.hidden_act = hidden_act
            self.intermediate_size = intermediate_size
            self.hidden_dropout_prob = hidden_dropout_prob
            self.attention_probs_dropout_prob = attention_probs_dropout_prob
            self.max_position_embeddings = max_position_embeddings
            self.type_vocab_size = type_vocab_size
            self.initializer_range = initializer_range
        else:
            raise ValueError("First argument must be either a vocabulary size (int) or the path to a "
                             "pretrained model config file (str)")
        if self.hidden_act != "gelu":
            raise NotImplementedError("only the erf-GELU of the reference scripts is implemented in HIP")

    @classmethod
    def from_dict(cls, json_object):
        config = BertConfig(vocab_size_or_config_json_file=-1)
        for key, value in json_object.items():
            config.__dict__[key] = value
        return config

    @classmethod
    def from_json_file(cls, json_file):
        with open(json_file, "r", encoding='utf-8') as reader:
            return cls.from_dict(json.loads(reader.read()))

    def to_dict(self):
        return copy.deepcopy(self.__dict__)

    def to_json_string(self):
        return json.dumps(self.to_dict(), indent=2, sort_keys=True) + "\n"


def _2d(x):
    return x if x.dim() == 2 else x.reshape(-1, x.shape[-1])


def _mask2d(mask, B, S):
    """[B,1,1,S] additive mask of the reference (or None) -> contiguous fp32 [B,S]."""
    if mask is None:
        return None
    return mask.reshape(B, S).to(torch.float32).contiguous()


class BertEmbeddings(nn.Module):
    """ref: src/lxrt/modeling.py:278-313"""

    def __init__(self, config):
        super().__init__()
        self.word_embeddings = nn.Embedding(config.vocab_size, config.hidden_size, padding_idx=0)
        self.position_embeddings = nn.Embedding(config.max_position_embeddings, config.hidden_size, padding_idx=0)
        self.token_type_embeddings = nn.Embedding(config.type_vocab_size, config.hidden_size, padding_idx=0)
        self.LayerNorm = BertLayerNorm(config.hidden_size, eps=1e-12)
        self.dropout = nn.Dropout(config.hidden_dropout_prob)

    def forward(self, input_ids, token_type_ids=None):
        rt = runtime_of(self)
        B, T = input_ids.shape
        out = XF.EmbedFn.apply(rt, self, input_ids.contiguous(),
                               None if token_type_ids is None else token_type_ids.contiguous(),
                               *self.parameters())
        return out.view(B, T, -1)


class BertAttention(nn.Module):
    """parameter holder, ref: src/lxrt/modeling.py:316-343 (its forward lives in AttnBlockFn)"""

    def __init__(self, config, ctx_dim=None):
        super().__init__()
        if config.hidden_size % config.num_attention_heads != 0:
            raise ValueError("The hidden size (%d) is not a multiple of the number of attention heads (%d)"
                             % (config.hidden_size, config.num_attention_heads))
        self.num_attention_heads = config.num_attention_heads
        self.attention_head_size = int(config.hidden_size / config.num_attention_heads)
        self.all_head_size = self.num_attention_heads * self.attention_head_size
        if self.attention_head_size != 64:
            raise NotImplementedError("the HIP attention core is built for head size 64 (got %d)"
                                      % self.attention_head_size)
        if ctx_dim is None:
            ctx_dim = config.hidden_size
        self.query = nn.Linear(config.hidden_size, self.all_head_size)
        self.key = nn.Linear(ctx_dim, self.all_head_size)
        self.value = nn.Linear(ctx_dim, self.all_head_size)
        self.dropout = nn.Dropout(config.attention_probs_dropout_prob)


class BertAttOutput(nn.Module):
    """ref: src/lxrt/modeling.py:377-388"""

    def __init__(self, config):
        super().__init__()
        self.dense = nn.Linear(config.hidden_size, config.hidden_size)
        self.LayerNorm = BertLayerNorm(config.hidden_size, eps=1e-12)
        self.dropout = nn.Dropout(config.hidden_dropout_prob)


def _attn_block(att, outm, x, ctx, mask, salt=0):
    """x [B,Sq,H]; ctx None (self) or [B,Sk,H]; mask additive broadcastable to [B,Sk] or None."""
    rt = runtime_of(att)
    B, Sq, H = x.shape
    Sk = Sq if ctx is None else ctx.shape[1]
    y = XF.AttnBlockFn.apply(rt, att, outm, _2d(x), None if ctx is None else _2d(ctx), _mask2d(mask, B, Sk), B, Sq,
                             Sk, salt, *att.parameters(), *outm.parameters())
    return y.view(B, Sq, H)


class BertCrossattLayer(nn.Module):
    """ref: src/lxrt/modeling.py:391-400"""

    def __init__(self, config):
        super().__init__()
        self.att = BertAttention(config)
        self.output = BertAttOutput(config)

    def forward(self, input_tensor, ctx_tensor, ctx_att_mask=None, salt=1):
        return _attn_block(self.att, self.output, input_tensor, ctx_tensor, ctx_att_mask, salt)


class BertSelfattLayer(nn.Module):
    """ref: src/lxrt/modeling.py:403-414"""

    def __init__(self, config):
        super().__init__()
        self.self = BertAttention(config)
        self.output = BertAttOutput(config)

    def forward(self, input_tensor, attention_mask):
        return _attn_block(self.self, self.output, input_tensor, None, attention_mask)


class BertIntermediate(nn.Module):
    """ref: src/lxrt/modeling.py:417-431"""

    def __init__(self, config):
        super().__init__()
        self.dense = nn.Linear(config.hidden_size, config.intermediate_size)


class BertOutput(nn.Module):
    """ref: src/lxrt/modeling.py:434-445"""

    def __init__(self, config):
        super().__init__()
        self.dense = nn.Linear(config.intermediate_size, config.hidden_size)
        self.LayerNorm = BertLayerNorm(config.hidden_size, eps=1e-12)
        self.dropout = nn.Dropout(config.hidden_dropout_prob)


def _ffn_block(inter, outm, x):
    rt = runtime_of(inter)
    shape = x.shape
    y = XF.FFNFn.apply(rt, inter, outm, _2d(x), *inter.parameters(), *outm.parameters())
    return y.view(shape)


def _pair(kind, mods, lang, visn, lang_mask, params):
    """run the language and the vision side of one layer in lockstep (functional.PairFn)."""
    rt = runtime_of(mods[0] if kind == "cross" else mods[0][0])
    B, T, H = lang.shape
    N = visn.shape[1]
    y_l, y_v = XF.PairFn.apply(rt, kind, mods, _2d(lang), _2d(visn), _mask2d(lang_mask, B, T), B, T, N, *params)
    return y_l.view(B, T, H), y_v.view(B, N, H)


def bert_layer_pair(layer_l, layer_v, lang, lang_mask, visn, visn_mask):
    """BertLayer on the language stream and BertLayer on the vision stream, independent of each
    other (src/lxrt/modeling.py:593-598), executed together so their GEMMs share launches."""
    if visn_mask is not None:  # not used by any trainer; keep the plain path for it
        return layer_l(lang, lang_mask), layer_v(visn, visn_mask)
    al, av = layer_l.attention, layer_v.attention
    lang, visn = _pair("self", ((al.self, al.output), (av.self, av.output)), lang, visn, lang_mask,
                       [*al.parameters(), *av.parameters()])
    return _pair("ffn", ((layer_l.intermediate, layer_l.output), (layer_v.intermediate, layer_v.output)), lang, visn,
                 None, [*layer_l.intermediate.parameters(), *layer_l.output.parameters(),
                        *layer_v.intermediate.parameters(), *layer_v.output.parameters()])


class BertLayer(nn.Module):
    """ref: src/lxrt/modeling.py:448-459"""

    def __init__(self, config):
        super().__init__()
        self.attention = BertSelfattLayer(config)
        self.intermediate = BertIntermediate(config)
        self.output = BertOutput(config)

    def forward(self, hidden_states, attention_mask):
        attention_output = self.attention(hidden_states, attention_mask)
        return _ffn_block(self.intermediate, self.output, attention_output)


class LXRTXLayer(nn.Module):
    """ref: src/lxrt/modeling.py:469-527"""

    def __init__(self, config):
        super().__init__()
        self.visual_attention = BertCrossattLayer(config)
        self.lang_self_att = BertSelfattLayer(config)
        self.visn_self_att = BertSelfattLayer(config)
        self.lang_inter = BertIntermediate(config)
        self.lang_output = BertOutput(config)
        self.visn_inter = BertIntermediate(config)
        self.visn_output = BertOutput(config)

    def cross_att(self, lang_input, lang_attention_mask, visn_input, visn_attention_mask):
        lang_att_output = self.visual_attention(lang_input, visn_input, ctx_att_mask=visn_attention_mask, salt=1)
        visn_att_output = self.visual_attention(visn_input, lang_input, ctx_att_mask=lang_attention_mask, salt=2)
        return lang_att_output, visn_att_output

    def self_att(self, lang_input, lang_attention_mask, visn_input, visn_attention_mask):
        return (self.lang_self_att(lang_input, lang_attention_mask),
                self.visn_self_att(visn_input, visn_attention_mask))

    def output_fc(self, lang_input, visn_input):
        return (_ffn_block(self.lang_inter, self.lang_output, lang_input),
                _ffn_block(self.visn_inter, self.visn_output, visn_input))

    def forward(self, lang_feats, lang_attention_mask, visn_feats, visn_attention_mask):
        if visn_attention_mask is not None:  # unused by the trainers: unpaired path
            lang_att_output, visn_att_output = self.cross_att(lang_feats, lang_attention_mask, visn_feats,
                                                              visn_attention_mask)
            lang_att_output, visn_att_output = self.self_att(lang_att_output, lang_attention_mask, visn_att_output,
                                                             visn_attention_mask)
            return self.output_fc(lang_att_output, visn_att_output)
        va = self.visual_attention
        lang, visn = _pair("cross", (va.att, va.output), lang_feats, visn_feats, lang_attention_mask,
                           list(va.parameters()))
        ls, vs = self.lang_self_att, self.visn_self_att
        lang, visn = _pair("self", ((ls.self, ls.output), (vs.self, vs.output)), lang, visn, lang_attention_mask,
                           [*ls.parameters(), *vs.parameters()])
        return _pair("ffn", ((self.lang_inter, self.lang_output), (self.visn_inter, self.visn_output)), lang, visn,
                     None, [*self.lang_inter.parameters(), *self.lang_output.parameters(),
                            *self.visn_inter.parameters(), *self.visn_output.parameters()])


class VisualFeatEncoder(nn.Module):
    """ref: src/lxrt/modeling.py:530-556"""

    def __init__(self, config):
        super().__init__()
        feat_dim = VISUAL_CONFIG.visual_feat_dim
        pos_dim = VISUAL_CONFIG.visual_pos_dim
        if pos_dim != 4:
            raise NotImplementedError("the HIP visual embedding is built for 4-d boxes")
        self.visn_fc = nn.Linear(feat_dim, config.hidden_size)
        self.visn_layer_norm = BertLayerNorm(config.hidden_size, eps=1e-12)
        self.box_fc = nn.Linear(pos_dim, config.hidden_size)
        self.box_layer_norm = BertLayerNorm(config.hidden_size, eps=1e-12)
        self.dropout = nn.Dropout(config.hidden_dropout_prob)

    def forward(self, visn_input):
        feats, boxes = visn_input
        rt = runtime_of(self)
        B, N, F = feats.shape
        dt = rt.arena.compute_dtype
        f2 = feats.reshape(B * N, F)
        b2 = boxes.reshape(B * N, 4)
        f2 = ops.cast_from_f32(f2.contiguous(), dt) if f2.dtype == torch.float32 else f2.contiguous()
        b2 = ops.cast_from_f32(b2.contiguous(), dt) if b2.dtype == torch.float32 else b2.contiguous()
        out = XF.VisnEmbedFn.apply(rt, self, f2, b2, *self.parameters())
        return out.view(B, N, -1)


class LXRTEncoder(nn.Module):
    """ref: src/lxrt/modeling.py:559-605"""

    def __init__(self, config):
        super().__init__()
        self.visn_fc = VisualFeatEncoder(config)
        self.num_l_layers = VISUAL_CONFIG.l_layers
        self.num_x_layers = VISUAL_CONFIG.x_layers
        self.num_r_layers = VISUAL_CONFIG.r_layers
        print("LXRT encoder with %d l_layers, %d x_layers, and %d r_layers."
              % (self.num_l_layers, self.num_x_layers, self.num_r_layers))
        self.layer = nn.ModuleList([BertLayer(config) for _ in range(self.num_l_layers)])
        self.x_layers = nn.ModuleList([LXRTXLayer(config) for _ in range(self.num_x_layers)])
        self.r_layers = nn.ModuleList([BertLayer(config) for _ in range(self.num_r_layers)])

    def forward(self, lang_feats, lang_attention_mask, visn_feats, visn_attention_mask=None):
        visn_feats = self.visn_fc(visn_feats)
        # language layers and relational (vision) layers are independent chains: the first
        # min(l, r) layers of both run pairwise in lockstep, the rest alone
        n_pair = min(self.num_l_layers, self.num_r_layers)
        # data-parallel overlap: the autograd graph is cut at up to four places so the backward runs in stages
        # and the gradients above a cut go on the wire while the stage below it computes (Runtime.backward,
        # dist.stage_ranges).  Positions: right above the embeddings / visual-feature encoder (their tables and
        # the vector region are the only gradients that are final last: the exposed tail of the exchange), after
        # the first two layer pairs, before the first and before the second-to-last cross-modality layer.
        rt = runtime_of(self)
        cutting = rt.cut_enabled and torch.is_grad_enabled()
        pair_cut = 2 if n_pair >= 4 else None
        x_mid = self.num_x_layers - 2 if self.num_x_layers >= 4 else None
        emb_cut = bool(cutting and lang_feats.requires_grad and visn_feats.requires_grad)
        rt.cut_layout = dict(pair_cut=pair_cut, x_mid=x_mid, emb_cut=emb_cut)
        rt._cuts = []  # cuts of an earlier forward that never saw its backward are dropped

        def cut(tag, a, b):
            if cutting and a.requires_grad and b.requires_grad:
                return rt.make_cut(tag, a, b)
            return a, b

        if emb_cut:
            lang_feats, visn_feats = cut("emb", lang_feats, visn_feats)

        for i in range(n_pair):
            if i == pair_cut:
                lang_feats, visn_feats = cut("lower", lang_feats, visn_feats)
            lang_feats, visn_feats = bert_layer_pair(self.layer[i], self.r_layers[i], lang_feats,
                                                     lang_attention_mask, visn_feats, visn_attention_mask)
        for layer_module in self.layer[n_pair:]:
            lang_feats = layer_module(lang_feats, lang_attention_mask)
        for layer_module in self.r_layers[n_pair:]:
            visn_feats = layer_module(visn_feats, visn_attention_mask)
        lang_feats, visn_feats = cut("x0", lang_feats, visn_feats)
        for k, layer_module in enumerate(self.x_layers):
            if k == x_mid:
                lang_feats, visn_feats = cut("xmid", lang_feats, visn_feats)
            lang_feats, visn_feats = layer_module(lang_feats, lang_attention_mask, visn_feats, visn_attention_mask)
        return lang_feats, visn_feats


class BertPooler(nn.Module):
    """ref: src/lxrt/modeling.py:608-620"""

    def __init__(self, config):
        super().__init__()
        self.dense = nn.Linear(config.hidden_size, config.hidden_size)
        self.activation = nn.Tanh()

    def forward(self, hidden_states):
        rt = runtime_of(self)
        first_token_tensor = XF.FirstTokenFn.apply(hidden_states)  # hidden_states[:, 0]: strided rows, read in place
        return XF.LinearActFn.apply(rt, self.dense, first_token_tensor, ops.ACT_TANH, False, *self.dense.parameters())


class BertPreTrainedModel(nn.Module):
    """ref: src/lxrt/modeling.py:717-747.  ``from_pretrained`` of the reference downloads
    ``bert-base-uncased`` from S3; offline it can only read a local directory / state dict."""

    def __init__(self, config, *inputs, **kwargs):
        super().__init__()
        if not isinstance(config, BertConfig):
            raise ValueError("Parameter config in `{}(config)` should be an instance of class `BertConfig`."
                             .format(self.__class__.__name__))
        self.config = config

    def init_bert_weights(self, module):
        if isinstance(module, (nn.Linear, nn.Embedding)):
            module.weight.data.normal_(mean=0.0, std=self.config.initializer_range)
        elif isinstance(module, BertLayerNorm):
            module.bias.data.zero_()
            module.weight.data.fill_(1.0)
        if isinstance(module, nn.Linear) and module.bias is not None:
            module.bias.data.zero_()

    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path, state_dict=None, cache_dir=None, from_tf=False,
                        *inputs, **kwargs):
        import os
        if not os.path.isdir(str(pretrained_model_name_or_path)):
            raise FileNotFoundError(
                "xggm_amd runs offline: '%s' is not a local directory holding bert_config.json "
                "(+ pytorch_model.bin).  Build the model from a BertConfig instead."
                % pretrained_model_name_or_path)
        config = BertConfig.from_json_file(os.path.join(pretrained_model_name_or_path, "bert_config.json"))
        model = cls(config, *inputs, **kwargs)
        weights = os.path.join(pretrained_model_name_or_path, "pytorch_model.bin")
        if state_dict is None and os.path.exists(weights):
            state_dict = torch.load(weights, map_location="cpu", weights_only=True)
        if state_dict is not None:
            sd = {}
            for key, value in state_dict.items():  # same key surgery as modeling.py:848-858
                new_key = key.replace('gamma', 'weight') if 'gamma' in key else key
                new_key = new_key.replace('beta', 'bias') if 'beta' in new_key else new_key
                sd[new_key] = value
            prefix = '' if any(k.startswith('bert.') for k in sd) or not hasattr(model, 'bert') else 'bert.'
            missing, unexpected = model.load_state_dict({prefix + k: v for k, v in sd.items()}, strict=False)
            if missing:
                print("Weights of {} not initialized from pretrained model: {}".format(cls.__name__, missing))
        return model


class LXRTModel(BertPreTrainedModel):
    """ref: src/lxrt/modeling.py:894-952"""

    def __init__(self, config):
        super().__init__(config)
        self.embeddings = BertEmbeddings(config)
        self.encoder = LXRTEncoder(config)
        self.pooler = BertPooler(config)
        self.apply(self.init_bert_weights)

    def forward(self, input_ids, token_type_ids=None, attention_mask=None, visual_feats=None,
                visual_attention_mask=None):
        check_sequence_limits("LXRTModel.forward", input_ids.shape[1],
                              visual_feats[0].shape[1] if visual_feats is not None else None, self.config)
        if attention_mask is None:
            attention_mask = torch.ones_like(input_ids)
        if token_type_ids is None:
            token_type_ids = torch.zeros_like(input_ids)
        # additive masks (1 - m) * -10000, [B,1,1,S] as in the reference (:919-939)
        rt = runtime_of(self)
        side = []  # input glue done by workgroups appended to the embedding kernel's launch (ops.embed_fwd, side=)
        if attention_mask.is_cuda and attention_mask.dtype == torch.int64 and attention_mask.is_contiguous():
            # the reference's cast / subtract / multiply
            m = torch.empty(attention_mask.shape, device=attention_mask.device, dtype=torch.float32)
            side.append((ops.SIDE_ADDITIVE_MASK, attention_mask, m))
            extended_attention_mask = m.unsqueeze(1).unsqueeze(2)
        else:
            extended_attention_mask = (1.0 - attention_mask.unsqueeze(1).unsqueeze(2).to(torch.float32)) * -10000.0
        if visual_attention_mask is not None:
            extended_visual_attention_mask = (1.0 - visual_attention_mask.unsqueeze(1).unsqueeze(2).to(
                torch.float32)) * -10000.0
        else:
            extended_visual_attention_mask = None
        # fp8 forward: the producers' e4m3 copies of THIS forward start here -- in front of the embeddings, whose kernels
        # write the first two (begun inside the encoder, as it was, the registry was cleared right after they had
        # registered, and both streams of every pass went through the stand-alone quantiser)
        if rt.arena.fp8 is not None:
            rt.arena.fp8.begin_forward()
        if visual_feats is not None and rt.arena.compute_dtype == torch.bfloat16:
            # fp32 visual features / boxes: their bf16 copies (VisualFeatEncoder.forward) ride along too
            cast = []
            for t in visual_feats:
                if t.is_cuda and t.dtype == torch.float32 and len(side) < ops.SIDE_MAX:
                    t = t.contiguous()
                    c = torch.empty(t.shape, device=t.device, dtype=torch.bfloat16)
                    side.append((ops.SIDE_CAST_BF16, t, c))
                    t = c
                cast.append(t)
            visual_feats = tuple(cast)
        rt.side_jobs = side or None
        embedding_output = self.embeddings(input_ids, token_type_ids)
        if rt.side_jobs:  # an embedding module that does not take them along: launches of their own
            ops.run_side_jobs(rt.side_jobs)
            rt.side_jobs = None
        lang_feats, visn_feats = self.encoder(embedding_output, extended_attention_mask, visn_feats=visual_feats,
                                              visn_attention_mask=extended_visual_attention_mask)
        pooled_output = self.pooler(lang_feats)
        return (lang_feats, visn_feats), pooled_output


class BertPredictionHeadTransform(nn.Module):
    """ref: src/lxrt/modeling.py:623-639 (dense, GELU, LayerNorm): one fused block"""

    def __init__(self, config):
        super().__init__()
        self.dense = nn.Linear(config.hidden_size, config.hidden_size)
        self.transform_act_fn = GeLU()
        self.LayerNorm = BertLayerNorm(config.hidden_size, eps=1e-12)

    def forward(self, hidden_states):
        rt = runtime_of(self)
        return XF.MLPFn.apply(rt, self.dense, self.LayerNorm, 1e-12, hidden_states, *self.dense.parameters(),
                              *self.LayerNorm.parameters())


class _TiedLinear:
    """the decoder's weight with the head's own bias, as LinearActFn reads a Linear"""

    def __init__(self, weight, bias):
        self.weight, self.bias = weight, bias


class BertLMPredictionHead(nn.Module):
    """ref: src/lxrt/modeling.py:642-659.  ``decoder.weight`` IS the word-embedding table.  ``forward`` gives the scores of
    every row, as the reference does; training goes through ``masked_lm_loss``, which never forms them."""

    def __init__(self, config, bert_model_embedding_weights):
        super().__init__()
        self.transform = BertPredictionHeadTransform(config)
        self.decoder = nn.Linear(bert_model_embedding_weights.size(1), bert_model_embedding_weights.size(0), bias=False)
        self.decoder.weight = bert_model_embedding_weights
        self.bias = nn.Parameter(torch.zeros(bert_model_embedding_weights.size(0)))

    def forward(self, hidden_states):
        rt = runtime_of(self)
        h = self.transform(hidden_states)
        return XF.LinearActFn.apply(rt, _TiedLinear(self.decoder.weight, self.bias), h, ops.ACT_NONE, True,
                                    self.decoder.weight, self.bias)

    def masked_lm_loss(self, hidden_states, masked_lm_labels, mlm_capacity=None, overflow=None):
        """CrossEntropyLoss(ignore_index=-1) of the scores against the labels (:1009-1016) over the rows that carry a
        label only: select -> transform -> tied decoder -> loss, all on ``mlm_capacity`` compacted rows"""
        from .. import pretrain_heads as PH
        rt = runtime_of(self)
        M = masked_lm_labels.numel()
        holder = XF.Holder()
        rows = XF.MlmSelectFn.apply(hidden_states, masked_lm_labels, PH.mlm_capacity(M, mlm_capacity),
                                    self.decoder.weight.shape[0], overflow, holder)
        t = self.transform(rows)
        return XF.MlmDecoderFn.apply(rt, self, holder, t, rt.scalar_slot(), self.decoder.weight, self.bias)


class BertVisualAnswerHead(nn.Module):
    """ref: src/lxrt/modeling.py:662-674"""

    def __init__(self, config, num_answers):
        super().__init__()
        hid_dim = config.hidden_size
        self.logit_fc = nn.Sequential(nn.Linear(hid_dim, hid_dim * 2), GeLU(), BertLayerNorm(hid_dim * 2, eps=1e-12),
                                      nn.Linear(hid_dim * 2, num_answers))

    def forward(self, hidden_states):
        rt = runtime_of(self)
        fc = self.logit_fc
        y = XF.MLPFn.apply(rt, fc[0], fc[2], 1e-12, hidden_states, *fc[0].parameters(), *fc[2].parameters())
        return XF.LinearActFn.apply(rt, fc[3], y, ops.ACT_NONE, True, *fc[3].parameters())


class BertVisualObjHead(nn.Module):
    """ref: src/lxrt/modeling.py:677-701"""

    def __init__(self, config, visual_losses):
        super().__init__()
        self.transform = BertPredictionHeadTransform(config)
        visual_losses = visual_losses.split(",")
        for loss in visual_losses:
            assert loss in VISUAL_CONFIG.VISUAL_LOSSES
        self.visual_losses = visual_losses
        self.decoder_dict = nn.ModuleDict({key: nn.Linear(config.hidden_size, VISUAL_CONFIG.visual_loss_config[key][0])
                                           for key in self.visual_losses})

    def forward(self, hidden_states):
        rt = runtime_of(self)
        hs = XF.fan_out(self.transform(hidden_states), len(self.visual_losses))
        return {key: XF.LinearActFn.apply(rt, self.decoder_dict[key], h, ops.ACT_NONE, False,
                                          *self.decoder_dict[key].parameters())
                for key, h in zip(self.visual_losses, hs)}


class BertPreTrainingHeads(nn.Module):
    """ref: src/lxrt/modeling.py:704-714"""

    def __init__(self, config, bert_model_embedding_weights):
        super().__init__()
        self.predictions = BertLMPredictionHead(config, bert_model_embedding_weights)
        self.seq_relationship = nn.Linear(config.hidden_size, 2)

    def relationship(self, pooled_output):
        rt = runtime_of(self)
        return XF.LinearActFn.apply(rt, self.seq_relationship, pooled_output, ops.ACT_NONE, True,
                                    *self.seq_relationship.parameters())

    def forward(self, sequence_output, pooled_output):
        return self.predictions(sequence_output), self.relationship(pooled_output)


class LXRTPretraining(BertPreTrainedModel):
    """ref: src/lxrt/modeling.py:955-1061.  ``mlm_capacity``: slots of the compacted masked-LM rows -- None = B T (can
    never overflow), an int fixes them; more labelled rows than slots raise the device flag ``mlm_overflow`` and make
    the masked-LM loss NaN.  The word table's gradient is dense here (the decoder's share), so the arena's row-sparse
    bookkeeping of it is switched off."""

    def __init__(self, config, task_mask_lm=True, task_matched=True, task_obj_predict=True, visual_losses='',
                 task_qa=True, num_answers=2, mlm_capacity=None, compute_dtype=None):
        super().__init__(config)
        self.config = config
        self.num_answers = num_answers
        self.task_mask_lm = task_mask_lm
        self.task_obj_predict = task_obj_predict
        self.task_matched = task_matched
        self.task_qa = task_qa
        self.mlm_capacity = mlm_capacity
        self.mlm_overflow = None
        self.bert = LXRTModel(config)
        self.cls = BertPreTrainingHeads(config, self.bert.embeddings.word_embeddings.weight)
        if self.task_obj_predict:
            self.obj_predict_head = BertVisualObjHead(config, visual_losses)
        if self.task_qa:
            self.answer_head = BertVisualAnswerHead(config, self.num_answers)
        self.apply(self.init_bert_weights)
        bind_root(self, compute_dtype)

    def forward(self, input_ids, token_type_ids=None, attention_mask=None, masked_lm_labels=None, visual_feats=None,
                pos=None, obj_labels=None, matched_label=None, ans=None):
        rt = runtime_of(self)
        rt.arena.row_list_enabled = False
        dev = input_ids.device
        if self.mlm_overflow is None or self.mlm_overflow.device != dev:
            self.mlm_overflow = torch.zeros(1, device=dev, dtype=torch.int32)
        (lang_output, visn_output), pooled_output = self.bert(input_ids, token_type_ids, attention_mask,
                                                              visual_feats=(visual_feats, pos))
        p_rel, p_qa = XF.fan_out(pooled_output, 2)
        if self.task_qa:
            answer_score = self.answer_head(p_qa)
        else:
            answer_score = pooled_output[0][0]
        rt.begin_losses(4)
        ce = lambda z, y: XF.SoftmaxLossFn.apply(ops.SOFTMAX_CE, z, y.view(-1), None, None, -1, 1.0, rt.scalar_slot())
        terms, losses = [], ()
        if masked_lm_labels is not None and self.task_mask_lm:
            l = self.cls.predictions.masked_lm_loss(lang_output, masked_lm_labels, self.mlm_capacity, self.mlm_overflow)
            terms.append(l)
            losses += (l.detach(),)
        if matched_label is not None and self.task_matched:
            l = ce(self.cls.relationship(p_rel).view(-1, 2), matched_label)
            terms.append(l)
            losses += (l.detach(),)
        if obj_labels is not None and self.task_obj_predict:
            scores = self.obj_predict_head(visn_output)
            kinds = {'ce': ops.VISUAL_CE, 'l2': ops.VISUAL_L2}
            spec, ss, ls, cs = [], [], [], []
            for key in VISUAL_CONFIG.visual_losses:
                label, mask_conf = obj_labels[key]
                output_dim, loss_fct_name, label_shape, weight = VISUAL_CONFIG.visual_loss_config[key]
                spec.append((kinds[loss_fct_name], weight))
                ss.append(scores[key].view(-1, output_dim))
                ls.append(label.view(*label_shape) if loss_fct_name == 'ce' else label.view(*label_shape).float())
                cs.append(mask_conf.view(-1).float())
            holder = XF.Holder()
            terms.append(XF.VisualLossFn.apply(holder, spec, -1, *ss, *ls, *cs))
            losses += tuple(holder.losses[q].detach() for q in range(len(spec)))
        if ans is not None and self.task_qa:
            l = ce(answer_score.view(-1, self.num_answers), ans)
            terms.append(l)
            losses += (l.detach(),)
        total_loss = XF.LossSumFn.apply(*terms) if len(terms) > 1 else terms[0]
        return total_loss, torch.stack(losses).unsqueeze(0), answer_score.detach()


class LXRTFeatureExtraction(BertPreTrainedModel):
    """ref: src/lxrt/modeling.py:1064-1093"""

    def __init__(self, config, mode='lxr'):
        super().__init__(config)
        self.bert = LXRTModel(config)
        self.mode = mode
        self.apply(self.init_bert_weights)
        bind_root(self)

    def forward(self, input_ids, token_type_ids=None, attention_mask=None, visual_feats=None,
                visual_attention_mask=None):
        feat_seq, pooled_output = self.bert(input_ids, token_type_ids, attention_mask, visual_feats=visual_feats,
                                            visual_attention_mask=visual_attention_mask)
        if 'x' == self.mode:
            return pooled_output
        elif 'x' in self.mode and ('l' in self.mode or 'r' in self.mode):
            return feat_seq, pooled_output
        elif 'l' in self.mode or 'r' in self.mode:
            return feat_seq


VisualBertForLXRFeature = LXRTFeatureExtraction  # name used by src/lxrt/entry.py:26
