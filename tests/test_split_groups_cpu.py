"""``split_groups`` without a GPU: the id map of the mapped update, the grouping helper of ``make_optimizer``, the new
symbols with the argument checks that run before any launch, and the constructor keyword."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import shapes
from xggm_amd import _lib, arena, optim as xo
from xggm_amd.lxrt.optimization import BertAdam
from xggm_amd.vqa.vqacpv2 import NO_DECAY, param_depth, split_param_names

CLASSES = [BertAdam, xo.Adam, xo.AdamW, xo.Adamax, xo.SGD, xo.RMSprop]


# ------------------------------------------------------------------------------------------------------------------ id map
def test_id_map_on_a_hand_made_layout():
    """8-aligned starts; a tensor of 1 element; one with numel % 4 != 0 followed by a gap; a 256-aligned matrix; a
    parameter owned by no group.  Every element of every tensor carries its owner's id, the unowned one 0; one byte per 8
    elements of the arena."""
    info = {  # name: (offset, numel, group, atomic)
        "mat": (0, 300, "g", False),        # 256-aligned matrix, ends inside a chunk: gap up to 512
        "mat2": (512, 256, "g", False),
        "one": (768, 1, "g", True),         # 1 element, then 7 of gap
        "odd": (776, 13, "g", True),        # numel % 4 != 0, gap of 3 up to 792 ...
        "free": (800, 24, "g", True),       # ... and a whole id of gap (792 .. 800) in front of an unowned tensor
        "last": (824, 10, "h", True),
    }
    total = 1024
    owner = {"mat": 1, "mat2": 2, "one": 3, "odd": 1, "last": 2}  # "free" is in no param_group
    ids = arena.hyper_id_map(info, owner, total)
    assert ids.dtype == np.uint8 and ids.shape == (total // 8,) and ids.nbytes * 8 == total  # 1/8 byte per parameter
    per_elem = np.repeat(ids, 8)
    for name, (o, k, _, _) in info.items():
        assert (per_elem[o:o + k] == owner.get(name, 0)).all(), name
    # gaps carry the id of the tensor in front of them (they hold zeros: any id would do)
    assert (per_elem[300:512] == 1).all() and (per_elem[769:776] == 3).all() and (per_elem[789:800] == 1).all()
    assert (per_elem[834:] == 2).all()
    # a total that is no multiple of 8 still gets its last, partial id
    assert arena.hyper_id_map({"a": (0, 3, "g", True)}, {"a": 1}, 3).tolist() == [1]


def test_id_map_refuses_what_it_cannot_hold():
    info = {"a": (0, 8, "g", True), "b": (8, 8, "g", True)}
    assert arena.hyper_id_map(info, {"a": 255, "b": 1}, 16).tolist() == [255, 1]
    with pytest.raises(ValueError, match="param_groups"):
        arena.hyper_id_map(info, {"a": 256, "b": 1}, 16)
    with pytest.raises(ValueError, match="misaligned"):
        arena.hyper_id_map({"a": (4, 8, "g", True)}, {"a": 1}, 16)
    with pytest.raises(ValueError, match="overlaps"):
        arena.hyper_id_map({"a": (0, 9, "g", True), "b": (8, 8, "g", True)}, {"a": 1, "b": 1}, 16)


def test_id_map_of_a_real_layout_matches_the_layout():
    """the layout of the tiny model's names (arena.layout on shapes alone): tensors of different owners never share an id"""
    class P:
        def __init__(self, shape):
            self.shape = shape

        def dim(self):
            return len(self.shape)

        def numel(self):
            return int(np.prod(self.shape))

    named = [(n, P(s)) for n, s in shapes.model_shapes(shapes.TINY, 29).items()]
    _, groups, info, total = arena.layout(named, arena.default_group_of)
    owner = {n: (1 if n.endswith("bias") else 2) for n, _ in named}
    ids = np.repeat(arena.hyper_id_map(info, owner, total), 8)
    assert all((ids[o:o + k] == owner[n]).all() for n, (o, k, _, _) in info.items())
    assert all(o % 8 == 0 for o, _, _, _ in info.values()) and all(G.start % 8 == 0 for G in groups.values())


# --------------------------------------------------------------------------------------------------------- grouping helper
FULL_NAMES = list(shapes.model_shapes(shapes.FULL, 3129))  # 9 / 5 / 5


def test_depths_of_a_9_5_5_model():
    enc = shapes.ENC
    d = lambda n: param_depth(n, 9, 5, 5)  # noqa: E731
    assert d(enc + "embeddings.word_embeddings.weight") == 0 and d(enc + "embeddings.LayerNorm.bias") == 0
    assert d(enc + "encoder.visn_fc.box_fc.weight") == 0 and d(enc + "encoder.visn_fc.visn_layer_norm.weight") == 0
    for i in range(9):
        assert d(enc + "encoder.layer.%d.attention.self.query.weight" % i) == i + 1
    for i in range(5):
        assert d(enc + "encoder.r_layers.%d.output.dense.bias" % i) == i + 5      # the towers end level at 9
        assert d(enc + "encoder.x_layers.%d.visn_output.LayerNorm.weight" % i) == 10 + i
    assert d(enc + "pooler.dense.weight") == 15
    for n in ("logit_fc.0.weight", "generator.gnn_layers.0.gnn_layers.1.ctx_layer.weight", "encoder_adj.0.bias",
              "node_fc.2.weight", "fusion_fc.0.bias"):
        assert d(n) == 15
    assert sorted({d(n) for n in FULL_NAMES}) == list(range(16))
    # a language tower shorter than the visual one is the one that is shifted
    assert param_depth(enc + "encoder.layer.0.output.dense.bias", 2, 2, 3) == 2
    assert param_depth(enc + "encoder.r_layers.0.output.dense.bias", 2, 2, 3) == 1
    assert param_depth(enc + "encoder.x_layers.1.lang_inter.dense.bias", 2, 2, 3) == 5
    assert param_depth("logit_fc.3.bias", 2, 2, 3) == 6


def test_every_name_lands_in_exactly_one_group():
    lr, dcy = 5e-5, 0.9
    groups = split_param_names(FULL_NAMES, lr, NO_DECAY, dcy, 9, 5, 5)
    flat = [n for g in groups for n in g["names"]]
    assert sorted(flat) == sorted(FULL_NAMES) and len(flat) == len(set(flat))
    assert len(groups) <= 255
    for g in groups:
        nd = [any(s in n for s in NO_DECAY) for n in g["names"]]
        assert all(nd) or not any(nd)
        assert (g.get("weight_decay") == 0.0) if nd[0] else ("weight_decay" not in g)
        depths = {param_depth(n, 9, 5, 5) for n in g["names"]}
        encs = {n.startswith("lxrt_encoder.") for n in g["names"]}
        assert len(depths) == 1 and len(encs) == 1
        base = lr if encs.pop() else 4 * lr
        assert g["lr"] == pytest.approx(base * dcy ** (15 - depths.pop()), rel=1e-12)
        # named_parameters() order is kept inside a group
        pos = [FULL_NAMES.index(n) for n in g["names"]]
        assert pos == sorted(pos)


def test_no_decay_names_are_the_biases_and_every_layernorm_weight():
    """the LayerNorm weights by the structure of the state_dict (shapes._ln): a 1-D ``weight`` with a ``bias`` twin"""
    sh = shapes.model_shapes(shapes.FULL, 3129)
    for gnn in ("GIN", "GAT"):
        sh.update(shapes.generator_shapes(gnn, 768, 2))
    ln_w = {n for n, s in sh.items() if n.endswith(".weight") and len(s) == 1}
    bias = {n for n in sh if n.endswith("bias")}
    groups = split_param_names(list(sh), 1e-4, NO_DECAY, None, 9, 5, 5)
    got = {n for g in groups if g.get("weight_decay") == 0.0 for n in g["names"]}
    assert got == ln_w | bias
    assert len(groups) == 4 and sorted(g["lr"] for g in groups) == [1e-4, 1e-4, 4e-4, 4e-4]
    # the plain BERT list misses the heads' and generators' LayerNorms (Sequential item 2): why NO_DECAY has ".2.weight"
    bert = ("bias", "LayerNorm.weight", "layer_norm.weight")
    missed = (ln_w | bias) - {n for n in sh if any(s in n for s in bert)}
    assert missed and all(n.endswith(".2.weight") for n in missed)


def test_none_none_gives_the_two_groups_of_today():
    groups = split_param_names(FULL_NAMES, 5e-5, None, None, 9, 5, 5)
    assert len(groups) == 2 and all("weight_decay" not in g for g in groups)
    head, enc = groups
    assert head["lr"] == 4 * 5e-5 and enc["lr"] == 5e-5
    assert head["names"] == [n for n in FULL_NAMES if not n.startswith("lxrt_encoder.")]
    assert enc["names"] == [n for n in FULL_NAMES if n.startswith("lxrt_encoder.")]


# --------------------------------------------------------------------------------------------------------------------- ABI
def _fake_map(ids=0x1000, n_ids=4, table=0x2000, n_table=2):
    from xggm_amd import ops
    return ops.HyperMap(ids, n_ids, table, n_table)


def test_new_symbols_are_declared_and_exported():
    decl = _lib.parse_header()
    name = "xggm_optim_multi"  # the map is an argument of the one update entry
    assert name in decl and hasattr(_lib.lib, name) and len(decl[name]) == 4
    assert "xggm_hyper_map" in open(_lib.HEADER_PATH).read()
    assert _lib.lib.xggm_version() == 100


def test_struct_mirrors_keep_their_layout():
    from xggm_amd import ops
    assert ctypes.sizeof(ops.HyperMap) == 32 and ops.HyperMap.table.offset == 16 and ops.HyperMap.n_table.offset == 24
    assert ctypes.sizeof(ops.OptimArgs) == ctypes.sizeof(ops.AdamArgs) + 64  # the span structs are the ones they were
    assert ops.HYPER_MAP_ELEMS == arena.ALIGN and ops.HYPER_MAP_MAX_ID == arena.HYPER_MAX_ID


@pytest.mark.parametrize("rule", ["bertadam", "adam"])
def test_argument_checks_come_before_any_launch(rule):
    """no GPU here: every call below has to return non-zero with a message from the host-side checks"""
    from xggm_amd import ops
    fn = _lib.lib.xggm_optim_multi
    arr = (ops.OptimArgs * 1)()
    arr[0].rule = ops.RULES[rule]
    span = arr[0].a
    pa, ok = ctypes.cast(arr, ctypes.c_void_p), _fake_map()
    # (no map is the unmapped update: the span itself is looked at)
    assert fn(pa, 1, None, None) != 0 and "bad arguments" in _lib.last_error()
    assert fn(None, 1, ctypes.byref(ok), None) != 0 and "no spans" in _lib.last_error()
    assert fn(pa, 1, ctypes.byref(_fake_map(ids=None)), None) != 0 and "id map" in _lib.last_error()
    assert fn(pa, 1, ctypes.byref(_fake_map(table=None)), None) != 0 and "table" in _lib.last_error()
    assert fn(pa, 1, ctypes.byref(_fake_map(n_table=0)), None) != 0 and "0 entries" in _lib.last_error()
    assert fn(pa, 1, ctypes.byref(_fake_map(n_table=257)), None) != 0 and "257 entries" in _lib.last_error()
    span.n, span.elem0 = 8, 4
    assert fn(pa, 1, ctypes.byref(ok), None) != 0 and "multiple of 8" in _lib.last_error()
    span.n, span.elem0 = 32, 8  # [8, 40) needs 5 ids, the map has 4
    assert fn(pa, 1, ctypes.byref(ok), None) != 0 and "outside the id map" in _lib.last_error()
    span.n, span.elem0 = 24, 8  # inside the map: now the span itself is looked at (null p / g / m / v)
    assert fn(pa, 1, ctypes.byref(ok), None) != 0 and "bad arguments" in _lib.last_error()


# ------------------------------------------------------------------------------------------------------------- constructor
@pytest.mark.parametrize("cls", CLASSES, ids=lambda c: c.__name__)
def test_split_groups_keyword(cls):
    w = torch.nn.Parameter(torch.zeros(3))
    kw = dict(lr=1e-3)
    assert cls([w], **kw).split_groups is False
    o = cls([w], split_groups=True, **kw)
    assert o.split_groups is True
    assert "split_groups" not in o.defaults and "split_groups" not in o.state_dict()["param_groups"][0]
