"""``BertLamb`` without a GPU: the fp64 restatement of the step against the golden trajectory, the order of its sums, the
tensor table, the constructor, the refusals, the groups ``make_optimizer`` builds, the ``state_dict`` exchange with
``BertAdam``, and the new symbols with the argument checks that run before any launch."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

from oracle import shapes
from xggm_amd import _lib, arena, ops
from xggm_amd.lxrt.optimization import SCHEDULES, BertAdam, BertLamb, lamb_step_host, lamb_sum_host
from xggm_amd.vqa.vqacpv2 import NO_DECAY, make_optimizer

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lamb.npz")


# ---------------------------------------------------------------------------------------------------------- the restatement
def test_restatement_follows_the_golden_trajectory():
    """six steps of ``lamb_step_host`` over the golden's fp32 inputs.  Both sides are fp64 and differ only in the order of
    the two sums per tensor (at most 2500 non-negative terms: 2500 * 2^-53 = 2.8e-13 relative on a sum, half of it on a
    norm) and in the ratio's rounding to fp32 here (2^-24 = 6e-8 relative on r, hence on p's CHANGE, which is below 1e-3 of
    |p|): 1e-7 relative on the ratios, 1e-10 of max|p| on p, 1e-12 relative on m and v, which no ratio touches."""
    g = np.load(GOLDEN)
    lengths = g["lengths"].tolist()
    off = np.concatenate([[0], np.cumsum(lengths)])
    lr0, b1, b2, e, warmup, t_total = g["hyper"].tolist()
    P = [g["p0"][a:b].astype(np.float64) for a, b in zip(off[:-1], off[1:])]
    M = [np.zeros(n) for n in lengths]
    V = [np.zeros(n) for n in lengths]
    for s in range(g["grads"].shape[0]):
        lr = lr0 * SCHEDULES["warmup_linear"](s / t_total, warmup)
        for i, (a, b) in enumerate(zip(off[:-1], off[1:])):
            P[i], M[i], V[i], r = lamb_step_host(P[i], g["grads"][s, a:b], M[i], V[i], lr, b1, b2, e,
                                                 float(g["weight_decay"][i]), bool(g["adapted"][i]))
            assert abs(r - g["ratios"][s, i]) <= 1e-7 * g["ratios"][s, i], (s, i, r)
        if s == 0:
            assert np.array_equal(np.concatenate(P), g["p_first"])  # lr 0: p keeps its bits
            assert np.allclose(np.concatenate(M), g["m_first"], rtol=1e-12, atol=0)
    p, m, v = (np.concatenate(X) for X in (P, M, V))
    assert np.abs(p - g["p_last"]).max() <= 1e-10 * np.abs(g["p_last"]).max()
    assert np.allclose(m, g["m_last"], rtol=1e-12, atol=0) and np.allclose(v, g["v_last"], rtol=1e-12, atol=0)
    assert np.abs(g["p_last"] - g["p_first"]).max() > 1e-5  # the trajectory moves


def test_sum_order_is_the_documented_one():
    """a hand evaluation of include/xggm.h's "ORDER OF THE SUMS" on a case where the order shows: one chunk and a bit, with
    terms of very different size"""
    rng = np.random.default_rng(5)
    x = rng.standard_normal(2048 + 9) ** 2 * np.where(rng.random(2048 + 9) < 0.1, 1e12, 1.0)
    parts = []
    for c in range(2):
        ch = np.zeros(2048)
        seg = x[2048 * c:2048 * (c + 1)]
        ch[:seg.size] = seg
        a = [0.0] * 256
        for t in range(256):
            for e in list(range(4 * t, 4 * t + 4)) + list(range(1024 + 4 * t, 1024 + 4 * t + 4)):
                a[t] = a[t] + ch[e]
        parts.append(a)

    def reduce(a):
        a = list(a)
        for w in range(4):
            h = 32
            while h:
                for l in range(h):
                    a[64 * w + l] = a[64 * w + l] + a[64 * w + l + h]
                h //= 2
        return (a[0] + a[64]) + (a[128] + a[192])

    b = [0.0] * 256
    b[0], b[1] = 0.0 + reduce(parts[0]), 0.0 + reduce(parts[1])
    want = reduce(b)
    assert lamb_sum_host(x) == want
    assert want != float(sum(x.tolist()))  # (an order, not just a sum: the running sum rounds differently here)
    assert lamb_sum_host(np.zeros(5)) == 0.0 and lamb_sum_host(np.array([3.0])) == 3.0


# --------------------------------------------------------------------------------------------------------- the tensor table
def test_tensor_table_on_a_hand_made_layout():
    info = {"b": (256, 7, "g", True), "a": (0, 130, "g", False), "c": (264, 1, "g", True), "d": (512, 4096, "h", False)}
    table, names = arena.lamb_tensor_table(info, {"a": True, "c": False, "d": 1}, 4608)
    assert names == ["a", "b", "c", "d"] and table.dtype == np.int64
    assert table.tolist() == [[0, 130, 1], [256, 7, 0], [264, 1, 0], [512, 4096, 1]]
    for bad in ({"x": (4, 4, "g", True)}, {"x": (0, 9, "g", True), "y": (8, 8, "g", True)}, {"x": (0, 16, "g", True)},
                {"x": (0, 0, "g", True)}):
        with pytest.raises(ValueError, match="lamb_tensor_table"):
            arena.lamb_tensor_table(bad, {}, 8)


def test_tensor_table_of_a_real_layout():
    sh = shapes.model_shapes(shapes.FULL, 3129)

    class P:
        def __init__(self, s):
            self.shape = tuple(s)

        def dim(self):
            return len(self.shape)

        def numel(self):
            return int(np.prod(self.shape))

    named = [(n, P(s)) for n, s in sh.items()]
    _, groups, info, total = arena.layout(named, arena.default_group_of)
    table, names = arena.lamb_tensor_table(info, {n: not n.endswith("bias") for n in info}, total)
    assert len(names) == len(sh) and sorted(names) == sorted(sh)
    assert (np.diff(table[:, 0]) >= table[:-1, 1]).all() and (table[:, 0] % 8 == 0).all()
    assert table[:, 1].sum() == sum(p.numel() for _, p in named) and table[-1, 0] + table[-1, 1] <= total
    assert all(bool(a) == (not n.endswith("bias")) for n, a in zip(names, table[:, 2]))
    # the scratch: one pair of doubles per chunk, and a tensor's chunks never run into the next tensor's
    slots = _lib.lib.xggm_lamb_workspace_bytes(total, len(names)) // 16
    first = table[:, 0] // ops.LAMB_CHUNK + np.arange(len(names))
    last = first + (table[:, 1] + ops.LAMB_CHUNK - 1) // ops.LAMB_CHUNK - 1
    assert (first[1:] > last[:-1]).all() and last[-1] < slots


# ------------------------------------------------------------------------------------------------ constructor and refusals
def test_constructor_defaults_and_checks():
    w = torch.nn.Parameter(torch.zeros(3))
    a, o = BertAdam([w], lr=1e-3), BertLamb([w], lr=1e-3)
    assert isinstance(o, BertAdam) and o.split_groups is False and BertLamb([w], lr=1e-3, split_groups=True).split_groups
    assert {k: v for k, v in o.defaults.items() if k != "layer_adaptation"} == a.defaults
    assert o.defaults["layer_adaptation"] is True and o.param_groups[0]["layer_adaptation"] is True
    assert BertLamb([{"params": [w], "layer_adaptation": False}], lr=1e-3).param_groups[0]["layer_adaptation"] is False
    assert "layer_adaptation" in BertLamb.SPLIT_KEYS and "layer_adaptation" not in BertAdam.SPLIT_KEYS
    assert o.trust_ratios() == {} and o.get_lr() == [0]
    for kw in (dict(lr=-1.0), dict(lr=1e-3, schedule="x"), dict(lr=1e-3, warmup=1.5), dict(lr=1e-3, b1=1.0), dict(lr=1e-3, e=-1.0)):
        with pytest.raises(ValueError):
            BertLamb([w], **kw)


def test_refusals_name_their_reason():
    o = BertLamb([torch.nn.Parameter(torch.zeros(3))], lr=1e-3)
    o._check_arena(types.SimpleNamespace(zero1=None, fp8=None))
    with pytest.raises(RuntimeError, match="zero1.*norm would cross"):
        o._check_arena(types.SimpleNamespace(zero1=object(), fp8=None))
    with pytest.raises(RuntimeError, match="fp8 forward"):
        o._check_arena(types.SimpleNamespace(zero1=None, fp8=object()))
    from xggm_amd.lxrt.optimization import require_arena_aware
    require_arena_aware(o)  # clip_and_step takes it


def _tiny_model():
    from xggm_amd import param
    from xggm_amd.lxrt.modeling import BertConfig, VISUAL_CONFIG
    from xggm_amd.vqa.vqacpv2_model import VQAModel
    cfg = shapes.TINY
    VISUAL_CONFIG.set_visual_dims(cfg["feat_dim"], 4)
    a = param.parse_args(["--llayers", "2", "--xlayers", "2", "--rlayers", "1"])
    bc = BertConfig(cfg["vocab"], hidden_size=cfg["hidden"], num_attention_heads=cfg["heads"],
                    intermediate_size=cfg["inter"], max_position_embeddings=cfg["max_pos"])
    return VQAModel(29, args=a, config=bc)


def test_groups_of_make_optimizer():
    from xggm_amd import param
    assert param.get_optimizer("bertlamb") == "bert"
    m = _tiny_model()
    names = {id(p): n for n, p in m.named_parameters()}
    o = make_optimizer(m, 1e-4, 100, optim="bertlamb", no_decay=NO_DECAY)
    assert type(o) is BertLamb and o.split_groups and len(o.param_groups) == 4
    plain = {names[id(p)] for pg in o.param_groups if not pg["layer_adaptation"] for p in pg["params"]}
    ln_w = {n for n, p in m.named_parameters() if n.endswith(".weight") and p.dim() == 1}
    assert plain == ln_w | {n for n in names.values() if n.endswith("bias")}
    for pg in o.param_groups:
        assert (pg["weight_decay"] == 0.0) == (pg["layer_adaptation"] is False)
        assert pg["weight_decay"] in (0.0, 0.01) and pg["warmup"] == 0.1 and pg["t_total"] == 100
    assert sum(len(pg["params"]) for pg in o.param_groups) == len(names)
    # without no_decay: the reference's two groups, every tensor adapted
    o2 = make_optimizer(m, 1e-4, 100, optim="bertlamb")
    assert type(o2) is BertLamb and not o2.split_groups
    assert [(pg["lr"], pg["layer_adaptation"]) for pg in o2.param_groups] == [(4e-4, True), (1e-4, True)]
    # and the default stays BertAdam itself
    assert type(make_optimizer(m, 1e-4, 100)) is BertAdam and type(make_optimizer(m, 1e-4, 100, no_decay=NO_DECAY)) is BertAdam


def test_state_dict_moves_to_bertadam_and_back():
    ws = [torch.nn.Parameter(torch.zeros(3)), torch.nn.Parameter(torch.zeros(2))]
    groups = lambda: [{"params": [ws[0]]}, {"params": [ws[1]], "weight_decay": 0.0}]  # noqa: E731
    lamb = BertLamb(groups(), lr=1e-3, warmup=0.1, t_total=10)
    lamb.param_groups[1]["layer_adaptation"] = False
    state = {0: {"step": 3, "next_m": torch.ones(3), "next_v": torch.full((3,), 2.0)},
             1: {"step": 3, "next_m": torch.ones(2), "next_v": torch.full((2,), 2.0)}}
    sd = lamb.state_dict()
    assert [sorted(k for k in g if k != "layer_adaptation") for g in sd["param_groups"]] == \
        [sorted(g) for g in BertAdam(groups(), lr=1e-3).state_dict()["param_groups"]]
    sd["state"] = state
    adam = BertAdam(groups(), lr=5e-3)
    adam.load_state_dict(sd)
    assert all("layer_adaptation" not in g for g in adam.param_groups) and adam.param_groups[0]["lr"] == 1e-3
    back = adam.state_dict()  # (no arena yet: the pending state travels)
    assert back["state"][0]["step"] == 3 and torch.equal(back["state"][1]["next_v"], state[1]["next_v"])
    lamb2 = BertLamb(groups(), lr=7e-3)
    lamb2.param_groups[1]["layer_adaptation"] = False
    lamb2.load_state_dict(back)
    assert [g["layer_adaptation"] for g in lamb2.param_groups] == [True, False]  # a BertAdam checkpoint has no flag: kept
    assert lamb2.param_groups[0]["lr"] == 1e-3 and lamb2.param_groups[1]["weight_decay"] == 0.0
    assert torch.equal(lamb2.state_dict()["state"][0]["next_m"], state[0]["next_m"])
    lamb2.load_state_dict(sd)  # a BertLamb checkpoint carries its flags
    assert [g["layer_adaptation"] for g in lamb2.param_groups] == [True, False]


# --------------------------------------------------------------------------------------------------------------------- ABI
def test_symbols_are_declared_exported_and_cited():
    decl = _lib.parse_header()
    assert len(decl["xggm_lamb_multi"]) == 9 and len(decl["xggm_lamb_workspace_bytes"]) == 2
    assert hasattr(_lib.lib, "xggm_lamb_multi") and hasattr(_lib.lib, "xggm_lamb_workspace_bytes")
    src = open(_lib.HEADER_PATH).read()
    body = src[src.index("/* BertLamb"):src.index("int xggm_lamb_multi")]
    assert "src/lxrt/optimization.py:159-193" in body and "src/vqa/vqacpv2.py:125-128" in body
    assert "ORDER OF THE SUMS" in body and "#define XGGM_LAMB_CHUNK 2048" in body and ops.LAMB_CHUNK == 2048
    assert _lib.lib.xggm_lamb_workspace_bytes(0, 0) == 16 and _lib.lib.xggm_lamb_workspace_bytes(4096, 3) == 16 * 6
    assert _lib.lib.xggm_lamb_workspace_bytes(-1, 3) == 0
    # the span struct is the one xggm_optim_multi takes; a row of the tensor table is three int64
    assert ctypes.sizeof(ops.AdamArgs) == 152 and ops.AdamArgs.elem0.offset == 136 and ops.AdamArgs.g_scale.offset == 144
    assert "int64_t elem0;" in body and "int64_t n;" in body and "int64_t adapted;" in body


def test_argument_checks_come_before_any_launch():
    """no GPU here: every call below has to return non-zero with a message from the host-side checks"""
    fn = _lib.lib.xggm_lamb_multi
    arr = (ops.AdamArgs * 2)()
    pa = ctypes.cast(arr, ctypes.c_void_p)
    T, R, W = 0x1000, 0x2000, 0x3000

    def err(*a):
        assert fn(*a) != 0
        return _lib.last_error()

    assert "no spans" in err(None, 1, T, 1, None, R, W, 1 << 20, None)
    assert "no spans" in err(pa, 0, T, 1, None, R, W, 1 << 20, None)
    assert "tensor table" in err(pa, 1, None, 1, None, R, W, 1 << 20, None)
    assert "tensor table" in err(pa, 1, T, 0, None, R, W, 1 << 20, None)
    assert "tensor table" in err(pa, 1, T + 4, 1, None, R, W, 1 << 20, None)
    assert "ratios_out" in err(pa, 1, T, 1, None, None, W, 1 << 20, None)
    assert "workspace" in err(pa, 1, T, 1, None, R, None, 1 << 20, None)
    assert "workspace" in err(pa, 1, T, 1, None, R, W + 8, 1 << 20, None)
    assert "id map" in err(pa, 1, T, 1, ctypes.byref(ops.HyperMap(None, 4, 0x4000, 2)), R, W, 1 << 20, None)
    assert "257 entries" in err(pa, 1, T, 1, ctypes.byref(ops.HyperMap(0x5000, 4, 0x4000, 257)), R, W, 1 << 20, None)
    assert "null pointer or no elements" in err(pa, 1, T, 1, None, R, W, 1 << 20, None)
    for s in arr:
        s.p, s.g, s.m, s.v, s.n = 0x10000, 0x20000, 0x30000, 0x40000, 64
    arr[0].m = 0x30004
    assert "16-byte aligned" in err(pa, 1, T, 1, None, R, W, 1 << 20, None)
    arr[0].m, arr[0].shadow8 = 0x30000, 0x50000
    assert "e4m3" in err(pa, 1, T, 1, None, R, W, 1 << 20, None)
    arr[0].shadow8, arr[0].elem0 = None, 4
    assert "multiple of 8" in err(pa, 1, T, 1, None, R, W, 1 << 20, None)
    arr[0].elem0, arr[1].elem0 = 0, 56  # the second span starts inside the first
    assert "do not overlap" in err(pa, 2, T, 1, None, R, W, 1 << 20, None)
    arr[1].elem0, arr[1].g_bf16 = 64, 1
    assert "gradient type" in err(pa, 2, T, 1, None, R, W, 1 << 20, None)
    arr[1].g_bf16 = 0
    assert "outside the id map" in err(pa, 2, T, 1, ctypes.byref(ops.HyperMap(0x5000, 15, 0x4000, 2)), R, W, 1 << 20, None)
    need = _lib.lib.xggm_lamb_workspace_bytes(128, 1)
    assert "workspace of %d bytes" % (need - 16) in err(pa, 2, T, 1, None, R, W, need - 16, None)
