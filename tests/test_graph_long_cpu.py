"""What the graph kernels for 65..128 objects promise without a GPU.

  * the yardstick: the oracle's generators in fp64 reproduce the three fixtures the reference's own generator classes
    produced at N = 100, 72 and 128 (tests/golden/make_graph_long_golden.py), with the bounds test_oracle_golden.py
    uses for the 36- and 64-object ones;
  * every ``_long`` entry point of include/xggm.h refuses N = 64, N = 129 and null pointers on the host, with its own name
    in xggm_last_error() -- nothing is enqueued (there is no GPU here to enqueue on);
  * ``long_graph=True`` builds the model classes and the generators without changing a state_dict key.
"""
import pytest
import torch

from oracle import shapes
from oracle import xggm_oracle as O
from xggm_amd import synth
from helpers import load_golden, seeded_params, probe, rel_err
from test_oracle_golden import TOL, check_grad_summary

FAKE = 0x10000  # a 16-byte aligned address nobody dereferences: validation happens on the host, before any launch


@pytest.mark.parametrize("tag", ["gen_gcn100", "gen_gin72", "gen_gat128"])
def test_oracle_generators_reproduce_the_long_goldens_in_fp64(tag):
    g = load_golden(tag)
    kind, H, N, B = str(g["kind"]), int(g["H"]), int(g["N"]), int(g["B"])
    nl, seed = int(g["n_layers"]), int(g["seed"])
    assert N > 64
    sh = shapes.generator_shapes(kind, H, nl)
    P = {k: v.double().requires_grad_(True) for k, v in seeded_params(sh, seed).items()}
    xn, an = synth.generator_inputs(tag, kind, B, N, H, seed)
    x = torch.from_numpy(xn).double().requires_grad_(True)
    adj = torch.from_numpy(an).double().requires_grad_(True)
    xo, ao = O.GENERATORS[kind](P, "generator.", x, adj, nl)
    assert rel_err(xo, torch.from_numpy(g["x_out"])) < TOL
    assert rel_err(ao, torch.from_numpy(g["adj_out"])) < TOL
    loss = (xo * probe("xo", xo.shape, seed).double()).sum() + (ao * probe("ao", ao.shape, seed).double()).sum()
    loss.backward()
    assert rel_err(x.grad, torch.from_numpy(g["dx"])) < 1e-4
    if kind != "GAT":
        assert rel_err(adj.grad, torch.from_numpy(g["dadj"])) < 1e-4
    check_grad_summary(g, {k: v.grad for k, v in P.items()}, seed)


def _entries():
    """name -> callable(N, null) issuing the call with fake pointers (``null``: every pointer NULL)"""
    def agg(name):
        return lambda L, N, null: getattr(L, name)(*((None,) * 3 if null else (FAKE,) * 3), 2, N, 64, 0, 1.0, None, 0.0, 0, None)

    def dot(name):
        return lambda L, N, null: getattr(L, name)(*((None,) * 4 if null else (FAKE,) * 4), 2, N, 64, None if null else FAKE, None)

    def gat_bwd(name):
        return lambda L, N, null: getattr(L, name)(*((None,) * 5 if null else (FAKE,) * 5), 2, N, 0.2, None)

    return {
        "xggm_aggregate_long_f32": agg("xggm_aggregate_long_f32"),
        "xggm_aggregate_long_bf16": agg("xggm_aggregate_long_bf16"),
        "xggm_agg_dot_long_f32": dot("xggm_agg_dot_long_f32"),
        "xggm_agg_dot_long_bf16": dot("xggm_agg_dot_long_bf16"),
        "xggm_adj_regen_long_fwd": lambda L, N, null: L.xggm_adj_regen_long_fwd(*((None,) * 4 if null else (FAKE,) * 4), 2, N, None),
        "xggm_adj_regen_long_bwd": lambda L, N, null: L.xggm_adj_regen_long_bwd(*((None,) * 6 if null else (FAKE,) * 6), 2, N, None),
        "xggm_adj_init_long_fwd": lambda L, N, null: L.xggm_adj_init_long_fwd(*((None,) * 4 if null else (FAKE,) * 4), 2, N, 1.0,
                                                                               None, 0, None),
        "xggm_adj_init_long_bwd": lambda L, N, null: L.xggm_adj_init_long_bwd(*((None,) * 2 if null else (FAKE,) * 2), 2, N, None),
        "xggm_gat_att_long_fwd": lambda L, N, null: L.xggm_gat_att_long_fwd(*((None,) * 3 if null else (FAKE,) * 3), 2, N, 0.2, None),
        "xggm_gat_att_long_bwd_f32": gat_bwd("xggm_gat_att_long_bwd_f32"),
        "xggm_gat_att_long_bwd_bf16": gat_bwd("xggm_gat_att_long_bwd_bf16"),
        "xggm_cosine_adjacency_long_f32": lambda L, N, null: L.xggm_cosine_adjacency_long_f32(
            *((None,) * 3 if null else (FAKE,) * 3), 2, N, 768, 1e-6, None),
    }


def test_entry_table_covers_every_long_symbol_of_the_header():
    from xggm_amd import _lib
    declared = sorted(n for n in _lib.parse_header() if "_long" in n and not n.startswith("xggm_attn"))
    assert declared == sorted(_entries())


@pytest.mark.parametrize("name", sorted(_entries()))
def test_long_entries_refuse_short_oversized_and_null_before_launch(name):
    from xggm_amd import _lib
    L, call = _lib.lib, _entries()[name]
    for N in (64, 129, 0, -5):
        rc = call(L, N, False)
        msg = L.xggm_last_error().decode()
        assert rc != 0 and name in msg and ("N=%d" % N) in msg, (name, N, rc, msg)
    rc = call(L, 100, True)
    msg = L.xggm_last_error().decode()
    assert rc != 0 and name in msg, (name, rc, msg)


def _tiny_args():
    from xggm_amd import param
    from xggm_amd.lxrt.modeling import BertConfig, VISUAL_CONFIG
    cfg = shapes.TINY
    VISUAL_CONFIG.set_visual_dims(cfg["feat_dim"], 4)
    a = param.parse_args(["--llayers", "1", "--xlayers", "1", "--rlayers", "1"])
    bc = BertConfig(cfg["vocab"], hidden_size=cfg["hidden"], num_attention_heads=cfg["heads"], intermediate_size=cfg["inter"],
                    max_position_embeddings=128)
    return a, bc


def test_long_graph_builds_the_classes_and_adds_no_state():
    from xggm_amd.gqa.gqa_ood_model import GQAModel
    from xggm_amd.module.graph_generative_modeling import GCNGenerator, GINGenerator, GATGenerator
    from xggm_amd.vqa.vqacpv2_model import VQAModel
    a, bc = _tiny_args()
    for cls in (VQAModel, GQAModel):
        for gnn in ("GCN", "GIN", "GAT"):
            on = cls(7, gnn=gnn, args=a, config=bc, n_objects=100, long_graph=True)
            off = cls(7, gnn=gnn, args=a, config=bc, n_objects=100)
            assert on.long_graph is True and off.long_graph is False
            assert list(on.state_dict()) == list(off.state_dict())
            assert [tuple(v.shape) for v in on.state_dict().values()] == [tuple(v.shape) for v in off.state_dict().values()]
    for cls, nl in ((GCNGenerator, 2), (GINGenerator, 2), (GATGenerator, 1)):
        on, off = cls(128, nl, long_graph=True), cls(128, nl)
        assert on.long_graph is True and off.long_graph is False
        assert list(on.state_dict()) == list(off.state_dict())
    with pytest.raises(ValueError, match="128"):  # check_sequence_limits is unchanged: the flag opens nothing past 128
        VQAModel(7, args=a, config=bc, n_objects=129, long_graph=True)


def test_long_graph_lives_on_the_runtime_and_defaults_off():
    from xggm_amd.functional import Runtime
    import inspect
    assert "long_graph = False" in inspect.getsource(Runtime.__init__)
    from xggm_amd import ops
    for fn in (ops.aggregate, ops.agg_dot, ops.adj_regen_fwd, ops.adj_regen_bwd, ops.adj_init_fwd, ops.adj_init_bwd,
               ops.gat_att_fwd, ops.gat_att_bwd):
        assert inspect.signature(fn).parameters["long"].default is False, fn.__name__
    # the symbol choice: the twin only with the opt-in AND N > 64
    assert ops._lg("xggm_aggregate", 64, True, "_f32") == "xggm_aggregate_f32"
    assert ops._lg("xggm_aggregate", 65, False, "_f32") == "xggm_aggregate_f32"
    assert ops._lg("xggm_aggregate", 65, True, "_f32") == "xggm_aggregate_long_f32"
    assert ops._lg("xggm_adj_regen", 128, True, "_bwd") == "xggm_adj_regen_long_bwd"


def test_near_tied_column_maxima_of_gen_gat128_and_their_admissible_references():
    """the restated regeneration with the oracle's own arg-max is the fixture's gradient; gen_gat128 has near-tied columns,
    and a gradient taken with the runner-up row of the closest pair -- 7e-2 away from the fixture -- is recognised as one of
    the admissible references, while a gradient that is simply wrong is not"""
    import graph_long_cases as C
    g = load_golden("gen_gat128")
    refs = C.GatTieRefs("gen_gat128", g)
    gold = torch.from_numpy(g["dx"])
    assert rel_err(refs.dx(refs.idx0), gold) < 1e-4
    assert refs.near and refs.min_gap < 1e-4
    err, flipped = refs.admissible_err(gold)
    assert err < 1e-4 and flipped == []
    b, j = refs.near[0]
    t = refs.idx0.clone()
    t[b, j] = refs.second[b, j]
    other = refs.dx(t)
    assert rel_err(other, gold) > 1e-2  # the discontinuity: one column, a visible share of the whole gradient
    err, flipped = refs.admissible_err(other)
    assert err < 1e-6 and flipped == [(b, j)]
    err, _ = refs.admissible_err(1.1 * gold)  # a wrong gradient stays wrong
    assert err > 9e-2
    # the 36-object fixture's restatement agrees with its golden too
    g36 = load_golden("gen_gat36")
    r36 = C.GatTieRefs("gen_gat36", g36)
    assert rel_err(r36.dx(r36.idx0), torch.from_numpy(g36["dx"])) < 1e-4
