"""Whole passes with more than 64 tokens or objects: the encoder on csrc/attention_long.hip.

The tiny model of oracle.shapes with a 128-row position table, fp32 execution, against the CPU oracle in the manner of
test_model_gpu.test_edge_configurations_match_oracle_fp32 and with its tolerances (losses within 1e-3 relative, three
named weights within 1e-4 after four passes):
  tokens72    T = 72, N = 36, B = 3: every language self-attention and both directions of every cross-attention are long
              on the token side and short on the object side (one long and one short problem in every grouped call)
  tokens128   T = 128, B = 2: the largest sentence
  objects100  N = 100, T = 20, B = 2: the 100-box features; plain passes only -- the generator's graph kernels stop at
              64 objects, and a GGM pass must keep failing in their entry points
A bf16 CapturedTrainer at T = 72 replays exactly what an eager twin computes (two iterations, torch.equal on every arena
buffer), and a CapturedPredictor at N = 100 gives the eager forward's answers.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from xggm_amd import synth  # noqa: E402
from helpers import batch_tensors, rel_err  # noqa: E402

DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def long_cfg(**kw):
    from oracle import shapes
    return dict(shapes.TINY, max_pos=128, **kw)


def build(cfg, A, T, N, dt, seed, gnn="GCN", n_layers=2):
    from xggm_amd import param
    from xggm_amd.lxrt.modeling import BertConfig, VISUAL_CONFIG
    from xggm_amd.vqa.vqacpv2_model import VQAModel
    VISUAL_CONFIG.set_visual_dims(cfg["feat_dim"], 4)
    a = param.parse_args(["--llayers", str(cfg["l_layers"]), "--xlayers", str(cfg["x_layers"]), "--rlayers", str(cfg["r_layers"])])
    bc = BertConfig(cfg["vocab"], hidden_size=cfg["hidden"], num_attention_heads=cfg["heads"], intermediate_size=cfg["inter"],
                    max_position_embeddings=cfg["max_pos"])
    m = VQAModel(A, gnn=gnn, n_layers=n_layers, args=a, config=bc, compute_dtype=dt, max_seq_length=T, n_objects=N)
    m.load_state_dict({k: torch.from_numpy(synth.seeded_param(k, v.shape, seed)) for k, v in m.state_dict().items()})
    return m.to(DEV)


@pytest.mark.parametrize("case", ["tokens72", "tokens128", "objects100"])
def test_long_configurations_match_oracle_fp32(case):
    from oracle import shapes, xggm_oracle as O
    from helpers import seeded_params
    from xggm_amd.vqa.vqacpv2 import plain_pass, ggm_pass, BCEWithLogitsLoss, make_optimizer
    cfg, A, seed, gnn, n_layers = long_cfg(), 19, 12, "GCN", 2
    B, N, T, kinds = {"tokens72": (3, 36, 72, ["plain", "rel", "node", "plain"]),
                      "tokens128": (2, 36, 128, ["plain", "rel", "node", "plain"]),
                      "objects100": (2, 100, 20, ["plain"] * 4)}[case]
    m = build(cfg, A, T, N, F32, seed).eval()
    opt = make_optimizer(m, 1e-3, 8)
    bn = synth.vqa_batch(B, A=A, N=N, T=T, F=cfg["feat_dim"], vocab=cfg["vocab"], seed=seed)
    bn["randn_node"] = synth.randn_nodes(B, N, cfg["hidden"], seed)
    b, bc = batch_tensors(bn, DEV), batch_tensors(bn)
    P = seeded_params(shapes.model_shapes(cfg, A, gnn=gnn, n_layers=n_layers, n_adj=N * (N - 1) // 2), seed)
    Mo = {k: torch.zeros_like(v) for k, v in P.items()}
    Vo = {k: torch.zeros_like(v) for k, v in P.items()}
    step = {k: 0 for k in P}
    sent = (b["input_ids"], b["input_mask"], b["segment_ids"])
    bce = BCEWithLogitsLoss()
    for kind in kinds:
        kw = {} if kind == "plain" else dict(sigma=1.0, kl_weight=8.0, gnn=gnn, n_layers=n_layers)
        lo, _, _, _ = O.train_pass(P, Mo, Vo, step, bc, cfg, kind, 1e-3, 8, **kw)
        if kind == "plain":
            l, _ = plain_pass(m, opt, bce, b["feats"], b["boxes"], sent, b["target"])
        else:
            l, _, _ = ggm_pass(m, opt, bce, b["feats"], b["boxes"], sent, b["target"], b["adj_true"], kind, sigma=1.0,
                               kl_weight=8.0, randn=b["randn_adj"] if kind == "rel" else b["randn_node"])
        print("%s %s: loss %.6f, oracle %.6f" % (case, kind, float(l), float(lo)))
        assert abs(float(l) - float(lo)) < 1e-3 * abs(float(lo)), (case, kind, float(l), float(lo))
    sd = m.state_dict()
    names = ["logit_fc.3.weight", "lxrt_encoder.model.bert.encoder.layer.0.attention.self.query.weight"]
    # the plain pass never reaches encoder_adj: at N = 100 the third weight is a cross-attention one
    names.append("encoder_adj.0.weight" if N <= 64 else "lxrt_encoder.model.bert.encoder.x_layers.0.visual_attention.att.query.weight")
    for n in names:
        assert rel_err(sd[n], P[n]) < 1e-4, (case, n, rel_err(sd[n], P[n]))
    if N > 64:  # the generator's graph kernels keep their 64-object tile: their entry points refuse the pass on the host
        with pytest.raises(RuntimeError, match="xggm_"):
            ggm_pass(m, opt, bce, b["feats"], b["boxes"], sent, b["target"], b["adj_true"], "node", sigma=1.0, kl_weight=8.0,
                     randn=b["randn_node"])


def _same_state(m1, m2):
    from xggm_amd.runtime import runtime_of
    a1, a2 = runtime_of(m1).arena, runtime_of(m2).arena
    bad = [k for k in ("params", "grads", "m", "v", "shadow") if not torch.equal(getattr(a1, k), getattr(a2, k))]
    assert not bad, bad
    assert a1.steps.tolist() == a2.steps.tolist() and runtime_of(m1).rng.tolist() == runtime_of(m2).rng.tolist()


def test_captured_trainer_at_72_tokens_equals_its_eager_twin():
    """bf16, dropout on: two captured iterations against the same schedule launched eagerly -- the same bits"""
    from xggm_amd.engine import CapturedTrainer
    from xggm_amd.runtime import runtime_of
    from xggm_amd.vqa.vqacpv2 import plain_pass, ggm_pass, BCEWithLogitsLoss, make_optimizer
    cfg, A, B, T, N = long_cfg(), 29, 3, 72, 36
    m1, m2 = (build(cfg, A, T, N, BF16, 5) for _ in range(2))
    for m in (m1, m2):
        m.seed = 11
    o1, o2 = make_optimizer(m1, 1e-4, 40), make_optimizer(m2, 1e-4, 40)
    batches = [batch_tensors(synth.vqa_batch(B, A=A, N=N, T=T, F=cfg["feat_dim"], vocab=cfg["vocab"], seed=s), DEV) for s in (3, 4)]
    branches = ["rel", "node"]
    tr = CapturedTrainer(m1, o1, batches[0], sigma=1.0, warmup_iters=1)
    cap = []
    for i, br in enumerate(branches):
        tr.load_batch(batches[i % 2])
        (lp, _, _), (lg, _, _) = tr.iteration(br)
        cap += [float(lp), float(lg)]
    bce, rt2 = BCEWithLogitsLoss(), runtime_of(m2)
    m2.train()

    def run(kind, b):
        sent = (b["input_ids"], b["input_mask"], b["segment_ids"])
        if kind == "plain":
            out = plain_pass(m2, o2, bce, b["feats"], b["boxes"], sent, b["target"])
        else:
            out = ggm_pass(m2, o2, bce, b["feats"], b["boxes"], sent, b["target"], b["adj_true"], kind, 1.0, 8.0)
        rt2.advance()
        return float(out[0])

    for kind in ("plain", "rel", "node"):  # the constructor's warm-up iteration
        run(kind, batches[0])
    eager = []
    for i, br in enumerate(branches):
        eager += [run("plain", batches[i % 2]), run(br, batches[i % 2])]
    assert cap == eager, (cap, eager)
    assert all(torch.isfinite(torch.tensor(cap)))
    _same_state(m1, m2)


def test_captured_predictor_at_100_objects_equals_the_eager_forward():
    from xggm_amd.engine import CapturedPredictor
    cfg, A, B, T, N = long_cfg(), 29, 3, 20, 100
    m = build(cfg, A, T, N, BF16, 7).eval()
    pred = CapturedPredictor(m, B, n_objects=N)
    for s in (3, 4):
        b = batch_tensors(synth.vqa_batch(B, A=A, N=N, T=T, F=cfg["feat_dim"], vocab=cfg["vocab"], seed=s), DEV)
        sent = (b["input_ids"], b["input_mask"], b["segment_ids"])
        label, logit = pred(b["feats"], b["boxes"], sent)
        label, logit = label.clone(), logit.clone()
        with torch.no_grad():
            _, _, x = m(b["feats"], b["boxes"], sent)
            ref = m.logit_fc(x)
        assert torch.equal(logit, ref) and torch.equal(label, ref.max(1)[1])
        assert bool(torch.isfinite(logit).all())
