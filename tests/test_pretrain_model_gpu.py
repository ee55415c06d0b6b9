"""LXRTPretraining on the GPU against what the reference's own model recorded in float64 (tests/golden/pretrain_h2.npz: the
fixture's two cases with 2 attention heads -- the HIP attention core is built for heads of 64, so H = 128 with the 4 heads
of pretrain.npz cannot run through the encoder; shapes, weights and batch are the same).  fp32: losses, answer_score and
gradients at ``tol(F32)``, two BertAdam steps through ``clip_and_step``; bf16: losses at the project's bf16 bar, gradient
cosine >= 0.99; ``mlm_capacity`` None against a tight one, the overflow flag, bit-equality across runs, and the heads alone
on the 4-head fixture's recorded encoder outputs."""
import json

import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import load_golden, rel_err  # noqa: E402
from test_kernels_gpu import tol  # noqa: E402
from test_pretrain_cpu import _tiny_model, _restore_visual_config  # noqa: E402

DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def golden():
    g = load_golden("pretrain_h2")
    return g, json.loads(str(g["meta_json"]))


def _batch(meta):
    from xggm_amd import synth
    c = meta["cfg"]
    x = synth.pretrain_case(c["B"], c["T"], c["O"], c["F"], c["vocab"], c["n_obj"], c["n_attr"], c["n_ans"], seed=meta["seed"])
    return {k: torch.from_numpy(v).to(DEV) for k, v in x.items()}


def _forward(model, t):
    obj_labels = {k: (t[k + "_label"], t[k + "_conf"]) for k in ("obj", "attr", "feat")}
    return model(t["input_ids"], t["segment_ids"], t["input_mask"], t["masked_lm_labels"], t["feats"], t["boxes"], obj_labels,
                 t["matched_label"], t["ans"])


def _run(case, dt, steps=0, **kw):
    """one forward + backward (and ``steps`` clipped BertAdam steps) -> (losses, total, answer_score, grads, params, model)"""
    from xggm_amd.lxrt.optimization import BertAdam
    from xggm_amd.runtime import runtime_of
    from xggm_amd.vqa.vqacpv2 import clip_and_step
    model, _, meta, _, saved = _tiny_model(case, compute_dtype=dt, **kw)
    try:
        model = model.to(DEV).eval()  # dropout off: the arithmetic of the recorded run
        t = _batch(meta)
        named = dict(model.named_parameters())
        optim = BertAdam(list(model.parameters()), lr=1e-3, warmup=0.1, t_total=8)
        out = None
        for step in range(max(steps, 1)):
            total, losses, answer_score = _forward(model, t)
            runtime_of(model).backward(total)
            if out is None:
                torch.cuda.synchronize()
                grads = {k: named[k].grad.detach().double().cpu().clone() for k in meta["grads"] if k in named}
                out = [losses.cpu().double().reshape(-1), float(total.detach()), answer_score.cpu().double(), grads]
            if steps:
                clip_and_step(model, optim, clip=1.0)
        params = {k: named[k].detach().double().cpu().reshape(-1)[:meta["slice"]].clone() for k in meta["grads"] if k in named}
        torch.cuda.synchronize()
        return out + [params, model]
    finally:
        _restore_visual_config(saved)


@pytest.mark.parametrize("case", ["full", "noqa"])
def test_fp32_model_against_the_reference(golden, case):
    g, meta = golden
    tag = case + "_h2"
    losses, total, answer_score, grads, params, model = _run(case, F32, steps=2)
    want = torch.from_numpy(g[tag + ".losses"])
    assert losses.numel() == want.numel() == meta["cases"][tag]["n_losses"]
    errs = {"loss%d" % i: abs(float(a) - float(b)) / abs(float(b)) for i, (a, b) in enumerate(zip(losses, want))}
    errs["total"] = abs(total - float(g[tag + ".total"][0])) / abs(float(g[tag + ".total"][0]))
    errs["answer_score"] = rel_err(answer_score, torch.from_numpy(g[tag + ".answer_score"]))
    for k, v in grads.items():
        errs["grad." + k] = rel_err(v, torch.from_numpy(g["%s.grad.%s" % (tag, k)]))
    for k, v in params.items():
        errs["after2." + k] = rel_err(v, torch.from_numpy(g["%s.after2.%s" % (tag, k)]))
    print(tag, {k: "%.1e" % v for k, v in errs.items()}, "(bound %.1e)" % tol(F32))
    assert int(model.mlm_overflow) == 0
    assert "grad.bert.embeddings.word_embeddings.weight" in errs and "after2.cls.predictions.bias" in errs
    assert max(errs.values()) <= tol(F32), errs
    # the parameters moved: the comparison above is not one of untouched weights
    from xggm_amd import synth
    w0 = synth.seeded_param("cls.predictions.bias", params["cls.predictions.bias"].shape, meta["seed"])[:meta["slice"]]
    assert float((params["cls.predictions.bias"] - torch.from_numpy(w0).double()).abs().max()) > 0


@pytest.mark.parametrize("case", ["full", "noqa"])
def test_bf16_model_against_the_reference(golden, case):
    g, meta = golden
    tag = case + "_h2"
    losses, total, _, grads, _, _ = _run(case, BF16)
    want = torch.from_numpy(g[tag + ".losses"])
    errs = {"loss%d" % i: abs(float(a) - float(b)) / abs(float(b)) for i, (a, b) in enumerate(zip(losses, want))}
    cos = {k: float(torch.nn.functional.cosine_similarity(v.reshape(-1), torch.from_numpy(g["%s.grad.%s" % (tag, k)])
                                                            .double().reshape(-1), dim=0)) for k, v in grads.items()}
    print(tag, {k: "%.1e" % v for k, v in errs.items()}, {k: "%.4f" % v for k, v in cos.items()})
    assert max(errs.values()) <= tol(BF16), errs
    assert min(cos.values()) >= 0.99, cos


@pytest.mark.parametrize("dt", [F32, BF16])
def test_capacity_changes_no_bit_and_runs_repeat(dt):
    """mlm_capacity None (B T slots) against exactly as many slots as labelled rows, and the same run twice: torch.equal
    losses and gradients, the tied table's among them; one slot fewer raises the flag and a NaN masked-LM loss"""
    full = _run("full", dt)
    tight = _run("full", dt, mlm_capacity=5)
    again = _run("full", dt, mlm_capacity=5)
    for a, b in ((full, tight), (tight, again)):
        assert torch.equal(a[0], b[0]) and a[1] == b[1] and torch.equal(a[2], b[2])
        assert sorted(a[3]) == sorted(b[3]) and "bert.embeddings.word_embeddings.weight" in a[3]
        for k in a[3]:
            assert torch.equal(a[3][k], b[3][k]), k
    assert int(tight[5].mlm_overflow) == 0
    short = _run("full", dt, mlm_capacity=4)
    assert int(short[5].mlm_overflow) == 1 and bool(torch.isnan(short[0][0])) and not bool(torch.isnan(short[0][1:]).any())


def test_two_trained_steps_start_a_fine_tuning_model(tmp_path):
    """a snapshot of LXRTPretraining after two steps on the GPU loads into a VQAModel through ``lxrt_encoder.load``"""
    from xggm_amd import param
    from xggm_amd.vqa.vqacpv2_model import VQAModel
    *_, model = _run("full", F32, steps=2)
    sd = {k: v.cpu() for k, v in model.state_dict().items()}
    torch.save(sd, str(tmp_path / "snap_LXRT.pth"))
    model2, _, meta, bc, saved = _tiny_model("full")
    try:
        cfg = meta["cfg"]
        a = param.parse_args(["--llayers", str(cfg["l_layers"]), "--xlayers", str(cfg["x_layers"]), "--rlayers", str(cfg["r_layers"])])
        vqa = VQAModel(7, args=a, config=bc)
        vqa.lxrt_encoder.load(str(tmp_path / "snap"))
        enc = vqa.lxrt_encoder.model.state_dict()
        assert all(torch.equal(enc[k], sd[k]) for k in enc)
        assert not torch.equal(sd["bert.pooler.dense.weight"], model2.state_dict()["bert.pooler.dense.weight"])  # trained
    finally:
        _restore_visual_config(saved)
