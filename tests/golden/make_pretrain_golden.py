"""Generate tests/golden/pretrain.npz, pretrain_h2.npz (the same cases with 2 attention heads) + pretrain_state_dict.json by running the REFERENCE's own ``LXRTPretraining``
(src/lxrt/modeling.py:955-1061) and ``BertAdam`` (src/lxrt/optimization.py) in float64.
    python tests/golden/make_pretrain_golden.py <path to the reference's src directory>
The reference is imported with the module stubs of make_golden.py (download helpers that are absent offline), never copied.
Weights come from ``xggm_amd.synth.seeded_param`` by state_dict name, the batch from ``xggm_amd.synth.pretrain_case``
(seeded, not stored).  Model: 2 / 1 / 1 layers, H = 128, 4 heads, vocabulary 263, T = 8, 5 objects of 24 features,
37 object / 11 attribute classes, 19 answers, dropout 0, B = 3.

Case ``full``: every task on, visual_losses 'obj,attr,feat'.  Case ``noqa``: task_qa=False, visual_losses 'obj,feat'.
Stored per case: the losses in the reference's order, the total, answer_score; the encoder's outputs (lang_output,
visn_output, pooled_output) and the gradients that reach them -- what a restatement of the heads alone needs; gradients of
the tied word table, cls.predictions.bias, the object decoders, cls.seq_relationship.weight and one encoder weight; slices
of the same parameters after two clipped (max norm 1) BertAdam steps (lr 1e-3, warmup 0.1, t_total 8) on the same batch.

A gate on the INPUTS: the reference's own float32 run has to agree with its float64 run within 1e-5 (relative, ``rel_err``
for tensors) on every stored quantity; a seed that fails is replaced, the gate is never widened.  Both figures are
recorded in ``meta_json``.  Everything is stored as float64 except tensors of more than 4096 elements (the word table's and
the encoder weight's gradient), which are rounded to float32 to keep the file below the largest fixture already here."""
import inspect
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from xggm_amd import synth  # noqa: E402

GATE = 1e-5
CFG = dict(l_layers=2, x_layers=1, r_layers=1, hidden=128, heads=4, inter=256, vocab=263, max_pos=32, T=8, O=5, F=24,
           n_obj=37, n_attr=11, n_ans=19, B=3)
SEED = 5
CASES = {"full": dict(task_qa=True, visual_losses="obj,attr,feat"), "noqa": dict(task_qa=False, visual_losses="obj,feat")}
# The encoder's HIP attention core is built for heads of 64: H = 128 with 4 heads (heads of 32) cannot run through it.  The
# same two cases are therefore recorded a second time with 2 heads (same shapes, same weights and batch) into
# pretrain_h2.npz: the model-level GPU tests compare with those, the 4-head cases pin the heads and losses.
CASES_H2 = {k + "_h2": dict(v, heads=2) for k, v in CASES.items()}
ENC_WEIGHT = "bert.encoder.x_layers.0.visual_attention.att.query.weight"
GRADS = ["bert.embeddings.word_embeddings.weight", "cls.predictions.bias", "obj_predict_head.decoder_dict.obj.weight",
         "obj_predict_head.decoder_dict.attr.weight", "obj_predict_head.decoder_dict.feat.weight",
         "cls.seq_relationship.weight", ENC_WEIGHT]
SLICE = 256  # leading elements of a parameter kept after the two steps


def load_reference(src):
    for name in ["boto3", "botocore", "botocore.exceptions", "tensorboardX", "h5py", "prefetch_generator"]:
        if name not in sys.modules:
            sys.modules[name] = types.ModuleType(name)
    sys.modules["botocore.exceptions"].ClientError = type("ClientError", (Exception,), {})
    if not hasattr(inspect, "getargspec"):
        inspect.getargspec = inspect.getfullargspec
    sys.path.insert(0, src)
    from lxrt import modeling as M
    from lxrt.optimization import BertAdam
    return M, BertAdam


def rel_err(a, b):
    a, b = torch.as_tensor(a).double().reshape(-1), torch.as_tensor(b).double().reshape(-1)
    return float((a - b).norm() / (b.norm() + 1e-30))


def build(M, case, dt):
    vc = M.VISUAL_CONFIG
    vc.l_layers, vc.x_layers, vc.r_layers = CFG["l_layers"], CFG["x_layers"], CFG["r_layers"]
    vc.obj_id_num, vc.attr_id_num = CFG["n_obj"], CFG["n_attr"]
    vc.set_visual_dims(CFG["F"], 4)
    vc.visual_losses = case["visual_losses"].split(",")
    vc.visual_loss_config = {"obj": (CFG["n_obj"], "ce", (-1,), 1 / 0.15), "attr": (CFG["n_attr"], "ce", (-1,), 1 / 0.15),
                             "feat": (CFG["F"], "l2", (-1, CFG["F"]), 1 / 0.15)}
    bc = M.BertConfig(CFG["vocab"], hidden_size=CFG["hidden"], num_hidden_layers=2, num_attention_heads=case.get("heads", CFG["heads"]),
                      intermediate_size=CFG["inter"], hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0,
                      max_position_embeddings=CFG["max_pos"])
    model = M.LXRTPretraining(bc, task_mask_lm=True, task_matched=True, task_obj_predict=True,
                              visual_losses=case["visual_losses"], task_qa=case["task_qa"], num_answers=CFG["n_ans"])
    sd = model.state_dict()
    tied = "bert.embeddings.word_embeddings.weight"
    new = {k: torch.from_numpy(synth.seeded_param(tied if k == "cls.predictions.decoder.weight" else k, v.shape, SEED))
           for k, v in sd.items()}
    model.load_state_dict(new)
    assert model.cls.predictions.decoder.weight is model.bert.embeddings.word_embeddings.weight
    return model.to(dt).train()


def run(M, BertAdam, case, dt):
    model = build(M, case, dt)
    x = synth.pretrain_case(CFG["B"], CFG["T"], CFG["O"], CFG["F"], CFG["vocab"], CFG["n_obj"], CFG["n_attr"], CFG["n_ans"],
                            seed=SEED)
    t = {k: torch.from_numpy(v) for k, v in x.items()}
    obj_labels = {k: (t[k + "_label"] if k != "feat" else t[k + "_label"].to(dt), t[k + "_conf"].to(dt))
                  for k in ("obj", "attr", "feat")}
    named = dict(model.named_parameters())
    opt = BertAdam(list(model.parameters()), lr=1e-3, warmup=0.1, t_total=8)
    kept = {}
    # the encoder's outputs and the gradients that reach them (what the heads see)
    orig = model.bert.forward

    def spy(*a, **k):
        (lang, visn), pooled = orig(*a, **k)
        lang = lang * 1  # a node of its own: its gradient is what the heads send down, without the pooler's share
        for name, v in (("lang_output", lang), ("visn_output", visn), ("pooled_output", pooled)):
            v.retain_grad()
            kept[name] = v
        return (lang, visn), pooled
    model.bert.forward = spy
    out = {}
    for step in range(2):
        opt.zero_grad()
        total, losses, answer_score = model(t["input_ids"], t["segment_ids"], t["input_mask"], t["masked_lm_labels"],
                                            t["feats"].to(dt), t["boxes"].to(dt), obj_labels, t["matched_label"], t["ans"])
        total.backward()
        if step == 0:
            out["total"] = total.detach().double().reshape(1)
            out["losses"] = losses.detach().double().reshape(-1)
            out["answer_score"] = answer_score.detach().double()
            for name, v in kept.items():
                out[name] = v.detach().double()
                out["d." + name] = v.grad.detach().double()
            for k in GRADS:
                if k in named:
                    out["grad." + k] = named[k].grad.detach().double().clone()
        torch.nn.utils.clip_grad_norm_(model.parameters(), 1.0)  # src/pretrain/lxmert_pretrain.py:315
        opt.step()
    for k in GRADS:
        if k in named:
            out["after2." + k] = named[k].detach().double().reshape(-1)[:SLICE].clone()
    names = {k: list(v.shape) for k, v in model.state_dict().items()}
    return out, names


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    M, BertAdam = load_reference(sys.argv[1])
    torch.manual_seed(0)
    sd_names = {}
    for fname, cases in (("pretrain.npz", CASES), ("pretrain_h2.npz", CASES_H2)):
        arrays, meta = {}, dict(cfg=CFG, seed=SEED, gate=GATE, cases={}, slice=SLICE, grads=GRADS,
                                bert_adam=dict(lr=1e-3, warmup=0.1, t_total=8, max_grad_norm=1.0))
        for cname, case in cases.items():
            o64, names = run(M, BertAdam, case, torch.float64)
            o32, _ = run(M, BertAdam, case, torch.float32)
            fig = {k: rel_err(o32[k], v) for k, v in o64.items()}
            worst = max(fig.values())
            print("%s: float32 vs float64 of the reference, worst %.2e (%s), gate %.0e" % (cname, worst, max(fig, key=fig.get), GATE))
            if worst > GATE:
                sys.exit("case %s misses the gate with seed %d: %s" % (cname, SEED, {k: v for k, v in fig.items() if v > GATE}))
            for k, v in o64.items():
                # the two big gradients (word table, encoder weight) as float32: rounding 6e-8, far below every bound they meet
                arrays["%s.%s" % (cname, k)] = v.numpy().astype(np.float32) if v.numel() > 4096 else v.numpy()
            meta["cases"][cname] = dict(case, f32_vs_f64=fig, worst=worst, n_losses=int(o64["losses"].numel()))
            if "heads" not in case:
                sd_names[cname] = names
        arrays["meta_json"] = np.array(json.dumps(meta))
        path = os.path.join(HERE, fname)
        np.savez_compressed(path, **arrays)
        print("wrote %s: %d arrays, %d bytes" % (path, len(arrays), os.path.getsize(path)))
    with open(os.path.join(HERE, "pretrain_state_dict.json"), "w") as f:
        json.dump(sd_names, f, indent=1, sort_keys=True)

if __name__ == "__main__":
    main()
