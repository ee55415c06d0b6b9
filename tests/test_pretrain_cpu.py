"""CPU-only checks of the pre-training losses: the new entry points are exported and declared, every one of them refuses
bad arguments before anything is launched (no device is present here), the host wrappers refuse CPU tensors,
``synth.pretrain_case`` is reproducible, and the float64 restatement of the heads (tests/pretrain_ref.py) equals what the
reference's own ``LXRTPretraining`` recorded in tests/golden/pretrain.npz."""
import ctypes

import pytest
import torch


NEW_SYMBOLS = ["xggm_mlm_select_f32", "xggm_mlm_select_bf16", "xggm_mlm_scatter_f32", "xggm_mlm_scatter_bf16",
               "xggm_vocab_ce_fwd_f32", "xggm_vocab_ce_fwd_bf16", "xggm_vocab_ce_bwd_f32", "xggm_vocab_ce_bwd_bf16",
               "xggm_visual_loss_fwd_f32", "xggm_visual_loss_fwd_bf16", "xggm_visual_loss_bwd_f32",
               "xggm_visual_loss_bwd_bf16"]


def test_new_symbols_are_exported_and_cite_the_reference():
    from xggm_amd import _lib, ops
    decl = _lib.parse_header()
    for name in NEW_SYMBOLS:
        assert name in decl and hasattr(_lib.lib, name), name
    src = open(_lib.HEADER_PATH).read()
    for cite in ("src/lxrt/modeling.py:955-1061", "src/lxrt/modeling.py:1009-1016", "src/lxrt/modeling.py:1024-1046",
                 "src/pretrain/lxmert_pretrain.py:221-306"):
        assert cite in src, cite
    for name in ("mlm_select", "mlm_scatter", "vocab_ce_fwd", "vocab_ce_bwd", "visual_loss_fwd", "visual_loss_bwd", "vocab_ld"):
        assert callable(getattr(ops, name)), name
    assert "#define XGGM_VOCAB_CE_REG_MAX %d" % ops.VOCAB_CE_REG_MAX in src
    assert "#define XGGM_VISUAL_MAX_JOBS %d" % ops.VISUAL_MAX_JOBS in src
    for name in ("VOCAB_CE_FWD_GRID", "VOCAB_CE_BWD_GRID", "VISUAL_LOSS_GRID", "MLM_SELECT_MAX_ROWS"):
        assert "#define XGGM_%s %d" % (name, getattr(ops, name)) in src, name  # the grids the GPU tests size their cases by
    assert ops.vocab_ld(30522, torch.bfloat16) == 30528 and ops.vocab_ld(30522, torch.float32) == 30524
    assert ops.vocab_ld(8, torch.bfloat16) == 8 and ops.vocab_ld(1, torch.float32) == 4


P = 4096  # a non-null, 16-byte aligned address nothing dereferences: every call below is refused on the host


def _refused(name, a, *extra):
    from xggm_amd import _lib
    rc = getattr(_lib.lib, name)(ctypes.addressof(a) if a is not None else None, *extra, None)
    assert rc != 0, name
    return _lib.lib.xggm_last_error()


@pytest.mark.parametrize("sfx", ["f32", "bf16"])
def test_mlm_select_validation(sfx):
    from xggm_amd import ops

    def good():
        a = ops.MlmSelectArgs()
        a.labels = a.x = a.row_index = a.label = a.n = a.overflow = a.out = P
        a.M, a.H, a.cap, a.V, a.ignore_index = 40, 8, 6, 263, -1
        return a
    name = "xggm_mlm_select_" + sfx
    assert b"null arguments" in _refused(name, None)
    for field in ("labels", "x", "row_index", "label", "n", "overflow", "out"):
        a = good()
        setattr(a, field, None)
        assert b"required" in _refused(name, a), field
    for cap in (0, -3):
        a = good()
        a.cap = cap
        assert b"capacity" in _refused(name, a)
    a = good()
    a.H = 3  # rows that are no multiple of 16 bytes
    assert b"16" in _refused(name, a)
    a = good()
    a.V = 0
    assert b"bad shape" in _refused(name, a)
    from xggm_amd import _lib
    rc = getattr(_lib.lib, "xggm_mlm_scatter_" + sfx)(P, P, P, P, 40, 8, 0, None)
    assert rc != 0 and b"capacity" in _lib.lib.xggm_last_error()
    rc = getattr(_lib.lib, "xggm_mlm_scatter_" + sfx)(None, P, P, P, 40, 8, 6, None)
    assert rc != 0 and b"required" in _lib.lib.xggm_last_error()


@pytest.mark.parametrize("sfx,gran", [("f32", 4), ("bf16", 8)])
@pytest.mark.parametrize("way", ["fwd", "bwd"])
def test_vocab_ce_validation(sfx, gran, way):
    from xggm_amd import ops

    def good():
        a = ops.VocabCeArgs()
        a.logits = a.label = a.n = a.loss = a.ws = a.save = a.gout = P
        a.cap, a.V, a.ld = 6, 263, 264
        return a
    name = "xggm_vocab_ce_%s_%s" % (way, sfx)
    assert b"null arguments" in _refused(name, None)
    for field in ("logits", "label", "n", "save") + (("loss", "ws") if way == "fwd" else ("gout",)):
        a = good()
        setattr(a, field, None)
        assert b"required" in _refused(name, a), field
    for cap in (0, -1):
        a = good()
        a.cap = cap
        assert b"capacity" in _refused(name, a)
    a = good()
    a.ld = 256  # ld < V
    assert b"shorter than V" in _refused(name, a)
    a = good()
    a.ld = 264 + gran // 2  # rows that do not start 16-byte aligned
    assert b"multiple of" in _refused(name, a)
    a = good()
    a.logits = P + 4
    assert b"aligned" in _refused(name, a)
    a = good()
    a.V = 0
    assert b"vocabulary" in _refused(name, a)


@pytest.mark.parametrize("sfx", ["f32", "bf16"])
@pytest.mark.parametrize("way", ["fwd", "bwd"])
def test_visual_loss_validation(sfx, way):
    from xggm_amd import ops

    def good(n_jobs=3):
        a = ops.VisualLossArgs()
        for q in range(ops.VISUAL_MAX_JOBS):
            j = a.job[q]
            j.kind, j.W = (ops.VISUAL_CE, ops.VISUAL_CE, ops.VISUAL_L2)[q], (1600, 400, 2048)[q]
            j.scores = j.label_index = j.target = j.mask_conf = j.loss = j.d_score = P
            j.weight = 1.0
        a.n_jobs, a.R, a.ignore_index = n_jobs, 72, -1
        a.ws = a.save = a.gout = P
        return a
    name = "xggm_visual_loss_%s_%s" % (way, sfx)
    assert b"null arguments" in _refused(name, None)
    for n_jobs in (0, 4, -1):  # more than three jobs, or none
        assert b"jobs" in _refused(name, good(n_jobs))
    a = good()
    a.job[1].kind = 7
    assert b"unknown kind 7" in _refused(name, a)
    a = good(1)
    a.job[2].kind = 7  # a job behind n_jobs is not looked at ...
    a.R = 0            # ... and the row count is
    assert b"row count" in _refused(name, a)
    a = good()
    a.job[0].W = 0
    assert b"width" in _refused(name, a)
    for q, field in ((0, "scores"), (2, "mask_conf"), (1, "label_index"), (2, "target"),
                     (0, "loss" if way == "fwd" else "d_score")):
        a = good()
        setattr(a.job[q], field, None)
        assert b"job %d" % q in _refused(name, a), field
    for field in ("save", "ws" if way == "fwd" else "gout"):
        a = good()
        setattr(a, field, None)
        assert b"required" in _refused(name, a), field


def test_host_wrappers_check_operands_and_refuse_cpu_tensors():
    from xggm_amd import ops
    labels = torch.zeros(6, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.mlm_select(labels, torch.zeros(6, 8), 4, 263)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.vocab_ce_fwd(torch.zeros(4, 264), torch.zeros(4, dtype=torch.int32), torch.zeros(1, dtype=torch.int32), 263)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.visual_loss_fwd([(ops.VISUAL_CE, torch.zeros(4, 7), labels[:4], torch.zeros(4), 1.0)])
    with pytest.raises(ValueError, match="jobs"):
        ops.visual_loss_fwd([])
    with pytest.raises(ValueError, match="jobs"):
        ops.visual_loss_fwd([None] * 4)
    with pytest.raises(ValueError, match="unknown kind"):
        ops.visual_loss_fwd([(9, torch.zeros(4, 7), labels[:4], torch.zeros(4), 1.0)])


# ------------------------------------------------------------------------------------------------ the restatement's pin
def _golden():
    import json
    from helpers import load_golden
    g = load_golden("pretrain")
    return g, json.loads(str(g["meta_json"]))


def _golden_inputs(meta):
    import numpy as np
    from xggm_amd import synth
    c = meta["cfg"]
    x = synth.pretrain_case(c["B"], c["T"], c["O"], c["F"], c["vocab"], c["n_obj"], c["n_attr"], c["n_ans"], seed=meta["seed"])
    y = synth.pretrain_case(c["B"], c["T"], c["O"], c["F"], c["vocab"], c["n_obj"], c["n_attr"], c["n_ans"], seed=meta["seed"])
    assert sorted(x) == sorted(y) and all(np.array_equal(x[k], y[k]) for k in x)  # reproducible from its seed
    other = synth.pretrain_case(c["B"], c["T"], c["O"], c["F"], c["vocab"], c["n_obj"], c["n_attr"], c["n_ans"], seed=meta["seed"] + 1)
    assert not np.array_equal(x["feats"], other["feats"])
    return x


def test_pretrain_case_is_reproducible_and_holds_every_edge():
    _, meta = _golden()
    x = _golden_inputs(meta)
    lab, mask = x["masked_lm_labels"], x["input_mask"]
    assert (lab[0] == -1).all()                                   # a sample with no masked token
    last = int(mask[1].sum()) - 1
    assert lab[1, 1] != -1 and lab[1, last] != -1                 # position 1 and the last real token
    assert (lab[mask == 0] == -1).all()
    assert set(x["matched_label"].tolist()) == {0, 1} and -1 in x["ans"].tolist()
    assert x["obj_label"][0, 0] == -1 and x["obj_conf"][0, 0] > 0   # an ignored object label under a positive confidence
    assert all(x[k + "_conf"][0, -1] == 0 for k in ("obj", "attr", "feat"))  # a row of confidence 0


@pytest.mark.parametrize("case", ["full", "noqa"])
def test_restatement_equals_the_reference_recorded_results(case):
    """tests/pretrain_ref.heads on the encoder outputs the reference recorded == the reference's own losses, answer_score
    and gradients (tests/golden/pretrain.npz, float64), within 2e-5; the word table's recorded gradient also holds the
    embedding's rows, so the decoder's share is checked through cls.predictions.bias and d lang_output instead"""
    import pretrain_ref as R
    from helpers import rel_err
    from xggm_amd import synth
    g, meta = _golden()
    cfg, c = meta["cfg"], meta["cases"][case]
    x = _golden_inputs(meta)
    import json
    import os
    from helpers import GOLDEN
    names = json.load(open(os.path.join(GOLDEN, "pretrain_state_dict.json")))[case]
    tied = "bert.embeddings.word_embeddings.weight"
    assert names["cls.predictions.decoder.weight"] == names[tied] == [cfg["vocab"], cfg["hidden"]]
    P = {k: torch.from_numpy(synth.seeded_param(tied if k == "cls.predictions.decoder.weight" else k, shp, meta["seed"]))
         for k, shp in names.items() if not k.startswith("bert.")}
    losses_on = c["visual_losses"].split(",")
    assert ("answer_head.logit_fc.3.weight" in P) == c["task_qa"]
    assert [k.split(".")[2] for k in sorted(P) if k.startswith("obj_predict_head.decoder_dict.") and k.endswith("weight")] \
        == sorted(losses_on)
    t = {k: torch.from_numpy(g["%s.%s" % (case, k)]) for k in R.HEAD_INPUTS}
    for k in ("masked_lm_labels", "matched_label", "ans"):
        t[k] = torch.from_numpy(x[k])
    for k in losses_on:
        t[k + "_label"], t[k + "_conf"] = torch.from_numpy(x[k + "_label"]), torch.from_numpy(x[k + "_conf"])
    vlc = {"obj": (cfg["n_obj"], "ce", (-1,), 1 / 0.15), "attr": (cfg["n_attr"], "ce", (-1,), 1 / 0.15),
           "feat": (cfg["F"], "l2", (-1, cfg["F"]), 1 / 0.15)}
    out = R.heads(P, t, task_qa=c["task_qa"], visual_losses_on=losses_on, visual_loss_config=vlc)
    want = g[case + ".losses"]
    assert len(out["losses"]) == c["n_losses"] == 2 + len(losses_on) + int(c["task_qa"])
    errs = {"total": abs(out["total"] - float(g[case + ".total"][0])) / abs(float(g[case + ".total"][0]))}
    for i, (a, b) in enumerate(zip(out["losses"], want)):
        errs["loss%d" % i] = abs(a - float(b)) / abs(float(b))
    errs["answer_score"] = rel_err(out["answer_score"], torch.from_numpy(g[case + ".answer_score"]))
    for k in R.HEAD_INPUTS:
        errs["d." + k] = rel_err(out["grads"][k], torch.from_numpy(g["%s.d.%s" % (case, k)]))
    for k in meta["grads"]:
        if k.startswith("bert.") or ("%s.grad.%s" % (case, k)) not in g.files:
            continue
        errs["grad." + k] = rel_err(out["grads"][k], torch.from_numpy(g["%s.grad.%s" % (case, k)]))
    print(case, {k: "%.1e" % v for k, v in errs.items()})
    assert "grad.cls.predictions.bias" in errs and "grad.obj_predict_head.decoder_dict.feat.weight" in errs
    assert max(errs.values()) <= 2e-5, errs
    assert c["worst"] <= meta["gate"] == 1e-5  # the reference's own float32 run against its float64 run


# ------------------------------------------------------------------------------------------------ the module classes
def _tiny_model(case="full", heads=2, **kw):
    """LXRTPretraining at the fixture's shapes; 2 heads (the HIP attention core is built for heads of 64; the head
    count changes no shape), seeded weights by state_dict name"""
    import json
    import os
    from helpers import GOLDEN, load_golden
    from xggm_amd import synth
    from xggm_amd.lxrt import modeling as M
    meta = json.loads(str(load_golden("pretrain")["meta_json"]))
    cfg, c = meta["cfg"], meta["cases"][case]
    vc = M.VISUAL_CONFIG
    saved = dict(vc.__dict__)
    vc.l_layers, vc.x_layers, vc.r_layers = cfg["l_layers"], cfg["x_layers"], cfg["r_layers"]
    vc.obj_id_num, vc.attr_id_num = cfg["n_obj"], cfg["n_attr"]
    vc.set_visual_dims(cfg["F"], 4)
    vc.visual_losses = c["visual_losses"].split(",")
    vc.visual_loss_config = {"obj": (cfg["n_obj"], "ce", (-1,), 1 / 0.15), "attr": (cfg["n_attr"], "ce", (-1,), 1 / 0.15),
                             "feat": (cfg["F"], "l2", (-1, cfg["F"]), 1 / 0.15)}
    bc = M.BertConfig(cfg["vocab"], hidden_size=cfg["hidden"], num_attention_heads=heads, intermediate_size=cfg["inter"],
                      max_position_embeddings=cfg["max_pos"])
    model = M.LXRTPretraining(bc, visual_losses=c["visual_losses"], task_qa=c["task_qa"], num_answers=cfg["n_ans"], **kw)
    tied = "bert.embeddings.word_embeddings.weight"
    model.load_state_dict({k: torch.from_numpy(synth.seeded_param(tied if k == "cls.predictions.decoder.weight" else k,
                                                                  v.shape, meta["seed"]))
                           for k, v in model.state_dict().items()})
    names = json.load(open(os.path.join(GOLDEN, "pretrain_state_dict.json")))[case]
    return model, names, meta, bc, saved


def _restore_visual_config(saved):
    from xggm_amd.lxrt import modeling as M
    M.VISUAL_CONFIG.__dict__.clear()
    M.VISUAL_CONFIG.__dict__.update(saved)


@pytest.mark.parametrize("case", ["full", "noqa"])
def test_state_dict_is_the_reference_contract(case):
    """names and shapes of LXRTPretraining.state_dict() == what the reference's own object reported
    (tests/golden/pretrain_state_dict.json), for both task selections"""
    from xggm_amd.lxrt import modeling as M
    model, names, meta, _, saved = _tiny_model(case)
    try:
        sd = model.state_dict()
        assert sorted(sd) == sorted(names)
        assert all(list(sd[k].shape) == names[k] for k in names)
        assert ("answer_head.logit_fc.3.weight" in sd) == (case == "full")
        for cls in ("BertPredictionHeadTransform", "BertLMPredictionHead", "BertVisualObjHead", "BertVisualAnswerHead",
                    "BertPreTrainingHeads", "LXRTPretraining"):
            assert hasattr(M, cls), cls
        vc = M.VisualConfig()
        assert (vc.obj_id_num, vc.attr_id_num, vc.visual_losses) == (1600, 400, ['obj', 'attr', 'feat'])
        assert vc.visual_loss_config == {'obj': (1600, 'ce', (-1,), 1 / 0.15), 'attr': (400, 'ce', (-1,), 1 / 0.15),
                                         'feat': (2048, 'l2', (-1, 2048), 1 / 0.15)}
    finally:
        _restore_visual_config(saved)


def test_decoder_is_the_word_table_and_the_arena_counts_it_once():
    from xggm_amd import arena
    model, names, _, _, saved = _tiny_model()
    try:
        dec, emb = model.cls.predictions.decoder.weight, model.bert.embeddings.word_embeddings.weight
        assert dec is emb and dec.data_ptr() == emb.data_ptr()
        named = list(model.named_parameters())
        order, groups, info, total = arena.layout(named, arena.default_group_of, model)
        assert "bert.embeddings.word_embeddings.weight" in info and "cls.predictions.decoder.weight" not in info
        assert sum(v[1] for v in info.values()) == sum(p.numel() for p in set(model.parameters()))
        sd_numel = sum(v.numel() for v in model.state_dict().values())
        assert sd_numel - sum(v[1] for v in info.values()) == emb.numel()  # state_dict names the table twice, the arena holds it once
        assert info["bert.embeddings.word_embeddings.weight"][3]  # vector class: its two gradients are added in place
        assert model.mlm_capacity is None and model.mlm_overflow is None
    finally:
        _restore_visual_config(saved)


def test_snapshot_loads_through_the_fine_tuning_loaders(tmp_path, monkeypatch):
    """torch.save(LXRTPretraining.state_dict()) -> ``lxrt_encoder.load`` and ``load_lxmert_qa`` of a VQAModel: the encoder
    arrives whole, the answer head is copied, ``logit_fc.3`` gets the snapshot's row of every answer the pre-training
    table knows and zero rows for the rest"""
    import json
    import os
    from xggm_amd import param
    from xggm_amd.pretrain.qa_answer_table import AnswerTable, load_lxmert_qa
    from xggm_amd.vqa.vqacpv2_model import VQAModel
    model, names, meta, bc, saved = _tiny_model()
    try:
        cfg = meta["cfg"]
        os.makedirs(tmp_path / "data" / "lxmert")
        pre = ["ans%d" % i for i in range(cfg["n_ans"])]
        (tmp_path / "data" / "lxmert" / "all_ans.json").write_text(json.dumps([{"ans": a, "dsets": ["vqa"]} for a in pre]))
        torch.save(model.state_dict(), str(tmp_path / "snap_LXRT.pth"))
        monkeypatch.chdir(tmp_path)
        a = param.parse_args(["--llayers", str(cfg["l_layers"]), "--xlayers", str(cfg["x_layers"]), "--rlayers",
                              str(cfg["r_layers"])])
        labels = ["ans7", "never seen", "ans0", "ans18", "nor this"]
        sd = model.state_dict()
        for how in ("encoder", "qa"):
            vqa = VQAModel(len(labels), args=a, config=bc)
            if how == "encoder":
                vqa.lxrt_encoder.load(str(tmp_path / "snap"))
            else:
                load_lxmert_qa(str(tmp_path / "snap"), vqa, labels, AnswerTable())
            enc = vqa.lxrt_encoder.model.state_dict()
            assert sorted(enc) == sorted(k for k in sd if k.startswith("bert."))
            assert all(torch.equal(enc[k], sd[k]) for k in enc)
        own = vqa.state_dict()
        for k in ("0.weight", "0.bias", "2.weight", "2.bias"):
            assert torch.equal(own["logit_fc." + k], sd["answer_head.logit_fc." + k]), k
        for row, src in ((0, 7), (2, 0), (3, 18)):
            assert torch.equal(own["logit_fc.3.weight"][row], sd["answer_head.logit_fc.3.weight"][src])
            assert torch.equal(own["logit_fc.3.bias"][row], sd["answer_head.logit_fc.3.bias"][src])
        for row in (1, 4):
            assert not own["logit_fc.3.weight"][row].any() and not own["logit_fc.3.bias"][row].any()
    finally:
        _restore_visual_config(saved)


def test_fixture_batch_has_feature_differences_on_both_sides_of_one():
    """the SmoothL1 switch at |d| = 1: under a positive confidence the reference-shaped predictions of the fixture lie on
    both sides of it"""
    import pretrain_ref as R
    from xggm_amd import synth
    g, meta = _golden()
    cfg = meta["cfg"]
    x = _golden_inputs(meta)
    import json
    import os
    from helpers import GOLDEN
    names = json.load(open(os.path.join(GOLDEN, "pretrain_state_dict.json")))["full"]
    P = {k: torch.from_numpy(synth.seeded_param(k, shp, meta["seed"])).double() for k, shp in names.items()
         if k.startswith("obj_predict_head.")}
    h = R.transform(torch.from_numpy(g["full.visn_output"]).reshape(-1, cfg["hidden"]), P, "obj_predict_head.transform.")
    s = h @ P["obj_predict_head.decoder_dict.feat.weight"].t() + P["obj_predict_head.decoder_dict.feat.bias"]
    d = (s - torch.from_numpy(x["feat_label"]).double().reshape(-1, cfg["F"])).abs()[torch.from_numpy(x["feat_conf"]).reshape(-1) > 0]
    assert int((d < 1).sum()) > 10 and int((d > 1).sum()) > 10
