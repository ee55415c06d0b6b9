"""What scoring a sweep on the device saves, and what the fine-tuning driver costs per iteration; one process, GPU only:

  (a) a synthetic sweep at VQA-CP v2 test size (219 928 samples, K = 10 label slots, A = 2274 answers) whose answers lie in an
      ``AnswerLog``.  Leg A is the host path the reference takes four times per epoch: ``log.read()`` + ``to_quesid2ans`` +
      ``VQAEvaluator.evaluate``; leg B is ``AnswerLog.score_store`` (one launch, one read-back of three words) with the
      keep mask of the data set order.  Legs alternate and repeat; host clock around calls that end in a synchronise
      themselves; the kernel alone is timed with device events around launches replayed from one graph;
  (b) the full-size batch-32 bf16 iteration: ``CapturedTrainer.iteration`` on the static batch beside an epoch of
      ``VQA.train`` (``load_resident`` + ``iteration`` + the per-epoch reads and the train score; no validation tuple) on
      the SAME engine, legs alternating, host clock around windows that end in a synchronise.

    python tools/bench_sweep_score.py [--out profiles/finetune/sweep_score_ab.txt] [--repeats 5] [--epoch-batches 24]
"""
import argparse
import os
import random
import statistics
import sys
import tempfile
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

N_TEST, K, A = 219928, 10, 2274


def _stats(v):
    return "median %.3f (min %.3f, max %.3f)" % (statistics.median(v), min(v), max(v))


def leg_score(out, dev, repeats):
    from xggm_amd import ops
    from xggm_amd.answers import last_occurrence_mask, to_quesid2ans
    from xggm_amd.engine import AnswerLog
    from xggm_amd.vqa.vqacpv2_data import VQADataset, VQAEvaluator
    rng = np.random.default_rng(0)
    used = rng.integers(1, K + 1, N_TEST)
    # K distinct labels per sample: an arithmetic progression mod A (stride * K < A), the slots behind `used` unused
    lab = (rng.integers(0, A, (N_TEST, 1)) + np.arange(K)[None] * rng.integers(1, A // K, (N_TEST, 1))) % A
    live = np.arange(K)[None] < used[:, None]
    q_label = np.where(live, lab, -1).astype(np.int32)
    q_score = np.where(live, rng.choice(np.asarray([0.3, 0.6, 0.9, 1.0], dtype=np.float32), size=(N_TEST, K)), 0).astype(np.float32)
    data = [{"question_id": s, "image_id": 0, "label": q_label[s, :used[s]].tolist(), "score": q_score[s, :used[s]].tolist(),
             "question": ""} for s in range(N_TEST)]
    l2a = ["a%d" % k for k in range(A)]
    dset = VQADataset("test", data=data, ans2label={a: k for k, a in enumerate(l2a)}, label2ans=l2a)
    ev = VQAEvaluator(dset)
    qids = list(range(N_TEST))
    store = types.SimpleNamespace(tables=dict(q_label=torch.from_numpy(q_label).to(dev), q_score=torch.from_numpy(q_score).to(dev)), G=0)
    keep = torch.from_numpy(last_occurrence_mask(qids)).to(dev)
    log = AnswerLog(N_TEST, dev, with_scores=False)
    answers = rng.integers(0, A, N_TEST)
    hit = rng.random(N_TEST) < 0.5
    answers[hit] = q_label[hit, 0]
    log.labels.copy_(torch.from_numpy(answers).to(dev))
    log.cursor.fill_(N_TEST)
    log.count = N_TEST

    def host():
        labels = log.read()[0]
        return ev.evaluate(to_quesid2ans(qids, labels, l2a))

    def device():
        return log.score_store(store, keep=keep)["score"]

    a, b = host(), device()
    out("(a) sweep of %d samples, K=%d, A=%d: host score %.9f, device score %.9f (difference %.2e)" % (N_TEST, K, A, a, b, abs(a - b)))
    ms = {"A": [], "B": []}
    for r in range(repeats + 1):  # the first round warms both legs up
        for name, fn in (("A", host), ("B", device)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            if r:
                ms[name].append(1000.0 * (time.perf_counter() - t0))
    out("(a) leg A  log.read() + to_quesid2ans + evaluator.evaluate: %s ms per sweep, %d repeats" % (_stats(ms["A"]), repeats))
    out("(a) leg B  AnswerLog.score_store (launch + read-back + decode): %s ms per sweep, %d repeats" % (_stats(ms["B"]), repeats))
    # the kernel alone: 64 launches as one graph between device events
    ws, res = ops.answer_score_workspace(N_TEST, 0, dev), torch.zeros(3, dtype=torch.int64, device=dev)
    launches = 64

    def issue():
        for _ in range(launches):
            ops.answer_score(log.labels, store.tables["q_label"], store.tables["q_score"], N_TEST, keep=keep, cursor=log.cursor, out=res, ws=ws)

    issue()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        issue()
    us = []
    for r in range(repeats + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        graph.replay()
        e1.record()
        e1.synchronize()
        if r:
            us.append(1000.0 * e0.elapsed_time(e1) / launches)
    nbytes = N_TEST * (8 + 1 + K * 4 + 4)  # label, keep, the label slots and one score per position (an upper bound: a match stops the row)
    out("(a) xggm_answer_score alone, %d launches replayed from one graph: %s us per launch; <= %d bytes read -> %.0f GB/s at the median"
        % (launches, _stats(us), nbytes, nbytes / statistics.median(us) / 1e3))


def leg_driver(out, dev, repeats, epoch_batches):
    from xggm_amd import param
    from xggm_amd.lxrt.modeling import BertConfig, VISUAL_CONFIG
    from xggm_amd.tools.resident import ResidentDataset
    from xggm_amd.vqa.vqacpv2 import VQA
    from xggm_amd.vqa.vqacpv2_data import VQAEvaluator
    from xggm_amd.vqa.vqacpv2_model import VQAModel
    bargs = bench.parse(["--steps", "1"])
    VISUAL_CONFIG.set_visual_dims(2048, 4)
    tmp_out = tempfile.mkdtemp(prefix="xggm_sweep_")
    a = param.parse_args(["--bs", str(bargs.batch), "--epochs", "1", "--lr", "1e-6", "--seed", str(bargs.seed), "--output", tmp_out])
    torch.manual_seed(bargs.seed)
    model = VQAModel(bargs.answers, gnn="GCN", n_layers=2, args=a, config=BertConfig(30522), compute_dtype=torch.bfloat16,
                     tokenizer=bench.synthetic_tokenizer())
    model.seed = bargs.seed
    model = model.to(dev)
    loader, _, tmp = bench.make_loader(model, bargs, dev, n_batches=epoch_batches)
    store = ResidentDataset(loader.ds, model.lxrt_encoder.batcher, dev, batch_size=bargs.batch)
    tup = (loader.ds.raw_dataset, store, VQAEvaluator(loader.ds.raw_dataset))
    drv = VQA(model, tup, None, args=a)
    random.seed(0)
    drv.train(tup, None)  # builds and warms the engine
    tr = drv.trainer
    rng = random.Random(0)

    def static():
        tr.answer_log.reset()  # the plain passes append to the epoch-sized log, which the driver's epoch has filled
        for _ in range(epoch_batches):
            tr.iteration("rel" if rng.randint(1, 10) <= a.delta else "node")
        tr.train_log.reset()   # the driver expects to find its own epoch's records only

    def driver():
        drv.train(tup, None)

    ms = {"static": [], "driver": []}
    for r in range(repeats + 1):
        for name, fn in (("static", static), ("driver", driver)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if r:
                ms[name].append(1000.0 * (time.perf_counter() - t0) / epoch_batches)
    out("(b) batch %d bf16 full-size, %d iterations per window, %d repeats: CapturedTrainer.iteration on the static batch %s ms per iteration"
        % (bargs.batch, epoch_batches, repeats, _stats(ms["static"])))
    out("(b) VQA.train, one epoch (load_resident + iteration, the epoch's TrainLog read and train score included): %s ms per iteration; "
        "driver - static at the medians: %+.3f ms (spread of the static leg, max - min: %.3f ms)"
        % (_stats(ms["driver"]), statistics.median(ms["driver"]) - statistics.median(ms["static"]), max(ms["static"]) - min(ms["static"])))
    import shutil
    shutil.rmtree(tmp, ignore_errors=True)
    shutil.rmtree(tmp_out, ignore_errors=True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "finetune", "sweep_score_ab.txt"))
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--epoch-batches", type=int, default=24)
    p.add_argument("--only", choices=["a", "b"], default=None)
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sweep_score: needs a GPU (nothing here is measured on a CPU)")
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)

    out("# python tools/bench_sweep_score.py --repeats %d --epoch-batches %d   (%s)" % (a.repeats, a.epoch_batches, torch.cuda.get_device_name(0)))
    if a.only != "b":
        leg_score(out, dev, a.repeats)
    if a.only != "a":
        leg_driver(out, dev, a.repeats, a.epoch_batches)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
