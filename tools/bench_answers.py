"""What the device-resident answer log costs and what it buys (xggm_answer_pick_f32, engine.AnswerLog).
  python tools/bench_answers.py [--out profiles/r06_experiments/answers.txt] [--reps 15]
Three steps, each a fresh child process under its own time limit; the first one that fails ends the run:
  kernel   xggm_answer_pick_f32 inside replayed graphs (64 launches per graph, four replays per event-timed window, time
           per launch) at (B, A) = (32, 2274), (92, 2274), (512, 3129), without and with a target, beside the ATen
           ``logit.max(1)`` it displaces on the same tensors, captured the same way.  The variants alternate; every variant is measured by TWO
           graphs of its own, and the difference between such twins is the A/A spread a difference has to exceed.
  replay   one replay of the full-size predictor (9/5/5 LXMERT, batch 512, inputs resident): the plain CapturedPredictor
           -- the parent's graph, ATen arg-max and all, which this tree does not touch -- twice (A/A) and the logging one.
  sweep    wall time of ``predict`` over a 40-batch in-memory loader (pinned host batches) at batch 512: today's path
           with its ``.cpu()`` per batch against the log with its one read-back, alternating.
Medians and ranges (min .. max) over --reps rounds after warm-up."""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STEPS = (("kernel", 240), ("replay", 420), ("sweep", 600))
PER_GRAPH, REPLAYS = 64, 4  # launches per graph, replays per timed window (the first replay's launch latency is diluted)


def stat(xs):
    return "%8.3f  (%.3f .. %.3f)" % (statistics.median(xs), min(xs), max(xs))


def full_model():
    import torch
    from xggm_amd import param
    from xggm_amd.lxrt.modeling import BertConfig, VISUAL_CONFIG
    from xggm_amd.vqa.vqacpv2_model import VQAModel
    VISUAL_CONFIG.set_visual_dims(2048, 4)
    a = param.parse_args(["--llayers", "9", "--xlayers", "5", "--rlayers", "5"])
    torch.manual_seed(0)
    return VQAModel(2274, args=a, config=BertConfig(30522), compute_dtype=torch.bfloat16).to("cuda")


def step_kernel(reps):
    import torch
    from xggm_amd import ops
    from xggm_amd.engine import AnswerLog
    print("kernel: us per launch inside replayed graphs of %d launches (%d replays per timed window), median (min .. max) of "
          "%d rounds" % (PER_GRAPH, REPLAYS, reps))
    for B, A in ((32, 2274), (92, 2274), (512, 3129)):
        g = torch.Generator(device="cuda").manual_seed(B)
        x = torch.randn(B, A, device="cuda", generator=g)
        t = torch.rand(B, A, device="cuda", generator=g)
        log = AnswerLog(REPLAYS * PER_GRAPH * B, "cuda")
        ops.answer_pick(x, log)  # the workspace exists before any capture
        want = x.cpu().max(1)[1]
        assert torch.equal(log.read()[0], want)

        def capture(fn):
            graph = torch.cuda.CUDAGraph()
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                fn()
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            keep = []
            with torch.cuda.graph(graph):
                for _ in range(PER_GRAPH):
                    keep.append(fn())
            return graph, keep

        variants = {}
        for name, fn in (("pick", lambda: ops.answer_pick(x, log)), ("pick+target", lambda: ops.answer_pick(x, log, target=t)),
                         ("aten max(1)", lambda: x.max(1))):
            log.reset()
            variants[name] = [capture(fn), capture(fn)]
        times = {(n, k): [] for n in variants for k in (0, 1)}
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for r in range(reps + 3):
            for n in variants:
                for k in (0, 1):
                    log.reset()
                    a.record()
                    for _ in range(REPLAYS):
                        variants[n][k][0].replay()
                    b.record()
                    torch.cuda.synchronize()
                    if r >= 3:
                        times[(n, k)].append(a.elapsed_time(b) * 1e3 / (PER_GRAPH * REPLAYS))
        labels = log.read()[0]
        assert torch.equal(labels[:B], want) and torch.equal(variants["aten max(1)"][0][1][0][1].cpu(), want)
        print("  B = %d, A = %d (%.1f KB per row, %.2f MB)" % (B, A, A * 4 / 1e3, B * A * 4 / 1e6))
        for n in variants:
            m0, m1 = statistics.median(times[(n, 0)]), statistics.median(times[(n, 1)])
            print("    %-12s %s | twin %s | A/A %+.3f" % (n, stat(times[(n, 0)]), stat(times[(n, 1)]), m1 - m0))
        med = {n: statistics.median(times[(n, 0)] + times[(n, 1)]) for n in variants}
        print("    pick - aten: %+.3f us, pick+target - aten: %+.3f us" % (med["pick"] - med["aten max(1)"],
                                                                          med["pick+target"] - med["aten max(1)"]), flush=True)


def _inputs(B):
    import torch
    from xggm_amd import synth
    b = synth.vqa_batch(B, A=2274, seed=5)
    feats, boxes = torch.from_numpy(b["feats"]), torch.from_numpy(b["boxes"])
    sent = tuple(torch.from_numpy(b[k]) for k in ("input_ids", "input_mask", "segment_ids"))
    return feats, boxes, sent


def step_replay(reps):
    import torch
    from xggm_amd.engine import AnswerLog, CapturedPredictor
    B = 512
    model = full_model()
    feats, boxes, sent = _inputs(B)
    feats, boxes, sent = feats.cuda(), boxes.cuda(), tuple(s.cuda() for s in sent)
    log = AnswerLog(B * 8, "cuda", with_scores=False)
    preds = {"plain": CapturedPredictor(model, B), "plain twin": CapturedPredictor(model, B),
             "logging": CapturedPredictor(model, B, log=log)}
    for p in preds.values():
        p.push(feats, boxes, sent)
    torch.cuda.synchronize()
    times = {n: [] for n in preds}
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for r in range(reps + 3):
        for n, p in preds.items():
            log.reset()
            a.record()
            for _ in range(4):
                p.graph.replay()
            b.record()
            torch.cuda.synchronize()
            if r >= 3:
                times[n].append(a.elapsed_time(b) / 4)
    assert torch.equal(log.read()[0][:B], preds["plain"].label.cpu())
    print("replay: ms per replay of the full-size predictor at batch %d, median (min .. max) of %d rounds of 4" % (B, reps))
    for n in preds:
        print("    %-11s %s" % (n, stat(times[n])))
    med = {n: statistics.median(times[n]) for n in preds}
    print("    A/A (plain twin - plain): %+.4f ms; logging - plain: %+.4f ms" % (med["plain twin"] - med["plain"],
                                                                                med["logging"] - med["plain"]), flush=True)


def step_sweep(reps):
    import torch
    from xggm_amd.engine import AnswerLog, CapturedPredictor
    from xggm_amd.vqa.vqacpv2 import predict
    B, n_batches = 512, 40
    model = full_model()
    feats, boxes, sent = _inputs(B)
    slots = [(feats.clone().pin_memory(), boxes.clone().pin_memory(), tuple(s.clone().pin_memory() for s in sent))
             for _ in range(2)]

    class DSet:
        label2ans = ["ans%d" % i for i in range(2274)]

    def loader():
        for i in range(n_batches):
            f, bx, s = slots[i % 2]
            yield torch.arange(i * B, (i + 1) * B), f, bx, s

    log = AnswerLog(B * n_batches, "cuda", with_scores=False)
    preds = {"per-batch .cpu()": CapturedPredictor(model, B), "answer log": CapturedPredictor(model, B, log=log)}
    reps = max(3, reps // 3)
    times, out = {n: [] for n in preds}, {}
    for r in range(reps + 1):
        for n, p in preds.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out[n] = predict(model, (DSet, loader(), None), predictor=p)
            torch.cuda.synchronize()
            if r >= 1:
                times[n].append((time.perf_counter() - t0) * 1e3)
    assert out["per-batch .cpu()"] == out["answer log"] and len(out["answer log"]) == B * n_batches
    print("sweep: ms of wall time per %d-batch sweep at batch %d (pinned in-memory loader), median (min .. max) of %d"
          % (n_batches, B, reps))
    for n in preds:
        print("    %-17s %s   = %.3f ms per batch" % (n, stat(times[n]), statistics.median(times[n]) / n_batches))
    print("    answer log - per-batch .cpu(): %+.2f ms per sweep"
          % (statistics.median(times["answer log"]) - statistics.median(times["per-batch .cpu()"])), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r06_experiments", "answers.txt"))
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--step", choices=[s for s, _ in STEPS])
    args = ap.parse_args()
    if args.step:
        import torch
        if not torch.cuda.is_available():
            sys.exit("bench_answers: no GPU -- nothing is measured without one")
        {"kernel": step_kernel, "replay": step_replay, "sweep": step_sweep}[args.step](args.reps)
        return
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        for step, limit in STEPS:
            r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", step,
                                "--reps", str(args.reps)], capture_output=True, text=True)
            f.write(r.stdout)
            f.flush()
            sys.stdout.write(r.stdout)
            if r.returncode != 0:
                msg = "step %s ended with status %d; nothing further was started\n%s" % (step, r.returncode, r.stderr[-2000:])
                f.write(msg)
                sys.exit(msg)


if __name__ == "__main__":
    main()
