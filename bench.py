#!/usr/bin/env python3
"""Benchmark of the X-GGM training iteration on MI355X.

    python bench.py --gpus N --steps K --warmup W
    (N > 1 without a launcher: this process spawns the N ranks itself, BEFORE any GPU call;
     under `python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N ...` the ranks
     are already there and RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* come from the environment)

One "step" = one training iteration of the reference loop (src/vqa/vqacpv2.py:164-254): a
plain-VQA pass and a graph-generative pass, EACH a full forward + backward + grad-norm clip +
BertAdam update of the 220.8 M-parameter LXMERT(9/5/5) + GCNx2 generator + heads model, on a
synthetic VQA-CP-v2-shaped batch of 32 samples per GPU (36 objects x 2048-d, 20 tokens,
A = 2274), bf16 storage / fp32 accumulate, dropout on.  Weak scaling: 32 samples per rank,
gradients averaged over RCCL.  Prints ONE JSON line (rank 0).

    --order gqa        the GQA-OOD loop (src/gqa/gqa_ood.py:165-292): GGM pass first, KL weight 12, A = 1842
    --dtype fp8        e4m3 operands for the forward QKV / FFN products (BASELINE configs[4]); bf16 GNN + backward
    --workload c4      BASELINE configs[3]: generator only, 64 objects x 64 adjacency, batch 64, forward + backward

A plain run sets up, warms up, times the K steps and prints the line: `metric`, `value`, `unit`,
`higher_is_better`, `dtype`, `ms_per_step` (milliseconds of one timed step) and the configuration.

    --dump-outputs DIR after the timed steps, write what the last timed step computed (the arrays a caller of the
                       timed path receives: losses, logits, clip norms, a fixed seeded sample of the updated weights and
                       moments; c4: the generator's outputs and gradients) as DIR/<name>.npy in float32
    --full             also run everything below (each leg can still be switched off by its --no-* option)

Extra objects on the line (--full only; null in a plain run, as are `ms_per_step_by_branch`, `ms_per_pass`, `kernels`):
  roofline           the dominant kernel family of the step (c4: the LDS-tiled aggregate kernel), timed live with
                     HIP events on the launch stream in an instrumented (un-captured) iteration
  cpu_baseline       the CPU oracle (oracle/xggm_oracle.py, torch fp32) timed on this box's host cores on a bounded
                     sample of the same workload (N = 1 only)
  value_with_loader  the same steps with the loader boundary inside the timed region: a fresh host batch every
                     step (tokenised strings + pinned feature buffers), H2D on a copy stream, double-buffered
  value_ref_batch    the same iteration at the batch size the reference's own scripts train with (92 for VQA-CP v2,
                     script/vqacpv2.sh:10,23; 96 for GQA-OOD, script/gqa_ood.sh:10,24) -- never `value`, whose
                     configuration (32 samples per GPU) is BASELINE.json's
"""
import argparse
import json
import os
import random
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

PEAK_BF16_TFLOPS = 2500.0  # dense bf16 MFMA, /opt/skills/guides/MI355X_MICROARCH.md
PEAK_HBM_GBS = 8000.0


def parse(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--batch", type=int, default=None, help="samples per GPU (32; c4: 64)")
    p.add_argument("--answers", type=int, default=None, help="answer vocabulary (2274 VQA-CP v2; 1842 with --order gqa)")
    p.add_argument("--order", default="vqa", choices=["vqa", "gqa"],
                   help="vqa: plain pass then GGM pass, KL x 8; gqa: GGM first, KL x 12 (src/gqa/gqa_ood.py:165-292)")
    p.add_argument("--workload", default="train", choices=["train", "c4"])
    p.add_argument("--delta", type=int, default=5, help="relation-branch probability delta/10")
    p.add_argument("--dtype", default="bf16", choices=["bf16", "f32", "fp8"])
    p.add_argument("--no-graph", action="store_true", help="eager launches instead of hipGraph replay")
    p.add_argument("--no-cpu-baseline", action="store_true")
    p.add_argument("--no-kernel-timing", action="store_true")
    p.add_argument("--cpu-warmup", type=int, default=3, help="CPU baseline: warm-up iterations per branch (BASELINE.md section 3)")
    p.add_argument("--cpu-iters", type=int, default=10, help="CPU baseline: timed iterations per branch, the median is reported")
    p.add_argument("--no-loader", action="store_true", help="skip the loader-inclusive leg")
    p.add_argument("--no-ref-batch", action="store_true", help="skip the leg at the reference's own training batch size")
    p.add_argument("--wire", default="bf16", choices=["bf16", "f32"], help="gradient all-reduce dtype")
    p.add_argument("--zero1", type=int, default=None, help="1: shard the update over the ranks (reduce-scatter -> "
                   "BertAdam on the shard -> all-gather of the weights, stage by stage beside the next forward); "
                   "default: off at every world size until an N >= 4 scaling record exists (DESIGN.md section 6)")
    p.add_argument("--seed", type=int, default=9595)
    p.add_argument("--full", action="store_true", help="after the headline figure, also run the loader-inclusive leg, the "
                   "reference batch, the per-branch / per-pass times, the kernel timing and the CPU baseline")
    p.add_argument("--dump-outputs", metavar="DIR", default=None, help="write what the last timed step computed as "
                   "DIR/<name>.npy (float32, at most 64 MB in all)")
    a = p.parse_args(argv)
    if a.answers is None:
        a.answers = 1842 if a.order == "gqa" else 2274
    if a.batch is None:
        a.batch = 64 if a.workload == "c4" else 32
    return a


# ------------------------------------------------------------------------------------------ rank spawn
def spawn_ranks(args):
    """`python bench.py --gpus N` without a launcher: start N copies of this script, one per GPU, from a parent
    that has made no GPU call (a process that initialised the GPU must never exec another program on this pool);
    rank 0 prints the JSON line on the stdout it inherits."""
    import socket
    n = args.gpus
    if not os.environ.get("XGGM_SHARE_GPU"):
        have = torch.cuda.device_count()  # counting devices does not initialise the GPU
        if have < n:
            raise SystemExit("bench.py --gpus %d: only %d GPU(s) visible (XGGM_SHARE_GPU=1 + XGGM_DIST_BACKEND=gloo "
                             "rehearses the multi-rank path on one GPU)" % (n, have))
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env))
    rc = 0
    try:
        while procs:
            for p in list(procs):
                r = p.poll()
                if r is None:
                    continue
                procs.remove(p)
                if r != 0 and rc == 0:
                    rc = r
                    for q in procs:  # one rank died: the others would wait in a collective forever
                        q.terminate()
            time.sleep(0.05)
    finally:
        for p in procs:
            p.kill()
    raise SystemExit(rc)


# ------------------------------------------------------------------------------------------ model / data
def zero1_default(world):
    """The sharded update (ZeRO-1) is OPT-IN (``--zero1 1``) at every world size: no scaling run on more than one real
    GPU exists yet (SCALE_r03 is a skipped record) and the one measurement there is -- one rank on RCCL -- has it
    slower (12.4 against 11.8 ms per iteration).  A default belongs to a measured N >= 4 record, not to a model."""
    return False


def build(args, device):
    from xggm_amd import param, synth
    from xggm_amd.lxrt.modeling import BertConfig, VISUAL_CONFIG
    from xggm_amd.vqa.vqacpv2_model import VQAModel
    from xggm_amd.gqa.gqa_ood_model import GQAModel
    from xggm_amd.vqa.vqacpv2 import make_optimizer
    VISUAL_CONFIG.set_visual_dims(2048, 4)
    a = param.parse_args(["--llayers", "9", "--xlayers", "5", "--rlayers", "5"])
    torch.manual_seed(args.seed)
    dt = torch.float32 if args.dtype == "f32" else torch.bfloat16
    cls = GQAModel if args.order == "gqa" else VQAModel
    model = cls(args.answers, gnn="GCN", n_layers=2, args=a, config=BertConfig(30522), compute_dtype=dt,
                tokenizer=synthetic_tokenizer())
    model.seed = args.seed
    model = model.to(device)
    if args.dtype == "fp8":
        from xggm_amd.fp8 import enable_fp8
        enable_fp8(model)
    rank = int(os.environ.get("RANK", 0))
    b = synth.vqa_batch(args.batch, A=args.answers, seed=1000 + rank)
    batch = {k: torch.from_numpy(v).to(device) for k, v in b.items() if k != "randn_adj"}
    if dt == torch.bfloat16:
        batch["feats"] = batch["feats"].to(torch.bfloat16)  # as the shard format stores them (tools/shards.py)
    n_iters = 2 * args.steps + args.warmup + 128  # the timed steps, the loader leg and the diagnostic legs behind them
    lr = 5e-6 if args.order == "gqa" else 1e-6  # script/gqa_ood.sh:27, script/vqacpv2.sh:26; t_total = 2 * iterations
    optim = make_optimizer(model, lr, 2 * n_iters)
    return model, optim, batch


_WORDS = None


def synthetic_tokenizer():
    """a WordPiece tokenizer over a synthetic 30522-entry vocabulary (there is no bert-base-uncased vocab.txt
    offline): the loader-inclusive leg feeds question STRINGS through the same host path the reference uses
    (src/lxrt/entry.py:37-72)."""
    import tempfile
    from xggm_amd.lxrt.tokenization import BertTokenizer
    global _WORDS
    special = ["[PAD]"] + ["[unused%d]" % i for i in range(99)] + ["[UNK]", "[CLS]", "[SEP]", "[MASK]"]
    _WORDS = ["w%d" % i for i in range(30522 - len(special))]
    with tempfile.NamedTemporaryFile("w", suffix=".txt", delete=False) as f:
        f.write("\n".join(special + _WORDS) + "\n")
        path = f.name
    try:
        return BertTokenizer(path, do_lower_case=True)
    finally:
        os.unlink(path)


def make_loader(model, args, device, n_batches=8):
    """the input pipeline of the package on synthetic data: a shard file (xggm_amd.tools.shards: bf16 features,
    normalised boxes, adjacency -- what replaces the reference's per-image h5 groups, src/vqa/vqacpv2_data.py:95-127)
    of ``n_batches`` x batch images, question annotations over the synthetic vocabulary, the dataset mirror and the
    prefetching ``DataLoaderX`` (src/tools/data_loader.py:8-10) with tokenisation and H2D on its producer thread."""
    import tempfile
    import numpy as np
    from xggm_amd import synth
    from xggm_amd.tools.shards import ShardWriter
    from xggm_amd.tools.data_loader import DataLoaderX
    from xggm_amd.vqa.vqacpv2_data import VQADataset, VQATorchDataset
    rank = int(os.environ.get("RANK", 0))
    rng = random.Random(args.seed + 77 * rank)
    tmp = tempfile.mkdtemp(prefix="xggm_bench_")
    path = os.path.join(tmp, "train_obj36.xgs")
    w = ShardWriter(path, n_objects=36, feat_dim=2048)
    data, img = [], 0
    for i in range(n_batches):
        b = synth.vqa_batch(args.batch, A=args.answers, seed=5000 + 100 * rank + i)
        for k in range(args.batch):
            w.add(img, b["feats"][k], b["boxes"][k] * np.float32(0.999), 1.0, 1.0, b["adj_true"][k])
            lab = int(b["target"][k].argmax())
            data.append({"question_id": img, "image_id": img, "label": [lab], "score": [1.0],
                         "question": " ".join(rng.choice(_WORDS) for _ in range(rng.randint(3, 17)))})
            img += 1
    w.close()
    label2ans = ["a%d" % k for k in range(args.answers)]
    ds = VQADataset("train", data=data, ans2label={a: k for k, a in enumerate(label2ans)}, label2ans=label2ans)
    ts = VQATorchDataset(ds, shard=path)
    # handover="inline": the producer fills pinned slots, the trainer ships a slot with ONE stream-ordered copy into its
    # static inputs (CapturedTrainer.load_packed).  XGGM_LOADER_RING=1: the round-2 path (copy stream + device ring +
    # per-field hand-over copies), kept for the same-box comparison
    mode = "ring" if os.environ.get("XGGM_LOADER_RING") else "inline"
    loader = DataLoaderX(ts, args.batch, shuffle=True, drop_last=True, device=device, batcher=model.lxrt_encoder.batcher,
                         depth=3, seed=args.seed + rank, epochs=None, handover=mode)
    host_bytes = args.batch * (36 * 2048 * 2 + 36 * 4 * 4 + args.answers * 4 + 36 * 36 * 4 + 3 * 20 * 8)
    return loader, host_bytes, tmp


def batch_of(item):
    qid, feats, boxes, sent, target, adj = item
    return dict(feats=feats, boxes=boxes, input_ids=sent[0], input_mask=sent[1], segment_ids=sent[2], target=target,
                adj_true=adj)


# ------------------------------------------------------------------------------------------ output dump
DUMP_LIMIT_BYTES = 64 << 20
DUMP_SAMPLE = 1 << 20  # entries of a flat state buffer kept in the dump


def sample_index(n, k=DUMP_SAMPLE, seed=0):
    """a fixed, seeded, sorted sample of ``k`` positions out of ``n`` (all of them when ``n <= k``)"""
    import numpy as np
    if n <= k:
        return None
    return torch.from_numpy(np.sort(np.random.default_rng(seed).choice(n, size=k, replace=False)))


def dump_outputs(path, arrays):
    """``arrays``: {name: tensor}; each is written as ``path/<name>.npy`` in float32 (float64 stays float64)."""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    host = {}
    for name, t in arrays.items():
        t = t.detach()
        t = t.double() if t.dtype == torch.float64 else t.float()
        host[name] = t.cpu().numpy()
    total = sum(a.nbytes for a in host.values())
    if total > DUMP_LIMIT_BYTES:
        raise SystemExit("bench.py --dump-outputs: %d bytes, more than the %d allowed" % (total, DUMP_LIMIT_BYTES))
    for name, a in host.items():
        np.save(os.path.join(path, name + ".npy"), a)
    log("dumped %d arrays (%.1f MB) to %s" % (len(host), total / 1e6, path))


def train_outputs(trainer, last):
    """what one training iteration hands back, by pass kind, plus a seeded sample of the state it updated"""
    a, b = last  # (plain pass, GGM pass): CapturedTrainer.iteration returns them in that order for both loop orders
    out = {}
    for kind, (loss, logit, norm) in (("plain", a), ("ggm", b)):
        out[kind + "_loss"] = loss.reshape(-1)
        out[kind + "_logit"] = logit
        out[kind + "_grad_norm"] = norm.reshape(-1)
    arena = trainer.rt.arena
    idx = sample_index(arena.params.numel())
    for name in ("params", "m", "v"):
        buf = getattr(arena, name)
        out["sample_" + name] = buf if idx is None else buf[idx.to(buf.device)]
    return out


# ------------------------------------------------------------------------------------------ kernel timing
def kernel_timing(run_passes):
    """time every C-ABI launch of un-captured passes with HIP events recorded on the launch stream; a long sleep
    kernel is queued first so the host runs ahead and the events bracket back-to-back GPU execution, not Python
    latency.  ``run_passes``: list of callables, each one pass."""
    from xggm_amd import _lib
    import xggm_amd.ops as ops_mod
    rec = []
    orig = _lib.call

    def timed(name, *a):
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        work, probs = 0.0, None
        fam = name
        if name.startswith("xggm_gemm_grouped_"):
            probs = (ops_mod.GemmProblem * a[1]).from_address(a[0].value)
            work = sum(2.0 * p.M * p.N * p.K * p.batch for p in probs)
            fam = "xggm_gemm_" + name.rsplit("_", 1)[1]  # same kernel family as the single launches
        elif name.startswith("xggm_gemm_fp8"):
            work = 2.0 * a[3] * a[4] * a[5]
        elif name.startswith("xggm_gemm_"):
            work = 2.0 * a[3] * a[4] * a[5] * a[11]
        e0.record()
        orig(name, *a)
        e1.record()
        desc = ""
        if os.environ.get("XGGM_DUMP_GEMMS") and fam.startswith("xggm_gemm_"):
            if probs is not None:
                desc = " + ".join("%dx%dx%d%s" % (p.M, p.N, p.K, "f" if p.c_f32 else "") for p in probs)
            else:
                desc = "%dx%dx%d" % (a[3], a[4], a[5])
        rec.append((fam, a, e0, e1, work, desc))

    for run in run_passes:
        torch.cuda.synchronize()
        torch.cuda._sleep(int(5e7))  # head start for the host: launches queue up behind it
        ops_mod.call = timed
        try:
            run()
        finally:
            ops_mod.call = orig
        torch.cuda.synchronize()
    fam = {}
    if os.environ.get("XGGM_DUMP_GEMMS"):
        agg = {}
        for name, a, e0, e1, work, desc in rec:
            if desc:
                t = agg.setdefault(desc, [0.0, 0, 0.0])
                t[0] += e0.elapsed_time(e1); t[1] += 1; t[2] += work
        for desc, (ms, n, w) in sorted(agg.items(), key=lambda kv: -kv[1][0])[:40]:
            log("gemm %-60s n=%3d total %.3f ms avg %.1f us %.0f TF" % (desc, n, ms, 1000 * ms / n, w / ms / 1e9))
    for name, a, e0, e1, work, desc in rec:
        ms = e0.elapsed_time(e1)
        f = fam.setdefault(name, dict(ms=0.0, n=0, flops=0.0, bytes=0.0))
        f["ms"] += ms
        f["n"] += 1
        if name.startswith("xggm_gemm_"):
            f["flops"] += work
        elif name == "xggm_bertadam_f32":
            f["bytes"] += a[5] * (16 + 12 + (2 if a[4] else 0))
        elif name == "xggm_bertadam_ex":
            st = a[0]._obj  # the argument block: p, g (fp32 or bf16), m, v read; p, m, v (+ bf16 / e4m3 copies) written
            f["bytes"] += st.n * ((14 if st.g_bf16 else 16) + 12 + (2 if st.shadow_bf16 else 0) + (1 if st.shadow8 else 0))
        elif name == "xggm_sqnorm_f32":
            f["bytes"] += a[1] * 4
        elif name.startswith("xggm_aggregate_"):
            # x read once + out written once (T) + the fp32 adjacency read once
            B, N, H = a[3], a[4], a[5]
            es = 4 if name.endswith("f32") else 2
            f["bytes"] += B * N * H * es * (3 if a[10] else 2) + B * N * N * 4
    return fam


def cpu_baseline(args):
    """the CPU oracle on a bounded sample of the same workload, per BASELINE.md section 3: configuration C2 (this
    bench's batch) with the relation and the node branch timed separately (each iteration = plain pass + GGM
    pass, each fwd + bwd + clip + BertAdam), and C1 (4 samples).  Weights are random (values do not affect the
    timing).  ``value`` = the delta = 5 mix (mean of the two branch times)."""
    from oracle import shapes, xggm_oracle as O
    from xggm_amd import synth
    # the GPU box gives one GPU a 16-core CPU share; more threads than that only thrash
    cores = min(len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1), 16)
    torch.set_num_threads(cores)
    cfg = shapes.FULL
    g = torch.Generator().manual_seed(0)
    P = {}
    for k, s in shapes.model_shapes(cfg, args.answers).items():
        t = torch.randn(s, generator=g) * 0.02
        if len(s) == 1 and k.endswith("weight"):
            t = t + 1.0
        P[k] = t
    M = {k: torch.zeros_like(v) for k, v in P.items()}
    V = {k: torch.zeros_like(v) for k, v in P.items()}
    step = {k: 0 for k in P}
    kl = 12.0 if args.order == "gqa" else 8.0

    def batch_of(B):
        b = synth.vqa_batch(B, A=args.answers, seed=1000)
        b["randn_node"] = synth.randn_nodes(B, 36, 768, 0)
        return {k: torch.from_numpy(v) for k, v in b.items()}

    def iteration(b, branch):
        passes = [("plain", {}), (branch, dict(sigma=1.0, kl_weight=kl, gnn="GCN"))]
        if args.order == "gqa":
            passes.reverse()
        for kind, kw in passes:
            O.train_pass(P, M, V, step, b, cfg, kind, 1e-6, 100, **kw)

    def timed(b, branch, warm, iters):
        """warm-up iterations at the measured batch, then `iters` timed ones; the median"""
        for _ in range(warm):
            iteration(b, branch)
        ts = []
        for _ in range(iters):
            t0 = time.perf_counter()
            iteration(b, branch)
            ts.append(time.perf_counter() - t0)
        ts.sort()
        return ts[len(ts) // 2], ts

    t_all = time.perf_counter()
    b2, b1 = batch_of(args.batch), batch_of(4)
    warm, iters = args.cpu_warmup, args.cpu_iters
    s_rel, t_rel = timed(b2, "rel", warm, iters)
    s_node, t_node = timed(b2, "node", warm, iters)
    s_c1, t_c1 = timed(b1, "node", 1, 3)
    mix = 0.5 * (s_rel + s_node)
    model, phys = cpu_info()
    log("cpu baseline host: %s, %s physical cores, %d threads used" % (model, phys, cores))
    return {"value": round(args.batch / mix, 3), "unit": "samples/s", "cores": cores, "kind": "port",
            "cpu_model": model, "physical_cores": phys,
            "threads_note": "torch.set_num_threads(min(cores this process may run on, 16)): the GPU box gives one GPU a "
                            "16-core share, more threads than that only thrash",
            "by_branch": {"rel": {"s_per_iteration": round(s_rel, 3), "samples_per_s": round(args.batch / s_rel, 3),
                                  "ms_per_pass": round(500 * s_rel, 1), "min_max_s": [round(t_rel[0], 3), round(t_rel[-1], 3)]},
                          "node": {"s_per_iteration": round(s_node, 3), "samples_per_s": round(args.batch / s_node, 3),
                                   "ms_per_pass": round(500 * s_node, 1), "min_max_s": [round(t_node[0], 3), round(t_node[-1], 3)]}},
            "c1_batch4": {"s_per_iteration": round(s_c1, 3), "samples_per_s": round(4 / s_c1, 3)},
            "sample": "torch CPU oracle, fp32, full 9/5/5 model, A=%d, %s order: per branch %d warm-up + %d timed iterations "
                      "at %d samples, MEDIAN (plain pass + relation / node generation pass, each fwd+bwd+clip+BertAdam); "
                      "1 + 3 at 4 samples (config C1); value = mean of the two branch medians; %.1f s in all"
                      % (args.answers, args.order, warm, iters, args.batch, time.perf_counter() - t_all)}


def cpu_info():
    """CPU model and physical core count of the host (lscpu when present, /proc/cpuinfo otherwise)"""
    model, phys = "unknown", None
    try:
        import subprocess
        out = subprocess.run(["lscpu"], capture_output=True, text=True, timeout=10).stdout
        kv = {}
        for ln in out.splitlines():
            if ":" in ln:
                k, v = ln.split(":", 1)
                kv[k.strip()] = v.strip()
        model = kv.get("Model name", model)
        if "Core(s) per socket" in kv and "Socket(s)" in kv:
            phys = int(kv["Core(s) per socket"]) * int(kv["Socket(s)"])
    except Exception:
        pass
    if phys is None:
        try:
            cores = set()
            pid = cid = None
            for ln in open("/proc/cpuinfo"):
                if ln.startswith("model name") and model == "unknown":
                    model = ln.split(":", 1)[1].strip()
                elif ln.startswith("physical id"):
                    pid = ln.split(":", 1)[1].strip()
                elif ln.startswith("core id"):
                    cid = ln.split(":", 1)[1].strip()
                elif not ln.strip():
                    if cid is not None:
                        cores.add((pid, cid))
                    pid = cid = None
            phys = len(cores) or None
        except Exception:
            pass
    return model, phys


def pmc_traffic(family):
    """HBM-side bytes per C-ABI launch of a kernel family, from the committed PMC passes (profiles/*pmc_traffic.json:
    rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE on this bench in separate eager runs, gfx950 correction applied by
    tools/pmc_summary.py); the newest round's file that covers the family wins; None when none does."""
    import glob
    key = {"xggm_gemm_bf16": "gemm_", "xggm_bertadam_f32": "bertadam_kernel", "xggm_bertadam_ex": "bertadam_kernel",
           "xggm_ln_bwd_bf16": "ln_bwd_kernel",
           "xggm_ln_fwd_bf16": "ln_fwd_kernel", "xggm_attn_bwd_bf16": "attn_bwd", "xggm_attn_fwd_bf16": "attn_fwd",
           "xggm_aggregate_bf16": "aggregate_"}.get(family)
    if key is None:
        return None, None
    for path in sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_traffic*.json")), reverse=True):
        tot = n = 0.0
        for name, r in json.load(open(path)).items():
            if key in name:
                tot += (r["read_bytes_per_launch"] + r["write_bytes_per_launch"]) * r["launches"]
                n += r["launches"]
        if n:
            return round(tot / n), os.path.relpath(path, ROOT)
    return None, None


def roofline_step(args, ms_step):
    """The whole step against its own floors (SURVEY section 8d / BASELINE.md section 2): the batch-independent HBM
    traffic of an iteration (bf16 weights read by forward, dgrad and the shadow write, fp32 gradients, the fused
    clip + BertAdam streams, two passes: 17.7 GB) and its matrix work (65 GFLOP per sample), each at the nominal peak."""
    hbm_ms = 17.7e9 / (PEAK_HBM_GBS * 1e9) * 1e3
    mfma_ms = 65e9 * args.batch / (PEAK_BF16_TFLOPS * 1e12) * 1e3
    floor = max(hbm_ms, mfma_ms)
    return {"hbm_floor_ms": round(hbm_ms, 3), "mfma_floor_ms": round(mfma_ms, 3), "bound": "hbm" if hbm_ms >= mfma_ms else "mfma",
            "frac_of_step": round(floor / ms_step, 4),
            "note": "17.7 GB at 8 TB/s and 65 GFLOP per sample at 2.5 PFLOP/s dense bf16; the two overlap at best, so the "
                    "larger one is the floor"}


def log(msg):
    """progress on stderr (the JSON line is the only thing on stdout)"""
    print("[bench %6.1fs] %s" % (time.perf_counter() - T_START, msg), file=sys.stderr, flush=True)


T_START = time.perf_counter()


def roofline_of(fam, prefer=None):
    tot = sum(f["ms"] for f in fam.values())
    kernels = {k: {"ms": round(f["ms"], 3), "launches": f["n"], "share": round(f["ms"] / tot, 4)}
               for k, f in sorted(fam.items(), key=lambda kv: -kv[1]["ms"])[:8]}
    dom = prefer if prefer in fam else max(fam, key=lambda k: fam[k]["ms"])
    f = fam[dom]
    if dom.startswith("xggm_gemm_"):
        ach = f["flops"] / (f["ms"] * 1e-3) / 1e12
        traffic, src = pmc_traffic(dom)
        roofline = {"kernel": dom, "bound": "mfma", "achieved": round(ach, 2), "peak": PEAK_BF16_TFLOPS,
                    "unit": "TFLOP/s", "frac": round(ach / PEAK_BF16_TFLOPS, 4), "traffic": traffic,
                    "traffic_source": src and (src + " (PMC passes of an earlier run of this command, not of this run)"),
                    "timing": "HIP events around the eager C-ABI launches of one un-captured iteration (plain + rel + node "
                              "passes); the replayed graphs run the same kernels without the eager launch overhead: "
                              "profiles/README.md gives the rocprofv3 durations",
                    "launches": f["n"], "avg_us": round(1000 * f["ms"] / f["n"], 2)}
    else:
        ach = f["bytes"] / (f["ms"] * 1e-3) / 1e9 if f["bytes"] else 0.0
        traffic, src = pmc_traffic(dom)
        roofline = {"kernel": dom, "bound": "hbm", "achieved": round(ach, 1), "peak": PEAK_HBM_GBS,
                    "unit": "GB/s", "frac": round(ach / PEAK_HBM_GBS, 4), "traffic": traffic,
                    "traffic_source": src and (src + " (PMC passes of an earlier run of this command, not of this run)"),
                    "launches": f["n"], "avg_us": round(1000 * f["ms"] / f["n"], 2)}
    for k in ("xggm_bertadam_f32", "xggm_bertadam_ex", "xggm_aggregate_bf16"):  # the HBM-bound families: always with their rate
        if k in fam and fam[k]["ms"] > 0 and fam[k]["bytes"]:
            kernels.setdefault(k, {"ms": round(fam[k]["ms"], 3), "launches": fam[k]["n"],
                                   "share": round(fam[k]["ms"] / tot, 4)})
            kernels[k]["GB/s"] = round(fam[k]["bytes"] / (fam[k]["ms"] * 1e-3) / 1e9, 1)
    return roofline, kernels


# ------------------------------------------------------------------------------------------ C4: generator stress
def main_c4(args, device):
    """BASELINE configs[3]: the graph generator alone on 64 objects x 64 x 64 adjacency, batch 64: forward +
    backward of GCNGenerator(768, 2) (src/module/graph_generative_modeling.py:199-233) per step, captured into a
    hipGraph; roofline = the LDS-tiled aggregate kernel (out = adj @ x per sample) against HBM."""
    from xggm_amd import synth
    from xggm_amd.module.graph_generative_modeling import GCNGenerator
    from xggm_amd.runtime import bind_root, runtime_of
    B, N, H = args.batch, 64, 768
    torch.manual_seed(args.seed)
    gen = GCNGenerator(hidden_dim=H, n_layers=2)
    bind_root(gen, torch.float32 if args.dtype == "f32" else torch.bfloat16)
    gen = gen.to(device).train()
    x_np, adj_np = synth.generator_inputs("c4", "GCN", B, N, H, 0)
    dt = torch.float32 if args.dtype == "f32" else torch.bfloat16
    x = torch.from_numpy(x_np).to(device=device, dtype=dt).requires_grad_(True)
    adj = torch.from_numpy(adj_np).to(device).requires_grad_(True)
    rt = runtime_of(gen)
    gx = torch.randn(B, N, H, device=device, dtype=dt) / (N * H) ** 0.5
    ga = torch.randn(B, N, N, device=device) / N

    out = {}

    def step():
        gen.zero_grad()
        rt.arena.begin_pass()
        x.grad = adj.grad = None
        xo, ao = gen(x, adj)
        torch.autograd.backward([xo, ao], [gx, ga])
        rt.advance()
        out.update(x_out=xo, adj_out=ao)  # a replay rewrites these in place

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = None
    if not args.no_graph:
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            step()
    run = graph.replay if graph is not None else step
    for _ in range(args.warmup):
        run()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        run()
    torch.cuda.synchronize()
    dtm = time.perf_counter() - t0
    ms_step = 1000.0 * dtm / args.steps
    value = B * args.steps / dtm
    log("c4 timed region: %.3f ms/step, %.1f samples/s" % (ms_step, value))
    if args.dump_outputs:
        arrays = dict(out, x_grad=x.grad, adj_grad=adj.grad)
        arrays.update(("grad_" + k, p.grad) for k, p in gen.named_parameters() if p.grad is not None)
        dump_outputs(args.dump_outputs, arrays)
    roofline = kernels = None
    if args.full and not args.no_kernel_timing:
        fam = kernel_timing([step])
        roofline, kernels = roofline_of(fam, prefer="xggm_aggregate_" + ("f32" if args.dtype == "f32" else "bf16"))
    cpu = None
    if args.full and not args.no_cpu_baseline:
        cpu = cpu_baseline_c4(args, B, N, H)
    print(json.dumps({
        "metric": "generator fwd+bwd samples/sec (64-obj x 64 adjacency stress, BASELINE configs[3])",
        "value": round(value, 2), "unit": "samples/s", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": round(ms_step, 4), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": args.dtype, "data": "synthetic",
        "config": {"workload": "C4 stress: GCNGenerator(768, 2 layers) forward + backward, batch=%d, 64 objects x 64 x 64 "
                               "adjacency, 1 GPU, dropout on" % B, "global_batch": B, "parallelism": "dp1",
                   "hip_graph": graph is not None},
        "roofline": roofline, "kernels": kernels, "cpu_baseline": cpu}))


def cpu_baseline_c4(args, B, N, H):
    from oracle import shapes, xggm_oracle as O
    from xggm_amd import synth
    cores = min(len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1), 16)
    torch.set_num_threads(cores)
    P = {k: torch.from_numpy(synth.seeded_param(k, s, 0)).requires_grad_(True)
         for k, s in shapes.generator_shapes("GCN", H, 2).items()}
    x_np, adj_np = synth.generator_inputs("c4", "GCN", B, N, H, 0)
    x = torch.from_numpy(x_np).requires_grad_(True)
    adj = torch.from_numpy(adj_np).requires_grad_(True)
    t0 = time.perf_counter()
    n = 0
    while n < 20 and (n < 2 or time.perf_counter() - t0 < 10.0):
        xo, ao = O.gcn_generator(P, "generator.", x, adj, 2)
        torch.autograd.grad([xo.sum() + ao.sum()], [x, adj] + list(P.values()))
        n += 1
    dt = time.perf_counter() - t0
    return {"value": round(B * n / dt, 2), "unit": "samples/s", "cores": cores, "kind": "port",
            "sample": "torch CPU oracle gcn_generator forward + backward, fp32, batch %d, N=%d: %d steps, %.1f s"
                      % (B, N, n, dt)}


# ------------------------------------------------------------------------------------------ the training step
def main():
    args = parse()
    env_world = os.environ.get("WORLD_SIZE")
    if args.gpus > 1 and env_world is None:
        spawn_ranks(args)  # does not return
    world = int(env_world or 1)
    if world != args.gpus and not os.environ.get("XGGM_DP_FORCE"):
        raise SystemExit("bench.py: --gpus %d but WORLD_SIZE=%d; launch with `python bench.py --gpus N` (spawns the "
                         "ranks) or `python -m torch.distributed.run --nproc-per-node N bench.py --gpus N`"
                         % (args.gpus, world))
    rank = int(os.environ.get("RANK", 0))
    local = int(os.environ.get("LOCAL_RANK", 0))
    if os.environ.get("XGGM_SHARE_GPU"):  # several ranks on one GPU (logic rehearsal only)
        local = 0
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU: the HIP path has no CPU fallback")
    torch.cuda.set_device(local)
    device = torch.device("cuda", local)
    if args.workload == "c4":
        if world > 1:
            raise SystemExit("bench.py --workload c4 is a one-GPU configuration")
        return main_c4(args, device)
    force_dp = world == 1 and bool(os.environ.get("XGGM_DP_FORCE"))  # one-rank RCCL rehearsal of the N > 1 path
    if force_dp:
        os.environ.setdefault("MASTER_PORT", "29533")
        os.environ.setdefault("RANK", "0")
        os.environ.setdefault("WORLD_SIZE", "1")
    backend = None
    if world > 1 or force_dp:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        backend = os.environ.get("XGGM_DIST_BACKEND", "nccl")  # "gloo": logic check of the N>1 path on one GPU
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=device)
        else:
            dist.init_process_group(backend)
        assert dist.get_world_size() == world
    from xggm_amd.engine import CapturedTrainer
    from xggm_amd.runtime import runtime_of
    if os.environ.get("XGGM_GROUP_TILE"):  # A/B hook: pin the tile of grouped GEMM launches (1: 64x64, 2: 128x64, 3: 128x128)
        from xggm_amd import _lib
        _lib.lib.xggm_gemm_set_group_tile(int(os.environ["XGGM_GROUP_TILE"]))
    if os.environ.get("XGGM_GEMM_FLAGS"):  # A/B hook: xggm_gemm_set_tile flags (0x400: register-staged k-loops, 0x800 / 0x1000: 2 / 3 LDS stages)
        from xggm_amd import _lib
        _lib.lib.xggm_gemm_set_tile(int(os.environ["XGGM_GEMM_FLAGS"], 0))

    log("building the model (rank %d/%d)" % (rank, world))
    model, optim, batch = build(args, device)
    log("model on %s" % device)
    # first forward creates the arena; data parallel hooks need it
    rt = runtime_of(model)
    zero1 = False
    if world > 1 or force_dp:
        from xggm_amd.vqa.vqacpv2 import enable_data_parallel
        # The sharded update trades (world - 1) / world of the update's HBM traffic (1.0 of 1.17 ms per pass at 8 ranks) for
        # an all-gather of the bf16 matrix weights (388 MB) -- the same bytes on the links as the all-reduce it replaces,
        # split into a reduce-scatter under the backward stages and a gather that now runs stage by stage under the NEXT
        # pass's forward graphs (engine.CapturedTrainer).  At 2 ranks half of the update is too little to pay for the two
        # extra graph boundaries and the norm's scalar exchange (+0.45 ms per iteration measured at one rank).  Opt-in
        # (--zero1 1) at every world size until it has been measured on a real multi-GPU node: zero1_default.
        zero1 = bool(args.zero1) if args.zero1 is not None else zero1_default(world)
        enable_data_parallel(model, wire_dtype=torch.bfloat16 if args.wire == "bf16" else None, zero1=zero1)
    loader_parts = None
    if args.full and not args.no_loader:
        loader_parts = make_loader(model, args, device)  # before the trainer: its static inputs take the loader's slot layout
    inline = loader_parts is not None and loader_parts[0].handover == "inline"
    trainer = CapturedTrainer(model, optim, batch, sigma=1.0, order=args.order, use_graph=not args.no_graph,
                              packed_spec=loader_parts[0].spec if inline else None)
    log("trainer ready (hip_graph=%s)" % (not args.no_graph))
    pyrng = random.Random(args.seed)  # identical draws on every rank (src/vqa/vqacpv2.py:192)

    def branch():
        return "rel" if pyrng.randint(1, 10) <= args.delta else "node"

    def barrier():
        if world > 1:
            import torch.distributed as dist
            dist.barrier()
        torch.cuda.synchronize()

    def max_over_ranks(dt):
        if world > 1:
            import torch.distributed as dist
            t = torch.tensor([dt], device=device, dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            return float(t.item())
        return dt

    for _ in range(args.warmup):
        trainer.iteration(branch())
    barrier()
    log("warmup done")
    t0 = time.perf_counter()
    host_s = 0.0
    last = None
    for _ in range(args.steps):
        h0 = time.perf_counter()
        last = trainer.iteration(branch())
        host_s += time.perf_counter() - h0
    barrier()
    dt = max_over_ranks(time.perf_counter() - t0)
    log("host time in iteration(): %.3f ms/step" % (1000 * host_s / args.steps))
    ms_step = 1000.0 * dt / args.steps
    value = args.batch * world * args.steps / dt
    log("timed region: %.3f ms/step, %.1f samples/s" % (ms_step, value))
    if args.dump_outputs and rank == 0 and last is not None:
        dump_outputs(args.dump_outputs, train_outputs(trainer, last))

    # the same steps with the loader boundary inside the timed region (never `value`)
    with_loader = None
    if loader_parts is not None:
        import shutil
        loader, host_bytes, tmp = loader_parts
        it = iter(loader)

        def hand_over(item):
            if inline:
                trainer.load_packed(it)  # one host-to-device copy of the slot, stream-ordered
            else:
                trainer.load_batch(batch_of(item))

        try:
            for i in range(3):
                hand_over(next(it))
                trainer.iteration(branch())
            barrier()
            t1 = time.perf_counter()
            dbg = [0.0, 0.0, 0.0] if os.environ.get("XGGM_LOADER_DEBUG") else None
            for i in range(args.steps):
                # batch i was assembled, tokenised and copied to the device by the producer thread while step i - 1
                # ran; load_batch hands it to the captured graphs' input buffers (device to device)
                if dbg is None:
                    hand_over(next(it))
                    trainer.iteration(branch())
                else:  # host-side time of the three calls
                    a = time.perf_counter(); item = next(it)
                    b_ = time.perf_counter(); hand_over(item)
                    c = time.perf_counter(); trainer.iteration(branch())
                    d = time.perf_counter()
                    dbg[0] += b_ - a; dbg[1] += c - b_; dbg[2] += d - c
            barrier()
            dtl = max_over_ranks(time.perf_counter() - t1)
            if dbg is not None:
                log("loader leg host ms/step: next %.3f, load_batch %.3f, iteration %.3f"
                    % tuple(1000 * x / args.steps for x in dbg))
        finally:
            it.close()
            shutil.rmtree(tmp, ignore_errors=True)
        with_loader = {"value": round(args.batch * world * args.steps / dtl, 2),
                       "ms_per_step": round(1000.0 * dtl / args.steps, 3), "host_bytes_per_step": host_bytes,
                       "what": "a fresh batch every step through the package's input pipeline: memory-mapped shard "
                               "(bf16 features) -> pinned buffers -> cached WordPiece tokenisation of %d question "
                               "strings (producer thread, 3 pinned slots in flight) -> %s" % (args.batch,
                               "ONE stream-ordered host-to-device copy of the slot into the captured graphs' input buffers"
                               if inline else "H2D on a copy stream -> device-side hand-over to the captured graphs' input buffers"),
                       "handover": "inline" if inline else "ring"}
        log("with loader: %.3f ms/step" % with_loader["ms_per_step"])

    # the reference's own training batch size (script/vqacpv2.sh:10,23: 92; script/gqa_ood.sh:10,24: 96): row counts
    # that are no multiple of any GEMM tile (1840 / 3312 and 1920 / 3456 rows).  A second captured trainer on the same
    # model and optimiser; an extra key, never `value`.
    ref_batch = None
    if args.full and world == 1 and not force_dp and not args.no_ref_batch:
        from xggm_amd import synth
        Bref = 96 if args.order == "gqa" else 92
        nb = synth.vqa_batch(Bref, A=args.answers, seed=2000)
        bref = {k: torch.from_numpy(v).to(device) for k, v in nb.items() if k != "randn_adj"}
        if args.dtype != "f32":
            bref["feats"] = bref["feats"].to(torch.bfloat16)
        tr_ref = CapturedTrainer(model, optim, bref, sigma=1.0, order=args.order, use_graph=not args.no_graph, warmup_iters=1)
        n_ref = max(5, min(args.steps, 10))
        for _ in range(2):
            tr_ref.iteration(branch())
        barrier()
        t1 = time.perf_counter()
        for _ in range(n_ref):
            tr_ref.iteration(branch())
        barrier()
        dtr = time.perf_counter() - t1
        ref_batch = {"batch": Bref, "value": round(Bref * n_ref / dtr, 2), "unit": "samples/s",
                     "ms_per_step": round(1000.0 * dtr / n_ref, 3), "steps": n_ref,
                     "what": "the same iteration at the reference's training batch size (%s)"
                             % ("script/gqa_ood.sh:10,24" if args.order == "gqa" else "script/vqacpv2.sh:10,23")}
        log("reference batch %d: %.3f ms/step, %.1f samples/s" % (Bref, ref_batch["ms_per_step"], ref_batch["value"]))
        del tr_ref, bref
        torch.cuda.empty_cache()

    # per-branch step time (diagnostic; not part of the timed region)
    per_branch = per_pass = None
    if args.full:
        per_branch = {}
        for br in ("rel", "node"):
            barrier()
            t1 = time.perf_counter()
            for _ in range(5):
                trainer.iteration(br)
            barrier()
            per_branch[br] = round(1000.0 * (time.perf_counter() - t1) / 5, 3)

        # per-pass time: forward + backward + clip + BertAdam of ONE pass (SURVEY section 8d asks for both views)
        per_pass = {}
        for kind in ("plain", "rel", "node"):
            barrier()
            t1 = time.perf_counter()
            for _ in range(5):
                trainer.run_pass(kind)
            barrier()
            per_pass[kind] = round(1000.0 * (time.perf_counter() - t1) / 5, 3)

    roofline, kernels = None, None
    if args.full and not args.no_kernel_timing:
        # EVERY rank runs the instrumented passes (they contain the gradient exchange: a rank that skipped them
        # would leave the others waiting in a collective); rank 0 reports
        log("kernel timing pass")
        fam = kernel_timing([lambda k=k: trainer._eager_pass(k) for k in ("plain", "rel", "node")])
        if rank == 0:
            roofline, kernels = roofline_of(fam)

    cpu = None
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline:
        log("cpu baseline (oracle)")
        cpu = cpu_baseline(args)
        log("cpu baseline done: %s" % cpu["value"])

    if rank == 0:
        line = {
            "metric": "train samples/sec (36-obj VQA batch); one step = plain + GGM pass, each fwd+bwd+clip+BertAdam",
            "value": round(value, 2), "unit": "samples/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(ms_step, 3), "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": args.dtype, "data": "synthetic",
            "config": {"workload": "%dxMI355X %s: %s-shaped synthetic batch=%d/GPU, 36 objects x 2048, "
                                   "20 tokens, A=%d, LXMERT 9/5/5 + GCNx2, full fwd+bwd+clip+BertAdam x2 passes "
                                   "(%s), dropout on, delta=%d branch mix"
                                   % (world, args.dtype, "GQA-OOD" if args.order == "gqa" else "VQA-CP-v2", args.batch,
                                      args.answers, "GGM pass first, KL x 12" if args.order == "gqa" else
                                      "plain pass first, KL x 8", args.delta),
                       "global_batch": args.batch * world, "parallelism": "dp%d" % world, "order": args.order,
                       "world_size": world, "backend": backend, "zero1": zero1,
                       "hip_graph": not args.no_graph, "grad_wire": args.wire if (world > 1 or force_dp) else None},
            "ms_per_step_by_branch": per_branch, "ms_per_pass": per_pass, "value_with_loader": with_loader,
            "value_ref_batch": ref_batch,
            "roofline": roofline, "roofline_step": roofline_step(args, ms_step), "kernels": kernels, "cpu_baseline": cpu,
        }
        print(json.dumps(line), flush=True)
    if world > 1 or force_dp:
        import torch.distributed as dist
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
