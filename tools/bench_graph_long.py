"""What the graph kernels for 65..128 objects (csrc/graph_long.hip) take; one process, GPU only.  Nothing here is a gate:
the 64-object kernels cannot run these shapes at all, so there is no "before".  Each number is named for what it is.

  (a) every long kernel at B = 32, H = 768, N = 100 and 128, fp32 and bf16 node features, beside
        leg T  a torch composition of the same arithmetic on the same GPU (torch.bmm, softmax, max, ...), and
        floor  the bytes the kernel must move (computed from the shapes below) over the HBM peak of MI355X_MICROARCH.md
      Device events around windows of launches sized to at least --window seconds; every shape is warmed up; the two legs
      alternate in one process and repeat; median (min, max) per launch.
  (b) one full-size captured GGM iteration (LXMERT 9/5/5, GCN x 2, bf16, B = 32; a plain pass + a rel or node pass) at
      N = 100 objects (long_graph=True) beside the same at N = 64 (the short kernels), for scale.  Host clock around windows
      that end in a synchronise, the two sizes alternating.

    python tools/bench_graph_long.py [--out profiles/graph_long/graph_long_ab.txt] [--repeats 5] [--window 0.25] [--only a|b]
"""
import argparse
import math
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12  # bytes / s (MI355X: 8 TB/s HBM3E)
B, H, D_EMB = 32, 768, 768
F32, BF16 = torch.float32, torch.bfloat16


def _stats(v):
    return "median %.2f (min %.2f, max %.2f)" % (statistics.median(v), min(v), max(v))


def _window(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return 1000.0 * e0.elapsed_time(e1) / n  # us per launch


def ab(out, name, ours, torch_leg, nbytes, repeats, window):
    """alternate the two legs; windows of at least ``window`` seconds each"""
    for fn in (ours, torch_leg):  # warm-up of this shape
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    reps = {k: max(10, int(math.ceil(window * 1e6 / max(_window(fn, 10), 0.5)))) for k, fn in (("K", ours), ("T", torch_leg))}
    us = {"K": [], "T": []}
    for _ in range(repeats):
        for k, fn in (("K", ours), ("T", torch_leg)):
            us[k].append(_window(fn, reps[k]))
    floor = nbytes / HBM_PEAK * 1e6
    mk, mt = statistics.median(us["K"]), statistics.median(us["T"])
    out("%-34s kernel %s us | torch %s us | byte floor %.2f us (%d bytes; kernel = %.1f x floor) | kernel / torch %.2f%s"
        % (name, _stats(us["K"]), _stats(us["T"]), floor, nbytes, mk / floor, mk / mt, "  SLOWER than torch" if mk > mt else ""))


def leg_kernels(out, dev, repeats, window):
    from xggm_amd import ops
    from xggm_amd.preprocess.compute_adjacency import compute_cosin_sim_v2
    g = torch.Generator(device="cpu").manual_seed(0)
    for N in (100, 128):
        NE = N * (N - 1) // 2
        adj = torch.rand(B, N, N, generator=g).to(dev)
        mask = (adj > 0.6).float()
        S_in = torch.randn(B, N, N, generator=g).to(dev)
        d_nn = torch.randn(B, N, N, generator=g).to(dev)
        e = torch.rand(B, NE, generator=g).to(dev)
        s = torch.randn(B * N, 2, generator=g).to(dev)
        eye = torch.eye(N, device=dev).unsqueeze(0)
        iu = torch.triu_indices(N, N, 1, device=dev)
        nn4 = B * N * N * 4
        # adjacency-only kernels (fp32 whatever the node type)
        a_fwd, cm, am = ops.adj_regen_fwd(S_in, long=True)

        def regen_t():
            mx = S_in.max(dim=1)[0]
            return torch.sigmoid(S_in / mx.unsqueeze(-1)) * (1.0 - eye)

        def regen_bwd_t():
            dr = d_nn * a_fwd * (1.0 - a_fwd) * (1.0 - eye)
            dS = dr / cm.unsqueeze(-1)
            dm = -(dr * S_in).sum(2) / (cm * cm)
            return dS.scatter_add_(1, am.long().unsqueeze(1), dm.unsqueeze(1))

        def init_t():
            a0 = torch.zeros(B, N, N, device=dev)
            a0[:, iu[0], iu[1]] = e
            nz = torch.triu(d_nn, 1) * 0.7
            nz = nz + nz.transpose(1, 2)
            return a0 + a0.transpose(1, 2) + nz, -nz / 0.49

        def init_bwd_t():
            return d_nn[:, iu[0], iu[1]] + d_nn[:, iu[1], iu[0]]

        def gat_t():
            sv = s.view(B, N, 2)
            ee = torch.nn.functional.leaky_relu(sv[:, :, 0].unsqueeze(2) + sv[:, :, 1].unsqueeze(1), 0.2)
            return torch.softmax(ee.masked_fill(mask == 0, -9e15), dim=-1)

        att = ops.gat_att_fwd(s, mask, 0.2, long=True)

        def gat_bwd_t():
            sv = s.view(B, N, 2)
            raw = sv[:, :, 0].unsqueeze(2) + sv[:, :, 1].unsqueeze(1)
            de = att * (d_nn - (att * d_nn).sum(-1, keepdim=True)) * torch.where(raw > 0, 1.0, 0.2) * (mask != 0)
            return torch.stack([de.sum(2), de.sum(1)], dim=-1)

        cls = torch.randn(B, N, D_EMB, generator=g).to(dev)
        atr = torch.randn(B, N, D_EMB, generator=g).to(dev)

        def cos_t():
            an = cls / cls.norm(dim=-1, keepdim=True).clamp_min(1e-6)
            bn = atr / atr.norm(dim=-1, keepdim=True).clamp_min(1e-6)
            c = torch.bmm(an, bn.transpose(1, 2)).triu()
            c = c + c.transpose(1, 2)
            return c / c.flatten(1).max(dim=1)[0].view(B, 1, 1)

        tag = "N=%d " % N
        ab(out, tag + "adj_regen_long_fwd", lambda: ops.adj_regen_fwd(S_in, long=True), regen_t, 2 * nn4, repeats, window)
        ab(out, tag + "adj_regen_long_bwd", lambda: ops.adj_regen_bwd(d_nn, S_in, a_fwd, cm, am, long=True), regen_bwd_t, 4 * nn4,
           repeats, window)
        ab(out, tag + "adj_init_long_fwd", lambda: ops.adj_init_fwd(e, N, 0.7, randn=d_nn, long=True), init_t,
           2 * nn4 + 2 * B * NE * 4, repeats, window)
        ab(out, tag + "adj_init_long_bwd", lambda: ops.adj_init_bwd(d_nn, long=True), init_bwd_t, nn4 + B * NE * 4, repeats, window)
        ab(out, tag + "gat_att_long_fwd", lambda: ops.gat_att_fwd(s, mask, 0.2, long=True), gat_t, 2 * nn4, repeats, window)
        ab(out, tag + "gat_att_long_bwd_f32", lambda: ops.gat_att_bwd(d_nn, att, s, mask, 0.2, F32, long=True), gat_bwd_t, 3 * nn4,
           repeats, window)
        ab(out, tag + "cosine_adjacency_long_f32 (D=768)", lambda: compute_cosin_sim_v2(cls, atr, normalize=True), cos_t,
           2 * B * N * D_EMB * 4 + nn4, repeats, window)
        for dt in (F32, BF16):
            x = torch.randn(B, N, H, generator=g).to(dev, dt)
            dh = torch.randn(B, N, H, generator=g).to(dev, dt)
            acc = torch.zeros(1, device=dev)
            xb = B * N * H * x.element_size()
            sfx = ops.sfx(dt)
            adj_t = adj.to(dt)  # the torch leg of bf16 rounds the adjacency to bf16 (outside the window); the kernel does not
            ab(out, tag + "aggregate_long_%s plain" % sfx, lambda: ops.aggregate(adj, x, long=True), lambda: torch.bmm(adj_t, x),
               nn4 + 2 * xb, repeats, window)
            ab(out, tag + "aggregate_long_%s transpose" % sfx, lambda: ops.aggregate(adj, x, mode=ops.AGG_TRANSPOSE, long=True),
               lambda: torch.bmm(adj_t.transpose(1, 2), x), nn4 + 2 * xb, repeats, window)
            ab(out, tag + "aggregate_long_%s symmetrise" % sfx, lambda: ops.aggregate(adj, x, mode=ops.AGG_SYMMETRIZE, long=True),
               lambda: torch.bmm(adj_t + adj_t.transpose(1, 2), x), nn4 + 2 * xb, repeats, window)
            ab(out, tag + "agg_dot_long_%s" % sfx, lambda: ops.agg_dot(adj, x, dh, acc, long=True),
               lambda: (torch.bmm(adj_t, x).float() * dh.float()).sum(), nn4 + 2 * xb, repeats, window)


def leg_iteration(out, dev, repeats, window):
    from xggm_amd import param, synth
    from xggm_amd.engine import CapturedTrainer
    from xggm_amd.lxrt.modeling import BertConfig, VISUAL_CONFIG
    from xggm_amd.vqa.vqacpv2 import make_optimizer
    from xggm_amd.vqa.vqacpv2_model import VQAModel
    A, T, F = 2274, 20, 2048
    VISUAL_CONFIG.set_visual_dims(F, 4)
    a = param.parse_args(["--llayers", "9", "--xlayers", "5", "--rlayers", "5"])
    trainers = {}
    for N in (64, 100):
        torch.manual_seed(0)
        m = VQAModel(A, gnn="GCN", n_layers=2, args=a, config=BertConfig(30522), compute_dtype=BF16, n_objects=N,
                     long_graph=N > 64).to(dev)
        m.seed = 1
        opt = make_optimizer(m, 1e-6, 100000)
        batch = {k: torch.from_numpy(v).to(dev) for k, v in synth.vqa_batch(B, A=A, N=N, T=T, F=F, vocab=30522, seed=2).items()}
        trainers[N] = CapturedTrainer(m, opt, batch, sigma=1.0, warmup_iters=2)

    def run(N, n):
        tr = trainers[N]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(n):
            tr.iteration("rel" if i % 2 == 0 else "node")
        torch.cuda.synchronize()
        return 1000.0 * (time.perf_counter() - t0) / n

    n = {N: max(4, 2 * int(math.ceil(window * 1e3 / run(N, 4) / 2))) for N in trainers}
    ms = {N: [] for N in trainers}
    for _ in range(repeats):
        for N in trainers:
            ms[N].append(run(N, n[N]))
    for N in trainers:
        out("(b) captured GGM iteration (plain + rel / node alternating), LXMERT 9/5/5, GCN x 2, bf16, B = %d, N = %d%s: %s ms per "
            "iteration, windows of %d iterations, %d repeats"
            % (B, N, " (long_graph)" if N > 64 else " (short kernels)", _stats(ms[N]), n[N], repeats))
    out("(b) N = 100 over N = 64 at the medians: %.2f x (objects: 1.56 x; adjacency entries: 2.44 x)"
        % (statistics.median(ms[100]) / statistics.median(ms[64])))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "graph_long", "graph_long_ab.txt"))
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--window", type=float, default=0.25, help="seconds of work per timed window, at least")
    p.add_argument("--only", choices=["a", "b"], default=None)
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_graph_long: needs a GPU (nothing here is measured on a CPU)")
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)

    out("# python tools/bench_graph_long.py --repeats %d --window %.2f   (%s)" % (a.repeats, a.window, torch.cuda.get_device_name(0)))
    out("# (a) B = %d, H = %d; us per launch through the ops wrappers (output allocation included, as the model calls them); "
        "byte floor at %.1f TB/s" % (B, H, HBM_PEAK / 1e12))
    if a.only != "b":
        leg_kernels(out, dev, a.repeats, a.window)
    if a.only != "a":
        leg_iteration(out, dev, a.repeats, a.window)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
