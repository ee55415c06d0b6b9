"""Bit-level fixture of the fused optimiser update: ``optim_update_bits.json``.

Every case runs three steps of ``ops.optim_multi`` (schedule and step scalars from ``ops.sched_step_ex``) over nine spans
of one flat arena -- past the eight spans of one launch, so a call is two launches -- and records one SHA-256 per buffer
the update writes: p, m, v, the bf16 shadow, the e4m3 copy and the amax table, each hashed over its state after every
step.  Only those two wrappers are used; their signatures are the same on both sides of a change to the update.

    python tests/golden/make_optim_update_golden.py <commit id> [out.json]     (on the GPU, with that commit's library)

tests/test_optim_gpu.py::test_update_bits_equal_the_recorded_commit regenerates the digests and compares.

Shapes: the smallest that reach where the update can go wrong -- the ``n & 3`` tail alone (1, 3: no float4 at all), one
float4 (4), float4 + tail (7), one wave's worth and less (12, 256), both unrolled quadruples of a thread with and
without a tail (2048 / 2055: 512 float4 > 256 threads), an odd middle (1027), and for the e4m3 copy a 5120-element span on
a 256-element chunk whose chunks change their scale-table entry (and have none) along the way.  The grid-stride loop's
second trip needs more than 134 M elements and is not covered."""
import hashlib
import json
import os
import sys

import torch

DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
MAX_NORM = 5.0
LENGTHS = [1, 3, 4, 7, 12, 256, 1027, 2048, 2055]
E4M3_LEN = 5120
N_STEPS = 3
N_TABLE = 3  # hyper table: entry 0 + two param_groups; the id map also holds a 3 (>= n_table: treated as 0)
BUFFERS = ("p", "m", "v", "shadow", "e4m3", "amax")

# rule of ops.optim_multi, the span's (lr, b1, b2, eps, weight_decay), the rule's keyword arguments
RULES = {
    "bertadam": ("bertadam", (1e-2, 0.9, 0.999, 1e-6, 0.01), {}),
    "adam": ("adam", (1e-2, 0.0, 0.0, 1e-8, 0.1), dict(b1=0.9, b2=0.999)),
    "adamw": ("adamw", (1e-2, 0.0, 0.0, 1e-8, 0.1), dict(b1=0.9, b2=0.999)),
    "adamax": ("adamax", (2e-2, 0.0, 0.0, 1e-8, 0.1), dict(b1=0.9, b2=0.999)),
    "sgd0": ("sgd", (1e-2, 0.0, 0.0, 0.0, 0.1), dict(momentum=0.0)),
    "sgdn": ("sgd", (1e-2, 0.0, 0.0, 0.0, 0.1), dict(momentum=0.9, nesterov=True)),
    "rms0": ("rmsprop", (1e-2, 0.0, 0.0, 1e-8, 0.1), dict(alpha=0.99, momentum=0.0)),
    "rmsm": ("rmsprop", (1e-2, 0.0, 0.0, 1e-8, 0.1), dict(alpha=0.99, momentum=0.9)),
}


def cases():
    """[(case id, key of RULES, gradient dtype, with a hyper map, with e4m3 copy + lr_dev + g_scale 0.5)]"""
    out = []
    for key in RULES:
        for gname, gdt in (("f32", F32), ("bf16", BF16)):
            for mapped in (False, True):
                for extra in ((False, True) if key == "bertadam" else (False,)):
                    cid = "%s-%s-%s%s" % (key, gname, "map" if mapped else "nomap", "-e4m3" if extra else "")
                    out.append((cid, key, gdt, mapped, extra))
    return out


def _digest(h):
    return h.hexdigest()


def run_case(ops, key, gdt, mapped, extra):
    """{buffer: SHA-256 over the buffer's bytes after each of the three steps}"""
    rule, (lr, b1, b2, eps, wd), rkw = RULES[key]
    lengths = LENGTHS + ([E4M3_LEN] if extra else [])
    offs, o = [], 0
    for n in lengths:  # every span on a 256-element chunk (so also on a whole id of the hyper map)
        offs.append(o)
        o = (o + n + 255) // 256 * 256
    total = o
    gen = torch.Generator().manual_seed(20 + len(key))
    p = torch.randn(total, generator=gen).to(DEV)
    m = (torch.randn(total, generator=gen) * 0.1).to(DEV)
    v = (torch.rand(total, generator=gen) * 0.1).to(DEV)
    shadow = torch.full((total,), 3.0, device=DEV, dtype=BF16)
    s8 = torch.full((total,), 0x55, device=DEV, dtype=torch.uint8)
    g = torch.zeros(total, device=DEV, dtype=gdt)
    steps = torch.zeros(1, device=DEV, dtype=torch.int64)
    lr_scale = torch.ones(1, device=DEV)
    hs = torch.zeros(4, device=DEV)
    sq = torch.zeros(1, device=DEV)
    lr_dev = torch.tensor([lr], device=DEV)
    # e4m3: the chunks of the last span cycle through the table's entries {1, 0 = no copy, 2, 3}; entry 1 quantises with a
    # range its maxima stay inside, entries 2 and 3 with ranges the maxima of N(0, 1) weights come near or exceed
    chunk_id = torch.zeros(total // 256, dtype=torch.int16)
    if extra:
        c0 = offs[-1] // 256
        chunk_id[c0:c0 + E4M3_LEN // 256] = torch.tensor([1, 0, 2, 3, 3] * (E4M3_LEN // 256 // 5), dtype=torch.int16)
    chunk_id = chunk_id.to(DEV)
    qtab = torch.tensor([1.0, 16.0, 112.0, 160.0], device=DEV)
    amax = torch.zeros(4 * 2, device=DEV)  # two slots per entry
    hyper_map = None
    if mapped:
        # one id per 8 elements, changing every 5 ids (40 elements: a wave's 256 elements mix tensors); 0 = not in the
        # optimiser, 3 = an id the table does not hold
        j = torch.arange((total + 7) // 8)
        ids = torch.tensor([1, 2, 0, 1, 3, 2], dtype=torch.uint8)[(j // 5) % 6]
        ids[offs[0] // 8] = 2  # the one-element span is updated, the three-element span is not
        ids[offs[1] // 8] = 0
        table = torch.tensor([[0.0, 0.0], [lr, wd], [0.5 * lr, 0.0]])
        assert table.shape[0] == N_TABLE and int(ids.max()) >= N_TABLE and int(ids.min()) == 0
        hyper_map = (ids.to(DEV), table.to(DEV))
    hashes = {k: hashlib.sha256() for k in BUFFERS}
    for s in range(N_STEPS):
        gs = torch.randn(total, generator=gen)
        gs[torch.rand(total, generator=gen) < 0.05] = 0.0
        if s % 2:
            gs *= 0.01  # the clip at MAX_NORM is active on the even steps only
        g.copy_(gs)
        live = torch.cat([g[a:a + n].double() for a, n in zip(offs, lengths)])
        sqv = float((live ** 2).sum())
        assert (sqv ** 0.5 > MAX_NORM) == (s % 2 == 0), (s, sqv)
        sq.fill_(sqv)
        ops.sched_step_ex(steps, lr_scale, hs, [(0, 10, 0.0, "warmup_cosine", rkw.get("b1", 0.0), rkw.get("b2", 0.0))])
        jobs = []
        for i, (a, n) in enumerate(zip(offs, lengths)):
            sl = slice(a, a + n)
            kw = dict(elem0=a)
            if extra:
                kw.update(lr_dev=lr_dev, g_scale=0.5)
                if i == len(lengths) - 1:
                    kw["w8"] = (s8[sl], chunk_id, qtab, amax, 2)
            jobs.append(((p[sl], g[sl], m[sl], v[sl], shadow[sl], sq, MAX_NORM, 123.0 if extra else lr, lr_scale, b1, b2, eps, wd),
                         kw, dict(rkw, step_scalars=hs) if rkw else {}))
        ops.optim_multi(rule, jobs, hyper_map=hyper_map)
        torch.cuda.synchronize()
        for k, buf in zip(BUFFERS, (p, m, v, shadow, s8, amax)):
            hashes[k].update(buf.cpu().contiguous().view(torch.uint8).numpy().tobytes())
    return {k: _digest(h) for k, h in hashes.items()}


def generate():
    from xggm_amd import ops
    return {cid: run_case(ops, key, gdt, mapped, extra) for cid, key, gdt, mapped, extra in cases()}


if __name__ == "__main__":
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.dirname(os.path.dirname(here)))
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(here, "optim_update_bits.json")
    doc = {"commit": sys.argv[1], "steps": N_STEPS, "cases": generate()}
    with open(out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %s: %d cases" % (out, len(doc["cases"])))
