"""Six-step trajectory of BertLamb in fp64: ``lamb.npz``.

    python tests/golden/make_lamb_golden.py <path to the reference's src directory>

The reference's ``BertAdam`` (src/lxrt/optimization.py:58-203, loaded by path, never copied) gives the defaults -- b1, b2, e,
weight_decay -- and the schedule function; the step itself is restated here in fp64 over fp32 inputs (weights, gradients
and the hyper-parameters as the C ABI's floats hold them), with the trust ratio between the reference's lines 171 and 192:

    m = b1 m + (1 - b1) g            v = b2 v + (1 - b2) g^2
    u = m / (sqrt(v) + e) + weight_decay * p             (the weight-decay term only when weight_decay > 0)
    r = ||p|| / ||u||  if both norms are > 0 and the tensor is adapted, else 1
    p -= lr * schedule(step / t_total, warmup) * r * u

The norms are plain fp64 norms (numpy's pairwise sum): the order in which the device adds its doubles changes them by
parts in 1e16.  Nothing here is taken from the code under test.

Tensors: the short lengths (1, 7, 8, 9, 24), an all-zero tensor, a tensor that is not adapted and not decayed (the BERT
recipe for biases and LayerNorm weights), one element more than a 2048-element chunk, and a tensor of more than one chunk
with an ``n & 3`` tail.  Six steps with a warm-up of 0.3 over t_total = 12: the first step has lr 0 (p keeps its bits, m and
v move), steps 1-3 warm up, 4-5 decay.  Recorded: the inputs (p0 and the six gradients, fp32), p, m, v after the first and
after the last step (fp64) and the ratios of all six steps."""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
LENGTHS = [1, 7, 8, 9, 24, 300, 130, 2049, 2500]
ZERO, PLAIN = 5, 6          # index of the all-zero tensor; of the tensor that is neither adapted nor decayed
STEPS, T_TOTAL, WARMUP, LR = 6, 12, 0.3, 2e-3


def load_reference(src):
    spec = importlib.util.spec_from_file_location("ref_optimization", os.path.join(src, "lxrt", "optimization.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main(src):
    ref = load_reference(src)
    opt = ref.BertAdam([torch.nn.Parameter(torch.zeros(1))], lr=LR, warmup=WARMUP, t_total=T_TOTAL)
    hp = opt.param_groups[0]
    # fp32 inputs: the hyper-parameters too are the values the C ABI carries (float b1, b2, eps, weight_decay, lr), taken
    # exactly; 1 - b2 below is then the fp64 difference of THAT b2 (1 - 0.999f is 1.3e-5 below 0.001)
    f32 = lambda x: float(np.float32(x))  # noqa: E731
    b1, b2, e, wd0, lr0 = f32(hp['b1']), f32(hp['b2']), f32(hp['e']), f32(hp['weight_decay']), f32(hp['lr'])
    schedule = ref.SCHEDULES[hp['schedule']]
    rng = np.random.default_rng(20261021)
    p0 = [rng.standard_normal(n).astype(np.float32) * np.float32(0.05) for n in LENGTHS]
    p0[ZERO][:] = 0.0
    grads = []
    for s in range(STEPS):
        gs = [rng.standard_normal(n).astype(np.float32) * np.float32(0.01) for n in LENGTHS]
        for g in gs:
            g[rng.random(g.size) < 0.05] = 0.0
        gs[ZERO][:] = 0.0
        grads.append(gs)
    adapted = [i != PLAIN for i in range(len(LENGTHS))]
    wd = [0.0 if i == PLAIN else wd0 for i in range(len(LENGTHS))]
    P = [x.astype(np.float64) for x in p0]
    M = [np.zeros(n) for n in LENGTHS]
    V = [np.zeros(n) for n in LENGTHS]
    ratios = np.ones((STEPS, len(LENGTHS)))
    out = {}
    for s in range(STEPS):
        lr = lr0 * schedule(s / hp['t_total'], hp['warmup'])
        for i, g in enumerate(grads[s]):
            g = g.astype(np.float64)
            M[i] = b1 * M[i] + (1.0 - b1) * g
            V[i] = b2 * V[i] + (1.0 - b2) * g * g
            u = M[i] / (np.sqrt(V[i]) + e)
            if wd[i] > 0.0:
                u = u + wd[i] * P[i]
            np_, nu = float(np.linalg.norm(P[i])), float(np.linalg.norm(u))
            r = np_ / nu if (adapted[i] and np_ > 0.0 and nu > 0.0) else 1.0
            ratios[s, i] = r
            P[i] = P[i] - lr * r * u
        if s in (0, STEPS - 1):
            tag = "first" if s == 0 else "last"
            out["p_" + tag], out["m_" + tag], out["v_" + tag] = (np.concatenate(X) for X in (P, M, V))
    assert np.array_equal(out["p_first"], np.concatenate(p0).astype(np.float64))  # lr 0 at step 0
    assert ratios[:, ZERO].tolist() == [1.0] * STEPS and ratios[:, PLAIN].tolist() == [1.0] * STEPS
    assert float(np.abs(np.delete(ratios, [ZERO, PLAIN], axis=1) - 1.0).min()) > 1e-3  # the adapted ratios are far from 1
    out.update(lengths=np.array(LENGTHS), adapted=np.array(adapted), weight_decay=np.array(wd), p0=np.concatenate(p0),
               grads=np.stack([np.concatenate(gs) for gs in grads]), ratios=ratios,
               hyper=np.array([lr0, b1, b2, e, hp['warmup'], hp['t_total']]))
    path = os.path.join(HERE, "lamb.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d tensors, %d elements, %d bytes; ratios of the last step %s"
          % (path, len(LENGTHS), sum(LENGTHS), os.path.getsize(path), np.round(ratios[-1], 4).tolist()))


if __name__ == "__main__":
    main(sys.argv[1])
