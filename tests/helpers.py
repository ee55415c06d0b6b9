"""shared test helpers: seeded parameters as torch tensors, probes, golden loading."""
import os

import numpy as np
import torch

from xggm_amd import synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_golden(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)


def golden_cfg(g):
    return {str(k): int(v) for k, v in zip(g["cfg_keys"], g["cfg_vals"])}


def seeded_params(shapes, seed, dtype=torch.float32, device="cpu"):
    return {k: torch.from_numpy(synth.seeded_param(k, s, seed)).to(device=device, dtype=dtype)
            for k, s in shapes.items()}


def probe(name, shape, seed, dtype=torch.float32, device="cpu"):
    v = synth._rng(seed, "probe:" + name).standard_normal(tuple(shape), dtype=np.float32)
    return torch.from_numpy(v).to(device=device, dtype=dtype)


def batch_tensors(b, device="cpu", dtype=torch.float32):
    out = {}
    for k, v in b.items():
        t = torch.from_numpy(np.ascontiguousarray(v)).to(device)
        out[k] = t.to(dtype) if t.is_floating_point() else t
    return out


def rel_err(a, b):
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


# ---- element-wise GEMM bound -------------------------------------------------------------------------------------
# rel_err is a norm ratio over the whole tensor: a truncating store, a few dozen wrong elements or a wrong 8 x 8
# corner of a 640 x 768 output all stay under its 1.2e-2 (tests/test_gemm_edges_cpu.py shows it).  gemm_excess
# compares every element with a bound DERIVED from the arithmetic, never fitted to what a kernel returns:
#   accumulation   c * (K + 3) * 2^-24 * S     S = |A| . |B| (+ |bias| + |residual| + |old C|), fp64.  Products of bf16
#                                              (or e4m3) values are exact in fp32 and K - 1 fp32 additions in ANY order
#                                              stay within (K - 1) u S, u = 2^-24; the + 3 covers the epilogue's
#                                              additions; c = 2 is the margin for the MFMA's internal order.
#   bf16 store     2^-8 * |ref|                bf16's unit round-off under round-to-nearest; no margin on this term.
#   extra          caller's term               e.g. 4 * 2^-24 * (1 + |f|) for an activation evaluated in fp32.
# An activation with Lipschitz constant L enters through S (pass L * S).  A non-finite result has excess +inf.
U32 = 2.0 ** -24
U_BF16 = 2.0 ** -8


def gemm_excess(got, ref64, S64, K, out_dtype, extra=0.0, c=2.0):
    """|got - ref| / bound per element (fp64, on ref64's device); the caller asserts max <= 1 (assert_excess)."""
    ref = ref64.double()
    g = got.detach().to(ref.device).double()
    if torch.is_tensor(extra):
        extra = extra.to(ref.device).double()
    bound = c * (K + 3) * U32 * S64.to(ref.device).double() + extra
    if out_dtype == torch.bfloat16:
        bound = bound + U_BF16 * ref.abs()
    elif out_dtype != torch.float32:
        raise TypeError("gemm_excess: fp32 or bf16 outputs, got %s" % out_dtype)
    err = (g - ref).abs()
    inf = torch.full_like(err, float("inf"))
    # a zero bound (ref == 0 and S == 0) admits only the exact value
    exc = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err == 0, torch.zeros_like(err), inf))
    return torch.where(torch.isfinite(g), exc, inf)


def excess_argmax(exc):
    """(largest excess, its index as a tuple) of a gemm_excess tensor."""
    flat = int(torch.argmax(exc.reshape(-1)))
    idx = tuple(int(i) for i in np.unravel_index(flat, tuple(exc.shape))) if exc.dim() else ()
    return float(exc.reshape(-1)[flat]), idx


def assert_excess(exc, what):
    """max(exc) <= 1, with the arg-max index (row, column) in the message; returns the maximum."""
    mx, idx = excess_argmax(exc)
    assert mx <= 1.0, "%s: |err| / bound = %.3f at index %s (row %s, column %s); %d of %d elements over the bound" % (
        what, mx, idx, idx[-2] if len(idx) > 1 else 0, idx[-1] if idx else 0, int((exc > 1).sum()), exc.numel())
    return mx
