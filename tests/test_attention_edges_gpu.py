"""The attention core (csrc/attention.hip, attention_mfma.hip) at every padding border, element by element, with write
canaries, on every path.

Every case (attention_cases.Case) has B = 3 samples of 3 heads with the mask rows "all keys", "half the keys" and "exactly
one key", its operands inside NaN moats, its outputs (out, dq, dk, dv, the fp32 bias partials, the e4m3 copy) inside
sentinel buffers, and is compared with the fp64 reference of the same stored operands through the derived bound of
helpers.AttnRef (never fitted).  With dropout the reference uses the keep-scales ops.dropout_mask exports for the
problem's own stream id.
Paths: ``f32`` (scalar kernels, fp32 storage), ``bf16-mfma`` (matrix cores), ``bf16-scalar-hook`` (xggm_attn_set_scalar),
``bf16-scalar-odd4`` (row stride H + 4: mfma_ok sends the problem to the scalar kernels by itself).
Matrix: the 14 shapes x 4 paths, forward and backward, masked; dropout p = 0.1 and 0.5 at 9 shapes holding both branches
of Drop::scale4; the wide layout (canaries 8 elements behind every row) at 3 shapes; a fully masked sample; grouped
launches (two problems of different B, heads and shape, pair + single, a scalar-path problem between two matrix-core
ones) against the reference; every combination of bias partials, B == 1 with db_bs = 0, and the reduce launch behind
them; sharp softmax rows (q x 6, and q x 30 where the scores pass exp's fp32 range); the e4m3 copy and its amax slot;
bit-identity of two launches.

Largest |err| / bound observed on an MI355X (informative; the bound is the derived one, c = 2 throughout):
  path / cases                              out    dq     dk     dv     bias dq  bias dk  bias dv
  f32, all but the fully masked sample      0.004  0.003  0.004  0.007  0.001    0.001    0.002
  f32, fully masked sample                  0.111  0.062  0.076  0.139  0.012    < 0.001  0.006
  bf16-mfma, 14 shapes                      0.602  0.670  0.767  0.824  0.493    0.189    0.274
  bf16-mfma, dropout 0.1 / 0.5              0.824  0.707  0.800  0.839  0.469    0.395    0.754
  bf16-mfma, wide / fully masked / sharp    0.743  0.680  0.691  0.802  0.140    0.167    0.141
  bf16-mfma, grouped (2 and 3 problems)     0.685  0.632  0.815  0.914  0.530    0.310    0.334
  bf16-scalar-hook, 14 shapes               0.951  0.878  0.889  0.960  < 0.001  < 0.001  0.002
  bf16-scalar-hook, dropout 0.1 / 0.5       0.956  0.897  0.907  0.960  0.001    < 0.001  0.001
  bf16-scalar-hook, wide / masked / sharp   0.951  0.865  0.883  0.945  0.013    < 0.001  0.004
  bf16-scalar-odd4                          the same figures as bf16-scalar-hook in every row: the same kernel, the same bits
  mfma, odd4, mfma in one call              0.943  0.866  0.880  0.916  0.105    0.105    0.080
  reduced bias gradients (all paths)                                    0.068    0.075    0.052
The e4m3 copy was bit-exact and its amax slot equal to max |out|; every canary was intact; two launches gave the same
bits.  bf16 outputs of the scalar kernels sit just under 1 as they must (the 2^-8 |ref| term is the store's own
round-off, the fp32 arithmetic in front of it adds little); the matrix-core outputs share the bound between that term and
the 2^-8 of the bf16 operands P D and dS; fp32 outputs sit far under the accumulation bound, which is a worst case over
summation orders -- the fully masked sample most visibly, whose scores near -10000 carry the 2 u |S| term.  No violation
was seen, so no term was added and c never moved.  The whole file took 3.9 s on the MI355X (161 cases).
A scratch build of attention_mfma.hip whose forward kernel lets the zero-padded key columns up to the 16-wide tile edge
into the softmax (score 0) failed test_every_shape_on_every_path[*-bf16-mfma] at exactly the 11 shapes with
Sk % 16 != 0 (|err| / bound 89 - 124 on out) and passed 16 x 16, 63 x 64 and 64 x 64.
"""
import contextlib

import pytest
import torch

pytestmark = pytest.mark.gpu

from attention_cases import BF16, DROPOUT_SHAPES, F32, LEAD, SHAPES, WIDE_SHAPES, Case, ids, problem_array  # noqa: E402
from helpers import U32, assert_excess, bound_excess  # noqa: E402

DEV = "cuda"
B, HEADS = 3, 3
# path -> (storage type, layout in place of fused / wide, scalar hook, arithmetic of the bound)
PATHS = {"f32": (F32, ("fused", "wide"), False, "scalar"), "bf16-mfma": (BF16, ("fused", "wide"), False, "mfma"),
         "bf16-scalar-hook": (BF16, ("fused", "wide"), True, "scalar"),
         "bf16-scalar-odd4": (BF16, ("odd4", "odd12"), False, "scalar")}


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from xggm_amd import ops as o
    return o


@pytest.fixture(scope="module")
def lib():
    from xggm_amd import _lib
    return _lib.lib


@contextlib.contextmanager
def scalar_hook(lib, on):
    """bf16 on the scalar kernels while the block runs; always reset"""
    if on:
        lib.xggm_attn_set_scalar(1)
    try:
        yield
    finally:
        if on:
            lib.xggm_attn_set_scalar(0)


def make(path, shape, wide=False, **kw):
    dt, layouts, _, _ = PATHS[path]
    kw.setdefault("masked", True)
    return Case(kw.pop("B", B), kw.pop("heads", HEADS), shape[0], shape[1], dt, DEV, layout=layouts[1 if wide else 0], **kw)


def launch(ops, lib, group, hook, fwd=True, bwd=True, rng=None, sids=None):
    """one grouped forward and / or backward call over ``group``; with dropout every case takes its keep-scales from the
    export of its own stream id"""
    from xggm_amd._lib import call, ptr, stream
    sids = list(range(11, 11 + len(group))) if sids is None else sids
    if any(c.p > 0 for c in group):
        rng = ops.make_rng(20240 + group[0].Sq, DEV) if rng is None else rng
        for c, sid in zip(group, sids):
            if c.p > 0:
                c.set_keep(ops.dropout_mask(c.B * c.heads * c.Sq * c.Sk, c.p, rng, sid, DEV))
    for c in group:
        c.reset()
    arr, p = problem_array(ops, group, sids)
    sfx = ops.sfx(group[0].dt)
    with scalar_hook(lib, hook):
        if fwd:
            call("xggm_attn_fwd_grouped_" + sfx, p, len(group), 64, ptr(rng), None, stream())
        if bwd:
            call("xggm_attn_bwd_grouped_" + sfx, p, len(group), 64, ptr(rng), None, stream())
    return arr


def run(ops, lib, path, group, tag, arith=None, **kw):
    """launch, then check every case (canaries on); prints and returns the largest |err| / bound per output"""
    _, _, hook, arithmetic = PATHS[path]
    launch(ops, lib, group, hook, **kw)
    worst = {}
    for i, c in enumerate(group):
        a = arithmetic if arith is None else arith[i]
        for k, v in c.check("%s %s" % (path, tag), a, fwd=kw.get("fwd", True), bwd=kw.get("bwd", True)).items():
            worst[k] = max(worst.get(k, 0.0), v)
    print("ATTN-MAX %s | %s | %s | %s" % (path, tag, "; ".join(c.name for c in group),
                                         ", ".join("%s %.3f" % kv for kv in sorted(worst.items()))))
    return worst


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_every_shape_on_every_path(ops, lib, path, shape):
    run(ops, lib, path, [make(path, shape)], "shapes")


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("shape", DROPOUT_SHAPES, ids=ids)
def test_dropout_on_every_path(ops, lib, path, shape, p):
    """both branches of Drop::scale4 (one Philox call per four keys when Sk % 4 == 0, one per key otherwise) and the
    scalar kernels' per-element call, against the exported keep-scales"""
    run(ops, lib, path, [make(path, shape, p=p)], "dropout")


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("shape", WIDE_SHAPES, ids=ids)
def test_wide_rows(ops, lib, path, shape):
    """row stride H + 8 (H + 12 on the odd-stride path): sentinels right behind every row of every output"""
    run(ops, lib, path, [make(path, shape, wide=True)], "wide")


@pytest.mark.parametrize("path", list(PATHS))
def test_fully_masked_sample(ops, lib, path):
    """every key of sample 1 masked: all its scores shift by -10000, which is still a proper softmax"""
    run(ops, lib, path, [make(path, (20, 36), masked=[36, 0, 1])], "fully masked sample")
    run(ops, lib, path, [make(path, (33, 31), masked=[0, 31, 15], p=0.1)], "fully masked sample")


@pytest.mark.parametrize("path", list(PATHS))
def test_sharp_softmax(ops, lib, path):
    """q x 6: scores up to 27 and rows that are nearly one-hot; q x 30: scores up to 135, past the 88.7 where exp leaves
    fp32 unless the row maximum is subtracted first; finite and inside the bound"""
    for shape in ((36, 36), (64, 63)):
        for sharp in (6.0, 30.0):
            c = make(path, shape, sharp=sharp)
            run(ops, lib, path, [c], "sharp")
            for t in (c.out, c.dq, c.dk, c.dv):
                assert bool(torch.isfinite(t).all())
            S = c.reference().S
            top = float(S[S > -5000].abs().max())
            print("sharp %s: largest |score| of an unmasked key %.1f" % (c.name, top))
            assert sharp < 30 or top > 88.7


@pytest.mark.parametrize("path", ["f32", "bf16-mfma"])
def test_grouped_launches_against_the_reference(ops, lib, path):
    """two problems of different B, heads and shape in one call (the segment split and the shared LDS size), and three
    (pair + single), forward and backward, with dropout in one of the groups and a stream id per problem"""
    groups = [[make(path, (1, 7), B=2, heads=3), make(path, (64, 64), B=3, heads=2)],
              [make(path, (64, 64), B=1, heads=2), make(path, (1, 7), B=3, heads=1)],
              [make(path, (36, 36), B=3, heads=3, p=0.1), make(path, (20, 20), B=1, heads=2, p=0.1)],
              [make(path, (17, 15), B=2, heads=1), make(path, (36, 20), B=1, heads=3), make(path, (49, 47), B=3, heads=2)],
              [make(path, (33, 31), B=1, heads=2, p=0.5), make(path, (15, 17), B=3, heads=1, p=0.5),
               make(path, (64, 63), B=2, heads=2, p=0.5)]]
    for g in groups:
        run(ops, lib, path, g, "grouped %d" % len(g), sids=[5 + 3 * i for i in range(len(g))])


def test_scalar_problem_between_two_matrix_core_ones(ops, lib):
    """[mfma-eligible, odd4, mfma-eligible] in one bf16 call: the pending matrix-core problem is flushed as a single,
    the odd-stride one runs on the scalar kernel, the third is launched alone behind it"""
    for p in (0.0, 0.1):
        g = [make("bf16-mfma", (36, 20), B=2, heads=3, p=p), make("bf16-scalar-odd4", (17, 15), B=3, heads=2, p=p),
             make("bf16-mfma", (20, 36), B=1, heads=1, p=p)]
        run(ops, lib, "bf16-mfma", g, "mfma, odd4, mfma", arith=["mfma", "scalar", "mfma"])


@pytest.mark.parametrize("path", list(PATHS))
def test_bias_partials(ops, lib, path):
    """all three partial rows, only dbq, only dbk + dbv, none (the rows of a kind that was not asked for are canaries);
    B == 1 with db_bs = 0; B = 3 with db_bs = 3 H and the reduce launch behind it against the fp64 sums"""
    arith = PATHS[path][3]
    for shape in ((17, 15), (36, 20), (64, 64)):
        for db in ("qkv", "q", "kv", ""):
            run(ops, lib, path, [make(path, shape, db=db)], "bias partials " + (db or "none"), fwd=False)
        run(ops, lib, path, [make(path, shape, B=1, db_bs=0, masked=[max(1, shape[1] // 2)])], "bias partials B 1", fwd=False)
        c = make(path, shape, ws_heads=HEADS)  # rows of exactly H columns: [B][3][H], db_bs = 3 H
        run(ops, lib, path, [c], "bias partials db_bs 3H", fwd=False)
        # second stage: target += sum_b partial[b], fp32 additions in index order
        gen = torch.Generator().manual_seed(3)
        t0 = [torch.randn(c.H, generator=gen).to(DEV) for _ in range(3)]
        tg = [t.clone() for t in t0]
        ops.reduce_batch([(c.ws.buf[LEAD:LEAD + 3 * c.B], c.B, 3, c.H, tuple(tg))])
        R = c.reference()
        for name, t, t_old in zip(("dq", "dk", "dv"), tg, t0):
            ref, bound = R.bias_bound(name, arith == "mfma")
            # the partials' own bounds summed over b, plus the B additions onto the running value
            mag = t_old.double().cpu().abs() + ref.abs().sum(0)
            exc = bound_excess(t.double().cpu(), t_old.double().cpu() + ref.sum(0), bound.sum(0) + (c.B + 1) * U32 * mag)
            mx = assert_excess(exc, "%s reduced %s" % (c.name, name))
            print("ATTN-MAX %s | reduced bias gradient | %s | b%s %.3f" % (path, c.name, name, mx))


@pytest.mark.parametrize("shape", [(17, 15), (64, 64)], ids=ids)
def test_e4m3_copy(ops, lib, shape):
    """the matrix-core forward writes the context a second time as e4m3: bit-exact from the stored bf16 value, canaries
    in the byte buffer (row stride H + 8 bytes), the amax slot equal to max |out|"""
    c = make("bf16-mfma", shape, wide=True, out8=True)
    run(ops, lib, "bf16-mfma", [c], "e4m3 copy", bwd=False)  # check(): the copy, its canaries and amax
    assert float(c.amax) > 0.5 * 448 / float(c.q8)  # the recorded maximum is past the entry's recording threshold


@pytest.mark.parametrize("path", list(PATHS))
def test_two_launches_give_the_same_bits(ops, lib, path):
    _, _, hook, _ = PATHS[path]
    for shape, p in (((33, 31), 0.0), ((64, 64), 0.1), ((20, 36), 0.5)):
        c = make(path, shape, p=p)
        rng = ops.make_rng(77, DEV)
        launch(ops, lib, [c], hook, rng=rng)
        first = c.snapshot()
        launch(ops, lib, [c], hook, rng=rng)
        for name, buf in c.snapshot().items():
            assert torch.equal(buf.view(torch.uint8), first[name].view(torch.uint8)), \
                "%s %s: %s differs between two launches" % (c.name, path, name)
        c.check(path + " second launch", PATHS[path][3])
