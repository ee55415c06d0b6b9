"""The attention core with 65 .. 128 rows on a side (csrc/attention_long.hip), element by element, with write canaries, on
every path.

Every case (attention_long_cases.LongCase) has B = 3 samples of 3 heads with the mask rows "all keys", "half the keys" and
"exactly one key", its operands inside NaN moats, its outputs (out, dq, dk, dv, the fp32 bias partials) inside sentinel
buffers, and is compared with the fp64 reference of the same stored operands through the derived bound of
helpers.AttnRef, whose row-sum term follows the row length (max(Sk, 64) u; see attention_long_cases).  With dropout the
reference uses the keep-scales ops.dropout_mask exports for the problem's own stream id.
Paths: ``f32`` (fp32 kernels, fp32 storage), ``bf16-mfma`` (matrix cores), ``bf16-odd4`` (row stride H + 4: the alignment
rule sends the problem to the fp32-arithmetic kernels).  All launches go through the grouped entry points.
Matrix: the 13 long shapes x 3 paths, forward and backward, masked; dropout p = 0.1 and 0.5 at 6 shapes holding both
branches of the four-key Philox call; the wide layout (canaries 8 elements behind every row) at 2 shapes; a fully masked
sample; sharp softmax rows (q x 6, q x 30); every combination of bias partials, B == 1 with db_bs = 0 and the reduce launch
behind them; bit-identity of two launches; one grouped call holding short, long, short, whose short problems must give
the bits of a call without the long one.

Largest |err| / bound observed on an MI355X (informative; the bound is the derived one, c = 2 throughout):
  path / cases                              out    dq     dk     dv     bias dq  bias dk  bias dv
  f32, 13 shapes                            0.004  0.002  0.002  0.005  0.001    < 0.001  0.002
  f32, dropout 0.1 / 0.5                    0.004  0.002  0.002  0.006  < 0.001  < 0.001  0.001
  f32, wide / fully masked / sharp          0.136  0.070  0.068  0.097  0.005    < 0.001  0.002
  bf16-mfma, 13 shapes                      0.630  0.660  0.864  0.930  0.287    0.062    0.121
  bf16-mfma, dropout 0.1 / 0.5              0.690  0.659  0.700  0.632  0.067    0.064    0.166
  bf16-mfma, wide / fully masked / sharp    0.736  0.661  0.681  0.751  0.109    0.091    0.111
  bf16-mfma, short + long + short           0.625  0.654  0.660  0.698  0.093    0.079    0.115
  bf16-odd4, 13 shapes                      0.959  0.911  0.917  0.967  0.001    < 0.001  0.002
  bf16-odd4, dropout 0.1 / 0.5              0.949  0.902  0.903  0.956  < 0.001  < 0.001  0.001
  bf16-odd4, wide / fully masked / sharp    0.936  0.859  0.852  0.926  0.007    < 0.001  0.002
  reduced bias gradients (all paths)                                    0.025    0.022    0.014
The figures of the 64-row file: the fp32 arithmetic sits far under its worst-case accumulation bound (the fully masked
sample most visibly), its bf16 stores sit just under 1 as they must, the matrix-core outputs share the bound between the
store and the 2^-8 of the bf16 operands.  Every canary was intact, two launches gave the same bits, and the short
problems of a mixed call carried the bits of a call without the long one.  No violation was seen, so no term was added
and c never moved.  The whole file took 3.8 s on the MI355X (96 cases).
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from attention_cases import BF16, F32, LEAD, Case, ids, problem_array  # noqa: E402
from attention_long_cases import LONG_DROPOUT_SHAPES, LONG_SHAPES, LONG_WIDE_SHAPES, LongCase  # noqa: E402
from helpers import U32, assert_excess, bound_excess  # noqa: E402

DEV = "cuda"
B, HEADS = 3, 3
# path -> (storage type, layout in place of fused / wide, arithmetic of the bound)
PATHS = {"f32": (F32, ("fused", "wide"), "scalar"), "bf16-mfma": (BF16, ("fused", "wide"), "mfma"),
         "bf16-odd4": (BF16, ("odd4", "odd12"), "scalar")}


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from xggm_amd import ops as o
    return o


def make(path, shape, wide=False, cls=LongCase, **kw):
    dt, layouts, _ = PATHS[path]
    kw.setdefault("masked", True)
    return cls(kw.pop("B", B), kw.pop("heads", HEADS), shape[0], shape[1], dt, DEV, layout=layouts[1 if wide else 0], **kw)


def launch(ops, group, fwd=True, bwd=True, rng=None, sids=None):
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
    if fwd:
        call("xggm_attn_fwd_grouped_" + sfx, p, len(group), 64, ptr(rng), None, stream())
    if bwd:
        call("xggm_attn_bwd_grouped_" + sfx, p, len(group), 64, ptr(rng), None, stream())
    return arr


def run(ops, path, group, tag, arith=None, **kw):
    """launch, then check every case (canaries on); prints and returns the largest |err| / bound per output"""
    launch(ops, group, **kw)
    worst = {}
    for i, c in enumerate(group):
        a = PATHS[path][2] if arith is None else arith[i]
        for k, v in c.check("%s %s" % (path, tag), a, fwd=kw.get("fwd", True), bwd=kw.get("bwd", True)).items():
            worst[k] = max(worst.get(k, 0.0), v)
    print("ATTN-MAX %s | %s | %s | %s" % (path, tag, "; ".join(c.name for c in group),
                                         ", ".join("%s %.3f" % kv for kv in sorted(worst.items()))))
    return worst


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("shape", LONG_SHAPES, ids=ids)
def test_every_long_shape_on_every_path(ops, path, shape):
    run(ops, path, [make(path, shape)], "shapes")


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("shape", LONG_DROPOUT_SHAPES, ids=ids)
def test_dropout_on_every_path(ops, path, shape, p):
    """both branches of the four-key Philox call of the matrix-core kernels (one call per four keys when Sk % 4 == 0, one per
    key otherwise) and the fp32 kernels' per-element call, against the exported keep-scales"""
    run(ops, path, [make(path, shape, p=p)], "dropout")


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("shape", LONG_WIDE_SHAPES, ids=ids)
def test_wide_rows(ops, path, shape):
    """row stride H + 8 (H + 12 on the odd-stride path): sentinels right behind every row of every output"""
    run(ops, path, [make(path, shape, wide=True)], "wide")


@pytest.mark.parametrize("path", list(PATHS))
def test_fully_masked_sample(ops, path):
    """every key of sample 1 masked: all its scores shift by -10000, which is still a proper softmax"""
    run(ops, path, [make(path, (100, 36), masked=[36, 0, 1])], "fully masked sample")
    run(ops, path, [make(path, (72, 97), masked=[0, 97, 48], p=0.1)], "fully masked sample")


@pytest.mark.parametrize("path", list(PATHS))
def test_sharp_softmax(ops, path):
    """q x 6: rows that are nearly one-hot; q x 30: scores past the 88.7 where exp leaves fp32 unless the row maximum is
    subtracted first; finite and inside the bound"""
    for shape in ((72, 72), (128, 127)):
        for sharp in (6.0, 30.0):
            c = make(path, shape, sharp=sharp)
            run(ops, path, [c], "sharp")
            for t in (c.out, c.dq, c.dk, c.dv):
                assert bool(torch.isfinite(t).all())
            S = c.reference().S
            top = float(S[S > -5000].abs().max())
            assert sharp < 30 or top > 88.7


@pytest.mark.parametrize("path", list(PATHS))
def test_bias_partials(ops, path):
    """all three partial rows, only dbq, only dbk + dbv, none (the rows of a kind that was not asked for are canaries);
    B == 1 with db_bs = 0; B = 3 with db_bs = 3 H and the reduce launch behind it against the fp64 sums"""
    arith = PATHS[path][2]
    for shape in ((100, 36), (36, 100), (97, 113)):
        for db in ("qkv", "q", "kv", ""):
            run(ops, path, [make(path, shape, db=db)], "bias partials " + (db or "none"), fwd=False)
        run(ops, path, [make(path, shape, B=1, db_bs=0, masked=[max(1, shape[1] // 2)])], "bias partials B 1", fwd=False)
        c = make(path, shape, ws_heads=HEADS)  # rows of exactly H columns: [B][3][H], db_bs = 3 H
        run(ops, path, [c], "bias partials db_bs 3H", fwd=False)
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


@pytest.mark.parametrize("path", list(PATHS))
def test_two_launches_give_the_same_bits(ops, path):
    for shape, p in (((97, 113), 0.0), ((128, 128), 0.1), ((20, 100), 0.5)):
        c = make(path, shape, p=p)
        rng = ops.make_rng(77, DEV)
        launch(ops, [c], rng=rng)
        first = c.snapshot()
        launch(ops, [c], rng=rng)
        for name, buf in c.snapshot().items():
            assert torch.equal(buf.view(torch.uint8), first[name].view(torch.uint8)), \
                "%s %s: %s differs between two launches" % (c.name, path, name)
        c.check(path + " second launch", PATHS[path][2])


@pytest.mark.parametrize("path", list(PATHS))
def test_short_long_short_in_one_call(ops, path):
    """[short, long, short] in one grouped call: the short problems are paired and launched as if the long one were not
    there -- their outputs carry the bits of a call that holds only the two of them -- and the long one is inside its bound"""
    for p in (0.0, 0.1):
        s0, s1 = make(path, (36, 20), cls=Case, B=2, heads=3, p=p), make(path, (20, 36), cls=Case, B=1, heads=2, p=p)
        lg = make(path, (100, 72), B=3, heads=2, p=p)
        rng = ops.make_rng(31, DEV)
        launch(ops, [s0, s1], rng=rng, sids=[5, 8])
        alone = [c.snapshot() for c in (s0, s1)]
        arith = PATHS[path][2]
        run(ops, path, [s0, lg, s1], "short, long, short", arith=[arith] * 3, rng=rng, sids=[5, 6, 8])
        for c, ref in zip((s0, s1), alone):
            for name, buf in c.snapshot().items():
                assert torch.equal(buf.view(torch.uint8), ref[name].view(torch.uint8)), \
                    "%s %s: %s differs from the call without the long problem" % (c.name, path, name)
