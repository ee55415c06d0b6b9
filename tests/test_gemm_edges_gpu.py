"""Edge tiles of csrc/gemm.hip under every pinned tile, checked element by element, with write canaries.

Every case (gemm_edge_cases.Case) steps one row or column past a 64 or a 128 tile edge, has its operands inside NaN
moats and its outputs inside sentinel buffers, and is compared with an fp64 reference of the same rounded inputs through
helpers.gemm_excess: |err| <= 2^-8 |ref| (bf16 store) + 2 (K + 3) 2^-24 S (fp32 accumulation), derived, not fitted.
Paths: grouped launches under tile 0-4 and 7-9 (one problem, and mixed groups of three with whole and with ragged
k-tiles), single launches under every variant of xggm_gemm_set_tile, LDS-DMA with 2 and 3 stages, the generic kernel in
fp32 and bf16, batched launches, the e4m3 forward (single and grouped), the three epilogue kinds, column sums and norm
slots against the launch's own stored output, and bit-identity of everything but the norm slots across the tile pins.

Largest |err| / bound observed on an MI355X (informative; the bound is the derived one, c = 2 throughout):
  path                                               C      preact  colsum partials  colsum  e4m3 copy  norm slots
  grouped tile 0, 1, 2, 3, 4, 7, 8, 9 (each), n = 1  0.989  0.983   0.931            0.932   0.937      < 0.001
  the same tiles, three whole-k problems             0.982  0.972   0.931            0.932   0.922      < 0.001
  the same tiles, three problems, one ragged K       0.989  0.983   0.931            0.932   0.937      < 0.001
  single launch variant 1, 2, 3, 5, 6, 7, 8 (each)   0.989  0.983   0.931            0.932   0.937      < 0.001
  LDS-DMA 2 stages / 3 stages, tiles 1-4             0.982  0.972   0.878            0.186 / 0.275  0.922  < 0.001
  generic fp32                                       0.250  0.077   0.016
  generic bf16                                       0.971  0.969   0.578
  e4m3 single (variants 0, 1, 3, 5)                  0.975  0.975
  e4m3 grouped (tiles 0-3)                           0.975  0.975                            0.922
  split-K slabs M = 37 (fp32 slabs)                  0.004
  bmm_nt N = 5, bf16 / fp32 storage                  0.012 / 0.031
Every tile and variant gives the same figures because it gives the same bits (test_tiles_give_the_same_bits_at_edges).
bf16 outputs sit just under 1 as they must (the 2^-8 |ref| term is the store's own round-off); fp32 outputs and the norm
slots sit far under their accumulation bound, which is a worst case over summation orders.  No violation was seen on the
tuned kernels, so c never moved.  The one finding: the generic kernel's fp32-storage GELU was 1.010 (one element, x = -3.14,
off by 2.4e-7: the cancellation of 1 + erf behind the 1.5e-7 of erf_fast); gemm.hip now evaluates it through erfc.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from gemm_edge_cases import (BF16, F32, SHAPES, Case, e4m3_cases, matrix_cases, padded_cases)  # noqa: E402
from helpers import assert_excess, gemm_excess  # noqa: E402

DEV = "cuda"
GROUP_TILES = [0, 1, 2, 3, 4, 7, 8, 9]
PINS = [1, 2, 3, 4, 7, 8, 9]
SINGLE_VARIANTS = [1, 2, 3, 5, 6, 7, 8]
NO_SINGLE_GROUPED = 0x8000  # xggm_gemm_set_tile: single problems with whole k-tiles stay on the single-launch kernel


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


@pytest.fixture(scope="module")
def cases(ops):
    """the matrix (6 shapes x 4 operand forms x the epilogues of each form) and the padded-edge cases, built once: the
    fp64 references are shared by every test and never written"""
    by_shape = {s: matrix_cases(DEV, shapes=[s]) for s in SHAPES}
    return {"by_shape": by_shape, "matrix": [c for s in SHAPES for c in by_shape[s]], "padded": padded_cases(DEV),
            "e4m3": e4m3_cases(DEV)}


def triples(a, b, c):
    """mixed groups of three: problem i of the first shape with problems i + 7 and i + 12 of the other two, so that the
    three differ in edge shape, K and (nearly always) operand form and epilogue"""
    n = len(a)
    return [[a[i], b[(i + 7) % n], c[(i + 12) % n]] for i in range(n)]


def whole_k_groups(cases):
    """every problem has whole 64-wide k-tiles: tiles 7-9 run the role k-loop"""
    s = cases["by_shape"]
    return triples(s[(65, 72, 64)], s[(129, 136, 128)], s[(63, 200, 192)]) + \
        triples(s[(1, 8, 64)], s[(63, 200, 192)], s[(129, 136, 128)])


def ragged_k_groups(cases):
    """one problem per group has a ragged k-tile (K = 72, 200, or K = 100 behind a padded stride): the group leaves
    LDS-DMA for that problem, and tiles 7-9 fall back to the four-wave tile of the same shape"""
    s, pad = cases["by_shape"], cases["padded"]
    tails = [c for c in pad if c.K == 100]
    return triples(s[(100, 264, 72)], s[(129, 136, 128)], s[(63, 200, 192)]) + \
        triples(s[(180, 136, 200)], s[(65, 72, 64)], s[(1, 8, 64)]) + \
        [[t, s[(65, 72, 64)][3 * i], s[(63, 200, 192)][3 * i + 1]] for i, t in enumerate(tails)]


def launch(ops, group, tile, dt=BF16):
    for c in group:
        c.reset()
    ops.gemm_group(dt, [c.problem(ops) for c in group], tile=tile)
    for c in group:
        c.reduce_colsum(ops)


def run(ops, groups, tile, tag, dt=BF16):
    """launch every group, check every case; prints and returns the largest |err| / bound per checked quantity"""
    worst = {}
    for group in groups:
        launch(ops, group, tile, dt)
        for c in group:
            for k, v in c.check(tag).items():
                worst[k] = max(worst.get(k, 0.0), v)
    print("EDGE-MAX %s: %s" % (tag, ", ".join("%s %.3f" % kv for kv in sorted(worst.items()))))
    return worst


# ---- grouped launches ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", GROUP_TILES)
def test_grouped_one_problem(ops, cases, tile):
    """n = 1: problems with whole k-tiles take the grouped LDS-DMA kernel (tiles 7-9: the role k-loop) under the pinned
    tile, the others the single-launch kernel of the library's choice"""
    run(ops, [[c] for c in cases["matrix"] + cases["padded"]], tile, "grouped tile %d, n = 1" % tile)


@pytest.mark.parametrize("tile", GROUP_TILES)
def test_grouped_mixed_whole_k(ops, cases, tile):
    run(ops, whole_k_groups(cases), tile, "grouped tile %d, three whole-k problems" % tile)


@pytest.mark.parametrize("tile", GROUP_TILES)
def test_grouped_mixed_ragged_k(ops, cases, tile):
    run(ops, ragged_k_groups(cases), tile, "grouped tile %d, three problems, one ragged K" % tile)


# ---- single launches -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", SINGLE_VARIANTS)
def test_single_launch_variants(ops, lib, cases, variant):
    """xggm_gemm_set_tile(variant | 0x8000): every problem, whole k-tiles or not, on the pinned single-launch kernel
    (1 / 2: 64 x 64 depth 2 / 4, 3: 128 x 64, 5: 128 x 128, 6-8: the same tiles at depth 1)"""
    lib.xggm_gemm_set_tile(variant | NO_SINGLE_GROUPED)
    try:
        run(ops, [[c] for c in cases["matrix"] + cases["padded"]], 0, "single launch variant %d" % variant)
    finally:
        lib.xggm_gemm_set_tile(0)


@pytest.mark.parametrize("flag,shape", [(0x800, (129, 136, 128)), (0x1000, (63, 200, 192))])
def test_lds_dma_stages(ops, lib, cases, flag, shape):
    """2 (0x800) and 3 (0x1000) LDS stages of the LDS-DMA k-loop pinned, at one edge shape each, every four- and
    eight-wave tile, alone and in a mixed group"""
    lib.xggm_gemm_set_tile(flag)
    try:
        groups = [[c] for c in cases["by_shape"][shape]] + whole_k_groups(cases)[:6]
        for tile in (1, 2, 3, 4):
            run(ops, groups, tile, "LDS-DMA %d stages, tile %d" % (2 if flag == 0x800 else 3, tile))
    finally:
        lib.xggm_gemm_set_tile(0)


# ---- the generic kernel --------------------------------------------------------------------------------------------
GENERIC_SHAPES = [(37, 50, 100), (65, 3, 7), (1, 1, 1)]
GENERIC_EPILOGUES = ("plain", "bias", "gelu_pre", "sigmoid_f32", "tanh", "bias_res", "acc", "gelugrad_colsum", "f32_acc")


@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
def test_generic_kernel(ops, lib, dt):
    """fp32 storage, and bf16 with xggm_gemm_set_generic(1): odd shapes, every operand form, element-wise loads"""
    cs = [Case(M, N, K, form, epi, DEV, dt=dt) for (M, N, K) in GENERIC_SHAPES for form in ("11", "10", "00", "01")
          for epi in GENERIC_EPILOGUES]
    lib.xggm_gemm_set_generic(1)
    try:
        run(ops, [[c] for c in cs], 0, "generic %s" % ("fp32" if dt == F32 else "bf16"), dt)
    finally:
        lib.xggm_gemm_set_generic(0)


# ---- batch > 1 with ragged M ---------------------------------------------------------------------------------------
def test_batched_ragged_rows(ops):
    """split-K slabs (the batch index walks K) with M = 37, and bmm_nt with 5 rows per batch entry"""
    M, N, K, S = 37, 72, 256, 2
    x = Case(M, N, K, "11", "plain", DEV)  # its guarded operands: x [37, 256] behind a padded stride, w made contiguous
    w = x.B.view.contiguous()
    a64, b64 = x.A.view.double(), w.double()
    worst = 0.0
    for tile in (0, 1, 2, 3, 4, 7, 8, 9):
        p, part = ops.p_fwd_splitk(x.A.view, w, S)
        ops.gemm_group(BF16, [p], tile=tile)
        for s in range(S):
            ks = slice(s * K // S, (s + 1) * K // S)
            ref, mag = a64[:, ks] @ b64[:, ks].t(), a64[:, ks].abs() @ b64[:, ks].abs().t()
            worst = max(worst, assert_excess(gemm_excess(part[s], ref, mag, K // S, F32), "split-K slab %d, tile %d" % (s, tile)))
    print("EDGE-MAX split-K slabs M = 37: C %.3f" % worst)
    for dt in (BF16, F32):
        g = torch.Generator().manual_seed(5)
        xb = torch.randn(3, 5, 64, generator=g).to(dt).to(DEV)
        out = ops.bmm_nt(xb, xb)
        x64 = xb.double()
        mx = assert_excess(gemm_excess(out, x64 @ x64.transpose(1, 2), x64.abs() @ x64.abs().transpose(1, 2), 64, F32),
                           "bmm_nt N = 5 %s" % dt)
        print("EDGE-MAX bmm_nt N = 5 %s: C %.3f" % (dt, mx))


# ---- e4m3 forward --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", [0, 1, 3, 5])
def test_e4m3_single(ops, lib, cases, tile):
    """xggm_gemm_fp8e4m3 under the pins of xggm_gemm_set_tile; reference: the fp64 product of the dequantised operands
    times sx sw"""
    from xggm_amd._lib import call, ptr, stream
    cs = [c for c in cases["e4m3"] if c.c8 is None]
    lib.xggm_gemm_set_tile(tile)
    try:
        worst = {}
        for c in cs:
            c.reset()
            v = lambda g: None if g is None else g.view
            call("xggm_gemm_fp8e4m3", ptr(c.A.view), ptr(c.B.view), ptr(c.C.view), c.M, c.N, c.K, c.a_rs, c.b_ns, c.C.ld,
                 ptr(c.sx), ptr(c.sw), ptr(c.bias.view[0]), ptr(v(c.res)), ptr(v(c.pre)), c.e["act"], int(c.e["f32"]),
                 stream())
            for k, x in c.check("e4m3 single, variant %d" % tile).items():
                worst[k] = max(worst.get(k, 0.0), x)
        print("EDGE-MAX e4m3 single variant %d: %s" % (tile, ", ".join("%s %.3f" % kv for kv in sorted(worst.items()))))
    finally:
        lib.xggm_gemm_set_tile(0)


@pytest.mark.parametrize("tile", [0, 1, 2, 3])
def test_e4m3_grouped(ops, cases, tile):
    cs = cases["e4m3"]
    n = len(cs) // 3
    groups = [[c] for c in cs] + [[cs[i], cs[n + (i + 1) % n], cs[2 * n + (i + 2) % n]] for i in range(n)]
    run(ops, groups, tile, "e4m3 grouped tile %d" % tile, "e4m3")


# ---- bit-identity across tiles -------------------------------------------------------------------------------------
def test_tiles_give_the_same_bits_at_edges(ops, cases):
    """products, gradients, pre-activations, e4m3 copies and column sums are the same bits under every tile pin, on
    edge tiles too (xggm.h: `tile`); the norm slots add in a tile-dependent order and agree to rtol 2e-6"""
    groups = [[c] for c in cases["matrix"] + cases["padded"]] + whole_k_groups(cases) + ragged_k_groups(cases)
    for gi, group in enumerate(groups):
        first = None
        for tile in PINS:
            launch(ops, group, tile)
            snaps = [c.snapshot() for c in group]
            if first is None:
                first = snaps
                continue
            for c, (bits, sq), (bits0, sq0) in zip(group, snaps, first):
                for k in bits:
                    assert torch.equal(bits[k], bits0[k]), "%s: %s differs between tile %d and tile %d (group %d of %d)" % (
                        c.name, k, PINS[0], tile, gi, len(group))
                if sq is not None:
                    torch.testing.assert_close(sq, sq0, rtol=2e-6, atol=0)
