"""The row kernels of csrc/rowops.hip on every predicated path, checked element by element, with write canaries.

Every case (row_cases.RowCase) has its operands inside NaN moats and its outputs inside sentinel buffers and is compared
with an fp64 reference of the same stored operands through the bounds of helpers.py (ln_terms, ln_out_bound,
ln_bwd_terms, colsum_bound: derived, not fitted; c = 2).  Canaries are asserted first, then every element of every
output with nothing excluded.
  * LayerNorm family: H in LN_H (every NV of DISPATCH_NV full and with a partly filled last vector, the two widths that
    run with one whole vector switched off, both sides of ln_bwd's fused-tail limit) x M in LN_M (fewer rows than waves,
    one and two workgroups, three backward workgroups) x fp32 / bf16 x the variants of row_cases (bias, residual, z_out,
    both dropouts, accumulate with out_scale, split-K input of 1 / 2 / 4 / 5 / 8 slabs, 1-4 summed terms, d_res fresh
    and accumulated, gelu_aux, each gradient vector null in turn, pre-filled gradient vectors), grouped launches
    bit-equal to the separate ones, the deferred reduction through reduce_batch, a constant row,
  * one case per grid cap at H = 8 (the only cases where a wave takes a second row),
  * embeddings (duplicate and padding ids, with and without segment ids, every table gradient, the padding row exactly
    zero), visual embeddings (all ten gradient vectors, the stride-4 columns of dWb), column sums (ld = N and N + 8 with
    NaN in the gap),
  * refusals: RuntimeError with the entry point's own message, every output still sentinel.

Largest |err| / bound observed on an MI355X (informative; the bound is the derived one, c = 2, nothing excluded):
  output                              fp32 storage     bf16 storage
  ln_fwd z / stats / out              0.629 / 0.138 / 0.410    0.996 / 0.074 / 0.995
  ln_sum stats / out (cap case)       0.113 / 0.068            0.064 / 0.994
  ln_bwd d_in / d_res                 0.558 / 0.149            0.989 / 0.989
  ln_bwd dgamma / dbeta / dbias       0.062 / 0.067 / 0.044    0.066 / 0.018 / 0.038
  embed z / out / dz                  0.474 / 0.101 / 0.148    0.996 / 0.971 / 0.994
  embed dword / dpos / dgamma         0.425 / 0.328 / 0.270    0.316 / 0.325 / 0.287
  visn z1 / z2 / out / du             0.250 / 0.182 / 0.069 / 0.138    0.995 / 0.994 / 0.994 / 0.995
  visn the six vectors / dWb          0.112 / 0.029            0.109 / 0.017
  grid caps (M = 2059 .. 32771)       every output inside the figures above
No kernel left its bound or touched a canary: rowops.hip is unchanged.  bf16 outputs sit just under 1 as they must; the
fp32 outputs and the statistics sit well under bounds that are a worst case over summation orders.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from row_cases import (BF16, BWD_VARIANTS, COLSUM_M, COLSUM_N, EMBED_H, EMBED_T, EPS, F32, FWD_VARIANTS, LN_H, LN_M,  # noqa: E402
                       SID_POST, SID_PRE, SUM_VARIANTS, VISN_H, VISN_M, RowCase, launch_bwd_group, launch_fwd_group, sfx,
                       snapshot)

DEV = "cuda"
DTS = [F32, BF16]


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from xggm_amd import ops as o
    return o


@pytest.fixture(scope="module")
def rng(ops):
    return ops.make_rng(1234, DEV)


@pytest.fixture(scope="module")
def mask_fn(ops, rng):
    """the kernels' own keep-scales: ops.dropout_mask with the same state and stream ids (pinned in test_glue_gpu.py)"""
    return lambda n, p, sid: ops.dropout_mask(n, p, rng, sid, DEV)


@pytest.fixture(autouse=True)
def stop_after_a_gpu_error():
    """a HIP error (an illegal access, say) ends the session here: nothing more is started on a device that faulted"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit("GPU error during a row-edge test: %s" % e, returncode=3)


def go(ops, rng, mask_fn, kind, M, H, dt, tag="single", **opt):
    c = RowCase(kind, M, H, dt, DEV, mask_fn=mask_fn, **opt)
    if "ws" in c.outs:  # the window is exactly what the library reports; everything behind it is canary
        fn = {"ln_bwd": "xggm_ln_bwd_workspace_bytes", "embed": "xggm_ln_bwd_workspace_bytes",
              "visn": "xggm_visn_embed_bwd_workspace_bytes", "colsum": "xggm_colsum_workspace_bytes"}[kind]
        assert getattr(ops._lib.lib, fn)(M, H) == c.outs["ws"].cols * 4, (c.name, fn)
    c.launch(ops, rng)
    return c, c.check(tag)


def same_bits(a, b):
    return all(torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)) for k in a)


@pytest.mark.parametrize("dt", DTS, ids=sfx)
@pytest.mark.parametrize("H", LN_H)
def test_ln_fwd(ops, rng, mask_fn, H, dt):
    worst = {}
    for M in LN_M:
        for name, opt in FWD_VARIANTS.items():
            _, mx = go(ops, rng, mask_fn, "ln_fwd", M, H, dt, name, **opt)
            worst = {k: max(v, worst.get(k, 0.0)) for k, v in mx.items()}
    print("ln_fwd H=%d %s: %s" % (H, sfx(dt), worst))
    # two problems of different M in one launch: the bits of the separate launches, each inside the bound
    for opt in (FWD_VARIANTS["dropout"], FWD_VARIANTS["slabs5"]):
        cs = [RowCase("ln_fwd", M, H, dt, DEV, seed=M, mask_fn=mask_fn, **opt) for M in (7, 17)]
        alone = []
        for c in cs:
            launch_fwd_group(ops, [c], rng)
            alone.append(snapshot(c))
            c.reset()
        launch_fwd_group(ops, cs, rng)
        for c, a in zip(cs, alone):
            c.check("grouped")
            assert same_bits(snapshot(c), a), c.name
    # a constant row: finite statistics and out = beta bit for bit
    c, _ = go(ops, rng, mask_fn, "ln_fwd", 9, H, dt, "constant row", const=True)
    assert torch.isfinite(c.outs["stats"].view).all()
    assert torch.equal(c.outs["out"].view[0].float(), c.ins["beta"].view[0].to(dt).float())


@pytest.mark.parametrize("dt", DTS, ids=sfx)
@pytest.mark.parametrize("H", LN_H)
def test_ln_sum_fwd(ops, rng, mask_fn, H, dt):
    for M in LN_M:
        for opt in SUM_VARIANTS:
            go(ops, rng, mask_fn, "ln_sum", M, H, dt, **opt)


@pytest.mark.parametrize("dt", DTS, ids=sfx)
@pytest.mark.parametrize("H", LN_H)
def test_ln_bwd(ops, rng, mask_fn, H, dt):
    worst = {}
    for M in LN_M:
        for name, opt in BWD_VARIANTS.items():
            _, mx = go(ops, rng, mask_fn, "ln_bwd", M, H, dt, name, **opt)
            worst = {k: max(v, worst.get(k, 0.0)) for k, v in mx.items()}
    print("ln_bwd H=%d %s: %s" % (H, sfx(dt), worst))
    for opt in (BWD_VARIANTS["dropout"], BWD_VARIANTS["prefill"]):
        cs = [RowCase("ln_bwd", M, H, dt, DEV, seed=M, mask_fn=mask_fn, **opt) for M in (7, 17)]
        alone = []
        for c in cs:
            c.launch(ops, rng)
            alone.append(snapshot(c))
            c.reset()
        launch_bwd_group(ops, cs, rng)
        for c, a in zip(cs, alone):
            c.check("grouped")
            assert same_bits(snapshot(c), a), c.name


@pytest.mark.parametrize("dt", DTS, ids=sfx)
@pytest.mark.parametrize("H", [4, 260])
def test_ln_bwd_deferred_reduction(ops, rng, mask_fn, H, dt):
    """the gradient vectors left in the workspace and added by reduce_batch: d_in / d_res bit-equal, vectors in the bound"""
    for M in LN_M:
        for opt in (BWD_VARIANTS["prefill"], BWD_VARIANTS["null_dbeta"], BWD_VARIANTS["dropout"]):
            c = RowCase("ln_bwd", M, H, dt, DEV, mask_fn=mask_fn, **opt)
            c.launch(ops, rng)
            c.check("immediate")
            now = snapshot(c)
            c.reset()
            c.o["defer"] = True
            c.launch(ops, rng)
            c.check("deferred")
            for k in ("d_in", "d_res"):
                if k in now:
                    assert torch.equal(now[k], c.outs[k].view), (c.name, k)


CAPS = [("ln_bwd", 2059, dict(want_dres=True, gelu=True, prefill=True)), ("visn", 2059, {}),
        ("ln_fwd", 32771, dict(bias=True, res=True, zout=True)), ("ln_sum", 32771, dict(n=2)),
        ("embed", 16387, dict(T=1)), ("visn", 16387, {})]


@pytest.mark.parametrize("dt", DTS, ids=sfx)
@pytest.mark.parametrize("kind,M,opt", CAPS, ids=["%s-%d" % (k, m) for k, m, _ in CAPS])
def test_grid_caps(ops, rng, mask_fn, kind, M, opt, dt):
    """more rows than the capped grid has waves: the only cases where a wave takes a second row"""
    _, mx = go(ops, rng, mask_fn, kind, M, 8, dt, "grid cap", **opt)
    print("%s M=%d %s: %s" % (kind, M, sfx(dt), mx))


@pytest.mark.parametrize("dt", DTS, ids=sfx)
@pytest.mark.parametrize("H", EMBED_H)
def test_embed(ops, rng, mask_fn, H, dt):
    for T in EMBED_T:
        for seg in (True, False):
            for p in (0.0, 0.1):
                _, mx = go(ops, rng, mask_fn, "embed", 3 * T, H, dt, T=T, seg=seg, p_post=p)
        print("embed H=%d T=%d %s: %s" % (H, T, sfx(dt), mx))


@pytest.mark.parametrize("dt", DTS, ids=sfx)
@pytest.mark.parametrize("H", VISN_H)
def test_visn_embed(ops, rng, mask_fn, H, dt):
    for M in VISN_M:
        for p in (0.0, 0.1):
            _, mx = go(ops, rng, mask_fn, "visn", M, H, dt, p_post=p)
    print("visn H=%d %s: %s" % (H, sfx(dt), mx))


@pytest.mark.parametrize("dt", DTS, ids=sfx)
def test_colsum(ops, rng, mask_fn, dt):
    for N in COLSUM_N:
        for M in COLSUM_M:
            for ld in (N, N + 8):
                c, _ = go(ops, rng, mask_fn, "colsum", M, N, dt, ld=ld)
                c.reset()  # and through the wrapper, which sizes its own workspace
                ops.colsum(c.ins["x"].view, c.outs["out"].view[0])
                c.outs["ws"].view.zero_()
                c.check("ops.colsum")


@pytest.mark.parametrize("dt", DTS, ids=sfx)
def test_wrappers(ops, rng, mask_fn, dt):
    """ops.ln_fwd / ops.ln_bwd / ops.ln_sum_fwd on a case's operands: the wrapper's results inside the same bounds"""
    M, H = 9, 260
    v = lambda c, nm: c.ins[nm].view[0] if c.ins[nm].rows == 1 else c.ins[nm].view
    c = RowCase("ln_fwd", M, H, dt, DEV, mask_fn=mask_fn, **FWD_VARIANTS["dropout"])
    out, z, stats = ops.ln_fwd(v(c, "in").clone(), v(c, "bias"), v(c, "residual"), v(c, "gamma"), v(c, "beta"), EPS, p_pre=0.1,
                               p_post=0.5, rng=rng, sid_pre=SID_PRE, sid_post=SID_POST)
    c.w("out", out), c.w("z_out", z), c.w("stats", stats)
    c.check("ops.ln_fwd")
    b = RowCase("ln_bwd", M, H, dt, DEV, mask_fn=mask_fn, **BWD_VARIANTS["dropout"])
    g = {nm: b.outs[nm].view[0] for nm in ("dgamma", "dbeta", "dbias")}
    d_in, d_res = ops.ln_bwd(v(b, "dy"), v(b, "z"), v(b, "stats"), v(b, "gamma"), g["dgamma"], g["dbeta"], g["dbias"],
                             want_dres=True, p_pre=0.1, p_post=0.5, rng=rng, sid_pre=SID_PRE, sid_post=SID_POST, out_scale=0.37)
    b.w("d_in", d_in), b.w("d_res", d_res)
    b.outs["ws"].view.zero_()
    b.check("ops.ln_bwd")
    s = RowCase("ln_sum", M, H, dt, DEV, mask_fn=mask_fn, n=3, p_post=0.5)
    out, stats = ops.ln_sum_fwd([v(s, "in%d" % k) for k in range(3)], [v(s, "gamma%d" % k) for k in range(3)],
                                [v(s, "beta%d" % k) for k in range(3)], EPS, 0.5, rng, [SID_POST + k for k in range(3)])
    s.w("out", out)
    for k in range(3):
        s.w("stats%d" % k, stats[k])
    s.check("ops.ln_sum_fwd")


def refused(ops, rng, c, message, launch=None):
    with pytest.raises(RuntimeError, match=message):
        (launch or c.launch)(ops, rng)
    assert c.untouched(), "%s: a refused launch wrote to an output" % c.name


@pytest.mark.parametrize("dt", DTS, ids=sfx)
def test_refusals(ops, rng, mask_fn, dt):
    kinds = (("ln_fwd", "xggm_ln_fwd", {}), ("ln_sum", "xggm_ln_sum_fwd", dict(n=2)), ("ln_bwd", "xggm_ln_bwd", {}),
             ("embed", "xggm_embed_fwd", {}), ("visn", "xggm_visn_embed_fwd", {}))
    for kind, who, opt in kinds:
        c = RowCase(kind, 9, 8, dt, DEV, mask_fn=mask_fn, **opt)
        c.H = 6
        refused(ops, rng, c, who + ": H=6 must be a multiple of 4")
        c = RowCase(kind, 9, 2052, dt, DEV, mask_fn=mask_fn, **opt)
        refused(ops, rng, c, who + ": H=2052 must be a multiple of 4 and <= 2048")
        c = RowCase(kind, 9, 8, dt, DEV, mask_fn=mask_fn, **opt)
        c.M = 0
        refused(ops, rng, c, who + ": empty input M=0")
    c = RowCase("visn", 9, 1028, dt, DEV, mask_fn=mask_fn)
    c.launch_visn_fwd(ops, rng)
    for g in c.outs.values():
        g.seal()  # the forward's results are the backward's operands: from here on nothing may change
    refused(ops, rng, c, "xggm_visn_embed_bwd: H=1028 > 1024", c.launch_visn_bwd)
    for kind, who in (("ln_bwd", "xggm_ln_bwd"), ("colsum", "xggm_colsum")):
        c = RowCase(kind, 9, 260, dt, DEV, mask_fn=mask_fn, ws_short=1)
        refused(ops, rng, c, who + ": workspace of")
    c = RowCase("visn", 9, 260, dt, DEV, mask_fn=mask_fn, ws_short=1)
    c.launch_visn_fwd(ops, rng)
    for g in c.outs.values():
        g.seal()
    refused(ops, rng, c, "xggm_visn_embed_bwd: workspace of", c.launch_visn_bwd)
