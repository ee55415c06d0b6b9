"""The element-wise attention bound (helpers.AttnRef, attn_fwd_excess / attn_bwd_excess) can fail, and the old metric
cannot: host-only.

For every (Sq, Sk) of attention_cases.SHAPES -- B = 2, two heads, one half-masked sample or no mask, no dropout or a
host-made keep mask with p = 0.1 -- both arithmetic models of the kernels are emulated in fp32 torch
(attention_cases.Case.emulate: ``mfma`` = bf16 operands P D and dS, fp32 accumulation, bf16 store; ``scalar`` = fp32
throughout with a bf16 or an fp32 store) and written through the same guarded windows the GPU test uses:
  * every emulation stays inside the derived bound with ZERO exclusions, and is not trivially exact (max > 0) except
    where it must be: with a single key the softmax is the identity, dq = dk = 0 and (without dropout) out = v, dv = dO
    bit for bit.  Largest |err| / bound of a case over out / dq / dk / dv (1 x 1 aside): 0.47 - 0.86 (mfma), 0.90 - 0.97
    (scalar, bf16 store: the store's own half ulp), 0.002 - 0.005 (scalar, fp32 store),
  * seven defects a padded tile, a clamped row or a wrong index can produce leave the bound, and the arg-max the checker
    reports lies in the corrupted row or column (see DEFECTS),
  * rel_err (a norm ratio over the whole tensor) at the suite's 1.2e-2 accepts a dropped key and a padding query row at
    36 x 36 and 64 x 64 in a launch of the training step's size (B = 32, 12 heads); the figures are printed beside each
    excess -- at B = 2 with two heads one (sample, head) is a quarter of the tensor and the norm ratio does see them,
  * a stray store into a stride gap, a row past the end or a foreign head's bias-partial columns fails check().
"""
import pytest

from attention_cases import BF16, F32, LEAD, SHAPES, Case, ids, shifted
from helpers import ATTN_D, excess_argmax, rel_err

OLD_TOL = 1.2e-2  # tests/test_kernels_gpu.py: tol(bf16)
B, HEADS = 2, 2
MODELS = {"mfma": ("mfma", BF16), "scalar-bf16": ("scalar", BF16), "scalar-f32": ("scalar", F32)}


def half_masked(Sk):
    return [Sk, max(1, Sk // 2)]


@pytest.fixture(scope="module")
def cases():
    """(shape, storage type, masked, p) -> Case, built on first use: the fp64 references are shared and never written"""
    made = {}

    def get(shape, dt, masked, p):
        key = (shape, dt, masked, p)
        if key not in made:
            c = Case(B, HEADS, shape[0], shape[1], dt, "cpu", masked=half_masked(shape[1]) if masked else False, p=p)
            made[key] = c.host_keep() if p else c
        return made[key]
    return get


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "masked"])
@pytest.mark.parametrize("model", list(MODELS))
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_emulated_kernels_stay_inside_the_bound(cases, shape, model, masked, p):
    path, dt = MODELS[model]
    c = cases(shape, dt, masked, p)
    c.reset()
    c.store(c.emulate(path))
    mx = c.check("emulated " + model, path)  # canaries, every element of every output <= 1: nothing is excluded
    print("emulated %s %s: max |err| / bound %s" % (c.name, model, ", ".join("%s %.3f" % kv for kv in sorted(mx.items()))))
    for name in ("out", "dq", "dk", "dv"):
        if shape[1] == 1 and (p == 0.0 or name in ("dq", "dk")):
            # one key: the softmax is the identity and dS = 0 -- out = v and dv = dO (without the keep-scale 1 / 0.9,
            # which is rounded) and dq = dk = 0 are exact
            assert mx[name] == 0.0, (name, mx[name])
        else:
            assert 0.0 < mx[name] <= 1.0, (name, mx[name])


def rows_of(b, S):
    return range(b * S, (b + 1) * S)


def cols_of(h):
    return range(h * ATTN_D, (h + 1) * ATTN_D)


def leaves(c, path, name, bad, rows, h, note):
    """the corrupted result leaves the bound of ``name`` and the reported arg-max lies in ``rows`` x the columns of head
    ``h``; returns (excess, rel_err of the old metric)"""
    mx, idx = excess_argmax(c.excess(name, bad[name], path))
    ref = c.reference().bias_bound(name[1:], path == "mfma")[0] if name[0] == "b" else c.reference().bound(name, c.dt, path == "mfma")[0]
    r = rel_err(bad[name], ref)
    print("%s %s: %s, %s: |err| / bound %.1f at %s, rel_err %.1e" % (c.name, path, note, name, mx, idx, r))
    assert mx > 1.0 and idx[0] in rows and idx[1] in cols_of(h), (note, name, mx, idx)
    return mx, r


@pytest.mark.parametrize("path", ["mfma", "scalar"])
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_planted_defects_leave_the_bound(cases, shape, path):
    """DEFECTS, each wherever it is defined:
      1. dropped_key     one query row renormalised without its most probable key (never the last key): out, dq
      2. padding_key     the zero key row j = Sk takes part in the softmax of one (sample, head) with score 0
                         (Sk % 16 != 0): out, dq
      3. padding_query   the padding row i = Sq enters dk / dv as a copy of the last query row (Sq % 32 != 0): dv, and
                         dk where dS is not identically zero (Sk > 1)
      4. copied_row      the last query row of a (sample, head) holds the row before it: out, dq
      5. wrong_mask_row  the mask row of sample b is applied to sample b ^ 1: out, dq
      6. shifted_keep    the dropout keep mask is one element late (p = 0.1): out
      7. short_partial   a bias partial misses its last 16-row tile (S > 16): the partial rows"""
    Sq, Sk = shape
    c = cases(shape, BF16, True, 0.0)
    b0, h0, i0 = at = (0, HEADS - 1, Sq // 2)  # sample 0 sees every key
    good = c.emulate(path)
    for name in ("out", "dq", "dk", "dv", "bdq", "bdk", "bdv"):
        assert float(c.excess(name, good[name], path).max()) <= 1.0
    row = [b0 * Sq + i0]
    if Sk > 1:
        bad = c.emulate(path, "dropped_key", at)
        for name in ("out", "dq"):
            leaves(c, path, name, bad, row, h0, "dropped key")
    if Sk % 16:
        bad = c.emulate(path, "padding_key", at)
        for name in ("out", "dq") if Sk > 1 else ("out",):
            leaves(c, path, name, bad, rows_of(b0, Sq), h0, "padding key")
    if Sq % 32:
        bad = c.emulate(path, "padding_query", at)
        for name in ("dk", "dv") if Sk > 1 else ("dv",):
            leaves(c, path, name, bad, rows_of(b0, Sk), h0, "padding query row")
    if Sq > 1:
        bad = c.emulate(path, "copied_row", at)
        for name in ("out", "dq"):
            leaves(c, path, name, bad, [b0 * Sq + Sq - 1], h0, "copied row")
    if Sk > 1:  # the two mask rows differ
        bad = c.emulate(path, "wrong_mask_row", at)
        for name in ("out", "dq"):
            mx, idx = excess_argmax(c.excess(name, bad[name], path))
            print("%s %s: wrong mask row, %s: |err| / bound %.1f at %s, rel_err %.1e" % (
                c.name, path, name, mx, idx, rel_err(bad[name], c.reference().bound(name, BF16, path == "mfma")[0])))
            assert mx > 1.0, (name, mx, idx)  # every row of both samples is corrupted
    for name, S in (("bdq", Sq), ("bdk", Sk), ("bdv", Sk)):
        if S > 16:
            bad = c.emulate(path, "short_partial", at)
            leaves(c, path, name, bad, [b0], h0, "short bias partial")
    # 6: dropout on
    d = cases(shape, BF16, True, 0.1)
    assert float(d.excess("out", d.emulate(path)["out"], path).max()) <= 1.0
    if bool((shifted(d.keep) == d.keep).all()):  # 1 x 1: four decisions, all "keep" -- a shift changes nothing
        assert shape == (1, 1)
        return
    bad = d.emulate(path, "shifted_keep", at)
    mx, idx = excess_argmax(d.excess("out", bad["out"], path))
    b, i, h = idx[0] // Sq, idx[0] % Sq, idx[1] // ATTN_D
    print("%s %s: shifted keep mask, out: |err| / bound %.1f at %s" % (d.name, path, mx, idx))
    assert mx > 1.0 and bool((shifted(d.keep)[b, h, i] != d.keep[b, h, i]).any()), (mx, idx)


@pytest.mark.parametrize("shape", [(36, 36), (64, 64)], ids=ids)
def test_rel_err_accepts_defects_1_and_3(shape):
    """the old metric at the suite's 1.2e-2 accepts a dropped key (defect 1) and a padding query row (defect 3) at 36 x 36
    and 64 x 64, where the element-wise bound is left by a wide margin.  The problem has the size of the training step's
    attention launch (B = 32, 12 heads): one (sample, head) is then 1 / 384 of the tensor.  At B = 2 with two heads one
    (sample, head) is a quarter of the tensor and even the norm ratio sees it (the figures of
    test_planted_defects_leave_the_bound: 0.03 for the dropped key, 0.06 for the padding row).  At 64 x 64 the tile has no
    padding row (64 % 32 == 0); the emulation adds the last row a second time all the same -- the same slip one row tile
    later."""
    Sq, Sk = shape
    Bt, heads = 32, 12
    c = Case(Bt, heads, Sq, Sk, BF16, "cpu", masked=[(Sk, max(1, Sk // 2), 1)[b % 3] for b in range(Bt)])
    b0, h0, i0 = at = (3, 7, Sq // 2)  # sample 3 sees every key
    for path in ("mfma", "scalar"):
        bad = c.emulate(path, "dropped_key", at)
        for name in ("out", "dq"):
            mx, r = leaves(c, path, name, bad, [b0 * Sq + i0], h0, "dropped key")
            assert r < OLD_TOL, (name, r)
        bad = c.emulate(path, "padding_query", at)
        for name in ("dk", "dv"):
            mx, r = leaves(c, path, name, bad, rows_of(b0, Sk), h0, "padding query row")
            assert r < OLD_TOL, (name, r)


def test_check_sees_stray_stores():
    """one cell outside the owned regions fails check(): a stride gap of dq (fused: the k / v columns of the gradient
    buffer; wide: the 8 elements behind a row), the row past B * Sk of dv, a foreign head's columns of a partial row"""
    for layout in ("fused", "wide"):
        c = Case(B, HEADS, 17, 15, BF16, "cpu", masked=half_masked(15), layout=layout)
        H = c.H

        def relaunch():
            c.reset()
            c.store(c.emulate("mfma"))
            c.check("emulated", "mfma")
        relaunch()
        c.dq_slab.buf[LEAD + 3, H + 2] = 1.0
        with pytest.raises(AssertionError, match="outside the region of dq"):
            c.check("stray store in a stride gap of dq", "mfma")
        relaunch()
        c.dv_slab.buf[LEAD + B * 15, (2 * H if layout == "fused" else 0) + 5] = 1.0
        with pytest.raises(AssertionError, match="outside the region of d[kv]"):
            c.check("stray store past B * Sk of dv", "mfma")
        relaunch()
        c.ws.buf[LEAD + 1, H + 7] = 1.0
        with pytest.raises(AssertionError, match="outside the region of bias partials"):
            c.check("stray store in a foreign head's partial columns", "mfma")
        relaunch()
    # partial rows of a kind that was not asked for are canaries too
    c = Case(B, HEADS, 17, 15, BF16, "cpu", masked=half_masked(15), db="q")
    c.store(c.emulate("scalar"))
    c.check("emulated", "scalar")
    c.ws.buf[LEAD + 2, 0] = 1.0
    with pytest.raises(AssertionError, match="outside the region of bias partials"):
        c.check("stray store in the dv partial row", "scalar")
