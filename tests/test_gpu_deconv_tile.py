"""The row-tiled correction kernel of the flux-error-convolved likelihood (csrc/lf_deconv_tile.h, context option "deconv_tile";
DESIGN.md section 3.20) at the shapes of tests/test_gpu_deconv.py: against the NumPy twin with that file's bound

    |dev - (lnprob + Delta_twin)| <= 1e-12 (|lnprob| + sum_i |Delta_i|),   -inf pattern identical to lnprob's,

then exact zeros, the same bits for a row whatever shares its tile (the tile holds 8 rows: batches of 1, 7, 8, 9, 37 and 300),
tiles with skipped rows, the per-row kernels within twice the bound, and the two places where the option changes nothing: a
FREE context and the gradient entries."""
import os

import numpy as np
import pytest

from lf_testlib import O, make_inputs, synth
from lumfuncmcmc_amd import deconv as D

pytestmark = pytest.mark.gpu
TOL = 1e-12
ORDERS = (4, 32)
RT = 8                                  # DECONV_RT of csrc/lf_deconv_tile.h
CH = D.CHUNK
FIELDS = {1: [(n,) for n in (1, CH - 1, CH, CH + 1)], 5: [(1, CH - 1, CH, CH + 1, 7)]}


def seeded_sigma(n, seed):
    """sigma in [0, 0.09], a tenth of the sources at exactly 0"""
    rng = np.random.default_rng(seed)
    sg = rng.uniform(0.0, 0.09, n)
    sg[rng.permutation(n)[:max(1, n // 10)]] = 0.0
    return sg


def rows37(inp, seed):
    nf = len(inp["field_ind"]) - 1
    th = synth.walkers(inp["variant"], 37, seed=seed, fix_sch_al=bool(inp["fix_sch_al"]), nf=nf)
    th[3, 0] = 39.5                      # outside the box
    th[20, 0] = 40.001                   # inside, but the bright sources underflow
    if inp["variant"] == "zevol":
        th[20, 0:3] = 40.001
    return th


def check_case(inp, th, label, seed=1):
    """tile against the twin (the bound above) and against the per-row kernels (twice the bound); the largest ratios"""
    from lumfuncmcmc_amd.capi import LFContext
    sg = seeded_sigma(len(inp["lum"]), seed)
    ctx = LFContext(inp)
    try:
        lp = ctx.lnprob_batch(th)
        fin = np.isfinite(lp)
        for K in ORDERS:
            ctx.set_lum_err(sg, K, unchecked=True)
            ctx.set_option("deconv_tile", 0)
            row = ctx.lnprob_err_batch(th)
            ctx.set_option("deconv_tile", 1)
            dev = ctx.lnprob_err_batch(th)
            tot, _, sabs = D.delta(inp, sg, th, K=K, terms=True)
            for v in (dev, row):
                assert np.array_equal(np.isneginf(v), np.isneginf(lp)) and not np.isnan(v).any(), "%s K=%d: -inf pattern" % (label, K)
            bound = np.abs(lp[fin]) + sabs[fin]
            w = float((np.abs(dev[fin] - (lp[fin] + tot[fin])) / bound).max()) if fin.any() else 0.0
            w2 = float((np.abs(dev[fin] - row[fin]) / bound).max()) if fin.any() else 0.0
            print("deconv_tile %-30s K=%2d rows %2d finite, max |tile - twin| / bound = %.3e, max |tile - per-row| / (2 bound) = %.3e"
                  % (label, K, int(fin.sum()), w / TOL, w2 / (2 * TOL)))
            assert w <= TOL, (label, K, w)
            assert w2 <= 2 * TOL, (label, K, w2)
    finally:
        ctx.close()


@pytest.mark.parametrize("name,variant", [("fixcomp_n50", "fixcomp"), ("zevol_n800", "zevol")])
def test_tile_against_twin_goldens(golden_dir, name, variant):
    g = np.load(os.path.join(golden_dir, name + ".npz"))
    check_case(O.inputs_from_golden(g, variant), np.asarray(g["theta"], dtype=np.float64), name)


@pytest.mark.parametrize("variant", ["fixcomp", "zevol"])
@pytest.mark.parametrize("nf", [1, 5])
def test_tile_against_twin_chunk_edges(variant, nf):
    """1, chunk - 1, chunk and chunk + 1 sources in a field"""
    for sizes in FIELDS[nf]:
        inp = make_inputs(variant, int(sum(sizes)), seed=5 + sizes[0], S=23, nf=nf)
        inp["field_ind"] = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        check_case(inp, rows37(inp, 7)[:12], "%s nf=%d sizes=%s" % (variant, nf, sizes), seed=sizes[0])


@pytest.mark.parametrize("variant", ["fixcomp", "zevol"])
def test_tile_bits(variant):
    """sigma = 0 everywhere: lf_lnprob_batch's bits; a row alone (B = 1) and in batches of 7, 8, 9, 37 and a permuted 300,
    twice, and through the device entry point on a stream of its own: the same bits"""
    import torch
    from lumfuncmcmc_amd.capi import LFContext
    inp = make_inputs(variant, 4500, seed=2, S=23)
    th = rows37(inp, 3)
    rng = np.random.default_rng(5)
    idx = rng.integers(0, 37, 300)
    idx[:37] = rng.permutation(37)
    ctx = LFContext(inp)
    try:
        ctx.set_option("deconv_tile", 1)
        lp = ctx.lnprob_batch(th)
        ctx.set_lum_err(np.zeros(4500))
        assert np.array_equal(ctx.lnprob_err_batch(th), lp)
        ctx.set_lum_err(seeded_sigma(4500, 4), 8, unchecked=True)
        e37 = ctx.lnprob_err_batch(th)
        assert np.array_equal(ctx.lnprob_err_batch(th), e37)
        assert np.array_equal(np.array([ctx.lnprob_err_batch(th[i:i + 1])[0] for i in range(37)]), e37)
        for B in (RT - 1, RT, RT + 1):
            for lo in (0, 5, 37 - B):
                assert np.array_equal(ctx.lnprob_err_batch(th[lo:lo + B]), e37[lo:lo + B]), (B, lo)
        assert np.array_equal(ctx.lnprob_err_batch(th[idx]), e37[idx])
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            dev = ctx.lnprob_err_torch(torch.from_numpy(th).cuda())
            dev300 = ctx.lnprob_err_torch(torch.from_numpy(th[idx]).cuda())
        st.synchronize()
        assert np.array_equal(dev.cpu().numpy(), e37) and np.array_equal(dev300.cpu().numpy(), e37[idx])
        assert np.isfinite(e37).sum() >= 30 and np.any(e37[np.isfinite(e37)] != lp[np.isfinite(e37)])
    finally:
        ctx.close()


@pytest.mark.parametrize("variant", ["fixcomp", "zevol"])
def test_tiles_with_skipped_rows(variant):
    """rows outside the box and underflowing rows share tiles with finite ones, one tile has no finite row at all and a finite
    tile follows it: every finite row has the bits it has alone, every other row is -inf"""
    from lumfuncmcmc_amd.capi import LFContext
    inp = make_inputs(variant, 2300, seed=8, S=23)
    th = rows37(inp, 11)
    out, under = th[3], th[20]
    good = [i for i in range(37) if i not in (3, 20)]
    rows = []
    rows += [th[good[0]], out, th[good[1]], under, th[good[2]], th[good[3]], out, th[good[4]]]     # tile 0: mixed
    rows += [out, under] * (RT // 2)                                                               # tile 1: nothing finite
    rows += [th[i] for i in good[5:5 + RT]]                                                        # tile 2: all finite
    rows += [under] + [th[i] for i in good[13:13 + RT - 2]] + [out]                                # tile 3: its ends skipped
    rows += [out, th[good[20]], th[good[21]]]                                                      # tile 4: partial
    rows = np.array(rows)
    assert len(rows) == 4 * RT + 3
    ctx = LFContext(inp)
    try:
        ctx.set_option("deconv_tile", 1)
        ctx.set_lum_err(seeded_sigma(2300, 6), 8, unchecked=True)
        lp = ctx.lnprob_batch(rows)
        fin = np.isfinite(lp)
        assert not fin[RT:2 * RT].any() and fin[2 * RT:3 * RT].all() and fin.sum() == len(rows) - RT - 6
        got = ctx.lnprob_err_batch(rows)
        alone = np.array([ctx.lnprob_err_batch(r[None])[0] for r in rows])
        assert np.array_equal(got, alone)
        assert np.array_equal(np.isneginf(got), ~fin) and not np.isnan(got).any()
        assert np.any(got[fin] != lp[fin])
    finally:
        ctx.close()


def test_free_context_takes_the_option_without_effect():
    from lumfuncmcmc_amd.capi import LFContext
    inp = make_inputs("free", 2300, seed=4, S=23)
    th = rows37(inp, 9)
    ctx = LFContext(inp)
    try:
        ctx.set_lum_err(seeded_sigma(2300, 3), 8, unchecked=True)
        off = ctx.lnprob_err_batch(th)
        ctx.set_option("deconv_tile", 1)
        on = ctx.lnprob_err_batch(th)
        ctx.set_option("deconv_tile", 0)
        assert np.array_equal(on, off) and np.array_equal(ctx.lnprob_err_batch(th), off)
        assert np.isfinite(off).sum() >= 30
    finally:
        ctx.close()


@pytest.mark.parametrize("variant", ["fixcomp", "zevol"])
def test_gradient_ignores_the_option(variant):
    """lf_lnprob_err_grad_batch: value and gradient have the same bits with the option on as off (the per-row kernels)"""
    from lumfuncmcmc_amd.capi import LFContext
    inp = make_inputs(variant, 2300, seed=12, S=23)
    th = rows37(inp, 13)
    ctx = LFContext(inp)
    try:
        ctx.set_lum_err(seeded_sigma(2300, 2), 8, unchecked=True)
        v0, g0 = ctx.lnprob_err_grad(th)
        assert np.array_equal(v0, ctx.lnprob_err_batch(th))
        ctx.set_option("deconv_tile", 1)
        v1, g1 = ctx.lnprob_err_grad(th)
        assert np.array_equal(v0, v1) and np.array_equal(g0, g1, equal_nan=True)
        assert np.isfinite(g0).any()
    finally:
        ctx.close()
