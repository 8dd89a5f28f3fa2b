"""The per-source posterior of the true luminosity on the device (csrc/lf_lumpost.h, lf_lum_posterior)
against its NumPy twin (lumfuncmcmc_amd/deconv.py: lum_posterior, itself checked against 30-digit integration in
tests/test_lumpost_cpu.py), with the project's standing device-against-twin bound on each moment's own scale:

    n_used equal,   |m1_dev - m1_twin| <= 1e-12 s1_abs,   |m2_dev - m2_twin| <= 1e-12 m2_twin,   sigma = 0: exactly 0, 0,

then every chunk and row-tile edge, the bits (two calls; one row against a batch of equal rows), the caller's order after a
constructor that permutes, the refusals, and the model classes on top.  The row-sharing form the issue allows for FIXCOMP and
ZEVOL is not built: there is one form and nothing to compare it with."""
import ctypes
import os

import numpy as np
import pytest

import lf_deconvlib as L
from lf_testlib import O, make_inputs, synth
from lumfuncmcmc_amd import deconv as D
from test_gpu_deconv_wide import edge_case, mixed_sigma, rows37

pytestmark = pytest.mark.gpu
TOL = 1e-12
ORDERS = (4, 32)
GOLDENS = [("free_n50", "free"), ("fixcomp_n50", "fixcomp"), ("zevol_n800", "zevol")]
VARIANTS = ["free", "fixcomp", "zevol"]


def _rt():
    from lumfuncmcmc_amd import capi
    return capi.lum_posterior_info()["row_tile"]


def check(ctx, inp, th, sg, K, label, wide=True):
    """one call on the device against the twin, the context's errors set here; returns the device's (m1, m2, n_used)"""
    ctx.set_lum_err(sg, K, wide=wide)
    m1, m2, used = ctx.lum_posterior(th)
    t1, t2, tu, s1 = D.lum_posterior(inp, sg, th, K=K, wide=wide, terms=True)
    assert used == tu, (label, K, used, tu)
    off = sg == 0.0
    assert np.all(m1[off] == 0.0) and np.all(m2[off] == 0.0), "%s K=%d: a source with sigma = 0 is not exactly 0" % (label, K)
    if used == 0:
        assert np.all(np.isnan(m1[~off])) and np.all(np.isnan(m2[~off])), (label, K)
        return m1, m2, used
    on = ~off
    assert np.all(np.isfinite(t1[on])) and np.all(t2[on] > 0.0) and np.all(s1[on] > 0.0), (label, K)
    w1 = float(np.max(np.abs(m1[on] - t1[on]) / s1[on])) if on.any() else 0.0
    w2 = float(np.max(np.abs(m2[on] - t2[on]) / t2[on])) if on.any() else 0.0
    print("lum posterior %-30s K=%2d rows %2d used %2d: max |dev - twin| / bound = %.3e (m1), %.3e (m2)"
          % (label, K, len(np.atleast_2d(th)), used, w1 / TOL, w2 / TOL))
    assert w1 <= TOL and w2 <= TOL, (label, K, w1, w2)
    return m1, m2, used


@pytest.mark.parametrize("name,variant", GOLDENS)
def test_device_against_twin_goldens(golden_dir, name, variant):
    """sigma up to the wide rule's top edge with a tenth at 0, K = 4 and 32, 37 rows (two launch groups) of which one lies
    outside the box and one underflows"""
    from lumfuncmcmc_amd.capi import LFContext
    g = np.load(os.path.join(golden_dir, name + ".npz"))
    inp = O.inputs_from_golden(g, variant)
    sg = mixed_sigma(len(inp["lum"]), 1)
    assert (sg > D.SIGMA_MAX).sum() >= 10 and (sg == 0.0).any()
    th = rows37(inp, 11)
    ctx = LFContext(inp)
    try:
        for K in ORDERS:
            _, _, used = check(ctx, inp, th, sg, K, name)
            assert 0 < used < 37
    finally:
        ctx.close()


def _edge_rows():
    rt = _rt()
    return sorted({1, rt - 1, rt, rt + 1, 2 * rt + 1} - {0})


@pytest.mark.parametrize("variant", VARIANTS)
def test_wide_chunk_edges_and_row_tile_edges(variant):
    """wide chunks of 1, CH - 1, CH, CH + 1 and 0 sources with an empty class (the edge case of tests/test_gpu_deconv_wide.py),
    R = 1, RT - 1, RT, RT + 1, 2 RT + 1 (row 3 lies outside the box: the last takes a skipped row)"""
    from lumfuncmcmc_amd.capi import LFContext
    inp, sg = edge_case(variant)
    th = rows37(inp, 7)
    ctx = LFContext(inp)
    try:
        for R in _edge_rows():
            _, _, used = check(ctx, inp, th[:R], sg, 32, "%s wide edges R=%d" % (variant, R))
            assert used == int(np.isfinite(ctx.lnprob_batch(th[:R])).sum()) and (used < R) == (R > 3)
    finally:
        ctx.close()


@pytest.mark.parametrize("variant", VARIANTS)
def test_narrow_chunk_edges(variant):
    """fields of DECONV_CH - 1, DECONV_CH and DECONV_CH + 1 sources: full, short and one-source chunks of the narrow table"""
    from lumfuncmcmc_amd.capi import LFContext
    ch = D.CHUNK
    sizes = (ch - 1, ch, ch + 1)
    inp = make_inputs(variant, int(sum(sizes)), seed=6, S=23, nf=3)
    inp["field_ind"] = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    sg = np.random.default_rng(12).uniform(0.0, D.SIGMA_MAX, int(sum(sizes)))
    sg[::7] = 0.0
    sg[ch - 2], sg[2 * ch - 2], sg[-1] = 0.05, 0.06, 0.09          # the last source of every field is on
    th = rows37(inp, 7)
    ctx = LFContext(inp)
    try:
        for R in _edge_rows():
            check(ctx, inp, th[:R], sg, 32, "%s narrow edges R=%d" % (variant, R), wide=False)
    finally:
        ctx.close()


@pytest.mark.parametrize("variant", VARIANTS)
def test_bits(variant):
    """Two calls give the same bits.  One row alone (R = 1: exactly that row's moments, 0 + x and x / 1 being exact) against
    RT + 1 copies of it: with RT = 2 the tile's sum x + x is exact, but (2 x) + x and the division by 3 round once each, so the
    tile sums are NOT exact in general and the comparison is to 2 ulp of the row's own value, not np.array_equal."""
    from lumfuncmcmc_amd.capi import LFContext
    n = 1500
    inp = make_inputs(variant, n, seed=2, S=23)
    th = rows37(inp, 3)
    sg = mixed_sigma(n, 4)
    rt = _rt()
    ctx = LFContext(inp)
    try:
        ctx.set_lum_err(sg, 8, wide=True)
        a = ctx.lum_posterior(th)
        b = ctx.lum_posterior(th)
        assert a[2] == b[2] and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        on = sg > 0.0
        for r in (0, 9):
            one = ctx.lum_posterior(th[r])
            many = ctx.lum_posterior(np.repeat(th[r][None], rt + 1, axis=0))
            assert one[2] == 1 and many[2] == rt + 1
            for x, y in zip(one[:2], many[:2]):
                assert np.all(x[~on] == 0.0) and np.all(y[~on] == 0.0) and np.all(np.isfinite(x[on]))
                assert np.all(np.abs(y[on] - x[on]) <= 2.0 * np.spacing(np.abs(x[on])))
            # the row embedded among skipped rows at another position: the same bits as alone
            emb = np.repeat(th[3][None], rt + 1, axis=0)                  # (row 3 lies outside the box)
            emb[rt] = th[r]
            e = ctx.lum_posterior(emb)
            assert e[2] == 1 and np.array_equal(e[0], one[0]) and np.array_equal(e[1], one[1])
    finally:
        ctx.close()


@pytest.mark.parametrize("variant", VARIANTS)
def test_caller_order(variant):
    """800 sources in random flux order (the context sorts them when it uploads): one source with sigma > 0 at caller index j,
    narrow or wide - the output is not 0 at j only, and agrees with the twin there"""
    from lumfuncmcmc_amd.capi import LFContext
    n, j = 800, 613
    inp = make_inputs(variant, n, seed=21, S=23)
    th = rows37(inp, 5)[:5]
    ctx = LFContext(inp)
    try:
        for s in (0.07, 0.2):
            sg = np.zeros(n)
            sg[j] = s
            m1, m2, _ = check(ctx, inp, th, sg, 32, "%s one source sigma=%.2f" % (variant, s))
            assert m1[j] != 0.0 and m2[j] > 0.0 and np.count_nonzero(m1) == 1 and np.count_nonzero(m2) == 1
    finally:
        ctx.close()


def test_refusals():
    """before set_lum_err, R = 0, R above the limit, a NULL pointer, a source-sharded context: LF_ERR_ARG with a message; the
    next good call gives the bits of the one before"""
    from lumfuncmcmc_amd import capi
    from lumfuncmcmc_amd.capi import LFContext, LFError
    inp = make_inputs("free", 300, seed=4, S=23)
    th = np.ascontiguousarray(rows37(inp, 9))
    ctx = LFContext(inp)
    try:
        with pytest.raises(LFError, match="error -1.*lf_lum_posterior.*lf_set_lum_err"):
            ctx.lum_posterior(th)
        ctx.set_lum_err(np.full(300, 0.05))
        ok = ctx.lum_posterior(th)
        with pytest.raises(LFError, match="error -1.*lf_lum_posterior"):
            ctx.lum_posterior(np.zeros((0, ctx.ndim)))
        big = np.repeat(th[:1], capi.lum_posterior_info()["max_rows"] + 1, axis=0)
        with pytest.raises(LFError, match="error -1.*lf_lum_posterior.*4096"):
            ctx.lum_posterior(big)
        m = np.empty(300)
        used = ctypes.c_int(0)
        lib, p = ctx._lib, capi._ptr
        for args in ((None, 37, p(m), p(m), ctypes.byref(used)), (p(th), 37, None, p(m), ctypes.byref(used)),
                     (p(th), 37, p(m), None, ctypes.byref(used)), (p(th), 37, p(m), p(m), None)):
            assert lib.lf_lum_posterior(ctx._h, *args) == capi.LF_ERR_ARG
            assert b"lf_lum_posterior" in lib.lf_last_error(ctx._h)
        ctx.set_option("skip_grid", 1)
        with pytest.raises(LFError, match="error -1.*source-sharded"):
            ctx.lum_posterior(th)
        ctx.set_option("skip_grid", 0)
        again = ctx.lum_posterior(th)
        assert again[2] == ok[2] and np.array_equal(again[0], ok[0]) and np.array_equal(again[1], ok[1])
    finally:
        ctx.close()


def _surface(o):
    """deconvolved_luminosities on the device and with device=False over the same draws: the host path is the twin's result on
    the rows _posterior_rows gives for that seed, the device's lies within the bounds of `check` of it (its m2 rebuilt from the
    dict's spread and shift: a few roundings more)"""
    res = {}
    for dev in (True, False):
        np.random.seed(2024)
        res[dev] = o.deconvolved_luminosities(ndraws=12, device=dev)
    np.random.seed(2024)
    rows = o._posterior_rows(12, 7.5)[:, :-1]
    t1, t2, tu, s1 = D.lum_posterior(o.kernel_inputs(), np.asarray(o.lum_e, dtype=np.float64), rows, K=o.deconvolve_order, terms=True)
    d, t = res[True], res[False]
    assert sorted(d) == sorted(t) == ["lum_true", "lum_true_e", "n_used", "shift"] and d["n_used"] == t["n_used"] == tu == 12
    lum = np.asarray(o.lum)
    assert np.array_equal(t["shift"], t1) and np.array_equal(t["lum_true"], lum + t1)
    assert np.array_equal(t["lum_true_e"], np.sqrt(np.maximum(t2 - t1 * t1, 0.0)))
    assert np.all(np.abs(d["shift"] - t1) <= TOL * s1)
    m2_dev = d["lum_true_e"] ** 2 + d["shift"] ** 2
    assert np.all(np.abs(m2_dev - t2) <= TOL * t2 + 4.0 * np.spacing(t2))
    assert np.array_equal(d["lum_true"], lum + d["shift"]) and np.all(d["lum_true_e"] > 0.0)
    return d


def test_class_surface():
    """a 32-walker, 20-step seeded fit of a 1000-source mock with 0.05 dex of noise, then the per-source posterior over 12 draws
    on the device and on the host; an object without deconvolve refuses"""
    np.random.seed(5)
    o, _, _ = L.noisy_mock(1000, 0.05, 11, deconvolve=True)
    try:
        o.fit_model()
        before = np.array(o.lum)
        _surface(o)
        assert np.array_equal(before, o.lum)
    finally:
        o.close()
    plain = L.fixcomp_model(synth.catalogue(300, seed=17))
    try:
        with pytest.raises(ValueError, match="deconvolve=True"):
            plain.deconvolved_luminosities()
    finally:
        plain.close()


def test_class_surface_z():
    from lumfuncmcmc_amd.model import LumFuncMCMCz
    cat = synth.catalogue(600, seed=5)
    fi = cat["field_ind"]
    kw = dict(lum=synth.split_fields(cat["lum"], fi), lum_e=synth.split_fields(np.full(600, 0.06), fi), Flim=list(synth.FLIM),
              alpha=synth.ALPHA_C, Omega_0=list(synth.OMEGA_0), sch_al=synth.SCH_AL, nwalkers=32, nsteps=20, min_comp_frac=0.0,
              field_ind=fi)
    np.random.seed(1)
    oz = LumFuncMCMCz(synth.split_fields(cat["z"], fi), deconvolve=True, **kw)
    try:
        oz.fit_model()
        _surface(oz)
    finally:
        oz.close()
    plain = LumFuncMCMCz(synth.split_fields(cat["z"], fi), **kw)
    try:
        with pytest.raises(ValueError, match="deconvolve=True"):
            plain.deconvolved_luminosities()
    finally:
        plain.close()
