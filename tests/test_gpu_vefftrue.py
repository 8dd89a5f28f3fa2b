"""The deconvolved 1/Veff points on the device (csrc/lf_vefftrue.h, lf_veff_true) against their NumPy
twin (lumfuncmcmc_amd/deconv.py: veff_true, checked in tests/test_vefftrue_cpu.py), with the project's standing
device-against-twin bound per bin - every term is positive, so a bin's value is its own scale:

    n_used equal,   |dev - twin| <= 1e-12 twin,   a bin that is 0 in the twin is exactly 0,   an unused row is NaN,

then every chunk, row-group and bin-count edge, nodes engineered onto the edges, the bits (two calls; a row alone, in a batch
and in a permuted batch), the quantiles against NumPy on the device's own values, the refusals and the model classes on top."""
import ctypes
import os

import numpy as np
import pytest

import lf_deconvlib as L
from lf_testlib import O, make_inputs, synth
from lumfuncmcmc_amd import deconv as D
from test_gpu_deconv_wide import edge_case, mixed_sigma, rows37
from test_vefftrue_cpu import PREF0, VOL, engineered_edges

pytestmark = pytest.mark.gpu
TOL = 1e-12
GOLDENS = [("free_n50", "free"), ("fixcomp_n50", "fixcomp"), ("zevol_n800", "zevol")]
VARIANTS = ["free", "fixcomp", "zevol"]
Q = (0.0, 16.0, 50.0, 84.0, 100.0)


def _edges(inp, nbin):
    lum = np.asarray(inp["lum"])
    return np.linspace(lum.min() - 0.3, lum.max() + 0.2, nbin + 1)


def check(ctx, inp, th, sg, K, edges, label, wide=True, set_err=True):
    """one call on the device against the twin; returns the device's (out, values, n_used)"""
    if set_err:
        ctx.set_lum_err(sg, K, wide=wide)
    out, vals, used = ctx.veff_true(th, edges, PREF0, VOL, q=Q)
    tw, tu = D.veff_true(inp, sg, th, edges, PREF0, VOL, K=K, wide=wide)
    assert used == tu and vals.shape == tw.shape, (label, K, used, tu)
    off = np.isnan(tw)
    assert np.array_equal(np.isnan(vals), off), "%s K=%d: NaN pattern" % (label, K)
    assert np.array_equal(off.all(axis=1), off.any(axis=1))
    zero = tw == 0.0
    assert np.all(vals[zero] == 0.0), "%s K=%d: a bin that is 0 in the twin is not exactly 0" % (label, K)
    pos = ~off & ~zero
    w = float(np.max(np.abs(vals[pos] - tw[pos]) / tw[pos])) if pos.any() else 0.0
    print("veff true %-34s K=%2d rows %2d used %2d bins %4d (%d empty): max |dev - twin| / bound = %.3e"
          % (label, K, len(np.atleast_2d(th)), used, len(edges) - 1, int(zero[~off.any(axis=1)].all(axis=0).sum()) if used else 0, w / TOL))
    assert w <= TOL, (label, K, w)
    rows = vals[~off.any(axis=1)]
    if used:
        assert np.array_equal(out, np.percentile(rows, Q, axis=0)), "%s K=%d: quantiles" % (label, K)
    else:
        assert np.all(np.isnan(out))
    return out, vals, used


@pytest.mark.parametrize("name,variant", GOLDENS)
def test_device_against_twin_goldens(golden_dir, name, variant):
    """sigma up to the wide rule's top edge with a tenth at 0, K = 4 and 32, 37 rows (three launch groups) of which one lies
    outside the box and one underflows, 1, 25 and 1024 bins"""
    from lumfuncmcmc_amd.capi import LFContext
    g = np.load(os.path.join(golden_dir, name + ".npz"))
    inp = O.inputs_from_golden(g, variant)
    sg = mixed_sigma(len(inp["lum"]), 1)
    assert (sg > D.SIGMA_MAX).sum() >= 10 and (sg == 0.0).any()
    th = rows37(inp, 11)
    ctx = LFContext(inp)
    try:
        for K in (4, 32):
            for nbin in (1, 25, 1024):
                _, _, used = check(ctx, inp, th, sg, K, _edges(inp, nbin), name, set_err=nbin == 1)
                assert 0 < used < 37
    finally:
        ctx.close()


def _edge_rows():
    from lumfuncmcmc_amd import capi
    return (1, 2, 3, 5, capi.veff_true_info()["row_group"] + 1)


@pytest.mark.parametrize("variant", VARIANTS)
def test_wide_chunk_edges_and_row_group_edges(variant):
    """wide chunks of 1, CH - 1, CH, CH + 1 and 0 sources with an empty class, R = 1, 2, 3, 5 and one more than the row group
    (row 3 lies outside the box)"""
    from lumfuncmcmc_amd.capi import LFContext
    inp, sg = edge_case(variant)
    th = rows37(inp, 7)
    ctx = LFContext(inp)
    try:
        for i, R in enumerate(_edge_rows()):
            _, _, used = check(ctx, inp, th[:R], sg, 32, _edges(inp, 25), "%s wide edges R=%d" % (variant, R), set_err=i == 0)
            assert (used < R) == (R > 3)
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
        for i, R in enumerate((1, 5)):
            check(ctx, inp, th[:R], sg, 32, _edges(inp, 25), "%s narrow edges R=%d" % (variant, R), wide=False, set_err=i == 0)
    finally:
        ctx.close()


@pytest.mark.parametrize("variant", VARIANTS)
def test_one_source_and_lonely_bins(variant):
    """a catalogue of one source (sigma = 0, narrow and wide); then a bin that holds nodes of exactly one source - the lowest nodes of
    the faintest, below the others' reach - next to bins of none"""
    from lumfuncmcmc_amd.capi import LFContext
    one = make_inputs(variant, 1, seed=3, S=23, nf=1)
    th = rows37(one, 5)[:5]
    ctx = LFContext(one)
    try:
        for s in (0.0, 0.07, 0.2):
            _, vals, _ = check(ctx, one, th, np.array([s]), 32, _edges(one, 25), "%s one source sigma=%.2f" % (variant, s))
            assert np.all(np.nansum(vals, axis=1)[~np.isnan(vals[:, 0])] > 0.0)
    finally:
        ctx.close()
    n = 300
    inp = make_inputs(variant, n, seed=21, S=23)
    lum = np.asarray(inp["lum"], dtype=np.float64)
    sg = np.full(n, 0.03)
    x, _ = D.gauss_hermite(32)
    low = lum + (np.sqrt(2.0) * sg) * x[0]                         # every source's lowest node
    j = int(np.argmin(low))
    nxt = float(np.sort(low)[1])
    assert low[j] < nxt
    # bin 0: below every node; bin 1: the lowest nodes of the faintest source alone; bin 2: all the rest; bins 3, 4: none
    edges = np.array([low[j] - 1.0, low[j] - 1e-9, nxt, lum.max() + 1.0, lum.max() + 5.0, lum.max() + 6.0])
    ctx = LFContext(inp)
    try:
        _, vals, _ = check(ctx, inp, rows37(inp, 5)[:5], sg, 32, edges, "%s lonely bins" % variant, wide=False)
        live = ~np.isnan(vals[:, 0])
        assert np.all(vals[live, 1] > 0.0) and np.all(vals[live, 2] > 0.0) and np.all(vals[live][:, [0, 3, 4]] == 0.0)
    finally:
        ctx.close()


@pytest.mark.parametrize("variant", VARIANTS)
def test_nodes_engineered_onto_the_edges(variant):
    """edges equal to node luminosities lum_i + dl_ik, and the same one ulp higher: the device's bins are the twin's - a node's
    whole mass sits on one side, so a contracted lum + dl would show as a difference of that mass, far above the bound"""
    from lumfuncmcmc_amd.capi import LFContext
    n = 60
    inp = make_inputs(variant, n, seed=8, S=11)
    th = rows37(inp, 5)[:3]
    sg = np.random.default_rng(5).uniform(0.02, 0.09, n)
    edges, pick, Ln = engineered_edges(inp, sg, count=40)
    ctx = LFContext(inp)
    try:
        check(ctx, inp, th, sg, 32, edges, "%s engineered edges" % variant, wide=False)
        up = edges.copy()
        up[1:-1] = np.nextafter(up[1:-1], np.inf)
        check(ctx, inp, th, sg, 32, up, "%s engineered edges + 1 ulp" % variant, wide=False, set_err=False)
    finally:
        ctx.close()


@pytest.mark.parametrize("variant", VARIANTS)
def test_bits(variant):
    """two calls give the same bits; row r of the 37-row call is the single row of an R = 1 call and its row of a permuted batch"""
    from lumfuncmcmc_amd.capi import LFContext
    n = 1500
    inp = make_inputs(variant, n, seed=2, S=23)
    th = rows37(inp, 3)
    sg = mixed_sigma(n, 4)
    edges = _edges(inp, 50)
    ctx = LFContext(inp)
    try:
        ctx.set_lum_err(sg, 8, wide=True)
        a = ctx.veff_true(th, edges, PREF0, VOL, q=Q)
        b = ctx.veff_true(th, edges, PREF0, VOL, q=Q)
        assert a[2] == b[2] and np.array_equal(a[0], b[0], equal_nan=True) and np.array_equal(a[1], b[1], equal_nan=True)
        perm = np.random.default_rng(1).permutation(37)
        p = ctx.veff_true(th[perm], edges, PREF0, VOL, q=Q)
        assert p[2] == a[2] and np.array_equal(p[1], a[1][perm], equal_nan=True)
        assert np.array_equal(p[0], a[0])                              # (the quantiles sort: the order of the rows does not show)
        for r in (0, 9, 17, 36):
            one = ctx.veff_true(th[r], edges, PREF0, VOL, q=Q)
            assert one[2] == 1 and np.array_equal(one[1][0], a[1][r]) and np.all(one[1] >= 0.0)
            assert np.array_equal(one[0], np.repeat(one[1], len(Q), axis=0))
        assert np.all(np.isnan(ctx.veff_true(th[3], edges, PREF0, VOL, q=Q)[0]))      # (row 3 lies outside the box: R' = 0)
        med = ctx.veff_true(th, edges, PREF0, VOL, method=1)
        assert np.array_equal(med[0], np.median(a[1][~np.isnan(a[1][:, 0])], axis=0)[None])
    finally:
        ctx.close()


def test_the_largest_r_and_an_empty_catalogue(golden_dir):
    """R = 4096, the entry's limit - 256 launch groups, the quantile stage at its slot limit - on a 50-source golden: 110 tilings
    of the 37 rows plus 26, every row with the bits it has in the 37-row call, the quantiles NumPy's; then a catalogue of no
    source: every used row is exactly 0"""
    from lumfuncmcmc_amd import capi
    from lumfuncmcmc_amd.capi import LFContext
    g = np.load(os.path.join(golden_dir, "free_n50.npz"))
    inp = O.inputs_from_golden(g, "free")
    sg = mixed_sigma(len(inp["lum"]), 1)
    th = rows37(inp, 11)
    R = capi.veff_true_info()["max_rows"]
    assert R == 4096
    big = np.tile(th, (R // 37 + 1, 1))[:R]
    edges = _edges(inp, 25)
    ctx = LFContext(inp)
    try:
        ctx.set_lum_err(sg, 32, wide=True)
        _, v37, u37 = ctx.veff_true(th, edges, PREF0, VOL, q=Q)
        out, vals, used = ctx.veff_true(big, edges, PREF0, VOL, q=Q)
        ref = np.tile(v37, (R // 37 + 1, 1))[:R]
        assert np.array_equal(vals, ref, equal_nan=True)
        live = ~np.isnan(vals[:, 0])
        assert used == live.sum() and used > 110 * u37 - 1
        assert np.array_equal(out, np.percentile(vals[live], Q, axis=0))
    finally:
        ctx.close()
    none = make_inputs("fixcomp", 0, seed=8)
    th = rows37(none, 7)[:5]
    ctx = LFContext(none)
    try:
        out, vals, used = check(ctx, none, th, np.zeros(0), 32, np.linspace(40.0, 44.0, 6), "no source")
        assert used == 4 and np.all(vals[~np.isnan(vals[:, 0])] == 0.0) and np.all(out == 0.0)
    finally:
        ctx.close()


def test_refusals():
    """every refusal of the entry: LF_ERR_ARG with a message, and the next good call gives the bits of the one before"""
    from lumfuncmcmc_amd import capi
    from lumfuncmcmc_amd.capi import LFContext, LFError
    inp = make_inputs("free", 300, seed=4, S=23)
    th = np.ascontiguousarray(rows37(inp, 9))
    edges = _edges(inp, 25)
    ctx = LFContext(inp)
    try:
        with pytest.raises(LFError, match="error -1.*lf_veff_true.*lf_set_lum_err"):
            ctx.veff_true(th, edges, PREF0, VOL)
        ctx.set_lum_err(np.full(300, 0.05))
        ok = ctx.veff_true(th, edges, PREF0, VOL)
        info = capi.veff_true_info()
        bad = [
            lambda: ctx.veff_true(np.zeros((0, ctx.ndim)), edges, PREF0, VOL),
            lambda: ctx.veff_true(np.repeat(th[:1], info["max_rows"] + 1, axis=0), edges, PREF0, VOL),
            lambda: ctx.veff_true(th, edges[:1], PREF0, VOL),
            lambda: ctx.veff_true(th, np.linspace(40.0, 44.0, info["max_bins"] + 2), PREF0, VOL),
            lambda: ctx.veff_true(th, edges[::-1], PREF0, VOL),
            lambda: ctx.veff_true(th, np.concatenate([edges[:3], edges[2:]]), PREF0, VOL),
            lambda: ctx.veff_true(th, np.where(np.arange(26) == 4, np.nan, edges), PREF0, VOL),
            lambda: ctx.veff_true(th, np.where(np.arange(26) == 25, np.inf, edges), PREF0, VOL),
            lambda: ctx.veff_true(th, edges, 0.0, VOL),
            lambda: ctx.veff_true(th, edges, PREF0, -1.0),
            lambda: ctx.veff_true(th, edges, PREF0, VOL, q=(50.0, 101.0)),
            lambda: ctx.veff_true(th, edges, PREF0, VOL, q=(np.nan,)),
            lambda: ctx.veff_true(th, edges, PREF0, VOL, q=np.linspace(0, 100, 33)),
            lambda: ctx.veff_true(th, edges, PREF0, VOL, method=7),
        ]
        for f in bad:
            with pytest.raises(LFError, match="error -1.*lf_veff_true"):
                f()
        out, used = np.empty((3, 25)), ctypes.c_int(0)
        q = np.array([16.0, 50.0, 84.0])
        lib, p = ctx._lib, capi._ptr
        good = [p(th), 37, p(edges), 25, PREF0, VOL, 3, p(q), 0, p(out), None, ctypes.byref(used)]
        for at in (0, 2, 7, 9, 11):
            args = list(good)
            args[at] = None
            assert lib.lf_veff_true(ctx._h, *args) == capi.LF_ERR_ARG
            assert b"lf_veff_true" in lib.lf_last_error(ctx._h)
        assert lib.lf_veff_true(ctx._h, *good) == capi.LF_OK and np.array_equal(out, ok[0])       # values may be NULL
        for opt, v in (("skip_grid", 1), ("grid_share", 1 + 65536 * 2)):
            ctx.set_option(opt, v)
            with pytest.raises(LFError, match="error -1.*source-sharded"):
                ctx.veff_true(th, edges, PREF0, VOL)
            ctx.set_option(opt, 0)
        again = ctx.veff_true(th, edges, PREF0, VOL)
        assert again[2] == ok[2] and np.array_equal(again[0], ok[0]) and np.array_equal(again[1], ok[1], equal_nan=True)
        # the stages' times exist only for calls made under set_profiling
        ctx.set_profiling(1)
        timed = ctx.veff_true(th, edges, PREF0, VOL)
        ctx.set_profiling(0)
        assert np.array_equal(timed[1], ok[1], equal_nan=True) and np.all(capi.veff_true_ms() >= 0.0)
    finally:
        ctx.close()


def _surface(o):
    """veff_deconvolved on the device and with device=False over the same draws: the host path is the twin's result, the
    device's lies within the bound of `check` of it"""
    res = {}
    for dev in (True, False):
        np.random.seed(2024)
        res[dev] = o.veff_deconvolved(ndraws=12, device=dev)
    d, t = res[True], res[False]
    assert sorted(d) == sorted(t) == ["Lavg", "n_used", "percentiles", "values", "var_post"] and d["n_used"] == t["n_used"] == 12
    assert np.array_equal(d["Lavg"], t["Lavg"]) and d["values"].shape == t["values"].shape == (12, o.nbins)
    assert np.all((t["values"] == 0.0) == (d["values"] == 0.0)) and t["values"].sum() > 0.0
    assert np.all(np.abs(d["values"] - t["values"]) <= TOL * t["values"])
    # (the dict's arrays are divided by the bin width after the device's quantiles: a rounding each)
    assert np.allclose(d["percentiles"], np.percentile(d["values"], (16, 50, 84), axis=0), rtol=1e-14, atol=0.0)
    assert np.array_equal(d["var_post"], np.var(d["values"], axis=0, ddof=1))
    return d


def test_class_surface():
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
            plain.veff_deconvolved()
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
