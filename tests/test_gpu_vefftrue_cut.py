"""The deconvolved 1/Veff points under the cut on the observed flux on the device (csrc/lf_vefftrue_cut.h; option
"deconv_cut_veff", lf_veff_true_cut, lf_cut_volume) against their NumPy twins (deconv.py:
cut_volume_fraction, veff_true(cut=...), checked in tests/test_vefftrue_cut_cpu.py):

    lf_cut_volume:  the zero and one patterns and a field without errors exactly; elsewhere |dev - twin| <= 5e-13 twin - half
                    the bins' standing 1e-12: all terms are positive, so a bin's relative error is at most the worst element's;
    lf_veff_true:   n_used equal, per bin |dev - twin| <= 1e-12 twin (section 3.26's bound), a bin that is 0 in the twin exactly 0;

then the bits (a row alone, in a batch, permuted; two calls; the table made again after a second lf_set_lum_err), min_vol_frac's
dropped count, the paths that must keep their bits or their refusal, and the model classes."""
import numpy as np
import pytest

import lf_cutlib as C
import lf_deconvlib as L
from lf_testlib import make_inputs, synth
from lumfuncmcmc_amd import deconv as D
from test_gpu_deconv_wide import mixed_sigma, rows37
from test_vefftrue_cut_cpu import element_points

pytestmark = pytest.mark.gpu
TOL, TOL_G = 1e-12, 5e-13
PREF0, VOL = 3.1e-5, 2.7e6
VARIANTS = ["free", "fixcomp", "zevol"]
Q = (0.0, 16.0, 50.0, 84.0, 100.0)


def cut_model(M, nf):
    """M = 1: one node; 16: a model with kinks in both directions; 64: proportional to 1 / flux"""
    if M == 1:
        return C.const_model(0.2, nf=nf)
    if M == 16:
        nodes = np.log10(C.FCUT) + np.linspace(-0.6, 1.0, 16)
        return nodes, np.repeat((0.1 + 0.05 * np.sin(np.arange(16.0)))[None], nf, axis=0)
    return C.flux_model(0.09, nf=nf, M=M)


def context(inp, model, sg=None, K=32, wide=True, veff=True):
    from lumfuncmcmc_amd.capi import LFContext
    ctx = LFContext(inp)
    ctx.set_cut_error_model(*model)
    ctx.set_option("deconv_cut_veff", 1 if veff else 0)
    if sg is not None:
        ctx.set_lum_err(sg, K, wide=wide)
    return ctx


@pytest.mark.parametrize("nf", [1, 5])
@pytest.mark.parametrize("M", [1, 16, 64])
@pytest.mark.parametrize("S", [5, 101])
def test_cut_volume_against_twin(S, M, nf):
    inp = C.cut_inputs("free", n=60, S=S, nf=nf)
    nodes, sig = cut_model(M, nf)
    if nf > 1:
        sig = np.minimum(sig * np.array([1.0, 0.5, 0.0, 0.8, 1.4])[:, None], D.CUT_SIGMA_MAX)     # field 2 has no errors: the step
    ctx = context(inp, (nodes, sig))
    try:
        worst = 0.0
        for f in range(nf):
            pts = element_points(inp, nodes, sig[f] if sig[f].max() > 0 else sig[0])
            tw = D.cut_volume_fraction(inp, nodes, sig, f, pts)
            dev = ctx.cut_volume(f, pts)
            assert np.array_equal(dev == 0.0, tw == 0.0) and np.array_equal(dev == 1.0, tw == 1.0), (S, M, f)
            if sig[f].max() == 0.0:
                assert np.array_equal(dev, tw), (S, M, f)
            pos = tw > 0.0
            worst = max(worst, float(np.max(np.abs(dev[pos] - tw[pos]) / tw[pos])))
        print("cut volume S=%3d M=%2d nf=%d: max |dev - twin| / twin = %.3e (%.3f of the bound)" % (S, M, nf, worst, worst / TOL_G))
        assert worst <= TOL_G
    finally:
        ctx.close()


def _edges(inp, nbin):
    lum = np.asarray(inp["lum"])
    return np.linspace(lum.min() - 0.3, lum.max() + 0.2, nbin + 1)


def check(ctx, inp, model, th, sg, K, edges, label, wide=True, mvf=0.0):
    out, vals, used = ctx.veff_true(th, edges, PREF0, VOL, q=Q, min_vol_frac=mvf)
    tw, tu = D.veff_true(inp, sg, th, edges, PREF0, VOL, K=K, wide=wide, cut=model, min_vol_frac=mvf)
    assert used == tu and vals.shape == tw.shape, (label, used, tu)
    off = np.isnan(tw)
    assert np.array_equal(np.isnan(vals), off), label
    zero = tw == 0.0
    assert np.all(vals[zero] == 0.0), label
    pos = ~off & ~zero
    if inp["variant"] == "zevol":
        # section 3.26's stated limit of the bound: bins fed from sources up to about 1.5 dex above L*
        th2 = np.atleast_2d(th)
        pos &= edges[None, 1:] <= th2[:, 0:3].min(axis=1)[:, None] + 1.5
    w = float(np.max(np.abs(vals[pos] - tw[pos]) / tw[pos])) if pos.any() else 0.0
    info = ctx.veff_true_cut_info()
    print("veff true cut %-30s K=%2d rows %2d used %2d bins %4d dropped %d of %d: max |dev - twin| / bound = %.3e"
          % (label, K, len(np.atleast_2d(th)), used, len(edges) - 1, info["dropped"], info["slots"], w / TOL))
    assert w <= TOL, (label, w)
    rows = vals[~off.any(axis=1)]
    if used:
        assert np.array_equal(out, np.percentile(rows, Q, axis=0)), label
    return vals, info


@pytest.mark.parametrize("variant", VARIANTS)
def test_points_against_twin(variant):
    """the grids of tests/test_gpu_deconv_cut.py (min_comp_frac = 0.5's shape: an edge per column), five fields, sigma up to the
    wide rule's top with a tenth at 0, K = 4 and 32, 37 rows (three launch groups), 1 / 25 / 1024 bins"""
    inp = C.cut_inputs(variant, n=400, S=23, nf=5)
    model = C.flux_model(0.09, nf=5)
    sg = mixed_sigma(400, 1)
    th = rows37(inp, 11)
    ctx = context(inp, model)
    try:
        for K in (4, 32):
            ctx.set_lum_err(sg, K, wide=True)
            want = D.cut_volume_table(inp, sg, model, K=K, wide=True)[1]
            for nbin in (1, 25, 1024):
                _, info = check(ctx, inp, model, th, sg, K, _edges(inp, nbin), "%s n=400" % variant)
                assert info["dropped"] == want and info["bytes"] == 8 * info["slots"]
    finally:
        ctx.close()


@pytest.mark.parametrize("variant", VARIANTS)
def test_chunk_edges(variant):
    """fields of 1023, 1024 and 1025 sources (the narrow chunks) of which 255, 256 and 257 stand in one wide class each (the
    wide chunks); rows 1, 16, 17"""
    sizes = (1023, 1024, 1025)
    n = int(sum(sizes))
    inp = C.cut_inputs(variant, n=n, S=5, nf=3)
    fi = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    inp["field_ind"] = fi
    rng = np.random.default_rng(12)
    sg = rng.uniform(0.005, 0.09, n)
    sg[::10] = 0.0
    for f, (nw, s) in enumerate(zip((255, 256, 257), (0.095, 0.14, 0.19))):
        sg[fi[f] + rng.permutation(sizes[f])[:nw]] = s
    cls = D.wide_class(sg, 32)
    assert [(cls == c).sum() for c in range(3)] == [255, 256, 257]
    model = C.flux_model(0.09, nf=3)
    th = rows37(inp, 7)
    ctx = context(inp, model, sg, 32)
    try:
        for R in (1, 16, 17):
            check(ctx, inp, model, th[4:4 + R], sg, 32, _edges(inp, 25), "%s chunk edges R=%d" % (variant, R))
    finally:
        ctx.close()


@pytest.mark.parametrize("variant", VARIANTS)
def test_one_source(variant):
    one = D._subset(C.cut_inputs(variant, n=40, S=5, nf=1), np.array([7]))       # (the grid of the 40-source catalogue)
    assert len(one["lum"]) == 1
    model = C.const_model(0.1)
    th = rows37(one, 5)[:5]
    ctx = context(one, model)
    try:
        for s in (0.0, 0.07, 0.2):
            ctx.set_lum_err(np.array([s]), 32, wide=True)
            check(ctx, one, model, th, np.array([s]), 32, _edges(one, 25), "%s one source sigma=%.2f" % (variant, s))
    finally:
        ctx.close()


@pytest.mark.parametrize("variant", VARIANTS)
def test_bits_and_rebuilt_table(variant):
    inp = C.cut_inputs(variant, n=600, S=23, nf=5)
    model = C.flux_model(0.09, nf=5)
    sg = mixed_sigma(600, 4)
    th = rows37(inp, 3)
    edges = _edges(inp, 50)
    ctx = context(inp, model, sg, 8)
    try:
        a = ctx.veff_true(th, edges, PREF0, VOL, q=Q)
        b = ctx.veff_true(th, edges, PREF0, VOL, q=Q)
        assert a[2] == b[2] and np.array_equal(a[0], b[0], equal_nan=True) and np.array_equal(a[1], b[1], equal_nan=True)
        perm = np.random.default_rng(1).permutation(37)
        p = ctx.veff_true(th[perm], edges, PREF0, VOL, q=Q)
        assert p[2] == a[2] and np.array_equal(p[1], a[1][perm], equal_nan=True) and np.array_equal(p[0], a[0])
        for r in (0, 9, 17, 36):
            one = ctx.veff_true(th[r], edges, PREF0, VOL, q=Q)
            assert one[2] == 1 and np.array_equal(one[1][0], a[1][r])
        # other errors: the table is made again, and made again for the first ones it gives the first bits
        info_a = ctx.veff_true_cut_info()
        sg2 = mixed_sigma(600, 9)
        ctx.set_lum_err(sg2, 8, wide=True)
        check(ctx, inp, model, th[:5], sg2, 8, edges, "%s second lum err" % variant)
        assert ctx.veff_true_cut_info()["dropped"] == D.cut_volume_table(inp, sg2, model, K=8, wide=True)[1]
        ctx.set_lum_err(sg, 8, wide=True)
        c = ctx.veff_true(th, edges, PREF0, VOL, q=Q)
        assert np.array_equal(c[1], a[1], equal_nan=True) and ctx.veff_true_cut_info()["dropped"] == info_a["dropped"]
    finally:
        ctx.close()


def test_min_vol_frac_and_the_dropped_count():
    inp = C.cut_inputs("fixcomp", n=300, S=23, nf=2)
    model = C.flux_model(0.09, nf=2)
    sg = mixed_sigma(300, 2)
    th = rows37(inp, 5)[:5]
    ctx = context(inp, model, sg, 8)
    try:
        counts = []
        for mvf in (0.0, 0.25, 0.0):
            _, info = check(ctx, inp, model, th, sg, 8, _edges(inp, 25), "min_vol_frac %.2f" % mvf, mvf=mvf)
            assert info["dropped"] == D.cut_volume_table(inp, sg, model, K=8, wide=True, min_vol_frac=mvf)[1]
            counts.append(info["dropped"])
        assert counts[0] == counts[2] < counts[1]
        from lumfuncmcmc_amd.capi import LFError
        with pytest.raises(LFError, match="error -1.*lf_veff_true_cut.*min_vol_frac"):
            ctx.veff_true(th, _edges(inp, 25), PREF0, VOL, min_vol_frac=1.5)
    finally:
        ctx.close()


def test_existing_paths_keep_their_bits_and_their_refusal():
    from lumfuncmcmc_amd.capi import LFContext, LFError
    inp = make_inputs("fixcomp", 500, seed=2, S=23)
    sg = mixed_sigma(500, 4)
    th = rows37(inp, 3)
    edges = _edges(inp, 25)
    res = []
    for opt in (0, 1):
        ctx = LFContext(inp)
        try:
            ctx.set_option("deconv_cut_veff", opt)
            ctx.set_lum_err(sg, 8, wide=True)
            res.append(ctx.veff_true(th, edges, PREF0, VOL, q=Q))
            if opt:
                with pytest.raises(LFError, match="no table"):
                    ctx.veff_true_cut_info()
                with pytest.raises(LFError, match="min_vol_frac > 0 needs a cut model"):
                    ctx.veff_true(th, edges, PREF0, VOL, min_vol_frac=0.1)
                with pytest.raises(LFError, match="no cut model"):
                    ctx.cut_volume(0, np.array([42.0]))
        finally:
            ctx.close()
    assert res[0][2] == res[1][2] and np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1], equal_nan=True)
    cinp = C.cut_inputs("fixcomp", n=100, S=5, nf=2)
    ctx = context(cinp, C.flux_model(0.09, nf=2), np.full(100, 0.03), 8, veff=False)
    try:
        with pytest.raises(LFError, match="lf_veff_true: not under a cut on the observed flux \\(lf_set_cut_error_model\\): per-source "
                                          "volumes \\(a z_max per source under the cut\\) are not provided: the points take one volume"):
            ctx.veff_true(rows37(cinp, 7)[:3], np.linspace(41.0, 44.0, 7), 1.0, 1.0)
        with pytest.raises(LFError, match="field outside"):
            ctx.cut_volume(2, np.array([42.0]))
    finally:
        ctx.close()


def _surface(o):
    res = {}
    for dev in (True, False):
        np.random.seed(2024)
        res[dev] = o.veff_deconvolved(ndraws=8, device=dev)
    d, t = res[True], res[False]
    assert sorted(d) == sorted(t) == ["Lavg", "n_dropped", "n_used", "percentiles", "values", "var_post"]
    assert d["n_used"] == t["n_used"] == 8 and d["n_dropped"] == t["n_dropped"]
    assert np.all((t["values"] == 0.0) == (d["values"] == 0.0)) and t["values"].sum() > 0.0
    assert np.all(np.abs(d["values"] - t["values"]) <= TOL * t["values"])
    # the cut's volume shows: the points are not those of one scalar volume
    np.random.seed(2024)
    some = o.veff_deconvolved(ndraws=8, device=True, min_vol_frac=0.3)
    assert some["n_dropped"] >= d["n_dropped"] and np.all(some["values"] <= d["values"])


def test_class_surface():
    cat = synth.catalogue(400, seed=17)
    kw = dict(deconvolve=True, min_comp_frac=0.5, deconvolve_cut=True, deconvolve_order=12)
    np.random.seed(5)
    o = L.fixcomp_model(cat, deconvolve_cut_veff=True, **kw)
    try:
        o.fit_model()
        _surface(o)
    finally:
        o.close()
    o = L.fixcomp_model(cat, **kw)
    try:
        with pytest.raises(NotImplementedError, match="own volume"):
            o.veff_deconvolved()
    finally:
        o.close()
    with pytest.raises(ValueError, match="deconvolve_cut_veff=True needs deconvolve_cut=True"):
        L.fixcomp_model(cat, deconvolve=True, deconvolve_cut_veff=True)


def test_class_surface_z():
    from lumfuncmcmc_amd.model import LumFuncMCMCz
    cat = synth.catalogue(400, seed=5)
    fi = cat["field_ind"]
    kw = dict(lum=synth.split_fields(cat["lum"], fi), lum_e=synth.split_fields(np.full(400, 0.06), fi), Flim=list(synth.FLIM),
              alpha=synth.ALPHA_C, Omega_0=list(synth.OMEGA_0), sch_al=synth.SCH_AL, nwalkers=32, nsteps=20, min_comp_frac=0.5,
              field_ind=fi)
    np.random.seed(1)
    oz = LumFuncMCMCz(synth.split_fields(cat["z"], fi), deconvolve=True, deconvolve_cut=True, deconvolve_cut_veff=True, **kw)
    try:
        oz.fit_model()
        _surface(oz)
    finally:
        oz.close()
