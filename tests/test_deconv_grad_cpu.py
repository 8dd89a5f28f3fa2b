"""The gradient of the flux-error-convolved likelihood on the host (lumfuncmcmc_amd/deconv.py: delta_grad, lnprob_err_grad, the
NumPy twin of csrc/lf_deconv_grad.h): the formulas against 30-digit differentiation of the K-point
sum and against central differences of deconv.delta, exact zeros, additivity, the signs around the two maxima of the seeded
Eddington-bias profile, a MAP fit over the twin, the model classes' `likelihood` keyword and the C ABI's bookkeeping.  No GPU.

Formula check.  The twin is the exact derivative of the quadrature sum, so the reference differentiates that sum (mp.diff of
ln sum_k ...), not the integral.  Probe set of tests/test_deconv_cpu.py (sources at 0.5 Flim, at L* and 1 dex above; theta at
the box's centre and at alpha_C = 7 with alpha = -3 and +1), sigma in {0.02, 0.09}, K in {4, 32}.  Measured worst
|twin - mpmath| / S_abs per source and element: 3.6e-16 (centre, sigma = 0.09, K = 32); every case lies between 1.7e-16 and
3.6e-16.  The bound asserted is ten times that, 3.6e-15 - far below 1e-11: the difference form has no cancellation to remove."""
import os
import re

import numpy as np
import pytest

from lf_testlib import make_inputs, synth
from lumfuncmcmc_amd import deconv as D
from lumfuncmcmc_amd import grad as G
from lumfuncmcmc_amd import mapfit
from test_deconv_cpu import FCMIN, PROBE_THETA, _probe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMULA_BOUND = 10 * 3.6e-16              # ten times the measured worst (the docstring above)
ELEMS = (0, 2, 3, 4)                      # the probe's theta: L*, phi*, alpha, Flim, alpha_C - phi* is checked to be exactly 0


def _exact_grad(name, sig, K):
    """d ln sum_k (w_k / sqrt(pi)) exp(t_ik - t_i) / d (L*, alpha, Flim, alpha_C) for the three probe sources, 30 digits"""
    import mpmath as mp
    mp.mp.dps = 30
    inp, th = _probe(name)
    x, lnw = D.gauss_hermite(K)
    a = (2 * mp.mpf(FCMIN) - 1) ** 2
    kappa = mp.sqrt(abs(a / (1 - a)))
    out = []
    for Li, lf in zip(inp["lum"], inp["logf"]):
        Li, lf = mp.mpf(float(Li)), mp.mpf(float(lf))

        def lnsum(Ls, al, Flim, aC):
            def t(L, lfx):
                y = lfx + 17 - mp.log10(Flim)
                num = aC * y
                fc = (1 + num / mp.sqrt(1 + num * num)) / 2
                d = 1 - mp.exp(-mp.mpf(10) ** (y + kappa / aC))
                return mp.log(10) * (al + 1) * (L - Ls) - mp.mpf(10) ** (L - Ls) + mp.log(fc) / d

            t0 = t(Li, lf)
            tot = mp.mpf(0)
            for k in range(K):
                dl = mp.sqrt(2) * mp.mpf(sig) * mp.mpf(float(x[k]))
                tot += mp.exp(mp.mpf(float(lnw[k])) + t(Li + dl, lf + dl) - t0)
            return mp.log(tot)

        at = tuple(mp.mpf(float(th[e])) for e in ELEMS)
        out.append([float(mp.diff(lnsum, at, tuple(int(i == j) for i in range(4)))) for j in range(4)])
    return np.array(out)


@pytest.mark.parametrize("K", [4, 32])
@pytest.mark.parametrize("sig", [0.02, 0.09])
def test_formulas_against_30_digit_differentiation_of_the_sum(sig, K):
    worst = 0.0
    for name in PROBE_THETA:
        inp, th = _probe(name)
        Di, g, s = D.delta_grad(inp, np.full(3, sig), th, K=K, per_source=True)
        assert np.array_equal(Di, D.delta(inp, np.full(3, sig), th, K=K, terms=True)[1])
        assert np.all(g[:, 1] == 0.0) and np.all(s[:, 1] == 0.0)                # phi*
        ratio = np.abs(g[:, ELEMS] - _exact_grad(name, sig, K)) / s[:, ELEMS]
        print("formula %-9s sigma = %.2f K = %2d: worst |twin - mpmath| / S_abs = %.2e" % (name, sig, K, ratio.max()))
        worst = max(worst, float(ratio.max()))
    assert FORMULA_BOUND <= 1e-11
    assert worst <= FORMULA_BOUND


def _case(variant, n=257, seed=5):
    inp = make_inputs(variant, n, seed=seed, S=23)
    n = len(inp["lum"])
    sg = np.random.default_rng(1).uniform(0.0, 0.09, n)
    sg[::10] = 0.0
    th = synth.walkers(variant, 3, seed=3, fix_sch_al=False, nf=len(inp["field_ind"]) - 1)
    return inp, sg, th


@pytest.mark.parametrize("variant", ["free", "fixcomp", "zevol"])
def test_central_differences_of_delta(variant):
    inp, sg, th = _case(variant)
    tot, g = D.delta_grad(inp, sg, th)
    assert np.array_equal(tot, D.delta(inp, sg, th))
    h = 1e-5
    worst = 0.0
    for e in range(th.shape[1]):
        up, dn = th.copy(), th.copy()
        up[:, e] += h
        dn[:, e] -= h
        fd = (D.delta(inp, sg, up) - D.delta(inp, sg, dn)) / (2 * h)
        worst = max(worst, float(np.max(np.abs(g[:, e] - fd) / (np.abs(fd) + 1e-6))))
        assert np.all(np.abs(g[:, e] - fd) <= 1e-7 * (np.abs(fd) + 1e-6)), (variant, e)
    print("central differences %s: worst |g - fd| / (|fd| + 1e-6) = %.2e" % (variant, worst))


@pytest.mark.parametrize("variant", ["free", "fixcomp", "zevol"])
def test_exact_zeros_and_additivity_over_fields(variant):
    inp, sg, th = _case(variant)
    n = len(sg)
    # all sigma 0: no correction, and the gradient is the plain one's, bit for bit
    tot, g, s = D.delta_grad(inp, np.zeros(n), th, terms=True)
    assert np.all(tot == 0.0) and np.all(g == 0.0) and np.all(s == 0.0) and not np.signbit(g).any()
    val, ge = D.lnprob_err_grad(inp, np.zeros(n), th)
    lp, gp = G.lnprob_grad(inp, th)
    assert np.array_equal(val, lp) and np.array_equal(ge, gp, equal_nan=True) and np.isfinite(lp).any()
    # the phi elements, and the sources with sigma = 0
    tot, g, s = D.delta_grad(inp, sg, th, terms=True)
    phi = slice(3, 6) if variant == "zevol" else slice(1, 2)
    assert np.all(g[:, phi] == 0.0) and np.all(s[:, phi] == 0.0)
    gi = D.delta_grad(inp, sg, th, per_source=True)[1]
    assert np.all(gi[:, ::10] == 0.0) and np.all(np.isfinite(g)) and np.any(g != 0.0)
    # additive over fields
    fi = inp["field_ind"]
    per_field = np.zeros_like(g)
    for f in range(len(fi) - 1):
        only = np.zeros(n)
        only[fi[f]:fi[f + 1]] = sg[fi[f]:fi[f + 1]]
        per_field += D.delta_grad(inp, only, th)[1]
    assert np.all(np.abs(per_field - g) <= 1e-13 * s)
    # the value is lnprob_err's; a row outside the box has NaN in every element, S_abs is the sum of both parts
    th[1, 0] = 39.0
    val, ge, se = D.lnprob_err_grad(inp, sg, th, terms=True)
    assert np.array_equal(val, D.lnprob_err(inp, sg, th)) and val[1] == -np.inf
    assert np.isnan(ge[1]).all() and not np.isnan(ge[[0, 2]]).any()
    lp, gp, sp = G.lnprob_grad(inp, th, terms=True)
    assert np.array_equal(ge[[0, 2]], gp[[0, 2]] + g[[0, 2]]) and np.array_equal(se[[0, 2]], sp[[0, 2]] + s[[0, 2]])
    one = D.lnprob_err_grad(inp, sg, th[0])
    assert one[0] == val[0] and np.array_equal(one[1], ge[0])


def test_eddington_signs_and_map_over_the_twin():
    """the seeded profile of tests/test_deconv_cpu.py: its convolved maximum lies on the truth (offset 0.00), the plain one at
    +0.04 dex - so the convolved d / d L* changes sign between -0.02 and +0.02 while the plain one is still positive at +0.02;
    then both maxima by mapfit.maximise over the twins from 4 starts: the convolved L* lies below the plain one"""
    import lf_deconvlib as L
    inp, sigma, theta, rows = L.eddington_case()
    i0 = L.EDD_GRID.size // 2
    at = rows[[i0 - 1, i0 + 1]]
    gc = D.lnprob_err_grad(inp, sigma, at)[1][:, 0]
    gp = G.lnprob_grad(inp, at)[1][:, 0]
    print("Eddington d lnprob / d L* at -0.02, +0.02 dex: convolved %+.2f %+.2f, plain %+.2f %+.2f" % (gc[0], gc[1], gp[0], gp[1]))
    assert gc[0] > 0.0 > gc[1]
    assert gp[1] > 0.0
    lims = inp["lims"]
    box = np.array([lims["Lstar"], lims["phistar"], lims["sch_al"]], dtype=np.float64)
    conv = lambda t: D.lnprob_err_grad(inp, sigma, t)       # noqa: E731
    plain = lambda t: G.lnprob_grad(inp, t)                 # noqa: E731
    rng = np.random.default_rng(12)
    starts = rng.uniform(box[:, 0], box[:, 1], (4, 3))
    for _ in range(100):
        bad = ~(np.isfinite(conv(starts)[0]) & np.isfinite(plain(starts)[0]))
        if not bad.any():
            break
        starts[bad] = rng.uniform(box[:, 0], box[:, 1], (int(bad.sum()), 3))
    rc = mapfit.maximise(conv, box, starts, tol=1e-6)
    rp = mapfit.maximise(plain, box, starts, tol=1e-6)
    print("twin MAP: convolved %s (%d iterations), plain %s (%d), truth %s"
          % (np.round(rc["theta"], 4), rc["niter"], np.round(rp["theta"], 4), rp["niter"], np.round(theta, 4)))
    assert rc["converged"] and rp["converged"]
    assert rc["theta"][0] < rp["theta"][0]


def test_class_surface():
    import lf_deconvlib as L
    cat = synth.catalogue(300, seed=17)
    cat["lum_e"] = np.full(300, 0.05)
    o = L.fixcomp_model(cat, deconvolve=True)
    p = L.fixcomp_model(cat)
    try:
        for obj in (o, p):
            with pytest.raises(ValueError, match="likelihood"):
                obj.fit_model_map(likelihood="bogus")
            obj.map_theta, obj.map_cov = np.zeros(3), np.eye(3)
            with pytest.raises(ValueError, match="likelihood"):
                obj.map_init_walkers(likelihood="bogus")
        with pytest.raises(ValueError, match="deconvolve=True"):
            p.fit_model_map(likelihood="convolved")
        with pytest.raises(ValueError, match="deconvolve=True"):
            p.map_init_walkers(likelihood="convolved")
        # the argument-less refusal is unchanged, and now names the keyword
        with pytest.raises(NotImplementedError, match="deconvolve") as ei:
            o.fit_model_map()
        assert "likelihood=" in str(ei.value)
        with pytest.raises(NotImplementedError, match="deconvolve"):
            o.map_init_walkers()
        for call in (o.fit_model_converged, o.fit_model_pt):
            with pytest.raises(NotImplementedError, match="deconvolve"):
                call()
    finally:
        o.close()
        p.close()


def test_c_abi_entries():
    from lumfuncmcmc_amd import build, capi
    hdr = open(os.path.join(ROOT, "include", "lfmcmc.h")).read()
    assert re.search(r"int lf_lnprob_err_grad_batch\(lf_ctx \*ctx, const double \*theta, int B, double \*lnprob_err, double \*grad\);", hdr)
    assert re.search(r"int lf_lnprob_err_grad_batch_device\(lf_ctx \*ctx, const double \*d_theta, int B, double \*d_lnprob_err, "
                     r"double \*d_grad, void \*hip_stream\);", hdr)
    assert "#define LF_ABI_VERSION 3" in hdr
    lib = capi.load()
    for n in ("lf_lnprob_err_grad_batch", "lf_lnprob_err_grad_batch_device"):
        assert n in capi.EXPORTS and hasattr(lib, n)
    assert lib.lf_abi_version() == 3
    # refused before any device is touched
    assert lib.lf_lnprob_err_grad_batch(None, None, 1, None, None) == capi.LF_ERR_ARG
    assert lib.lf_lnprob_err_grad_batch_device(None, None, 1, None, None, None) == capi.LF_ERR_ARG
    assert "lf_deconv_grad.h" in " ".join(build.HEADERS)
    for name in ("lnprob_err_grad", "lnprob_err_grad_torch"):
        assert callable(getattr(capi.LFContext, name))
