"""The per-source posterior of the true luminosity on the host (lumfuncmcmc_amd/deconv.py: lum_posterior, the NumPy twin of
csrc/lf_lumpost.h): the moments against 30-digit integration over the posterior weight, their
calibration on a seeded mock with known true luminosities, and the conventions (sigma = 0, caller order, skipped rows, no used
row, one row).  No GPU.

Probe set and reference: those of tests/test_deconv_wide_cpu.py (its _mp_term and breakpoints; sources at 0.25, 0.5, 5 and 50
Flim), in all three variants - the fixed-completeness ones take the probe's Flim and alpha_C as the fixed curve, the z-evolving
one the probe's L* at all three pivots.  Measured worst over the probe set, sources and variants (the figures of DESIGN.md
section 3.22; mpmath is deterministic, the margin of four covers libm differences between hosts):
    sigma 0.09, K = 32: |m1 - ref| / sigma 4.67e-08, |m2 - ref| / sigma^2 1.12e-07;   sigma 0.03, K = 6: 1.00e-06, 2.33e-05;
    class edges 0.10 .. 0.30: |m1 - ref| / sigma 3.40e-08, 9.88e-08, 6.74e-08, 3.57e-08, 2.73e-08;
                              |m2 - ref| / sigma^2 3.24e-07, 3.93e-07, 4.45e-07, 8.81e-08, 1.27e-07 (all below 1e-5)."""
import functools

import numpy as np
import pytest

import lf_deconvlib as L
from lf_testlib import make_inputs, synth
from lumfuncmcmc_amd import deconv as D
from lumfuncmcmc_amd import grad as G
from test_deconv_cpu import PROBE_THETA
from test_deconv_wide_cpu import _mp_term, _probe

VARIANTS = ["free", "fixcomp", "zevol"]
# (sigma, K, wide): the default order at its limit, a low order at its limit, every wide class at its upper edge
CASES = [(0.09, 32, False), (0.03, 6, False)] + [(s, 32, True) for s in D.WIDE_EDGES]
# four times the measured worst (module docstring), rounded up to one digit: |m1 - ref| / sigma, |m2 - ref| / sigma^2
BOUNDS = {(0.09, 32): (2e-7, 5e-7), (0.03, 6): (5e-6, 1e-4), (0.10, 32): (2e-7, 2e-6), (0.15, 32): (4e-7, 2e-6),
          (0.20, 32): (3e-7, 2e-6), (0.25, 32): (2e-7, 4e-7), (0.30, 32): (2e-7, 6e-7)}


def _probe_variant(name, variant):
    """the probe's four sources and row as kernel inputs of `variant`: the same term in all three"""
    inp, th = _probe(name)
    Ls, al, Flim, aC = PROBE_THETA[name]
    if variant == "free":
        return inp, th
    inp = dict(inp, variant=variant, Flim0=np.array([Flim]), alpha0=aC)
    if variant == "fixcomp":
        return inp, np.array([Ls, -3.0, al])
    inp.update(z=np.array([1.25, 1.4, 1.53, 1.8]), pivots=(1.20, 1.53, 1.86))
    return inp, np.array([Ls, Ls, Ls, -3.0, -3.0, -3.0, al])


@functools.lru_cache(maxsize=None)
def _exact(name, sig):
    """(E[delta], E[delta^2]) under the posterior weight N(delta; 0, sigma^2) exp(t(L + delta, f 10^delta) - t(L, f)) of the four
    probe sources, by 30-digit quadrature"""
    import mpmath as mp
    mp.mp.dps = 30
    inp, _ = _probe(name)
    t = _mp_term(mp, *(mp.mpf(v) for v in PROBE_THETA[name]))
    sig = mp.mpf(sig)
    brk = [k * sig for k in (-12, -9, -6, -4, -3, -2, -1, 0, 1, 2, 3, 4, 6, 9, 12)]
    out = []
    for Li, lf in zip(inp["lum"], inp["logf"]):
        Li, lf = mp.mpf(float(Li)), mp.mpf(float(lf))
        t0 = t(Li, lf)
        w = lambda u: mp.exp(-u * u / (2 * sig * sig)) / (sig * mp.sqrt(2 * mp.pi)) * mp.exp(t(Li + u, lf + u) - t0)   # noqa: E731
        n0 = mp.quad(w, brk)
        out.append((float(mp.quad(lambda u: u * w(u), brk) / n0), float(mp.quad(lambda u: u * u * w(u), brk) / n0)))
    return np.array(out).T


def _twin_moments(inp, sig, th, K, wide):
    """the twin's per-row moments of the four probe sources (the rule per source: _rules, as lum_posterior takes it)"""
    sg = np.full(4, sig)
    out = np.zeros((3, 4))
    with np.errstate(all="ignore"):
        for sub, idx, x, lnw in D._rules(inp, sg, K, wide):
            idx = slice(None) if idx is None else idx
            out[:, idx] = D._row_terms(sub, sg[idx], th, x, lnw, moments=True)
    return out


@pytest.mark.parametrize("sig,K,wide", CASES)
def test_twin_against_30_digit_integration(sig, K, wide):
    w1 = w2 = 0.0
    for name in PROBE_THETA:
        ref = _exact(name, float(sig))
        for variant in VARIANTS:
            inp, th = _probe_variant(name, variant)
            e1, e2, ea = _twin_moments(inp, sig, th, K, wide)
            assert np.all(ea >= np.abs(e1)) and np.all(e2 > 0.0)
            w1 = max(w1, float(np.max(np.abs(e1 - ref[0]))) / sig)
            w2 = max(w2, float(np.max(np.abs(e2 - ref[1]))) / sig ** 2)
    print("lum posterior sigma = %.2f K = %d wide = %d: worst |m1 - ref| / sigma = %.2e, |m2 - ref| / sigma^2 = %.2e" % (sig, K, wide, w1, w2))
    if wide:
        assert w1 <= 1e-5 and w2 <= 1e-5           # (the issue's stop line for a class edge)
    b1, b2 = BOUNDS[(sig, K)]
    assert w1 <= b1 and w2 <= b2, (w1, w2)


CAL_SEED, CAL_NOISE_SEED, CAL_N, CAL_ERR = 5, 23, 3000, 0.08


@functools.lru_cache(maxsize=None)
def _calibration_case():
    """(kernel inputs of a free-completeness model over a seeded mock with Gaussian noise of 0.08 dex added here, sigma, theta of
    the truth, the noiseless luminosities)"""
    base = L.fixcomp_model(synth.catalogue(2000, seed=17), fix_comp=False)
    theta = np.array([synth.LSTAR, synth.PHISTAR, synth.SCH_AL] + list(synth.FLIM) + [synth.ALPHA_C])
    m0 = base._mock_generator(False).counts(theta[None], 0)[0].sum()
    theta[1] += np.log10(CAL_N / m0)
    mc = base.mock_catalogue(theta, seed=CAL_SEED, device=False)
    base.close()
    true = np.concatenate(mc["lum"])
    noise = np.random.default_rng(CAL_NOISE_SEED).normal(0.0, CAL_ERR, true.size)
    fi = np.asarray(mc["field_ind"])
    mc["lum"] = synth.split_fields(true + noise, fi)
    mc["lum_e"] = synth.split_fields(np.full(true.size, CAL_ERR), fi)
    o = L.fixcomp_model(mc, fix_comp=False)
    inp = o.kernel_inputs()
    o.close()
    return inp, np.full(true.size, CAL_ERR), theta, true


def test_calibration_on_a_seeded_mock():
    """true - lum - m1 has mean 0 and variance m2 - m1^2 in each of five quantile bins of the catalogued luminosity, within 4
    standard errors (the posterior is exact for this noise model; seeds checked once: the worst bin lies at 1.9 and 0.9
    standard errors)"""
    inp, sigma, theta, true = _calibration_case()
    assert 2500 <= true.size <= 3500
    m1, m2, used = D.lum_posterior(inp, sigma, theta)
    assert used == 1
    lum = np.asarray(inp["lum"])
    resid, var = true - lum - m1, m2 - m1 * m1
    assert np.all(var > 0.0)
    edges = np.quantile(lum, np.linspace(0.0, 1.0, 6))
    which = np.clip(np.searchsorted(edges, lum, side="right") - 1, 0, 4)
    for b in range(5):
        r, v = resid[which == b], var[which == b]
        n = r.size
        z1 = np.mean(r) / (np.std(r, ddof=1) / np.sqrt(n))
        q = r * r / v
        z2 = (np.mean(q) - 1.0) / (np.std(q, ddof=1) / np.sqrt(n))
        print("calibration bin %d: n = %d, mean shift %+.4f dex, mean residual %+.2f se, mean z^2 - 1 %+.2f se" % (b, n, np.mean(m1[which == b]), z1, z2))
        assert abs(z1) <= 4.0 and abs(z2) <= 4.0, (b, z1, z2)
    # the brightest fifth is corrected downwards (the steep end of the LF), the faintest upwards (the completeness acts on the true flux)
    assert np.mean(m1[which == 4]) < 0.0 < np.mean(m1[which == 0])


@pytest.mark.parametrize("variant", VARIANTS)
def test_conventions(variant):
    n = 120
    inp = make_inputs(variant, n, seed=8, S=11)
    th = synth.walkers(variant, 6, seed=3, fix_sch_al=False, nf=5)
    lp = G.lnprob_grad(inp, th)[0]
    assert np.isfinite(lp).all()
    sg = np.random.default_rng(2).uniform(0.01, 0.09, n)
    sg[::5] = 0.0
    m1, m2, used, s1 = D.lum_posterior(inp, sg, th, terms=True)
    assert used == 6 and np.all(m1[sg == 0.0] == 0.0) and np.all(m2[sg == 0.0] == 0.0) and np.all(s1[sg == 0.0] == 0.0)
    assert np.all(m2[sg > 0.0] > 0.0) and np.all(s1 >= np.abs(m1)) and np.all(m2 >= m1 * m1)
    # one source with sigma > 0 at caller index j: only index j is not 0
    j = 77
    one = np.zeros(n)
    one[j] = 0.07
    a1, a2, _ = D.lum_posterior(inp, one, th)
    assert a1[j] != 0.0 and a2[j] > 0.0 and np.count_nonzero(a1) == 1 and np.count_nonzero(a2) == 1
    # a row outside the box is skipped: the result is that of the other rows
    out = th.copy()
    out[2, 0] = 39.5
    b1, b2, ub = D.lum_posterior(inp, sg, out)
    c1, c2, uc = D.lum_posterior(inp, sg, np.delete(th, 2, axis=0))
    assert ub == uc == 5 and np.array_equal(b1, c1) and np.array_equal(b2, c2)
    # no row is used: NaN where sigma > 0, exactly 0 elsewhere
    out[:, 0] = 39.5
    d1, d2, ud = D.lum_posterior(inp, sg, out)
    assert ud == 0 and np.all(np.isnan(d1[sg > 0.0])) and np.all(np.isnan(d2[sg > 0.0]))
    assert np.all(d1[sg == 0.0] == 0.0) and np.all(d2[sg == 0.0] == 0.0)
    # one row: the per-row terms themselves
    x, lnw = D.gauss_hermite(D.DEFAULT_ORDER)
    with np.errstate(all="ignore"):
        e1, e2, ea = D._row_terms(inp, sg, th[4], x, lnw, moments=True)
    r1, r2, ur, ra = D.lum_posterior(inp, sg, th[4], terms=True)
    assert ur == 1 and np.array_equal(r1, e1) and np.array_equal(r2, e2) and np.array_equal(ra, ea)
    # the wide rule: a source above the order's limit is taken by its class's table, the others keep their bits
    sw = sg.copy()
    sw[3] = 0.2
    w1, w2, _ = D.lum_posterior(inp, sw, th, wide=True)
    keep = np.arange(n) != 3
    assert np.array_equal(w1[keep], m1[keep]) and np.array_equal(w2[keep], m2[keep]) and w2[3] > m2.max()
    with pytest.raises(ValueError, match="above 0.30 dex"):
        D.lum_posterior(inp, np.full(n, 0.31), th, wide=True)


def test_model_surface_refuses_without_deconvolve():
    cat = synth.catalogue(300, seed=17)
    o = L.fixcomp_model(cat)
    with pytest.raises(ValueError, match="deconvolve=True"):
        o.deconvolved_luminosities(device=False)
    o.close()


def test_c_abi_entries_and_constants():
    import os
    import re
    from lumfuncmcmc_amd import build, capi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "lfmcmc.h")).read()
    assert re.search(r"int lf_lum_posterior\(lf_ctx \*ctx, const double \*theta, int R, double \*m1, double \*m2, int \*n_used\);", hdr)
    assert re.search(r"int lf_lum_posterior_info\(int \*row_tile, int \*max_rows\);", hdr)
    lib = capi.load()
    for name in ("lf_lum_posterior", "lf_lum_posterior_info"):
        assert name in capi.EXPORTS and hasattr(lib, name)
    info = capi.lum_posterior_info()
    lay = open(os.path.join(root, "lumfuncmcmc_amd", "csrc", "lf_layout.h")).read()
    assert "constexpr int LUMPOST_RT = %d;" % info["row_tile"] in lay and info["max_rows"] == 4096
    assert "lf_lumpost.h" in " ".join(build.HEADERS)
