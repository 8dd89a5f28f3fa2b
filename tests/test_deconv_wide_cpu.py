"""The wide rule of the flux-error-convolved likelihood on the host (lumfuncmcmc_amd/deconv.py with wide=True, the NumPy twin of
csrc/lf_deconv_wide.h): the tables against numpy's Gauss-Legendre rule and the library's own, the
quadrature against 30-digit integration at every class's upper edge and just above every order's limit, the class assignment
at the edges, the refusal above the top edge, the gradient against 30-digit differentiation, the seeded Eddington profile
without "deconv_unchecked", and the C ABI's bookkeeping.  No GPU.

Probe set: that of tests/test_deconv_cpu.py (sources at 0.5 Flim, at L* and 1 dex above it; theta at the centre of the prior
box and at alpha_C = 7 with alpha = -3 and +1) extended with a source at 0.25 Flim, 1.3 dex below L*.  It is the faint
sources at alpha_C = 7 that decide the range: their integrand peaks up to 2 sigma above the catalogued flux, so +-7 sigma leaves
1.5e-7 at 0.10 dex and +-7.5 sigma is taken (measured worst per class edge 0.10 .. 0.30: 3.6e-8, 6.1e-8, 4.3e-8, 3.0e-8,
3.8e-8; the table of what was tried is in DESIGN.md section 3.21)."""
import functools
import os
import re

import numpy as np
import pytest

import lf_deconvlib as L
from lumfuncmcmc_amd import deconv as D
from lumfuncmcmc_amd import grad as G
from test_deconv_cpu import FCMIN, PROBE_THETA
from test_deconv_grad_cpu import FORMULA_BOUND

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLUX = np.array([0.25, 0.5, 5.0, 50.0])            # in units of Flim
DLUM = np.array([-1.3, -1.0, 0.0, 1.0])            # L - L*
ELEMS = (0, 2, 3, 4)                               # the probe's theta: L*, phi*, alpha, Flim, alpha_C


def _probe(name):
    Ls, al, Flim, aC = PROBE_THETA[name]
    inp = {"variant": "free", "fix_sch_al": False, "sch_al0": -1.6, "field_ind": np.array([0, 4]), "lum": Ls + DLUM,
           "logf": np.log10(FLUX * Flim) - 17.0, "fcmin": FCMIN}
    return inp, np.array([Ls, -3.0, al, Flim, aC])


def _mp_term(mp, Ls, al, Flim, aC):
    a = (2 * mp.mpf(FCMIN) - 1) ** 2
    kappa = mp.sqrt(abs(a / (1 - a)))

    def t(L, lf):
        y = lf + 17 - mp.log10(Flim)
        num = aC * y
        fc = (1 + num / mp.sqrt(1 + num * num)) / 2
        d = 1 - mp.exp(-mp.mpf(10) ** (y + kappa / aC))
        return mp.log(10) * (al + 1) * (L - Ls) - mp.mpf(10) ** (L - Ls) + mp.log(fc) / d
    return t


@functools.lru_cache(maxsize=None)
def _exact(name, sig):
    """ln of the convolution integral over the plain term, for the four probe sources, by 30-digit quadrature"""
    import mpmath as mp
    mp.mp.dps = 30
    inp, _ = _probe(name)
    t = _mp_term(mp, *(mp.mpf(v) for v in PROBE_THETA[name]))
    sig = mp.mpf(sig)
    out = []
    for Li, lf in zip(inp["lum"], inp["logf"]):
        Li, lf = mp.mpf(float(Li)), mp.mpf(float(lf))
        t0 = t(Li, lf)
        f = lambda u: mp.exp(-u * u / (2 * sig * sig)) / (sig * mp.sqrt(2 * mp.pi)) * mp.exp(t(Li + u, lf + u) - t0)   # noqa: E731
        out.append(float(mp.log(mp.quad(f, [k * sig for k in (-12, -9, -6, -4, -3, -2, -1, 0, 1, 2, 3, 4, 6, 9, 12)]))))
    return np.array(out)


def _worst(sig, K=D.DEFAULT_ORDER):
    w = 0.0
    for name in PROBE_THETA:
        inp, th = _probe(name)
        di = D.delta(inp, np.full(4, sig), th, K=K, terms=True, wide=True)[1]
        w = max(w, float(np.max(np.abs(di - _exact(name, float(sig))))))
    return w


def test_constants_and_panels():
    assert len(D.WIDE_EDGES) == len(D.WIDE_PANELS) and list(D.WIDE_EDGES) == sorted(D.WIDE_EDGES)
    assert D.WIDE_EDGES[0] > D.SIGMA_MAX and D.WIDE_SIGMA_MAX == D.WIDE_EDGES[-1] == 0.30
    for s, p in zip(D.WIDE_EDGES, D.WIDE_PANELS):          # the fewest panels that are at most h dex wide at the upper edge
        assert 2 * D.WIDE_T * s / p <= D.WIDE_H * (1 + 1e-12) and 2 * D.WIDE_T * s / (p - 1) > D.WIDE_H


@pytest.mark.parametrize("n", [1, 2, 5, 6, 8, 12, 16])
def test_gauss_legendre_against_numpy(n):
    x, w = D.gauss_legendre(n)
    rx, rw = np.polynomial.legendre.leggauss(n)
    assert np.max(np.abs(x.astype(np.float64) - rx)) <= 1e-15 and np.max(np.abs(w.astype(np.float64) - rw)) <= 1e-15


@pytest.mark.parametrize("c", range(len(D.WIDE_EDGES)))
def test_tables(c):
    """the twin's table is numpy's rule panel by panel, the library's own derivation (lf_hostprep.h) agrees to 1e-15, and the
    weights sum to 1 within the +-T tail mass plus the rule's own error on the Gaussian (8 nodes on a panel of 2.5 sigma:
    measured 1.7e-11 for class 0, far below the 1e-7 the rule is chosen for; bound 1e-10)"""
    from math import erfc, sqrt
    from lumfuncmcmc_amd import capi
    x, lnw = D.wide_table(c)
    P, n, T = D.WIDE_PANELS[c], D.WIDE_NPANEL, D.WIDE_T
    assert x.size == lnw.size == P * n and np.all(np.diff(x) > 0.0)
    rx, rw = np.polynomial.legendre.leggauss(n)
    half = T / P
    u = np.concatenate([-T + (2 * p + 1) * half + half * rx for p in range(P)])
    wt = np.concatenate([rw * half * np.exp(-0.5 * (-T + (2 * p + 1) * half + half * rx) ** 2) / np.sqrt(2 * np.pi) for p in range(P)])
    assert np.max(np.abs(x * np.sqrt(2.0) - u)) <= 1e-14 and np.max(np.abs(np.exp(lnw) / wt - 1.0)) <= 1e-13
    tail = erfc(T / sqrt(2.0))
    assert abs(np.sum(np.exp(lnw)) - 1.0) <= tail + 1e-10
    info = capi.deconv_wide_info(tables=True)
    cx, cl = info["tables"][c]
    assert info["nodes"][c] == x.size and np.max(np.abs(cx - x)) <= 1e-15 and np.max(np.abs(cl - lnw)) <= 1e-15


@pytest.mark.parametrize("c", range(len(D.WIDE_EDGES)))
def test_wide_rule_reaches_1e_7_at_each_class_upper_edge(c):
    w = _worst(D.WIDE_EDGES[c])
    print("class %d sigma = %.2f, %d nodes: worst per-source error %.2e" % (c, D.WIDE_EDGES[c], D.wide_table(c)[0].size, w))
    assert w < 1e-7


@pytest.mark.parametrize("K", [4, 12, 32])
def test_wide_rule_reaches_1e_7_just_above_the_narrow_limit(K):
    sig = np.nextafter(D.sigma_max(K), 1.0)
    assert D.wide_class([sig], K)[0] == 0
    w = _worst(sig, K)
    print("K = %d sigma = nextafter(%.2f): worst per-source error %.2e" % (K, D.sigma_max(K), w))
    assert w < 1e-7


def test_class_assignment_at_the_edges():
    for K in (4, 32):
        lim = D.sigma_max(K)
        sg = [0.0, lim, np.nextafter(lim, 1.0)] + [v for s in D.WIDE_EDGES for v in (s, np.nextafter(s, 1.0))][:-1]
        want = [-1, -1, 0] + [v for c in range(len(D.WIDE_EDGES)) for v in (c, c + 1)][:-1]
        assert list(D.wide_class(sg, K)) == want
    # a source at or below the limit keeps the order's sum and its bits
    inp, th = _probe("centre")
    sg = np.array([0.0, 0.05, D.SIGMA_MAX, 0.2])
    a = D.delta(inp, sg, th, terms=True, wide=True)[1]
    b = D.delta(inp, np.where(sg > D.SIGMA_MAX, 0.0, sg), th, terms=True)[1]
    assert np.array_equal(a[:3], b[:3]) and a[0] == 0.0 and a[3] != 0.0 and b[3] == 0.0


def test_top_edge_is_accepted_and_above_it_refused_with_the_limit_stated():
    inp, th = _probe("centre")
    assert np.isfinite(D.delta(inp, np.full(4, D.WIDE_SIGMA_MAX), th, wide=True, unchecked=False))
    with pytest.raises(ValueError, match="above 0.30 dex.*deconv_wide"):
        D.delta(inp, np.array([0.0, 0.1, np.nextafter(D.WIDE_SIGMA_MAX, 1.0), 0.2]), th, wide=True)
    with pytest.raises(ValueError, match="0.09 dex"):                       # without the option: the order's refusal as it was
        D.delta(inp, np.full(4, 0.2), th, unchecked=False)
    from lf_testlib import synth
    cat = synth.catalogue(300, seed=17)
    cat["lum_e"] = np.full(300, 0.2)
    with pytest.raises(ValueError, match="0.09 dex"):
        L.fixcomp_model(cat, deconvolve=True)
    o = L.fixcomp_model(cat, deconvolve=True, deconvolve_wide=True)
    assert o.deconvolve_wide and L.fixcomp_model(cat).deconvolve_wide is False
    cat["lum_e"][5] = 0.31
    with pytest.raises(ValueError, match="above 0.30 dex"):
        L.fixcomp_model(cat, deconvolve=True, deconvolve_wide=True)


def _exact_grad(name, sig, x, lnw):
    """d ln sum_k exp(lnw_k + t_ik - t_i) / d (L*, alpha, Flim, alpha_C) for the four probe sources, 30 digits: the twin is the
    exact derivative of the sum, so the reference differentiates that sum (tests/test_deconv_grad_cpu.py)"""
    import mpmath as mp
    mp.mp.dps = 30
    inp, th = _probe(name)
    out = []
    for Li, lf in zip(inp["lum"], inp["logf"]):
        Li, lf = mp.mpf(float(Li)), mp.mpf(float(lf))

        def lnsum(Ls, al, Flim, aC):
            t = _mp_term(mp, Ls, al, Flim, aC)
            t0 = t(Li, lf)
            tot = mp.mpf(0)
            for k in range(len(x)):
                dl = mp.sqrt(2) * mp.mpf(sig) * mp.mpf(float(x[k]))
                tot += mp.exp(mp.mpf(float(lnw[k])) + t(Li + dl, lf + dl) - t0)
            return mp.log(tot)

        at = tuple(mp.mpf(float(th[e])) for e in ELEMS)
        out.append([float(mp.diff(lnsum, at, tuple(int(i == j) for i in range(4)))) for j in range(4)])
    return np.array(out)


@pytest.mark.parametrize("name,c", [("centre", 0), ("aC7_al-3", 2), ("aC7_al+1", 4)])
def test_wide_gradient_against_30_digit_differentiation(name, c):
    sig = D.WIDE_EDGES[c]
    inp, th = _probe(name)
    _, g, s = D.delta_grad(inp, np.full(4, sig), th, per_source=True, wide=True)
    ref = _exact_grad(name, sig, *D.wide_table(c))
    assert np.all(g[:, 1] == 0.0)
    ratio = np.abs(g[:, ELEMS] - ref) / s[:, ELEMS]
    print("wide gradient %s class %d: worst |twin - mpmath| / S_abs = %.2e" % (name, c, ratio.max()))
    assert ratio.max() <= FORMULA_BOUND


def test_eddington_profile_under_the_wide_rule():
    """the seeded 0.25-dex mock of tests/test_deconv_cpu.py with no "deconv_unchecked": the convolved maximum lies on the truth
    on the 41-point grid, the plain one above it"""
    inp, sigma, theta, rows = L.eddington_case()
    lp = G.lnprob_grad(inp, rows)[0]
    wide = lp + D.delta(inp, sigma, rows, wide=True, unchecked=False)
    k32 = lp + D.delta(inp, sigma, rows)
    i0 = L.EDD_GRID.size // 2
    print("Eddington profile, wide rule: N = %d, plain argmax %+.2f dex, convolved argmax %+.2f dex; the unchecked K = 32 sum lies "
          "%.3e .. %.3e from it in lnprob over the grid (%.3e at the truth)"
          % (len(sigma), L.EDD_GRID[int(np.argmax(lp))], L.EDD_GRID[int(np.argmax(wide))], np.min(k32 - wide), np.max(k32 - wide),
             (k32 - wide)[i0]))
    assert int(np.argmax(wide)) == i0 and int(np.argmax(lp)) > i0


def test_c_abi_entries_and_constants():
    from lumfuncmcmc_amd import build, capi
    hdr = open(os.path.join(ROOT, "include", "lfmcmc.h")).read()
    assert re.search(r"int lf_deconv_wide_info\(double \*edges, int32_t \*nodes, int cap, int \*chunk, double \*T, int \*npanel, "
                     r"double \*h, int cls, double \*x,\s+double \*lnw\);", hdr)
    lib = capi.load()
    assert "lf_deconv_wide_info" in capi.EXPORTS and hasattr(lib, "lf_deconv_wide_info")
    info = capi.deconv_wide_info()
    assert info["edges"] == D.WIDE_EDGES and info["nodes"] == tuple(p * D.WIDE_NPANEL for p in D.WIDE_PANELS)
    assert (info["chunk"], info["T"], info["nodes_per_panel"], info["h"]) == (D.WIDE_CHUNK, D.WIDE_T, D.WIDE_NPANEL, D.WIDE_H)
    x = np.empty(info["nodes"][0])
    assert lib.lf_deconv_wide_info(None, None, 0, None, None, None, None, 0, capi._ptr(x), None) == capi.LF_ERR_ARG
    assert lib.lf_deconv_wide_info(None, None, 0, None, None, None, None, len(D.WIDE_EDGES), capi._ptr(x), capi._ptr(x)) == capi.LF_ERR_ARG
    assert "lf_deconv_wide.h" in " ".join(build.HEADERS)
    lay = open(os.path.join(ROOT, "lumfuncmcmc_amd", "csrc", "lf_layout.h")).read()
    assert "constexpr int DECONV_WIDE_CH = %d;" % D.WIDE_CHUNK in lay
