"""The catalogued volume per node and the deconvolved 1/Veff points under the cut on the observed flux, on the host
(lumfuncmcmc_amd/deconv.py: cut_volume_fraction, cut_volume_table, veff_true(cut=...), the NumPy twins of
csrc/lf_vefftrue_cut.h).  No GPU.

Element accuracy: g against the same sum in 40-digit arithmetic.  The bound is derived, not measured: the relative condition of
Q(-u) in u is at most u^2 + 1 <= 82 inside |u| <= 9, u carries about 3 roundings (the subtraction, sigma's interpolation, the
division), erfc a few ulp: about 3e-14; asserted 1e-13 of g.  The truncation at |u| = 9 is part of the sum's definition: the
reference takes the branch the double u takes, and the double u is held to the 40-digit u separately (4 ulp).

Unbiasedness (test_points_are_unbiased_with_g_and_biased_without), seed 20 of tests/lf_cutlib.py's host generator, 200
replicates, one row at the truth: the margins found are printed by the test and recorded in its docstring."""
import numpy as np
import pytest

import lf_cutlib as C
from lf_testlib import synth
from lumfuncmcmc_amd import deconv as D
from lumfuncmcmc_amd import grad as G

EPS = np.finfo(np.float64).eps
MODELS = ["one", "sixteen", "flux"]


def model(kind, nf=1):
    if kind == "one":
        return C.const_model(0.2, nf=nf)
    if kind == "sixteen":
        nodes = np.log10(C.FCUT) + np.linspace(-0.6, 1.0, 16)
        sig = 0.05 + 0.2 * np.abs(np.sin(3.0 * np.arange(16)))               # kinks in both directions
        return nodes, np.repeat(sig[None], nf, axis=0)
    return C.flux_model(0.09, nf=nf)


def u_of(inp, nodes, sig, j, L):
    lam, _, _, _, _, ld2 = D._cut_grid(inp)
    return (L - lam[j]) / D._cut_sigma(nodes, sig, L - ld2[j])


def points_at_u(inp, nodes, sig, j, target):
    """L with u_j(L) = target to the last bits (bisection on the double u, monotone here), and its neighbours"""
    lam = D._cut_grid(inp)[0]
    lo, hi = lam[j] - 4.0, lam[j] + 4.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if mid == lo or mid == hi:
            break
        if u_of(inp, nodes, sig, j, mid) < target:
            lo = mid
        else:
            hi = mid
    return [np.nextafter(lo, -np.inf), lo, hi, np.nextafter(hi, np.inf)]


def element_points(inp, nodes, sig):
    """L on each lam_j and one ulp either side; at u = +/-9 and one ulp either side (the first, a middle and the last column)"""
    lam = D._cut_grid(inp)[0]
    S = lam.size
    pts = []
    for j in range(S):
        pts += [np.nextafter(lam[j], -np.inf), lam[j], np.nextafter(lam[j], np.inf)]
    for j in sorted({0, S // 2, S - 1}):
        for t in (-9.0, 9.0):
            pts += points_at_u(inp, nodes, sig, j, t)
    return np.array(pts)


def mp_g(inp, nodes, sig, L):
    """(g, worst |u_double - u_40| / |u_40|) of one point: the same sum in 40 digits, the truncation's branch the double's"""
    import mpmath as mp
    mp.mp.dps = 40
    lam, _, _, wz, vol, ld2 = D._cut_grid(inp)
    wv = wz * vol
    nd = [mp.mpf(float(x)) for x in nodes]
    sg = [mp.mpf(float(x)) for x in sig]
    Lm = mp.mpf(float(L))

    def s_of(t):
        if len(nd) == 1 or not t > nd[0]:
            return sg[0]
        if t >= nd[-1]:
            return sg[-1]
        i = max(k for k in range(len(nd) - 1) if nd[k] <= t)
        return sg[i] + (t - nd[i]) * ((sg[i + 1] - sg[i]) / (nd[i + 1] - nd[i]))

    num, den, du = mp.mpf(0), mp.mpf(0), 0.0
    for j in range(lam.size):
        u = (Lm - mp.mpf(float(lam[j]))) / s_of(Lm - mp.mpf(float(ld2[j])))
        ud = u_of(inp, nodes, sig, j, float(L))
        if u != 0:
            du = max(du, float(abs(mp.mpf(ud) - u) / abs(u)))
        w = mp.mpf(float(wv[j]))
        den += w
        if ud > D.CUT_UMAX:
            num += w
        elif not ud < -D.CUT_UMAX:
            num += w * mp.erfc(-u / mp.sqrt(2)) / 2
    return num / den, du


@pytest.mark.parametrize("S", [5, 101])
@pytest.mark.parametrize("kind", MODELS)
def test_element_accuracy_against_40_digits(kind, S):
    import mpmath as mp
    inp = C.cut_inputs("free", n=50, S=S, nf=1)
    nodes, sig = model(kind)
    L = element_points(inp, nodes, sig[0])
    g = D.cut_volume_fraction(inp, nodes, sig, 0, L)
    worst, worst_u = 0.0, 0.0
    for Li, gi in zip(L, g):
        ref, du = mp_g(inp, nodes, sig[0], Li)
        worst_u = max(worst_u, du)
        if ref == 0:
            assert gi == 0.0, (kind, S, Li, gi)
            continue
        worst = max(worst, float(abs(mp.mpf(float(gi)) - ref) / ref))
    print("cut volume %-8s S=%3d: %d points, worst |g - ref| / ref = %.2e (bound 1e-13), worst u %.2e (%.1f ulp)"
          % (kind, S, L.size, worst, worst_u, worst_u / EPS))
    assert worst <= 1e-13 and worst_u <= 4 * EPS
    assert np.all((g >= 0.0) & (g <= 1.0 + 4 * S * EPS))


@pytest.mark.parametrize("S", [5, 101])
@pytest.mark.parametrize("kind", MODELS)
def test_exact_above_and_below_every_edge(kind, S):
    inp = C.cut_inputs("free", n=50, S=S, nf=1)
    nodes, sig = model(kind)
    lam = D._cut_grid(inp)[0]
    smax = float(sig.max())
    L = np.array([lam.max() + 9.0 * smax + 1e-9, lam.max() + 3.0, lam.min() - 9.0 * smax - 1e-9, lam.min() - 3.0])
    g = D.cut_volume_fraction(inp, nodes, sig, 0, L)
    assert g[0] == 1.0 and g[1] == 1.0 and g[2] == 0.0 and g[3] == 0.0, g


@pytest.mark.parametrize("S", [5, 101])
def test_zero_sigma_field_is_the_steps_prefix_sum(S):
    """two fields, the second without errors: g is the prefix sum of wv over the columns with lam_j <= L, bit for bit"""
    inp = C.cut_inputs("free", n=60, S=S, nf=2)
    nodes, sig = C.const_model(0.1, nf=2)
    sig[1] = 0.0
    lam, _, _, wz, vol, _ = D._cut_grid(inp)
    L = np.concatenate([lam, np.nextafter(lam, -np.inf), np.nextafter(lam, np.inf), [lam.min() - 1.0, lam.max() + 1.0]])
    g = D.cut_volume_fraction(inp, nodes, sig, 1, L)
    wv = wz * vol
    den = 0.0
    for j in range(S):
        den += float(wv[j])
    ref = np.empty(L.size)
    for i, Li in enumerate(L):
        acc = 0.0
        for j in range(S):
            acc += float(wv[j]) if Li >= lam[j] else 0.0
        ref[i] = acc / den
    assert np.array_equal(g, ref)
    assert g[-2] == 0.0 and g[-1] == 1.0
    # the other field, with errors, differs at the edges
    assert not np.array_equal(D.cut_volume_fraction(inp, nodes, sig, 0, L), ref)


def _catalogue_above(variant, n=120, nf=2):
    """a catalogue wholly above every lam_j, a tenth of the sources without errors"""
    inp = C.cut_inputs(variant, n=n, S=5, nf=nf)
    lam = D._cut_grid(inp)[0]
    lum = np.asarray(inp["lum"], dtype=np.float64)
    shift = max(0.0, float(lam.max() + 0.5 - lum.min()))
    inp["lum"] = lum + shift
    if inp.get("logf") is not None:
        inp["logf"] = np.asarray(inp["logf"]) + shift
    sg = np.random.default_rng(5).uniform(0.01, 0.09, n)
    sg[::10] = 0.0
    return inp, sg


@pytest.mark.parametrize("variant", ["free", "fixcomp", "zevol"])
def test_zero_sigma_model_above_every_edge_keeps_the_bits(variant):
    inp, sg = _catalogue_above(variant)
    nf = len(inp["field_ind"]) - 1
    th = synth.walkers(variant, 4, seed=3, fix_sch_al=False, nf=nf)
    lum = np.asarray(inp["lum"])
    edges = np.linspace(lum.min() - 0.3, lum.max() + 0.3, 12)
    plain, used = D.veff_true(inp, sg, th, edges, 3.1e-5, 2.7e6, K=8)
    cutv, used_c = D.veff_true(inp, sg, th, edges, 3.1e-5, 2.7e6, K=8, cut=C.const_model(0.0, nf=nf))
    assert used == used_c and used > 0
    assert np.array_equal(plain, cutv, equal_nan=True)
    q0 = D.veff_true_quantiles(inp, sg, th, edges, 3.1e-5, 2.7e6, K=8)
    q1 = D.veff_true_quantiles(inp, sg, th, edges, 3.1e-5, 2.7e6, K=8, cut=C.const_model(0.0, nf=nf))
    assert np.array_equal(q0[0], q1[0], equal_nan=True)


def test_min_vol_frac_drops_exactly_the_nodes_below_it():
    inp = C.cut_inputs("free", n=150, S=23, nf=2)
    n = len(inp["lum"])
    sg = np.random.default_rng(2).uniform(0.02, 0.3, n)
    sg[::10] = 0.0
    cut = C.flux_model(0.09, nf=2)
    K = 8
    tab0, d0 = D.cut_volume_table(inp, sg, cut, K=K, wide=True)
    slots = 0
    gs = []
    for (g, keep), (sub, idx, x, lnw) in zip(tab0, D._rules(inp, sg, K, True)):
        s = sg[idx]
        live = np.ones(g.shape, dtype=bool)
        live[1:, s == 0.0] = False
        slots += int(live.sum())
        gs.append(g[live])
    gs = np.concatenate(gs)
    assert slots == int((sg == 0).sum()) + sum(int(((sg > 0) & (D.wide_class(sg, K) == c)).sum()) * k
                                                for c, k in [(-1, K)] + [(c, len(D.wide_table(c)[0])) for c in range(5)])
    assert d0 == int((gs == 0.0).sum())
    mvf = float(np.median(gs[gs > 0.0]))
    tab1, d1 = D.cut_volume_table(inp, sg, cut, K=K, wide=True, min_vol_frac=mvf)
    assert d1 == int((gs < mvf).sum()) and d0 < d1 < slots
    # the points: dropping the nodes can only lower a bin, and the kept nodes' bins are those of a table masked by hand
    th = C.probe_thetas(inp)[:1]
    th = np.concatenate([th[0, :3], [3.5, 3.5, 4.0]])[None]
    edges = np.linspace(np.min(inp["lum"]) - 0.5, np.max(inp["lum"]) + 0.5, 9)
    v0, _ = D.veff_true(inp, sg, th, edges, 3.1e-5, 2.7e6, K=K, wide=True, cut=cut)
    v1, _ = D.veff_true(inp, sg, th, edges, 3.1e-5, 2.7e6, K=K, wide=True, cut=cut, min_vol_frac=mvf)
    assert np.all(v1 <= v0) and np.any(v1 < v0) and np.all(np.isfinite(v0))


def _truth(th, edges):
    """int over each bin of phi(L) dL, phi per dex as deconv._cut_phi_omega writes it"""
    from scipy.integrate import quad
    Ls, ph, al = th[0], th[1], th[2]
    f = lambda L: G.LN10 * np.exp(G.LN10 * (ph + (L - Ls) * (al + 1.0)) - 10.0 ** (L - Ls))        # noqa: E731
    return np.array([quad(f, a, b, epsabs=0.0, epsrel=1e-11)[0] for a, b in zip(edges[:-1], edges[1:])])


SEED, REPS, SIGMA = 20, 200, 0.2
PHI_SHIFT = -0.7                # phi* below the synthetic one: about 1300 catalogued sources per replicate


def test_points_are_unbiased_with_g_and_biased_without():
    """The host generator of the cut process (tests/lf_cutlib.py: poisson_catalogue), one field, sigma = 0.2 dex, alpha = -2, 200
    replicates, one row at the truth, vol = sum_j wz_j V_j (so that the expectation of a bin is int phi dL).  With g the mean
    of the binned points agrees with the binned truth within 4 standard errors in every bin of at least 50 sources (mean per
    replicate) whose lower edge lies above the faintest lam_j + 1 sigma; with cut=None at least one bin within 3 sigma of the
    edges misses by more than 5.  Margins found with seed 20 (about 1300 catalogued sources per replicate; the faintest edge at
    41.53, bins of 0.2 dex): four tested bins, [41.93, 42.73), with g at -0.62, +0.34, +0.24, +0.00 standard errors (worst 0.62
    of the 4 allowed); the same bins with cut=None at -46.3, -6.05, -0.18, -0.01, and the two bins just above the edge at -602
    and -187 (5 needed in one).  The three bins below the faintest edge hold no catalogued source and are fed by posterior
    nodes with g far below 1 (heavy tails: +4.0, +4.4, +1.4 with g); they are not tested, as the issue sets it."""
    inp = C.cut_inputs("free", n=50, S=5, nf=1)
    cut = C.const_model(SIGMA)
    th = np.array([synth.LSTAR, synth.PHISTAR + PHI_SHIFT, -2.0, 3.5, 4.0])
    lam, _, _, wz, vol, _ = D._cut_grid(inp)
    den = float(np.sum(wz * vol))
    pref0 = float(np.asarray(inp["Omega_0"], dtype=np.float64)[0]) / G.SQARCSEC
    edges = lam.min() - 0.6 + 0.2 * np.arange(13)
    assert edges[-1] < synth.LH - 4 * SIGMA
    truth = _truth(th, edges)
    with_g, plain, counts = (np.empty((REPS, edges.size - 1)) for _ in range(3))
    for r in range(REPS):
        cat, s = C.poisson_catalogue(inp, th, cut[0], cut[1][0], seed=SEED * 1000 + r)
        assert np.all(s == SIGMA)
        with_g[r] = D.veff_true(cat, s, th, edges, pref0, den, K=8, wide=True, cut=cut)[0][0]
        plain[r] = D.veff_true(cat, s, th, edges, pref0, den, K=8, wide=True)[0][0]
        counts[r] = np.histogram(cat["lum"], edges)[0]
    se = lambda a: a.std(axis=0, ddof=1) / np.sqrt(REPS)                       # noqa: E731
    zg = (with_g.mean(axis=0) - truth) / se(with_g)
    zp = (plain.mean(axis=0) - truth) / se(plain)
    tested = (counts.mean(axis=0) >= 50.0) & (edges[:-1] > lam.min() + SIGMA)
    near = (edges[1:] > lam.min() - 3 * SIGMA) & (edges[:-1] < lam.max() + 3 * SIGMA)
    for b in range(edges.size - 1):
        print("bin %2d [%.2f, %.2f) sources %6.1f truth %.4e with g %+6.2f se, plain %+7.2f se%s%s"
              % (b, edges[b], edges[b + 1], counts[:, b].mean(), truth[b], zg[b], zp[b], "  tested" if tested[b] else "",
                 "  near" if near[b] else ""))
    print("with g: worst |z| of %d tested bins %.2f (bound 4); plain: worst |z| of %d near bins %.2f (must exceed 5)"
          % (tested.sum(), np.abs(zg[tested]).max(), near.sum(), np.abs(zp[near]).max()))
    assert tested.sum() >= 3
    assert np.all(np.abs(zg[tested]) <= 4.0)
    assert np.any(np.abs(zp[near]) > 5.0)

