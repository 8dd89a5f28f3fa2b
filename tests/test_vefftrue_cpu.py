"""The deconvolved 1/Veff points on the host (lumfuncmcmc_amd/deconv.py: veff_true, the NumPy twin of csrc/lf_vefftrue.h;
DESIGN.md section 3.26): the all-zero-error limit against veff.veff_draws, the bin arithmetic and the edge rule, dropped nodes,
unused rows, the accuracy of the binned rule against 30-digit integrals, and the calibration against the binned TRUE luminosities of a seeded mock.  No GPU.

Calibration, measured on the seeded 0.08-dex mock of tests/test_lumpost_cpu.py (one row at the truth, 25 bins; distance =
sum_b |points_b - truth_b| / sum_b truth_b): the figures are printed by the test and recorded in DESIGN.md section 3.26.  The binned rule itself - a discrete measure on the nodes - is held against per-source
integrals between the bin edges in 30-digit arithmetic (test_accuracy_of_the_binned_rule_against_30_digit_integrals)."""
import numpy as np
import pytest

from lf_testlib import make_inputs, synth
from lumfuncmcmc_amd import deconv as D
from lumfuncmcmc_amd import grad as G
from lumfuncmcmc_amd import hostsetup as hs
from lumfuncmcmc_amd import veff

PREF0, VOL = 3.1e-5, 2.7e6


def _free_inputs(n, seed=8):
    inp = make_inputs("free", n, seed=seed, S=11)
    nf = len(inp["field_ind"]) - 1
    th = synth.walkers("free", 6, seed=3, fix_sch_al=False, nf=nf)
    assert np.isfinite(G.lnprob_grad(inp, th)[0]).all()
    return inp, th


def _node_lums(inp, sg, K=D.DEFAULT_ORDER):
    """lum_i + dl_ik by the stated expression: one rounded product, one rounded add"""
    x, _ = D.gauss_hermite(K)
    s2 = np.sqrt(2.0) * sg
    return np.asarray(inp["lum"], dtype=float)[None] + s2[None] * x[:, None]


def test_all_zero_errors_equal_veff_draws():
    """sigma = 0 everywhere, FREE: every source is veff_draws' own term - exp(-l) against 1 / fleming, to rtol 1e-12 per bin
    (fluxes >= 0.5 Flim, alpha_C <= 3.5: beyond, fleming's own cancellation shows)"""
    inp, th = _free_inputs(3000, seed=17)
    fi = np.asarray(inp["field_ind"])
    nf = len(fi) - 1
    field = np.repeat(np.arange(nf), np.diff(fi))
    th[:, 3 + nf] = np.linspace(2.0, 3.5, len(th))
    assert np.isfinite(G.lnprob_grad(inp, th)[0]).all()
    logf = G.log_flux(inp["lum"], inp["DLz"])
    flux = 10.0 ** logf
    keep = np.flatnonzero(flux >= 0.5 * 1e-17 * th[:, 3:3 + nf].max(axis=0)[field])
    assert keep.size >= 1500
    sub = D._subset(inp, keep)
    lum = np.asarray(sub["lum"])
    sfield = field[keep]
    edges, _, _, idx = veff.luminosity_bins(lum, 25)
    vals, used = D.veff_true(sub, np.zeros(keep.size), th, edges, PREF0, VOL)
    assert used == len(th)
    draws = np.column_stack([1.0e-17 * th[:, 3:3 + nf], th[:, 3 + nf]])
    ref = veff.veff_draws(flux[keep], sfield, VOL, PREF0, inp["fcmin"], idx, 25, draws)
    assert np.all(ref > 0.0)
    worst = float(np.max(np.abs(vals - ref) / ref))
    print("sigma = 0 against veff_draws: worst relative difference %.2e" % worst)
    assert worst <= 1e-12


@pytest.mark.parametrize("variant", ["free", "fixcomp", "zevol"])
def test_one_bin_is_the_sum_of_25(variant):
    n = 400
    inp = make_inputs(variant, n, seed=8, S=11)
    th = synth.walkers(variant, 3, seed=3, fix_sch_al=False, nf=5)
    sg = np.random.default_rng(2).uniform(0.0, D.WIDE_SIGMA_MAX, n)
    sg[::5] = 0.0
    lum = np.asarray(inp["lum"])
    edges = np.linspace(lum.min() - 0.2, lum.max() + 0.1, 26)
    many, used = D.veff_true(inp, sg, th, edges, PREF0, VOL, wide=True)
    one, _ = D.veff_true(inp, sg, th, edges[[0, -1]], PREF0, VOL, wide=True)
    assert used == 3 and np.all(many >= 0.0) and np.all(one > 0.0)
    assert np.all(np.abs(many.sum(axis=1) - one[:, 0]) <= 1e-12 * one[:, 0])


def test_dropped_nodes_and_unused_rows():
    n = 120
    inp, th = _free_inputs(n)
    sg = np.random.default_rng(2).uniform(0.01, 0.09, n)
    sg[::5] = 0.0
    L = _node_lums(inp, sg)
    # edges above every node of every source: nothing lands, exactly 0
    hi = np.linspace(L.max() + 0.01, L.max() + 1.0, 5)
    vals, used = D.veff_true(inp, sg, th, hi, PREF0, VOL)
    assert used == 6 and np.all(vals == 0.0)
    # the faintest source's nodes all lie below edges[0]: the values are those of the catalogue without it, bit for bit
    j = int(np.argmin(inp["lum"]))
    sj = sg.copy()
    sj[j] = 0.05
    Lj = _node_lums(inp, sj)
    ed = np.linspace(Lj[:, j].max() + 1e-6, Lj.max(), 11)
    assert (np.asarray(inp["lum"]) > ed[0]).sum() > n // 2
    a, _ = D.veff_true(inp, sj, th, ed, PREF0, VOL)
    rest = np.delete(np.arange(n), j)
    c, _ = D.veff_true(D._subset(inp, rest), sj[rest], th, ed, PREF0, VOL)
    assert np.array_equal(a, c) and np.all(a.sum(axis=1) > 0.0)
    # a row outside the box: NaN row, n_used one less, the other rows keep their bits
    edges = np.linspace(L.min(), L.max(), 26)
    full, _ = D.veff_true(inp, sg, th, edges, PREF0, VOL)
    out = th.copy()
    out[2, 0] = 39.5
    b, ub = D.veff_true(inp, sg, out, edges, PREF0, VOL)
    assert ub == 5 and np.all(np.isnan(b[2])) and np.array_equal(np.delete(b, 2, axis=0), np.delete(full, 2, axis=0))
    q, _, uq = D.veff_true_quantiles(inp, sg, out, edges, PREF0, VOL, q=(0.0, 50.0, 100.0))
    assert uq == 5 and np.array_equal(q, np.percentile(np.delete(full, 2, axis=0), (0.0, 50.0, 100.0), axis=0))
    out[:, 0] = 39.5
    q, v, uq = D.veff_true_quantiles(inp, sg, out, edges, PREF0, VOL)
    assert uq == 0 and np.all(np.isnan(q)) and np.all(np.isnan(v)) and q.shape == (3, 25)


def engineered_edges(inp, sg, K=D.DEFAULT_ORDER, count=12, seed=4):
    """edges equal to `count` node luminosities lum_i + dl_ik of sources with sigma > 0 (plus an outer pair), and the (k, i)
    of those nodes"""
    L = _node_lums(inp, sg, K)
    rng = np.random.default_rng(seed)
    on = np.flatnonzero(sg > 0.0)
    pick = [(int(rng.integers(0, L.shape[0])), int(i)) for i in rng.permutation(on)[:count]]
    vals = sorted({float(L[k, i]) for k, i in pick})
    edges = np.array([min(L.min(), vals[0]) - 0.5] + vals + [max(L.max(), vals[-1]) + 0.5])
    assert np.all(np.diff(edges) > 0.0)
    return edges, pick, L


def test_a_node_on_an_edge_goes_to_the_upper_bin():
    n = 60
    inp, th = _free_inputs(n)
    sg = np.random.default_rng(5).uniform(0.02, 0.09, n)
    edges, pick, L = engineered_edges(inp, sg)
    x, lnw = D.gauss_hermite(D.DEFAULT_ORDER)
    with np.errstate(all="ignore"):
        p, Lk, l = D._row_terms(inp, sg, th[0], x, lnw, nodes=True)
    assert np.array_equal(Lk, L)
    base, _ = D.veff_true(inp, sg, th[0], edges, PREF0, VOL)
    for k, i in pick:
        e = int(np.flatnonzero(edges == L[k, i])[0])
        assert np.searchsorted(edges, L[k, i], side="right") - 1 == e            # the bin that starts at this edge
        mass = p[k, i] * (np.exp(-l[k, i]) / (PREF0 * VOL))
        assert mass > 0.0
        # the edge one ulp higher: this node (and any other exactly there) moves to the bin below
        up = edges.copy()
        up[e] = np.nextafter(up[e], np.inf)
        moved, _ = D.veff_true(inp, sg, th[0], up, PREF0, VOL)
        there = Lk == L[k, i]
        m_all = float(np.sum(p[there] * (np.exp(-l[there]) / (PREF0 * VOL))))
        assert mass <= m_all * (1 + 1e-15)
        assert abs((base[0, e] - moved[0, e]) - m_all) <= 1e-12 * base[0, e]
        assert abs((moved[0, e - 1] - base[0, e - 1]) - m_all) <= 1e-12 * moved[0, e - 1]


def test_calibration_against_the_binned_true_luminosities():
    """on the seeded 0.08-dex mock with one row at the truth, 25 bins: over the populated bins the deconvolved points lie
    closer than the plain 1/Veff points to the binned TRUE luminosities weighted 1 / (pref0 fc(true flux) vol); distance =
    sum_b |points_b - truth_b| / sum_b truth_b.  Populated: at least 50 catalogued sources, the line the accuracy record of
    DESIGN.md section 3.26 draws too.  Below it the truth itself is no yardstick: the weights 1 / fc are heavy-tailed at the
    faint end (the largest is 8e5 times the smallest on this mock), and a bin of 4 to 37 sources is the weight of the one
    faintest true flux that happened to land in it - over the bins of 5 .. 49 sources the two distances are 1.63 (deconvolved)
    and 1.13 (plain), both of the order of the truth itself; they are printed, not asserted."""
    from test_lumpost_cpu import _calibration_case
    inp, sigma, theta, true = _calibration_case()
    fi = np.asarray(inp["field_ind"])
    nf = len(fi) - 1
    field = np.repeat(np.arange(nf), np.diff(fi))
    lum = np.asarray(inp["lum"])
    logf = G.log_flux(lum, inp["DLz"])
    flux, flux_true = 10.0 ** logf, 10.0 ** (logf + (true - lum))
    edges, _, _, idx = veff.luminosity_bins(lum, 25)
    draws = np.concatenate([1.0e-17 * theta[3:3 + nf], theta[3 + nf:]])[None]
    plain = veff.veff_draws(flux, field, VOL, PREF0, inp["fcmin"], idx, 25, draws)[0]
    tidx = np.searchsorted(edges, true, side="right") - 1
    tidx[(tidx < 0) | (tidx >= 25)] = 25
    w_true = 1.0 / (PREF0 * hs.fleming(flux_true, draws[0, :nf][field], draws[0, nf], inp["fcmin"]) * VOL)
    truth = np.bincount(tidx, weights=w_true, minlength=26)[:25]
    dec, used = D.veff_true(inp, sigma, theta, edges, PREF0, VOL)
    assert used == 1
    cnt = np.bincount(idx, minlength=26)[:25]
    dist = lambda x, sel: float(np.sum(np.abs(x[sel] - truth[sel])) / np.sum(truth[sel]))          # noqa: E731
    pop, few = cnt >= 50, (cnt >= 5) & (cnt < 50)
    assert pop.sum() >= 10
    d_dec, d_plain = dist(dec[0], pop), dist(plain, pop)
    print("calibration over the %d bins of >= 50 sources: distance to the binned truth %.4f (deconvolved), %.4f (plain)"
          % (pop.sum(), d_dec, d_plain))
    print("             over the %d bins of 5 .. 49 sources (not asserted): %.4f (deconvolved), %.4f (plain)"
          % (few.sum(), dist(dec[0], few), dist(plain, few)))
    assert d_dec < d_plain


ACC_BINS, ACC_WINDOW = 25, 9        # bins of the accuracy case; half-width of a source's integration window in sigma


def _exact_points(inp, sigma, theta, edges, gl_degree=3, only=None):
    """values[b] of the section's quantity with the rule replaced by the integral: per source (FREE) the posterior density
    N(u; 0, sigma^2) exp(t(L + u, f 10^u) - t(L, f)) / Z_i integrated between the bin edges against 1 / fc(f 10^u), in 30-digit
    arithmetic.  The window [-9 sigma, 9 sigma] (the mass beyond is below 1e-18) is cut at every bin edge and each panel - at
    most one bin wide, 1.4 sigma here - taken by mpmath's Gauss-Legendre rule of the given degree (3: 12 nodes, error below
    1e-20 of the panel's value, checked against degree 4 in the test); t is tests/test_deconv_wide_cpu.py's _mp_term, written
    out so that 10^u is formed once per node.  In the product density x 1 / fc the completeness cancels: the numerator needs
    no fc at all.  No source's window lies inside one bin at these widths, so the closed form the section mentions has no
    case.  only: the sources to take (default all).  Returns the float array [nbin]."""
    import mpmath as mp
    from mpmath.calculus.quadrature import GaussLegendre
    mp.mp.dps = 30
    gl = GaussLegendre(mp.mp).calc_nodes(gl_degree, mp.mp.prec)
    fi = np.asarray(inp["field_ind"])
    nf = len(fi) - 1
    field = np.repeat(np.arange(nf), np.diff(fi))
    lum = np.asarray(inp["lum"], dtype=float)
    logf = G.log_flux(lum, inp["DLz"])
    Ls, al, aC = mp.mpf(float(theta[0])), mp.mpf(float(theta[2])), mp.mpf(float(theta[3 + nf]))
    lF = [mp.log10(mp.mpf(float(theta[3 + f]))) for f in range(nf)]
    a = (2 * mp.mpf(float(inp["fcmin"])) - 1) ** 2
    kappa = mp.sqrt(abs(a / (1 - a)))
    ln10, c1l = mp.log(10), mp.log(10) * (al + 1)
    ed = [mp.mpf(float(e)) for e in edges]
    nbin = len(ed) - 1
    tot = [mp.mpf(0)] * nbin
    for i in (range(len(lum)) if only is None else only):
        sig = mp.mpf(float(sigma[i]))
        Li = mp.mpf(float(lum[i]))
        y0 = mp.mpf(float(logf[i])) + 17 - lF[field[i]]
        T = mp.exp(ln10 * (Li - Ls))
        v0 = mp.exp(ln10 * (y0 + kappa / aC))
        i2s = 1 / (2 * sig * sig)

        def lcomp(y, v):
            num = aC * y
            return mp.log((1 + num / mp.sqrt(1 + num * num)) / 2) / (1 - mp.exp(-v))
        l0 = lcomp(y0, v0)
        lo, hi = -ACC_WINDOW * sig, ACC_WINDOW * sig
        cuts = [lo] + [e - Li for e in ed if lo < e - Li < hi] + [hi]
        Z, parts = mp.mpf(0), []
        for pa, pb in zip(cuts[:-1], cuts[1:]):
            half, mid = (pb - pa) / 2, (pb + pa) / 2
            sn = sz = mp.mpf(0)
            for xg, wg in gl:
                u = mid + half * xg
                E = mp.exp(ln10 * u)
                g = wg * mp.exp(c1l * u - T * (E - 1) - u * u * i2s)
                sn += g
                sz += g * mp.exp(lcomp(y0 + u, v0 * E) - l0)
            Z += half * sz
            b = int(np.searchsorted(edges, float(Li + mid), side="right")) - 1
            if 0 <= b < nbin:
                parts.append((b, half * sn))
        for b, v in parts:
            tot[b] += v * mp.exp(-l0) / Z
    return np.array([float(v / (mp.mpf(PREF0) * mp.mpf(VOL))) for v in tot])


def _accuracy_case():
    """(per-bin catalogued counts, exact points, the twin's points at K = 32) on the seeded 0.08-dex mock, one row at the truth"""
    from test_lumpost_cpu import _calibration_case
    inp, sigma, theta, _ = _calibration_case()
    lum = np.asarray(inp["lum"])
    edges, _, _, idx = veff.luminosity_bins(lum, ACC_BINS)
    cnt = np.bincount(idx, minlength=ACC_BINS + 1)[:ACC_BINS]
    exact = _exact_points(inp, sigma, theta, edges)
    twin, used = D.veff_true(inp, sigma, theta, edges, PREF0, VOL)
    assert used == 1
    return cnt, exact, twin[0]


# the worst relative deviation of the binned rule over the bins of at least 50 sources, as measured (test docstring below)
ACC_MEASURED = 6.12e-2


def test_accuracy_of_the_binned_rule_against_30_digit_integrals():
    """On the seeded 3068-source 0.08-dex mock, one row at the truth, 25 bins (0.116 dex), K = 32: every bin's value by the rule
    against the per-source integrals between the bin edges at 30 digits (_exact_points).  Nothing can be fixed in advance: the
    posterior is binned as the rule's discrete measure, whose central nodes lie 0.045 dex apart here, so a source's bin masses
    are granular and the figure is what the sum over a bin's sources leaves of that.  Measured (mpmath is deterministic):
        bins of at least 50 sources (17): worst |rule - exact| / exact = 6.11e-2 (bin 3, 53 sources, at the faint end where the
            weights 1 / fc are heavy-tailed; 4.6e-2 and 4.1e-2 in the next two; at most 2.2e-2 from 200 sources on) - asserted
            at twice that;
        bins of 5 .. 49 sources (6): 3.46e-1, printed only;
        K = 32 at sigma = 0.09 against the wide class-0 table (48 nodes) on the same catalogue: 1.49e-1 over the bins of at
            least 50 sources, 4.13e-1 over those of 5 .. 49 - recorded in DESIGN.md section 3.26, not computed here."""
    cnt, exact, twin = _accuracy_case()
    dev = np.abs(twin - exact) / exact
    pop, few = cnt >= 50, (cnt >= 5) & (cnt < 50)
    print("binned rule against 30-digit integrals: worst relative deviation %.3e over the %d bins of >= 50 sources, %.3e over the "
          "%d bins of 5 .. 49 (not asserted)" % (dev[pop].max(), pop.sum(), dev[few].max(), few.sum()))
    for b in np.flatnonzero(cnt >= 5):
        print("  bin %2d: %4d sources, exact %.6e, rule %.6e, deviation %+.3e" % (b, cnt[b], exact[b], twin[b], twin[b] / exact[b] - 1.0))
    assert pop.sum() >= 10
    assert dev[pop].max() <= 2.0 * ACC_MEASURED
    # the reference's own quadrature error: every hundredth source, 12 nodes per panel against 24
    from test_lumpost_cpu import _calibration_case
    inp, sigma, theta, _ = _calibration_case()
    edges = veff.luminosity_bins(np.asarray(inp["lum"]), ACC_BINS)[0]
    some = list(range(0, len(sigma), 100))
    a, b = (_exact_points(inp, sigma, theta, edges, deg, some) for deg in (3, 4))
    assert np.all(np.abs(a - b) <= 1e-15 * b)


def test_model_surface_refuses_without_deconvolve():
    import lf_deconvlib as L
    o = L.fixcomp_model(synth.catalogue(300, seed=17))
    with pytest.raises(ValueError, match="deconvolve=True"):
        o.veff_deconvolved(device=False)
    o.close()


def test_c_abi_entries_and_constants():
    import os
    import re
    from lumfuncmcmc_amd import build, capi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "lfmcmc.h")).read()
    assert re.search(r"int lf_veff_true\(lf_ctx \*ctx, const double \*theta, int R, const double \*edges, int nbin, double pref0, "
                     r"double vol, int nq,\s+const double \*q, int method, double \*out, double \*values, int \*n_used\);", hdr)
    assert "int lf_veff_true_info(int *max_rows, int *max_bins);" in hdr and "int lf_veff_true_ms(double ms[3]);" in hdr
    assert "#define LF_ABI_VERSION 3" in hdr
    lib = capi.load()
    for name in ("lf_veff_true", "lf_veff_true_info", "lf_veff_true_ms"):
        assert name in capi.EXPORTS and hasattr(lib, name)
    info = capi.veff_true_info()
    src = open(os.path.join(root, "lumfuncmcmc_amd", "csrc", "lf_vefftrue.h")).read()
    assert "constexpr int VEFFT_ROWS = %d;" % info["row_group"] in src
    assert info["max_rows"] == 4096 and info["max_bins"] == 1024
    assert "lf_vefftrue.h" in " ".join(build.HEADERS)
