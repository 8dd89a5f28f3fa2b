"""The integrated LF without a GPU (lfintegrals): the NumPy twin of Gamma(a, x) against mpmath at
40 digits, the normalisation against a quadrature of the package's own LF, the quantile statement, the argument checks
of the C entry (made before the device is touched) and the model classes' host paths."""
import mpmath as mp
import numpy as np
import pytest

import lf_integlib
from lf_testlib import synth
from lumfuncmcmc_amd import capi, hostsetup as hs, lfbands, lfintegrals as li

# Largest relative error of the twin over the lattice below, measured on the CPU: 3.0e-15 (at
# x just below the switch, where the series' difference loses most).  The tests assert twice that.
TWIN_MAX_REL = 3.0e-15
TINY = np.finfo(np.float64).tiny
DMAX = np.finfo(np.float64).max


def _lattice():
    """270 orders less their duplicates and 91 arguments (lf_integlib): the whole accepted domain of the order, and every
    scale of x from the smallest subnormal to past the last x whose exp(-x / 2) is not 0."""
    return lf_integlib.orders(), lf_integlib.arguments()


@pytest.fixture(scope="module")
def lattice():
    mp.mp.dps = 40
    a, x = _lattice()
    truth = [[(mp.gamma(float(ai)) if ai > 0 else mp.inf) if xi == 0.0 else mp.gammainc(mp.mpf(float(ai)), mp.mpf(float(xi)), mp.inf)
              for xi in x] for ai in a]
    aa, xx = np.meshgrid(a, x, indexing="ij")
    got, counts = li.gammainc_upper(aa, xx, counts=True)
    return a, x, truth, got, counts


def test_twin_against_mpmath_on_the_lattice(lattice):
    """Truth at the doubles the twin received.  A truth above the largest double must come out +inf, nothing inside the
    domain is NaN, and below the smallest normal double the absolute bound holds.  Before the bracket took x^a0 - 1 for
    |a0 ln x| > 1 and the downward recurrence its scale and its +inf, this lattice gave NaN at 1384 points (a = -5, x = 1e-100
    among them: inf - inf one step after x^(c-1) e^-x overflowed), +inf for a truth of 0.65 of the largest double at
    a = -4.4102, x = 1e-70, and 4.4e-14 at a = -0.461, x = 4.9e-324."""
    a, x, truth, got, _ = lattice
    worst = (0.0, None, None)
    region = {}
    nan = [(ai, xj) for i, ai in enumerate(a) for j, xj in enumerate(x) if np.isnan(got[i, j])]
    assert not nan, (len(nan), nan[:5])
    for i, ai in enumerate(a):
        for j, xj in enumerate(x):
            t, g = truth[i][j], got[i, j]
            if t > DMAX:
                assert g == np.inf, (ai, xj, g)
            elif abs(t) < TINY:
                assert abs(g - float(t)) <= 1e-300, (ai, xj, g)
            else:
                assert np.isfinite(g), (ai, xj, g, float(t / DMAX))
                rel = float(abs((mp.mpf(float(g)) - t) / t))
                if rel > worst[0]:
                    worst = (rel, ai, xj)
                key = "x < 1e-6" if xj < 1e-6 else "[1e-6, 1)" if xj < 1.0 else "[1, 512)" if xj < 512.0 else "[512, 1490)"
                region[key] = max(region.get(key, 0.0), rel)
    print("largest relative error of the twin: %.3e at a = %r, x = %r" % worst)
    print("by region: " + ", ".join("%s %.2e" % kv for kv in region.items()))
    assert worst[0] <= 2.0 * TWIN_MAX_REL, worst


def test_no_loop_reaches_its_cap_on_the_lattice(lattice):
    nser, ncf, nrec = lattice[4]
    print("most trips: series %d, continued fraction %d, recurrence %d" % (nser.max(), ncf.max(), nrec.max()))
    assert nser.max() < li.GI_SER_CAP
    assert ncf.max() < li.GI_CF_CAP
    assert nrec.max() <= li.GI_REC_CAP                     # a counted loop: 6 steps at a = 7 exactly


def test_special_values_and_everything_outside_the_domain():
    g = li.gammainc_upper
    assert g(1.0, 0.0) == 1.0 and g(3.0, 0.0) == 2.0 and g(0.5, 0.0) == pytest.approx(np.sqrt(np.pi), rel=1e-15)
    assert g(0.0, 0.0) == np.inf and g(-1.0, 0.0) == np.inf and g(-2.5, 0.0) == np.inf
    assert g(2.0, np.inf) == 0.0 and g(-3.0, 1e6) == 0.0 and g(6.0, 1e4) == 0.0
    sub = g(1.0, 740.0)
    assert 0.0 < sub < TINY
    for a, x in ((np.nan, 1.0), (1.0, np.nan), (1.0, -1e-300), (-5.000001, 1.0), (7.000001, 1.0), (np.inf, 1.0), (1.0, -np.inf)):
        assert np.isnan(g(a, x)), (a, x)
    assert g(1.0, 0.25) == pytest.approx(np.exp(-0.25), rel=1e-15)


def test_exp10_of_the_twin():
    mp.mp.dps = 40
    t = np.concatenate([np.random.default_rng(4).uniform(-7.0, 7.0, 2000), np.random.default_rng(5).uniform(-307.0, 308.0, 500)])
    v = li.exp10(t)
    rel = max(float(abs(mp.mpf(float(vi)) / mp.power(10, mp.mpf(float(ti))) - 1)) for vi, ti in zip(v, t))
    assert rel <= 2.0 ** -52                               # one ulp at the most
    np.testing.assert_array_equal(li.exp10(np.array([-np.inf, -331.0, 0.0, 1.0, 309.0, np.inf])), [0.0, 0.0, 1.0, 10.0, np.inf, np.inf])
    assert np.isnan(li.exp10(np.nan))
    # the lattice the device is held to bit for bit (lf_integlib.exp10_lattice: down to -330, and the edges): one ulp where
    # the truth is a normal number, one spacing of the subnormals (ldexp rounds once more there) below, +inf above
    t = lf_integlib.exp10_lattice()
    v = li.exp10(t)
    sub = 0
    for vi, ti in zip(v, t):
        truth = mp.power(10, mp.mpf(float(ti)))
        if truth > DMAX:
            assert vi == np.inf, (ti, vi)
        elif truth < TINY:
            sub += 1
            assert abs(mp.mpf(float(vi)) - truth) <= mp.mpf(2) ** -1074, (ti, vi)
        else:
            assert abs(mp.mpf(float(vi)) / truth - 1) <= 2.0 ** -52, (ti, vi)
    assert sub >= 5 and np.isinf(v).any() and (v == 0.0).sum() >= 2        # each of the three rules met something
    e = dict(zip(lf_integlib.EXP10_EDGES, li.exp10(np.array(lf_integlib.EXP10_EDGES))))
    assert e[-331.0] == 0.0 and e[-330.0] == 0.0 and e[-323.3] == 5e-324 and 0.0 < e[-307.7] < TINY and e[0.0] == 1.0
    assert TINY < e[308.25] < np.inf and e[309.0] == np.inf


def test_the_device_lattice_holds_what_it_claims():
    """tests/test_gpu_integrals.py runs lf_integlib's orders and points through the entry; here, that they reach every
    branch, edge and recurrence depth of Gamma(a, x), and that the draws give the prefactor 1 and logLmin - logL* = logLmin."""
    t = lf_integlib.lattice_points()
    x = li.exp10(t)
    assert not np.isnan(t).any() and t.size <= 100
    one = 1.0
    assert (x == 0.0).sum() >= 3 and (x == one).any() and (x == np.nextafter(one, 0.0)).any() and (x == np.nextafter(one, 2.0)).any()
    assert ((x > 0.0) & (x < TINY)).sum() >= 3 and (x == 5e-324).any()
    assert ((x >= 512.0) & (x < 745.0)).any() and ((x >= 745.0) & (x < 1490.0)).any()
    with np.errstate(all="ignore"):
        assert ((np.exp(-0.5 * x) == 0.0) & np.isfinite(x)).any() and np.isinf(x).any()
    assert ((x > 0.0) & (x < 1e-6)).sum() >= 30 and (x == li.exp10(-62.0)).any() and (x == li.exp10(-63.0)).any()
    up, down = set(), set()
    for kind, k in li.KINDS.items():
        al = lf_integlib.lattice_alpha(kind)
        assert al.min() == li.ALPHA_MIN and al.max() == li.ALPHA_MAX
        a = al + 1.0 + k
        assert a.min() == li.GI_A_MIN + k and a.max() == li.GI_A_MAX - 1 + k
        aa, xx = np.meshgrid(a, x, indexing="ij")
        v, (nser, ncf, nrec) = li.gammainc_upper(aa, xx, counts=True)
        assert not np.isnan(v).any()
        m = np.rint(aa)
        for b, branch in ((1, nser > 0), (2, ncf > 0)):    # the series (0 < x < 1) and the continued fraction (x >= 1)
            up |= set(10 * b + int(d) for d in np.unique(nrec[branch & (m >= 1)]))
        down |= set(int(d) for d in np.unique(nrec[(nser > 0) & (m <= 0)]))
        for variant in ("free", "zevol"):
            draws, z = lf_integlib.lattice_draws(variant, kind)
            np.testing.assert_array_equal(li.integral_values(variant, kind, draws, t, z), v)
    # upward 1 .. 6 steps (m = 2 .. 7) below and above the switch; downward 1 .. 5: m = -5 is the lowest order the domain has
    # (GI_REC_CAP = 6 is the upward side's)
    assert up >= set(10 * b + d for b in (1, 2) for d in range(1, 7)), up
    assert down >= set(range(1, 6)), down


def test_the_exp10_and_sort_inputs_are_what_they_claim():
    """The one-draw "zevol" call of lf_integlib.exp10_case returns exp10(t_p) (logphi* = 0 (z z) + 1 z + 0 = z exactly,
    Gamma(1, 0) = 1 exactly), and the columns of lf_integlib.sort_draws are exp10(t_r) in the order of the pattern."""
    t = lf_integlib.exp10_lattice()
    assert t.size == 2507
    for kind, tt in (("number", t), ("lumdens", np.concatenate([t[:193], t[-7:]]))):
        draws, lmin, z, want = lf_integlib.exp10_case(kind, tt)
        d = draws[0]
        np.testing.assert_array_equal(d[3] * z ** 2 + d[4] * z + d[5], tt)
        assert li.gammainc_upper(d[6] + 1.0 + li.KINDS[kind], 0.0) == 1.0
        v = li.integral_values("zevol", kind, draws, lmin, z)
        np.testing.assert_array_equal(v[0], want)
        if kind == "number":
            np.testing.assert_array_equal(v[0], li.exp10(tt))
    for R in lf_integlib.SORT_R:
        asc = li.exp10(lf_integlib.sort_pattern("ascending", R))
        assert np.all(np.diff(asc) > 0.0)
        for name in lf_integlib.SORT_PATTERNS:
            tr = lf_integlib.sort_pattern(name, R)
            assert tr.shape == (R,)
            v = li.integral_values("zevol", "number", lf_integlib.sort_draws(tr), np.full(3, -np.inf), np.array([0.0, 1.0, 2.0]))
            np.testing.assert_array_equal(v, np.repeat(li.exp10(tr)[:, None], 3, axis=1))
            col = v[:, 0]
            if name == "descending":
                assert np.all(np.diff(col) < 0.0)
            elif name == "equal":
                assert np.all(col == col[0])
            elif name == "inf first":
                assert col[0] == np.inf and np.all(np.diff(col[1:]) > 0.0)
            elif name == "organ-pipe" and R >= 3:
                k = int(np.argmax(col))
                assert np.all(np.diff(col[:k + 1]) > 0.0) and np.all(np.diff(col[k:]) < 0.0)
            elif name == "two runs" and R >= 4:
                assert np.all(np.diff(col[0::2]) > 0.0) and np.all(np.diff(col[1::2]) > 0.0) and col[1] > col[2]


@pytest.mark.parametrize("kind", ["number", "lumdens"])
@pytest.mark.parametrize("alpha", [-2.5, -2.0, -1.6, -1.0, 0.5])
@pytest.mark.parametrize("off", [-2.0, 0.0, 1.0])
def test_the_definition_against_a_quadrature_of_true_lum_func(kind, alpha, off):
    from scipy.integrate import quad
    lstar, lphi = 42.5, -2.5
    lmin = lstar + off
    if kind == "number":
        f = lambda t: float(hs.true_lum_func(t, alpha, lstar, lphi))
    else:
        f = lambda t: float(10.0 ** t * hs.true_lum_func(t, alpha, lstar, lphi))
    hi = lstar + 3.0
    if lmin < lstar:
        want = quad(f, lmin, lstar, epsabs=0, epsrel=1e-12, limit=200)[0] + quad(f, lstar, hi, epsabs=0, epsrel=1e-12, limit=200)[0]
    else:
        want = quad(f, lmin, hi, epsabs=0, epsrel=1e-12, limit=200, points=[lstar] if lmin < lstar < hi else None)[0]
    got = li.integral_values("free", kind, [[lstar, lphi, alpha]], [lmin])[0, 0]
    assert got == pytest.approx(want, rel=1e-9)


def _draws(variant, R, rng):
    if variant == "free":
        return np.column_stack([rng.normal(42.5, 0.3, R), rng.normal(-2.5, 0.4, R), rng.uniform(-3.0, 1.0, R)])
    rows = np.column_stack([rng.normal(42.5, 0.15, (R, 3)), rng.normal(-2.5, 0.15, (R, 3)), rng.uniform(-3.0, 1.0, R)])
    return lfbands.pack_draws("zevol", rows, pivots=(1.2, 1.53, 1.86))


@pytest.mark.parametrize("variant", ["free", "zevol"])
@pytest.mark.parametrize("kind", ["number", "lumdens"])
@pytest.mark.parametrize("method", ["linear", "median"])
def test_quantiles_host_is_numpy_on_integral_values(variant, kind, method):
    rng = np.random.default_rng(3)
    R, P = 37, 400
    lmin = rng.uniform(39.0, 46.0, P)
    lmin[5] = -np.inf
    z = rng.uniform(1.1, 2.0, P) if variant == "zevol" else None
    draws = _draws(variant, R, rng)
    q = (2.5, 16, 50, 84, 97.5)
    v = li.integral_values(variant, kind, draws, lmin, z)
    assert v.shape == (R, P)
    with np.errstate(all="ignore"):
        want = np.percentile(v, q, axis=0) if method == "linear" else np.median(v, axis=0)[None]
    for chunk in (None, 97):
        got = li.quantiles_host(variant, kind, draws, lmin, z=z, q=q, method=method, chunk=chunk)
        assert got.shape == want.shape
        np.testing.assert_array_equal(got, want)


def test_host_statement_refuses_what_the_entry_refuses():
    d = np.array([[42.5, -2.5, -1.5]])
    with pytest.raises(ValueError):
        li.quantiles_host("free", "volume", d, [42.0])
    with pytest.raises(ValueError):
        li.quantiles_host("free", "number", [[42.5, -2.5, 5.5]], [42.0])
    with pytest.raises(ValueError):
        li.quantiles_host("free", "number", d, [np.nan])
    with pytest.raises(ValueError):
        li.quantiles_host("free", "number", d, [42.0], method="nearest")


# ------------------------------------------------------------------------------------------------ the C entry's checks
@pytest.fixture(scope="module")
def lib():
    from lumfuncmcmc_amd import build
    build.build_library(verbose=False)
    return capi.load()


def test_the_entries_are_exported(lib):
    for name in ("lf_lumfunc_integral_quantiles", "lf_lumfunc_integral_quantiles_ms"):
        assert hasattr(lib, name) and name in capi.EXPORTS
    assert (capi.LF_INT_NUMBER, capi.LF_INT_LUMDENS) == (0, 1)
    assert li.KINDS == {"number": capi.LF_INT_NUMBER, "lumdens": capi.LF_INT_LUMDENS}


def _call(lib, variant=0, kind=0, R=4, P=8, draws=True, logL=True, z=False, nq=1, q=(50.0,), method=0, out=True, alpha=-1.5,
          lmin=42.0):
    p = capi._ptr
    d = np.zeros((max(R, 1), 7 if variant == 2 else 3))
    d[:, -1] = -1.5
    d[-1, -1] = alpha
    L = np.full(max(P, 1), 42.0)
    L[-1] = lmin
    qa = np.array(q, dtype=np.float64) if q is not None else None
    o = np.zeros(max(nq, 1) * max(P, 1))
    return lib.lf_lumfunc_integral_quantiles(0, variant, kind, R, p(d) if draws else None, P, p(L) if logL else None,
                                             p(L) if z else None, nq, p(qa) if qa is not None else None, method,
                                             p(o) if out else None, None)


@pytest.mark.parametrize("kw", [
    dict(kind=2), dict(kind=-1),
    dict(alpha=float("nan")), dict(alpha=float("inf")), dict(alpha=-6.000001), dict(alpha=5.000001), dict(variant=2, z=True, alpha=7.0),
    dict(lmin=float("nan")),
    dict(R=0), dict(R=4097), dict(R=-1),
    dict(nq=0, q=()), dict(nq=33, q=tuple(range(33))),
    dict(q=(-1e-9,)), dict(q=(100.0000001,)), dict(q=(float("nan"),)), dict(nq=2, q=(50.0, float("nan"))),
    dict(draws=False), dict(logL=False), dict(out=False), dict(q=None), dict(variant=2, z=False),
    dict(variant=3), dict(variant=-1), dict(method=2), dict(method=-1),
    dict(method=1, nq=2, q=(50.0, 50.0)), dict(method=1, nq=0, q=None),
    dict(P=0), dict(P=-5),
])
def test_bad_arguments_are_refused_before_the_device_is_touched(lib, kw):
    assert _call(lib, **kw) == capi.LF_ERR_ARG


def test_wrapper_raises_lferror(lib):
    with pytest.raises(capi.LFError):
        capi.lumfunc_integral_quantiles("free", 2, np.array([[42.5, -2.5, -1.5]]), np.array([42.0]))
    with pytest.raises(capi.LFError):
        capi.lumfunc_integral_quantiles("free", 0, np.array([[42.5, -2.5, np.nan]]), np.array([42.0]))


# ------------------------------------------------------------------------------------------------------------ the models
def _model(fix_sch_al=False, sch_al=synth.SCH_AL):
    from lumfuncmcmc_amd.model import LumFuncMCMC
    cat = synth.catalogue(1500, seed=7)
    fi = cat["field_ind"]
    m = LumFuncMCMC(synth.split_fields(cat["z"], fi), lum=synth.split_fields(cat["lum"], fi),
                    lum_e=synth.split_fields(cat["lum_e"], fi), Flim=list(synth.FLIM), alpha=synth.ALPHA_C,
                    Omega_0=list(synth.OMEGA_0), sch_al=sch_al, sch_al_lims=synth.SCH_AL_LIMS, Lstar=synth.LSTAR,
                    Lstar_lims=synth.LSTAR_LIMS, phistar=synth.PHISTAR, phistar_lims=synth.PHISTAR_LIMS, Lc=synth.LC,
                    Lh=synth.LH, nwalkers=32, nsteps=10, min_comp_frac=0.0, field_ind=fi, Flim_lims=synth.FLIM_LIMS,
                    alpha_lims=synth.ALPHA_LIMS, fix_sch_al=fix_sch_al)
    rng = np.random.default_rng(7)
    th = np.column_stack([rng.normal(42.6, 0.05, 600), rng.normal(-2.1, 0.05, 600)] +
                         ([] if fix_sch_al else [rng.normal(-1.5, 0.05, 600)]) +
                         [rng.normal(f, 0.1, 600) for f in synth.FLIM] + [rng.normal(synth.ALPHA_C, 0.1, 600)])
    m.samples = np.column_stack([th, rng.normal(-100.0, 3.0, 600)])
    return m


@pytest.mark.parametrize("kind", ["number", "lumdens"])
def test_lf_integrals_shapes_draws_and_monotony(kind):
    m = _model()
    np.random.seed(5)
    one = m.lf_integrals(kind=kind, ndraws=40, device=False)
    assert one.shape == (3, 1) and np.all(one[0] <= one[1]) and np.all(one[1] <= one[2]) and np.all(one > 0.0)
    state = np.random.get_state()
    np.random.seed(5)
    m.lf_percentiles(logL=[42.0], ndraws=40, device=False)            # the same draws, the same use of numpy's stream
    np.testing.assert_array_equal(state[1], np.random.get_state()[1])
    np.random.seed(5)
    lmin = np.linspace(40.0, 45.0, 41)
    out = m.lf_integrals(kind=kind, logLmin=lmin, percentiles=(16, 50, 84), ndraws=40, device=False)
    assert out.shape == (3, 41)
    assert np.all(np.diff(out, axis=1) <= 0.0)
    with pytest.raises(ValueError):
        m.lf_integrals(kind="volume", device=False)
    assert m.lf_integrals(kind=kind, method="median", ndraws=11, device=False).shape == (1, 1)


def test_lf_integrals_with_alpha_fixed_at_minus_one():
    m = _model(fix_sch_al=True, sch_al=-1.0)
    np.random.seed(1)
    out = m.lf_integrals(kind="number", logLmin=[41.0, 42.0, -np.inf], ndraws=30, device=False)
    assert out.shape == (3, 3) and np.all(np.isfinite(out[:, :2])) and np.all(out[:, 0] > out[:, 1])
    assert not np.isfinite(out[:, 2]).any()                    # Gamma(0, 0) = +inf in every draw: inf, or NaN by numpy's lerp
    np.random.seed(1)
    rho = m.lf_integrals(kind="lumdens", logLmin=[-np.inf], ndraws=30, device=False)
    assert np.all(np.isfinite(rho)) and np.all(rho > 0.0)      # Gamma(1, 0) = 1: rho_tot = phi* L*


def test_z_model_lf_integrals():
    from lumfuncmcmc_amd.model import LumFuncMCMCz
    cat = synth.catalogue(1500, seed=5)
    fi = cat["field_ind"]
    np.random.seed(1)
    m = LumFuncMCMCz(synth.split_fields(cat["z"], fi), lum=synth.split_fields(cat["lum"], fi),
                     lum_e=synth.split_fields(cat["lum_e"], fi), Flim=list(synth.FLIM), alpha=synth.ALPHA_C,
                     Omega_0=list(synth.OMEGA_0), sch_al=synth.SCH_AL, nwalkers=32, nsteps=10, min_comp_frac=0.0, field_ind=fi)
    rng = np.random.default_rng(5)
    m.samples = np.column_stack([rng.normal(42.4, 0.05, (300, 3)), rng.normal(-2.3, 0.05, (300, 3)), rng.normal(-1.5, 0.05, 300),
                                 rng.normal(-50.0, 2.0, 300)])
    for kind in ("number", "lumdens"):
        np.random.seed(77)
        out = m.lf_integrals(kind, device=False)
        assert out.shape == (3, 100) and np.all(out[0] <= out[1]) and np.all(out[1] <= out[2]) and np.all(out > 0.0)
        zz = np.full(30, 1.5)
        np.random.seed(77)
        out = m.lf_integrals(kind, logLmin=np.linspace(40.0, 45.0, 30), z=zz, ndraws=50, device=False)
        assert out.shape == (3, 30) and np.all(np.diff(out, axis=1) <= 0.0)
        np.random.seed(77)
        assert m.lf_integrals(kind, logLmin=41.5, z=[1.3, 1.6], ndraws=20, device=False).shape == (3, 2)
