"""The integrated LF on the device (lf_lumfunc_integral_quantiles, lf_bands_integ in csrc/lf_bands.h, Gamma(a, x) of
csrc/lf_gammainc.h): the values against the NumPy twin, the quantiles bit for bit against np.percentile / np.median of the
device's own values, the special points, the unchanged differential kernel, the model classes' device paths, and Gamma(a, x),
10^t and the band sort over the entry's whole accepted domain (inputs of tests/lf_integlib.py)."""
import numpy as np
import pytest

import lf_integlib
from lf_testlib import synth
from lumfuncmcmc_amd import capi, lfbands, lfintegrals as li

pytestmark = pytest.mark.gpu

PIV = (1.2, 1.53, 1.86)
Q7 = (0.0, 2.5, 16.0, 50.0, 84.0, 97.5, 100.0)
KINDS = ("number", "lumdens")
# 4 x the twin's largest relative error against mpmath (3.0e-15, tests/test_integrals_cpu.py) + 1e-13 for the device
# library's exp / log / expm1 / pow, which differ from the C library's in the last bits.
TWIN_MAX_REL = 3.0e-15
VAL_RTOL = 4.0 * TWIN_MAX_REL + 1e-13
TINY = np.finfo(np.float64).tiny


def _bits_equal(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape
    gn, wn = np.isnan(got), np.isnan(want)
    np.testing.assert_array_equal(gn, wn)
    bad = got[~gn].view(np.int64) != want[~wn].view(np.int64)
    assert not bad.any(), (got[~gn][bad][:5], want[~wn][bad][:5])


def _values_close(dev, host, label=""):
    """VAL_RTOL; absolute 1e-300 where either side is subnormal or zero; inf / NaN / exact zeros in the same places."""
    np.testing.assert_array_equal(np.isnan(dev), np.isnan(host))
    np.testing.assert_array_equal(np.isinf(dev), np.isinf(host))
    np.testing.assert_array_equal(dev == 0.0, host == 0.0)
    fin = np.isfinite(dev) & np.isfinite(host)
    d, h = dev[fin], host[fin]
    small = (np.abs(d) < TINY) | (np.abs(h) < TINY)
    assert np.all(np.abs(d[small] - h[small]) <= 1e-300)
    rel = np.abs(d[~small] - h[~small]) / np.abs(h[~small])
    print("%s largest relative difference device - twin: %.3e over %d values" % (label, rel.max(initial=0.0), rel.size))
    assert rel.max(initial=0.0) <= VAL_RTOL


def _draws(variant, R, rng):
    """test_gpu_bands._draws with alpha spread over [-3, 1]."""
    if variant == "free":
        return np.column_stack([rng.normal(42.5, 0.3, R), rng.normal(-2.5, 0.4, R), rng.uniform(-3.0, 1.0, R)])
    rows = np.column_stack([rng.normal(42.5, 0.15, (R, 3)), rng.normal(-2.5, 0.15, (R, 3)), rng.uniform(-3.0, 1.0, R)])
    return lfbands.pack_draws("zevol", rows, pivots=PIV)


def _check_bitwise(variant, kind, draws, lmin, z, q=Q7):
    out, v = capi.lumfunc_integral_quantiles(variant, li.KINDS[kind], draws, lmin, z=z, q=q, values=True)
    with np.errstate(all="ignore"):
        _bits_equal(out, np.percentile(v, q, axis=0))
        med = capi.lumfunc_integral_quantiles(variant, li.KINDS[kind], draws, lmin, z=z, method=capi.LF_Q_MEDIAN)
        _bits_equal(med, np.median(v, axis=0)[None])
    return out, v


@pytest.mark.parametrize("variant", ["free", "zevol"])
@pytest.mark.parametrize("kind", KINDS)
def test_values_against_the_twin(variant, kind):
    rng = np.random.default_rng(1)
    R, P = 200, 257
    lmin = rng.uniform(39.0, 46.0, P)
    lmin[100] = -np.inf
    z = rng.uniform(1.1, 2.0, P) if variant == "zevol" else None
    draws = _draws(variant, R, rng)
    draws[7, -1], draws[150, -1] = -1.0, -2.0
    out, v = _check_bitwise(variant, kind, draws, lmin, z)
    host = li.integral_values(variant, kind, draws, lmin, z)
    _values_close(v, host, "%s %s:" % (variant, kind))
    assert np.isinf(v[:, 100]).any() and (v == 0.0).any()
    assert capi.lumfunc_integral_quantiles_ms() > 0.0


@pytest.mark.parametrize("R", [1, 2, 63, 64, 65, 200, 257, 4096])
@pytest.mark.parametrize("variant", ["free", "zevol"])
def test_every_draw_count_is_bitwise_numpy(R, variant):
    rng = np.random.default_rng(R)
    P = 129
    lmin = rng.uniform(40.5, 44.5, P)
    z = rng.uniform(1.1, 2.0, P) if variant == "zevol" else None
    _check_bitwise(variant, KINDS[R % 2], _draws(variant, R, rng), lmin, z)


def test_zeros_infinities_and_ties():
    rng = np.random.default_rng(9)
    base = np.array([[42.5, -2.5, -1.5], [42.5, -2.4, -1.0], [42.5, -2.7, -2.0], [42.5, -2.6, 0.5], [42.5, -2.5, -0.5]])
    draws = base[rng.integers(0, len(base), 300)]                          # with replacement: many duplicate rows
    lmin = np.concatenate([rng.uniform(41.0, 44.0, 50), [46.5, 46.5, 46.5], [-np.inf]])
    for kind in KINDS:
        out, v = _check_bitwise("free", kind, draws, lmin, None, q=(0.0, 16.0, 50.0, 84.0, 100.0))
        _values_close(v, li.integral_values("free", kind, draws, lmin), "special points, %s:" % kind)
        assert np.all(v[:, 50:53] == 0.0) and np.all(out[:, 50:53] == 0.0)      # logLmin - logL* = +4: exp(-10^4) = 0
        a = draws[:, 2] + 1.0 + li.KINDS[kind]
        np.testing.assert_array_equal(np.isinf(v[:, 53]), a <= 0.0)             # x = 0: +inf where alpha + 1 + kind <= 0
        assert np.isinf(v[:, 53]).any() and np.isfinite(v[:, 53]).any()
        assert np.isnan(out[-1, 53])                  # np.percentile(.., 100) with an inf maximum is NaN (inf - inf)
        assert len(np.unique(v[:, 0])) == len(base)   # ties: one value per distinct draw


@pytest.mark.parametrize("variant", ["free", "zevol"])
def test_the_differential_kernel_is_unchanged(variant):
    """test_gpu_bands.test_every_draw_count_is_bitwise_numpy's shape at R = 200, through the shared sort and quantile stages."""
    R = 200
    rng = np.random.default_rng(R)
    P = 129
    logL = rng.uniform(40.5, 44.5, P)
    z = rng.uniform(1.1, 2.0, P) if variant == "zevol" else None
    if variant == "free":
        draws = np.column_stack([rng.normal(42.5, 0.3, R), rng.normal(-2.5, 0.4, R), rng.normal(-1.5, 0.3, R)])
    else:
        rows = np.column_stack([rng.normal(42.5, 0.15, (R, 3)), rng.normal(-2.5, 0.15, (R, 3)), rng.normal(-1.5, 0.3, R)])
        draws = lfbands.pack_draws("zevol", rows, pivots=PIV)
    out, v = capi.lumfunc_quantiles(variant, draws, logL, z=z, q=Q7, values=True)
    with np.errstate(all="ignore"):
        _bits_equal(out, np.percentile(v, Q7, axis=0))
        _bits_equal(capi.lumfunc_quantiles(variant, draws, logL, z=z, method=capi.LF_Q_MEDIAN), np.median(v, axis=0)[None])
    np.testing.assert_allclose(v, lfbands.lf_values(variant, draws, logL, z), rtol=1e-12, atol=1e-300)


def test_model_device_path_agrees_with_the_host_path():
    from lumfuncmcmc_amd.model import LumFuncMCMC
    cat = synth.catalogue(5000, seed=7)
    fi = cat["field_ind"]
    m = LumFuncMCMC(synth.split_fields(cat["z"], fi), lum=synth.split_fields(cat["lum"], fi),
                    lum_e=synth.split_fields(cat["lum_e"], fi), Flim=list(synth.FLIM), alpha=synth.ALPHA_C,
                    Omega_0=list(synth.OMEGA_0), sch_al=synth.SCH_AL, sch_al_lims=synth.SCH_AL_LIMS, Lstar=synth.LSTAR,
                    Lstar_lims=synth.LSTAR_LIMS, phistar=synth.PHISTAR, phistar_lims=synth.PHISTAR_LIMS, Lc=synth.LC,
                    Lh=synth.LH, nwalkers=32, nsteps=10, min_comp_frac=0.0, field_ind=fi, Flim_lims=synth.FLIM_LIMS,
                    alpha_lims=synth.ALPHA_LIMS)
    rng = np.random.default_rng(7)
    th = np.column_stack([rng.normal(42.6, 0.05, 400), rng.normal(-2.1, 0.05, 400), rng.normal(-1.5, 0.05, 400)] +
                         [rng.normal(f, 0.1, 400) for f in synth.FLIM] + [rng.normal(synth.ALPHA_C, 0.1, 400)])
    m.samples = np.column_stack([th, rng.normal(-100.0, 3.0, 400)])
    lmin = np.linspace(40.0, 44.5, 33)
    for kind in KINDS:
        res = {}
        for dev in (False, True):
            np.random.seed(2024)
            res[dev] = m.lf_integrals(kind=kind, logLmin=lmin, device=dev)
        assert res[True].shape == (3, 33)
        _values_close(res[True], res[False], "LumFuncMCMC %s:" % kind)


def test_z_model_device_path_agrees_with_the_host_path():
    from lumfuncmcmc_amd.model import LumFuncMCMCz
    cat = synth.catalogue(5000, seed=5)
    fi = cat["field_ind"]
    np.random.seed(1)
    m = LumFuncMCMCz(synth.split_fields(cat["z"], fi), lum=synth.split_fields(cat["lum"], fi),
                     lum_e=synth.split_fields(cat["lum_e"], fi), Flim=list(synth.FLIM), alpha=synth.ALPHA_C,
                     Omega_0=list(synth.OMEGA_0), sch_al=synth.SCH_AL, nwalkers=32, nsteps=10, min_comp_frac=0.0, field_ind=fi)
    rng = np.random.default_rng(5)
    m.samples = np.column_stack([rng.normal(42.4, 0.05, (300, 3)), rng.normal(-2.3, 0.05, (300, 3)), rng.normal(-1.5, 0.05, 300),
                                 rng.normal(-50.0, 2.0, 300)])
    for kind in KINDS:
        res = {}
        for dev in (False, True):
            np.random.seed(77)
            res[dev] = m.lf_integrals(kind, device=dev)
        assert res[True].shape == (3, 100)
        _values_close(res[True], res[False], "LumFuncMCMCz %s:" % kind)


# ------------------------------------------------------------------- the entry's whole accepted domain (lf_integlib.py)
@pytest.mark.parametrize("kind", KINDS)
def test_gamma_over_the_whole_accepted_domain(kind):
    """Gamma(alpha + 1 + kind, gi_exp10(logLmin)) itself: draws with the prefactor 1 and logL* = 0, one per lattice order
    (a over [-5, 6] and [-4, 7]), at 88 limits from x = 0 over the subnormals, the overflow edge of x^-5, both neighbours of
    the switch and [512, 1490) to x = +inf; both template instances.  tests/test_integrals_cpu.py holds the twin to mpmath on
    the same domain and checks what these inputs reach."""
    lmin = lf_integlib.lattice_points()
    x = li.exp10(lmin)
    host = None
    for variant in ("free", "zevol"):
        draws, z = lf_integlib.lattice_draws(variant, kind)
        out, v = capi.lumfunc_integral_quantiles(variant, li.KINDS[kind], draws, lmin, z=z, q=Q7, values=True)
        if host is None:
            host = li.integral_values(variant, kind, draws, lmin, z)
            assert not np.isnan(host).any() and np.isinf(host).any() and (host == 0.0).any()
        else:
            np.testing.assert_array_equal(host, li.integral_values(variant, kind, draws, lmin, z))
        assert v.shape == host.shape == (draws.shape[0], lmin.size)
        with np.errstate(all="ignore"):
            _bits_equal(out, np.percentile(v, Q7, axis=0))
        fin = np.isfinite(v) & np.isfinite(host) & (np.abs(host) >= TINY) & (np.abs(v) >= TINY)
        with np.errstate(all="ignore"):
            rel = np.where(fin, np.abs(v - host) / np.abs(host), 0.0)
        for label, cols in lf_integlib.lattice_regions(x).items():
            assert cols.any()
            print("%s %s, x in %s: largest relative difference device - twin %.3e over %d values"
                  % (variant, kind, label, rel[:, cols].max(), fin[:, cols].sum()))
        assert not np.isnan(v).any()
        _values_close(v, host, "%s %s, whole domain:" % (variant, kind))


def test_exp10_bit_for_bit():
    """gi_exp10 against lfintegrals.exp10 through the entry: one "zevol" draw with logphi* = z and Gamma(1, 0) = 1, so that
    values[0][p] = gi_exp10(z_p) ("number"), or gi_exp10(z_p) gi_exp10(z_p / 2) ("lumdens", on 200 of the values)."""
    t = lf_integlib.exp10_lattice()
    for kind, tt in (("number", t), ("lumdens", np.concatenate([t[:193], t[-7:]]))):
        draws, lmin, z, want = lf_integlib.exp10_case(kind, tt)
        _, v = _check_bitwise("zevol", kind, draws, lmin, z, q=(50.0,))
        assert v.shape == (1, tt.size) and np.isinf(want).any() and (want == 0.0).any()
        _bits_equal(v[0], want)
        if kind == "number":
            assert ((want > 0.0) & (want < TINY)).any()
            _bits_equal(v[0], li.exp10(tt))


@pytest.mark.parametrize("R", lf_integlib.SORT_R)
def test_the_band_sort_on_ordered_inputs(R):
    """Ascending, descending, all equal, organ-pipe, two interleaved runs and "+inf first, rest ascending" columns at every
    draw count around the powers of two, through lf_bands_integ<7, 0> (values gi_exp10(t_r), bit for bit) and lf_bands<7>."""
    z = np.array([0.0, 1.0, 2.0])
    for name in lf_integlib.SORT_PATTERNS:
        tr = lf_integlib.sort_pattern(name, R)
        _, v = _check_bitwise("zevol", "number", lf_integlib.sort_draws(tr), np.full(3, -np.inf), z)
        _bits_equal(v, np.repeat(li.exp10(tr)[:, None], 3, axis=1))
        draws, logL = lf_integlib.sort_draws(tr, alpha=-1.5), np.array([-1.0, 0.0, 0.5])
        out, w = capi.lumfunc_quantiles("zevol", draws, logL, z=z, q=Q7, values=True)
        with np.errstate(all="ignore"):
            _bits_equal(out, np.percentile(w, Q7, axis=0))
            _bits_equal(capi.lumfunc_quantiles("zevol", draws, logL, z=z, method=capi.LF_Q_MEDIAN), np.median(w, axis=0)[None])
        assert w.shape == (R, 3) and not np.isnan(w).any()
        np.testing.assert_array_equal(np.argsort(w[:, 1], kind="stable"), np.argsort(v[:, 1], kind="stable"))    # the same order
