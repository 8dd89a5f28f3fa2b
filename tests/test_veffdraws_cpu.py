"""The 1/Veff LF marginalised over the completeness posterior, without a GPU: the NumPy twin of
lf_veff_draws (veff.veff_draws) against lumfunc_weights + boot_err_log, its percentiles, the draws and the median row of
LumFuncMCMC.veff_percentiles, and the argument checks of the C entry (made before the device is touched)."""
import ctypes

import numpy as np
import pytest

from lf_testlib import synth
from lumfuncmcmc_amd import capi, hostsetup as hs, veff


def _model(n, seed=7, **kw):
    from lumfuncmcmc_amd.model import LumFuncMCMC
    cat = synth.catalogue(n, seed=seed)
    fi = cat["field_ind"]
    args = dict(Flim=list(synth.FLIM), alpha=synth.ALPHA_C, Omega_0=list(synth.OMEGA_0), sch_al=synth.SCH_AL,
                sch_al_lims=synth.SCH_AL_LIMS, Lstar=synth.LSTAR, Lstar_lims=synth.LSTAR_LIMS, phistar=synth.PHISTAR,
                phistar_lims=synth.PHISTAR_LIMS, Lc=synth.LC, Lh=synth.LH, nwalkers=32, nsteps=10, min_comp_frac=0.0, field_ind=fi,
                Flim_lims=synth.FLIM_LIMS, alpha_lims=synth.ALPHA_LIMS, nboot=20, nbins=25)
    args.update(kw)
    m = LumFuncMCMC(synth.split_fields(cat["z"], fi), lum=synth.split_fields(cat["lum"], fi),
                    lum_e=synth.split_fields(cat["lum_e"], fi), **args)
    rng = np.random.default_rng(seed)
    th = np.column_stack([rng.normal(42.6, 0.05, 400), rng.normal(-2.1, 0.05, 400)] +
                         ([] if args.get("fix_sch_al") else [rng.normal(-1.5, 0.05, 400)]) +
                         [rng.normal(f, 0.1, 400) for f in synth.FLIM] + [rng.normal(synth.ALPHA_C, 0.1, 400)])
    m.samples = np.column_stack([th, rng.normal(-100.0, 3.0, 400)])
    return m


def _field(m):
    return np.repeat(np.arange(m.nfields), np.diff(m.field_ind))


@pytest.mark.parametrize("mcf", [0.0, 0.5])
@pytest.mark.parametrize("fcmin", [0.1, 0.0])
def test_one_draw_is_lumfunc_weights_and_the_bincount_of_boot_err_log_bit_for_bit(mcf, fcmin):
    from lumfuncmcmc_amd.cosmology import cosmo
    m = _model(1500, fcmin=fcmin, min_comp_frac=mcf)
    m.getFlim()
    if mcf <= 0.001:
        zmaxval = m.zmax
    else:
        zmaxval = np.minimum(m.zmax, veff.max_redshift(10 ** m.lum, m.rootsf.ev(m.Flims_arr, m.alpha), cosmo))
        assert (zmaxval <= m.zmin).any() or (zmaxval < m.zmax).any()
    phi = veff.lumfunc_weights(m.flux, m.dVdzf, sum(m.Omega_0), m.zmin, zmaxval, 1.0e-17 * m.Flims_arr, m.alpha, m.fcmin)
    _, lfbinorig, _ = veff.boot_err_log(m.lum, phi, nboot=2, nbin=m.nbins)
    _, _, dL, idx = veff.luminosity_bins(m.lum, m.nbins)
    draw = np.array(list(1.0e-17 * np.array(m.Flim)) + [m.alpha])
    vol = veff.comoving_volume(m.dVdzf, m.zmin, zmaxval)
    got = veff.veff_draws(m.flux, _field(m), vol, sum(m.Omega_0) / hs.SQARCSEC, m.fcmin, idx, m.nbins, draw[None])
    assert got.shape == (1, m.nbins)
    np.testing.assert_array_equal(got[0] / dL, lfbinorig)
    assert (lfbinorig > 0).any()


@pytest.mark.parametrize("method", ["linear", "median"])
def test_the_twins_percentiles_are_numpys_of_its_values(method):
    rng = np.random.default_rng(2)
    n, nf, nbin, R = 700, 3, 9, 37
    flux = rng.uniform(2e-17, 9e-17, n)
    field = rng.integers(0, nf, n)
    bin_of = rng.integers(-1, nbin + 1, n)
    vol = rng.uniform(1e5, 1e6, n)
    vol[::50] = 0.0
    draws = np.column_stack([rng.uniform(2e-17, 4e-17, (R, nf)), rng.uniform(3.0, 6.0, R)])
    q = (0, 2.5, 16, 50, 84, 100)
    out, values = veff.veff_draws_quantiles(flux, field, vol, 0.04, 0.1, bin_of, nbin, draws, q=q, method=method, device=False)
    np.testing.assert_array_equal(values, veff.veff_draws(flux, field, vol, 0.04, 0.1, bin_of, nbin, draws))
    want = np.percentile(values, q, axis=0) if method == "linear" else np.median(values, axis=0)[None]
    np.testing.assert_array_equal(out, want)
    # the sources outside [0, nbin) and the ones without a volume count nowhere
    keep = (bin_of >= 0) & (bin_of < nbin) & (vol > 0)
    one = veff.veff_draws(flux[keep], field[keep], vol[keep], 0.04, 0.1, bin_of[keep], nbin, draws[:1])
    np.testing.assert_array_equal(one, values[:1])
    with pytest.raises(ValueError):
        veff.veff_draws_quantiles(flux, field, vol, 0.04, 0.1, bin_of, nbin, draws, method="nearest")


@pytest.mark.parametrize("fix_sch_al", [False, True])
def test_veff_percentiles_draws_the_rows_lf_percentiles_draws(fix_sch_al):
    m = _model(5000, fix_sch_al=fix_sch_al)
    R = 31
    np.random.seed(3)
    res = m.veff_percentiles(ndraws=R, device=False)
    state = np.random.get_state()
    np.random.seed(3)
    m.lf_percentiles(ndraws=R, logL=np.array([42.0]), device=False)
    want = np.random.get_state()
    assert state[0] == want[0] and state[2:] == want[2:]
    np.testing.assert_array_equal(state[1], want[1])
    # ... and reads Flim (x 1e-17) and alpha out of them through theta's layout
    np.random.seed(3)
    rows = m._posterior_rows(R, 7.5)
    k = 2 if fix_sch_al else 3
    draws = np.column_stack([1.0e-17 * rows[:, k:k + 5], rows[:, k + 5]])
    _, Lavg, dL, idx = veff.luminosity_bins(m.lum, m.nbins)
    vol = veff.comoving_volume(m.dVdzf, m.zmin, m.zmax)
    values = veff.veff_draws(m.flux, _field(m), vol, sum(m.Omega_0) / hs.SQARCSEC, m.fcmin, idx, m.nbins, draws) / dL
    assert res["values"].shape == (R, m.nbins) and res["percentiles"].shape == (3, m.nbins)
    np.testing.assert_array_equal(res["values"], values)
    np.testing.assert_array_equal(res["Lavg"], Lavg)
    np.testing.assert_array_equal(res["var_comp"], np.var(values, axis=0, ddof=1))
    np.testing.assert_allclose(res["percentiles"], np.percentile(values, (16, 50, 84), axis=0), rtol=1e-15)
    assert np.all(res["percentiles"][0] <= res["percentiles"][1]) and np.all(res["percentiles"][1] <= res["percentiles"][2])
    assert (res["var_comp"] > 0).any()
    med = m.veff_percentiles(ndraws=R, method="median", device=False)
    assert med["percentiles"].shape == (1, m.nbins)


def test_the_row_of_the_median_parameters_reproduces_lfbinorig():
    m = _model(5000)
    np.random.seed(12)
    m.set_median_fit()                          # host: the median Flim and alpha, then VeffLF at them
    lfbinorig, var, Flim, alpha = m.lfbinorig.copy(), m.var.copy(), list(m.Flim), m.alpha
    row = np.array([m.Lstar, m.phistar, m.sch_al] + Flim + [alpha, -90.0])
    m.samples = np.tile(row, (8, 1))            # a posterior that is the median row alone
    res = m.veff_percentiles(ndraws=5, device=False)
    assert (lfbinorig > 0).any()
    for r in range(5):
        np.testing.assert_allclose(res["values"][r], lfbinorig, rtol=1e-14, atol=0)
    np.testing.assert_allclose(res["percentiles"][1], lfbinorig, rtol=1e-14, atol=0)
    np.testing.assert_array_equal(res["Lavg"], m.Lavg)
    assert np.all(res["var_comp"] <= (1e-15 * lfbinorig) ** 2)     # identical rows: the rounding of their mean, no more
    np.testing.assert_array_equal(m.var, var)                  # the method leaves the object's estimate alone
    assert list(m.Flim) == Flim and m.alpha == alpha


def test_fixed_completeness_has_nothing_to_marginalise_over():
    m = _model(600, fix_comp=True)
    with pytest.raises(ValueError):
        m.veff_percentiles(device=False)
    from lumfuncmcmc_amd.model import LumFuncMCMCz
    assert not hasattr(LumFuncMCMCz, "veff_percentiles")


# ------------------------------------------------------------------------------------------------ the C entry's checks
@pytest.fixture(scope="module")
def lib():
    from lumfuncmcmc_amd import build
    build.build_library(verbose=False)
    return capi.load()


def test_the_entries_are_exported_and_the_abi_is_version_3(lib):
    assert lib.lf_abi_version() == 3 == capi.LF_ABI_VERSION
    for name in ("lf_veff_draws", "lf_veff_draws_ms", "lf_veff_draws_chunk"):
        assert hasattr(lib, name) and name in capi.EXPORTS
    assert capi.veff_draws_chunk() >= 1
    assert lib.lf_veff_draws_ms(None) == capi.LF_ERR_ARG


def _call(lib, n=6, nbin=4, nf=2, R=3, nq=1, q=(50.0,), method=0, pref0=0.04, flux=True, field=True, bin_of=True, draws=True, out=True,
          field_vals=None, draw_vals=None):
    p = capi._ptr
    ip = ctypes.POINTER(ctypes.c_int32)
    nn, nb, f, r = max(n, 1), max(nbin, 1), max(nf, 1), max(R, 1)
    fx = np.full(nn, 3e-17)
    fl = np.zeros(nn, dtype=np.int32) if field_vals is None else np.asarray(field_vals, dtype=np.int32)
    bo = np.zeros(nn, dtype=np.int32)
    d = np.tile(np.array([2.7e-17] * f + [4.5]), (r, 1)) if draw_vals is None else np.asarray(draw_vals, dtype=np.float64)
    qa = np.array(q, dtype=np.float64) if q is not None else None
    o = np.zeros(max(nq, 1) * nb)
    return lib.lf_veff_draws(0, n, p(fx) if flux else None, fl.ctypes.data_as(ip) if field else None, None, 1.0e6, pref0, 0.1,
                             bo.ctypes.data_as(ip) if bin_of else None, nbin, nf, R, p(d) if draws else None, nq,
                             p(qa) if qa is not None else None, method, p(o) if out else None, None)


def _bad_draw(f, col, val):
    d = np.tile(np.array([2.7e-17] * f + [4.5]), (3, 1))
    d[1, col] = val
    return d


@pytest.mark.parametrize("kw", [
    dict(flux=False), dict(field=False), dict(bin_of=False), dict(draws=False), dict(out=False), dict(q=None),
    dict(n=0), dict(n=-3),
    dict(nbin=0), dict(nbin=1025), dict(nbin=-1),
    dict(nf=0), dict(nf=17), dict(nf=-1),
    dict(R=0), dict(R=4097), dict(R=-1),
    dict(nq=0, q=()), dict(nq=33, q=tuple(range(33))),
    dict(q=(-1e-9,)), dict(q=(100.0000001,)), dict(q=(float("nan"),)), dict(nq=2, q=(50.0, float("nan"))),
    dict(method=2), dict(method=-1), dict(method=1, nq=2, q=(50.0, 50.0)), dict(method=1, nq=0, q=None),
    dict(field_vals=[0, 1, 2, 0, 0, 0]), dict(field_vals=[0, 0, 0, 0, 0, -1]),
    dict(pref0=0.0), dict(pref0=-1.0), dict(pref0=float("nan")),
    dict(draw_vals=_bad_draw(2, 0, float("nan"))), dict(draw_vals=_bad_draw(2, 1, float("inf"))),
    dict(draw_vals=_bad_draw(2, 2, float("-inf"))), dict(draw_vals=_bad_draw(2, 2, float("nan"))),
    dict(draw_vals=_bad_draw(2, 0, 0.0)), dict(draw_vals=_bad_draw(2, 1, -2.7e-17)), dict(draw_vals=_bad_draw(2, 2, 0.0)),
])
def test_bad_arguments_are_refused_before_the_device_is_touched(lib, kw):
    assert _call(lib, **kw) == capi.LF_ERR_ARG


def test_wrapper_raises_lferror(lib):
    with pytest.raises(capi.LFError):
        capi.veff_draws_device(np.full(4, 3e-17), np.zeros(4), 1.0e6, 0.04, 0.1, np.zeros(4), 3, np.zeros((2, 2)))
    with pytest.raises(ValueError):
        capi.veff_draws_device(np.full(4, 3e-17), np.zeros(3), 1.0e6, 0.04, 0.1, np.zeros(4), 3, np.full((2, 2), 3.0))
