"""Posterior LF bands on the device (lf_lumfunc_quantiles, csrc/lf_bands.h): the values against the host formula, the
quantiles bit for bit against np.percentile / np.median applied to the device's own values, the special values of the
Schechter form (0, +inf, NaN, ties), and the model classes' device paths against their host paths."""
import numpy as np
import pytest

from lf_testlib import synth
from lumfuncmcmc_amd import capi, lfbands

pytestmark = pytest.mark.gpu

Q5 = (2.5, 16.0, 50.0, 84.0, 97.5)
PIV = (1.2, 1.53, 1.86)


def _bits_equal(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape
    gn, wn = np.isnan(got), np.isnan(want)
    np.testing.assert_array_equal(gn, wn)
    bad = got[~gn].view(np.int64) != want[~wn].view(np.int64)
    assert not bad.any(), (got[~gn][bad][:5], want[~wn][bad][:5])


def _values_close(dev, host):
    """rtol 1e-12; absolute 1e-300 where either side is subnormal or zero; inf / NaN in the same places."""
    tiny = np.finfo(np.float64).tiny
    np.testing.assert_array_equal(np.isnan(dev), np.isnan(host))
    np.testing.assert_array_equal(np.isinf(dev), np.isinf(host))
    fin = np.isfinite(dev) & np.isfinite(host)
    d, h = dev[fin], host[fin]
    small = (np.abs(d) < tiny) | (np.abs(h) < tiny)
    assert np.all(np.abs(d[small] - h[small]) <= 1e-300)
    np.testing.assert_allclose(d[~small], h[~small], rtol=1e-12, atol=0)


def _draws(variant, R, rng):
    if variant == "free":
        return np.column_stack([rng.normal(42.5, 0.3, R), rng.normal(-2.5, 0.4, R), rng.normal(-1.5, 0.3, R)])
    rows = np.column_stack([rng.normal(42.5, 0.15, (R, 3)), rng.normal(-2.5, 0.15, (R, 3)), rng.normal(-1.5, 0.3, R)])
    return lfbands.pack_draws("zevol", rows, pivots=PIV)


def _check_bitwise(variant, draws, logL, z, q=Q5):
    out, v = capi.lumfunc_quantiles(variant, draws, logL, z=z, q=q, values=True)
    with np.errstate(all="ignore"):
        _bits_equal(out, np.percentile(v, q, axis=0))
        med = capi.lumfunc_quantiles(variant, draws, logL, z=z, method=capi.LF_Q_MEDIAN)
        _bits_equal(med, np.median(v, axis=0)[None])
    return out, v


@pytest.mark.parametrize("variant", ["free", "zevol"])
def test_values_and_quantiles_at_1e5_points(variant):
    rng = np.random.default_rng(1)
    P, R = 100000, 200
    logL = rng.uniform(40.0, 45.0, P)
    z = rng.uniform(1.1, 2.0, P) if variant == "zevol" else None
    draws = _draws(variant, R, rng)
    out, v = _check_bitwise(variant, draws, logL, z)
    _values_close(v, lfbands.lf_values(variant, draws, logL, z))
    assert capi.lumfunc_quantiles_ms() > 0.0


@pytest.mark.parametrize("R", [1, 2, 3, 63, 64, 65, 200, 256, 257, 1000, 4096])
@pytest.mark.parametrize("variant", ["free", "zevol"])
def test_every_draw_count_is_bitwise_numpy(R, variant):
    rng = np.random.default_rng(R)
    P = 129
    logL = rng.uniform(40.5, 44.5, P)
    z = rng.uniform(1.1, 2.0, P) if variant == "zevol" else None
    _check_bitwise(variant, _draws(variant, R, rng), logL, z, q=(0.0, 2.5, 16.0, 50.0, 84.0, 97.5, 100.0))


def test_ties_zeros_infinities_and_nans():
    rng = np.random.default_rng(9)
    base = np.array([[42.5, -2.5, -1.5], [42.7, -2.4, -1.2], [42.3, -2.7, -2.0], [42.6, -2.6, 0.5], [42.4, -2.5, -0.5]])
    draws = base[rng.integers(0, len(base), 300)]                          # with replacement: many duplicate rows
    logL = np.concatenate([
        rng.uniform(41.0, 44.0, 50),
        [46.0, 48.0, 60.0],                   # far above L*: exp(-10^t) underflows, the LF is 0 for every draw
        [42.5 - 400.0, 42.5 - 350.0],         # far below L*: 10^(t (alpha + 1)) = inf for alpha + 1 < 0, finite otherwise
        [42.5 + 400.0],                       # far above with alpha + 1 > 0: inf * 0 = NaN for some draws
    ])
    with np.errstate(all="ignore"):
        out, v = _check_bitwise("free", draws, logL, None, q=(0.0, 16.0, 50.0, 84.0, 100.0))
        _values_close(v, lfbands.lf_values("free", draws, logL))
    assert np.all(v[:, 50:53] == 0.0)
    assert np.isinf(v[:, 53]).any() and np.isfinite(v[:, 53]).any()
    assert np.isnan(v[:, 55]).any()
    assert np.isnan(out[-1, 53])                  # np.percentile(.., 100) with an inf maximum is NaN (inf - inf)
    assert np.all(np.isnan(out[:, 55]))           # a NaN among the values: every quantile NaN
    assert np.all(out[:, 50:53] == 0.0)


def _model(n, seed=7):
    from lumfuncmcmc_amd.model import LumFuncMCMC
    cat = synth.catalogue(n, seed=seed)
    fi = cat["field_ind"]
    m = LumFuncMCMC(synth.split_fields(cat["z"], fi), lum=synth.split_fields(cat["lum"], fi),
                    lum_e=synth.split_fields(cat["lum_e"], fi), Flim=list(synth.FLIM), alpha=synth.ALPHA_C,
                    Omega_0=list(synth.OMEGA_0), sch_al=synth.SCH_AL, sch_al_lims=synth.SCH_AL_LIMS, Lstar=synth.LSTAR,
                    Lstar_lims=synth.LSTAR_LIMS, phistar=synth.PHISTAR, phistar_lims=synth.PHISTAR_LIMS, Lc=synth.LC,
                    Lh=synth.LH, nwalkers=32, nsteps=10, min_comp_frac=0.0, field_ind=fi, Flim_lims=synth.FLIM_LIMS,
                    alpha_lims=synth.ALPHA_LIMS, nboot=20, nbins=25)
    rng = np.random.default_rng(seed)
    th = np.column_stack([rng.normal(42.6, 0.05, 400), rng.normal(-2.1, 0.05, 400), rng.normal(-1.5, 0.05, 400)] +
                         [rng.normal(f, 0.1, 400) for f in synth.FLIM] + [rng.normal(synth.ALPHA_C, 0.1, 400)])
    m.samples = np.column_stack([th, rng.normal(-100.0, 3.0, 400)])
    return m


def test_set_median_fit_device_agrees_with_the_host_path():
    m = _model(5000)
    m.context()                                   # the object holds a context: VeffLF takes its device path both times
    res = {}
    for dev in (False, True):
        np.random.seed(2024)
        m.set_median_fit(device=dev)
        res[dev] = (m.medianLF.copy(), list(m.Flim), m.alpha, m.Lavg.copy(), m.lfbinorig.copy(), m.var.copy(), np.random.get_state())
    m.close()
    h, d = res[False], res[True]
    np.testing.assert_allclose(d[0], h[0], rtol=1e-12, atol=1e-300)
    assert d[1] == h[1] and d[2] == h[2]
    np.testing.assert_array_equal(d[3], h[3])
    # lfbinorig and var come from lf_veff in both runs, with the same inputs and the same seed; its bins are summed with
    # atomics, whose order differs from launch to launch, so two calls agree to rounding, not bit for bit
    for a, b in zip(d[4:6], h[4:6]):
        np.testing.assert_allclose(a, b, rtol=1e-12, atol=0)
    np.testing.assert_array_equal(d[6][1], h[6][1])
    assert d[6][2:] == h[6][2:]


def test_z_model_band_on_the_default_mesh():
    from lumfuncmcmc_amd.model import LumFuncMCMCz
    cat = synth.catalogue(2000, seed=5)
    fi = cat["field_ind"]
    np.random.seed(1)
    m = LumFuncMCMCz(synth.split_fields(cat["z"], fi), lum=synth.split_fields(cat["lum"], fi),
                     lum_e=synth.split_fields(cat["lum_e"], fi), Flim=list(synth.FLIM), alpha=synth.ALPHA_C,
                     Omega_0=list(synth.OMEGA_0), sch_al=synth.SCH_AL, nwalkers=32, nsteps=10, min_comp_frac=0.0, field_ind=fi)
    rng = np.random.default_rng(5)
    th = np.column_stack([rng.normal(42.4, 0.05, (300, 3)), rng.normal(-2.3, 0.05, (300, 3)), rng.normal(-1.5, 0.05, 300),
                          rng.normal(-50.0, 2.0, 300)])
    m.samples = th
    out = {}
    for dev in (False, True):
        np.random.seed(77)
        out[dev] = m.lf_percentiles(percentiles=(16, 50, 84), device=dev)
    assert out[True].shape == (3, 100, 100)
    _values_close(out[True], out[False])
    np.random.seed(77)
    med = m.lf_percentiles(method="median", device=True)
    assert med.shape == (1, 100, 100)


def test_a_million_points_spot_checked():
    rng = np.random.default_rng(12)
    P, R = 1000000, 200
    logL = rng.uniform(40.0, 45.0, P)
    draws = _draws("free", R, rng)
    out = capi.lumfunc_quantiles("free", draws, logL, q=Q5)
    idx = rng.choice(P, 1000, replace=False)
    want = lfbands.quantiles_host("free", draws, logL[idx], q=Q5)
    _values_close(out[:, idx], want)
