"""The 1/Veff LF marginalised over the completeness posterior on the device (lf_veff_draws, csrc/lf_veffdraws.h; DESIGN.md
section 3.17): the per-draw binned sums against the NumPy twin (veff.veff_draws), the percentiles bit for bit against
np.percentile / np.median of the device's own values, the fixed order of summation (same bits on every call, a row that
depends on its draw alone), the chunk edges, and LumFuncMCMC.veff_percentiles's device path against its host path.

Tolerance of the sums: rtol 1e-12, the standing tolerance of lf_veff's bins against the host (test_gpu_veff.py)."""
import functools

import numpy as np
import pytest

from lf_testlib import synth
from lumfuncmcmc_amd import capi, hostsetup as hs, veff

pytestmark = pytest.mark.gpu

N = 3000
RTOL = 1e-12
PREF0 = sum(synth.OMEGA_0) / hs.SQARCSEC
Q = (0.0, 16.0, 50.0, 84.0, 100.0)


def _bits_equal(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape
    assert not np.isnan(got).any() and not np.isnan(want).any()
    bad = got.view(np.int64) != want.view(np.int64)
    assert not bad.any(), (got[bad][:5], want[bad][:5])


@functools.lru_cache(maxsize=None)
def _catalogue():
    from lumfuncmcmc_amd.cosmology import cosmo
    cat = synth.catalogue(N, seed=11)
    flux = 10 ** cat["lum"] / (4.0 * np.pi * (capi.MPC_CM * np.asarray(cosmo.luminosity_distance(cat["z"]))) ** 2)
    rng = np.random.default_rng(4)
    vol = rng.uniform(2.0e5, 1.0e6, N)                         # per-source volumes, some sources without one
    vol[rng.choice(N, 40, replace=False)] = 0.0
    vol[rng.choice(N, 10, replace=False)] = -1.0
    return {"lum": cat["lum"], "flux": flux, 5: np.repeat(np.arange(5), np.diff(cat["field_ind"])), 1: np.zeros(N, dtype=np.int64),
            "vol": vol}


def _bins(lum, nbin):
    """veff.luminosity_bins's index for any nbin >= 1 (nbin = no bin)"""
    edges = np.linspace(min(lum) * 1.001, max(lum), nbin + 1)
    idx = np.searchsorted(edges, lum, side="right") - 1
    idx[(lum < edges[0]) | (lum >= edges[-1])] = nbin
    return idx


@functools.lru_cache(maxsize=None)
def _draws(nf):
    """4096 draws from N(synth.FLIM, 0.1) and N(synth.ALPHA_C, 0.1), clipped into the prior box"""
    rng = np.random.default_rng(100 + nf)
    R = 4096
    cols = [np.clip(rng.normal(f, 0.1, R), *synth.FLIM_LIMS) * 1.0e-17 for f in synth.FLIM[:nf]]
    return np.ascontiguousarray(np.column_stack(cols + [np.clip(rng.normal(synth.ALPHA_C, 0.1, R), *synth.ALPHA_LIMS)]))


@functools.lru_cache(maxsize=None)
def _phi(nf, fcmin, per_source, R):
    """The twin's weight of every source under the first R draws: the twin with one bin per source (0 + phi is phi).
    Computed once per configuration; the references of all bin counts and of all smaller R are sums / rows of it."""
    c = _catalogue()
    phi = veff.veff_draws(c["flux"], c[nf], c["vol"] if per_source else 1.0e6, PREF0, fcmin, np.arange(N), N, _draws(nf)[:R])
    phi.setflags(write=False)
    return phi


def _twin(nf, fcmin, per_source, R, nbin):
    idx = _bins(_catalogue()["lum"], nbin)
    phi = _phi(nf, fcmin, per_source, 4096 if (nf, fcmin, per_source) == (5, 0.1, False) else 257)
    return np.array([np.bincount(idx, weights=p, minlength=nbin + 1)[:nbin] for p in phi[:R]])


@functools.lru_cache(maxsize=None)
def _device(nf, fcmin, per_source, R, nbin, method=capi.LF_Q_LINEAR):
    c = _catalogue()
    return capi.veff_draws_device(c["flux"], c[nf], c["vol"] if per_source else 1.0e6, PREF0, fcmin, _bins(c["lum"], nbin), nbin,
                                  _draws(nf)[:R], q=Q, method=method)


def _check_values(nf, fcmin, per_source, R, nbin):
    _, v = _device(nf, fcmin, per_source, R, nbin)
    want = _twin(nf, fcmin, per_source, R, nbin)
    assert v.shape == want.shape == (R, nbin)
    with np.errstate(divide="ignore", invalid="ignore"):
        print("nf %d fcmin %g per-source %d R %d nbin %d: max rel diff %.3e" %
              (nf, fcmin, per_source, R, nbin, np.nanmax(np.where(want != 0, np.abs(v / want - 1.0), 0.0))))
    np.testing.assert_array_equal(v[:, (want == 0).all(axis=0)], 0.0)
    np.testing.assert_allclose(v, want, rtol=RTOL, atol=0)
    assert (want > 0).any()


@pytest.mark.parametrize("R", [1, 2, 200, 256, 257, 4096])
def test_values_against_the_twin_for_every_draw_count(R):
    _check_values(5, 0.1, False, R, 25)
    assert all(t >= 0.0 for t in capi.veff_draws_ms())


@pytest.mark.parametrize("nbin", [1, 1024])
def test_values_against_the_twin_with_one_bin_and_with_more_bins_than_chunks_have_sources(nbin):
    _check_values(5, 0.1, False, 257, nbin)


@pytest.mark.parametrize("nf,fcmin,per_source", [(5, 0.1, True), (5, 0.0, False), (5, 0.0, True), (1, 0.1, False), (1, 0.1, True),
                                                 (1, 0.0, False), (1, 0.0, True)])
def test_values_against_the_twin_for_one_field_the_plain_curve_and_per_source_volumes(nf, fcmin, per_source):
    _check_values(nf, fcmin, per_source, 257, 25)


@pytest.mark.parametrize("R", [1, 2, 200, 257, 4096])
def test_percentiles_are_numpys_of_the_devices_values_bit_for_bit(R):
    out, v = _device(5, 0.1, False, R, 25)
    assert out.shape == (len(Q), 25)
    _bits_equal(out, np.percentile(v, Q, axis=0))
    med, v2 = _device(5, 0.1, False, R, 25, method=capi.LF_Q_MEDIAN)
    _bits_equal(v2, v)
    _bits_equal(med, np.median(v, axis=0)[None])


def test_two_calls_give_the_same_bits_and_a_row_depends_on_its_draw_alone():
    c = _catalogue()
    idx = _bins(c["lum"], 25)
    D = _draws(5)

    def run(draws):
        return capi.veff_draws_device(c["flux"], c[5], c["vol"], PREF0, 0.1, idx, 25, draws, q=Q)

    out_a, a = run(D[:257])
    out_b, b = run(D[:257])
    _bits_equal(a, b)
    _bits_equal(out_a, out_b)
    _bits_equal(run(D[100:101])[1][0], a[100])                                 # alone
    _bits_equal(run(np.vstack([D[100:101], D[:199]]))[1][0], a[100])           # first of 200, in another lane and tile


def test_chunk_edges_dropped_sources_and_an_empty_field():
    C = capi.veff_draws_chunk()
    counts = [0, 1, C - 1, C, C + 1, 2 * C + 1]
    nbin, nf = len(counts), 4
    rng = np.random.default_rng(8)
    bin_of = np.concatenate([np.full(k, b) for b, k in enumerate(counts)] + [np.full(7, -1), np.full(5, nbin), [nbin + 3, -9]])
    rng.shuffle(bin_of)                       # the sort has to gather the bins, and keep the order within each
    n = bin_of.size
    flux = rng.uniform(2.0e-17, 9.0e-17, n)
    field = rng.choice([0, 1, 3], n)          # no source in field 2
    vol = rng.uniform(2.0e5, 1.0e6, n)
    vol[rng.choice(n, 9, replace=False)] = 0.0
    draws = np.column_stack([rng.uniform(2.0e-17, 4.0e-17, (300, nf)), rng.uniform(3.0, 6.0, 300)])
    for v in (vol, 7.0e5):
        out, got = capi.veff_draws_device(flux, field, v, PREF0, 0.1, bin_of, nbin, draws, q=Q)
        want = veff.veff_draws(flux, field, v, PREF0, 0.1, bin_of, nbin, draws)
        np.testing.assert_array_equal(got[:, 0], 0.0)
        assert np.all(got[:, 1:] > 0.0)
        np.testing.assert_allclose(got, want, rtol=RTOL, atol=0)
        _bits_equal(out, np.percentile(got, Q, axis=0))
    # every source outside the bins: nothing to sum
    out, got = capi.veff_draws_device(flux, field, vol, PREF0, 0.1, np.full(n, -1), nbin, draws[:3], q=Q)
    np.testing.assert_array_equal(got, 0.0)
    np.testing.assert_array_equal(out, 0.0)


def test_one_source():
    draws = np.column_stack([np.array([2.5e-17, 2.7e-17, 3.0e-17]), np.array([4.0, 4.5, 5.0])])
    for b in (0, 2):
        out, got = capi.veff_draws_device([3.1e-17], [0], 6.0e5, PREF0, 0.1, [b], 3, draws, q=Q)
        want = veff.veff_draws(np.array([3.1e-17]), [0], 6.0e5, PREF0, 0.1, [b], 3, draws)
        np.testing.assert_allclose(got, want, rtol=RTOL, atol=0)
        np.testing.assert_array_equal(got[:, [k for k in range(3) if k != b]], 0.0)
        assert np.all(got[:, b] > 0.0)
        _bits_equal(out, np.percentile(got, Q, axis=0))


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


def test_veff_percentiles_device_agrees_with_the_host_path():
    m = _model(5000)
    res = {}
    for dev in (False, True):
        np.random.seed(2024)
        res[dev] = (m.veff_percentiles(device=dev), np.random.get_state())
    (h, hs_), (d, ds_) = res[False], res[True]
    np.testing.assert_array_equal(d["Lavg"], h["Lavg"])
    assert d["values"].shape == h["values"].shape == (200, 25) and d["percentiles"].shape == (3, 25)
    np.testing.assert_allclose(d["values"], h["values"], rtol=RTOL, atol=0)
    np.testing.assert_allclose(d["percentiles"], h["percentiles"], rtol=RTOL, atol=0)
    np.testing.assert_allclose(d["var_comp"], np.var(d["values"], axis=0, ddof=1), rtol=1e-15, atol=0)
    np.testing.assert_array_equal(ds_[1], hs_[1])
    assert ds_[0] == hs_[0] and ds_[2:] == hs_[2:]
    m.close()
