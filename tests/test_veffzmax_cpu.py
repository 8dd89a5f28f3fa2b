"""z_max per source and draw in the marginalised 1/Veff points, host side: the NumPy twin
veff.veff_draws_zmax is a loop over the existing functions bit for bit, the volume table (voltable) holds eps_T <= 1e-13 of
the total volume with exact clamps and no step down across a piece edge, and LumFuncMCMC.veff_percentiles(volumes=...)
keeps the fixed path's bits where the two must agree.  No GPU."""
import functools
import os
import re

import numpy as np
import pytest

from lf_testlib import synth
from lumfuncmcmc_amd import hostsetup as hs, veff, voltable
from lumfuncmcmc_amd.cosmology import cosmo

N = 3000
PREF0 = sum(synth.OMEGA_0) / hs.SQARCSEC
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_COMPLETENESS_ROOTS = hs.completeness_roots                    # the real one, whatever a test patches in below


def _bits_equal(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape
    assert not np.isnan(got).any() and not np.isnan(want).any()
    bad = got.view(np.int64) != want.view(np.int64)
    assert not bad.any(), (got[bad][:5], want[bad][:5])


@functools.lru_cache(maxsize=None)
def _setup():
    cat = synth.catalogue(N, seed=11)
    t = hs.distance_tables(cat["z"], cosmo)
    flux = 10 ** cat["lum"] / (4.0 * np.pi * (hs.MPC_CM * np.asarray(cosmo.luminosity_distance(cat["z"]))) ** 2)
    field = np.repeat(np.arange(5), np.diff(cat["field_ind"]))
    rng = np.random.default_rng(5)
    R = 6
    draws = np.column_stack([np.clip(rng.normal(f, 0.1, R), *synth.FLIM_LIMS) * 1.0e-17 for f in synth.FLIM] +
                            [np.clip(rng.normal(synth.ALPHA_C, 0.1, R), *synth.ALPHA_LIMS)])
    fmin = _roots41().ev(draws[:, :5] / 1.0e-17, draws[:, 5][:, None])
    fmin[3] = 0.0                                              # a row without a cut
    fmin[4, 2] = 0.0                                           # and one field of another row
    _, _, _, idx = veff.luminosity_bins(cat["lum"], 25)
    return {"lum": cat["lum"], "flux": flux, "field": field, "draws": draws, "fmin": fmin, "idx": idx, "dVdzf": t["dVdzf"],
            "zmin": cat["z"].min(), "zmax": cat["z"].max()}


@functools.lru_cache(maxsize=None)
def _table():
    s = _setup()
    return voltable.build(cosmo, s["dVdzf"], s["zmin"], s["zmax"])


def test_every_twin_row_is_veff_draws_with_that_rows_volumes_bit_for_bit():
    s = _setup()
    got = veff.veff_draws_zmax(s["lum"], s["flux"], s["field"], s["fmin"], s["zmin"], s["zmax"], s["dVdzf"], cosmo, PREF0, 0.1, s["idx"],
                               25, s["draws"])
    assert got.shape == (6, 25)
    between = 0
    for r in range(6):
        fm = s["fmin"][r][s["field"]]
        with np.errstate(divide="ignore"):                         # the definition: max_redshift on the whole array
            zi = np.where(fm > 0, veff.max_redshift(10 ** s["lum"], fm, cosmo), np.inf)
        zi = np.minimum(s["zmax"], zi)
        vol = veff.comoving_volume(s["dVdzf"], s["zmin"], zi)
        between += int(((zi > s["zmin"]) & (zi < s["zmax"])).sum())
        _bits_equal(got[r], veff.veff_draws(s["flux"], s["field"], vol, PREF0, 0.1, s["idx"], 25, s["draws"][r:r + 1])[0])
    assert between > 0.05 * 6 * N                              # the cut moves inside the survey for many pairs
    out, values = veff.veff_draws_zmax_quantiles(s["lum"], s["flux"], s["field"], s["fmin"], s["zmin"], s["zmax"], s["dVdzf"], cosmo, PREF0,
                                                 0.1, s["idx"], 25, s["draws"], q=(16.0, 50.0, 84.0))
    _bits_equal(values, got)
    _bits_equal(out, np.percentile(got, (16.0, 50.0, 84.0), axis=0))
    med, _ = veff.veff_draws_zmax_quantiles(s["lum"], s["flux"], s["field"], s["fmin"], s["zmin"], s["zmax"], s["dVdzf"], cosmo, PREF0,
                                            0.1, s["idx"], 25, s["draws"], method="median")
    _bits_equal(med, np.median(got, axis=0)[None])


def test_a_row_without_a_cut_is_veff_draws_with_the_full_volume():
    """fmin = 0: every source's volume is the array branch's full volume (the exact integral of the interpolant), which
    differs from the scalar branch's scipy.quad by quad's own tolerance - 1e-8 is the documented bound (veff.lumfunc_weights)"""
    s = _setup()
    row = veff.veff_draws_zmax(s["lum"], s["flux"], s["field"], s["fmin"][3:4], s["zmin"], s["zmax"], s["dVdzf"], cosmo, PREF0, 0.1,
                               s["idx"], 25, s["draws"][3:4])[0]
    full = veff.comoving_volume(s["dVdzf"], s["zmin"], np.array([s["zmax"]]))[0]
    _bits_equal(row, veff.veff_draws(s["flux"], s["field"], np.full(N, full), PREF0, 0.1, s["idx"], 25, s["draws"][3:4])[0])
    scalar = veff.veff_draws(s["flux"], s["field"], veff.comoving_volume(s["dVdzf"], s["zmin"], s["zmax"]), PREF0, 0.1, s["idx"], 25,
                             s["draws"][3:4])[0]
    np.testing.assert_allclose(row, scalar, rtol=1e-8, atol=0)
    assert (row > 0).any()


def test_max_redshift_kept_its_bits_when_the_inverse_was_split_out():
    s = _setup()
    z = veff.max_redshift(10 ** s["lum"], 3.0e-17, cosmo)
    want = veff.redshift_at_distance(np.sqrt(10 ** s["lum"] / (4.0 * np.pi * 3.0e-17)) / veff.MPC_CM_EXACT, cosmo)
    _bits_equal(z, want)
    np.testing.assert_allclose(np.asarray(cosmo.luminosity_distance(z)), np.sqrt(10 ** s["lum"] / (4.0 * np.pi * 3.0e-17)) / veff.MPC_CM_EXACT,
                               rtol=1e-12)


def test_volume_table_holds_1e13_of_the_total_volume():
    s, tab = _setup(), _table()
    print("eps_T = %.3e over %d node pieces and %d z pieces" % (tab.eps, len(tab.rec), voltable.NPIECE))
    assert tab.eps <= 1e-13
    # the same samples against the twin's own stop (1e-13 in z): the twin's polish is not the floor
    D = np.exp(np.linspace(np.log(tab.d_lo), np.log(tab.d_hi), 100000))
    zt = np.minimum(s["zmax"], veff.redshift_at_distance(D, cosmo))
    e_twin = np.max(np.abs(tab.eval(D) - veff.comoving_volume(s["dVdzf"], s["zmin"], zt))) / tab.v_total
    print("against the twin's own inverse: %.3e" % e_twin)
    assert e_twin <= 1e-13


def test_volume_table_clamps_are_exact():
    s, tab = _setup(), _table()
    full = veff.comoving_volume(s["dVdzf"], s["zmin"], np.full(3, s["zmax"]))
    _bits_equal(tab.eval([tab.d_hi, np.nextafter(tab.d_hi, np.inf), np.inf]), full)
    np.testing.assert_array_equal(tab.eval([tab.d_lo, np.nextafter(tab.d_lo, 0.0), 1.0, 0.0, np.nan]), 0.0)
    assert tab.d_lo == cosmo.luminosity_distance(np.array([s["zmin"]]))[0]
    assert 0.0 < tab.eval([np.nextafter(tab.d_lo, np.inf)])[0] < 1e-9 * tab.v_total
    assert tab.eval([np.nextafter(tab.d_hi, 0.0)])[0] <= tab.v_total


def test_volume_table_does_not_decrease_across_any_piece_edge():
    tab = _table()
    e = tab.edges()
    assert len(e) == len(tab.rec) + 1 + voltable.NPIECE - 1
    lo, hi = np.nextafter(e, -np.inf), np.nextafter(e, np.inf)
    ve, vlo, vhi = tab.eval(e), tab.eval(lo), tab.eval(hi)
    assert np.all(vlo <= ve) and np.all(ve <= vhi)
    assert np.all(np.diff(ve) > 0)
    # every node piece stays between the twin's own volumes of its two knots, whatever the last bits of z
    for d in (tab.rec[:, 0], np.nextafter(tab.rec[:, 1], 0.0)):
        assert np.all(tab.eval(d) >= tab.rec[:, 3]) and np.all(tab.eval(d) <= tab.rec[:, 4])


def test_a_table_that_misses_the_bound_is_refused_wherever_it_is_used():
    """equal pieces in D do not reach 1e-13 over z = 0.1 .. 6: voltable.require refuses the table, for the class and for a
    direct caller of the quantile wrapper alike (the refusal comes before the device is looked for)"""
    z = np.linspace(0.1, 6.0, 400)
    t = hs.distance_tables(z, cosmo)
    tab = voltable.build(cosmo, t["dVdzf"], 0.1, 6.0)
    print("eps_T over z = 0.1 .. 6: %.3e" % tab.eps)
    assert tab.eps > voltable.EPS_MAX
    with pytest.raises(ValueError, match="reaches only"):
        voltable.require(tab)
    with pytest.raises(ValueError, match="not validated"):
        voltable.require(voltable.build(cosmo, t["dVdzf"], 0.1, 6.0, validate=False))
    assert voltable.require(_table()) is _table()
    s = _setup()
    for table in (None, tab):
        with pytest.raises(ValueError, match="reaches only"):
            veff.veff_draws_zmax_quantiles(np.array([42.0]), np.array([3.0e-17]), [0], [[3.0e-17]], 0.1, 6.0, t["dVdzf"], cosmo, PREF0, 0.1,
                                           [0], 1, s["draws"][:1, [0, 5]], device=True, table=table)


def test_table_constants_match_the_kernels():
    src = open(os.path.join(ROOT, "lumfuncmcmc_amd", "csrc", "lf_veffdraws.h")).read()
    for name, val in (("VEFFZ_NPIECE", voltable.NPIECE), ("VEFFZ_DEG", voltable.DEG), ("VEFFZ_REC", voltable.REC)):
        assert int(re.search(r"constexpr int %s = (\d+);" % name, src).group(1)) == val


def test_the_entry_is_declared_and_exported():
    from lumfuncmcmc_amd import build, capi
    build.build_library(verbose=False)
    lib = capi.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lfmcmc.h")).read(), flags=re.S)
    assert "lf_veff_draws_zmax" in header and "lf_veff_draws_zmax" in capi.EXPORTS and hasattr(lib, "lf_veff_draws_zmax")


def test_argument_errors_come_before_the_device():
    """no GPU here: a call that reached the device would return LF_ERR_NODEV or LF_ERR_HIP, not LF_ERR_ARG"""
    from lumfuncmcmc_amd import capi
    s, tab = _setup(), _table()
    dist = veff.source_distance_scale(s["lum"])

    def run(**kw):
        a = dict(flux=s["flux"], field=s["field"], dist=dist, pref0=PREF0, fcmin=0.1, bin_of=s["idx"], nbin=25, draws=s["draws"],
                 fmin=s["fmin"], table=tab)
        a.update(kw)
        with pytest.raises(capi.LFError) as e:
            capi.veff_draws_zmax_device(a["flux"], a["field"], a["dist"], a["pref0"], a["fcmin"], a["bin_of"], a["nbin"], a["draws"],
                                        a["fmin"], a["table"])
        return str(e.value)

    def broken(**kw):
        t = voltable.VolumeTable(tab.head.copy(), tab.zc.copy(), tab.rec.copy())
        for k, (idx, v) in kw.items():
            getattr(t, k)[idx] = v
        return t

    bad = lambda a, i, v: np.concatenate([a[:i], [v], a[i + 1:]])
    f2 = s["fmin"].copy()
    f2[1, 1] = -1.0e-17
    f3 = s["fmin"].copy()
    f3[5, 4] = np.nan
    cases = [dict(fmin=f2), dict(fmin=f3), dict(dist=bad(dist, 7, -1.0)), dict(dist=bad(dist, N - 1, np.inf)),
             dict(dist=bad(dist, 0, np.nan)), dict(pref0=0.0), dict(nbin=0), dict(field=bad(s["field"], 3, 5)),
             dict(table=broken(rec=((10, 0), np.nan))), dict(table=broken(rec=((10, 1), tab.rec[10, 0]))),
             dict(table=broken(rec=((5, 4), tab.rec[5, 3] * 0.5))), dict(table=broken(head=(2, -1.0))),
             dict(table=broken(head=(1, tab.head[0]))), dict(table=broken(zc=((3, 2), np.inf))),
             dict(table=broken(rec=((0, 3), 1.0))), dict(table=broken(head=(3, 2.0 * tab.head[3])))]
    for kw in cases:
        assert "(%d)" % capi.LF_ERR_ARG in run(**kw), kw.keys()


# ------------------------------------------------------------------------------------------ the class
@functools.lru_cache(maxsize=None)
def _roots41():
    return _COMPLETENESS_ROOTS(synth.FLIM_LIMS, synth.ALPHA_LIMS, 0.1, 0.5, 41)


def _model(monkeypatch, min_comp_frac, spread, n=2000, seed=7, fix_comp=False):
    """a LumFuncMCMC with a fake chain around the truth; the completeness roots on a 41 x 41 surface (the class builds
    201 x 201: 4 s of fsolve that these tests do not need)"""
    from lumfuncmcmc_amd import model
    real = _COMPLETENESS_ROOTS
    monkeypatch.setattr(model.hs, "completeness_roots",
                        lambda fl, al, fcmin, mcf, size=201: _roots41() if mcf == 0.5 and fcmin == 0.1 else real(fl, al, fcmin, mcf, 41))
    cat = synth.catalogue(n, seed=seed)
    fi = cat["field_ind"]
    m = model.LumFuncMCMC(synth.split_fields(cat["z"], fi), lum=synth.split_fields(cat["lum"], fi),
                          lum_e=synth.split_fields(cat["lum_e"], fi), Flim=list(synth.FLIM), alpha=synth.ALPHA_C,
                          Omega_0=list(synth.OMEGA_0), sch_al=synth.SCH_AL, sch_al_lims=synth.SCH_AL_LIMS, Lstar=synth.LSTAR,
                          Lstar_lims=synth.LSTAR_LIMS, phistar=synth.PHISTAR, phistar_lims=synth.PHISTAR_LIMS, Lc=synth.LC,
                          Lh=synth.LH, nwalkers=32, nsteps=10, min_comp_frac=min_comp_frac, field_ind=fi, Flim_lims=synth.FLIM_LIMS,
                          alpha_lims=synth.ALPHA_LIMS, nboot=20, nbins=25, fix_comp=fix_comp)
    rng = np.random.default_rng(seed)
    th = np.column_stack([rng.normal(42.6, 0.05, 400), rng.normal(-2.1, 0.05, 400), rng.normal(-1.5, 0.05, 400)] +
                         [rng.normal(f, spread, 400) for f in synth.FLIM] + [rng.normal(synth.ALPHA_C, spread, 400)])
    m.samples = np.column_stack([th, rng.normal(-100.0, 3.0, 400)])
    return m


def _both(m, ndraws=20):
    res = {}
    for v in ("fixed", "per_draw"):
        np.random.seed(2024)
        res[v] = (m.veff_percentiles(ndraws=ndraws, device=False, volumes=v), np.random.get_state())
    assert res["fixed"][1][0] == res["per_draw"][1][0] and np.array_equal(res["fixed"][1][1], res["per_draw"][1][1])
    assert res["fixed"][1][2:] == res["per_draw"][1][2:]                  # the global stream is consumed alike
    return res["fixed"][0], res["per_draw"][0]


def test_per_draw_without_a_flux_cut_is_the_fixed_path_bit_for_bit(monkeypatch):
    m = _model(monkeypatch, 0.0, 0.1)
    fixed, per = _both(m)
    for k in ("Lavg", "percentiles", "values", "var_comp"):
        _bits_equal(per[k], fixed[k])
    np.random.seed(2024)
    _bits_equal(m.veff_percentiles(ndraws=20, device=False)["values"], fixed["values"])      # the default is "fixed"
    assert (fixed["values"] > 0).any()


def test_per_draw_on_a_chain_that_holds_the_current_completeness_is_the_fixed_path(monkeypatch):
    m = _model(monkeypatch, 0.5, 0.0)
    fixed, per = _both(m, ndraws=5)
    assert (fixed["values"] > 0).any()
    np.testing.assert_allclose(per["values"], fixed["values"], rtol=1e-12, atol=0)
    np.testing.assert_allclose(per["percentiles"], fixed["percentiles"], rtol=1e-12, atol=0)


def test_per_draw_moves_the_points_when_the_completeness_varies(monkeypatch):
    m = _model(monkeypatch, 0.5, 0.1)
    fixed, per = _both(m, ndraws=5)
    assert per["values"].shape == fixed["values"].shape == (5, 25)
    assert np.any(per["values"] != fixed["values"])
    assert np.all(np.isfinite(per["values"])) and np.all(per["values"] >= 0)


def test_refusals(monkeypatch):
    m = _model(monkeypatch, 0.0, 0.1)
    with pytest.raises(ValueError, match="volumes"):
        m.veff_percentiles(device=False, volumes="per-draw")
    with pytest.raises(ValueError, match="volumes"):
        m.veff_percentiles(device=False, volumes=None)
    mf = _model(monkeypatch, 0.0, 0.1, fix_comp=True)
    with pytest.raises(ValueError, match="fix_comp"):
        mf.veff_percentiles(device=False, volumes="per_draw")
