"""The 1/Veff points in redshift slices without a GPU: the equal-count edges against an independent
restatement, slice membership at the edges, the tie of the NumPy twin to boot_err_log / lumfunc_weights (which are pinned to the
reference's fixtures), the slice volumes against comoving_volume, the refusals of the C entry (made before the device is touched)
and the slice average of the model band."""
import ctypes

import numpy as np
import pytest

from lf_sliceslib import PIVOTS, model as _model, zmodel as _zmodel
from lumfuncmcmc_amd import capi, hostsetup as hs, lfbands, veff


# ---------------------------------------------------------------------------------------------- the edges
def _edges_restated(z, S):
    """the rule of the design, source by source: rank by a stable sort, slice floor(r S / N), inner edges half way between"""
    N = len(z)
    ranked = sorted(range(N), key=lambda i: (z[i], i))
    members = [[] for _ in range(S)]
    for r, i in enumerate(ranked):
        members[(r * S) // N].append(z[i])
    e = [min(z)]
    for s in range(S - 1):
        e.append((max(members[s]) + min(members[s + 1])) / 2.0)
    return np.array(e + [max(z)])


@pytest.mark.parametrize("case", ["n7s3", "ties", "s1", "sN"])
def test_slice_edges_against_an_independent_restatement(case):
    rng = np.random.default_rng(3)
    if case == "n7s3":
        z, S = rng.uniform(1.2, 1.9, 7), 3
    elif case == "ties":
        z, S = np.array([1.3, 1.5, 1.5, 1.5, 1.2, 1.8, 1.5, 1.8, 1.25, 1.3]), 4
    elif case == "s1":
        z, S = rng.uniform(1.2, 1.9, 31), 1
    else:
        z, S = rng.uniform(1.2, 1.9, 9), 9
    got = veff.slice_edges(z, S)
    assert got.shape == (S + 1,) and np.array_equal(got, _edges_restated(list(z), S))
    if case != "ties":
        so = veff.slice_index(z, got)
        cnt = np.bincount(so, minlength=S)
        assert so.min() >= 0 and cnt.max() - cnt.min() <= 1
    with pytest.raises(ValueError):
        veff.slice_edges(z, len(z) + 1)


def test_slice_membership_at_the_edges():
    e = np.array([1.2, 1.4, 1.55, 1.9])
    z = np.array([e[0], e[1], e[2], e[3], np.nextafter(e[0], 0.0), np.nextafter(e[3], 9.0), np.nextafter(e[1], 0.0),
                  np.nextafter(e[3], 0.0), np.nan])
    assert veff.slice_index(z, e).tolist() == [0, 1, 2, 2, -1, -1, 0, 2, -1]
    for bad in ([1.2], [1.2, 1.2], [1.3, 1.2], np.linspace(1.0, 2.0, 66)):
        with pytest.raises(ValueError):
            veff.slice_index(z, bad)


# ---------------------------------------------------------------------------------------------- the tie to the pinned path
def test_one_slice_is_the_pinned_estimator_bit_for_bit():
    """One slice [zmin, zmax] with boot_idx from a seeded np.random.randint stream: lf and var are boot_err_log's under the
    same seed, phi is lumfunc_weights', bit for bit."""
    m = _zmodel(n=1500, mcf=0.5)
    zmaxval = m._veff_zmaxval()
    assert np.ndim(zmaxval) == 1 and zmaxval.min() < m.zmax
    nboot, nbin, n = 30, 25, m.lum.size
    flim = 1.0e-17 * m.Flims_arr
    phi_ref = veff.lumfunc_weights(m.flux, m.dVdzf, sum(m.Omega_0), m.zmin, zmaxval, flim, m.alpha, m.fcmin)
    np.random.seed(99)
    Lavg_ref, lf_ref, var_ref = veff.boot_err_log(m.lum, phi_ref, nboot, nbin)
    np.random.seed(99)
    idx = np.array([np.random.randint(n, size=n) for _ in range(nboot)])
    edges = np.array([m.zmin, m.zmax])
    so = veff.slice_index(m.z, edges)
    assert np.all(so == 0)
    vol = veff.slice_volumes(m.dVdzf, edges, so, zmaxval)
    phi, Lavg, lf, var, counts, n_slice = veff.veff_slices_host(m.lum, m.flux, flim, vol, so, 1, sum(m.Omega_0), m.alpha, m.fcmin,
                                                                nboot=nboot, nbin=nbin, boot_idx=idx)
    assert np.array_equal(phi, phi_ref) and np.any(phi == 0.0) and np.any(phi > 0.0)
    assert np.array_equal(Lavg[0], Lavg_ref) and np.array_equal(lf[0], lf_ref) and np.array_equal(var[0], var_ref)
    inbins = (m.lum >= min(m.lum) * 1.001) & (m.lum < max(m.lum))       # (the brightest and the faintest sources fall in no bin)
    assert n_slice.tolist() == [n] and counts.sum() == inbins.sum() < n


def test_twin_draws_its_slices_independently_and_keeps_an_empty_slice_at_zero():
    rng = np.random.default_rng(5)
    n, S, nbin, nboot = 700, 4, 6, 5
    so = rng.integers(-1, S, n).astype(np.int32)
    so[so == 2] = 3                                   # slice 2 is empty
    bins = rng.integers(-1, nbin + 1, n)
    phi = rng.uniform(0.5, 2.0, n)
    sums, counts, n_slice = veff.veff_slices(phi, so, S, bins, nbin, nboot=nboot, seed=7)
    assert n_slice[2] == 0 and np.all(sums[:, 2] == 0.0) and np.all(counts[2] == 0)
    for s in (0, 1, 3):
        sel = so == s
        assert np.array_equal(counts[s], np.bincount(bins[sel & (bins >= 0) & (bins < nbin)], minlength=nbin))
        np.testing.assert_allclose(sums[0, s], np.bincount(bins[sel & (bins >= 0) & (bins < nbin)],
                                                           weights=phi[sel & (bins >= 0) & (bins < nbin)], minlength=nbin), rtol=1e-13)
    # another slice's sources do not move a slice's resamples: slices 0 and 1 alone give the same rows
    keep = so != 3
    sums2, _, _ = veff.veff_slices(phi[keep], so[keep], S, bins[keep], nbin, nboot=nboot, seed=7)
    assert np.array_equal(sums2[:, :2], sums[:, :2]) and not np.array_equal(sums[1, 0], sums[2, 0])
    lf, var = veff.slice_variance(sums, np.full(S, 0.1))
    assert np.all(var[2] == 0.0) and np.all(var[[0, 1, 3]] > 0.0)
    assert np.all(veff.slice_variance(sums[:2], np.full(S, 0.1))[1] == 0.0)          # one resample: no variance, no raise


# ---------------------------------------------------------------------------------------------- volumes
def test_slice_volumes_add_up_to_the_comoving_volume():
    m = _zmodel(n=1200, mcf=0.5)
    zmaxval = m._veff_zmaxval()
    edges = veff.slice_edges(m.z, 5)
    assert edges[0] == m.zmin and edges[-1] == m.zmax
    so = veff.slice_index(m.z, edges)
    total = veff.comoving_volume(m.dVdzf, m.zmin, zmaxval)
    # the slice that holds z_max and every slice below it (a slice above z_max has no volume): together the whole volume
    acc = np.zeros(m.z.size)
    for s in range(5):
        part = veff.slice_volumes(m.dVdzf, edges, np.full(m.z.size, s), zmaxval)
        assert np.all(part[zmaxval <= edges[s]] == 0.0) and np.all(part[zmaxval > edges[s]] > 0.0)
        acc += part
    inner = (zmaxval > edges[1]) & (zmaxval < m.zmax)
    assert inner.sum() > 100 and (zmaxval == m.zmax).sum() > 100
    print("slices' volumes against the whole: max %.2f ulp" % np.max(np.abs(acc - total) / np.spacing(total)))
    assert np.all(np.abs(acc - total) <= 4 * np.spacing(total))
    own = veff.slice_volumes(m.dVdzf, edges, so, zmaxval)
    below = zmaxval <= edges[so]
    assert below.any() and np.all(own[below] == 0.0) and np.all(own[~below] > 0.0)
    # a scalar z_max and a source without a slice: the whole range
    whole = veff.slice_volumes(m.dVdzf, edges, np.array([-1, -1]), m.zmax)
    assert np.all(np.abs(whole - veff.comoving_volume(m.dVdzf, m.zmin, np.full(2, m.zmax))) <= 4 * np.spacing(whole))


# ---------------------------------------------------------------------------------------------- refusals
def _args(n=50, S=3, nbin=4, nboot=2, boot=False):
    rng = np.random.default_rng(1)
    so = (np.arange(n) % S).astype(np.int32)
    so[:5] = -1
    so[5:12] = 0                                      # slice 0 is the largest
    a = {"flux": rng.uniform(2e-17, 9e-17, n), "flim": np.full(n, 2.7e-17), "vol": rng.uniform(1e5, 1e6, n), "pref0": 0.04,
         "alpha": 4.56, "fcmin": 0.1, "slice_of": so, "nslice": S, "bin_of": rng.integers(0, nbin, n).astype(np.int32), "nbin": nbin,
         "nboot": nboot, "boot_idx": None, "seed": 3}
    if boot:
        order, off = veff.slice_sort(so, S)
        ns = np.diff(off)[so[order]]
        a["boot_idx"] = (rng.integers(0, 1 << 30, (nboot, order.size)) % ns).astype(np.int64)
    return a


def _call(a, device=1 << 20, null=()):
    """lf_veff_slices as it stands in the library, on a device that does not exist: a call that passes the checks gets as far
    as choosing the device (not LF_ERR_ARG), a refused one never does"""
    lib = capi.load()
    dp, ip, lp = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64)
    n = a["flux"].size
    m = int((a["slice_of"] >= 0).sum())
    out = {"phi": np.zeros(n), "sums": np.zeros((max(a["nboot"], 0) + 1) * 64 * 64), "counts": np.zeros(64 * 64, dtype=np.int64)}
    assert a["boot_idx"] is None or a["boot_idx"].shape == (a["nboot"], m)

    def p(name, arr, t):
        return None if name in null else np.ascontiguousarray(arr).ctypes.data_as(t)
    return lib.lf_veff_slices(device, a.get("n", n), p("flux", a["flux"], dp), p("flim", a["flim"], dp), p("vol", a["vol"], dp), a["pref0"],
                              a["alpha"], a["fcmin"], p("slice_of", a["slice_of"], ip), a["nslice"], p("bin_of", a["bin_of"], ip),
                              a["nbin"], a["nboot"], None if a["boot_idx"] is None else a["boot_idx"].ctypes.data_as(lp),
                              ctypes.c_uint64(a["seed"]), p("phi", out["phi"], dp), p("sums", out["sums"], dp),
                              p("counts", out["counts"], lp))


def test_bad_arguments_are_refused_before_the_device():
    assert capi.veff_slices_ms() == -1.0 or capi.veff_slices_ms() > 0.0
    good = _call(_args())
    assert good != capi.LF_ERR_ARG and good != capi.LF_OK          # no such device: the checks were passed
    assert _call(_args(boot=True)) == good
    for name in ("flux", "flim", "vol", "slice_of", "bin_of", "phi", "sums", "counts"):
        assert _call(_args(), null=(name,)) == capi.LF_ERR_ARG, name
    for key, bad in (("n", 0), ("n", -3), ("nslice", 0), ("nslice", 65), ("nbin", 0), ("nbin", 65), ("nboot", -1), ("nboot", 10001),
                     ("pref0", 0.0), ("pref0", -1.0), ("pref0", float("nan"))):
        a = _args()
        a[key] = bad
        assert _call(a) == capi.LF_ERR_ARG, (key, bad)
    for key, ok in (("nslice", 64), ("nbin", 64), ("nboot", 0)):
        a = _args()
        a[key] = ok
        assert _call(a) == good, (key, ok)
    a = _args(nboot=10000)
    assert _call(a) == good
    # boot_idx: a draw outside its own slice's [0, n_s) - also one that another, larger slice would hold
    base = _args(boot=True)
    order, off = veff.slice_sort(base["slice_of"], 3)
    n_s = np.diff(off)
    assert n_s[0] > n_s[2]
    for pos, bad in ((0, -1), (0, int(n_s[0])), (int(off[2]), int(n_s[2])), (int(off[3]) - 1, 1 << 40)):
        a = _args(boot=True)
        a["boot_idx"][1, pos] = bad
        assert _call(a) == capi.LF_ERR_ARG, (pos, bad)
    with pytest.raises(capi.LFError):
        capi.veff_slices(base["flux"], base["flim"], base["vol"], 0.04, 4.56, 0.1, base["slice_of"], 3, base["bin_of"], 65)


# ---------------------------------------------------------------------------------------------- the model band
def _slice_average(m, edges, Lavg, recs, G):
    zg, wg = veff.slice_nodes(edges, G)
    S, nb = zg.shape[0], Lavg.shape[1]
    Lp = np.broadcast_to(Lavg[:, None, :], (S, G, nb)).ravel()
    zp = np.broadcast_to(zg[:, :, None], (S, G, nb)).ravel()
    v = lfbands.lf_values("zevol", recs, Lp, z=zp).reshape(-1, S, G, nb)
    return veff.slice_model_average(v, wg * m.dVdzf(zg))


def test_slice_average_without_evolution_is_the_plain_schechter():
    m = _zmodel()
    edges = veff.slice_edges(m.z, 5)
    Lavg = np.tile(np.linspace(41.2, 43.4, 25), (5, 1))
    rows = np.array([[42.6, 42.6, 42.6, -2.2, -2.2, -2.2, -1.45]])
    recs = lfbands.pack_draws("zevol", rows, pivots=PIVOTS)
    got = _slice_average(m, edges, Lavg, recs, m.SLICE_NODES)[0]
    want = hs.true_lum_func(Lavg, -1.45, 42.6, -2.2)
    print("equal pivots: max relative difference %.3g" % np.max(np.abs(got / want - 1.0)))
    assert np.all(np.abs(got - want) <= 1e-14 * want)


def test_eight_nodes_per_slice_agree_with_thirty_two():
    """DESIGN.md section 3.36 states the bound: below 1e-6 relative on the z-evolving posterior cloud of _zmodel, five
    equal-count slices, the bins of the catalogue."""
    m = _zmodel()
    edges = veff.slice_edges(m.z, 5)
    _, Lavg, _, _ = veff.luminosity_bins(m.lum, 25)
    Lavg = np.tile(Lavg, (5, 1))
    recs = lfbands.pack_draws("zevol", m.samples[:, :-1], pivots=PIVOTS)
    a, b = _slice_average(m, edges, Lavg, recs, m.SLICE_NODES), _slice_average(m, edges, Lavg, recs, 32)
    rel = np.max(np.abs(a - b) / b)
    print("G = %d against G = 32: max relative difference %.3g" % (m.SLICE_NODES, rel))
    assert m.SLICE_NODES == 8 and rel < 1e-6


def test_model_surface_on_the_host():
    m = _zmodel(n=2000)
    before = (getattr(m, "Lavg", None), getattr(m, "lfbinorig", None), getattr(m, "var", None))
    np.random.seed(4)
    r = m.veff_slices(z_edges=3, device=False, ndraws=40)
    assert r["z_edges"].shape == (4,) and r["Lavg"].shape == r["lf"].shape == r["var"].shape == r["counts"].shape == (3, 25)
    assert r["model"].shape == (3, 3, 25) and r["n_slice"].sum() == 2000 and np.all(r["model"][0] <= r["model"][2])
    assert (getattr(m, "Lavg", None), getattr(m, "lfbinorig", None), getattr(m, "var", None)) == before
    np.random.seed(4)
    again = m.veff_slices(z_edges=r["z_edges"], device=False, model=False)
    assert again["seed"] == r["seed"] and np.array_equal(again["lf"], r["lf"]) and np.array_equal(again["var"], r["var"]) and "model" not in again
    own = m.veff_slices(z_edges="auto", bins="slice", device=False, model=False)
    assert own["Lavg"].shape == (5, 25) and not np.array_equal(own["Lavg"][0], own["Lavg"][4])
    with pytest.raises(ValueError):
        m.veff_slices(z_edges=[m.zmin - 0.1, m.zmax], device=False, model=False)


def test_single_schechter_band_is_lf_percentiles_at_the_bin_centres():
    m = _model(n=1500)
    np.random.seed(8)
    r = m.veff_slices(z_edges=2, device=False, ndraws=30)
    np.random.seed(8)
    np.random.randint(0, 2 ** 31 - 1)                      # (the bootstrap's seed is drawn first)
    want = m.lf_percentiles(logL=r["Lavg"].ravel(), ndraws=30, device=False)
    assert r["model"].shape == (3, 2, 25) and np.array_equal(r["model"].reshape(3, -1), want)
    assert np.array_equal(r["Lavg"][0], r["Lavg"][1]) and r["n_slice"].tolist() == [750, 750]
