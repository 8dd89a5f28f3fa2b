"""lf_veff_slices on the device (csrc/lf_veffslices.h) against its NumPy twin (veff.veff_slices).

The bound of the sums, derived and not measured: a sum of n_s non-negative terms, added in any order in fp64, lies within
(n_s - 1) 2^-53 relative of the exact sum, on the device and in the twin alike; the test allows four times that,
|dev - twin| <= n_s 2^-51 twin per (resample, slice, bin).  With integer-valued weights every partial sum is exact, and the
device must then give the twin's bits: that pins Philox, the counter layout, the clamp to n_s - 1 and the slice offsets.

One catalogue serves the tests: slices of 0, 1, CHUNK - 1, CHUNK, CHUNK + 1 and 2 CHUNK + 1 sources (S = 6), sources without a
slice, sources without a bin and sources without a volume."""
import numpy as np
import pytest

from lf_sliceslib import model as _model, zmodel as _zmodel
from lumfuncmcmc_amd import capi, hostsetup as hs, veff

pytestmark = pytest.mark.gpu

C = veff.SLICES_CHUNK
SIZES = (0, 1, C - 1, C, C + 1, 2 * C + 1)
S = len(SIZES)
PREF0, ALPHA, FCMIN = 0.04, 4.56, 0.1
SEED = (0x2468 << 32) | 0x13579bdf


@pytest.fixture(scope="module")
def cat():
    """the catalogue, in a shuffled order (the device sorts by slice), with a bin index for the widest case, 64 bins"""
    rng = np.random.default_rng(20261021)
    so = np.concatenate([np.full(k, s) for s, k in enumerate(SIZES)] + [np.full(60, -1), np.full(40, S), np.full(11, 1000)])
    so = so[rng.permutation(so.size)].astype(np.int32)
    n = so.size
    flim = rng.uniform(2.0e-17, 4.0e-17, n)
    flux = flim * 10.0 ** rng.uniform(-0.3, 1.5, n)
    vol = rng.uniform(1.0e5, 5.0e6, n)
    vol[rng.permutation(n)[:90]] = np.repeat([0.0, -1.0, -3.5], 30)
    bin64 = rng.integers(-2, 64 + 3, n).astype(np.int32)
    return {"n": n, "slice_of": so, "flux": flux, "flim": flim, "vol": vol, "bin64": bin64}


def _bins(cat, nbin):
    """bin_of for nbin bins: the 64-bin index folded, its overflow kept outside [0, nbin)"""
    b = cat["bin64"].copy()
    ok = (b >= 0) & (b < 64)
    b[ok] = b[ok] % nbin
    return b


def _bound(n_slice, twin):
    return n_slice[None, :, None] * 2.0 ** -51 * twin


def _device(cat, bin_of, nbin, nboot, **kw):
    return capi.veff_slices(cat["flux"], cat["flim"], cat["vol"], PREF0, ALPHA, FCMIN, cat["slice_of"], S, bin_of, nbin, nboot=nboot, **kw)


def test_index_stream_exactly(cat):
    """flux = 10 Flim with alpha = 1e9 and the plain Fleming curve make fc exactly 1 (num / sqrt(1 + num^2) rounds to 1), so with
    pref0 = 1 and vol a power of two phi = 1 / vol is a small integer: every sum is exact in any order."""
    rng = np.random.default_rng(1)
    n, nbin, nboot = cat["n"], 25, 7
    vol = rng.choice([1.0, 0.5, 0.25, 0.125, 0.0], n)
    bin_of = _bins(cat, nbin)
    phi, sums, counts = capi.veff_slices(10.0 * cat["flim"], cat["flim"], vol, 1.0, 1.0e9, 0.0, cat["slice_of"], S, bin_of, nbin,
                                         nboot=nboot, seed=SEED)
    with np.errstate(divide="ignore"):
        assert np.array_equal(phi, np.where(vol > 0, 1.0 / vol, 0.0))
    tw, tc, n_slice = veff.veff_slices(phi, cat["slice_of"], S, bin_of, nbin, nboot=nboot, seed=SEED)
    assert n_slice.tolist() == list(SIZES)
    assert np.array_equal(sums, tw) and np.array_equal(counts, tc)
    assert np.all(sums[:, 0] == 0.0) and sums[0].sum() == phi[(cat["slice_of"] >= 0) & (cat["slice_of"] < S) & (bin_of >= 0) & (bin_of < nbin)].sum()
    other = capi.veff_slices(10.0 * cat["flim"], cat["flim"], vol, 1.0, 1.0e9, 0.0, cat["slice_of"], S, bin_of, nbin, nboot=nboot,
                             seed=SEED + 1)[1]
    assert np.array_equal(other[0], sums[0]) and not np.array_equal(other[1:, 2:], sums[1:, 2:])


@pytest.mark.parametrize("nboot", [0, 1, 7])
@pytest.mark.parametrize("nbin", [1, 25, 64])
def test_sums_against_the_twin(cat, nbin, nboot):
    bin_of = _bins(cat, nbin)
    assert (bin_of < 0).sum() > 50 and (bin_of >= nbin).sum() > 50
    phi, sums, counts = _device(cat, bin_of, nbin, nboot, seed=SEED)
    assert sums.shape == (nboot + 1, S, nbin) and counts.shape == (S, nbin) and counts.dtype == np.int64
    assert np.all(phi[cat["vol"] <= 0] == 0.0) and np.all(phi[cat["vol"] > 0] > 0.0)
    tw, tc, n_slice = veff.veff_slices(phi, cat["slice_of"], S, bin_of, nbin, nboot=nboot, seed=SEED)      # (the device's own phi)
    assert n_slice.tolist() == list(SIZES)
    tol = _bound(n_slice, tw)
    with np.errstate(invalid="ignore", divide="ignore"):
        print("nbin %d nboot %d: max |dev - twin| / bound %.3g" % (nbin, nboot, np.nanmax(np.where(tol > 0, np.abs(sums - tw) / tol, 0.0))))
    assert np.all(np.abs(sums - tw) <= tol) and np.all(tw[:, 2:].sum(axis=2) > 0)
    # counts: np.bincount, exactly
    for s in range(S):
        sel = (cat["slice_of"] == s) & (bin_of >= 0) & (bin_of < nbin)
        assert np.array_equal(counts[s], np.bincount(bin_of[sel], minlength=nbin)), s
    assert np.array_equal(counts, tc)


def test_two_calls_give_the_same_bits(cat):
    bin_of = _bins(cat, 25)
    a = _device(cat, bin_of, 25, 7, seed=SEED)
    b = _device(cat, bin_of, 25, 7, seed=SEED)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    assert capi.veff_slices_ms() > 0.0


def test_weights_against_lumfunc_weights():
    """phi with one slice [zmin, zmax] and a z_max per source against veff.lumfunc_weights, at the tolerance tests/test_gpu_veff.py
    holds lf_veff's phi to against the host (rtol 1e-13)"""
    m = _zmodel(n=3000, mcf=0.5)
    zmaxval = m._veff_zmaxval()
    flim = 1.0e-17 * m.Flims_arr
    want = veff.lumfunc_weights(m.flux, m.dVdzf, sum(m.Omega_0), m.zmin, zmaxval, flim, m.alpha, m.fcmin)
    edges = np.array([m.zmin, m.zmax])
    so = veff.slice_index(m.z, edges)
    vol = veff.slice_volumes(m.dVdzf, edges, so, zmaxval)
    phi = veff.veff_slices_device(m.lum, m.flux, flim, vol, so, 1, sum(m.Omega_0), m.alpha, m.fcmin, nboot=2, nbin=25, seed=1)[0]
    assert np.any(want == 0.0) and np.array_equal(phi == 0.0, want == 0.0)
    np.testing.assert_allclose(phi, want, rtol=1e-13)


def test_the_callers_indices(cat):
    """boot_idx reproduces the twin under the same bound; handing the device's own draws back gives the drawn sums' bits"""
    nbin, nboot = 25, 3
    bin_of = _bins(cat, nbin)
    order, off = veff.slice_sort(cat["slice_of"], S)
    n_of = np.diff(off)[cat["slice_of"][order]]
    rng = np.random.default_rng(9)
    idx = (rng.integers(0, 1 << 40, (nboot, order.size)) % n_of).astype(np.int64)
    phi, sums, _ = _device(cat, bin_of, nbin, nboot, boot_idx=idx, seed=5)
    tw, _, n_slice = veff.veff_slices(phi, cat["slice_of"], S, bin_of, nbin, nboot=nboot, boot_idx=idx)
    assert np.all(np.abs(sums - tw) <= _bound(n_slice, tw))
    replay = np.zeros_like(idx)
    for s in range(S):
        for k in range(1, nboot + 1):
            replay[k - 1, off[s]:off[s + 1]] = veff.slice_boot_indices(int(n_slice[s]), s, k, SEED)
    drawn = _device(cat, bin_of, nbin, nboot, seed=SEED)[1]
    given = _device(cat, bin_of, nbin, nboot, boot_idx=replay, seed=0)[1]
    assert np.array_equal(drawn, given)
    bad = idx.copy()
    bad[1, off[3]] = n_slice[3]                       # inside the catalogue, outside its slice
    with pytest.raises(capi.LFError):
        _device(cat, bin_of, nbin, nboot, boot_idx=bad)


def test_one_slice_agrees_with_lf_veff_on_the_same_indices(cat):
    """S = 1 with every source in the slice: the caller's indices are lf_veff's own; the two kernels differ in the order of their
    sums only - n 2^-51 relative"""
    n, nbin, nboot = 3 * C - 5, 25, 3
    rng = np.random.default_rng(4)
    flux, flim, vol = cat["flux"][:n], cat["flim"][:n], cat["vol"][:n]
    bin_of = _bins(cat, nbin)[:n]
    idx = rng.integers(0, n, (nboot, n))
    phi, sums, _ = capi.veff_slices(flux, flim, vol, PREF0, ALPHA, FCMIN, np.zeros(n, dtype=np.int32), 1, bin_of, nbin, nboot=nboot, boot_idx=idx)
    phi0, sums0 = capi.veff_device(flux, flim, vol, PREF0, ALPHA, FCMIN, bin_of=bin_of, nbin=nbin, nboot=nboot, boot_idx=idx)
    assert np.array_equal(phi, phi0)
    assert np.all(sums0 > 0) and np.all(np.abs(sums[:, 0] - sums0) <= n * 2.0 ** -51 * sums0)


@pytest.mark.parametrize("kind", ["zevol", "free"])
def test_model_level_device_and_host_agree(kind):
    """veff_slices(z_edges=3) on a 2000-source catalogue, device=True against device=False under the same numpy seed (the same
    posterior draws, the same bootstrap seed).  lf: the bound of the sums (the division by dL is the same on both sides).
    var: each resample's value moves by at most d = bound x its largest value, a deviation from the mean by 2 d, so
    |var_d - var_h| <= 4 d sqrt(nboot / (nboot - 1)) sqrt(var) + 4 d^2 nboot / (nboot - 1) (Cauchy-Schwarz on sum |dev_k|).
    model: the band kernels' own tolerance against the host (tests/test_gpu_bands.py: rtol 1e-12)."""
    m = _zmodel(n=2000, nboot=20) if kind == "zevol" else _model(n=2000, nboot=20)
    res = {}
    for dev in (False, True):
        np.random.seed(31)
        res[dev] = m.veff_slices(z_edges=3, device=dev, ndraws=50)
    h, d = res[False], res[True]
    assert h["seed"] == d["seed"] and np.array_equal(h["z_edges"], d["z_edges"]) and np.array_equal(h["counts"], d["counts"])
    assert np.array_equal(h["n_slice"], d["n_slice"]) and h["n_slice"].sum() == 2000 and np.array_equal(h["Lavg"], d["Lavg"])
    for r in (h, d):
        assert r["z_edges"].shape == (4,) and r["Lavg"].shape == r["lf"].shape == r["var"].shape == r["counts"].shape == (3, 25)
        assert r["model"].shape == (3, 3, 25) and r["n_slice"].shape == (3,)
    eps = h["n_slice"][:, None] * 2.0 ** -51
    print("%s: lf max |d - h| / bound %.3g" % (kind, np.max(np.abs(d["lf"] - h["lf"]) / np.maximum(eps * h["lf"], 1e-300))))
    assert np.all(np.abs(d["lf"] - h["lf"]) <= eps * h["lf"])
    nb = m.nboot
    # no resample's value of a bin exceeds n_s max(phi) / dL
    so = veff.slice_index(m.z, h["z_edges"])
    phi = veff.slice_weights(m.flux, 1.0e-17 * m.Flims_arr, veff.slice_volumes(m.dVdzf, h["z_edges"], so, m._veff_zmaxval()),
                             sum(m.Omega_0) / hs.SQARCSEC, m.alpha, m.fcmin)
    top = h["n_slice"][:, None] * phi.max() * 1.001 / (h["Lavg"][:, 1:2] - h["Lavg"][:, 0:1])
    dd = eps * top
    assert np.all(np.abs(d["var"] - h["var"]) <= 4 * dd * np.sqrt(nb / (nb - 1.0)) * np.sqrt(h["var"]) + 4 * dd ** 2 * nb / (nb - 1.0))
    np.testing.assert_allclose(d["model"], h["model"], rtol=1e-12)
    m.close()
