"""VeffLF on the device (lf_veff) against the host implementation and against the reference's own seeded results
(tests/golden/veff_*.npz, recorded from LumFuncMCMC.VeffLF: lumfuncmcmc.py:515-525, VmaxLumFunc.py:235-257, :304-378)."""
import os

import numpy as np
import pytest

from lf_testlib import synth

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _model(n, seed, mcf, nboot, nbins):
    from lumfuncmcmc_amd.model import LumFuncMCMC
    cat = synth.catalogue(n, seed=seed)
    fi = cat["field_ind"]
    return LumFuncMCMC(synth.split_fields(cat["z"], fi), lum=synth.split_fields(cat["lum"], fi),
                       lum_e=synth.split_fields(cat["lum_e"], fi), Flim=list(synth.FLIM), alpha=synth.ALPHA_C,
                       Omega_0=list(synth.OMEGA_0), sch_al=synth.SCH_AL, sch_al_lims=synth.SCH_AL_LIMS, Lstar=synth.LSTAR,
                       Lstar_lims=synth.LSTAR_LIMS, phistar=synth.PHISTAR, phistar_lims=synth.PHISTAR_LIMS, Lc=synth.LC,
                       Lh=synth.LH, nwalkers=32, nsteps=10, min_comp_frac=mcf, field_ind=fi, Flim_lims=synth.FLIM_LIMS,
                       alpha_lims=synth.ALPHA_LIMS, nboot=nboot, nbins=nbins)


@pytest.mark.parametrize("name", ["veff_n1000", "veff_n200_mcf50"])
def test_device_veff_reproduces_the_reference_under_its_own_seed(name):
    """Weights, binned LF and bootstrap variances of the reference, through the device kernels: the resample indices
    are the reference's own (np.random.seed(rseed); one randint(N, size=N) per resample) handed to lf_veff."""
    from lumfuncmcmc_amd import veff
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    n, nboot, nbins, mcf = len(g["lum"]), int(g["nboot"]), int(g["nbins"]), float(g["min_comp_frac"])
    o = _model(n, int(g["seed"]), mcf, nboot, nbins)
    np.testing.assert_array_equal(o.lum, g["lum"])
    o.getFlim()
    if mcf <= 0.001:
        zmaxval = o.zmax
    else:
        from lumfuncmcmc_amd.cosmology import cosmo
        zmaxval = np.minimum(o.zmax, veff.max_redshift(10 ** o.lum, o.rootsf.ev(o.Flims_arr, o.alpha), cosmo))
    vol = veff.comoving_volume(o.dVdzf, o.zmin, zmaxval)
    np.random.seed(int(g["rseed"]))
    idx = np.array([np.random.randint(n, size=n) for _ in range(nboot)])
    phi, Lavg, lfbin, var = veff.veff_device(o.lum, o.flux, 1.0e-17 * o.Flims_arr, vol, sum(o.Omega_0), o.alpha, o.fcmin,
                                             nboot=nboot, nbin=nbins, boot_idx=idx)
    # (per-source z_max: the reference's adaptive quadrature of an interpolant agrees with the exact integral to ~1e-8)
    tol = 1e-12 if mcf <= 0.001 else 5e-7
    np.testing.assert_allclose(phi, g["phifunc"], rtol=tol)
    np.testing.assert_allclose(Lavg, g["Lavg"], rtol=1e-14)
    np.testing.assert_allclose(lfbin, g["lfbinorig"], rtol=tol)
    np.testing.assert_allclose(var, g["var"], rtol=max(tol, 1e-9))
    o.close()


def test_device_veff_against_the_host_at_catalogue_size():
    from lumfuncmcmc_amd import veff
    n = 400000
    o = _model(n, 3, 0.0, 60, 40)
    o.VeffLF(device=False)
    host = (o.phifunc.copy(), o.lfbinorig.copy(), o.var.copy())
    np.random.seed(5)
    o.VeffLF(device=True)
    np.testing.assert_allclose(o.phifunc, host[0], rtol=1e-13)
    np.testing.assert_allclose(o.lfbinorig, host[1], rtol=1e-12)       # (atomic adds: summation order)
    # different random streams: the two bootstrap variances agree as two draws of the same estimator do
    ok = host[1] > 0
    ratio = o.var[ok] / host[2][ok]
    assert 0.5 < np.median(ratio) < 2.0 and np.all(ratio > 0.1) and np.all(ratio < 10.0), ratio
    o.close()


def test_resampling_indices_outside_the_catalogue_are_refused():
    """boot_idx addresses the weights on the device: an index outside [0, n) is an argument error, not a stray read"""
    from lumfuncmcmc_amd import capi
    n = 1000
    rng = np.random.default_rng(1)
    flux, flim = rng.uniform(2e-17, 9e-17, n), np.full(n, 2.7e-17)
    bins = rng.integers(0, 10, n)
    for bad in (-1, n, 2 ** 40):
        idx = rng.integers(0, n, (3, n))
        idx[1, 17] = bad
        with pytest.raises(capi.LFError):
            capi.veff_device(flux, flim, 1.0e6, 0.04, 4.56, 0.1, bin_of=bins, nbin=10, nboot=3, boot_idx=idx)
    phi, sums = capi.veff_device(flux, flim, 1.0e6, 0.04, 4.56, 0.1, bin_of=bins, nbin=10, nboot=3, boot_idx=rng.integers(0, n, (3, n)))
    assert np.isfinite(phi).all() and sums.shape == (4, 10)


# ---------------------------------------------------------------------------------------------- the device-drawn bootstrap, replayed
def replayed_indices(n, nboot, seed):
    """idx[k - 1][j] of veff_bins (csrc/lf_kernels.h) for resample k = 1 .. nboot: Philox4x32-10 with counter (j lo, j hi, k,
    0x5eed) and key (seed lo, seed hi); floor(u53(r0, r1) n), clamped to n - 1"""
    from lumfuncmcmc_amd import philox
    j = np.arange(n, dtype=np.uint64)
    out = np.empty((nboot, n), dtype=np.int64)
    for k in range(1, nboot + 1):
        r = philox.philox4x32(j & np.uint64(philox.MASK), j >> np.uint64(32), np.full(n, k, dtype=np.uint64),
                              np.full(n, 0x5eed, dtype=np.uint64), seed & philox.MASK, (seed >> 32) & philox.MASK)
        out[k - 1] = np.minimum((philox.u53(r[0], r[1]) * float(n)).astype(np.int64), n - 1)
    return out


@pytest.mark.parametrize("n", [3000, 300001])
def test_device_drawn_bootstrap_is_the_replayed_one(n):
    """lf_veff with boot_idx == NULL (the form VeffLF(device=True) uses) draws its resampling indices on the device.  The same
    indices replayed on the host and handed back through boot_idx give the same binned sums - the order of the atomic adds
    differs, nothing else does - and both are the bincount over the replayed indices (math.fsum), to 1e-13 sum|phi| per bin.
    n = 300001 is past the 1024 x 256 span of the grid-stride loop; some sources have no bin and some no volume."""
    import math
    from lumfuncmcmc_amd import capi
    nbin, nboot, seed = 7, 3, (0x1234 << 32) | 0x9abcdef1
    rng = np.random.default_rng(n)
    flim = rng.uniform(2.0e-17, 4.0e-17, n)
    flux = flim * 10.0 ** rng.uniform(-0.3, 1.5, n)
    vol = rng.uniform(1.0e5, 5.0e6, n)
    vol[rng.permutation(n)[:9]] = np.repeat([0.0, -1.0, -3.5], 3)
    bin_of = rng.integers(-1, nbin + 2, n)
    assert (bin_of < 0).sum() > 100 and (bin_of >= nbin).sum() > 100
    idx = replayed_indices(n, nboot, seed)
    assert idx.min() >= 0 and idx.max() < n
    args = (flux, flim, vol, 0.04, 4.56, 0.1)
    phi, drawn = capi.veff_device(*args, bin_of=bin_of, nbin=nbin, nboot=nboot, seed=seed)
    phi2, given = capi.veff_device(*args, bin_of=bin_of, nbin=nbin, nboot=nboot, boot_idx=idx, seed=99)
    assert np.array_equal(phi, phi2) and np.all(phi[vol <= 0] == 0.0) and np.all(phi[vol > 0] > 0.0)
    want, scale = np.zeros((nboot + 1, nbin)), np.zeros((nboot + 1, nbin))
    for k in range(nboot + 1):
        sel = np.arange(n) if k == 0 else idx[k - 1]
        b, p = bin_of[sel], phi[sel]
        for q in range(nbin):
            want[k, q] = math.fsum(p[b == q])
            scale[k, q] = math.fsum(np.abs(p[b == q]))
    tol = 1e-13 * scale
    print("n %d: max |drawn - given| / bound %.3g, |drawn - bincount| / bound %.3g" %
          (n, (np.abs(drawn - given) / tol).max(), (np.abs(drawn - want) / tol).max()))
    assert np.all(scale > 0) and np.all(np.abs(drawn - given) <= tol) and np.all(np.abs(drawn - want) <= tol) and np.all(np.abs(given - want) <= tol)
    # another seed: other resamples, the catalogue's own row unchanged
    _, other = capi.veff_device(*args, bin_of=bin_of, nbin=nbin, nboot=nboot, seed=seed + 1)
    assert np.all(np.abs(other[0] - drawn[0]) <= tol[0]) and np.all(other[1:] != drawn[1:])


def test_weights_element_by_element_against_40_digits():
    """veff_weights against 40-digit values of 1 / (pref0 fleming(f, Flim, alpha, fcmin) vol) (tests/lf_gradproblib.py:
    case_veff): f / Flim from 1e-3 to 1e3, alpha 0.6, 4.56 and 10, fcmin 0.1 and 0 (the plain Fleming curve), vol per source
    and vol = NULL with vol_all; vol_i <= 0 gives exactly 0.  The kernel keeps the reference's 0.5 (1 + num / sqrt(1 + num^2)),
    which cancels for num << 0: the yardstick 2^-53 |phi| (1 + 1 / fc) carries that, times 1 + |ln fc / d| for fcmin > 0.
    Cap: max(2, 4 x the figure of hostsetup.fleming's NumPy expression), measured on the CPU by tests/test_gradterms_cpu.py
    (1.456 on 2026-10-19: lf_gradproblib.CAPS["veff_phi"] = 5.83)."""
    import lf_gradproblib as P
    from lumfuncmcmc_amd import capi
    worst = 0.0
    for cfg in P.veff_cases():
        c = P.case_veff(*cfg)
        phi, _ = capi.veff_device(c["flux"], c["flim"], c["vol"], P.VEFF_PREF0, c["alpha"], c["fcmin"])
        fig, i = P.measure(c, phi)
        print("veff_phi alpha %-5g fcmin %-4g vol %-10s device max err / yard %7.3f (cap %g) at f / Flim = %r: got %.17g ref %.17g" %
              (cfg[0], cfg[1], "per source" if cfg[2] else "shared", fig, P.CAPS["veff_phi"], c["flux"][i] / c["flim"][i], phi[i], c["ref"][0][i]))
        assert np.all(phi[c["zero"]] == 0.0) and not np.any(np.signbit(phi[c["zero"]]))
        worst = max(worst, fig)
    assert worst <= P.CAPS["veff_phi"], worst
