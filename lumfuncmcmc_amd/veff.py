"""1/Veff estimator of the binned luminosity function with bootstrap errors (post-fit diagnostic).

Reference: LumFuncMCMC.VeffLF (lumfuncmcmc.py:515-525, lumfuncmcmc_z.py:470-478) ->
V.lumfunc (VmaxLumFunc.py:235-257), V.getMaxz (:761-777), V.getBootErrLog (:304-378).

The reference calls scipy.quad once per source on an integrand whose only z dependence is the
interpolated dV/dz - the completeness is evaluated at the source's OBSERVED flux, a constant of
the integral (VmaxLumFunc.py:215-233).  So the weight of source i is

    phi_i = 1 / ( sum(Omega_0)/sqarcsec * fleming(F_i, Flim_i, alpha) * int_{zmin}^{zmax_i} dV/dz dz )

and with min_comp_frac <= 0.001 the integral is the same for every source: one quadrature instead
of N.  The bootstrap is a bincount per resample instead of nboot x nbins boolean masks over the
catalogue.  Host NumPy is O(N) (N = 10^6: ~1 s; the reference needs N quad calls plus 5000 N-long masks);
`veff_device` does the weights, the binning and the nboot resamples in two HIP kernels (lf_veff).
"""
import numpy as np

from . import hostsetup as hs


def _interp_integral(f, a, b):
    """Exact integral of the piecewise-linear interpolant f (hostsetup.LinearInterp) over [a, b_i]."""
    x, y = f.x, f.y
    seg = 0.5 * (y[1:] + y[:-1]) * np.diff(x)
    cum = np.concatenate([[0.0], np.cumsum(seg)])

    def F(t):
        t = np.asarray(t, dtype=np.float64)
        hi = np.searchsorted(x, t).clip(1, len(x) - 1)
        lo = hi - 1
        yt = f(t)
        return cum[lo] + 0.5 * (y[lo] + yt) * (t - x[lo])
    return F(b) - F(a)


MPC_CM_EXACT = 3.0856775814913673e24      # astropy's Mpc in cm: get_L_constF uses .to('cm'), not the 3.086e24 literal


def max_redshift_fsolve(lum_lin, fmin, cosmo, z0=1.5):
    """The reference's own procedure (V.getMaxz, VmaxLumFunc.py:761-777): one scipy fsolve of
    get_L_constF(fmin, z) - L per source, from z = 1.5.  Kept for the tests; 2 ms per source."""
    from scipy.optimize import fsolve
    out = np.empty(len(lum_lin))
    for i, (L, fm) in enumerate(zip(lum_lin, fmin)):
        out[i] = fsolve(lambda x: 4.0 * np.pi * (cosmo.luminosity_distance(x) * MPC_CM_EXACT) ** 2 * fm - L, z0)[0]
    return out


def redshift_at_distance(target, cosmo, tol=1e-13, maxit=6):
    """DL^-1 of luminosity distances in Mpc (NaN where the distance is not finite and positive): a table gives the first
    guess, Newton steps on the exact DL (secant slope from the table) polish it until the largest step is below tol."""
    target = np.asarray(target, dtype=np.float64)
    out = np.full(target.shape, np.nan)
    good = np.isfinite(target) & (target > 0)
    if not good.any():
        return out
    zhi = 4.0
    while cosmo.luminosity_distance(np.array([zhi]))[0] < target[good].max() and zhi < 1.0e4:
        zhi *= 2.0
    ztab = np.linspace(0.0, zhi, 8193)
    dtab = np.asarray(cosmo.luminosity_distance(ztab))
    slope = np.gradient(dtab, ztab)
    z = np.interp(target[good], dtab, ztab)
    for _ in range(maxit):
        step = (np.asarray(cosmo.luminosity_distance(z)) - target[good]) / np.interp(z, ztab, slope)
        z = np.clip(z - step, 0.0, zhi)
        if np.max(np.abs(step)) < tol * max(1.0, zhi):
            break
    out[good] = z
    return out


def max_redshift(lum_lin, fmin, cosmo, z0=1.5):
    """Redshift at which luminosity lum_lin (erg/s) is seen at flux fmin: the root of
    4 pi (DL(z) Mpc)^2 fmin = L that V.getMaxz finds with fsolve, for all sources at once.  DL is monotonic, so
    the root is DL^-1 of a target distance (redshift_at_distance), polished to 1e-13 - the reference's fsolve stops at
    1.5e-8."""
    lum_lin = np.asarray(lum_lin, dtype=np.float64)
    fmin = np.asarray(fmin, dtype=np.float64)
    return redshift_at_distance(np.sqrt(lum_lin / (4.0 * np.pi * fmin)) / MPC_CM_EXACT, cosmo)


def comoving_volume(dVdzf, zmin, zmaxval):
    """int_{zmin}^{zmax} dV/dz dz of the docstring: one scipy.quad for a scalar zmax (as V.lumfunc evaluates it), the
    exact integral of the interpolant per source otherwise; 0 where zmax <= zmin."""
    if np.ndim(zmaxval) == 0:
        if not zmaxval > zmin:
            return 0.0
        from scipy.integrate import quad
        return quad(lambda z: float(dVdzf(z)), zmin, zmaxval)[0]
    ok = zmaxval > zmin
    return np.where(ok, _interp_integral(dVdzf, zmin, np.where(ok, zmaxval, zmin)), 0.0)


def lumfunc_weights(flux, dVdzf, sum_omega, zmin, zmaxval, flim, alpha, fcmin):
    """phi_i of the docstring.  zmaxval: scalar (shared integral, evaluated with scipy.quad exactly
    as V.lumfunc does) or per-source array (exact integral of the interpolant; the reference's
    adaptive quadrature agrees with it to its own tolerance, ~1e-8)."""
    comp = hs.fleming(flux, flim, alpha, fcmin)
    pref = sum_omega / hs.SQARCSEC * comp
    phi = np.zeros_like(flux)
    if np.ndim(zmaxval) == 0:
        if zmaxval > zmin:
            from scipy.integrate import quad
            vol, _ = quad(lambda z: float(dVdzf(z)), zmin, zmaxval)
            phi = 1.0 / (pref * vol)
        return phi
    ok = zmaxval > zmin
    vol = _interp_integral(dVdzf, zmin, np.where(ok, zmaxval, zmin))
    with np.errstate(divide="ignore"):
        phi[ok] = 1.0 / (pref[ok] * vol[ok])
    return phi


def luminosity_bins(L, nbin):
    """Bin edges, centres, width and the bin index of every source (nbin = no bin) of V.getBootErrLog."""
    L = np.asarray(L, dtype=np.float64)
    Larr = np.linspace(min(L) * 1.001, max(L), nbin + 1)
    Lavg = np.linspace((Larr[0] + Larr[1]) / 2.0, (Larr[-1] + Larr[-2]) / 2.0, len(Larr) - 1)
    idx = np.searchsorted(Larr, L, side="right") - 1
    idx[(L < Larr[0]) | (L >= Larr[-1])] = nbin
    return Larr, Lavg, Lavg[1] - Lavg[0], idx


def veff_device(L, flux, flim, vol, sum_omega, alpha, fcmin, nboot=100, nbin=25, seed=None, boot_idx=None, device=0):
    """VeffLF on the GPU (lf_veff of include/lfmcmc.h): the per-source weights, the binned LF and the bootstrap sums in
    two kernels.  vol: the comoving-volume integral, scalar (min_comp_frac <= 0.001) or per source.  The resamples are
    drawn on the device (Philox keyed by `seed`, default: one draw from numpy's global state) unless `boot_idx`
    (nboot, N) is given - e.g. the reference's own seeded np.random.randint stream, which then reproduces
    V.getBootErrLog's variances exactly.  Returns (phifunc, Lavg, lfbinorig, var) as lumfunc_weights + boot_err_log do."""
    from .capi import veff_device as _dev
    _, Lavg, dL, idx = luminosity_bins(L, nbin)
    if seed is None:
        seed = int(np.random.randint(0, 2 ** 31 - 1))
    phi, sums = _dev(flux, flim, vol, sum_omega / hs.SQARCSEC, alpha, fcmin, bin_of=idx, nbin=nbin, nboot=nboot,
                     boot_idx=boot_idx, seed=seed, device=device)
    lfbin = sums[1:] / dL
    binavg = np.average(lfbin, axis=0)
    var = 1. / (nboot - 1) * np.sum((lfbin - binavg) ** 2, axis=0)
    var[var <= 0.0] = min(var[var > 0.0])
    return phi, Lavg, sums[0] / dL, var


def veff_draws(flux, field, vol, pref0, fcmin, bin_of, nbin, draws):
    """Binned 1/Veff sums of the catalogue under each completeness draw (NumPy twin of lf_veff_draws):
    values[r][b] = sum over the sources of bin b of 1 / (pref0 fleming(flux_i, Flim_r[field_i], alpha_r, fcmin) vol_i), 0 for
    a source with vol_i <= 0.  draws (R, nf + 1): Flim per field in erg cm^-2 s^-1, then alpha; vol: scalar or per source;
    bin_of outside [0, nbin): no bin.  One draw is lumfunc_weights + the bincount of boot_err_log, bit for bit."""
    flux = np.asarray(flux, dtype=np.float64)
    field = np.asarray(field, dtype=np.int64)
    draws = np.atleast_2d(np.asarray(draws, dtype=np.float64))
    nf = draws.shape[1] - 1
    idx = np.asarray(bin_of, dtype=np.int64).copy()
    idx[(idx < 0) | (idx >= nbin)] = nbin                  # overflow slot, dropped below
    scalar = np.ndim(vol) == 0
    ok = None if scalar else np.asarray(vol) > 0
    values = np.zeros((draws.shape[0], nbin))
    for r, d in enumerate(draws):
        pref = pref0 * hs.fleming(flux, d[:nf][field], d[nf], fcmin)
        phi = np.zeros_like(flux)
        if scalar:
            if vol > 0:
                phi = 1.0 / (pref * vol)
        else:
            with np.errstate(divide="ignore"):
                phi[ok] = 1.0 / (pref[ok] * np.asarray(vol)[ok])
        values[r] = np.bincount(idx, weights=phi, minlength=nbin + 1)[:nbin]
    return values


def veff_draws_quantiles(flux, field, vol, pref0, fcmin, bin_of, nbin, draws, q=(16.0, 50.0, 84.0), method="linear", device=False,
                         device_index=0):
    """Percentiles over the draws of veff_draws's values: (out (nq, nbin), values (R, nbin)); np.percentile's rule
    ("linear") or np.median's ("median": one row, q ignored).  device=True: one device job (lf_veff_draws), whose sums have a
    fixed order - the same bits on every call; False: the NumPy twin."""
    from . import lfbands
    lfbands._method(method)
    if device:
        from . import capi
        return capi.veff_draws_device(flux, field, vol, pref0, fcmin, bin_of, nbin, draws, q=q, method=lfbands.METHODS[method],
                                      device=device_index)
    values = veff_draws(flux, field, vol, pref0, fcmin, bin_of, nbin, draws)
    if method == "linear":
        out = np.percentile(values, np.atleast_1d(np.asarray(q, dtype=np.float64)), axis=0)
    else:
        out = np.median(values, axis=0)[None]
    return out, values


def veff_draws_zmax(lum, flux, field, fmin, zmin, zmax, dVdzf, cosmo, pref0, fcmin, bin_of, nbin, draws):
    """veff_draws with every source's volume ending at the z_max of the draw's own flux cut (NumPy twin of
    lf_veff_draws_zmax).  lum: log10 L per source; fmin (R, nf): the flux cut of each draw and
    field in erg cm^-2 s^-1 (0: no cut, z_max = zmax).  Row r is, by definition,
        zmax_i = min(zmax, max_redshift(10^lum, fmin[r][field]));  vol = comoving_volume(dVdzf, zmin, zmax_i)
        veff_draws(..., vol, ..., draws[r:r + 1])
    - a loop over the existing functions, N inversions of the luminosity distance per draw."""
    lum_lin = 10 ** np.asarray(lum, dtype=np.float64)
    field = np.asarray(field, dtype=np.int64)
    draws = np.atleast_2d(np.asarray(draws, dtype=np.float64))
    fmin = np.asarray(fmin, dtype=np.float64).reshape(draws.shape[0], draws.shape[1] - 1)
    values = np.zeros((draws.shape[0], nbin))
    for r in range(draws.shape[0]):
        fm = fmin[r][field]
        with np.errstate(divide="ignore", invalid="ignore"):
            # the whole array, as the definition has it: max_redshift itself leaves the fmin = 0 entries (an infinite distance)
            # out of the batch it inverts, so the Newton stop sees the same sources either way
            zi = np.where(fm > 0, max_redshift(lum_lin, fm, cosmo), np.inf)
        vol = comoving_volume(dVdzf, zmin, np.minimum(zmax, zi))
        values[r] = veff_draws(flux, field, vol, pref0, fcmin, bin_of, nbin, draws[r:r + 1])[0]
    return values


def source_distance_scale(lum):
    """s_i = sqrt(L_i / 4 pi) / Mpc_cm: a source's luminosity distance at the flux cut fmin is s_i fmin^(-1/2) Mpc."""
    return np.sqrt(10 ** np.asarray(lum, dtype=np.float64) / (4.0 * np.pi)) / MPC_CM_EXACT


def veff_draws_zmax_quantiles(lum, flux, field, fmin, zmin, zmax, dVdzf, cosmo, pref0, fcmin, bin_of, nbin, draws,
                              q=(16.0, 50.0, 84.0), method="linear", device=False, device_index=0, table=None):
    """Percentiles over the draws of veff_draws_zmax's values, as veff_draws_quantiles.  device=True: one device job
    (lf_veff_draws_zmax) that evaluates the volume per (source, draw) from `table` (voltable.build; built when None); a table
    that was not validated or misses 1e-13 of the total volume is refused (voltable.require)."""
    from . import lfbands
    lfbands._method(method)
    if device:
        from . import capi, voltable
        table = voltable.require(voltable.build(cosmo, dVdzf, zmin, zmax) if table is None else table)
        return capi.veff_draws_zmax_device(flux, field, source_distance_scale(lum), pref0, fcmin, bin_of, nbin, draws, fmin, table,
                                           q=q, method=lfbands.METHODS[method], device=device_index)
    values = veff_draws_zmax(lum, flux, field, fmin, zmin, zmax, dVdzf, cosmo, pref0, fcmin, bin_of, nbin, draws)
    if method == "linear":
        out = np.percentile(values, np.atleast_1d(np.asarray(q, dtype=np.float64)), axis=0)
    else:
        out = np.median(values, axis=0)[None]
    return out, values


def boot_err_log(L, phi, nboot=100, nbin=25):
    """Binned LF dn/dlogL, and bootstrap variances (V.getBootErrLog with correct_low=False).
    Bin edges linspace(min(L)*1.001, max(L), nbin+1), half-open bins [e_j, e_j+1): the brightest
    source and anything below min(L)*1.001 fall in no bin, as in the reference.  One
    np.random.randint(N, size=N) per resample, in order - the reference's use of the global state."""
    L = np.asarray(L, dtype=np.float64)
    phi = np.asarray(phi, dtype=np.float64)
    Larr = np.linspace(min(L) * 1.001, max(L), nbin + 1)
    Lavg = np.linspace((Larr[0] + Larr[1]) / 2.0, (Larr[-1] + Larr[-2]) / 2.0, len(Larr) - 1)
    dL = Lavg[1] - Lavg[0]
    idx = np.searchsorted(Larr, L, side="right") - 1
    idx[(L < Larr[0]) | (L >= Larr[-1])] = nbin            # overflow slot, dropped below
    lfbinorig = np.bincount(idx, weights=phi, minlength=nbin + 1)[:nbin] / dL
    lfbin = np.zeros((nboot, nbin))
    for k in range(nboot):
        boot = np.random.randint(len(phi), size=len(phi))
        lfbin[k] = np.bincount(idx[boot], weights=phi[boot], minlength=nbin + 1)[:nbin] / dL
    binavg = np.average(lfbin, axis=0)
    var = 1. / (nboot - 1) * np.sum((lfbin - binavg) ** 2, axis=0)
    var[var <= 0.0] = min(var[var > 0.0])
    return Lavg, lfbinorig, var


# ---------------------------------------------------------------------------------------------- redshift slices
SLICES_PURPOSE = 0x736c6963      # the Philox stream word of the slices' bootstrap (csrc/lf_veffslices.h: VEFFS_PURPOSE)
SLICES_MAX = 64                  # slices, and luminosity bins, of one call (VEFFS_MAXSLICE, VEFFS_MAXBIN)
SLICES_CHUNK = 4096              # draws per chunk of the device's summation order (VEFFS_CHUNK)


def slice_edges(z, S):
    """The S + 1 edges of S equal-count redshift slices (V.get_bins + V.zEvolSteps, VmaxLumFunc.py:45-48, :619-630): ranks from
    a stable argsort of z, the source of rank r in slice floor(r S / N); e_0 = min(z), e_S = max(z), an inner edge the mean
    of the largest z below it and the smallest above it."""
    z = np.asarray(z, dtype=np.float64)
    N, S = z.size, int(S)
    if not 1 <= S <= min(N, SLICES_MAX):
        raise ValueError("the number of slices must be between 1 and min(N, %d), not %d" % (SLICES_MAX, S))
    zs = z[np.argsort(z, kind="stable")]
    sl = (np.arange(N, dtype=np.int64) * S) // N                # the slice of every rank
    first = np.searchsorted(sl, np.arange(1, S))                # the first rank of slices 1 .. S - 1
    return np.concatenate([[zs[0]], (zs[first - 1] + zs[first]) / 2.0, [zs[-1]]])


def slice_index(z, z_edges):
    """slice_of per source: s where e_s <= z < e_s+1, the last slice also taking z == e_S; -1 for a source outside every slice."""
    z = np.asarray(z, dtype=np.float64)
    e = np.asarray(z_edges, dtype=np.float64)
    S = e.size - 1
    if S < 1 or S > SLICES_MAX or not np.all(np.diff(e) > 0):
        raise ValueError("z_edges must hold 2 to %d strictly increasing redshifts" % (SLICES_MAX + 1))
    s = np.searchsorted(e, z, side="right") - 1
    s[z == e[-1]] = S - 1
    s[(s < 0) | (s >= S) | ~np.isfinite(z)] = -1
    return s.astype(np.int32)


def slice_volumes(dVdzf, z_edges, slice_of, zmaxval):
    """vol_i = int dV/dz dz from e_s to min(e_s+1, zmax_i) for the source's own slice s - the exact integral of the interpolant
    (_interp_integral), 0 where the upper limit is not above the lower; a source without a slice gets the volume of all the
    slices together, e_0 to min(e_S, zmax_i).  zmaxval: scalar or per source."""
    e = np.asarray(z_edges, dtype=np.float64)
    s = np.asarray(slice_of, dtype=np.int64)
    has = s >= 0
    lo = np.where(has, e[np.where(has, s, 0)], e[0])
    hi = np.minimum(np.where(has, e[np.where(has, s, 0) + 1], e[-1]), np.broadcast_to(np.asarray(zmaxval, dtype=np.float64), s.shape))
    ok = hi > lo
    return np.where(ok, _interp_integral(dVdzf, lo, np.where(ok, hi, lo)), 0.0)


def slice_weights(flux, flim, vol, pref0, alpha, fcmin):
    """phi_i = 1 / (pref0 fleming(F_i, Flim_i, alpha, fcmin) vol_i), 0 where vol_i <= 0: lumfunc_weights' operations with a given
    volume per source (the NumPy twin of the veff_weights kernel)."""
    flux, vol = np.asarray(flux, dtype=np.float64), np.asarray(vol, dtype=np.float64)
    pref = pref0 * hs.fleming(flux, flim, alpha, fcmin)
    phi = np.zeros_like(flux)
    ok = vol > 0
    with np.errstate(divide="ignore"):
        phi[ok] = 1.0 / (pref[ok] * vol[ok])
    return phi


def slice_bins(L, slice_of, nslice, nbin, bins="common"):
    """The luminosity bins of the slices: (Lavg (nslice, nbin), dL (nslice,), bin_of per source, nbin = no bin).
    bins="common": luminosity_bins of the whole catalogue for every slice, so that the slices compare bin by bin; "slice": every
    slice its own luminosity_bins of its own sources (V.zEvolSteps), NaN centres, dL = NaN and no bins for a slice with fewer
    than 2 sources, or whose luminosities do not reach past the first edge, 1.001 min(L)."""
    if bins not in ("common", "slice"):
        raise ValueError("bins must be 'common' or 'slice', not %r" % (bins,))
    L = np.asarray(L, dtype=np.float64)
    s = np.asarray(slice_of)
    if bins == "common":
        _, Lavg, dL, idx = luminosity_bins(L, nbin)
        return np.tile(Lavg, (nslice, 1)), np.full(nslice, dL), idx.astype(np.int32)
    Lavg, dL, idx = np.full((nslice, nbin), np.nan), np.full(nslice, np.nan), np.full(L.size, nbin, dtype=np.int32)
    for k in range(nslice):
        sel = s == k
        if sel.sum() >= 2 and L[sel].max() > L[sel].min() * 1.001:
            _, Lavg[k], dL[k], idx[sel] = luminosity_bins(L[sel], nbin)
    return Lavg, dL, idx


def slice_sort(slice_of, nslice):
    """The stable counting sort by slice of the sources that have one: (order (m,), off (nslice + 1,))."""
    s = np.asarray(slice_of, dtype=np.int64)
    has = (s >= 0) & (s < nslice)
    order = np.flatnonzero(has)
    order = order[np.argsort(s[order], kind="stable")]
    off = np.concatenate([[0], np.cumsum(np.bincount(s[has], minlength=nslice)[:nslice])]).astype(np.int64)
    return order, off


def slice_boot_indices(n_s, s, k, seed):
    """The n_s draws of resample k (1 .. nboot) of slice s, source numbers within the slice: min(floor(u53(r0, r1) n_s),
    n_s - 1), r = Philox4x32-10(counter (j, s, k, SLICES_PURPOSE), key seed) - veffs_partial's own."""
    from . import philox
    j = np.arange(n_s, dtype=np.uint64)
    seed = int(seed)
    r = philox.philox4x32(j, np.full(n_s, s, dtype=np.uint64), np.full(n_s, k, dtype=np.uint64),
                          np.full(n_s, SLICES_PURPOSE, dtype=np.uint64), seed & philox.MASK, (seed >> 32) & philox.MASK)
    return np.minimum((philox.u53(r[0], r[1]) * float(n_s)).astype(np.int64), n_s - 1)


def veff_slices(phi, slice_of, nslice, bin_of, nbin, nboot=0, seed=0, boot_idx=None):
    """NumPy twin of lf_veff_slices's sums (include/lfmcmc.h): (sums (nboot + 1, nslice, nbin), counts (nslice, nbin) int64,
    n_slice (nslice,)).  k = 0 is the catalogue; resample k of slice s draws n_s sources of the slice (slice_boot_indices, or
    boot_idx (nboot, m): source numbers within the slice, for the sources with a slice in slice-sorted order); every sum is one
    np.bincount over the draws in their order."""
    phi = np.asarray(phi, dtype=np.float64)
    order, off = slice_sort(slice_of, nslice)
    idx = np.asarray(bin_of, dtype=np.int64)[order].copy()
    idx[(idx < 0) | (idx >= nbin)] = nbin                  # overflow slot, dropped below
    w = phi[order]
    if boot_idx is not None:
        boot_idx = np.asarray(boot_idx, dtype=np.int64)
        if boot_idx.shape != (nboot, order.size):
            raise ValueError("boot_idx must be (nboot, sources with a slice)")
    sums = np.zeros((nboot + 1, nslice, nbin))
    counts = np.zeros((nslice, nbin), dtype=np.int64)
    for s in range(nslice):
        a, n_s = int(off[s]), int(off[s + 1] - off[s])
        if n_s == 0:
            continue
        counts[s] = np.bincount(idx[a:a + n_s], minlength=nbin + 1)[:nbin]
        for k in range(nboot + 1):
            if k == 0:
                boot = np.arange(n_s)
            elif boot_idx is not None:
                boot = boot_idx[k - 1, a:a + n_s]
                if boot.min() < 0 or boot.max() >= n_s:
                    raise ValueError("boot_idx outside its slice")
            else:
                boot = slice_boot_indices(n_s, s, k, seed)
            sums[k, s] = np.bincount(idx[a + boot], weights=w[a + boot], minlength=nbin + 1)[:nbin]
    return sums, counts, np.diff(off)


def slice_variance(sums, dL):
    """(lf (nslice, nbin), var (nslice, nbin)) from sums (nboot + 1, nslice, nbin) and the slices' bin widths, per slice exactly
    as veff_device takes them: lfbin = sums[1:] / dL, ddof = 1, non-positive entries replaced by the slice's smallest positive
    one - and left 0 where the slice has none (an empty slice, or nboot < 2)."""
    sums = np.asarray(sums, dtype=np.float64)
    nboot, nslice, nbin = sums.shape[0] - 1, sums.shape[1], sums.shape[2]
    lf, var = np.zeros((nslice, nbin)), np.zeros((nslice, nbin))
    for s in range(nslice):
        lf[s] = sums[0, s] / dL[s]
        if nboot < 2:
            continue
        lfbin = sums[1:, s] / dL[s]
        binavg = np.average(lfbin, axis=0)
        v = 1. / (nboot - 1) * np.sum((lfbin - binavg) ** 2, axis=0)
        if np.any(v > 0.0):
            v[~(v > 0.0)] = min(v[v > 0.0])
            var[s] = v
    return lf, var


def _slices_run(device, L, flux, flim, vol, slice_of, nslice, sum_omega, alpha, fcmin, nboot, nbin, bins, seed, boot_idx, device_index):
    if not 1 <= nbin <= SLICES_MAX or not 1 <= nslice <= SLICES_MAX:
        raise ValueError("nbin and the number of slices must be between 1 and %d" % SLICES_MAX)
    Lavg, dL, idx = slice_bins(L, slice_of, nslice, nbin, bins)
    if seed is None:
        seed = int(np.random.randint(0, 2 ** 31 - 1))
    pref0 = sum_omega / hs.SQARCSEC
    if device:
        from . import capi
        phi, sums, counts = capi.veff_slices(flux, flim, vol, pref0, alpha, fcmin, slice_of, nslice, idx, nbin, nboot=nboot,
                                             boot_idx=boot_idx, seed=seed, device=device_index)
        n_slice = np.diff(slice_sort(slice_of, nslice)[1])
    else:
        phi = slice_weights(flux, flim, vol, pref0, alpha, fcmin)
        sums, counts, n_slice = veff_slices(phi, slice_of, nslice, idx, nbin, nboot=nboot, seed=seed, boot_idx=boot_idx)
    lf, var = slice_variance(sums, dL)
    return phi, Lavg, lf, var, counts, np.asarray(n_slice, dtype=np.int64)


def veff_slices_host(L, flux, flim, vol, slice_of, nslice, sum_omega, alpha, fcmin, nboot=100, nbin=25, bins="common", seed=None,
                     boot_idx=None):
    """The sliced 1/Veff points in NumPy: (phi, Lavg (nslice, nbin), lf (nslice, nbin), var (nslice, nbin), counts, n_slice).
    vol: the volume per source (slice_volumes); slice_of: slice_index; seed None: one draw from numpy's global state."""
    return _slices_run(False, L, flux, flim, vol, slice_of, nslice, sum_omega, alpha, fcmin, nboot, nbin, bins, seed, boot_idx, 0)


def veff_slices_device(L, flux, flim, vol, slice_of, nslice, sum_omega, alpha, fcmin, nboot=100, nbin=25, bins="common", seed=None,
                       boot_idx=None, device=0):
    """veff_slices_host on the GPU (lf_veff_slices): the weights, the binned sums and the nboot resamples of every slice in one
    call, with a fixed order of summation - the same bits on every call.  Same arguments and results."""
    return _slices_run(True, L, flux, flim, vol, slice_of, nslice, sum_omega, alpha, fcmin, nboot, nbin, bins, seed, boot_idx, device)


def slice_nodes(z_edges, G):
    """Gauss-Legendre nodes and weights of every slice: (z (S, G), w (S, G)), sum_g w_sg = e_s+1 - e_s."""
    e = np.asarray(z_edges, dtype=np.float64)
    x, w = np.polynomial.legendre.leggauss(int(G))
    half, mid = 0.5 * np.diff(e), 0.5 * (e[1:] + e[:-1])
    return mid[:, None] + half[:, None] * x[None, :], half[:, None] * w[None, :]


def slice_model_average(values, zw):
    """The model LF averaged over each slice in the volume measure: values (R, S, G, nbin) at the slices' nodes, zw (S, G) =
    w_g dV/dz(z_g); returns sum_g zw_sg values[r, s, g, b] / sum_g zw_sg, (R, S, nbin)."""
    zw = np.asarray(zw, dtype=np.float64)
    return np.einsum("rsgb,sg->rsb", values, zw) / zw.sum(axis=1)[None, :, None]
