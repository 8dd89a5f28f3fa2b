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
