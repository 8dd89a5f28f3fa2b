"""Posterior bands of the model luminosity function: exact percentiles over R posterior draws at P points.

Reference: LumFuncMCMC.set_median_fit (lumfuncmcmc.py:527-567) evaluates TrueLumFunc for 200 random posterior rows at
every source and takes np.median over the draws - an R x N float64 matrix on the host (1.6 GB at N = 10^6).  The same
contract, generalised to any percentiles and to the z-evolving model, is

    out[i][p] = np.percentile(v, q[i], axis=0)[p]    (method "linear"),   np.median(v, axis=0)[p]   (method "median")
    v[r][p]   = the model LF of draw r at point p  (hostsetup.true_lum_func / schechter_z)

`quantiles_host` states it in NumPy, a chunk of points at a time so that memory stays bounded; `quantiles_device` runs
it in one HIP kernel (lf_lumfunc_quantiles, csrc/lf_bands.h) that never materialises v.

Draw records: single Schechter (LF_FREE / LF_FIXCOMP) (logLstar, logphistar, alpha); z-evolving (LF_ZEVOL)
(aL, bL, cL, aphi, bphi, cphi, alpha), the coefficients of the quadratics log L*(z), log phi*(z) through the pivots.
"""
import numpy as np

from . import hostsetup as hs

METHODS = {"linear": 0, "median": 1}
CHUNK_VALUES = 1 << 24          # values per host chunk (128 MB of float64)


def _method(method):
    if method not in METHODS:
        raise ValueError("method must be 'linear' or 'median', not %r" % (method,))
    return method


def pack_draws(variant, rows, fix_sch_al=False, sch_al=None, pivots=None):
    """Draw records from theta rows (any trailing columns - Flim, alpha_C, lnprob - are ignored).
    variant "free" / "fixcomp": theta = (Lstar, phistar, [sch_al], ...); "zevol": theta = (L1, L2, L3, phi1, phi2, phi3,
    [sch_al], ...) with pivots = (z1, z2, z3).  fix_sch_al: alpha is `sch_al`, not a theta column."""
    rows = np.atleast_2d(np.asarray(rows, dtype=np.float64))
    R = rows.shape[0]
    if variant in ("free", "fixcomp"):
        alpha = np.full(R, float(sch_al)) if fix_sch_al else rows[:, 2]
        return np.ascontiguousarray(np.column_stack([rows[:, 0], rows[:, 1], alpha]))
    if variant != "zevol":
        raise ValueError("variant must be 'free', 'fixcomp' or 'zevol'")
    z1, z2, z3 = pivots
    alum, blum, clum = hs.get_quad_coef(rows[:, 0], rows[:, 1], rows[:, 2], z1, z2, z3)
    aphi, bphi, cphi = hs.get_quad_coef(rows[:, 3], rows[:, 4], rows[:, 5], z1, z2, z3)
    alpha = np.full(R, float(sch_al)) if fix_sch_al else rows[:, 6]
    return np.ascontiguousarray(np.column_stack([alum, blum, clum, aphi, bphi, cphi, alpha]))


def lf_values(variant, draws, logL, z=None):
    """v[r][p] of the module docstring, (R, P), with the host's operations (schechter_z's grouping for "zevol")."""
    draws = np.asarray(draws, dtype=np.float64)
    logL = np.asarray(logL, dtype=np.float64)
    v = np.empty((draws.shape[0], logL.size))
    with np.errstate(all="ignore"):
        for r, d in enumerate(draws):
            if variant == "zevol":
                v[r] = hs.true_lum_func(logL, d[6], d[0] * z ** 2 + d[1] * z + d[2], d[3] * z ** 2 + d[4] * z + d[5])
            else:
                v[r] = hs.true_lum_func(logL, d[2], d[0], d[1])
    return v


def quantiles_host(variant, draws, logL, z=None, q=(16.0, 50.0, 84.0), method="linear", chunk=None):
    """NumPy statement of lf_lumfunc_quantiles: (nq, P) for "linear", (1, P) for "median"."""
    _method(method)
    draws = np.atleast_2d(np.asarray(draws, dtype=np.float64))
    logL = np.asarray(logL, dtype=np.float64).ravel()
    if variant == "zevol":
        z = np.asarray(z, dtype=np.float64).ravel()
    q = np.atleast_1d(np.asarray(q, dtype=np.float64))
    P = logL.size
    out = np.empty((q.size if method == "linear" else 1, P))
    step = chunk or max(1, CHUNK_VALUES // max(1, draws.shape[0]))
    for lo in range(0, P, step):
        hi = min(P, lo + step)
        v = lf_values(variant, draws, logL[lo:hi], None if z is None else z[lo:hi])
        with np.errstate(all="ignore"):
            out[:, lo:hi] = np.percentile(v, q, axis=0) if method == "linear" else np.median(v, axis=0)
    return out


def quantiles_device(variant, draws, logL, z=None, q=(16.0, 50.0, 84.0), method="linear", values=False, device=0):
    """lf_lumfunc_quantiles on the GPU: same contract and shapes as quantiles_host (values=True also returns v)."""
    from . import capi
    _method(method)
    return capi.lumfunc_quantiles(variant, draws, logL, z=z, q=q, method=METHODS[method], values=values, device=device)


def quantiles(variant, draws, logL, z=None, q=(16.0, 50.0, 84.0), method="linear", device=False, device_index=0):
    if device:
        return quantiles_device(variant, draws, logL, z=z, q=q, method=method, device=device_index)
    return quantiles_host(variant, draws, logL, z=z, q=q, method=method)
