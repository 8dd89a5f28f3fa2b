"""Posterior bands of the integrated luminosity function: number density n(>L) and luminosity density rho(>L).

For a Schechter function in hostsetup.true_lum_func's normalisation (phi per dlogL = ln10 phi* 10^(t (alpha + 1))
exp(-10^t), t = logL - logL*) both integrals over logL from logLmin up are upper incomplete gamma functions of
x = 10^(logLmin - logL*):

    n(>Lmin)   = 10^logphi*            Gamma(alpha + 1, x)      [Mpc^-3]                    kind "number"
    rho(>Lmin) = 10^logphi* 10^logL*   Gamma(alpha + 2, x)      [erg s^-1 Mpc^-3]           kind "lumdens"

`gammainc_upper` is the NumPy twin of csrc/lf_gammainc.h (same algorithm, operation for operation; DESIGN.md section
3.16), `integral_values` the (R, P) matrix over draws and points, and `quantiles_host` / `quantiles_device` /
`quantiles` mirror lfbands: np.percentile / np.median over the draws on the host, or one HIP kernel
(lf_lumfunc_integral_quantiles, lf_bands_integ in csrc/lf_bands.h) that never materialises the matrix.

Draw records are lfbands.pack_draws's: (logLstar, logphistar, alpha), or for "zevol" (aL, bL, cL, aphi, bphi, cphi, alpha).
"""
import numpy as np

from . import lfbands
from ._gammainc_coef import GI_E10, GI_LG2_HI, GI_LG2_LO, GI_LOG2_10, GI_W

KINDS = {"number": 0, "lumdens": 1}
ALPHA_MIN, ALPHA_MAX = -6.0, 5.0

# the algorithm's constants - lf_gammainc.h holds the same ones
GI_A_MIN, GI_A_MAX = -5.0, 7.0      # orders the function accepts (alpha + 1 + kind for alpha in [-6, 5])
GI_XSW = 1.0                        # series below, continued fraction from here on
GI_SER_CAP = 40                     # trip cap of either series (x < 1: reached by no input)
GI_CF_N0, GI_CF_K = 8, 120.0        # the continued fraction is evaluated bottom-up from term N0 + int(K / x) <= 128
GI_CF_CAP = 136                     # its trip cap
GI_REC_CAP = 6                      # recurrence steps: |round(a)| <= 7
GI_EPS = 2.0 ** -54
GI_A0_TINY = 2.0 ** -500            # below it the singular part takes its limit -euler - ln x
GI_AL_POW = 1.0                     # |a0 ln x| above it: the bracket takes x^a0 - 1 in the place of expm1(a0 ln x)
GI_REC_SCALE, GI_REC_UNSCALE = 2.0 ** -8, 2.0 ** 8  # the downward recurrence runs on 2^-8 of its terms (exact)


def _kind(kind):
    if kind not in KINDS:
        raise ValueError("kind must be 'number' or 'lumdens', not %r" % (kind,))
    return KINDS[kind]


def exp10(t):
    """10^t with the IEEE operations of lf_gammainc.h's gi_exp10 (the two agree to the bit): 2^k 10^r, k = rint(t
    log2(10)), r = t - k log10(2) in two parts, 10^r by its Taylor polynomial.  +inf from 309 up, 0 below -330."""
    t = np.asarray(t, dtype=np.float64)
    with np.errstate(all="ignore"):
        tc = np.where((t >= -330.0) & (t < 309.0), t, 0.0)
        k = np.rint(tc * GI_LOG2_10)
        r = (tc - k * GI_LG2_HI) - k * GI_LG2_LO
        p = np.full(t.shape, GI_E10[-1])
        for c in GI_E10[-2::-1]:
            p = p * r + c
        v = np.ldexp(p, k.astype(np.int32))
        return np.where(t >= 309.0, np.inf, np.where(t < -330.0, 0.0, np.where(np.isnan(t), np.nan, v)))


def gammainc_upper(a, x, counts=False):
    """Gamma(a, x) = int_x^inf t^(a-1) e^-t dt in fp64 for real a in [-5, 7] and x >= 0 (x = 0: Gamma(a) for a > 0, +inf
    otherwise; x = +inf: 0).  NaN for a NaN or anything outside the domain; inside it never NaN, and +inf where Gamma(a, x)
    is above the largest double (a < 0 and x below 1e-61 and less).  counts=True also returns the trip counts of
    the element's loops, (series, continued fraction, recurrence), as three int arrays."""
    a, x = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(x, dtype=np.float64))
    shape = a.shape
    a, x = a.ravel().copy(), x.ravel().copy()
    n = a.size
    res = np.full(n, np.nan)
    nser, ncf, nrec = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    with np.errstate(all="ignore"):
        ok = (x >= 0.0) & (a >= GI_A_MIN) & (a <= GI_A_MAX)
        m = np.rint(np.where(ok, a, 0.0))
        a0 = np.where(ok, a, 0.0) - m
        w = np.full(n, GI_W[-1])
        for c in GI_W[-2::-1]:
            w = w * a0 + c
        r = 1.0 + a0 * w                                    # 1 / Gamma(1 + a0)
        mi = m.astype(np.int64)
        up = mi >= 1
        b = a - (m - 1.0)                                   # base order of the upward side, in [0.5, 1.5]

        # x = 0
        s = ok & (x == 0.0)
        if s.any():
            g = 1.0 / r
            g0 = g / a0                                     # round(a) = 0
            for k in range(1, GI_REC_CAP + 1):
                g = np.where(k <= mi - 1, g * (a - k), g)
            res[s] = np.where(a > 0.0, np.where(up, g, g0), np.inf)[s]
            nrec[s] = np.maximum(mi - 1, 0)[s]

        # +inf, and every x whose exp(-x / 2) is already 0
        h = np.exp(-0.5 * x)
        z = ok & (x > 0.0) & (h == 0.0)
        res[z] = 0.0

        # 0 < x < XSW, round(a) >= 1: Gamma(b) - gamma(b, x) with the all-positive series, then upwards
        s = ok & (x > 0.0) & (x < GI_XSW) & up
        if s.any():
            i = np.flatnonzero(s)
            xs, bs = x[i], b[i]
            term = 1.0 / bs
            tot = term.copy()
            cnt = np.zeros(i.size, dtype=np.int64)
            live = np.ones(i.size, dtype=bool)
            for k in range(1, GI_SER_CAP + 1):
                term = np.where(live, term * (xs / (bs + k)), term)
                tot = np.where(live, tot + term, tot)
                cnt += live
                live = live & (term > tot * GI_EPS)
                if not live.any():
                    break
            f = np.power(xs, bs) * np.exp(-xs)
            g = 1.0 / r[i] - f * tot
            for k in range(GI_REC_CAP):
                act = k <= mi[i] - 2
                g = np.where(act, (bs + k) * g + f, g)
                f = np.where(act, f * xs, f)
            res[i] = g
            nser[i] = cnt
            nrec[i] = mi[i] - 1

        # 0 < x < XSW, round(a) <= 0: the singular part in Gautschi's form at the base order a0, then downwards
        s = ok & (x > 0.0) & (x < GI_XSW) & ~up
        if s.any():
            i = np.flatnonzero(s)
            xs, a0s, as_ = x[i], a0[i], a[i]
            t = np.ones(i.size)
            tot = np.zeros(i.size)
            cnt = np.zeros(i.size, dtype=np.int64)
            live = np.ones(i.size, dtype=bool)
            for k in range(1, GI_SER_CAP + 1):
                t = np.where(live, t * (-xs / k), t)
                term = t / (a0s + k)
                tot = np.where(live, tot + term, tot)
                cnt += live
                live = live & (np.abs(term) > np.abs(tot) * GI_EPS)
                if not live.any():
                    break
            lx = np.log(xs)
            p = np.power(xs, a0s)
            al = a0s * lx
            brk = np.where(np.abs(al) > GI_AL_POW, (p - 1.0) / a0s, np.expm1(al) / a0s)
            sing = np.where(np.abs(a0s) < GI_A0_TINY, -GI_W[0] - lx, -w[i] / r[i] - brk)
            g = (sing - p * tot) * GI_REC_SCALE
            f = (p * np.exp(-xs)) * GI_REC_SCALE
            for k in range(1, GI_REC_CAP + 1):
                act = k <= -mi[i]
                f = np.where(act, f / xs, f)
                g = np.where(act, np.where(f == np.inf, np.inf, (g - f) / (as_ + (-m[i] - k))), g)
            res[i] = g * GI_REC_UNSCALE
            nser[i] = cnt
            nrec[i] = -mi[i]

        # x >= XSW: the continued fraction bottom-up at the order itself (round(a) <= 0) or at b and then upwards
        s = ok & (x >= GI_XSW) & (h != 0.0)
        if s.any():
            i = np.flatnonzero(s)
            xs = x[i]
            c = np.where(up[i], b[i], a[i])
            nt = GI_CF_N0 + (GI_CF_K / xs).astype(np.int64)
            nt = np.minimum(nt, GI_CF_CAP)
            f = xs + (2.0 * nt + 1.0) - c
            for k in range(int(nt.max()), 0, -1):
                act = k <= nt
                f = np.where(act, (xs + (2.0 * k - 1.0) - c) + (-k * (k - c)) / f, f)
            q = 1.0 / f
            for k in range(GI_REC_CAP):
                q = np.where(k <= mi[i] - 2, ((b[i] + k) * q + 1.0) / xs, q)
            res[i] = ((np.power(xs, a[i]) * h[i]) * h[i]) * q
            ncf[i] = nt
            nrec[i] = np.maximum(mi[i] - 1, 0)
    res = res.reshape(shape)
    if counts:
        return res, (nser.reshape(shape), ncf.reshape(shape), nrec.reshape(shape))
    return res


def integral_values(variant, kind, draws, logLmin, z=None):
    """v[r][p] = prefactor * Gamma(alpha_r + 1 + kind, 10^(logLmin_p - logL*)), (R, P): the integrated LF of draw r
    above logLmin_p (at z_p for "zevol").  logLmin = -inf means x = 0.  The per-point powers of ten are exp10's, the
    per-draw prefactors of the single Schechter NumPy scalar powers (the C entry makes them with the host's pow)."""
    k = _kind(kind)
    draws = np.atleast_2d(np.asarray(draws, dtype=np.float64))
    logLmin = np.asarray(logLmin, dtype=np.float64).ravel()
    v = np.empty((draws.shape[0], logLmin.size))
    with np.errstate(all="ignore"):
        for r, d in enumerate(draws):
            if variant == "zevol":
                lstar = d[0] * z ** 2 + d[1] * z + d[2]
                lphi = d[3] * z ** 2 + d[4] * z + d[5]
                pref = exp10(lphi) * exp10(lstar) if k else exp10(lphi)
                al = d[6]
            else:
                lstar = d[0]
                pref = 10.0 ** d[1] * 10.0 ** d[0] if k else 10.0 ** d[1]
                al = d[2]
            v[r] = pref * gammainc_upper(al + 1.0 + k, exp10(logLmin - lstar))
    return v


def _check_draws(variant, draws):
    al = np.atleast_2d(np.asarray(draws, dtype=np.float64))[:, 6 if variant == "zevol" else 2]
    if not np.all((al >= ALPHA_MIN) & (al <= ALPHA_MAX)):
        raise ValueError("alpha must be finite and within [%g, %g]" % (ALPHA_MIN, ALPHA_MAX))


def quantiles_host(variant, kind, draws, logLmin, z=None, q=(16.0, 50.0, 84.0), method="linear", chunk=None):
    """NumPy statement of lf_lumfunc_integral_quantiles: (nq, P) for "linear", (1, P) for "median"."""
    lfbands._method(method)
    _kind(kind)
    draws = np.atleast_2d(np.asarray(draws, dtype=np.float64))
    _check_draws(variant, draws)
    logLmin = np.asarray(logLmin, dtype=np.float64).ravel()
    if np.isnan(logLmin).any():
        raise ValueError("logLmin holds a NaN")
    if variant == "zevol":
        z = np.asarray(z, dtype=np.float64).ravel()
    q = np.atleast_1d(np.asarray(q, dtype=np.float64))
    P = logLmin.size
    out = np.empty((q.size if method == "linear" else 1, P))
    step = chunk or max(1, lfbands.CHUNK_VALUES // max(1, draws.shape[0]))
    for lo in range(0, P, step):
        hi = min(P, lo + step)
        v = integral_values(variant, kind, draws, logLmin[lo:hi], None if z is None else z[lo:hi])
        with np.errstate(all="ignore"):
            out[:, lo:hi] = np.percentile(v, q, axis=0) if method == "linear" else np.median(v, axis=0)
    return out


def quantiles_device(variant, kind, draws, logLmin, z=None, q=(16.0, 50.0, 84.0), method="linear", values=False, device=0):
    """lf_lumfunc_integral_quantiles on the GPU: same contract and shapes as quantiles_host (values=True also returns v)."""
    from . import capi
    lfbands._method(method)
    return capi.lumfunc_integral_quantiles(variant, _kind(kind), draws, logLmin, z=z, q=q, method=lfbands.METHODS[method],
                                           values=values, device=device)


def quantiles(variant, kind, draws, logLmin, z=None, q=(16.0, 50.0, 84.0), method="linear", device=False, device_index=0):
    if device:
        return quantiles_device(variant, kind, draws, logLmin, z=z, q=q, method=method, device=device_index)
    return quantiles_host(variant, kind, draws, logLmin, z=z, q=q, method=method)
