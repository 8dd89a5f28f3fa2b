"""NumPy twin of the flux-error-convolved likelihood (csrc/lf_deconv.h), no GPU.

The catalogued log-luminosity of a source is its true one plus Gaussian noise of sigma_i dex (its lum_e), and the
completeness acts on the TRUE flux.  The noise integrates out of the expected counts (piece B is unchanged); each per-source
term ln[phi(L_i) Omega(L_i, z_i)] of piece A becomes ln of its convolution with N(0, sigma_i^2), taken by K-point
Gauss-Hermite quadrature and written as a correction to the plain value:

    lnprob_err = lnprob + Delta,   Delta = sum_i Delta_i,   Delta_i = ln sum_k (w_k / sqrt(pi)) exp(t_ik - t_i),
    delta_ik = sqrt(2) sigma_i x_k,
    t_ik - t_i = ln10 (alpha + 1) delta - 10^(L_i - L*) (10^delta - 1) + l(f_i 10^delta) - l(f_i),

l = ln fc^(1/d) the completeness in the form without cancellation (grad.py: _completeness; FREE: the row's Flim_f and
alpha_C, else the fixed ones), L* = L*(z_i) for the z-evolving model.  The statements below are the kernel's, written for
arrays: expm1 for 10^delta - 1, the inner sum as a log-sum-exp with a running maximum, a source with sigma_i = 0 skipped
(exactly 0).  The node tables are derived here (Newton on the orthonormal Hermite recurrence in extended precision), as
lf_hostprep.h derives the device's.
"""
import functools

import numpy as np

from . import grad as G

LN10 = G.LN10
ORDERS = (4, 6, 8, 10, 12, 16, 20, 24, 32)      # the supported quadrature orders (lf_layout.h: DECONV_ORDERS)
# the largest sigma (dex) each order is validated for: worst per-source error below 1e-7 over the probe set of
# tests/test_deconv_cpu.py (lf_layout.h: DECONV_SIGMA_MAX); no order up to 32 reaches 1e-7 above 0.09 dex
SIGMA_MAX_BY_ORDER = (0.01, 0.03, 0.04, 0.05, 0.06, 0.06, 0.07, 0.08, 0.09)
DEFAULT_ORDER = 32                              # the smallest order that reaches 1e-7 at 0.09 dex
SIGMA_MAX = 0.09
CHUNK = 1024                                    # sources per block of the device's fixed summation order (lf_layout.h: DECONV_CH)
# The wide rule (csrc/lf_deconv_wide.h; lf_layout.h: DECONV_WIDE_*), for sigma above the order's limit:
# sigma classes by their upper edges, per class a composite Gauss-Legendre rule on [-T, T] sigma of WIDE_PANELS[c] equal panels
# (the fewest that are at most WIDE_H dex wide at the class's upper edge) with WIDE_NPANEL nodes each.  Chosen against 30-digit
# integration on the probe set of tests/test_deconv_wide_cpu.py: worst per-source error below 1e-7 at every class's upper edge.
WIDE_EDGES = (0.10, 0.15, 0.20, 0.25, 0.30)
WIDE_PANELS = (6, 9, 12, 15, 18)
WIDE_NPANEL = 8
WIDE_T = 7.5
WIDE_H = 0.25
WIDE_SIGMA_MAX = WIDE_EDGES[-1]
WIDE_CHUNK = 256                                # sources per block of the wide kernels (lf_layout.h: DECONV_WIDE_CH)


def gauss_hermite(K):
    """(x[K] ascending, lnw[K] = ln(w_k / sqrt(pi))) of the K-point Gauss-Hermite rule (weight e^(-x^2)): Newton iterations
    on the orthonormal recurrence in extended precision, the positive roots from the largest down, mirrored."""
    K = int(K)
    if K < 2 or K > 64:
        raise ValueError("gauss_hermite: K must be in 2..64")
    ld = np.longdouble
    n = ld(K)
    pim4 = ld(1.0) / np.sqrt(np.sqrt(ld(np.pi) + ld(1.2246467991473532e-16)))
    x, w = np.zeros(K, dtype=ld), np.zeros(K, dtype=ld)
    z = ld(0.0)
    for i in range((K + 1) // 2):
        if i == 0:
            z = np.sqrt(2 * n + 1) - ld(1.85575) * (2 * n + 1) ** (ld(-1.0) / 6)
        elif i == 1:
            z = z - ld(1.14) * n ** ld(0.426) / z
        elif i == 2:
            z = ld(1.86) * z - ld(0.86) * x[K - 1]
        elif i == 3:
            z = ld(1.91) * z - ld(0.91) * x[K - 2]
        else:
            z = 2 * z - x[K - i + 1]
        pp = ld(1.0)
        for _ in range(100):
            p1, p2 = pim4, ld(0.0)
            for j in range(1, K + 1):
                p3, p2 = p2, p1
                p1 = z * np.sqrt(ld(2.0) / j) * p2 - np.sqrt(ld(j - 1) / j) * p3
            pp = np.sqrt(2 * n) * p2
            dz = p1 / pp
            z = z - dz
            if abs(dz) <= ld(1e-18) * max(abs(z), ld(1.0)):
                break
        if K % 2 == 1 and i == K // 2:
            z = ld(0.0)
            p1, p2 = pim4, ld(0.0)
            for j in range(1, K + 1):
                p3, p2 = p2, p1
                p1 = z * np.sqrt(ld(2.0) / j) * p2 - np.sqrt(ld(j - 1) / j) * p3
            pp = np.sqrt(2 * n) * p2
        x[K - 1 - i], x[i] = z, -z
        w[K - 1 - i] = w[i] = 2 / (pp * pp)
    lnw = np.log(w) - ld(0.5) * np.log(ld(np.pi) + ld(1.2246467991473532e-16))
    return x.astype(np.float64), lnw.astype(np.float64)


def gauss_legendre(n):
    """(x[n] ascending, w[n]) of the n-point Gauss-Legendre rule on [-1, 1]: Newton iterations on the Legendre recurrence in
    extended precision, the positive roots mirrored (lf_hostprep.h: gauss_legendre is the same routine)."""
    n = int(n)
    if n < 1 or n > 64:
        raise ValueError("gauss_legendre: n must be in 1..64")
    ld = np.longdouble
    pi = ld(np.pi) + ld(1.2246467991473532e-16)
    x, w = np.zeros(n, dtype=ld), np.zeros(n, dtype=ld)
    for i in range((n + 1) // 2):
        z = np.cos(pi * (ld(i) + ld(0.75)) / (ld(n) + ld(0.5)))
        pp = ld(1.0)
        for _ in range(100):
            p1, p2 = ld(1.0), ld(0.0)
            for j in range(1, n + 1):
                p3, p2 = p2, p1
                p1 = ((2 * j - 1) * z * p2 - (j - 1) * p3) / j
            pp = n * (z * p1 - p2) / (z * z - 1)
            dz = p1 / pp
            z = z - dz
            if abs(dz) <= ld(1e-19):
                break
        if n % 2 == 1 and i == n // 2:
            z = ld(0.0)
        p1, p2 = ld(1.0), ld(0.0)
        for j in range(1, n + 1):
            p3, p2 = p2, p1
            p1 = ((2 * j - 1) * z * p2 - (j - 1) * p3) / j
        pp = n * (z * p1 - p2) / (z * z - 1)
        x[i], x[n - 1 - i] = -z, z
        w[i] = w[n - 1 - i] = 2 / ((1 - z * z) * pp * pp)
    return x, w


def composite_table(panels, npan, T):
    """(x[panels * npan] ascending, lnw) of the composite Gauss-Legendre rule of `panels` equal panels with npan nodes each on
    [-T, T] in units of sigma, in the kernel's form: delta = sqrt(2) sigma x, and lnw the log of the whole weight, the
    Gaussian density included - ln[w_j (T / panels) exp(-u^2 / 2) / sqrt(2 pi)] at u = sqrt(2) x.  Extended precision, as
    lf_hostprep.h: wide_table derives the device's."""
    ld = np.longdouble
    gx, gw = gauss_legendre(npan)
    pi = ld(np.pi) + ld(1.2246467991473532e-16)
    half = ld(T) / ld(panels)
    x, lnw = np.empty(panels * npan), np.empty(panels * npan)
    for p in range(panels):
        u = -ld(T) + (2 * p + 1) * half + half * gx
        x[p * npan:(p + 1) * npan] = (u / np.sqrt(ld(2.0))).astype(np.float64)
        lnw[p * npan:(p + 1) * npan] = (np.log(gw * half) - ld(0.5) * u * u - ld(0.5) * np.log(2 * pi)).astype(np.float64)
    return x, lnw


@functools.lru_cache(maxsize=None)
def wide_table(c):
    """(x, lnw) of sigma class c, WIDE_PANELS[c] * WIDE_NPANEL nodes in the kernel's form"""
    return composite_table(WIDE_PANELS[c], WIDE_NPANEL, WIDE_T)


def wide_class(sigma, K=None):
    """The rule of every source: -1 for the Gauss-Hermite order (sigma at or below sigma_max(K); sigma = 0 among them), else
    the first class whose upper edge is not below sigma.  Sigma above the top edge is refused with the limit stated, as
    lf_set_lum_err with "deconv_wide" refuses it."""
    K = DEFAULT_ORDER if K is None else int(K)
    s = np.asarray(sigma, dtype=np.float64)
    if np.any(s > WIDE_SIGMA_MAX):
        raise ValueError("sigma = %.4g dex is above %.2f dex, the largest value the wide rule (option deconv_wide) is validated "
                         "for" % (s.max(), WIDE_SIGMA_MAX))
    cls = np.searchsorted(np.asarray(WIDE_EDGES), s, side="left").astype(np.int64)
    return np.where(s > sigma_max(K), cls, -1)


def _subset(inp, idx):
    """the kernel inputs of the sources idx (ascending, catalogue order) alone"""
    fi = np.asarray(inp["field_ind"])
    sub = dict(inp)
    for k in ("lum", "z", "DLz", "logf", "Om_arr"):
        if inp.get(k) is not None:
            sub[k] = np.asarray(inp[k])[idx]
    sub["field_ind"] = np.searchsorted(idx, fi, side="left").astype(np.int64)
    return sub


def _rules(inp, sigma, K, wide):
    """[(inputs, the sources' places in the catalogue or None for all, x, lnw)]: the Gauss-Hermite order for every source, or
    with wide=True for those at or below its limit, and the classes' tables for the others"""
    x, lnw = gauss_hermite(K)
    if not wide:
        return [(inp, None, x, lnw)]
    cls = wide_class(sigma, K)
    out = []
    for c in range(-1, len(WIDE_EDGES)):
        idx = np.flatnonzero(cls == c)
        if idx.size:
            out.append((_subset(inp, idx), idx) + ((x, lnw) if c < 0 else wide_table(c)))
    return out


def _lcomp(y, v, aC):
    """l = ln fc^(1/d) at y = log10(f / Flim), v = f / f_tau (grad.py: _completeness, the value only)"""
    num = aC * y
    den = np.sqrt(num * num + 1.0)
    d = -np.expm1(-v)
    neg = num < 0.0
    s = np.where(neg, den - num, den + num)
    lnfc = np.where(neg, -np.log(2.0 * den * s), np.log1p(-0.5 / (den * s)))
    return lnfc / d


def sigma_max(K):
    return SIGMA_MAX_BY_ORDER[ORDERS.index(int(K))]


def check_sigma(sigma, n, K=None, unchecked=False):
    """sigma as a float64 array [n], refused as lf_set_lum_err refuses it"""
    s = np.ascontiguousarray(sigma, dtype=np.float64).ravel()
    if s.size != n:
        raise ValueError("sigma must have one value per source (%d), got %d" % (n, s.size))
    if not np.all(np.isfinite(s)) or np.any(s < 0.0):
        raise ValueError("sigma must be finite and >= 0")
    if K is not None and not unchecked and np.any(s > sigma_max(K)):
        raise ValueError("sigma = %.4g dex is above %.2f dex, the largest value the order K = %d is validated for (per-source "
                         "error below 1e-7; K = 32 reaches 0.09)" % (s.max(), sigma_max(K), K))
    return s


def _row_terms(inp, sigma, th, x, lnw, moments=False, nodes=False):
    """Delta_i [N] of one theta row (catalogue order); no prior test: what the formulas give.  moments=True: instead the
    posterior moments of delta over the nodes (csrc/lf_lumpost.h), (e1 [N], e2 [N], e1_abs [N]) = sum_k p_k delta_k, sum_k p_k
    delta_k^2 and sum_k p_k |delta_k|, their numerators carried by the same running maximum; 0 where sigma = 0.  nodes=True:
    instead the nodes themselves (csrc/lf_vefftrue.h), (p [K, N], L [K, N], l [K, N]): the weight p_k = exp(a_k - m) / sum_j
    exp(a_j - m) with the loop's maximum and sum (0 for a node whose exponent is -inf, or when the sum is not > 0), the node's
    true luminosity lum + dl - one rounded product, one rounded add - and l at its true flux; a source with sigma = 0 is one
    node: p = (1, 0, ..), every L = lum.  nodes="product": one more, r [K, N] = p_k exp(-l_k) formed in ONE exponent,
    exp(b_k - m) / sum with b_k = a_k without its + l_k (far below Flim exp(a_k - m) is 0 or subnormal and exp(-l_k) is +inf
    while the product is an ordinary number); exactly 0 where p is 0 by rule (an exponent of -inf, the other nodes of a source
    with sigma = 0)."""
    v = inp["variant"]
    p = G._split(inp, th)
    fi = np.asarray(inp["field_ind"])
    lum = np.asarray(inp["lum"], dtype=float)
    N = lum.shape[0]
    kappa = G._kappa(inp["fcmin"])
    c1l = LN10 * (p["al"] + 1.0)
    if v == "zevol":
        ls = G._basis(np.asarray(inp["z"], dtype=float), inp["pivots"])
        t = np.exp(LN10 * (lum - ls.T @ np.asarray(p["L"], dtype=float)))
    else:
        t = 10.0 ** (lum - 42.0) * np.exp(LN10 * (42.0 - p["L"]))
    logf = G.log_flux(lum, inp["DLz"]) if inp.get("logf") is None else np.asarray(inp["logf"], dtype=float)
    U = 10.0 ** (logf + 17.0)
    if v == "free":
        Flim, aC = np.repeat(np.asarray(p["Flim"], dtype=float), np.diff(fi)), float(p["aC"])
    else:
        Flim, aC = np.repeat(np.asarray(inp["Flim0"], dtype=float), np.diff(fi)), float(inp["alpha0"])
    y0 = (logf + 17.0) - np.log10(Flim)
    v0 = U * (np.exp(LN10 * kappa / aC) / Flim)
    l0 = _lcomp(y0, v0, aC)
    s2 = np.sqrt(2.0) * sigma
    m = np.full(N, -np.inf)
    acc = np.zeros(N)
    num = np.zeros((3, N))             # moments: the weighted numerators of delta, delta^2, |delta|
    if nodes:
        ak, Lk, lk, bk = (np.empty((len(x), N)) for _ in range(4))
    for k in range(len(x)):
        dl = s2 * x[k]
        em = np.expm1(LN10 * dl)
        lc = _lcomp(y0 + dl, v0 * (em + 1.0), aC)
        sch = c1l * dl - t * em
        a = lnw[k] + (sch + (lc - l0))
        skip = a == -np.inf
        if nodes:
            ak[k], Lk[k], lk[k], bk[k] = a, lum + dl, lc, lnw[k] + (sch - l0)
        d = a - m
        e = np.exp(-np.abs(d))
        up = d > 0.0
        acc_n = np.where(up, acc * e + 1.0, acc + e)
        m_n = np.where(up, a, m)
        if moments:
            for j, q in enumerate((dl, dl * dl, np.abs(dl))):
                num[j] = np.where(skip, num[j], np.where(up, num[j] * e + q, num[j] + e * q))
        acc = np.where(skip, acc, acc_n)
        m = np.where(skip, m, m_n)
    if nodes:
        on = sigma > 0.0
        pk = np.where((ak == -np.inf) | ~(acc > 0.0), 0.0, np.exp(ak - m) / acc)
        pk = np.where(on, pk, 0.0)
        pk[0] = np.where(on, pk[0], 1.0)
        if nodes == "product":
            rk = np.where((ak == -np.inf) | ~(acc > 0.0), 0.0, np.exp(bk - m) / acc)
            rk = np.where(on, rk, 0.0)
            rk[0] = np.where(on, rk[0], np.exp(-l0))
            return pk, Lk, lk, rk
        return pk, Lk, lk
    if moments:
        on = sigma > 0.0
        return tuple(np.where(on, num[j] / acc, 0.0) for j in range(3))
    out = m + np.log(acc)
    return np.where(sigma == 0.0, 0.0, out)


def delta(inp, sigma, theta, K=None, terms=False, unchecked=True, wide=False):
    """theta (B, ndim) or (ndim,) -> Delta[B]; with terms=True also Delta_i [B, N] (catalogue order) and S_abs[B] = sum_i
    |Delta_i|, the scale rounding is judged by.  The sum over sources is taken in catalogue order (the device's order is its
    own: chunks of CHUNK sources of one field).  unchecked=False: sigma above the order's validated range is refused.
    wide=True: sources above that range, up to WIDE_SIGMA_MAX, are taken by their class's composite rule (wide_class)."""
    K = DEFAULT_ORDER if K is None else int(K)
    if K not in ORDERS:
        raise ValueError("deconvolve_order must be one of %s" % (ORDERS,))
    th = np.asarray(theta, dtype=np.float64)
    single = th.ndim == 1
    th = np.atleast_2d(th)
    if th.shape[1] != G.ndim_of(inp):
        raise ValueError("theta must be (B, %d), got %s" % (G.ndim_of(inp), th.shape))
    sigma = check_sigma(sigma, len(inp["lum"]), K, unchecked or wide)
    D = np.zeros((len(th), sigma.size))
    with np.errstate(all="ignore"):
        for sub, idx, x, lnw in _rules(inp, sigma, K, wide):
            idx = slice(None) if idx is None else idx
            for b, row in enumerate(th):
                D[b, idx] = _row_terms(sub, sigma[idx], row, x, lnw)
    tot, sabs = D.sum(axis=1), np.abs(D).sum(axis=1)
    if single:
        return (tot[0], D[0], sabs[0]) if terms else tot[0]
    return (tot, D, sabs) if terms else tot


def lnprob_err(inp, sigma, theta, K=None, terms=False, wide=False, cut=None):
    """lnprob + Delta per row, with lnprob from grad.py's twin; a row whose lnprob is -inf stays -inf, NaN becomes -inf.
    terms=True: (value, lnprob, S_abs).  cut=(nodes, sigma (nf, M)): the value under a cut on the observed flux, lnprob +
    Delta - Delta B (lnprob_err_cut)."""
    if cut is not None:
        return lnprob_err_cut(inp, sigma, theta, cut, K=K, terms=terms, wide=wide)
    th = np.asarray(theta, dtype=np.float64)
    single = th.ndim == 1
    th2 = np.atleast_2d(th)
    lp = np.atleast_1d(G.lnprob_grad(inp, th2)[0])
    tot, _, sabs = delta(inp, sigma, th2, K, terms=True, wide=wide)
    with np.errstate(all="ignore"):
        out = np.where(np.isfinite(lp), lp + tot, -np.inf)
    out = np.where(np.isnan(out), -np.inf, out)
    if single:
        return (out[0], lp[0], sabs[0]) if terms else out[0]
    return (out, lp, sabs) if terms else out


def lum_posterior(inp, sigma, theta, K=None, wide=False, terms=False):
    """The per-source posterior of the true log-luminosity under the convolved model, marginalised over the rows of theta
    (csrc/lf_lumpost.h): theta (R, ndim) or (ndim,) -> (m1 [N], m2 [N], n_used).  Per source and row
    the nodes delta_k = sqrt(2) sigma_i x_k of the source's rule (the one delta takes it by: _rules) carry the weights p_k
    proportional to exp(ln w_k + t_ik - t_i); m1 and m2 are the means over the used rows of sum_k p_k delta_k and sum_k p_k
    delta_k^2 (dex, dex^2): true = catalogued + m1, spread sqrt(max(m2 - m1^2, 0)).  A row is used when its plain lnprob
    (grad.py's twin) is finite; n_used = 0: NaN for every source with sigma > 0.  A source with sigma = 0: exactly 0, 0.
    terms=True: also s1_abs [N], the mean over the used rows of sum_k p_k |delta_k|, the scale of m1's rounding."""
    K = DEFAULT_ORDER if K is None else int(K)
    if K not in ORDERS:
        raise ValueError("deconvolve_order must be one of %s" % (ORDERS,))
    th = np.atleast_2d(np.asarray(theta, dtype=np.float64))
    if th.shape[1] != G.ndim_of(inp):
        raise ValueError("theta must be (R, %d), got %s" % (G.ndim_of(inp), th.shape))
    sigma = check_sigma(sigma, len(inp["lum"]), K, True)
    used = th[np.isfinite(np.atleast_1d(G.lnprob_grad(inp, th)[0]))]
    tot = np.zeros((3, sigma.size))
    with np.errstate(all="ignore"):
        for sub, idx, x, lnw in _rules(inp, sigma, K, wide):
            idx = slice(None) if idx is None else idx
            for row in used:                                   # (rows in row order, as the device adds them)
                tot[:, idx] += _row_terms(sub, sigma[idx], row, x, lnw, moments=True)
        out = np.where(sigma > 0.0, tot / len(used) if len(used) else np.full_like(tot, np.nan), 0.0)
    return (out[0], out[1], len(used)) + ((out[2],) if terms else ())


def veff_true(inp, sigma, theta, edges, pref0, vol, K=None, wide=False, cut=None, min_vol_frac=0.0):
    """The deconvolved 1/Veff points (csrc/lf_vefftrue.h): theta (R, ndim) or (ndim,), edges (nbin + 1,)
    ascending -> (values (R, nbin), n_used).  Per row, every source's posterior of its true luminosity - the weights p_k on
    the nodes L_k = lum + dl_k of the source's rule (_rules; a source with sigma = 0: one node at lum with p = 1) - is binned
    with the completeness at the node's TRUE flux:
        values[r][b] = sum_i sum_k [edges[b] <= L_ik < edges[b + 1]] p_irk exp(-l_irk) / (pref0 vol),
    exp(-l) being 1 / fc of the modified Fleming curve.  The bin of a node is searchsorted(edges, L, side="right") - 1; nodes
    outside [edges[0], edges[nbin]) are dropped.  A row is used when its plain lnprob (grad.py's twin) is finite; an unused row
    is NaN.  The posterior is binned as the rule's discrete measure: one source's bin masses are granular at the node spacing,
    the sum over sources spread against the edges is not (the section has the measured figures).
    cut=(nodes, sigma (nf, M)): under a cut on the observed flux every node's pf / (pref0 vol) is
    divided by g_f(L_ik), the part of the survey volume in which its true luminosity is catalogued (cut_volume_fraction); a
    node with g = 0 or g < min_vol_frac adds exactly 0.  cut=None: the bits of before."""
    K = DEFAULT_ORDER if K is None else int(K)
    if K not in ORDERS:
        raise ValueError("deconvolve_order must be one of %s" % (ORDERS,))
    th = np.atleast_2d(np.asarray(theta, dtype=np.float64))
    if th.shape[1] != G.ndim_of(inp):
        raise ValueError("theta must be (R, %d), got %s" % (G.ndim_of(inp), th.shape))
    ed = np.ascontiguousarray(edges, dtype=np.float64).ravel()
    nbin = ed.size - 1
    if nbin < 1 or not np.all(np.isfinite(ed)) or np.any(np.diff(ed) <= 0.0):
        raise ValueError("edges must be finite and strictly ascending, two at least")
    if not (pref0 > 0.0 and vol > 0.0):
        raise ValueError("pref0 and vol must be > 0")
    sigma = check_sigma(sigma, len(inp["lum"]), K, True)
    use = np.isfinite(np.atleast_1d(G.lnprob_grad(inp, th)[0]))
    values = np.full((len(th), nbin), np.nan)
    rules = _rules(inp, sigma, K, wide)
    pv = pref0 * vol
    gtab = None if cut is None else cut_volume_table(inp, sigma, cut, K=K, wide=wide, min_vol_frac=min_vol_frac)[0]
    with np.errstate(all="ignore"):
        for r in np.flatnonzero(use):
            acc = np.zeros(nbin)
            for ir, (sub, idx, x, lnw) in enumerate(rules):
                sg = sigma if idx is None else sigma[idx]
                p, L, l, pf = _row_terms(sub, sg, th[r], x, lnw, nodes="product")
                b = np.searchsorted(ed, L, side="right") - 1
                ok = (b >= 0) & (b < nbin) & (pf > 0.0)
                if gtab is None:
                    acc += np.bincount(b[ok], weights=pf[ok] / pv, minlength=nbin)
                else:
                    g, keep = gtab[ir]
                    ok &= keep
                    acc += np.bincount(b[ok], weights=(pf[ok] / pv) / g[ok], minlength=nbin)
            values[r] = acc
    return values, int(use.sum())


def veff_true_quantiles(inp, sigma, theta, edges, pref0, vol, q=(16.0, 50.0, 84.0), method="linear", K=None, wide=False, cut=None,
                        min_vol_frac=0.0):
    """veff_true and over its used rows np.percentile(q) per bin (method "linear") or np.median (method "median": one row):
    (out (nq, nbin), values (R, nbin), n_used); no used row: NaN everywhere.  cut, min_vol_frac: veff_true's."""
    if method not in ("linear", "median"):
        raise ValueError("method must be 'linear' or 'median'")
    values, used = veff_true(inp, sigma, theta, edges, pref0, vol, K=K, wide=wide, cut=cut, min_vol_frac=min_vol_frac)
    qa = np.atleast_1d(np.asarray(q, dtype=np.float64))
    nq = qa.size if method == "linear" else 1
    if used == 0:
        return np.full((nq, values.shape[1]), np.nan), values, 0
    rows = values[~np.all(np.isnan(values), axis=1)]              # (an unused row is NaN throughout)
    out = np.percentile(rows, qa, axis=0) if method == "linear" else np.median(rows, axis=0)[None]
    return out, values, used


def _lcomp_grad(y, v, aC, kappa):
    """(l, dF, dC) at y = log10(f / Flim), v = f / f_tau: l = ln fc^(1/d), Flim d l / d Flim and d l / d alpha_C (lf_grad.h:
    grad_comp's statements, taken at (y, v) as the kernel's nodes have them)"""
    num = aC * y
    den = np.sqrt(num * num + 1.0)
    e = np.exp(-v)
    d = -np.expm1(-v)
    neg = num < 0.0
    s = np.where(neg, den - num, den + num)
    lnfc = np.where(neg, -np.log(2.0 * den * s), np.log1p(-0.5 / (den * s)))
    gp = np.where(neg, s / (den * den), 1.0 / (den * den * s))
    l = lnfc / d
    lw = np.where(e > 0.0, l * (v * e / d), 0.0)
    dF = lw - gp * (aC / LN10) / d
    dC = lw * (LN10 * kappa / (aC * aC)) + gp * y / d
    return l, dF, dC


def _row_grad_terms(inp, sigma, th, x, lnw):
    """One theta row -> (Delta_i [N], g [N, ndim], sabs [N, ndim]): every source's correction, its derivative with respect to
    the row's elements and the scale of the derivative's terms (csrc/lf_deconv_grad.h).  One online
    softmax per source: the running maximum m, the sum s and one weighted numerator per quantity (delta, em; FREE: dF, dC),
    all rescaled by the same e^(-|d|) when a node raises the maximum."""
    v, fsa = inp["variant"], bool(inp["fix_sch_al"])
    p = G._split(inp, th)
    fi = np.asarray(inp["field_ind"])
    nf = len(fi) - 1
    lum = np.asarray(inp["lum"], dtype=float)
    N = lum.shape[0]
    nd = G.ndim_of(inp)
    kappa = G._kappa(inp["fcmin"])
    c1l = LN10 * (p["al"] + 1.0)
    ls = None
    if v == "zevol":
        ls = G._basis(np.asarray(inp["z"], dtype=float), inp["pivots"])
        t = np.exp(LN10 * (lum - ls.T @ np.asarray(p["L"], dtype=float)))
    else:
        t = 10.0 ** (lum - 42.0) * np.exp(LN10 * (42.0 - p["L"]))
    logf = G.log_flux(lum, inp["DLz"]) if inp.get("logf") is None else np.asarray(inp["logf"], dtype=float)
    U = 10.0 ** (logf + 17.0)
    free = v == "free"
    if free:
        Flim, aC = np.repeat(np.asarray(p["Flim"], dtype=float), np.diff(fi)), float(p["aC"])
    else:
        Flim, aC = np.repeat(np.asarray(inp["Flim0"], dtype=float), np.diff(fi)), float(inp["alpha0"])
    y0 = (logf + 17.0) - np.log10(Flim)
    v0 = U * (np.exp(LN10 * kappa / aC) / Flim)
    l0, dF0, dC0 = _lcomp_grad(y0, v0, aC, kappa)
    s2 = np.sqrt(2.0) * sigma
    m = np.full(N, -np.inf)
    acc = np.zeros(N)
    nq = 4 if free else 2
    num = np.zeros((nq, N))            # the weighted numerators of delta, em (, dF, dC)
    nab = np.zeros((nq, N))            # ... of their absolute values (S_abs only: the kernel does not keep them)
    for k in range(len(x)):
        dl = s2 * x[k]
        em = np.expm1(LN10 * dl)
        lk, dFk, dCk = _lcomp_grad(y0 + dl, v0 * (em + 1.0), aC, kappa)
        a = lnw[k] + ((c1l * dl - t * em) + (lk - l0))
        skip = a == -np.inf
        d = a - m
        e = np.exp(-np.abs(d))
        up = d > 0.0
        acc_n = np.where(up, acc * e + 1.0, acc + e)
        m_n = np.where(up, a, m)
        q = (dl, em, dFk, dCk)[:nq]
        for j in range(nq):
            num[j] = np.where(skip, num[j], np.where(up, num[j] * e + q[j], num[j] + e * q[j]))
            nab[j] = np.where(skip, nab[j], np.where(up, nab[j] * e + np.abs(q[j]), nab[j] + e * np.abs(q[j])))
        acc = np.where(skip, acc, acc_n)
        m = np.where(skip, m, m_n)
    on = sigma > 0.0
    D = np.where(on, m + np.log(acc), 0.0)
    ex = [np.where(on, num[j] / acc, 0.0) for j in range(nq)]          # E_p[.]
    ea = [np.where(on, nab[j] / acc, 0.0) for j in range(nq)]
    g, sabs = np.zeros((N, nd)), np.zeros((N, nd))
    gL, aL = t * ex[1], t * ea[1]
    if v == "zevol":
        for mm in range(3):
            g[:, mm] = LN10 * (ls[mm] * gL)
            sabs[:, mm] = LN10 * (np.abs(ls[mm]) * aL)
        if not fsa:
            g[:, 6], sabs[:, 6] = LN10 * ex[0], LN10 * ea[0]
    else:
        g[:, 0], sabs[:, 0] = LN10 * gL, LN10 * aL
        if not fsa:
            g[:, 2], sabs[:, 2] = LN10 * ex[0], LN10 * ea[0]
        if free:
            kF = 2 if fsa else 3
            for f in range(nf):
                sl = slice(fi[f], fi[f + 1])
                inv = 1.0 / p["Flim"][f]
                g[sl, kF + f] = inv * np.where(on[sl], ex[2][sl] - dF0[sl], 0.0)
                sabs[sl, kF + f] = abs(inv) * np.where(on[sl], ea[2][sl] + np.abs(dF0[sl]), 0.0)
            g[:, kF + nf] = np.where(on, ex[3] - dC0, 0.0)
            sabs[:, kF + nf] = np.where(on, ea[3] + np.abs(dC0), 0.0)
    return D, g, sabs


def delta_grad(inp, sigma, theta, K=None, terms=False, per_source=False, wide=False):
    """theta (B, ndim) or (ndim,) -> (Delta[B], dDelta[B, ndim]): the correction and its derivative with respect to the row's
    own elements, the exact derivative of the K-point sum; with terms=True also S_abs[B, ndim], per element the sum over the
    sources of sum_k p_ik |d a_ik / d theta_e| + |the subtracted term at f_i|: the scale rounding is judged by.  The elements
    of phi* are exactly 0; a source with sigma_i = 0 adds exactly 0 to every element.  No prior test: what the formulas give.
    per_source=True: the per-source arrays (Delta_i [B, N], dDelta_i [B, N, ndim], S_abs_i [B, N, ndim]) instead.
    wide=True: as delta's (the exact derivative of each source's own sum, whichever rule takes it)."""
    K = DEFAULT_ORDER if K is None else int(K)
    if K not in ORDERS:
        raise ValueError("deconvolve_order must be one of %s" % (ORDERS,))
    th = np.asarray(theta, dtype=np.float64)
    single = th.ndim == 1
    th = np.atleast_2d(th)
    nd = G.ndim_of(inp)
    if th.shape[1] != nd:
        raise ValueError("theta must be (B, %d), got %s" % (nd, th.shape))
    sigma = check_sigma(sigma, len(inp["lum"]), K, True)
    N = sigma.size
    D, g, s = np.zeros((len(th), N)), np.zeros((len(th), N, nd)), np.zeros((len(th), N, nd))
    with np.errstate(all="ignore"):
        for sub, idx, x, lnw in _rules(inp, sigma, K, wide):
            idx = slice(None) if idx is None else idx
            for b, row in enumerate(th):
                D[b, idx], g[b, idx], s[b, idx] = _row_grad_terms(sub, sigma[idx], row, x, lnw)
    if per_source:
        return (D[0], g[0], s[0]) if single else (D, g, s)
    out = (D.sum(axis=1), g.sum(axis=1), s.sum(axis=1))
    if single:
        out = tuple(o[0] for o in out)
    return out if terms else out[:2]


def lnprob_err_grad(inp, sigma, theta, K=None, terms=False, wide=False, cut=None, limit=0):
    """(value[B], grad[B, ndim]) of the convolved lnprob: lnprob_err's value, grad.lnprob_grad's gradient plus dDelta; a row
    whose lnprob is not finite gets NaN in every element (the plain gradient's convention).  terms=True: also S_abs[B, ndim],
    the sum of both parts' scales.  cut=(nodes, sigma (nf, M)): under a cut on the observed flux (DESIGN.md sections 3.31,
    3.33) - the value is lnprob_err_cut's, the gradient that minus cut_term_grad's, S_abs with the cut's scale added (limit:
    cut_nodes')."""
    th = np.asarray(theta, dtype=np.float64)
    single = th.ndim == 1
    th2 = np.atleast_2d(th)
    lp, g0, s0 = G.lnprob_grad(inp, th2, terms=True)
    tot, dD, s1 = delta_grad(inp, sigma, th2, K, terms=True, wide=wide)
    with np.errstate(all="ignore"):
        val = np.where(np.isfinite(lp), lp + tot, -np.inf)
        val = np.where(np.isnan(val), -np.inf, val)
        g, s = g0 + dD, s0 + s1                     # (g0, s0 are NaN where lnprob is not finite)
        if cut is not None:
            val = lnprob_err_cut(inp, sigma, th2, cut, K=K, wide=wide, limit=limit)
            _, gB, sB = cut_term_grad(inp, cut[0], cut[1], th2, terms=True, limit=limit)
            g, s = g - gB, s + sB
    if single:
        return (val[0], g[0], s[0]) if terms else (val[0], g[0])
    return (val, g, s) if terms else (val, g)


# ---------------------------------------------------------------------------------------------------------------------------
# The cut on the OBSERVED flux (csrc/lf_deconv_cut.h): contexts with min_comp_frac > 0.001, whose grid
# has its own luminosity nodes per redshift column.  A source is catalogued when L_o = L_t + eps >= Lam(z), the grid's lower
# edge (row 0 of logL), eps ~ N(0, s^2) with s = sigma_f(log10 of the TRUE flux) the field's error model (mock.sigma_lookup's
# arithmetic).  The expected counts become B + Delta B,
#     Delta B = sum_f sum_j wz_j V_j [ int_{Lam-H}^{Lam} phi Omega Q(-u) dL - int_{Lam}^{min(Lam+H, Lh)} phi Omega Q(u) dL ],
#     u = (L - Lam_j) / s_f(L - ld2_j),   Q(x) = erfc(x / sqrt 2) / 2,   H = CUT_T max sigma_f,
# and lnprob_cut = lnprob + Delta - Delta B.  cut_nodes places the same panels as lf_hostprep.h: cut_tables (statements in
# double, written the same way); cut_term evaluates Delta B directly, erfc per node, in double.
CUT_T = 7.5                     # lf_layout.h: DECONV_CUT_*
CUT_NPANEL = 8
CUT_PANEL_SIGMA = 2.5
CUT_H = 0.25
CUT_UMAX = 9.0
CUT_MAX_PANELS = 64
CUT_SIGMA_MAX = 0.30
CUT_MAX_NODES = 64
CUT_CHUNK = 1024


def check_cut_error_model(nodes, sigma, nf):
    """(nodes (M,), sigma (nf, M)) as float64, refused as lf_set_cut_error_model refuses them"""
    nd = np.ascontiguousarray(nodes, dtype=np.float64).ravel()
    sg = np.ascontiguousarray(np.atleast_2d(np.asarray(sigma, dtype=np.float64)))
    M = nd.size
    if M < 1 or M > CUT_MAX_NODES:
        raise ValueError("M must be in 1..%d" % CUT_MAX_NODES)
    if sg.shape != (nf, M):
        raise ValueError("sigma must be (nf, M) = (%d, %d), got %s" % (nf, M, sg.shape))
    if not np.all(np.isfinite(nd)) or np.any(np.diff(nd) <= 0.0):
        raise ValueError("nodes must be finite and increase")
    if not np.all(np.isfinite(sg)) or np.any(sg < 0.0):
        raise ValueError("sigma must be finite and >= 0")
    if np.any(sg > CUT_SIGMA_MAX):
        raise ValueError("sigma = %.4g dex is above %.2f dex, the largest value the cut model is validated for (per-column error "
                         "below 1e-7)" % (sg.max(), CUT_SIGMA_MAX))
    for f in range(nf):
        z = int(np.sum(sg[f] == 0.0))
        if z not in (0, M):
            raise ValueError("the sigma of field %d is 0 at some nodes and not at others: all 0 (no errors) or all > 0" % f)
    return nd, sg


def _cut_sigma(nodes, sig, t):
    """one field's sigma at log10 flux t, a scalar: lf_hostprep.h: cut_sigma's statements"""
    M = len(nodes)
    if M == 1 or not (t > nodes[0]):
        return float(sig[0])
    if t >= nodes[M - 1]:
        return float(sig[M - 1])
    i = min(max(int(np.searchsorted(nodes, t, side="right")) - 1, 0), M - 2)
    return float(sig[i] + (t - nodes[i]) * ((sig[i + 1] - sig[i]) / (nodes[i + 1] - nodes[i])))


def _cut_panels(lam, total, dirn, ld2, nodes, sig):
    """[(d, h)]: the panels of one side of one (field, column), from the edge outwards (lf_hostprep.h: cut_tables' loop)"""
    brk = []
    for m in range(len(nodes)):
        x = float(nodes[m]) + ld2
        dk = lam - x if dirn < 0 else x - lam
        if 0.0 < dk < total:
            brk.append(dk)
    brk.sort()
    out, d, kb = [], 0.0, 0
    while d < total:
        while kb < len(brk) and brk[kb] <= d:
            kb += 1
        seg_end = brk[kb] if kb < len(brk) else total
        s0 = _cut_sigma(nodes, sig, lam + dirn * d - ld2)
        h = min(min(CUT_PANEL_SIGMA * s0, CUT_H), seg_end - d)
        s1 = _cut_sigma(nodes, sig, lam + dirn * (d + h) - ld2)
        if s1 < s0:
            h = min(h, CUT_PANEL_SIGMA * s1)
            s1 = _cut_sigma(nodes, sig, lam + dirn * (d + h) - ld2)
        dn = d + h
        if seg_end - dn < 1.0e-9:
            dn = seg_end
            h = dn - d
        if not h > 0.0:
            break
        if not d > CUT_UMAX * max(s0, s1):
            out.append((d, h))
            if len(out) > CUT_MAX_PANELS:
                raise ValueError("the error model needs more than %d panels on one side of the cut: its sigma varies too strongly "
                                 "across the band of 7.5 sigma_max" % CUT_MAX_PANELS)
        d = dn
    return out


def _cut_grid(inp):
    logL = np.asarray(inp["logL"], dtype=np.float64)
    zarr = np.asarray(inp["zarr"], dtype=np.float64)
    wz = np.zeros_like(zarr)
    dz = np.diff(zarr)
    wz[1:] += dz
    wz[:-1] += dz
    wz *= 0.5                                            # (0.5 (dl + dr): lf_hostprep.h's statement)
    ld2 = np.log10(4.0 * np.pi * (G.MPC_CM * np.asarray(inp["DL_zarr"], dtype=np.float64)) ** 2)
    return logL[0], logL[-1], zarr, wz, np.asarray(inp["volume_part"], dtype=np.float64), ld2


def _cut_sigma_vec(nodes, sig, t):
    """_cut_sigma for an array t: the same statements, element by element"""
    M = len(nodes)
    if M == 1:
        return np.full(np.shape(t), float(sig[0]))
    i = np.clip(np.searchsorted(nodes, t, side="right") - 1, 0, M - 2)
    s = sig[i] + (t - nodes[i]) * ((sig[i + 1] - sig[i]) / (nodes[i + 1] - nodes[i]))
    s = np.where(t >= nodes[M - 1], sig[M - 1], s)
    return np.where(t > nodes[0], s, sig[0])


def cut_volume_fraction(inp, nodes, sigma, field, L):
    """g_f(L), the part of the survey volume in which a true luminosity L of field f is catalogued under the cut on the observed
    flux (csrc/lf_vefftrue_cut.h), on the likelihood's own grid and with its own error model:
        g_f(L) = (sum_j wv_j Q(-u_fj)) / (sum_j wv_j),  wv_j = wz_j V_j,  u_fj = (L - lam_j) / s_f(L - ld2_j),
    Q(x) = erfc(x / sqrt 2) / 2.  field (n,) or a scalar, L (n,) -> g (n,).  The kernel's statements: the columns added left to
    right into one accumulator, the denominator the same way; u > CUT_UMAX: a term of exactly wv_j, u < -CUT_UMAX: exactly 0,
    else wv_j 0.5 erfc(-u / sqrt 2); a field whose sigma is 0 at every node: the step, wv_j when L >= lam_j."""
    from scipy.special import erfc
    nf = len(inp["field_ind"]) - 1
    nd, sg = check_cut_error_model(nodes, sigma, nf)
    Lq = np.atleast_1d(np.asarray(L, dtype=np.float64))
    fq = np.broadcast_to(np.asarray(field, dtype=np.int64), Lq.shape)
    if np.any(fq < 0) or np.any(fq >= nf):
        raise ValueError("field must be in 0..%d" % (nf - 1))
    lam, _, _, wz, vol, ld2 = _cut_grid(inp)
    wv = wz * vol
    den = 0.0
    for j in range(len(wv)):
        den = den + float(wv[j])
    g = np.zeros(Lq.shape)
    with np.errstate(all="ignore"):
        for f in np.unique(fq):
            at = fq == f
            Lf = Lq[at]
            acc = np.zeros(Lf.shape)
            step = bool(np.all(sg[f] == 0.0))
            for j in range(len(wv)):
                if step:
                    term = np.where(Lf >= lam[j], wv[j], 0.0)
                else:
                    u = (Lf - lam[j]) / _cut_sigma_vec(nd, sg[f], Lf - ld2[j])
                    term = np.where(u > CUT_UMAX, wv[j], np.where(u < -CUT_UMAX, 0.0, wv[j] * (0.5 * erfc(-u / np.sqrt(2.0)))))
                acc = acc + term
            g[at] = acc / den
    return g


def cut_volume_table(inp, sigma, cut, K=None, wide=False, min_vol_frac=0.0):
    """([(g [K_rule, N_rule], keep [K_rule, N_rule])] per rule of _rules, n_dropped): cut_volume_fraction at every node L_ik =
    lum_i + sqrt(2) sigma_i x_k of every source's rule (one rounded product, one rounded add: the bits that choose the bin),
    which nodes are kept (g > 0 and g >= min_vol_frac), and how many (source, node) slots are dropped - a source with sigma
    = 0 has one slot, its node at lum_i.  None of it depends on theta."""
    K = DEFAULT_ORDER if K is None else int(K)
    sigma = check_sigma(sigma, len(inp["lum"]), K, True)
    out, dropped = [], 0
    for sub, idx, x, lnw in _rules(inp, sigma, K, wide):
        sg = sigma if idx is None else sigma[idx]
        lum = np.asarray(sub["lum"], dtype=np.float64)
        fld = np.repeat(np.arange(len(sub["field_ind"]) - 1), np.diff(np.asarray(sub["field_ind"])))
        L = lum[None, :] + (np.sqrt(2.0) * sg)[None, :] * np.asarray(x)[:, None]
        g = cut_volume_fraction(inp, cut[0], cut[1], np.broadcast_to(fld, L.shape).ravel(), L.ravel()).reshape(L.shape)
        keep = (g > 0.0) & (g >= min_vol_frac)
        slot = np.ones(L.shape, dtype=bool)
        slot[1:, sg == 0.0] = False
        dropped += int(np.sum(slot & ~keep))
        out.append((g, keep))
    return out, dropped


def cut_nodes(inp, nodes, sigma, limit=0, fields=None):
    """The node list of Delta B: per field a dict L, col, w (the signed weight of Delta B without Omega: +/- wz_j V_j (GL
    weight) Q(|u|); + below the edge, - above), logf (L - ld2_j); nodes whose w is exactly 0 dropped; limit > 0: the first
    `limit` nodes only (option "deconv_cut_limit").  Also H (nf,)."""
    nf = len(inp["field_ind"]) - 1
    nd, sg = check_cut_error_model(nodes, sigma, nf)
    from scipy.special import erfc
    lam, top, zarr, wz, vol, ld2 = _cut_grid(inp)
    gxl, gwl = gauss_legendre(CUT_NPANEL)
    gx, gw = gxl.astype(np.float64), gwl.astype(np.float64)
    out, H = [], np.zeros(nf)
    for f in range(nf):
        H[f] = CUT_T * sg[f].max()
        Ls, cols, ws = [], [], []
        for j in range(len(zarr) if H[f] > 0.0 and (fields is None or f in fields) else 0):
            for dirn in (-1.0, 1.0):
                total = H[f] if dirn < 0 else min(lam[j] + H[f], top[j]) - lam[j]
                for d, h in _cut_panels(float(lam[j]), float(total), dirn, float(ld2[j]), nd, sg[f]):
                    half = 0.5 * h
                    mid = (lam[j] + dirn * d) + dirn * half
                    Ln = mid + half * gx
                    s = np.array([_cut_sigma(nd, sg[f], t) for t in Ln - ld2[j]])
                    u = (Ln - lam[j]) / s
                    w = -dirn * (wz[j] * vol[j]) * (half * gw) * (0.5 * erfc(np.abs(u) / np.sqrt(2.0)))
                    Ls.append(Ln), cols.append(np.full(CUT_NPANEL, j)), ws.append(w)
        L = np.concatenate(Ls) if Ls else np.zeros(0)
        col = np.concatenate(cols).astype(np.int64) if Ls else np.zeros(0, dtype=np.int64)
        w = np.concatenate(ws) if Ls else np.zeros(0)
        keep = w != 0.0
        L, col, w = L[keep], col[keep], w[keep]
        if limit > 0:
            L, col, w = L[:limit], col[:limit], w[:limit]
        out.append({"L": L, "col": col, "w": w, "logf": L - ld2[col]})
    return out, H


def _cut_phi_omega(inp, th, f, L, col, logf):
    """phi_theta(L[, z_col]) Omega_theta(L, z_col) of field f's nodes at one theta row: piece B's node form, float Omega_0"""
    v = inp["variant"]
    p = G._split(inp, th)
    c1 = p["al"] + 1.0
    kappa = G._kappa(inp["fcmin"])
    om0 = float(np.asarray(inp["Omega_0"], dtype=np.float64)[f]) / G.SQARCSEC
    if v == "zevol":
        lg = G._basis(np.asarray(inp["zarr"], dtype=np.float64)[col], inp["pivots"])
        x = L - np.tensordot(np.asarray(p["L"], dtype=float), lg, axes=1)
        ph = np.tensordot(np.asarray(p["phi"], dtype=float), lg, axes=1)
    else:
        x, ph = L - p["L"], p["phi"]
    tlf = LN10 * np.exp(LN10 * (ph + x * c1) - 10.0 ** x)
    if v == "free":
        Flim, aC = float(p["Flim"][f]), float(p["aC"])
    else:
        Flim, aC = float(np.asarray(inp["Flim0"], dtype=float)[f]), float(inp["alpha0"])
    y = (logf + 17.0) - np.log10(Flim)
    vv = 10.0 ** (logf + 17.0) * (np.exp(LN10 * kappa / aC) / Flim)
    return tlf * om0 * np.exp(_lcomp(y, vv, aC))


def cut_term(inp, nodes, sigma, theta, terms=False, limit=0, fields=None, per_column=False):
    """theta (B, ndim) or (ndim,) -> Delta B [B]; terms=True: also S_abs [B] = sum_n |c_n phi Omega|, the scale rounding is
    judged by.  No prior test: what the formulas give (the device gives NaN for a row whose plain lnprob is not finite).  A
    node whose term is 0 or NaN adds exactly 0.  Summed field by field in node order.  fields: only these fields' nodes.
    per_column=True: instead Delta B per (row, field, column) [B, nf, S]."""
    th = np.asarray(theta, dtype=np.float64)
    single = th.ndim == 1
    th = np.atleast_2d(th)
    if th.shape[1] != G.ndim_of(inp):
        raise ValueError("theta must be (B, %d), got %s" % (G.ndim_of(inp), th.shape))
    nl, _ = cut_nodes(inp, nodes, sigma, limit=limit, fields=fields)
    S = len(inp["zarr"])
    tot, sabs = np.zeros(len(th)), np.zeros(len(th))
    pc = np.zeros((len(th), len(nl), S))
    with np.errstate(all="ignore"):
        for b, row in enumerate(th):
            for f, n in enumerate(nl):
                if n["L"].size == 0:
                    continue
                I = n["w"] * _cut_phi_omega(inp, row, f, n["L"], n["col"], n["logf"])
                I = np.where(np.abs(I) > 0.0, I, 0.0)
                tot[b] += I.sum()
                sabs[b] += np.abs(I).sum()
                if per_column:
                    pc[b, f] = np.bincount(n["col"], weights=I, minlength=S)
    if per_column:
        return pc[0] if single else pc
    if single:
        return (tot[0], sabs[0]) if terms else tot[0]
    return (tot, sabs) if terms else tot


def lnprob_err_cut(inp, sigma, theta, cut, K=None, terms=False, wide=False, limit=0):
    """lnprob + Delta - Delta B per row: lnprob_err's value and cut_term's, cut = (nodes, sigma (nf, M)); a row whose lnprob is
    not finite stays -inf.  terms=True: (value, lnprob, S_abs of Delta + S_abs of Delta B)."""
    th = np.asarray(theta, dtype=np.float64)
    single = th.ndim == 1
    th2 = np.atleast_2d(th)
    val, lp, sabs = lnprob_err(inp, sigma, th2, K=K, terms=True, wide=wide)
    dB, sB = cut_term(inp, cut[0], cut[1], th2, terms=True, limit=limit)
    with np.errstate(all="ignore"):
        out = np.where(np.isfinite(lp), val - dB, -np.inf)
    out = np.where(np.isnan(out), -np.inf, out)
    if single:
        return (out[0], lp[0], sabs[0] + sB[0]) if terms else out[0]
    return (out, lp, sabs + sB) if terms else out


def _cut_grad_terms(inp, th, f, L, col, logf, w):
    """Field f's nodes at one theta row -> (I [n], d [n, ndim]): the terms I_n = w_n phi Omega of Delta B (cut_term's, the same
    statements but for the z-evolving L*(z) and phi*(z), below) and every term's share of d Delta B / d theta_e - I_n times piece B's node derivatives (csrc/lf_grad.h: ln10
    (10^x - alpha - 1), ln10, ln10 x for L*, phi*, alpha; z-evolving: times the Lagrange basis; FREE: dF / Flim_f in field f's
    element, dC).  A node whose I is 0 or NaN is exactly 0 throughout."""
    v, fsa = inp["variant"], bool(inp["fix_sch_al"])
    p = G._split(inp, th)
    nd = G.ndim_of(inp)
    nf = len(inp["field_ind"]) - 1
    c1 = p["al"] + 1.0
    kappa = G._kappa(inp["fcmin"])
    om0 = float(np.asarray(inp["Omega_0"], dtype=np.float64)[f]) / G.SQARCSEC
    lg = None
    if v == "zevol":
        # L*(z) = sum_m l_m(z) L_m at |L_m| of 43 carries 43 eps sum_m |l_m| in double, which 10^x turns into a relative 1e-14 of
        # every term (the kernel's and cut_term's x; nothing cancels it).  Here the basis and both sums are taken in extended
        # precision and rounded once, so that the formula test against 30 digits sees the formulas, not that rounding.
        ld = np.longdouble
        z = np.asarray(inp["zarr"], dtype=np.float64)[col].astype(ld)
        z1, z2, z3 = (ld(float(q)) for q in inp["pivots"])
        le = [(z - z2) * (z - z3) / ((z1 - z2) * (z1 - z3)), (z - z1) * (z - z3) / ((z2 - z1) * (z2 - z3)),
              (z - z1) * (z - z2) / ((z3 - z1) * (z3 - z2))]
        x = (L.astype(ld) - sum(le[m] * ld(float(p["L"][m])) for m in range(3))).astype(np.float64)
        ph = sum(le[m] * ld(float(p["phi"][m])) for m in range(3)).astype(np.float64)
        lg = [q.astype(np.float64) for q in le]
    else:
        x, ph = L - p["L"], p["phi"]
    t = 10.0 ** x
    tlf = LN10 * np.exp(LN10 * (ph + x * c1) - t)
    if v == "free":
        Flim, aC = float(p["Flim"][f]), float(p["aC"])
    else:
        Flim, aC = float(np.asarray(inp["Flim0"], dtype=float)[f]), float(inp["alpha0"])
    y = (logf + 17.0) - np.log10(Flim)
    vv = 10.0 ** (logf + 17.0) * (np.exp(LN10 * kappa / aC) / Flim)
    lc, dF, dC = _lcomp_grad(y, vv, aC, kappa)
    I = w * (tlf * om0 * np.exp(lc))
    ok = np.abs(I) > 0.0
    I = np.where(ok, I, 0.0)
    d = np.zeros((L.size, nd))
    wl = LN10 * (I * (t - c1))
    if v == "zevol":
        for m in range(3):
            d[:, m] = lg[m] * wl
            d[:, 3 + m] = LN10 * (lg[m] * I)
        if not fsa:
            d[:, 6] = LN10 * (I * x)
    else:
        d[:, 0] = wl
        d[:, 1] = LN10 * I
        if not fsa:
            d[:, 2] = LN10 * (I * x)
        if v == "free":
            kF = 2 if fsa else 3
            d[:, kF + f] = (I * dF) / Flim
            d[:, kF + nf] = I * dC
    return I, np.where(ok[:, None], d, 0.0)


def cut_term_grad(inp, nodes, sigma, theta, terms=False, limit=0, fields=None):
    """theta (B, ndim) or (ndim,) -> (Delta B [B], d Delta B / d theta [B, ndim]): cut_term's sum over cut_nodes' tables (FREE,
    FIXCOMP: its bits; z-evolving: within 1e-13 of its scale, _cut_grad_terms says why) and its exact derivative with respect to the row's own elements, field by field in node order (csrc/lf_deconv_cut_grad.h; DESIGN.md
    section 3.33).  terms=True: also S_abs [B, ndim], per element the sum of the absolute values of its terms, the scale
    rounding is judged by.  No prior test: what the formulas give.  A node whose term is 0 or NaN adds exactly 0 to every
    element; the Flim_g element holds field g's nodes only.  fields: only these fields' nodes."""
    th = np.asarray(theta, dtype=np.float64)
    single = th.ndim == 1
    th = np.atleast_2d(th)
    nd = G.ndim_of(inp)
    if th.shape[1] != nd:
        raise ValueError("theta must be (B, %d), got %s" % (nd, th.shape))
    nl, _ = cut_nodes(inp, nodes, sigma, limit=limit, fields=fields)
    tot, g, sabs = np.zeros(len(th)), np.zeros((len(th), nd)), np.zeros((len(th), nd))
    with np.errstate(all="ignore"):
        for b, row in enumerate(th):
            for f, n in enumerate(nl):
                if n["L"].size == 0:
                    continue
                I, d = _cut_grad_terms(inp, row, f, n["L"], n["col"], n["logf"], n["w"])
                tot[b] += I.sum()
                g[b] += d.sum(axis=0)
                sabs[b] += np.abs(d).sum(axis=0)
    if single:
        return (tot[0], g[0], sabs[0]) if terms else (tot[0], g[0])
    return (tot, g, sabs) if terms else (tot, g)
