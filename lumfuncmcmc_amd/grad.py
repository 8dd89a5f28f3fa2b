"""NumPy twin of the device gradient (csrc/lf_grad.h): d lnprob / d theta in closed form, no GPU.

lnprob = A - B with A the per-source log-term sum and B the expected-count integral (the two pieces of lf_lnprob_pieces),
differentiated with respect to a row's own theta elements, in theta's own units (Flim in 1e-17).  The formulas are the
kernels', written for arrays:

    x = lum - L*, t = 10^x, c1 = alpha + 1:   d ln tlf / d L* = ln10 (t - c1),  d / d phi* = ln10,  d / d alpha = ln10 x
    z-evolving: L*(z) = sum_m l_m(z) L_m, phi*(z) = sum_m l_m(z) phi_m (Lagrange basis on the pivots): the above times l_m(z)
    completeness fc^(1/d):  l = ln(fc) / d,  y = log10(f / F),  num = alpha_C y,  den = sqrt(1 + num^2),
        v = f / f_tau = (f / F) 10^(kappa / alpha_C),  d = -expm1(-v),  w = v e^(-v) / d,
        num >= 0: ln fc = log1p(-1 / (2 den (den + num))),  g' = 1 / (den^2 (den + num))
        num <  0: ln fc = -ln(2 den (den - num)),           g' = (den - num) / den^2
        d l / d Flim = (l w - g' alpha_C / (ln10 d)) / Flim,   d l / d alpha_C = g' y / d + l w ln10 kappa / alpha_C^2

Piece B uses piece_b's trapezoid weights on all nf S^2 lattice points; a point whose integrand is exactly 0 adds exactly 0.
Rows whose lnprob is -inf (outside the prior box, or an underflowing product) get NaN in every element.
"""
import numpy as np

LN10 = np.log(10.0)
SQARCSEC = (180.0 / np.pi * 3600.0) ** 2
MPC_CM = 3.086e24


def ndim_of(inp):
    nf = len(inp["field_ind"]) - 1
    fsa = bool(inp["fix_sch_al"])
    if inp["variant"] == "free":
        return 2 + (0 if fsa else 1) + nf + 1
    if inp["variant"] == "fixcomp":
        return 2 + (0 if fsa else 1)
    return 6 + (0 if fsa else 1)


def _split(inp, th):
    v, fsa = inp["variant"], bool(inp["fix_sch_al"])
    nf = len(inp["field_ind"]) - 1
    if v == "zevol":
        return {"L": th[0:3], "phi": th[3:6], "al": inp["sch_al0"] if fsa else th[6]}
    k = 2 if fsa else 3
    p = {"L": th[0], "phi": th[1], "al": inp["sch_al0"] if fsa else th[2]}
    if v == "free":
        p["Flim"], p["aC"] = th[k:k + nf], th[k + nf]
    else:
        p["Flim"], p["aC"] = np.asarray(inp["Flim0"], dtype=float), float(inp["alpha0"])
    return p


def _in_prior(inp, p):
    lims = inp["lims"]

    def inc(x, name):
        return bool(np.all((np.asarray(x) >= lims[name][0]) & (np.asarray(x) <= lims[name][1])))

    def strict(x, name):
        return bool(np.all((np.asarray(x) > lims[name][0]) & (np.asarray(x) < lims[name][1])))

    if inp["variant"] == "zevol":
        ok = True if inp["fix_sch_al"] else inc(p["al"], "sch_al")
        return ok and strict(p["L"], "Lstar") and strict(p["phi"], "phistar")
    return inc(p["L"], "Lstar") and inc(p["phi"], "phistar") and inc(p["al"], "sch_al") and inc(p["Flim"], "Flim") and \
        inc(p["aC"], "alpha")


def _kappa(fcmin):
    a = (2.0 * fcmin - 1.0) ** 2
    return np.sqrt(abs(a / (1.0 - a)))


def _completeness(logf, Flim, aC, kappa):
    """l = ln of the completeness at log10 flux `logf`, and d l / d Flim, d l / d alpha_C."""
    y = (logf + 17.0) - np.log10(Flim)
    num = aC * y
    den = np.sqrt(1.0 + num * num)
    v = 10.0 ** (y + kappa / aC)
    e = np.exp(-v)
    d = -np.expm1(-v)
    neg = num < 0.0
    s = np.where(neg, den - num, den + num)
    lnfc = np.where(neg, -np.log(2.0 * den * s), np.log1p(-0.5 / (den * s)))
    gp = np.where(neg, s / (den * den), 1.0 / (den * den * s))
    l = lnfc / d
    lw = np.where(e > 0.0, l * (v * e / d), 0.0)
    dF = (lw - gp * aC / (LN10 * d)) / Flim
    dC = gp * y / d + lw * LN10 * kappa / (aC * aC)
    return l, dF, dC


def _basis(z, piv):
    z1, z2, z3 = piv
    a, b, c = z - z1, z - z2, z - z3
    return np.array([b * c / ((z1 - z2) * (z1 - z3)), a * c / ((z2 - z1) * (z2 - z3)), a * b / ((z3 - z1) * (z3 - z2))])


def lattice_weights(inp):
    """W[j][k]: piece_b's nested trapezoid rule as one weight per lattice point (luminosity spacing per column x redshift)."""
    logL, zarr = np.asarray(inp["logL"], dtype=float), np.asarray(inp["zarr"], dtype=float)
    wl = np.zeros_like(logL)
    dl = np.diff(logL, axis=0)
    wl[:-1] += 0.5 * dl
    wl[1:] += 0.5 * dl
    wz = np.zeros_like(zarr)
    dz = np.diff(zarr)
    wz[:-1] += 0.5 * dz
    wz[1:] += 0.5 * dz
    return wl * wz[None, :]


def log_flux(lum, dl_mpc):
    return np.asarray(lum, dtype=float) - np.log10(4.0 * np.pi * (MPC_CM * np.asarray(dl_mpc, dtype=float)) ** 2)


def _row(inp, th, W):
    """One theta row -> (lnprob, grad[ndim], S_abs[ndim])."""
    nd = ndim_of(inp)
    nan = np.full(nd, np.nan)
    p = _split(inp, th)
    if not _in_prior(inp, p):
        return -np.inf, nan, nan
    v, fsa = inp["variant"], bool(inp["fix_sch_al"])
    fi = np.asarray(inp["field_ind"])
    nf = len(fi) - 1
    lum = np.asarray(inp["lum"], dtype=float)
    logL = np.asarray(inp["logL"], dtype=float)
    c1 = p["al"] + 1.0
    kappa = _kappa(inp["fcmin"])
    g = np.zeros(nd)
    sabs = np.zeros(nd)

    def add(e, terms, sign=1.0):
        g[e] += sign * np.sum(terms)
        sabs[e] += np.sum(np.abs(terms))

    with np.errstate(all="ignore"):
        if v == "zevol":
            piv = inp["pivots"]
            ls = _basis(np.asarray(inp["z"], dtype=float), piv)
            x = lum - ls.T @ p["L"]
            t = 10.0 ** x
            lntlf = np.log(LN10) + LN10 * (ls.T @ p["phi"] + x * c1) - t
            A = np.sum(np.log(np.exp(lntlf) * inp["Om_arr"]))
            for m in range(3):
                add(m, LN10 * ls[m] * (t - c1))
                add(3 + m, LN10 * ls[m])
            if not fsa:
                add(6, LN10 * x)
            lg = _basis(np.repeat(np.asarray(inp["zarr"], dtype=float)[None], logL.shape[0], axis=0), piv)
            xg = logL - np.tensordot(p["L"], lg, axes=1)
            tg = 10.0 ** xg
            ip = inp["integ_part"] if inp.get("integ_part") is not None else inp["integ_sum"][None]
            I = W * np.sum(ip, axis=0) * LN10 * np.exp(LN10 * (np.tensordot(p["phi"], lg, axes=1) + xg * c1) - tg)
            Bv = np.sum(I)
            ok = np.abs(I) > 0.0
            for m in range(3):
                add(m, np.where(ok, I * LN10 * lg[m] * (tg - c1), 0.0), -1.0)
                add(3 + m, np.where(ok, I * LN10 * lg[m], 0.0), -1.0)
            if not fsa:
                add(6, np.where(ok, I * LN10 * xg, 0.0), -1.0)
        else:
            x = lum - p["L"]
            t = 10.0 ** x
            lntlf = np.log(LN10) + LN10 * (p["phi"] + x * c1) - t
            k = 2 if fsa else 3
            add(0, LN10 * (t - c1))
            add(1, np.full(lum.shape, LN10))
            if not fsa:
                add(2, LN10 * x)
            xg = logL - p["L"]
            tg = 10.0 ** xg
            tlfg = LN10 * np.exp(LN10 * (p["phi"] + xg * c1) - tg)
            if v == "free":
                logf = log_flux(lum, inp["DLz"]) if inp.get("logf") is None else np.asarray(inp["logf"], dtype=float)
                om = np.zeros(lum.shape)
                for f in range(nf):
                    sl = slice(fi[f], fi[f + 1])
                    l, dF, dC = _completeness(logf[sl], p["Flim"][f], p["aC"], kappa)
                    om[sl] = float(int(inp["Omega_0"][f])) / SQARCSEC * np.exp(l)
                    add(k + f, dF)
                    add(k + nf, dC)
                A = np.sum(np.log(np.exp(lntlf) * om))
                logfg = logL - np.log10(4.0 * np.pi * (MPC_CM * np.asarray(inp["DL_zarr"], dtype=float)) ** 2)[None, :]
                Wv = W * np.asarray(inp["volume_part"], dtype=float)[None, :]
                Bv = 0.0
                for f in range(nf):
                    l, dF, dC = _completeness(logfg, p["Flim"][f], p["aC"], kappa)
                    I = Wv * (inp["Omega_0"][f] / SQARCSEC) * tlfg * np.exp(l)
                    ok = np.abs(I) > 0.0
                    Bv += np.sum(np.where(ok, I, 0.0))
                    add(0, np.where(ok, I * LN10 * (tg - c1), 0.0), -1.0)
                    add(1, np.where(ok, I * LN10, 0.0), -1.0)
                    if not fsa:
                        add(2, np.where(ok, I * LN10 * xg, 0.0), -1.0)
                    add(k + f, np.where(ok, I * dF, 0.0), -1.0)
                    add(k + nf, np.where(ok, I * dC, 0.0), -1.0)
            else:
                A = np.sum(np.log(np.exp(lntlf) * inp["Om_arr"]))
                ip = inp["integ_part"] if inp.get("integ_part") is not None else inp["integ_sum"][None]
                I = W * np.sum(ip, axis=0) * tlfg
                ok = np.abs(I) > 0.0
                Bv = np.sum(np.where(ok, I, 0.0))
                add(0, np.where(ok, I * LN10 * (tg - c1), 0.0), -1.0)
                add(1, np.where(ok, I * LN10, 0.0), -1.0)
                if not fsa:
                    add(2, np.where(ok, I * LN10 * xg, 0.0), -1.0)
    lp = A - Bv
    if not np.isfinite(lp):
        return -np.inf, nan, nan
    return lp, g, sabs


def lnprob_grad(inp, theta, terms=False):
    """theta (K, ndim) or (ndim,) -> (lnprob[K], grad[K, ndim]); with terms=True also S_abs[K, ndim], the sum of the
    absolute values of all per-source and per-lattice-point contributions to each element: the scale rounding is judged by.
    A single row (ndim,) gives (lnprob, grad[ndim](, S_abs[ndim])).  Rows are evaluated one by one: a row's bits do not depend
    on the batch."""
    th = np.asarray(theta, dtype=np.float64)
    single = th.ndim == 1
    th = np.atleast_2d(th)
    nd = ndim_of(inp)
    if th.shape[1] != nd:
        raise ValueError("theta must be (K, %d), got %s" % (nd, th.shape))
    W = lattice_weights(inp)
    lp, g, s = np.empty(len(th)), np.empty((len(th), nd)), np.empty((len(th), nd))
    for i, row in enumerate(th):
        lp[i], g[i], s[i] = _row(inp, row, W)
    if single:
        return (lp[0], g[0], s[0]) if terms else (lp[0], g[0])
    return (lp, g, s) if terms else (lp, g)
