"""Inputs, 40-digit references and yardsticks for the element-wise probes of the gradient and flux-error forms
(csrc/lf_grad.h, csrc/lf_deconv.h, csrc/lf_deconv_grad.h) and of lf_veff's weights, in tests/lf_problib.py's format and under
its rules.  No GPU here: tests/test_gradterms_cpu.py checks the generators, measures the NumPy binary64 figures behind the
caps and shows that the metric sees a subtle error; tests/test_gpu_gradterms.py and tests/test_gpu_veff.py run the same cases
through tests/grad_probe.hip and lf_veff.

A case holds the exact binary64 inputs, `ref` (hi, lo) from mpmath at 40 digits, `yard`, `np` (the same expression in plain
NumPy binary64, taken from deconv._lcomp_grad, deconv._lcomp, deconv._row_terms, deconv._row_grad_terms and grad._basis) and
`exempt`.  Yardsticks, from the formula and the format alone:

  l, the basis, x:  the unit in the last place of the reference.
  dF:               the same for alpha_C > 0 (its two addends have one sign); for alpha_C < 0 as dC.
  dC:               2^-53 (|l w ln10 kappa / alpha_C^2| + |g' y / d|), its two addends at 40 digits.
  grad_comp:        forms y = (logf + 17) - log10 Flim and v = U 10^(kappa / alpha_C) / Flim itself: the roundings of those,
                    dy = 2^-53 (2 |lF| + |logf + 17| + |y|), dv = 2^-53 v (4 + 2 |ln10 kappa / alpha_C|), enter as
                    |X(y + dy, v) - X(y, v)| + |X(y, v + dv) - X(y, v)| at 40 digits, added to the above.
  what passes through an exponential (the lattice integrand I and its slots, t = 10^(L - L*)):
                    2^-53 x (the result's own addends' magnitude) x (1 + A), A the largest magnitude among the exponent's
                    addends (lf_problib.yard_E's rule); t enters I's exponent and the slot I (t - c1) with its own condition,
                    t (1 + A_t).  Where exp or I underflows, the absolute floor 2^-1074 times the factors it is multiplied
                    with is added.
  Delta_i = ln sum_k e^(a_k):  the sum S has positive addends, dS = 2^-53 S (1 + A), so dDelta = 2^-53 (1 + A), plus the
                    rounding of the result: 2^-53 (|Delta_i| + 1 + A); A over the nodes with p_ik >= 2^-53 of |c1l delta_k|,
                    |t em_k| (t with the condition of its own exponent, t (1 + A_t)), |l(f E_k)|, |l(f)|, |ln w_k|.
  sum_k p_ik q_k:   2^-53 (sum_k p_ik |q_k|) (1 + A); the differences nF / s - c0.dF and nC / s - c0.dC against
                    sum_k p_ik |dF_k| + |dF_0| (dC: the addends' magnitudes as above), not against the small difference.
                    (The rounding of y_0 = (logf + 17) - log10 Flim is left to the NumPy figure: the twin forms y_0 the same way.)
  lf_veff's phi:    2^-53 |phi| (1 + 1 / fc) (the reference's 0.5 (1 + num / sqrt(1 + num^2)) cancels for num << 0), times
                    1 + |ln fc / d| for fcmin > 0 (the exponent of fc^(1/d)).

No source inside the model's domain has a node exponent of -inf: the largest t em is 10^(45.4 - 40) x 1050 (K = 32, sigma =
0.3), and l = ln fc / d stays above -1e302 for any flux a double can hold with y > -300.  The skip of such a node is covered
by a node table with a zero weight (ln w = -inf): tests/test_gradterms_cpu.py for the twin, tests/test_gpu_gradterms.py
for the kernels, both against the table without that node, bit for bit."""
import functools
import math

import numpy as np

import lf_problib as L
from lumfuncmcmc_amd import deconv as D, grad as G, hostsetup as hs, synth

mp = L.mp
mpf, pair, ulp_of, ulps_around, U53, NMAX, measure, numpy_figure, cap_from = \
    L.mpf, L.pair, L.ulp_of, L.ulps_around, L.U53, L.NMAX, L.measure, L.numpy_figure, L.cap_from
MLN10 = mp.log(10)
LN10 = D.LN10
TINY = 5e-324
KAPPA = float(G._kappa(synth.FCMIN))
PIVOT_SETS = ((1.20, 1.53, 1.86), (1.18, 1.36, 1.54))
FLIM0, ALPHA0 = synth.FLIM[0], synth.ALPHA_C
OM0 = synth.OMEGA_0[0] / G.SQARCSEC
SIGMAS = (1e-8, 1e-4, 0.01, 0.09, 0.3)
FREE, FIXCOMP, ZEVOL = 0, 1, 2
VNAME = {FREE: "free", FIXCOMP: "fixcomp", ZEVOL: "zevol"}

# Caps on max err / yard: max(2, 4 x the NumPy binary64 figure), the figures measured on the CPU by
# tests/test_gradterms_cpu.py::test_numpy_figures_behind_the_caps (which asserts that they still hold) on 2026-10-19;
# DESIGN.md section 3.13 has the device's figures next to them.
CAPS = {
    "dgrad_comp_l": 15.8, "dgrad_comp_dF": 23.2, "dgrad_comp_dC": 25.1, "deconv_lcomp": 15.8, "grad_comp_l": 6.44,
    "grad_comp_dF": 8.87, "grad_comp_dC": 15.8, "grad_basis": 8.59, "grad_part_free": 12.7, "deconv_delta_free": 11.7,
    "deconv_grad_free": 7.42, "grad_part_fixcomp": 8.84, "deconv_delta_fixcomp": 9.16, "deconv_grad_fixcomp": 5.68,
    "grad_part_zevol": 13.5, "deconv_delta_zevol": 11.2, "deconv_grad_zevol": 4.73, "veff_phi": 5.83,
}


def pow10(x):
    """10^x as the host layer forms P and U: the C library's pow, element by element"""
    return np.array([math.pow(10.0, float(v)) for v in np.atleast_1d(x)])


def _case(ref_vals, yard, npv, **kw):
    ref = pair(list(ref_vals))
    c = {"ref": ref, "yard": np.maximum(L.f64(yard), TINY), "np": L.f64(npv)}
    c.update(kw)
    return c


# ---------------------------------------------------------------------------------------------- completeness forms
def comp_mp(aC, y, v, kappa):
    """(l, dF, dC, |dF's addends|, |dC's addends|) at 40 digits from 40-digit arguments"""
    num = aC * y
    s = mp.sqrt(1 + num * num)
    w = 1 + num / s if num >= 0 else 1 / (s * (s - num))
    lnfc = mp.log(w / 2)
    gp = 1 / (s ** 3 * w)
    e, d = mp.exp(-v), -mp.expm1(-v)
    l = lnfc / d
    lw = l * v * e / d
    f1, f2 = lw, gp * (aC / MLN10) / d
    c1, c2 = lw * MLN10 * kappa / (aC * aC), gp * y / d
    return l, f1 - f2, c1 + c2, abs(f1) + abs(f2), abs(c1) + abs(c2)


def comp_yards(aC, r):
    """ulp(l), dF's and dC's yardsticks from comp_mp's tuple"""
    yl = float(ulp_of(pair([r[0]]))[0])
    yF = float(ulp_of(pair([r[1]]))[0]) if aC > 0 else U53 * float(r[3])
    return yl, yF, U53 * float(r[4])


def comp_row_mp(flim, aC, kappa, logf, U):
    """grad_comp's (l, dF, dC) from the binary64 row and source values, the magnitudes of dF's and dC's addends, and the three
    yardsticks with the roundings of the y and v the function forms"""
    flim, aC, kappa, logf, U = mpf(flim), mpf(aC), mpf(kappa), mpf(logf), mpf(U)
    lF = mp.log10(flim)
    y = logf + 17 - lF
    arg = MLN10 * kappa / aC
    v = U * mp.exp(arg) / flim
    r = comp_mp(aC, y, v, kappa)
    dy = mp.mpf(U53) * (2 * abs(lF) + abs(logf + 17) + abs(y))
    dv = mp.mpf(U53) * v * (4 + 2 * abs(arg))
    ry, rv = comp_mp(aC, y + dy, v, kappa), comp_mp(aC, y, v + dv, kappa)
    base = comp_yards(float(aC), r)
    yards = tuple(base[j] + float(abs(ry[j] - r[j]) + abs(rv[j] - r[j])) for j in range(3))
    return r, yards


def dc_sign_change(aC, v, kappa=KAPPA):
    """y > 0 where dC = l w ln10 kappa / alpha_C^2 + g' y / d changes its sign (bisection on the twin; NaN if it has none)"""
    f = lambda y: D._lcomp_grad(np.float64(y), np.float64(v), aC, kappa)[2]       # noqa: E731
    lo, hi = 1e-9, 8.0
    if not (f(lo) < 0.0 < f(hi)):
        return np.nan
    for _ in range(70):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if f(mid) < 0.0 else (lo, mid)
    return lo


V_EDGES = np.concatenate([[1e-300, 1e-200, 1e-100, 1e-30, 1e-17, 1e-8, 1e-3, 0.1, 1.0, 5.0, 37.5, 100.0, 700.0],
                          ulps_around(L.LF_UNDERFLOW), [744.0, 745.2, 746.0, 750.0, 1000.0, 1.0e4]])
NUM_DECADES = (-300, -200, -100, -30, -17, -8, -4, -2, -1, 0, 1, 2, 3)
AC_EDGES = (synth.ALPHA_LIMS[0], synth.ALPHA_LIMS[1], -synth.ALPHA_C, synth.ALPHA_C)


@functools.lru_cache(None)
def case_dgrad_comp():
    """dgrad_comp(aC, aC_ln, kc2, y, v) and deconv_lcomp(aC, y, v) on (aC, y, v) directly: num = aC y through 0 (+-0,
    +-2^-1074, +-10^k and their neighbours), alpha_C at both ends of the prior box and negative, v from 1e-300 to where
    e^(-v) is subnormal and 0, y around the sign change of dC, a seeded fill."""
    rng = np.random.default_rng(201)
    tg = np.concatenate([[0.0, -0.0, TINY, -TINY]] + [s * ulps_around(10.0 ** k) for k in NUM_DECADES for s in (1.0, -1.0)])
    aC, y, v = [], [], []
    for a in AC_EDGES:
        for i, t in enumerate(tg):
            yy = t / a if abs(t) > TINY else t * np.sign(a)
            aC += [a, a]
            y += [yy, yy]
            v += [V_EDGES[i % len(V_EDGES)], 10.0 ** rng.uniform(-3, 3)]
    nz = len(aC)
    for a in (1.0, 2.0, 4.56, 7.0):
        for vv in (1e-8, 0.05, 0.5, 2.0, 6.0, 20.0):
            y0 = dc_sign_change(a, vv)
            if np.isfinite(y0):
                for yy in ulps_around(y0):
                    aC.append(a), y.append(yy), v.append(vv)
                    aC.append(a), y.append(-yy), v.append(vv)
    nsc = len(aC) - nz
    m = 1500
    a_f = rng.uniform(1.0, 7.0, m)
    a_f[::10] *= -1.0
    aC, y, v = L.f64(np.concatenate([aC, a_f])), L.f64(np.concatenate([y, rng.uniform(-1.5, 2.0, m)])), \
        L.f64(np.concatenate([v, 10.0 ** rng.uniform(-3, 3, m)]))
    kap = np.full(len(aC), KAPPA)
    rs = [comp_mp(mpf(a), mpf(b), mpf(c), mpf(KAPPA)) for a, b, c in zip(aC, y, v)]
    yd = np.array([comp_yards(a, r) for a, r in zip(aC, rs)])
    with np.errstate(all="ignore"):
        nl, nF, nC = D._lcomp_grad(y, v, aC, KAPPA)
        nl0 = D._lcomp(y, v, aC)
    base = {"aC": aC, "kappa": kap, "y": y, "v": v, "num": aC * y, "n_zero": nz, "n_signchange": nsc}
    out = {k: _case([r[j] for r in rs], yd[:, j], n_, **base) for j, (k, n_) in enumerate((("l", nl), ("dF", nF), ("dC", nC)))}
    out["lcomp"] = _case([r[0] for r in rs], yd[:, 0], nl0, **base)
    assert len(aC) <= NMAX
    return out


@functools.lru_cache(None)
def case_grad_comp():
    """grad_comp(grad_comp_row(row, kappa), logf, U): Flim and alpha_C at both ends of their boxes, a negative alpha_C, y
    from tiny to +-2 on both sides, U = 10^(logf + 17) as the host forms it."""
    rng = np.random.default_rng(202)
    flim = np.concatenate([np.repeat([synth.FLIM_LIMS[0], synth.FLIM_LIMS[1], 2.72], 120), rng.uniform(1.0, 6.0, 1200)])
    n = len(flim)
    aC = rng.uniform(1.0, 7.0, n)
    aC[:360] = np.tile(np.repeat(AC_EDGES, 30), 3)
    yt = np.tile(np.concatenate([[0.0, 1e-12, -1e-12, 1e-6, -1e-6, 1e-3, -1e-3], np.linspace(-1.5, 2.0, 23)]), n // 30 + 1)[:n]
    yt[360:] = rng.uniform(-1.5, 2.0, n - 360)
    logf = (np.log10(flim) + yt) - 17.0
    U = pow10(logf + 17.0)
    rs = [comp_row_mp(a, b, KAPPA, c, d) for a, b, c, d in zip(flim, aC, logf, U)]
    with np.errstate(all="ignore"):
        yn = (logf + 17.0) - np.log10(flim)
        vn = U * (np.exp(LN10 * KAPPA / aC) / flim)
        npv = D._lcomp_grad(yn, vn, aC, KAPPA)
    base = {"flim": L.f64(flim), "aC": L.f64(aC), "kappa": np.full(n, KAPPA), "logf": L.f64(logf), "U": L.f64(U), "y": yn}
    return {k: _case([r[0][j] for r in rs], [r[1][j] for r in rs], npv[j], **base) for j, k in enumerate(("l", "dF", "dC"))}


# ---------------------------------------------------------------------------------------------- basis
def basis_mp(piv, z):
    z1, z2, z3 = (mpf(p) for p in piv)
    z = mpf(z)
    a, b, c = z - z1, z - z2, z - z3
    return [b * c / ((z1 - z2) * (z1 - z3)), a * c / ((z2 - z1) * (z2 - z3)), a * b / ((z3 - z1) * (z3 - z2))]


@functools.lru_cache(None)
def case_basis():
    """grad_basis(grad_piv(gc), z): z at each pivot, +-1 and 2 ulp around it, midway, outside [z1, z3] by 0.5, a seeded fill;
    both pivot sets.  Outputs [n][3], flattened."""
    rng = np.random.default_rng(203)
    piv, z = [], []
    for ps in PIVOT_SETS:
        zs = np.concatenate([ulps_around(np.array(ps)), [(ps[0] + ps[1]) / 2, (ps[1] + ps[2]) / 2, ps[0] - 0.5, ps[2] + 0.5],
                             rng.uniform(ps[0] - 0.5, ps[2] + 0.5, 300)])
        z.append(zs)
        piv.append(np.tile(ps, (len(zs), 1)))
    z, piv = L.f64(np.concatenate(z)), L.f64(np.concatenate(piv))
    refs = [v for p, x in zip(piv, z) for v in basis_mp(p, x)]
    ref = pair(refs)
    npv = np.concatenate([G._basis(z[(piv == np.array(ps)).all(axis=1)], ps).T for ps in PIVOT_SETS]).ravel()
    return _case(refs, ulp_of(ref), npv, piv=piv, z=z, n_edges=15 + 4)


# ---------------------------------------------------------------------------------------------- lf_grad_part items
T_LOG = np.concatenate([np.linspace(-6.0, 2.6, 44), np.log10([600.0, 700.0, 740.0, 745.0, 745.13, 745.2, 746.0, 760.0, 800.0])])


def grad_rows(variant, fsa):
    """theta rows: the fiducial point, two corners of the prior box, one with c1 = alpha + 1 = 0"""
    if variant == ZEVOL:
        r = np.array([[42.3, 42.5, 42.7, -2.2, -2.0, -1.8, -1.49], [40.001, 40.2, 40.1, 4.9, 4.0, 3.0, 0.99],
                      [44.999, 44.5, 44.0, -7.9, -7.0, -7.5, -2.99], [42.0, 43.0, 42.2, -2.5, -2.4, -2.6, -1.0]])
        return L.f64(r[:, :6] if fsa else r)
    r = np.array([[42.5, -2.0, -1.49, 2.72, 4.56], [40.0, 5.0, 1.0, 1.0, 1.0], [45.0, -8.0, -3.0, 6.0, 7.0], [42.0, -2.5, -1.0, 3.3, 2.0]])
    if variant == FIXCOMP:
        r = r[:, :3]
    return L.f64(np.delete(r, 2, axis=1) if fsa else r)


def _row_parts(variant, fsa, th):
    al = synth.SCH_AL if fsa else (th[6] if variant == ZEVOL else th[2])
    if variant == ZEVOL:
        return th[0:3], th[3:6], al, None, None
    k = 2 if fsa else 3
    return th[0], th[1], al, (th[k] if variant == FREE else None), (th[k + 1] if variant == FREE else None)


@functools.lru_cache(None)
def case_grad_part(variant, fsa):
    """One source per block and one live lattice node per block of lf_grad_part<variant>: t = 10^(L - L*) from 1e-6 to 800
    for the first row (10^5.4 for the corner row: exp(-t) is 0, the node is skipped and its slots are exactly 0).
    ref / yard / np: [rows][items][GRAD_SLOTS] flattened, items = the sources then the nodes; slot 7 is never written."""
    rng = np.random.default_rng(204 + variant)
    rows = grad_rows(variant, fsa)
    n = len(T_LOG)
    lum = 42.5 + T_LOG
    z = rng.uniform(1.16, 1.90, n)
    yt = rng.uniform(-1.5, 2.0, n)
    logf = (np.log10(FLIM0) + yt) - 17.0
    P, U = pow10(lum - 42.0), pow10(logf + 17.0)
    W = 10.0 ** rng.uniform(-4, 0, n)
    ns = G_SLOTS
    R = len(rows)
    ref = [[[mp.mpf(0)] * ns for _ in range(2 * n)] for _ in range(R)]
    yard = np.full((R, 2 * n, ns), TINY)
    npv = np.zeros((R, 2 * n, ns))
    u = mp.mpf(U53)
    for b, th in enumerate(rows):
        Ls, ph, al, flim, aC = _row_parts(variant, fsa, th)
        c1 = mpf(al) + 1
        for i in range(n):
            if variant == ZEVOL:
                lb = basis_mp(PIVOT_SETS[0], z[i])
                adds = [l * mpf(v) for l, v in zip(lb, Ls)]
                x = mpf(lum[i]) - sum(adds)
                xmag = abs(mpf(lum[i])) + sum(abs(a) for a in adds)
                t = mp.exp(MLN10 * x)
                At = MLN10 * max([abs(mpf(lum[i]))] + [abs(a) for a in adds])
                phz = sum(l * mpf(v) for l, v in zip(lb, ph))
                Aph = MLN10 * max(abs(l * mpf(v)) for l, v in zip(lb, ph))
                E = MLN10 * (x * c1 + phz) - t
                A = max(abs(c1) * At, Aph, t * (1 + At))
                I = mpf(W[i]) * MLN10 * mp.exp(E)
                fl = abs(mpf(W[i]) * MLN10)
                for m in range(3):
                    ref[b][i][m] = lb[m] * (t - c1)
                    yard[b, i, m] = float(u * abs(lb[m]) * (t + abs(c1)) * (1 + At))
                    ref[b][n + i][m] = lb[m] * I * (t - c1)
                    ref[b][n + i][3 + m] = lb[m] * I
                    tm = abs(lb[m]) * (t * (1 + At) + abs(c1))
                    yard[b, n + i, m] = float(u * I * tm * (1 + A)) + TINY * (1 + float((1 + fl) * tm))
                    yard[b, n + i, 3 + m] = float(u * abs(lb[m]) * I * (1 + A)) + TINY * (1 + float((1 + fl) * abs(lb[m])))
                ref[b][i][6] = x
                yard[b, i, 6] = float(u * xmag)
                ref[b][n + i][6] = I * x
                yard[b, n + i, 6] = float(u * I * xmag * (1 + A)) + TINY * (1 + float((1 + fl) * xmag))
                continue
            x = mpf(lum[i]) - mpf(Ls)
            At = abs(MLN10 * (42 - mpf(Ls)))
            t = mpf(P[i]) * mp.exp(MLN10 * (42 - mpf(Ls)))
            ref[b][i][0], yard[b, i, 0] = t - c1, float(u * (t + abs(c1)) * (1 + At))
            ref[b][i][2], yard[b, i, 2] = x, float(ulp_of(pair([x]))[0])
            l = mp.mpf(0)
            if variant == FREE:
                r, ys = comp_row_mp(flim, aC, KAPPA, logf[i], U[i])
                l = r[0]
                ref[b][i][3], ref[b][i][4] = r[1], r[2]
                yard[b, i, 3], yard[b, i, 4] = ys[1], ys[2]
            E = MLN10 * (x * c1 + mpf(ph)) - t + l
            A = max(abs(MLN10 * x * c1), abs(MLN10 * mpf(ph)), t * (1 + At), abs(l))
            om0 = mpf(OM0) if variant == FREE else mp.mpf(1)
            I = mpf(W[i]) * om0 * MLN10 * mp.exp(E)
            fl = abs(mpf(W[i]) * om0 * MLN10)
            mags = [t * (1 + At) + abs(c1), mp.mpf(1), abs(x)] + ([r[3], r[4]] if variant == FREE else [])
            vals = [t - c1, mp.mpf(1), x] + ([r[1], r[2]] if variant == FREE else [])
            for s, (val, mag) in enumerate(zip(vals, mags)):
                ref[b][n + i][s] = I * val
                yard[b, n + i, s] = float(u * I * mag * (1 + A)) + TINY * (1 + float((1 + fl) * mag))
            if variant == FREE:      # the roundings of the y and v that grad_comp forms, on dF and dC
                yard[b, n + i, 3] += float(I) * ys[1]
                yard[b, n + i, 4] += float(I) * ys[2]
    flat = [v for rb in ref for it in rb for v in it]
    c = _case(flat, yard.ravel(), npv.ravel(), rows=rows, lum=L.f64(lum), z=L.f64(z), logf=L.f64(logf), P=P, U=U, W=L.f64(W),
              variant=variant, fsa=fsa, n=n, shape=(R, 2 * n, ns))
    c["np"] = grad_part_numpy(c)
    return c


G_SLOTS = 8


def grad_part_numpy(c):
    """The same contributions in plain NumPy binary64, from the twins' statements (grad._row's and grad._completeness's,
    deconv._lcomp_grad for the completeness at the (y, v) the kernel forms)"""
    variant, fsa, n = c["variant"], c["fsa"], c["n"]
    lum, z, logf, P, U, W = c["lum"], c["z"], c["logf"], c["P"], c["U"], c["W"]
    out = np.zeros(c["shape"])
    with np.errstate(all="ignore"):
        for b, th in enumerate(c["rows"]):
            Ls, ph, al, flim, aC = _row_parts(variant, fsa, th)
            c1 = al + 1.0
            if variant == ZEVOL:
                ls = G._basis(z, PIVOT_SETS[0])
                x = lum - ls.T @ Ls
                t = 10.0 ** x
                I = W * LN10 * np.exp(LN10 * (ls.T @ ph + x * c1) - t)
                ok = np.abs(I) > 0.0
                for m in range(3):
                    out[b, :n, m] = ls[m] * (t - c1)
                    out[b, n:, m] = np.where(ok, I * ls[m] * (t - c1), 0.0)
                    out[b, n:, 3 + m] = np.where(ok, I * ls[m], 0.0)
                out[b, :n, 6] = x
                out[b, n:, 6] = np.where(ok, I * x, 0.0)
                continue
            x = lum - Ls
            t = P * np.exp(LN10 * (42.0 - Ls))
            tlf = LN10 * np.exp(LN10 * (ph + x * c1) - t)
            out[b, :n, 0], out[b, :n, 2] = t - c1, x
            I = W * tlf
            vals = [t - c1, np.ones(n), x]
            if variant == FREE:
                y = (logf + 17.0) - np.log10(flim)
                v = U * (np.exp(LN10 * KAPPA / aC) / flim)
                l, dF, dC = D._lcomp_grad(y, v, aC, KAPPA)
                out[b, :n, 3], out[b, :n, 4] = dF, dC
                I = W * OM0 * tlf * np.exp(l)
                vals += [dF, dC]
            ok = np.abs(I) > 0.0
            for s, val in enumerate(vals):
                out[b, n:, s] = np.where(ok, I * val, 0.0)
    return out.ravel()


# ---------------------------------------------------------------------------------------------- deconvolution items
def deconv_rows(variant):
    return grad_rows(variant, False)


@functools.lru_cache(None)
def deconv_sources(variant):
    """200 sources: every sigma at 20 fluxes from 1.5 dex below Flim (exponent spreads of hundreds, maxima ascending with k)
    to 2 dex above (flat); bright-end sources (t large for the fiducial row: maxima descending with k); the prior's far
    corner (lum = 45.4 against L* = 40 of the corner row); every tenth source sigma = 0."""
    rng = np.random.default_rng(210 + variant)
    yt = np.concatenate([np.repeat(np.linspace(-1.5, 2.0, 20), len(SIGMAS)), rng.uniform(0.0, 2.0, 99), [2.0]])
    n = len(yt)
    sg = np.concatenate([np.tile(SIGMAS, 20), rng.choice(SIGMAS, 99), [0.3]])
    lum = np.concatenate([42.5 + rng.uniform(-1.0, 0.8, 100), 42.5 + rng.uniform(0.8, 2.5, 99), [45.4]])
    sg[5::10] = 0.0
    sg[n - 1] = 0.3
    logf = (np.log10(FLIM0) + yt) - 17.0
    z = rng.uniform(1.16, 1.90, n)
    return {"lum": L.f64(lum), "z": L.f64(z), "logf": L.f64(logf), "P": pow10(lum - 42.0), "U": pow10(logf + 17.0), "sigma": L.f64(sg), "n": n}


def deconv_inp(variant, s, fsa=False):
    """the twins' input dict for these sources (one field)"""
    return {"variant": VNAME[variant], "fix_sch_al": fsa, "sch_al0": synth.SCH_AL, "field_ind": np.array([0, s["n"]]), "lum": s["lum"],
            "z": s["z"], "logf": s["logf"], "fcmin": synth.FCMIN, "pivots": PIVOT_SETS[0], "Flim0": [FLIM0], "alpha0": ALPHA0}


D_SLOTS = 4


def deconv_slots_from_twin(variant, th, g):
    """the kernel's slots (without their final scales) from the twin's per-source gradient [N][ndim]"""
    n = len(g)
    out = np.zeros((n, D_SLOTS))
    if variant == ZEVOL:
        out[:, 0:3], out[:, 3] = g[:, 0:3] / LN10, g[:, 6] / LN10
    else:
        out[:, 0], out[:, 1] = g[:, 0] / LN10, g[:, 2] / LN10
        if variant == FREE:
            out[:, 2], out[:, 3] = g[:, 3] * th[3], g[:, 4]
    return out


def deconv_item_mp(variant, th, s, i, x, lnw, full=False):
    """(Delta_i, its yardstick, slots[4], yards[4], p_k, a_k) of source i under row th at 40 digits; full=True: one more, a
    dict of what tests/lf_convproblib.py judges the other copies of the node loop by - "A" (the yardsticks' largest exponent
    addend), "adds" (each node's own largest), "dl" (delta_k), "l" (l at the node's true flux), "l0" (at the catalogued flux)"""
    Ls, _, al, flim, aC = _row_parts(variant, False, th)
    if variant != FREE:
        flim, aC = FLIM0, ALPHA0
    flim, aC, kap = mpf(flim), mpf(aC), mpf(KAPPA)
    c1l = MLN10 * (mpf(al) + 1)
    lb = None
    if variant == ZEVOL:
        lb = basis_mp(PIVOT_SETS[0], s["z"][i])
        adds_L = [l * mpf(v) for l, v in zip(lb, Ls)]
        t = mp.exp(MLN10 * (mpf(s["lum"][i]) - sum(adds_L)))
        At = MLN10 * max([abs(mpf(s["lum"][i]))] + [abs(v) for v in adds_L])
    else:
        t = mpf(s["P"][i]) * mp.exp(MLN10 * (42 - mpf(Ls)))
        At = abs(MLN10 * (42 - mpf(Ls)))
    tc = t * (1 + At)                 # t with the condition of its own exponent
    y0 = mpf(s["logf"][i]) + 17 - mp.log10(flim)
    v0 = mpf(s["U"][i]) * mp.exp(MLN10 * kap / aC) / flim
    r0 = comp_mp(aC, y0, v0, kap)
    s2 = mp.sqrt(2) * mpf(s["sigma"][i])
    a, q, qa, adds, lk = [], [], [], [], []
    for k in range(len(x)):
        dl = s2 * mpf(x[k])
        em = mp.expm1(MLN10 * dl)
        rk = comp_mp(aC, y0 + dl, v0 * (1 + em), kap)
        lk.append(rk[0])
        a.append(mpf(lnw[k]) + c1l * dl - t * em + rk[0] - r0[0])
        adds.append(max(abs(c1l * dl), abs(tc * em), abs(rk[0]), abs(r0[0]), abs(mpf(lnw[k]))))
        q.append((dl, em, rk[1], rk[2]))
        qa.append((abs(dl), abs(em), rk[3], rk[4]))
    M = max(a)
    w = [mp.exp(v - M) for v in a]
    S = sum(w)
    p = [v / S for v in w]
    Dl = M + mp.log(S)
    A = max(ad for ad, pk in zip(adds, p) if pk >= mp.mpf(U53))
    u = mp.mpf(U53)
    ex = [sum(pk * qk[j] for pk, qk in zip(p, q)) for j in range(4)]
    ea = [sum(pk * qk[j] for pk, qk in zip(p, qa)) for j in range(4)]
    if variant == ZEVOL:
        slots = [lb[m] * t * ex[1] for m in range(3)] + [ex[0]]
        mags = [abs(lb[m]) * tc * ea[1] for m in range(3)] + [ea[0]]
    else:
        slots, mags = [t * ex[1], ex[0]], [tc * ea[1], ea[0]]
        if variant == FREE:
            slots += [ex[2] - r0[1], ex[3] - r0[2]]
            mags += [ea[2] + r0[3], ea[3] + r0[4]]
        else:
            slots += [mp.mpf(0)] * 2
            mags += [mp.mpf(0)] * 2
    out = (Dl, float(u * (abs(Dl) + 1 + A)), slots, [float(u * m * (1 + A)) for m in mags], p, a)
    return out + ({"A": A, "dl": [qk[0] for qk in q], "l": lk, "l0": r0[0], "adds": adds},) if full else out


@functools.lru_cache(None)
def case_deconv(variant, K):
    """The per-source values of lf_deconv_part<variant> (Delta_i) and lf_deconv_grad_part<variant> (its slots) for
    deconv_sources(variant) under the four rows of deconv_rows(variant), K Gauss-Hermite nodes (deconv.gauss_hermite's
    table, which both the reference and the kernels get).  "delta": [rows][n]; "grad": [rows][n][4]; a sigma = 0 source is
    exactly 0 in every slot.  Under row 0: `rises`, the number of nodes that raise the running maximum (each rescales s and all
    numerators); `max_first`, the maximum is the first node (no node rescales); `spread`, max - min of the exponents."""
    s = deconv_sources(variant)
    rows = deconv_rows(variant)
    x, lnw = D.gauss_hermite(K)
    n, R = s["n"], len(rows)
    dref, dyard = [], np.full((R, n), TINY)
    gref, gyard = [], np.full((R, n, D_SLOTS), TINY)
    rises, first = np.zeros(n, dtype=int), np.zeros(n, dtype=bool)
    spread = np.zeros(n)
    for b, th in enumerate(rows):
        for i in range(n):
            if s["sigma"][i] == 0.0:
                dref.append(mp.mpf(0))
                gref += [mp.mpf(0)] * D_SLOTS
                continue
            Dl, yd, slots, ys, p, a = deconv_item_mp(variant, th, s, i, x, lnw)
            dref.append(Dl)
            dyard[b, i] = yd
            gref += slots
            gyard[b, i] = np.maximum(ys, TINY)
            if b == 0:
                af = np.array([float(v) for v in a])
                rises[i] = 1 + int(np.sum(af[1:] > np.maximum.accumulate(af)[:-1]))
                first[i], spread[i] = int(np.argmax(af)) == 0, float(max(a) - min(a))
    inp = deconv_inp(variant, s)
    npd, npg = np.zeros((R, n)), np.zeros((R, n, D_SLOTS))
    with np.errstate(all="ignore"):
        for b, th in enumerate(rows):
            npd[b] = D._row_terms(inp, s["sigma"], th, x, lnw)
            npg[b] = deconv_slots_from_twin(variant, th, D._row_grad_terms(inp, s["sigma"], th, x, lnw)[1])
    base = {"rows": rows, "src": s, "nodes": L.f64(np.concatenate([x, lnw])), "K": K, "variant": variant, "rises": rises,
            "max_first": first, "spread": spread}
    return {"delta": _case(dref, dyard.ravel(), npd.ravel(), **base), "grad": _case(gref, gyard.ravel(), npg.ravel(), **base)}


def softmax_numpy(variant, th, s, x, lnw, mutate=None):
    """deconv._row_grad_terms's online softmax restated for ONE use: tests/test_gradterms_cpu.py asserts that it gives the
    twin's bits with mutate = None, then applies one mutation and asserts that the metric sees it.  Returns (Delta_i [n],
    slots [n][4]).  mutate: "no_rescale" (a numerator not rescaled when the maximum rises), "em_pow" (em replaced by
    10^delta), "gp_branch" (g' from the other branch), "w_no_e" (w without its e^(-v))."""
    Ls, _, al, flim, aC = _row_parts(variant, False, th)
    if variant != FREE:
        flim, aC = FLIM0, ALPHA0
    lum, sigma = s["lum"], s["sigma"]
    n = len(lum)
    c1l = LN10 * (al + 1.0)
    ls = None
    with np.errstate(all="ignore"):
        if variant == ZEVOL:
            ls = G._basis(s["z"], PIVOT_SETS[0])
            t = np.exp(LN10 * (lum - ls.T @ np.asarray(Ls, dtype=float)))
        else:
            t = 10.0 ** (lum - 42.0) * np.exp(LN10 * (42.0 - Ls))
        U = 10.0 ** (s["logf"] + 17.0)
        Fl = np.full(n, float(flim))
        y0 = (s["logf"] + 17.0) - np.log10(Fl)
        v0 = U * (np.exp(LN10 * KAPPA / aC) / Fl)
        l0, dF0, dC0 = lcomp_grad_numpy(y0, v0, aC, KAPPA, mutate)
        s2 = np.sqrt(2.0) * sigma
        m, acc = np.full(n, -np.inf), np.zeros(n)
        num = np.zeros((4, n))
        for k in range(len(x)):
            dl = s2 * x[k]
            em = np.expm1(LN10 * dl)
            if mutate == "em_pow":
                em = 10.0 ** dl
            lk, dFk, dCk = lcomp_grad_numpy(y0 + dl, v0 * (em + 1.0), aC, KAPPA, mutate)
            a = lnw[k] + ((c1l * dl - t * em) + (lk - l0))
            skip = a == -np.inf
            d = a - m
            e = np.exp(-np.abs(d))
            up = d > 0.0
            acc_n = np.where(up, acc * e + 1.0, acc + e)
            for j, qj in enumerate((dl, em, dFk, dCk)):
                risen = num[j] + qj if (mutate == "no_rescale" and j == 1) else num[j] * e + qj
                num[j] = np.where(skip, num[j], np.where(up, risen, num[j] + e * qj))
            acc = np.where(skip, acc, acc_n)
            m = np.where(skip, m, np.where(up, a, m))
        on = sigma > 0.0
        Dl = np.where(on, m + np.log(acc), 0.0)
        ex = [np.where(on, num[j] / acc, 0.0) for j in range(4)]
        g = np.zeros((n, G.ndim_of(deconv_inp(variant, s))))
        gL = t * ex[1]
        if variant == ZEVOL:
            for mm in range(3):
                g[:, mm] = LN10 * (ls[mm] * gL)
            g[:, 6] = LN10 * ex[0]
        else:
            g[:, 0], g[:, 2] = LN10 * gL, LN10 * ex[0]
            if variant == FREE:
                g[:, 3] = (1.0 / flim) * np.where(on, ex[2] - dF0, 0.0)
                g[:, 4] = np.where(on, ex[3] - dC0, 0.0)
    return Dl, g


def lcomp_grad_numpy(y, v, aC, kappa, mutate=None):
    """deconv._lcomp_grad restated for the mutations "gp_branch" and "w_no_e" (see softmax_numpy)"""
    num = aC * y
    den = np.sqrt(num * num + 1.0)
    e = np.exp(-v)
    d = -np.expm1(-v)
    neg = num < 0.0
    s = np.where(neg, den - num, den + num)
    lnfc = np.where(neg, -np.log(2.0 * den * s), np.log1p(-0.5 / (den * s)))
    if mutate == "gp_branch":
        gp = np.where(neg, 1.0 / (den * den * (den + num)), (den - num) / (den * den))
    else:
        gp = np.where(neg, s / (den * den), 1.0 / (den * den * s))
    l = lnfc / d
    w = v / d if mutate == "w_no_e" else v * e / d
    lw = np.where(e > 0.0, l * w, 0.0)
    dF = lw - gp * (aC / LN10) / d
    dC = lw * (LN10 * kappa / (aC * aC)) + gp * y / d
    return l, dF, dC


# ---------------------------------------------------------------------------------------------- lf_veff
VEFF_ALPHAS = (0.6, 4.56, 10.0)
VEFF_PREF0 = sum(synth.OMEGA_0) / hs.SQARCSEC


@functools.lru_cache(None)
def case_veff(alpha, fcmin, per_source_vol):
    """veff_weights: phi_i = 1 / (pref0 fleming(f, Flim, alpha, fcmin) vol_i), 0 where vol_i <= 0.  About 170 sources per
    configuration (2000 over the twelve), f / Flim from 1e-3 to 1e3; with fcmin > 0 the fluxes whose fc^(1/d) would underflow
    (ln fc / d < -600) are drawn again from [0.1, 1e3] Flim: a subnormal power has no relative accuracy to speak of."""
    rng = np.random.default_rng(220 + int(10 * alpha) + (1 if fcmin else 0) + (2 if per_source_vol else 0))
    n = 170
    flim = rng.uniform(1.0e-17, 6.0e-17, n)
    ratio = 10.0 ** np.concatenate([[-3.0, 3.0, 0.0], rng.uniform(-3.0, 3.0, n - 3)])
    a, fr = mpf(alpha), mp.mpf(0)
    if fcmin:
        aa = (2 * mpf(fcmin) - 1) ** 2
        fr = abs(aa / (1 - aa))

    def one(f, fl):
        num = a * mp.log10(mpf(f) / mpf(fl))
        fc = (1 + num / mp.sqrt(1 + num * num)) / 2
        ex = mp.mpf(1)
        if fcmin:
            ftau = mpf(fl) * mp.mpf(10) ** (-mp.sqrt(fr / (a * a)))
            ex = 1 / (1 - mp.exp(-mpf(f) / ftau))
        return fc, ex
    flux = ratio * flim
    if fcmin:
        for i in range(n):
            while True:
                fc, ex = one(flux[i], flim[i])
                if mp.log(fc) * ex > -600:
                    break
                flux[i] = 10.0 ** rng.uniform(-1.0, 3.0) * flim[i]
    vol = rng.uniform(1.0e5, 5.0e6, n)
    vol[7], vol[23] = 0.0, -1.0
    vol_all = 1.0e6
    refs, yard = [], np.zeros(n)
    with mp.workdps(80):          # (1 + num / sqrt(1 + num^2) loses 2 log10 |num| digits for num << 0)
        for i in range(n):
            v = mpf(vol[i]) if per_source_vol else mpf(vol_all)
            if v <= 0:
                refs.append(mp.mpf(0))
                yard[i] = TINY
                continue
            fc, ex = one(flux[i], flim[i])
            phi = 1 / (mpf(VEFF_PREF0) * fc ** ex * v)
            refs.append(+phi)
            yard[i] = float(mp.mpf(U53) * phi * (1 + 1 / fc) * ((1 + abs(mp.log(fc) * ex)) if fcmin else 1))
    with np.errstate(all="ignore"):
        comp = hs.fleming(flux, flim, alpha, fcmin)
        v = vol if per_source_vol else np.full(n, vol_all)
        npv = np.where(v > 0, 1.0 / (VEFF_PREF0 * comp * np.where(v > 0, v, 1.0)), 0.0)
    return _case(refs, yard, npv, flux=L.f64(flux), flim=L.f64(flim), vol=L.f64(vol) if per_source_vol else vol_all, alpha=alpha,
                 fcmin=fcmin, zero=(vol <= 0) if per_source_vol else np.zeros(n, dtype=bool))


def veff_cases():
    return [(al, fm, ps) for al in VEFF_ALPHAS for fm in (synth.FCMIN, 0.0) for ps in (True, False)]
