"""The NumPy twin of the device gradient (lumfuncmcmc_amd/grad.py) against 40-digit differentiation, without a GPU.

lnprob is restated term by term in mpmath (one term per source and per lattice point, as the oracle defines them:
piece_a, piece_b, fleming with the decay, schechter_z through get_quad_coef), the restatement is checked against
lf_oracle.lnprob to the project's 1e-12 - it is the same function - and every term is differentiated with mp.diff.  Then

    |twin - mp| <= 1e-12 S_abs   element-wise,   S_abs = the sum of |d term / d theta_e| over the terms, made in mpmath:

the project's parity tolerance for lnprob, made aware of the conditioning of each element.  Cancelling forms of 1 - fc or
1 - exp(-u) in the twin fail this.  Then the conventions (NaN rows, batch independence) and the C ABI's new entries."""
import os
import re

import mpmath as mp
import numpy as np
import pytest

from lf_testlib import O, make_inputs, synth
from lumfuncmcmc_amd import grad as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
mp.mp.dps = 40
TOL = 1e-12


def mp_terms(inp):
    """[(term, deps)]: lnprob(theta) = sum of term(theta) with theta a list of mpf; deps = the theta indices a term reads."""
    F = mp.mpf
    v, fsa = inp["variant"], bool(inp["fix_sch_al"])
    fi = [int(i) for i in inp["field_ind"]]
    nf = len(fi) - 1
    ln10 = mp.log(10)
    sq = (F(180) / mp.pi * 3600) ** 2
    logL, zarr = inp["logL"], inp["zarr"]
    S = logL.shape[0]
    a = (2 * F(float(inp["fcmin"])) - 1) ** 2
    ratio = abs(a / (1 - a))

    def alpha_of(th, i):
        return F(float(inp["sch_al0"])) if fsa else th[i]

    def tlf(L, al, Ls, ph):
        return ln10 * mp.power(10, ph) * mp.power(10, (L - Ls) * (al + 1)) * mp.exp(-mp.power(10, L - Ls))

    def comp(f, Flim, aC):
        Fl = Flim * F(10) ** -17
        num = aC * mp.log10(f / Fl)
        fc = (1 + num / mp.sqrt(1 + num ** 2)) / 2
        f_tau = Fl * mp.power(10, -mp.sqrt(ratio * aC ** -2))
        return mp.power(fc, 1 / (1 - mp.exp(-f / f_tau)))

    def flux(L, DL):
        return mp.power(10, L) / (4 * mp.pi * (F(3.086e24) * DL) ** 2)

    W = [[None] * S for _ in range(S)]
    for j in range(S):
        for k in range(S):
            wl = ((F(float(logL[j, k])) - F(float(logL[j - 1, k]))) if j > 0 else 0) + \
                 ((F(float(logL[j + 1, k])) - F(float(logL[j, k]))) if j < S - 1 else 0)
            wz = ((F(float(zarr[k])) - F(float(zarr[k - 1]))) if k > 0 else 0) + ((F(float(zarr[k + 1])) - F(float(zarr[k]))) if k < S - 1 else 0)
            W[j][k] = wl * wz / 4
    terms = []
    if v in ("free", "fixcomp"):
        k0 = 2 if fsa else 3
        sch = [0, 1] + ([] if fsa else [2])
        for f in range(nf):
            for i in range(fi[f], fi[f + 1]):
                L = F(float(inp["lum"][i]))
                if v == "free":
                    fl, om0 = flux(L, F(float(inp["DLz"][i]))), F(int(inp["Omega_0"][f])) / sq
                    terms.append((lambda th, L=L, fl=fl, om0=om0, f=f: mp.log(tlf(L, alpha_of(th, 2), th[0], th[1]) * om0
                                                                              * comp(fl, th[k0 + f], th[k0 + nf])),
                                  sch + [k0 + f, k0 + nf]))
                else:
                    om = F(float(inp["Om_arr"][i]))
                    terms.append((lambda th, L=L, om=om: mp.log(tlf(L, alpha_of(th, 2), th[0], th[1]) * om), sch))
        for j in range(S):
            for k in range(S):
                L = F(float(logL[j, k]))
                if v == "free":
                    fl = flux(L, F(float(inp["DL_zarr"][k])))
                    for f in range(nf):
                        c = W[j][k] * F(float(inp["volume_part"][k])) * F(float(inp["Omega_0"][f])) / sq
                        terms.append((lambda th, L=L, fl=fl, c=c, f=f: -c * tlf(L, alpha_of(th, 2), th[0], th[1])
                                      * comp(fl, th[k0 + f], th[k0 + nf]), sch + [k0 + f, k0 + nf]))
                else:
                    c = W[j][k] * sum(F(float(inp["integ_part"][f][j, k])) for f in range(nf))
                    terms.append((lambda th, L=L, c=c: -c * tlf(L, alpha_of(th, 2), th[0], th[1]), sch))
    else:
        z1, z2, z3 = (F(float(p)) for p in inp["pivots"])
        deps = list(range(6)) + ([] if fsa else [6])

        def quad(y1, y2, y3, z):
            qa = ((y3 - y1) + (y2 - y1) * (z1 - z3) / (z2 - z1)) / (z3 ** 2 - z1 ** 2 + (z2 ** 2 - z1 ** 2) * (z1 - z3) / (z2 - z1))
            qb = (y2 - y1 - qa * (z2 ** 2 - z1 ** 2)) / (z2 - z1)
            return qa * z ** 2 + qb * z + (y1 - qa * z1 ** 2 - qb * z1)

        def tlfz(L, z, th):
            return tlf(L, alpha_of(th, 6), quad(th[0], th[1], th[2], z), quad(th[3], th[4], th[5], z))

        for i in range(fi[-1]):
            L, z, om = F(float(inp["lum"][i])), F(float(inp["z"][i])), F(float(inp["Om_arr"][i]))
            terms.append((lambda th, L=L, z=z, om=om: mp.log(tlfz(L, z, th) * om), deps))
        for j in range(S):
            for k in range(S):
                L, z = F(float(logL[j, k])), F(float(zarr[k]))
                c = W[j][k] * sum(F(float(inp["integ_part"][f][j, k])) for f in range(nf))
                terms.append((lambda th, L=L, z=z, c=c: -c * tlfz(L, z, th), deps))
    return terms


def mp_lnprob_grad(inp, theta):
    """(lnprob, grad[ndim], S_abs[ndim]) of one row at 40 digits"""
    th = [mp.mpf(float(t)) for t in theta]
    nd = len(th)
    g, s = [mp.mpf(0)] * nd, [mp.mpf(0)] * nd
    lp = mp.mpf(0)
    for term, deps in mp_terms(inp):
        lp += term(th)
        for e in deps:
            d = mp.diff(lambda x: term(th[:e] + [x] + th[e + 1:]), th[e])
            g[e] += d
            s[e] += abs(d)
    return lp, g, s


def theta_rows(inp):
    """6 rows: interior ones, one with every FREE source faint (Flim at its upper bound: num < 0 for most sources) and one
    bright (Flim and alpha_C at their lower bounds: the decay factor of most sources is exactly 1)"""
    v, fsa = inp["variant"], bool(inp["fix_sch_al"])
    nf = len(inp["field_ind"]) - 1
    th = synth.walkers(v, 6, seed=41, fix_sch_al=fsa, nf=nf)
    th[:, 0] = np.linspace(41.8, 43.2, 6)          # (keep the rows where the catalogue's Schechter factor does not underflow)
    if v == "zevol":
        th[:, 1] = th[:, 0] + 0.2
        th[:, 2] = th[:, 0] - 0.3
    if v == "free":
        k = 2 if fsa else 3
        th[4, k:k + nf] = inp["lims"]["Flim"][1]
        th[5, k:k + nf] = inp["lims"]["Flim"][0]
        th[5, k + nf] = inp["lims"]["alpha"][0]
    return th


CASES = [(v, fsa, n, nf) for v in ("free", "fixcomp", "zevol") for fsa in (False, True) for n in (1, 50) for nf in (1, 2)]


@pytest.mark.parametrize("variant,fsa,n,nf", CASES)
def test_twin_against_40_digit_differentiation(variant, fsa, n, nf):
    inp = make_inputs(variant, n, S=11, nf=nf, fix_sch_al=fsa)
    th = theta_rows(inp)
    lp_t, g_t, s_t = G.lnprob_grad(inp, th, terms=True)
    ref = O.lnprob_batch(inp, th)
    assert np.all(np.isfinite(ref)), ref
    worst = 0.0
    for i, row in enumerate(th):
        lp, g, s = mp_lnprob_grad(inp, row)
        assert abs(float(lp) - ref[i]) <= TOL * abs(ref[i]), ("the restatement is not the oracle's function", i, float(lp), ref[i])
        assert abs(lp_t[i] - ref[i]) <= TOL * abs(ref[i])
        for e in range(len(row)):
            err = abs(mp.mpf(float(g_t[i, e])) - g[e])
            if s[e] > 0:        # (an element nothing contributes to - a field without sources on a lattice of zero width: exactly 0)
                worst = max(worst, float(err / s[e]))
            assert err <= TOL * s[e], (i, e, float(g_t[i, e]), float(g[e]), float(s[e]), float(err))
            assert abs(s_t[i, e] - float(s[e])) <= 1e-9 * float(s[e]), ("S_abs", i, e, s_t[i, e], float(s[e]))
    print("twin vs mp %s fsa=%d n=%d nf=%d: max |twin - mp| / S_abs = %.2e" % (variant, fsa, n, nf, worst))


@pytest.mark.parametrize("variant", ["free", "fixcomp", "zevol"])
def test_conventions(variant):
    """rows outside the prior box and rows whose oracle lnprob is -inf: NaN in every element; every other row finite; a row
    alone and inside a permuted batch of 37: the same bits"""
    inp = make_inputs(variant, 50, S=11, nf=2)
    th = synth.walkers(variant, 37, seed=8, nf=2)
    th[3, 0] = 39.5
    th[11, 1] = 5.5
    th[20, 0:(3 if variant == "zevol" else 1)] = 40.001          # exp(-10^(lum - L*)) underflows
    ref = O.lnprob_batch(inp, th)
    assert np.isinf(ref[[3, 11, 20]]).all() and np.isfinite(ref).sum() >= 30
    lp, g = G.lnprob_grad(inp, th)
    fin = np.isfinite(ref)
    assert np.array_equal(np.isfinite(lp), fin)
    assert np.isnan(g[~fin]).all() and np.isfinite(g[fin]).all()
    perm = np.random.default_rng(2).permutation(37)
    lp_p, g_p = G.lnprob_grad(inp, th[perm])
    assert np.array_equal(g_p, g[perm], equal_nan=True) and np.array_equal(lp_p, lp[perm])
    for i in (0, 3, 36):
        lp1, g1 = G.lnprob_grad(inp, th[i])
        assert np.array_equal(g1, g[i], equal_nan=True) and (lp1 == lp[i])


def test_zero_integrand_points_add_zero_not_nan():
    """lattice points whose completeness underflows to exactly 0 (far below the flux limit) contribute exactly 0"""
    inp = make_inputs("free", 50, S=11, nf=2)
    inp["logL"] = inp["logL"].copy()
    inp["logL"][0, :] = 36.0                       # five decades below the flux limit: fc^(1/d) = 0 in binary64
    th = theta_rows(inp)[:3]
    lp, g = G.lnprob_grad(inp, th)
    assert np.all(np.isfinite(lp)) and np.all(np.isfinite(g))


def test_c_abi_entries():
    import ctypes
    from lumfuncmcmc_amd import capi
    hdr = open(os.path.join(ROOT, "include", "lfmcmc.h")).read()
    assert re.search(r"int lf_lnprob_grad_batch\(lf_ctx \*ctx, const double \*theta, int B, double \*lnprob, double \*grad\);", hdr)
    assert re.search(r"int lf_lnprob_grad_batch_device\(lf_ctx \*ctx, const double \*d_theta, int B, double \*d_lnprob, "
                     r"double \*d_grad,\s+void \*hip_stream\);", hdr)
    assert "#define LF_ABI_VERSION 3" in hdr
    lib = capi.load()
    assert lib.lf_abi_version() == 3
    dp = ctypes.POINTER(ctypes.c_double)
    assert lib.lf_lnprob_grad_batch.argtypes == [ctypes.c_void_p, dp, ctypes.c_int, dp, dp]
    assert lib.lf_lnprob_grad_batch_device.argtypes == [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 3
    assert lib.lf_lnprob_grad_batch.restype == ctypes.c_int and lib.lf_lnprob_grad_batch_device.restype == ctypes.c_int
    assert hasattr(capi.LFContext, "lnprob_grad")
    # refused before any device is touched
    assert lib.lf_lnprob_grad_batch(None, None, 1, None, None) == capi.LF_ERR_ARG
