"""The gradient of Delta B, the cut's change of the expected counts, on the host (lumfuncmcmc_amd/deconv.py: cut_term_grad and
lnprob_err_grad(cut=...), the NumPy twin of csrc/lf_deconv_cut_grad.h): the formulas against 30-digit
differentiation of the same node sum and against central differences of deconv.cut_term, exact zeros and structure, the
combined twin and the model classes' keyword.  No GPU.

Formula check.  The twin is the exact derivative of the node sum, so the reference differentiates that sum (mp.diff of sum_n
w_n phi Omega over cut_nodes' tables), not the integral.  FREE, FIXCOMP and ZEVOL with the slope free and fixed, theta at the
box's centre and at the alpha_C = 7 corners with alpha = -3 and +1 (section 3.31's), error models of 0.09 and 0.30 dex.  The
bound is the one tests/test_deconv_grad_cpu.py applies to the Delta gradient's formula test, 3.6e-15 relative to S_abs, the sum
of the absolute values of an element's terms.  Measured worst |twin - mpmath| / S_abs: 5.7e-16 (FREE, alpha = +1 corner, 0.09
dex; FIXCOMP 4.4e-16, ZEVOL 3.7e-16); every case lies between 4.6e-17 and 5.7e-16.  The z-evolving twin takes L*(z) = sum_m
l_m(z) L_m in extended precision: in double, as the kernel and cut_term have it, that sum's rounding at |L_m| of 43 alone is
2.2e-14 of S_abs (measured) - the conditioning of x, not an error of the formulas."""
import numpy as np
import pytest

import lf_cutlib as C
from lf_testlib import synth
from lumfuncmcmc_amd import deconv as D
from lumfuncmcmc_amd import grad as G
from test_deconv_grad_cpu import FORMULA_BOUND

PROBES = {"centre": (-1.0, 4.0), "aC7_al-3": (-3.0, 7.0), "aC7_al+1": (1.0, 7.0)}        # name -> (alpha, alpha_C)


def probe(variant, fsa, name, nf=1):
    """(inputs, theta) of one probe: the slope and alpha_C where the variant holds them fixed go into the inputs"""
    al, aC = PROBES[name]
    inp = C.cut_inputs(variant, n=60, S=3, nf=nf, fix_sch_al=fsa)
    if variant == "zevol":
        th = [synth.LSTAR, synth.LSTAR + 0.1, synth.LSTAR - 0.1, synth.PHISTAR, synth.PHISTAR - 0.2, synth.PHISTAR + 0.1]
    else:
        th = [synth.LSTAR, synth.PHISTAR]
    if fsa:
        inp["sch_al0"] = al
    else:
        th = th + [al]
    if variant == "free":
        th = th + [3.5] * nf + [aC]
    else:
        inp["alpha0"] = aC
    return inp, np.array(th)


def same_value(variant, tot, ref, sabs):
    """cut_term_grad's Delta B is cut_term's: FREE and FIXCOMP bit for bit.  The z-evolving twin takes L*(z) = sum_m l_m(z) L_m
    in extended precision where cut_term (the kernel's statements) has it in double: 43 eps sum_m |l_m| in x, times ln10 (10^x
    + |alpha + 1|) in a term - below 1e-13 of the scale for sum_m |l_m| up to 10 and 10^x up to 1."""
    if variant != "zevol":
        return np.array_equal(tot, ref)
    return bool(np.all(np.abs(np.asarray(tot) - ref) <= 1e-13 * np.asarray(sabs)))


def mp_grad(inp, th, nl, digits=30):
    """d sum_f sum_n w_n phi Omega / d theta_e for every element e by mp.diff of the node sum itself, 30 digits"""
    import mpmath as mp
    mp.mp.dps = digits
    v, fsa = inp["variant"], bool(inp["fix_sch_al"])
    nf = len(nl)
    a = (2 * mp.mpf(float(inp["fcmin"])) - 1) ** 2
    kappa = mp.sqrt(abs(a / (1 - a)))
    ln10 = mp.log(10)
    piv = [mp.mpf(float(x)) for x in inp["pivots"]]
    zarr = [mp.mpf(float(x)) for x in inp["zarr"]]
    nodes = []
    for f, n in enumerate(nl):
        om0 = mp.mpf(float(inp["Omega_0"][f])) / mp.mpf(G.SQARCSEC)
        for L, col, w, lf in zip(n["L"], n["col"], n["w"], n["logf"]):
            z = zarr[int(col)]
            l = [(z - piv[1]) * (z - piv[2]) / ((piv[0] - piv[1]) * (piv[0] - piv[2])),
                 (z - piv[0]) * (z - piv[2]) / ((piv[1] - piv[0]) * (piv[1] - piv[2])),
                 (z - piv[0]) * (z - piv[1]) / ((piv[2] - piv[0]) * (piv[2] - piv[1]))]
            nodes.append((f, mp.mpf(float(L)), mp.mpf(float(w)) * om0, mp.mpf(float(lf)), l))

    def total(*t):
        if v == "zevol":
            al = mp.mpf(float(inp["sch_al0"])) if fsa else t[6]
        else:
            al = mp.mpf(float(inp["sch_al0"])) if fsa else t[2]
        kF = 2 if fsa else 3
        tot = mp.mpf(0)
        for f, L, w, lf, l in nodes:
            if v == "zevol":
                Ls = l[0] * t[0] + l[1] * t[1] + l[2] * t[2]
                ph = l[0] * t[3] + l[1] * t[4] + l[2] * t[5]
            else:
                Ls, ph = t[0], t[1]
            if v == "free":
                Flim, aC = t[kF + f], t[kF + nf]
            else:
                Flim, aC = mp.mpf(float(inp["Flim0"][f])), mp.mpf(float(inp["alpha0"]))
            x = L - Ls
            y = (lf + 17) - mp.log10(Flim)
            num = aC * y
            fc = (1 + num / mp.sqrt(1 + num * num)) / 2
            d = 1 - mp.exp(-mp.mpf(10) ** (y + kappa / aC))
            tot += w * ln10 * mp.exp(ln10 * (ph + x * (al + 1)) - mp.mpf(10) ** x + mp.log(fc) / d)
        return tot

    at = tuple(mp.mpf(float(x)) for x in th)
    return np.array([float(mp.diff(total, at, tuple(int(i == e) for i in range(len(at))))) for e in range(len(at))])


@pytest.mark.parametrize("fsa", [False, True])
@pytest.mark.parametrize("variant", ["free", "fixcomp", "zevol"])
def test_formulas_against_30_digit_differentiation_of_the_sum(variant, fsa):
    import mpmath  # noqa: F401  (a missing module is an error, not a skip: this is the only check of the formulas)
    worst = 0.0
    for sig in (0.09, 0.30):
        model = C.const_model(sig)
        for name in PROBES:
            inp, th = probe(variant, fsa, name)
            nl, _ = D.cut_nodes(inp, *model)
            tot, g, s = D.cut_term_grad(inp, *model, th, terms=True)
            assert same_value(variant, tot, *D.cut_term(inp, *model, th, terms=True)) and np.all(s > 0.0)
            ratio = np.abs(g - mp_grad(inp, th, nl)) / s
            print("formula %-7s fix_sch_al %d %-9s sigma = %.2f (%d nodes): worst |twin - mpmath| / S_abs = %.2e"
                  % (variant, fsa, name, sig, nl[0]["L"].size, ratio.max()))
            worst = max(worst, float(ratio.max()))
    print("formula %s fix_sch_al %d: worst ratio %.2e, bound %.1e" % (variant, fsa, worst, FORMULA_BOUND))
    assert FORMULA_BOUND == 10 * 3.6e-16
    assert worst <= FORMULA_BOUND


def case(variant, nf=3, fsa=False, S=5):
    inp = C.cut_inputs(variant, n=100, S=S, nf=nf, fix_sch_al=fsa)
    nodes, sig = C.flux_model(0.05, nf=nf)
    sig = np.minimum(sig * np.array([1.0, 0.5, 1.4, 0.8, 1.2])[:nf, None], D.CUT_SIGMA_MAX)
    th = synth.walkers(variant, 3, seed=5, fix_sch_al=fsa, nf=nf)
    return inp, (nodes, sig), th


@pytest.mark.parametrize("variant", ["free", "fixcomp", "zevol"])
def test_central_differences_of_cut_term(variant):
    """a loose sanity check: the step's truncation (h^2 f''' / 6) and the value's rounding over h"""
    inp, model, th = case(variant)
    tot, g, s = D.cut_term_grad(inp, *model, th, terms=True)
    assert same_value(variant, tot, *D.cut_term(inp, *model, th, terms=True))
    h = 1e-5
    worst = 0.0
    for e in range(th.shape[1]):
        up, dn = th.copy(), th.copy()
        up[:, e] += h
        dn[:, e] -= h
        fd = (D.cut_term(inp, *model, up) - D.cut_term(inp, *model, dn)) / (2 * h)
        worst = max(worst, float(np.max(np.abs(g[:, e] - fd) / s[:, e])))
        assert np.all(np.abs(g[:, e] - fd) <= 1e-6 * s[:, e]), (variant, e)
    print("central differences %s: worst |g - fd| / S_abs = %.2e" % (variant, worst))


@pytest.mark.parametrize("variant", ["free", "fixcomp", "zevol"])
def test_exact_zeros_and_structure(variant):
    nf = 3
    inp, model, th = case(variant)
    nd = G.ndim_of(inp)
    # sigma = 0 everywhere: exactly 0
    tot, g, s = D.cut_term_grad(inp, *C.const_model(0.0, nf=nf), th, terms=True)
    assert np.all(tot == 0.0) and np.all(g == 0.0) and np.all(s == 0.0) and not np.signbit(g).any()
    tot, g, s = D.cut_term_grad(inp, *model, th, terms=True)
    assert g.shape == (3, nd) and np.all(np.isfinite(g)) and np.all(g != 0.0) and np.all(s >= np.abs(g))
    # the sum over fields=[f] is the whole, up to ordering
    per = [D.cut_term_grad(inp, *model, th, fields=[f]) for f in range(nf)]
    assert np.all(np.abs(sum(p[1] for p in per) - g) <= 4e-16 * s)
    assert np.all(np.abs(sum(p[0] for p in per) - tot) <= 4e-16 * D.cut_term(inp, *model, th, terms=True)[1])
    # the elements: FREE has Flim_f - field f's nodes only - and alpha_C; FIXCOMP and ZEVOL have no completeness element
    if variant == "free":
        assert nd == 3 + nf + 1
        for f in range(nf):
            assert np.array_equal(per[f][1][:, 3 + f], g[:, 3 + f])
            others = [3 + q for q in range(nf) if q != f]
            assert np.all(per[f][1][:, others] == 0.0)
    else:
        assert nd == (7 if variant == "zevol" else 3)
    # phi does get a term here (unlike Delta's gradient): d Delta B / d phi* = ln10 Delta B
    if variant == "zevol":
        assert np.all(np.abs(g[:, 3:6].sum(axis=1) - G.LN10 * tot) <= 4e-16 * s[:, 3:6].sum(axis=1))
    else:
        assert np.all(np.abs(g[:, 1] - G.LN10 * tot) <= 4e-16 * s[:, 1])
    # fix_sch_al drops alpha: the other elements are those of the free slope held at sch_al0
    inp_f, _, _ = case(variant, fsa=True)
    ia = 6 if variant == "zevol" else 2
    th_al = th.copy()
    th_al[:, ia] = inp_f["sch_al0"]
    gf = D.cut_term_grad(inp_f, *model, np.delete(th_al, ia, axis=1))[1]
    assert gf.shape == (3, nd - 1) and np.array_equal(gf, np.delete(D.cut_term_grad(inp, *model, th_al)[1], ia, axis=1))
    # limit is honoured
    nl, _ = D.cut_nodes(inp, *model, limit=65)
    assert [n["L"].size for n in nl] == [65] * nf
    tl, gl = D.cut_term_grad(inp, *model, th, limit=65)
    assert same_value(variant, tl, *D.cut_term(inp, *model, th, terms=True, limit=65)) and np.all(gl != g)
    # one row
    one = D.cut_term_grad(inp, *model, th[1], terms=True)
    assert one[0] == tot[1] and np.array_equal(one[1], g[1]) and np.array_equal(one[2], s[1])


@pytest.mark.parametrize("variant", ["free", "fixcomp", "zevol"])
def test_combined_twin(variant):
    inp, model, th = case(variant)
    sg = np.random.default_rng(1).uniform(0.0, 0.04, len(inp["lum"]))
    th[1, 0] = 39.0                                  # outside the box
    val, g, s = D.lnprob_err_grad(inp, sg, th, K=8, terms=True, cut=model)
    assert np.array_equal(val, D.lnprob_err(inp, sg, th, K=8, cut=model)) and val[1] == -np.inf and np.isfinite(val[[0, 2]]).all()
    v0, g0, s0 = D.lnprob_err_grad(inp, sg, th, K=8, terms=True)
    _, gB, sB = D.cut_term_grad(inp, *model, th, terms=True)
    assert np.isnan(g[1]).all() and np.isnan(s[1]).all()
    ok = [0, 2]
    assert np.array_equal(g[ok], g0[ok] - gB[ok]) and np.array_equal(s[ok], s0[ok] + sB[ok])
    assert not np.array_equal(g[ok], g0[ok])
    # without `cut` nothing changes
    assert np.array_equal(D.lnprob_err_grad(inp, sg, th, K=8)[1], g0, equal_nan=True)
    one = D.lnprob_err_grad(inp, sg, th[0], K=8, cut=model)
    assert one[0] == val[0] and np.array_equal(one[1], g[0])
    # the limit reaches both parts
    vl, gl = D.lnprob_err_grad(inp, sg, th, K=8, cut=model, limit=65)
    assert np.array_equal(vl, D.lnprob_err_cut(inp, sg, th, model, K=8, limit=65))
    assert np.array_equal(gl[ok], g0[ok] - D.cut_term_grad(inp, *model, th, limit=65)[1][ok])


def test_class_surface():
    from lf_deconvlib import fixcomp_model
    cat = synth.catalogue(400, seed=17)
    with pytest.raises(ValueError, match="deconvolve_cut_grad=True needs deconvolve_cut=True"):
        fixcomp_model(cat, deconvolve=True, deconvolve_cut_grad=True)
    with pytest.raises(ValueError, match="deconvolve_cut_grad=True needs deconvolve_cut=True"):
        fixcomp_model(cat, deconvolve_cut_grad=True)
    o = fixcomp_model(cat, deconvolve=True, min_comp_frac=0.5, deconvolve_cut=True)
    assert o.deconvolve_cut_grad is False
    with pytest.raises(NotImplementedError, match="the convolved likelihood's gradient is not implemented under deconvolve_cut=True: "
                                                  "the gradient of Delta B, the cut's change of the expected counts, is missing"):
        o._grad_fn("convolved")
    on = fixcomp_model(cat, deconvolve=True, min_comp_frac=0.5, deconvolve_cut=True, deconvolve_cut_grad=True)
    assert on.deconvolve_cut_grad is True and on.deconvolve_cut is True


def test_c_abi_entry():
    import os
    import re
    from lumfuncmcmc_amd import build, capi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "lfmcmc.h")).read()
    assert re.search(r"int lf_cut_term_grad_batch\(lf_ctx \*ctx, const double \*theta, int B, double \*out, double \*grad\);", hdr)
    assert "#define LF_ABI_VERSION 3" in hdr and '"deconv_cut_grad"' in hdr
    lib = capi.load()
    assert "lf_cut_term_grad_batch" in capi.EXPORTS and hasattr(lib, "lf_cut_term_grad_batch")
    assert lib.lf_abi_version() == 3
    assert lib.lf_cut_term_grad_batch(None, None, 1, None, None) == capi.LF_ERR_ARG      # refused before any device is touched
    assert "lf_deconv_cut_grad.h" in " ".join(build.HEADERS)
    assert callable(capi.LFContext.cut_term_grad)
