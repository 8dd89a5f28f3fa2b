"""The element-wise probes of the gradient and flux-error forms without a GPU: tests/grad_probe.hip cross-compiles for gfx950
with the library's flags; every generator of tests/lf_gradproblib.py yields what it promises; the NumPy binary64 figures that
the caps of the GPU tests (tests/test_gpu_gradterms.py, tests/test_gpu_veff.py) rest on are measured here, on the CPU, from
the reference arithmetic; and for each family one seeded mutation of the NumPy expression shows that the metric sees a
subtle error (no mutated device code is built or run)."""
import math
import os

import numpy as np

import lf_gradproblib as P
import lf_isalib
from lumfuncmcmc_amd import deconv as D, grad as G, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "grad_probe.hip")
VARIANTS = (P.FREE, P.FIXCOMP, P.ZEVOL)


def test_probe_unit_compiles_for_gfx950():
    names = list(lf_isalib.remarks(SRC, "-c"))
    # three completeness forms and the basis; the library's own kernels, three variants each
    assert sum("probe_comp" in n for n in names) == 3 and sum("probe_basis" in n for n in names) == 1, names
    for k in ("lf_grad_part", "lf_deconv_part", "lf_deconv_grad_part"):
        assert sum(k in n for n in names) == 3, (k, names)


def test_completeness_inputs_cover_what_they_promise():
    c = P.case_dgrad_comp()["l"]
    aC, y, v, num = c["aC"], c["y"], c["v"], c["num"]
    assert len(aC) <= P.NMAX and c["n_signchange"] >= 100
    assert set(P.AC_EDGES) <= set(aC.tolist()) and synth.ALPHA_LIMS[0] in aC and synth.ALPHA_LIMS[1] in aC and np.any(aC < 0)
    z = num == 0.0
    assert np.any(z & np.signbit(num)) and np.any(z & ~np.signbit(num)) and np.any(num == P.TINY) and np.any(num == -P.TINY)
    for k in P.NUM_DECADES:                           # the neighbours of +-10^k, through the product alpha_C y
        for s in (1.0, -1.0):
            assert np.sum(np.abs(num / (s * 10.0 ** k) - 1.0) < 1e-14) >= 5, (k, s)
    assert v.min() == 1e-300 and np.any(v == 1.0) and np.any(v == 700.0) and v.max() >= 1.0e4
    assert np.all(np.isin(P.ulps_around(P.L.LF_UNDERFLOW), v))
    with np.errstate(under="ignore"):
        e = np.exp(-v)
    assert np.any(e == 0.0) and np.any((e > 0.0) & (e < 2.0 ** -1022))          # e == 0 and the subnormal e before it
    for k in ("l", "dF", "dC", "lcomp"):
        q = P.case_dgrad_comp()[k]
        assert np.all(np.isfinite(q["ref"][0])) and np.all(q["yard"] > 0) and np.all(np.isfinite(q["yard"])), k
    # dC near its sign change: both addends present, their sum small against them
    dC = P.case_dgrad_comp()["dC"]
    sc = slice(c["n_zero"], c["n_zero"] + c["n_signchange"], 2)
    assert np.median(np.abs(dC["ref"][0][sc]) / (dC["yard"][sc] / P.U53)) < 1e-10
    g = P.case_grad_comp()["l"]
    assert g["flim"].min() == synth.FLIM_LIMS[0] and g["flim"].max() == synth.FLIM_LIMS[1] and np.any(g["aC"] < 0)
    assert np.any(g["y"] < -1.4) and np.any(g["y"] > 1.9) and np.any(np.abs(g["y"]) < 1e-11)
    for k in ("l", "dF", "dC"):
        q = P.case_grad_comp()[k]
        assert np.all(np.isfinite(q["ref"][0])) and np.all(q["yard"] > 0), k


def test_basis_inputs_cover_the_pivots():
    c = P.case_basis()
    for ps in P.PIVOT_SETS:
        sel = (c["piv"] == np.array(ps)).all(axis=1)
        z = c["z"][sel]
        assert np.all(np.isin(P.ulps_around(np.array(ps)), z)) and ps[0] - 0.5 in z and ps[2] + 0.5 in z
        assert (ps[0] + ps[1]) / 2 in z and z.min() >= ps[0] - 0.5 and z.max() <= ps[2] + 0.5
    ref = c["ref"][0].reshape(-1, 3)
    at = (c["z"][:, None] == c["piv"])                # at a pivot the basis is the unit vector, exactly 0 elsewhere
    assert at.any(axis=1).sum() == 6 and np.all(ref[at.any(axis=1)][~at[at.any(axis=1)]] == 0.0)
    assert np.allclose(ref.sum(axis=1), 1.0, atol=1e-14)


def test_grad_part_items_reach_the_underflow():
    for v in VARIANTS:
        for fsa in (0, 1):
            c = P.case_grad_part(v, fsa)
            R, items, ns = c["shape"]
            n = c["n"]
            ref = c["ref"][0].reshape(c["shape"])
            assert np.all(np.isfinite(ref)) and np.all(c["yard"] > 0)
            t0 = 10.0 ** (c["lum"] - 42.5)
            assert t0.min() <= 1.01e-6 and t0.max() >= 799.0 and np.sum((t0 > 745.0) & (t0 < 746.5)) >= 3
            # nodes whose integrand is 0 in binary64 (exp(-t) past the underflow) and nodes with a subnormal one
            I = ref[:, n:, 4 if v == P.ZEVOL else 1] if v != P.ZEVOL else np.abs(ref[:, n:, 3:6]).sum(axis=2)
            assert np.sum(I == 0.0) >= 10 and np.sum(I > 1e-300) >= 100, (v, fsa)
            assert np.all(ref[:, :, 7] == 0.0)
    assert P.case_grad_part(P.FREE, 0)["rows"].shape == (4, 5) and P.case_grad_part(P.FREE, 1)["rows"].shape == (4, 4)
    assert P.case_grad_part(P.ZEVOL, 1)["rows"].shape == (4, 6)


def test_deconv_sources_cover_what_they_promise():
    for v in VARIANTS:
        s = P.deconv_sources(v)
        assert s["n"] == 200 and set(s["sigma"].tolist()) == set(P.SIGMAS) | {0.0} and np.sum(s["sigma"] == 0.0) == 20
        y0 = (s["logf"] + 17.0) - np.log10(P.FLIM0)
        assert y0.min() < -1.49 and y0.max() > 1.99
        assert s["lum"][-1] == 45.4 and s["sigma"][-1] == 0.3 and P.deconv_rows(v)[1, 0] < 40.01     # the far corner
        c4, c32 = P.case_deconv(v, 4)["delta"], P.case_deconv(v, 32)["delta"]
        on = s["sigma"] > 0.0
        # maxima ascending with k (every node rescales) and descending (none does), exponent spreads of hundreds
        assert np.sum(c4["rises"] == 4) >= 5 and np.sum(c4["max_first"] & on) >= 20
        assert c32["rises"].max() >= 20 and c32["rises"][on].min() <= 4 and c32["spread"].max() > 1.0e5
        assert np.sum(c32["spread"] > 300.0) >= 10 and np.sum(c4["spread"] > 300.0) >= 5
        for K in (4, 32):
            for k in ("delta", "grad"):
                c = P.case_deconv(v, K)[k]
                assert np.all(np.isfinite(c["ref"][0])) and np.all(c["yard"] > 0) and len(c["yard"]) <= P.NMAX
            d = P.case_deconv(v, K)["delta"]["ref"][0].reshape(4, -1)
            assert np.all(d[:, ~on] == 0.0) and np.all(P.case_deconv(v, K)["delta"]["np"].reshape(4, -1)[:, ~on] == 0.0)
    # no node exponent of -inf inside the model's domain (lf_gradproblib's docstring): the twin's exponents of the far-corner
    # source at K = 32, sigma = 0.3 are all finite
    s = P.deconv_sources(P.FREE)
    x, lnw = D.gauss_hermite(32)
    _, _, _, _, p, a = P.deconv_item_mp(P.FREE, P.deconv_rows(P.FREE)[1], s, s["n"] - 1, x, lnw)
    assert all(P.mp.isfinite(v) for v in a)


def test_a_node_of_zero_weight_is_skipped_by_the_twin():
    """The rule `a node whose exponent is -inf adds exactly 0`, stated on the twin alone: a table with one more node of weight 0
    (ln w = -inf), first, in the middle or last, gives the bits of the table without it."""
    for v in VARIANTS:
        s = P.deconv_sources(v)
        inp = P.deconv_inp(v, s)
        th = P.deconv_rows(v)[0]
        x, lnw = D.gauss_hermite(4)
        with np.errstate(all="ignore"):
            want = D._row_terms(inp, s["sigma"], th, x, lnw)
            wd, wg, _ = D._row_grad_terms(inp, s["sigma"], th, x, lnw)
            for pos in (0, 2, 4):
                x5, l5 = np.insert(x, pos, 0.3), np.insert(lnw, pos, -np.inf)
                assert np.array_equal(D._row_terms(inp, s["sigma"], th, x5, l5), want), (v, pos)
                gd, gg, _ = D._row_grad_terms(inp, s["sigma"], th, x5, l5)
                assert np.array_equal(gd, wd) and np.array_equal(gg, wg), (v, pos)


def test_veff_inputs_cover_what_they_promise():
    n = 0
    for cfg in P.veff_cases():
        c = P.case_veff(*cfg)
        r = c["flux"] / c["flim"]
        assert r.max() > 999.0 and (r.min() < 1.1e-3 or cfg[1] > 0) and np.all(np.isfinite(c["ref"][0])) and np.all(c["yard"] > 0)
        if cfg[2]:
            assert c["zero"].sum() == 2 and np.all(c["ref"][0][c["zero"]] == 0.0) and {0.0, -1.0} <= set(c["vol"].tolist())
        n += len(r)
    assert n >= 2000 and {cfg[0] for cfg in P.veff_cases()} == {0.6, 4.56, 10.0}


def numpy_figures():
    cd, cg = P.case_dgrad_comp(), P.case_grad_comp()
    figs = {"dgrad_comp_l": P.numpy_figure("dgrad_comp_l", cd["l"]), "dgrad_comp_dF": P.numpy_figure("dgrad_comp_dF", cd["dF"]),
            "dgrad_comp_dC": P.numpy_figure("dgrad_comp_dC", cd["dC"]), "deconv_lcomp": P.numpy_figure("deconv_lcomp", cd["lcomp"]),
            "grad_comp_l": P.numpy_figure("grad_comp_l", cg["l"]), "grad_comp_dF": P.numpy_figure("grad_comp_dF", cg["dF"]),
            "grad_comp_dC": P.numpy_figure("grad_comp_dC", cg["dC"]), "grad_basis": P.numpy_figure("grad_basis", P.case_basis())}
    for v in VARIANTS:
        nm = P.VNAME[v]
        figs["grad_part_" + nm] = max(P.numpy_figure("grad_part_" + nm, P.case_grad_part(v, f)) for f in (0, 1))
        figs["deconv_delta_" + nm] = max(P.numpy_figure("deconv_delta_" + nm, P.case_deconv(v, K)["delta"]) for K in (4, 32))
        figs["deconv_grad_" + nm] = max(P.numpy_figure("deconv_grad_" + nm, P.case_deconv(v, K)["grad"]) for K in (4, 32))
    figs["veff_phi"] = max(P.numpy_figure("veff_phi", P.case_veff(*cfg)) for cfg in P.veff_cases())
    return figs


def test_numpy_figures_behind_the_caps():
    """max err / yardstick of the same expressions in plain NumPy binary64 (the twins' statements), against the 40-digit values:
    the caps of the GPU tests are 4 x these and never below 2 (lf_gradproblib.CAPS holds them as constants; this test says
    when they have moved)."""
    figs = numpy_figures()
    assert set(figs) == set(P.CAPS)
    for k, (fig, i) in figs.items():
        print("numpy %-22s max err / yard %9.3f at index %d   cap %g" % (k, fig, i, P.CAPS[k]))
    for k, (fig, i) in figs.items():
        assert math.isfinite(fig), k
        assert P.cap_from(fig) <= P.CAPS[k] * 1.05 and P.cap_from(fig) >= P.CAPS[k] * 0.8, (k, fig, P.CAPS[k])


def test_the_restated_softmax_is_the_twin():
    """lf_gradproblib.softmax_numpy exists for the mutations below: without one it gives deconv._row_grad_terms's bits"""
    for v in VARIANTS:
        s = P.deconv_sources(v)
        inp = P.deconv_inp(v, s)
        for K in (4, 32):
            x, lnw = D.gauss_hermite(K)
            for th in P.deconv_rows(v):
                with np.errstate(all="ignore"):
                    d0, g0, _ = D._row_grad_terms(inp, s["sigma"], th, x, lnw)
                d1, g1 = P.softmax_numpy(v, th, s, x, lnw)
                assert np.array_equal(d0, d1) and np.array_equal(g0, g1), (v, K)


def _mutated_deconv(v, K, mutate):
    c = P.case_deconv(v, K)
    s, nodes = c["delta"]["src"], c["delta"]["nodes"]
    dl, gr = [], []
    for th in c["delta"]["rows"]:
        d, g = P.softmax_numpy(v, th, s, nodes[:K], nodes[K:], mutate)
        dl.append(d)
        gr.append(P.deconv_slots_from_twin(v, th, g))
    return P.measure(c["delta"], np.concatenate(dl))[0], P.measure(c["grad"], np.concatenate(gr).ravel())[0]


def test_the_metric_sees_a_subtle_error():
    """One mutation of the NumPy expression per family: each is an error a sum over a catalogue hides (a form that is
    mathematically the same but cancels, a factor that is 1 for most sources, a rescaling that only ascending maxima need), and
    each must push max err / yard above the cap, or the probes above mean nothing."""
    c = P.case_dgrad_comp()
    with np.errstate(all="ignore"):
        for mutate, outs in (("gp_branch", (1, 2)), ("w_no_e", (1, 2))):
            got = P.lcomp_grad_numpy(c["l"]["y"], c["l"]["v"], c["l"]["aC"], P.KAPPA, mutate)
            for j in outs:
                k = ("l", "dF", "dC")[j]
                fig = P.measure(c[k], got[j])[0]
                print("mutation %-10s dgrad_comp_%-2s max err / yard %.3g (cap %g)" % (mutate, k, fig, P.CAPS["dgrad_comp_" + k]))
                assert fig > P.CAPS["dgrad_comp_" + k], (mutate, k, fig)
        # ... and the unmutated restatement is the twin's
        ref = D._lcomp_grad(c["l"]["y"], c["l"]["v"], c["l"]["aC"], P.KAPPA)
        assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(ref, P.lcomp_grad_numpy(c["l"]["y"], c["l"]["v"], c["l"]["aC"], P.KAPPA)))
    for v in VARIANTS:
        nm = P.VNAME[v]
        for K in (4, 32):
            fd, fg = _mutated_deconv(v, K, "no_rescale")
            print("mutation no_rescale %-8s K=%2d grad %.3g (cap %g)" % (nm, K, fg, P.CAPS["deconv_grad_" + nm]))
            assert fg > P.CAPS["deconv_grad_" + nm], (nm, K, fg)
            fd, fg = _mutated_deconv(v, K, "em_pow")
            print("mutation em_pow     %-8s K=%2d delta %.3g grad %.3g" % (nm, K, fd, fg))
            assert fd > P.CAPS["deconv_delta_" + nm] and fg > P.CAPS["deconv_grad_" + nm], (nm, K, fd, fg)
    b = P.case_basis()
    sw = np.concatenate([G._basis(b["z"][(b["piv"] == np.array(ps)).all(axis=1)], (ps[1], ps[0], ps[2])).T for ps in P.PIVOT_SETS]).ravel()
    fig = P.measure(b, sw)[0]
    print("mutation pivots swapped: basis max err / yard %.3g" % fig)
    assert fig > P.CAPS["grad_basis"]
