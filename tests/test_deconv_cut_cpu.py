"""The convolved likelihood under a cut on the observed flux, on the CPU: the NumPy twin of Delta B
(deconv.cut_term) against 30-digit integration, its exact properties, the model itself against a seeded generator, and the
library's surface.  No GPU."""
import os
import re

import numpy as np
import pytest

from lumfuncmcmc_amd import deconv, synth
import lf_cutlib as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = {"0.02": lambda: C.const_model(0.02), "0.09": lambda: C.const_model(0.09), "0.30": lambda: C.const_model(0.30),
          "1/flux": lambda: C.flux_model(0.09)}


@pytest.mark.parametrize("name", sorted(MODELS))
def test_twin_against_30_digit_integration(name):
    """Per (field, column) |twin - mpmath| <= 1e-7 of the column's plain integral, at the box's centre and at the alpha_C = 7
    corners with alpha = -3 and +1, for sigma at the cut of 0.02, 0.09, 0.30 dex and a model proportional to 1 / flux."""
    import mpmath  # noqa: F401  (a missing module is an error, not a skip: this is the only check of the accuracy target)
    inp = C.cut_inputs("free", n=60, S=3, nf=1)
    nodes, sig = MODELS[name]()
    th = C.probe_thetas(inp)
    tw = deconv.cut_term(inp, nodes, sig, th, per_column=True)
    worst = 0.0
    for b in range(len(th)):
        for j in range(3):
            ref, plain = C.mp_column(inp, th[b], 0, j, nodes, sig[0])
            err = abs(tw[b, 0, j] - ref) / plain if plain > 0 else 0.0
            print("cut accuracy %s theta %d column %d: twin %.12e ref %.12e err/plain %.2e" % (name, b, j, tw[b, 0, j], ref, err))
            worst = max(worst, err)
    assert worst <= 1.0e-7, worst


def test_zero_error_is_exactly_zero():
    inp = C.cut_inputs("free", S=5, nf=2, n=100)
    th = synth.walkers("free", 4, seed=2, nf=2)
    dB, sabs = deconv.cut_term(inp, *C.const_model(0.0, nf=2), th, terms=True)
    assert np.all(dB == 0.0) and np.all(sabs == 0.0)


def test_additive_over_fields():
    inp = C.cut_inputs("free", S=5, nf=3, n=100)
    nodes, sig = C.flux_model(0.05, nf=3)
    sig = sig * np.array([1.0, 0.5, 1.4])[:, None]
    th = synth.walkers("free", 3, seed=5, nf=3)
    whole, sabs = deconv.cut_term(inp, nodes, sig, th, terms=True)
    parts = sum(deconv.cut_term(inp, nodes, sig, th, fields=(f,)) for f in range(3))
    assert np.all(np.abs(whole - parts) <= 4e-16 * sabs)
    one = np.where(np.arange(3)[:, None] == 1, sig, 0.0)
    assert np.all(deconv.cut_term(inp, nodes, one, th) == deconv.cut_term(inp, nodes, sig, th, fields=(1,)))


def test_limit_of_small_errors():
    inp = C.cut_inputs("free", S=5, nf=1, n=100)
    th = C.probe_thetas(inp)[:1]
    v = [abs(deconv.cut_term(inp, *C.const_model(s), th)[0]) for s in (0.1, 0.01, 0.001, 0.0001)]
    print("Delta B at sigma 0.1, 0.01, 0.001, 0.0001:", v)
    assert v[0] > v[1] > v[2] > v[3] > 0.0
    assert v[3] < 1e-4 * v[0]                      # (the leading term is of second order in sigma)


@pytest.mark.parametrize("M", [1, 16])
def test_error_model_sizes(M):
    inp = C.cut_inputs("free", S=5, nf=1, n=100)
    nodes, sig = (C.const_model(0.07) if M == 1 else C.flux_model(0.07, M=16))
    nl, H = deconv.cut_nodes(inp, nodes, sig)
    assert H[0] == 7.5 * sig.max() and nl[0]["L"].size % 8 == 0 and nl[0]["L"].size > 0
    lam = inp["logL"][0]
    below = nl[0]["L"] < lam[nl[0]["col"]]
    assert np.all(nl[0]["w"][below] > 0.0) and np.all(nl[0]["w"][~below] < 0.0)
    if M == 16:                                    # no panel straddles a node of the error model
        ld2 = nl[0]["L"] - nl[0]["logf"]
        for p in range(nl[0]["L"].size // 8):
            t = nl[0]["logf"][8 * p:8 * p + 8]
            assert np.searchsorted(nodes, t.min(), side="right") == np.searchsorted(nodes, t.max(), side="right"), (p, ld2[8 * p])
    assert np.isfinite(deconv.cut_term(inp, nodes, sig, C.probe_thetas(inp))).all()


def test_clamped_columns_share_their_edge():
    inp = C.cut_inputs("free", S=7, nf=1, n=100)
    lam = inp["logL"][0]
    assert lam[0] == lam[1] == lam[2] and lam[3] > lam[2]           # (the clamp: columns 0 .. S // 3)
    nodes, sig = C.flux_model(0.09)
    pc = deconv.cut_term(inp, nodes, sig, C.probe_thetas(inp)[0], per_column=True)
    assert np.all(pc[0, 1:-1] != 0.0) and pc[0, 0] != 0.0
    # in a clamped column the edge lies above the flux cut: the error model is read at a brighter flux there
    nl, _ = deconv.cut_nodes(inp, nodes, sig)
    n0 = nl[0]
    assert np.all(np.abs(n0["L"][n0["col"] == 0] - lam[0]) <= 7.5 * sig.max())


def test_refusals_of_the_twin():
    with pytest.raises(ValueError, match="0.30 dex"):
        deconv.check_cut_error_model([0.0], [[0.31]], 1)
    with pytest.raises(ValueError, match="increase"):
        deconv.check_cut_error_model([0.0, 0.0], [[0.1, 0.1]], 1)
    with pytest.raises(ValueError, match="all 0"):
        deconv.check_cut_error_model([0.0, 1.0], [[0.0, 0.1]], 1)
    with pytest.raises(ValueError, match=">= 0"):
        deconv.check_cut_error_model([0.0], [[-0.1]], 1)


def test_the_model_is_right():
    """A seeded host generator samples the Poisson process of one field down to Lam - H, adds the noise at the true flux and
    cuts on L_o.  Over R replicates at the true theta the mean count that passes agrees with B + Delta B within 4 standard
    errors and differs from B alone by more than 5.  B here is the generator's own expected count above the edge without noise
    (the same fine grid: the trapezoid rule's error of the S-point grid is not what is tested)."""
    inp = C.cut_inputs("free", S=5, nf=1, n=100)
    th = np.array([synth.LSTAR, -3.0, -2.0, 3.0, synth.ALPHA_C])
    nodes, sig = C.const_model(0.2)
    R = 200
    cnt, b_fine, tot = C.poisson_counts(inp, th, nodes, sig[0], R, seed=5)
    dB = float(deconv.cut_term(inp, nodes, sig, th))
    se = cnt.std(ddof=1) / np.sqrt(R)
    print("model check: B %.3f  Delta B (twin) %.3f  mean count %.3f  s.e. %.3f  -> (mean - B - dB) / se = %.2f, (mean - B) / se = %.2f"
          % (b_fine, dB, cnt.mean(), se, (cnt.mean() - b_fine - dB) / se, (cnt.mean() - b_fine) / se))
    assert abs(dB) > 5.0 * np.sqrt(b_fine / R)          # (the catalogue size and R resolve the term: checked for the twin)
    assert abs(cnt.mean() - (b_fine + dB)) <= 4.0 * se
    assert abs(cnt.mean() - b_fine) > 5.0 * se


def profile_maxima(cat, s, th, model):
    """{element: (offset of the maximum without Delta B, with it, the profile's curvature sigma)}: 1-D profiles of the convolved
    likelihood in L*, phi* and alpha around the truth, the others held at it; 21 points, a parabola through the top three"""
    out = {}
    for e, half in ((0, 0.1), (1, 0.1), (2, 0.2)):
        g = np.linspace(-half, half, 21)
        rows = np.repeat(th[None], g.size, axis=0)
        rows[:, e] += g
        val = deconv.lnprob_err(cat, s, rows, wide=True)
        dB = deconv.cut_term(cat, model[0], model[1], rows)
        res = []
        for y in (val, val - dB):
            i = int(np.clip(np.argmax(y), 1, g.size - 2))
            c = np.polyfit(g[i - 1:i + 2], y[i - 1:i + 2], 2)
            res.append(-c[1] / (2.0 * c[0]))
        out[e] = (res[0], res[1], 1.0 / np.sqrt(-2.0 * c[0]))
    return out


def test_the_term_removes_the_bias():
    """One seeded catalogue of the model's process (about 5800 sources that pass the cut, 0.2 dex of noise, alpha = -2, a grid of
    41 columns) and the convolved likelihood profiled in L*, phi* and alpha with and without Delta B.  Without it the expected
    counts are too high by the sources that scatter out across the edge, and phi*, which the counts fix, moves most: its
    maximum lies at -0.016 dex (2.8 of the profile's sigma), against -0.012 in L* and +0.006 in alpha.  With Delta B the
    maximum in phi* lies closer to the truth."""
    inp = C.cut_inputs("free", S=41, nf=1, n=100)
    model = C.const_model(0.2)
    th = np.array([synth.LSTAR, -3.0, -2.0, 3.0, synth.ALPHA_C])
    _, b, _ = C.poisson_counts(inp, th, model[0], model[1][0], 1, seed=1)
    th[1] += np.log10(6000.0 / b)
    cat, s = C.poisson_catalogue(inp, th, model[0], model[1][0], seed=8)
    m = profile_maxima(cat, s, th, model)
    for e, name in ((0, "L*"), (1, "phi*"), (2, "alpha")):
        print("bias profile %-5s: maximum without Delta B at %+.4f, with it at %+.4f (profile sigma %.4f); %d sources"
              % (name, m[e][0], m[e][1], m[e][2], len(s)))
    assert abs(m[1][0]) > abs(m[0][0]) and abs(m[1][0]) > abs(m[2][0])       # phi* is the parameter the missing term biases most
    assert abs(m[1][0]) > 2.0 * m[1][2]                                       # ... by more than the catalogue's noise
    assert abs(m[1][1]) < abs(m[1][0])                                        # and with the term the maximum lies closer to the truth
    assert abs(m[0][1]) < abs(m[0][0])


def test_surface():
    from lumfuncmcmc_amd import build, capi
    build.build_library(verbose=False)
    lib = capi.load()
    hdr = open(os.path.join(ROOT, "include", "lfmcmc.h")).read()
    assert "#define LF_ABI_VERSION 3" in hdr
    decl = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for n in ("lf_set_cut_error_model", "lf_cut_term_batch", "lf_cut_info"):
        assert n in decl and n in capi.EXPORTS and hasattr(lib, n)
    assert lib.lf_set_cut_error_model(None, None, 0, None) == -1
    assert lib.lf_cut_term_batch(None, None, 1, None) == -1
    layout = open(os.path.join(ROOT, "lumfuncmcmc_amd", "csrc", "lf_layout.h")).read()
    for name, val in (("DECONV_CUT_CH", deconv.CUT_CHUNK), ("DECONV_CUT_NPAN", deconv.CUT_NPANEL),
                      ("DECONV_CUT_MAX_PANELS", deconv.CUT_MAX_PANELS), ("DECONV_CUT_MAX_NODES", deconv.CUT_MAX_NODES)):
        assert re.search(r"%s = %d;" % (name, val), layout), name
    for name, val in (("DECONV_CUT_T", deconv.CUT_T), ("DECONV_CUT_PANEL_SIGMA", deconv.CUT_PANEL_SIGMA), ("DECONV_CUT_H", deconv.CUT_H),
                      ("DECONV_CUT_UMAX", deconv.CUT_UMAX), ("DECONV_CUT_SIGMA_MAX", deconv.CUT_SIGMA_MAX)):
        m = re.search(r"%s = ([0-9.]+);" % name, layout)
        assert m and float(m.group(1)) == val, name


def test_class_surface():
    """deconvolve_cut=True accepts min_comp_frac = 0.5; without it the refusal stays"""
    from lf_deconvlib import fixcomp_model
    cat = synth.catalogue(400, seed=17)
    with pytest.raises(ValueError, match="min_comp_frac"):
        fixcomp_model(cat, deconvolve=True, min_comp_frac=0.5)
    o = fixcomp_model(cat, deconvolve=True, min_comp_frac=0.5, deconvolve_cut=True)
    nodes, sig = o.deconvolve_cut_errors
    assert sig.shape == (o.nfields, nodes.size) and np.all(sig == 0.05)
    o2 = fixcomp_model(cat, deconvolve=True, min_comp_frac=0.5, deconvolve_cut=True,
                       deconvolve_cut_errors=(np.array([-17.0, -16.0]), np.full((5, 2), 0.04)))
    assert o2.deconvolve_cut_errors[1].shape == (5, 2)
    with pytest.raises(ValueError, match="deconvolve=True"):
        fixcomp_model(cat, min_comp_frac=0.5, deconvolve_cut=True)
    with pytest.raises(ValueError, match="no cut"):
        fixcomp_model(cat, deconvolve=True, min_comp_frac=0.0, deconvolve_cut=True)
