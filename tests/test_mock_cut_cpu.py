"""Mock catalogues of the cut process, the NumPy twin alone, no GPU: piece "above" is draw_noisy's
sources bit for bit; an all-zero table keeps exactly them; a row depends on (seed, row_id, theta, model) only; the mean kept
count agrees with B + Delta B, and each direction of scatter with its half of Delta B; the model class; the refusals; the
surface of the C ABI.

Expectation (measured, section 3.31's configuration: one field, 0.2 dex, alpha = -2, 200 replicates): the hat process
interpolates phi C linearly between the grid's nodes where Delta B integrates the curve, and next to the edge, where 0.2 dex of
noise weighs a steep curve, that shows on a coarse grid: (mean kept - B - Delta B) / s.e. = +10.8 at S = 5, +4.2 at S = 23, +2.5 at
S = 41 and +1.2 at S = 81 (out-scatter alone: -19.3, -7.9, -3.1, +0.4).  The test runs at S = 81."""
import os
import re

import numpy as np
import pytest

import lf_cutlib as C
import lf_mockcutlib as K
from lumfuncmcmc_amd import deconv, mock, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 4321


def _twin(variant, S, M, const=False, fix_sch_al=False):
    inp = K.inputs(variant, S, fix_sch_al)
    nodes, sig = K.table(M)
    if const:
        sig = np.repeat(sig[:, :1] + 0.05, M, axis=1)              # equal entries: the flux does not matter
    return inp, K.arm(mock.MockTwin(inp), inp, nodes, sig)


def _above(c, r, f):
    """slice of piece "above" of (row r, field f) in the candidate arrays"""
    start = int(c[6].reshape(-1, 2)[:r * c[6].shape[1] + f].sum())
    return slice(start, start + int(c[6][r, f, 0]))


@pytest.mark.parametrize("variant,M,const", [("free", 64, False), ("fixcomp", 1, True), ("zevol", 3, True)])
def test_piece_above_is_draw_noisy(variant, M, const):
    inp, tw = _twin(variant, 23, M, const)
    th = K.rows_for_means(tw, variant, False, (400.0, 30.0, 0.0), 0)
    rid = np.array([7, 1 << 40, 3], dtype=np.int64)
    c = tw.candidates_cut(th, SEED, rid)
    z, Lt, Lo, sg, fld, off = tw.draw_noisy(th, SEED, rid)
    np.testing.assert_array_equal(c[6][:, :, 0].ravel(), np.diff(off))           # the counts of lf_mock_counts
    kept = tw.draw_cut(th, SEED, rid)
    assert off[-1] > 300 and c[6][:, :, 1].sum() > 20
    for r in range(3):
        for f in range(tw.nf):
            a, d = _above(c, r, f), slice(off[r * tw.nf + f], off[r * tw.nf + f + 1])
            assert c[0][a].tobytes() == z[d].tobytes() and c[1][a].tobytes() == Lt[d].tobytes()
            if not const:
                continue
            assert c[2][a].tobytes() == Lo[d].tobytes() and c[3][a].tobytes() == sg[d].tobytes()    # and so the deviates n
            n = d.stop - d.start
            k = tw._sources(th[r], rid[r], f, f, SEED, np.arange(n, dtype=np.uint64))[2] if n else np.zeros(0, dtype=int)
            want = Lo[d] >= tw.logL[0][k]
            np.testing.assert_array_equal(c[5][a] != 0, want)
            ko = kept[5][r * tw.nf + f]
            m = int(want.sum())
            assert kept[2][ko:ko + m].tobytes() == Lo[d][want].tobytes()         # kept order: piece "above" first, in index order
            assert kept[6]["kept"][r, f] - kept[6]["n_scattered_in"][r, f] == m
    assert 0 < kept[6]["kept"].sum() < c[6].sum() and kept[6]["n_scattered_in"].sum() > 0


def test_an_all_zero_table_keeps_piece_above_and_nothing_else():
    inp = K.inputs("free", 23)
    nodes, sig = K.table(3)
    tw = K.arm(mock.MockTwin(inp), inp, nodes, np.zeros_like(sig), H=1.0)
    th = K.rows_for_means(tw, "free", False, (500.0, 20.0), 0)
    z, Lt, Lo, sg, fld, off, info = tw.draw_cut(th, SEED)
    pz, pL, pf, poff = tw.draw(th, SEED)
    assert not info["n_cand"][:, :, 1].any() and not info["mean"][:, :, 1].any() and not info["n_scattered_in"].any()
    assert z.tobytes() == pz.tobytes() and Lt.tobytes() == pL.tobytes() == Lo.tobytes() and not sg.any()
    np.testing.assert_array_equal(off, poff)
    np.testing.assert_array_equal(fld, pf)
    assert off[-1] > 400


def test_a_row_depends_on_seed_row_id_theta_and_model_only():
    inp, tw = _twin("zevol", 23, 64)
    rng = np.random.default_rng(3)
    th = K.rows_for_means(tw, "zevol", False, tuple(rng.uniform(50.0, 400.0, 64)), 0, seed=9)
    rid = rng.integers(0, 1 << 62, 64)
    big, again = tw.draw_cut(th, 77, rid), tw.draw_cut(th, 77, rid)
    perm = rng.permutation(64)
    sh = tw.draw_cut(th[perm], 77, rid[perm])
    nf = tw.nf
    for a, b in zip(big[:6], again[:6]):
        assert a.tobytes() == b.tobytes()
    for i in (0, 37, 63):
        one = tw.draw_cut(th[i:i + 1], 77, rid[i:i + 1])
        p = int(np.flatnonzero(perm == i)[0])
        lo, hi, slo, shi = big[5][i * nf], big[5][(i + 1) * nf], sh[5][p * nf], sh[5][(p + 1) * nf]
        assert hi > lo
        for a, b, c in zip(one[:5], big[:5], sh[:5]):
            assert a.tobytes() == b[lo:hi].tobytes() == c[slo:shi].tobytes()
        for key in ("n_cand", "mean", "kept", "n_scattered_in"):
            assert one[6][key][0].tobytes() == big[6][key][i].tobytes() == sh[6][key][p].tobytes()
    other = tw.draw_cut(th[:1], 78, rid[:1])
    assert other[2].tobytes() != big[2][:other[2].size].tobytes()


def test_the_mean_kept_count_is_b_plus_delta_b():
    """Section 3.31's configuration and criterion (tests/test_deconv_cut_cpu.py::test_the_model_is_right) for the project's own
    generator, S = 81 (the module comment): B is the twin's expected count of piece "above", the grid's trapezoid sum."""
    inp = C.cut_inputs("free", S=81, nf=1, n=100)
    th = np.array([synth.LSTAR, -3.0, -2.0, 3.0, synth.ALPHA_C])
    nodes, sig = C.const_model(0.2)
    tw = K.arm(mock.MockTwin(inp), inp, nodes, sig)
    R = 200
    info = tw.draw_cut(np.repeat(th[None], R, axis=0), 5)[6]
    B = float(info["mean"][0, 0, 0])
    assert B == float(tw.means(th)[0, 0])
    dB = float(deconv.cut_term(inp, nodes, sig, th))
    up, down = (float(v[0]) for v in K.halves(inp, nodes, sig, th))
    assert abs((up - down) - dB) < 1e-9 * (up + down)
    kept = info["kept"][:, 0].astype(float)
    sin = info["n_scattered_in"][:, 0].astype(float)
    sout = (info["n_cand"][:, 0, 0] - (info["kept"][:, 0] - info["n_scattered_in"][:, 0])).astype(float)
    se = lambda v: v.std(ddof=1) / np.sqrt(R)                                    # noqa: E731
    print("cut mock: B %.3f  Delta B %.3f (in %.3f, out %.3f)  mean kept %.3f s.e. %.3f -> (mean - B - dB) / se = %.2f, "
          "(mean - B) / se = %.2f; in %.3f (%.2f se), out %.3f (%.2f se); band candidates per source scattered in %.2f"
          % (B, dB, up, down, kept.mean(), se(kept), (kept.mean() - B - dB) / se(kept), (kept.mean() - B) / se(kept), sin.mean(),
             (sin.mean() - up) / se(sin), sout.mean(), (sout.mean() - down) / se(sout), info["n_cand"][:, 0, 1].sum() / sin.sum()))
    assert abs(dB) > 5.0 * np.sqrt(B / R)
    assert abs(kept.mean() - (B + dB)) <= 4.0 * se(kept)
    assert abs(kept.mean() - B) > 5.0 * se(kept)
    assert abs(sin.mean() - up) <= 4.0 * se(sin)
    assert abs(sout.mean() - down) <= 4.0 * se(sout)


def _class_object(**extra):
    from lf_deconvlib import fixcomp_model
    cat = synth.catalogue(400, seed=17)
    cat["lum_e"] = np.full(400, 0.2)
    # (one flux limit for all fields: the reference evaluates every field's completeness table on its own grid and
    # integrates all of them on the last field's - with different limits B's curve is not the one Delta B integrates)
    kw = dict(deconvolve=True, min_comp_frac=0.5, deconvolve_cut=True, deconvolve_wide=True, Flim=[synth.FLIM[0]] * 5)
    kw.update(extra)
    o = fixcomp_model(cat, **kw)
    theta = np.array([synth.LSTAR, synth.PHISTAR - 1.0, synth.SCH_AL])
    rng = np.random.default_rng(6)
    rows = theta[None] + rng.normal(0.0, 0.02, (100, 3))
    o.samples = np.concatenate([rows, -0.5 * rng.chisquare(3, 100)[:, None]], axis=1)
    return o, theta


def test_the_class_draws_the_process_its_likelihood_models():
    o, theta = _class_object()
    np.random.seed(5)
    pp = o.posterior_predictive(noise="catalogue", cut=True, device=False, ndraws=100, seed=31)
    np.random.seed(5)
    rows = o._posterior_rows(100, 7.5)[:, :-1]
    assert pp["cut"] is True and pp["noise"] == "catalogue"
    np.testing.assert_array_equal(pp["replicated_kept"], pp["replicated_total"])
    dB = deconv.cut_term(o.kernel_inputs(), pp["sigma_model"][0], pp["sigma_model"][1], rows)
    B, tot = pp["expected"].sum(axis=1), pp["replicated_total"].sum(axis=1)
    d, d0 = tot - (B + dB), tot - B
    se = lambda v: v.std(ddof=1) / np.sqrt(v.size)                               # noqa: E731
    print("class: B %.1f  Delta B %.2f  mean total %.1f -> %.2f se of B + Delta B, %.2f se of B"
          % (B.mean(), dB.mean(), tot.mean(), d.mean() / se(d), d0.mean() / se(d0)))
    assert abs(d.mean()) <= 4.0 * se(d)
    assert abs(d0.mean()) > 5.0 * se(d0)
    # the default error model of a deconvolve_cut=True object is the likelihood's
    np.random.seed(5)
    dflt = o.posterior_predictive(cut=True, device=False, ndraws=4, seed=31)
    assert dflt["noise"] == "model" and all(a.tobytes() == b.tobytes() for a, b in zip(dflt["sigma_model"], o.deconvolve_cut_errors))
    c = o.mock_catalogue(theta, seed=3, device=False, cut=True)
    fi = c["field_ind"]
    assert sorted(c) == sorted(["z", "lum", "lum_e", "lum_true", "field_ind", "n_candidates", "n_scattered_in", "theta", "seed"])
    edge = np.asarray(o.kernel_inputs()["logL"])[0].min()
    for f in range(o.nfields):
        n = fi[f + 1] - fi[f]
        assert len(c["lum"][f]) == n < c["n_candidates"][f] and 0 < c["n_scattered_in"][f] < n
        assert (c["lum"][f] >= edge).all() and (c["lum_true"][f] < edge).any()
        assert (c["lum_true"][f][n - c["n_scattered_in"][f]:] <= np.asarray(o.kernel_inputs()["logL"])[0].max()).all()
    # cut=False: what the methods gave before the keyword
    a = o.mock_catalogue(theta, seed=3, device=False, lum_err="catalogue")
    b = o.mock_catalogue(theta, seed=3, device=False, lum_err="catalogue", cut=False)
    assert sorted(a) == sorted(b) and all(x.tobytes() == y.tobytes() for k in ("z", "lum", "lum_e") for x, y in zip(a[k], b[k]))


def test_refusals_of_the_class():
    from lf_deconvlib import fixcomp_model
    o, theta = _class_object(deconvolve_cut=False, deconvolve=False)
    with pytest.raises(ValueError, match="flux-dependent error model"):
        o.mock_catalogue(theta, seed=1, device=False, cut=True)
    with pytest.raises(ValueError, match="flux-dependent error model"):
        o.mock_catalogue(theta, seed=1, device=False, cut=True, lum_err=0.1)
    with pytest.raises(ValueError, match="flux-dependent error model"):
        o.posterior_predictive(device=False, cut=True, ndraws=4)
    nodes = np.array([-17.0, -16.0])
    with pytest.raises(ValueError, match="sigma > 0"):
        o.mock_catalogue(theta, seed=1, device=False, cut=True, lum_err=(nodes, np.zeros((5, 2))))
    cat = synth.catalogue(400, seed=17)
    flat = fixcomp_model(cat, min_comp_frac=0.0)
    with pytest.raises(ValueError, match="min_comp_frac > 0.001"):
        flat.mock_catalogue(theta, seed=1, device=False, cut=True, lum_err="catalogue")
    with pytest.raises(ValueError, match="min_comp_frac > 0.001"):
        flat.posterior_predictive(device=False, cut=True, noise="catalogue")


def test_refusals_of_the_twin():
    inp = K.inputs("fixcomp", 5)
    nodes, sig = K.table(3)
    tw = mock.MockTwin(inp)
    th = synth.walkers("fixcomp", 2, seed=5)
    lb = mock.band_grid(inp, 1.0)
    ipb = mock.band_integ_part(inp, lb)
    with pytest.raises(mock.MockError, match="no error model"):
        tw.set_cut_band(lb, ipb)
    with pytest.raises(mock.MockError, match="no error model"):
        tw.draw_cut(th, 1)
    tw.set_error_model(nodes, sig)
    with pytest.raises(mock.MockError, match="no cut band"):
        tw.draw_cut(th, 1)
    with pytest.raises(mock.MockError, match="no cut band"):
        tw.hist_cut(th, np.linspace(40.0, 44.0, 5), 1)
    with pytest.raises(mock.MockError, match="integ_part_b"):
        tw.set_cut_band(lb, None)
    with pytest.raises(mock.MockError, match=r"\(S, S\)"):
        tw.set_cut_band(lb[:-1], ipb)
    with pytest.raises(mock.MockError, match=r"\(nf, S, S\)"):
        tw.set_cut_band(lb, ipb[:1])
    bad = lb.copy()
    bad[-1, 2] += 1e-9
    with pytest.raises(mock.MockError, match="column 2: row S - 1 of logLb must equal row 0 of logL"):
        tw.set_cut_band(bad, ipb)
    bad = lb.copy()
    bad[2, 1] = bad[1, 1]
    with pytest.raises(mock.MockError, match="column 1 node 2: the band's luminosity nodes must be finite and strictly ascending"):
        tw.set_cut_band(bad, ipb)
    bad = lb.copy()
    bad[0, 3] = np.nan
    with pytest.raises(mock.MockError, match="column 3 node 0"):
        tw.set_cut_band(bad, ipb)
    bad = ipb.copy()
    bad[1, 0, 0] = -1.0
    with pytest.raises(mock.MockError, match="field 1: integ_part_b must be finite and >= 0"):
        tw.set_cut_band(lb, bad)
    with pytest.raises(mock.MockError, match="H must be finite and > 0"):
        mock.band_grid(inp, 0.0)
    tw.set_cut_band(lb, ipb)
    assert tw.draw_cut(th, 1)[6]["n_cand"].shape == (2, K.NF, 2)
    nonfin = th.copy()
    nonfin[1, 0] = np.inf
    with pytest.raises(mock.MockError, match="row 1: theta is not finite"):
        tw.draw_cut(nonfin, 1)
    big = th.copy()
    big[0, 1] = 40.0
    with pytest.raises(mock.MockError, match=r'row 0 field 0: .*above 2\^31 \(piece "above"\)'):
        tw.draw_cut(big, 1)
    # piece "below" alone above the cap: a band so deep that it holds more than the grid
    tw2 = K.arm(mock.MockTwin(inp), inp, nodes, sig, H=6.0)
    th2 = th[:1].copy()
    th2[0, 2] = -2.9                                                             # a steep faint end: the band holds the most
    th2[0, 1] += np.log10(0.9 * mock.MAX_MEAN / tw2.means(th2)[0, 0])
    assert tw2.means(th2)[0, 0] < mock.MAX_MEAN
    assert tw2._band.means(th2)[0, 0] > mock.MAX_MEAN
    with pytest.raises(mock.MockError, match=r'row 0 field 0: .*\(piece "below"\)'):
        tw2.hist_cut(th2, np.linspace(40.0, 44.0, 5), 1)
    tw.set_error_model(nodes, sig)                                               # a new error model clears the band
    with pytest.raises(mock.MockError, match="no cut band"):
        tw.draw_cut(th, 1)


def test_surface():
    from lumfuncmcmc_amd import build, capi
    build.build_library(verbose=False)
    lib = capi.load()
    hdr = open(os.path.join(ROOT, "include", "lfmcmc.h")).read()
    assert "#define LF_ABI_VERSION 3" in hdr
    decl = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for n in ("lf_mock_set_cut_band", "lf_mock_draw_cut", "lf_mock_hist_cut"):
        assert n in decl and n in capi.EXPORTS and hasattr(lib, n)
    assert lib.lf_mock_set_cut_band(None, None, None) == -1
    assert lib.lf_mock_hist_cut(None, None, 1, None, 0, 1, None, None, None) == -1
    src = open(os.path.join(ROOT, "lumfuncmcmc_amd", "csrc", "lf_mock_cut.h")).read()
    assert re.search(r"MOCK_CUT_BAND = 4u << 8;", src) and mock.CUT_BAND == 4 << 8
    assert mock.cut_depth(np.array([[0.1, 0.2]])) == deconv.CUT_T * 0.2


def test_the_kernels_use_no_scratch_and_spill_nothing():
    import lf_isalib
    rem = lf_isalib.remarks()
    for name in ("lf_mock_draw_cut", "lf_mock_hist_cut", "lf_mock_count_cut"):
        hits = [v for k, v in rem.items() if re.match(r"_ZN2lf\d+%sE" % name, k)]
        assert len(hits) == 1, name
        print(name, hits[0])
        assert hits[0]["ScratchSize"] == 0 and hits[0]["VGPRs Spill"] == 0 and hits[0]["SGPRs Spill"] == 0, hits[0]
    old = [v for k, v in rem.items() if re.match(r"_ZN2lf\d+lf_mock_hist_errE", k)][0]
    new = [v for k, v in rem.items() if re.match(r"_ZN2lf\d+lf_mock_hist_cutE", k)][0]
    assert new["LDS Size"] <= old["LDS Size"] + 16
