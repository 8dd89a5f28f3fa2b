"""Mock catalogues, host side (lumfuncmcmc_amd/mock.py, csrc/lf_mock.h): the NumPy twin's expected
counts are piece B of lnprob, its Poisson draws follow the exact pmf, its sources follow the exact cell integrals of the
interpolated intensity, a row's catalogue does not depend on its batch, and the new C entry points and kernels are
declared, exported and free of scratch.  No GPU."""
import math
import os
import re

import numpy as np
import pytest

import lf_isalib
import lf_mockproblib
import lf_oracle as O
import lf_testlib as T
from lumfuncmcmc_amd import mock, synth

stats = pytest.importorskip("scipy.stats")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lfmcmc.h")
NEW_ENTRIES = ("lf_mock_create", "lf_mock_destroy", "lf_mock_counts", "lf_mock_draw", "lf_mock_hist", "lf_mock_last_error")


def _class_inputs(variant, fix_sch_al=False, n=3000):
    """kernel_inputs() of a model object built with min_comp_frac = 0.5: every redshift column has its own luminosity nodes."""
    from lumfuncmcmc_amd.model import LumFuncMCMC, LumFuncMCMCz
    cat = synth.catalogue(n, seed=4)
    fi = cat["field_ind"]
    kw = dict(lum=synth.split_fields(cat["lum"], fi), lum_e=synth.split_fields(cat["lum_e"], fi), Flim=list(synth.FLIM),
              alpha=synth.ALPHA_C, Omega_0=list(synth.OMEGA_0), sch_al=synth.SCH_AL, Lc=synth.LC, Lh=synth.LH, nwalkers=16,
              nsteps=4, min_comp_frac=0.5, field_ind=fi, fix_sch_al=fix_sch_al)
    zs = synth.split_fields(cat["z"], fi)
    np.random.seed(3)
    if variant == "zevol":
        m = LumFuncMCMCz(zs, **kw)
    else:
        m = LumFuncMCMC(zs, fix_comp=(variant == "fixcomp"), Flim_lims=synth.FLIM_LIMS, alpha_lims=synth.ALPHA_LIMS, **kw)
    inp = m.kernel_inputs()
    inp["lims"] = {k: list(v) for k, v in inp["lims"].items()}
    assert not np.all(inp["logL"] == inp["logL"][:, :1])           # the columns' luminosity nodes differ
    return inp


@pytest.mark.parametrize("grid", ["rect", "class"])
@pytest.mark.parametrize("fix_sch_al", [False, True])
@pytest.mark.parametrize("variant", ["free", "fixcomp", "zevol"])
def test_expected_counts_are_piece_b(variant, fix_sch_al, grid):
    inp = T.make_inputs(variant, 2000, fix_sch_al=fix_sch_al) if grid == "rect" else _class_inputs(variant, fix_sch_al)
    tw = mock.MockTwin(inp)
    th = synth.walkers(variant, 6, seed=11, fix_sch_al=fix_sch_al)
    mean, cnt = tw.counts(th, seed=5)
    assert mean.shape == cnt.shape == (6, 5) and cnt.dtype == np.int64
    pb = np.array([O.piece_b(inp, O.split_theta(inp, t)) for t in th])
    np.testing.assert_allclose(mean.sum(axis=1), pb, rtol=1e-13, atol=0)
    assert (mean >= 0).all() and (cnt >= 0).all()


@pytest.mark.parametrize("mu", [1e-3, 0.5, 5.0, 9.99, 10.0, 37.0, 1e4, 1e6])
def test_poisson_draws_follow_the_exact_pmf(mu):
    n = 40000
    k = mock.poisson(np.full(n, mu), np.arange(n, dtype=np.int64), 3, seed=20260101)
    assert k.dtype == np.int64 and (k >= 0).all()
    # chi^2 against the exact pmf, classes merged to >= 5 expected draws, p > 1e-4 (mu = 1e-3: the count of non-zero draws)
    lf_mockproblib.poisson_fit(k, mu)


def test_poisson_special_means():
    rid = np.arange(4, dtype=np.int64)
    assert (mock.poisson(np.zeros(4), rid, 0, 1) == 0).all()
    got = mock.poisson(np.array([np.nan, -1.0, np.inf, 2.0 ** 31 * 1.5]), rid, 0, 1)
    assert (got == -1).all()
    assert mock.loggam(np.array([1.0, 2.0]))[0] == 0.0
    x = np.array([3.0, 6.5, 7.0, 30.0, 1e6])
    np.testing.assert_allclose(mock.loggam(x), [math.lgamma(v) for v in x], rtol=1e-13)


def _hat_int(x, i, lo, hi):
    """Exact integral over [lo, hi] of the unit hat at node i of the nodes x."""
    out = 0.0
    if i > 0:                                               # rising side on [x[i-1], x[i]]
        a, b = max(lo, x[i - 1]), min(hi, x[i])
        if b > a:
            d = x[i] - x[i - 1]
            out += ((b - x[i - 1]) ** 2 - (a - x[i - 1]) ** 2) / (2 * d)
    if i < len(x) - 1:                                      # falling side on [x[i], x[i+1]]
        a, b = max(lo, x[i]), min(hi, x[i + 1])
        if b > a:
            d = x[i + 1] - x[i]
            out += ((x[i + 1] - a) ** 2 - (x[i + 1] - b) ** 2) / (2 * d)
    return out


def test_sources_follow_the_exact_cell_integrals():
    S, n = 11, 1000000
    inp = T.make_inputs("zevol", 500, S=S)
    tw = mock.MockTwin(inp)
    th = np.array([42.3, 42.6, 42.1, -2.2, -2.6, -2.4, -1.3])
    f = 2
    z, L = tw.sources(th, 17, f, seed=99, index=np.arange(n))
    zn, Ln = tw.zarr, tw.logL[:, 0]
    ze = np.sort(np.concatenate([zn, 0.5 * (zn[1:] + zn[:-1])]))      # every interval split in two: the hats' shape shows
    Le = np.sort(np.concatenate([Ln, 0.5 * (Ln[1:] + Ln[:-1])]))
    lam = tw.lam(th)[f]
    Iz = np.array([[_hat_int(zn, k, ze[c], ze[c + 1]) for c in range(len(ze) - 1)] for k in range(S)])    # [node][cell]
    IL = np.array([[_hat_int(Ln, j, Le[c], Le[c + 1]) for c in range(len(Le) - 1)] for j in range(S)])
    cell = IL.T @ lam @ Iz                                   # [L cell][z cell]
    expect = n * cell / cell.sum()
    obs, _, _ = np.histogram2d(L, z, bins=[Le, ze])
    assert obs.sum() == n
    use = expect >= 5.0
    assert obs[~use].sum() <= max(50.0, 5 * expect[~use].sum() + 25)
    chi2 = float(((obs[use] - expect[use]) ** 2 / expect[use]).sum())
    assert stats.chi2.sf(chi2, int(use.sum()) - 1) > 1e-4, (chi2, int(use.sum()))


@pytest.mark.parametrize("variant", ["free", "zevol"])
def test_a_rows_catalogue_does_not_depend_on_its_batch(variant):
    inp = T.make_inputs(variant, 500, S=31)
    tw = mock.MockTwin(inp)
    th = synth.walkers(variant, 5, seed=2)
    if variant == "free":
        th[:, 1] = -4.0                                       # keep the twin's catalogues small
    else:
        th[:, 3:6] = -4.0
    rid = np.array([7, 1 << 40, 3, 12345678901, 0], dtype=np.int64)
    alone = [tw.draw(th[i:i + 1], 42, row_ids=rid[i:i + 1]) for i in range(5)]
    perm = np.array([3, 0, 4, 2, 1])
    z, L, fld, off = tw.draw(th[perm], 42, row_ids=rid[perm])
    nf = tw.nf
    for pos, i in enumerate(perm):
        a = alone[i]
        lo, hi = off[pos * nf], off[(pos + 1) * nf]
        np.testing.assert_array_equal(z[lo:hi], a[0])
        np.testing.assert_array_equal(L[lo:hi], a[1])
        np.testing.assert_array_equal(fld[lo:hi], a[2])
    other = tw.draw(th[:1], 43, row_ids=rid[:1])
    assert other[0].size != alone[0][0].size or not np.array_equal(other[0], alone[0][0])


def test_hist_is_the_binning_of_the_draw():
    inp = T.make_inputs("fixcomp", 500, S=21)
    tw = mock.MockTwin(inp)
    th = synth.walkers("fixcomp", 3, seed=8)
    th[:, 1] = -3.5
    edges = np.linspace(41.5, 43.5, 9)
    h = tw.hist(th, edges, seed=3)
    z, L, fld, off = tw.draw(th, seed=3)
    assert h.shape == (3, 5, 10)
    want = np.array([np.bincount(np.searchsorted(edges, L[off[i]:off[i + 1]], side="right"), minlength=10) for i in range(15)])
    np.testing.assert_array_equal(h.reshape(15, 10), want)
    assert h[..., 0].sum() + h[..., -1].sum() > 0                # both overflow slots see sources here


def test_twin_refuses_what_the_library_refuses():
    inp = T.make_inputs("fixcomp", 100, S=11)
    tw = mock.MockTwin(inp)
    th = synth.walkers("fixcomp", 2, seed=1)
    th[1, 0] = np.nan
    with pytest.raises(mock.MockError, match="row 1"):
        tw.counts(th, 1)
    th = synth.walkers("fixcomp", 2, seed=1)
    th[0, 1] = 30.0                                            # phi* = 10^30: the expected count overflows the cap
    with pytest.raises(mock.MockError, match="row 0 field 0"):
        tw.counts(th, 1)
    with pytest.raises(ValueError):
        tw.hist(synth.walkers("fixcomp", 1, seed=1), np.linspace(0, 1, mock.MAX_BINS + 2), 1)


def test_header_declares_and_capi_exports_the_new_entries():
    from lumfuncmcmc_amd import build, capi
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(lf_[a-z_]+)\s*\(", src))
    for name in NEW_ENTRIES:
        assert name in declared and name in capi.EXPORTS, name
    assert "lf_mock.h" in " ".join(build.HEADERS)
    assert "typedef struct lf_mock lf_mock;" in src


@pytest.fixture(scope="module")
def remarks():
    return lf_isalib.remarks()


@pytest.mark.parametrize("kernel,lds", [("lf_mock_mass", 2048), ("lf_mock_total", 2048), ("lf_mock_draw", 0),
                                        ("lf_mock_hist", 12 * 1024)])
def test_mock_kernels_use_no_scratch_and_the_stated_lds(remarks, kernel, lds):
    hits = {k: v for k, v in remarks.items() if k.startswith("_ZN2lf%d%s" % (len(kernel), kernel))}
    assert len(hits) == 1, sorted(remarks)
    for name, r in hits.items():
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, (name, r)
        assert r["LDS Size"] == lds, (name, r)
