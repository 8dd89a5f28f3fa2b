"""The mocks binned in redshift and luminosity, host side (mock.bin_sources2, MockTwin.hist2*, mock.predictive2, mock.deviance,
posterior_predictive(z_edges=...)).  No GPU: the slots' definition against np.searchsorted on values
at, just below and just above the edges; the twin's histograms against the binning of its own draws and against its 1-D
histograms; predictive2's marginal against predictive; the deviance against a hand computation; the model class on the twin
path; the wrappers' refusals, which come before any library call."""
import re

import numpy as np
import pytest

import lf_mockcutlib as K
import lf_mockproblib as M
from lumfuncmcmc_amd import mock

SEED = 1234
RID = np.array([100, 1 << 40, 7], dtype=np.int64)
VARIANTS = ("free", "fixcomp", "zevol")


def _loop(z, L, off, ze, e):
    out = np.zeros((len(off) - 1, len(ze) + 1, len(e) + 1), dtype=np.int64)
    for s in range(len(off) - 1):
        for i in range(off[s], off[s + 1]):
            out[s, np.searchsorted(ze, z[i], side="right"), np.searchsorted(e, L[i], side="right")] += 1
    return out


def test_bin_sources2_is_searchsorted_right_on_both_axes_at_the_edges():
    ze = np.array([0.5, 1.0, 1.0, 1.5, 2.0])                    # a repeated edge: slot 2 is empty
    e = np.array([41.0, 42.0, 42.0, 42.0, 43.5])               # two empty slots
    around = lambda v: np.concatenate([v, np.nextafter(v, -np.inf), np.nextafter(v, np.inf)])      # noqa: E731
    zs, Ls = around(ze), around(e)
    z, L = (a.ravel() for a in np.meshgrid(zs, Ls, indexing="ij"))
    off = np.array([0, 0, 70, 71, z.size, z.size], dtype=np.int64)      # empty segments first, last and in between sizes
    got = mock.bin_sources2(z, L, off, ze, e)
    assert got.shape == (5, 6, 6) and got.dtype == np.int64
    np.testing.assert_array_equal(got, _loop(z, L, off, ze, e))
    assert got.sum() == z.size and not got[:, 2].any() and not got[:, :, 2].any() and not got[:, :, 3].any()
    # a value on an edge lands in the upper slot
    one = mock.bin_sources2(np.array([1.5]), np.array([43.5]), np.array([0, 1]), ze, e)
    assert one[0, 4, 5] == 1
    np.testing.assert_array_equal(got.sum(axis=1), mock.bin_sources(L, off, e))
    np.testing.assert_array_equal(got.sum(axis=2), mock.bin_sources(z, off, ze))


def _grids(z, L):
    ze = np.linspace(z.min() + 0.02, z.max() - 0.02, 6)
    e = np.linspace(L.min() + 0.1, L.max() - 0.3, 9)
    return ze, e


@pytest.mark.parametrize("variant", VARIANTS)
def test_twin_hist2_plain_and_noisy(variant):
    inp = M.edge_inputs(variant, 257)
    tw = mock.MockTwin(inp)
    th = M.scaled_rows(tw, variant, (3000.0, 300.0, 5.0))
    tw.set_error_model(np.array([-17.0, -16.0]), np.array([[0.05, 0.3], [0.0, 0.1]]))
    z, L, Lobs, sg, fld, off = tw.draw_noisy(th, SEED, RID)
    ze, e = _grids(z, L)
    cnt = tw.counts(th, SEED, RID)[1]
    for got, lum, one in ((tw.hist2(th, ze, e, SEED, RID), L, tw.hist(th, e, SEED, RID)),
                          (tw.hist2_noisy(th, ze, e, SEED, RID), Lobs, tw.hist_noisy(th, e, SEED, RID))):
        assert got.shape == (3, tw.nf, 7, 10)
        np.testing.assert_array_equal(got, mock.bin_sources2(z, lum, off, ze, e).reshape(got.shape))
        np.testing.assert_array_equal(got.sum(axis=2), one)
        np.testing.assert_array_equal(got.sum(axis=(2, 3)), cnt)
        assert got[:, :, 0].sum() > 0 and got[:, :, -1].sum() > 0 and got[..., 0].sum() > 0 and got[..., -1].sum() > 0
    # an explicit count gives the leading sources of the same streams
    few = np.array([[3, 0], [0, 5], [2, 2]], dtype=np.int64)
    zf, Lf, ff, of = tw.draw(th, SEED, RID, few)
    np.testing.assert_array_equal(tw.hist2(th, ze, e, SEED, RID, count=few), mock.bin_sources2(zf, Lf, of, ze, e).reshape(3, tw.nf, 7, 10))
    assert tw.hist2_noisy(th, ze, e, SEED, RID, count=few).sum() == few.sum()


@pytest.mark.parametrize("variant", VARIANTS)
def test_twin_hist2_cut(variant):
    inp = K.inputs(variant, 23)
    tw = K.arm(mock.MockTwin(inp), inp, *K.table(7))
    th = K.rows_for_means(tw, variant, False, (3000.0, 300.0, 0.0), 0)
    z, L, Lobs, sg, fld, off, info = tw.draw_cut(th, SEED, RID)
    ze, e = _grids(z, Lobs)
    got, kept = tw.hist2_cut(th, ze, e, SEED, RID)
    np.testing.assert_array_equal(got, mock.bin_sources2(z, Lobs, off, ze, e).reshape(got.shape))
    one, kept1 = tw.hist_cut(th, e, SEED, RID)
    np.testing.assert_array_equal(got.sum(axis=2), one)
    np.testing.assert_array_equal(kept, kept1)
    np.testing.assert_array_equal(got.sum(axis=(2, 3)), kept)
    assert kept.sum() > 1000 and info["n_scattered_in"].sum() > 0 and not got[2].any()


@pytest.mark.parametrize("process", ["plain", "noisy", "cut"])
def test_predictive2_marginal_is_predictive(process):
    inp = K.inputs("zevol", 23)
    tw = K.arm(mock.MockTwin(inp), inp, *K.table(7))
    th = K.rows_for_means(tw, "zevol", False, (600.0,) * 6, 0)
    th[:, 3:6] += np.linspace(-0.05, 0.05, 6)[:, None]
    z, L, Lobs, sg, fld, off, info = tw.draw_cut(th[:1] + 0.01, 99)
    fi = off.copy()
    e = np.linspace(Lobs.min() + 0.05, Lobs.max() - 0.2, 8)
    ze = np.linspace(z.min(), z.max(), 5)
    kw = dict(noisy=process != "plain", cut=process == "cut")
    old = mock.predictive(tw, th, e, Lobs, fi, 31, **kw)
    new = mock.predictive2(tw, th, ze, e, z, Lobs, fi, 31, **kw)
    for k, v in old.items():
        assert np.array_equal(new[k], v), k
    nf, R = tw.nf, 6
    assert new["observed_2d"].shape == (nf, 6, 9) and new["replicated_2d"].shape == (R, nf, 6, 9)
    assert new["percentiles_2d"].shape == (3, nf, 6, 9) and new["p_upper_2d"].shape == new["p_lower_2d"].shape == (nf, 6, 9)
    assert new["observed_z"].shape == (nf, 6) and new["replicated_z"].shape == (R, nf, 6)
    assert new["percentiles_z"].shape == (3, nf, 6) and new["p_upper_z"].shape == new["p_lower_z"].shape == (nf, 6)
    np.testing.assert_array_equal(new["replicated_2d"].sum(axis=2), old["replicated"])
    np.testing.assert_array_equal(new["replicated_2d"].sum(axis=3), new["replicated_z"])
    np.testing.assert_array_equal(new["observed_2d"].sum(axis=2), new["observed_z"])
    np.testing.assert_array_equal(new["observed_z"].sum(axis=1), np.diff(fi))
    for k in ("deviance", "p_deviance", "n_empty_cells", "observed_in_empty"):
        assert new[k].shape == (nf,), k
    assert new["replicated_deviance"].shape == (R, nf)
    np.testing.assert_array_equal(new["p_deviance"], np.mean(new["replicated_deviance"] >= new["deviance"][None], axis=0))
    assert new["z_edges"].tobytes() == ze.tobytes()
    assert sorted(set(new) - set(old)) == sorted(
        ["z_edges", "observed_2d", "replicated_2d", "percentiles_2d", "p_upper_2d", "p_lower_2d", "observed_z", "replicated_z",
         "percentiles_z", "p_upper_z", "p_lower_z", "deviance", "replicated_deviance", "p_deviance", "n_empty_cells",
         "observed_in_empty"])


def test_deviance_by_hand_on_a_2x2_example_with_an_empty_cell():
    # one field, cells (a, b; c, d); replicate means m = (2, 1, 3, 0): cell d is never filled by a replicate
    rep = np.array([[[[1, 0], [4, 0]]], [[[3, 2], [2, 0]]]], dtype=np.int64)
    obs = np.array([[[2, 0], [5, 1]]], dtype=np.int64)                      # one observed source sits in the empty cell
    d, dr, p, n_empty, in_empty = mock.deviance(obs, rep)
    term = lambda h, m: m - h + (h * np.log(h / m) if h > 0 else 0.0)       # noqa: E731
    want = 2.0 * (term(2, 2.0) + term(0, 1.0) + term(5, 3.0))
    want_r = [2.0 * (term(1, 2.0) + term(0, 1.0) + term(4, 3.0)), 2.0 * (term(3, 2.0) + term(2, 1.0) + term(2, 3.0))]
    np.testing.assert_allclose(d, [want], rtol=1e-14)
    np.testing.assert_allclose(dr[:, 0], want_r, rtol=1e-14)
    assert want == pytest.approx(2.0 * (1.0 + (-2.0 + 5.0 * np.log(5.0 / 3.0))))
    assert n_empty.tolist() == [1] and in_empty.tolist() == [1]
    assert p.tolist() == [np.mean(np.array(want_r) >= want)]
    # h = m everywhere: no deviance
    same = np.array([[[[2, 1], [3, 0]]]] * 3)
    assert mock.deviance(same[0], same)[0].tolist() == [0.0]


def test_the_model_class_without_and_with_z_edges():
    from lf_deconvlib import fixcomp_model
    from lumfuncmcmc_amd import synth
    cat = synth.catalogue(400, seed=17)
    o = fixcomp_model(cat)
    theta = np.array([synth.LSTAR, synth.PHISTAR - 1.0, synth.SCH_AL])
    rng = np.random.default_rng(6)
    rows = theta[None] + rng.normal(0.0, 0.02, (50, 3))
    o.samples = np.concatenate([rows, -0.5 * rng.chisquare(3, 50)[:, None]], axis=1)
    kw = dict(ndraws=8, seed=31, device=False)
    np.random.seed(5)
    plain = o.posterior_predictive(**kw)
    np.random.seed(5)
    none = o.posterior_predictive(z_edges=None, **kw)
    np.random.seed(5)
    prows = o._posterior_rows(8, 7.5)[:, :-1]
    fi = np.asarray(o.field_ind, dtype=np.int64)
    edges = np.linspace(np.min(o.lum), np.max(o.lum), 21)
    old = mock.predictive(mock.MockTwin(o.kernel_inputs()), prows, edges, o.lum, fi, 31)
    assert sorted(plain) == sorted(none) == sorted(list(old) + ["noise", "sigma_model"])
    for k, v in old.items():
        assert np.array_equal(plain[k], v) and np.array_equal(none[k], v), k
    np.random.seed(5)
    auto = o.posterior_predictive(z_edges="auto", **kw)
    nf = o.nfields
    assert auto["z_edges"].tobytes() == np.linspace(o.zmin, o.zmax, 11).tobytes()
    for k, v in old.items():
        assert np.array_equal(auto[k], v), k
    assert auto["observed_2d"].shape == (nf, 12, 22) and auto["replicated_2d"].shape == (8, nf, 12, 22)
    assert auto["percentiles_2d"].shape == (3, nf, 12, 22) and auto["p_upper_2d"].shape == auto["p_lower_2d"].shape == (nf, 12, 22)
    assert auto["observed_z"].shape == auto["p_upper_z"].shape == auto["p_lower_z"].shape == (nf, 12)
    assert auto["replicated_z"].shape == (8, nf, 12) and auto["replicated_deviance"].shape == (8, nf)
    for k in ("deviance", "p_deviance", "n_empty_cells", "observed_in_empty"):
        assert auto[k].shape == (nf,), k
    # every observed source is inside [zmin, zmax]: slot 0 is empty and zmax itself sits in the last slot
    assert not auto["observed_z"][:, 0].any() and auto["observed_z"][:, -1].sum() == 1
    assert auto["observed_2d"].sum() == len(o.lum) and auto["noise"] is None
    np.random.seed(5)
    arr = o.posterior_predictive(z_edges=[1.9, 2.5, 3.5], **kw)
    assert arr["observed_2d"].shape == (nf, 4, 22)
    np.testing.assert_array_equal(arr["replicated"], old["replicated"])
    with pytest.raises(ValueError, match="z_edges"):
        o.posterior_predictive(z_edges="equal", **kw)


def test_the_wrappers_refuse_a_bad_grid_before_any_library_call():
    """a MockGenerator without a library behind it: a call that reached the library would fail with AttributeError"""
    gen = object.__new__(mock.MockGenerator)
    gen._lib = gen._h = None
    gen.nf, gen.ndim, gen._band_set = 2, 3, True
    tw = mock.MockTwin(M.edge_inputs("fixcomp", 257))
    th = np.zeros((1, 3))
    ok = np.linspace(0.0, 1.0, 5)
    cases = [(np.linspace(0, 1, mock.MAX_BINS + 2), ok, "z_edges must hold 2 .. 1023 values"),
             (ok, np.linspace(0, 1, mock.MAX_BINS + 2), "edges must hold 2 .. 1023 values"),
             (np.array([0.5]), ok, "z_edges must hold"),
             (np.array([0.0, np.nan, 1.0]), ok, "z_edges must be finite and non-decreasing"),
             (ok[::-1], ok, "z_edges must be finite and non-decreasing"),
             (ok, np.array([0.0, np.inf]), "edges must be finite and non-decreasing"),
             (ok, ok[::-1], "edges must be finite and non-decreasing")]
    for ze, e, msg in cases:
        for obj in (gen, tw):
            for name in ("hist2", "hist2_noisy", "hist2_cut"):
                with pytest.raises(ValueError, match=re.escape(msg)):
                    getattr(obj, name)(th, ze, e, 1)
    # the slot limit: 64 x 128 = 8192 passes the check (and then fails at the absent library), 64 x 129 does not
    over = (np.linspace(0, 1, 63), np.linspace(0, 1, 128))
    for obj in (gen, tw):
        with pytest.raises(ValueError, match=re.escape("(nz + 2) * (nl + 2) = 8256 slots: the limit is 8192")):
            obj.hist2(th, *over, 1)
    with pytest.raises(AttributeError):
        gen.hist2(th, np.linspace(0, 1, 63), np.linspace(0, 1, 127), 1)
    ze, e = mock._edges2(np.linspace(0, 1, 63), np.linspace(0, 1, 127))
    assert (ze.size + 1) * (e.size + 1) == mock.MAX_SLOTS2


def test_the_constants_mirror_the_headers():
    import os
    csrc = os.path.join(os.path.dirname(os.path.abspath(mock.__file__)), "csrc")
    h1, h2 = open(os.path.join(csrc, "lf_mock.h")).read(), open(os.path.join(csrc, "lf_mock_hist2.h")).read()
    threads = int(re.search(r"MOCK_THREADS = (\d+);", h1).group(1))
    items = int(re.search(r"MOCK_HIST_ITEMS = (\d+);", h1).group(1))
    assert mock.HIST_CHUNK == threads * items
    assert mock.MAX_SLOTS2 == int(re.search(r"MOCK_HIST2_MAX_SLOTS = (\d+);", h2).group(1))
    from lumfuncmcmc_amd import capi
    header = open(os.path.join(os.path.dirname(csrc), "..", "include", "lfmcmc.h")).read()
    for n in capi.EXPORTS_HIST2:
        assert re.search(r"\b%s\(" % n, header), n
