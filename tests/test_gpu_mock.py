"""Mock catalogues on the device (lf_mock_*, csrc/lf_mock.h): parity with the NumPy twin for every
variant, the expected counts against the context's piece B, batch independence bit for bit, the histogram kernel against
the binning of the draw, the marginals of a 10^6-source mock, parameter recovery and the posterior predictive check
through the model class, and every LF_ERR_ARG case."""
import ctypes

import numpy as np
import pytest

import lf_testlib as T
from lumfuncmcmc_amd import capi, mock, synth

pytestmark = pytest.mark.gpu
stats = pytest.importorskip("scipy.stats")

TARGETS = (3.0e4, 5000.0, 400.0, 30.0, 6.0, 1.5, 0.2)      # expected sources per row; the eighth row has mean 0


def _class_inputs(variant, fix_sch_al):
    from lumfuncmcmc_amd.model import LumFuncMCMC, LumFuncMCMCz
    cat = synth.catalogue(3000, seed=4)
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
    return m.kernel_inputs()


def _scaled_rows(tw, variant, fix_sch_al, seed=5):
    """Eight rows of the prior box, phi* shifted so that their expected totals are TARGETS; the last row has L* so far
    below the grid that every node underflows (mean exactly 0)."""
    th = synth.walkers(variant, 8, seed=seed, fix_sch_al=fix_sch_al)
    phi = [3, 4, 5] if variant == "zevol" else [1]
    mean = tw.means(th).sum(axis=1)
    for i, t in enumerate(TARGETS):
        th[i, phi] += np.log10(t / mean[i])
    th[7, [0, 1, 2] if variant == "zevol" else [0]] = 20.0
    return th


@pytest.mark.parametrize("grid", ["rect", "class"])
@pytest.mark.parametrize("fix_sch_al", [False, True])
@pytest.mark.parametrize("variant", ["free", "fixcomp", "zevol"])
def test_device_matches_the_twin(variant, fix_sch_al, grid):
    inp = T.make_inputs(variant, 1000, fix_sch_al=fix_sch_al) if grid == "rect" else _class_inputs(variant, fix_sch_al)
    tw, gen = mock.MockTwin(inp), mock.MockGenerator(inp)
    th = _scaled_rows(tw, variant, fix_sch_al)
    rid = np.arange(100, 108, dtype=np.int64)
    m_d, n_d = gen.counts(th, 1234, rid)
    m_h, n_h = tw.counts(th, 1234, rid)
    np.testing.assert_allclose(m_d, m_h, rtol=1e-12, atol=0)
    np.testing.assert_array_equal(n_d, n_h)
    assert (m_d[7] == 0).all() and (n_d[7] == 0).all()
    assert (m_d.sum(axis=1)[4:7] < 10).all()
    zd, Ld, fd, od = gen.draw(th, 1234, rid)
    zh, Lh, fh, oh = tw.draw(th, 1234, rid)
    np.testing.assert_array_equal(od, oh)
    np.testing.assert_array_equal(fd, fh)
    np.testing.assert_allclose(zd, zh, rtol=0, atol=1e-12)
    np.testing.assert_allclose(Ld, Lh, rtol=0, atol=1e-12)
    # Sigma_f M_f is piece B of the context's lnprob for the same rows (rows inside the prior box)
    ctx = capi.LFContext(inp)
    try:
        _, pb = ctx.lnprob_pieces(th[:7])
    finally:
        ctx.close()
    ok = np.isfinite(pb)                                      # (rows whose shifted phi* left the prior box give NaN)
    assert ok.sum() >= 3
    np.testing.assert_allclose(m_d.sum(axis=1)[:7][ok], pb[ok], rtol=1e-12, atol=0)
    gen.close()


def test_a_row_does_not_depend_on_its_batch():
    inp = T.make_inputs("zevol", 1000)
    gen = mock.MockGenerator(inp)
    rng = np.random.default_rng(3)
    th = synth.walkers("zevol", 64, seed=9)
    th[:, 3:6] = rng.uniform(-6.5, -5.5, (64, 3))
    rid = rng.integers(0, 1 << 62, 64)
    big = gen.draw(th, 77, rid)
    means = gen.counts(th, 77, rid)[0]
    nf = gen.nf
    for i in (0, 37, 63):
        one = gen.draw(th[i:i + 1], 77, rid[i:i + 1])
        lo, hi = big[3][i * nf], big[3][(i + 1) * nf]
        for a, b in zip(one[:3], big[:3]):
            assert a.tobytes() == b[lo:hi].tobytes()
        assert gen.counts(th[i:i + 1], 77, rid[i:i + 1])[0].tobytes() == means[i:i + 1].tobytes()
    # the same row at another position of a shuffled batch
    perm = rng.permutation(64)
    sh = gen.draw(th[perm], 77, rid[perm])
    p = int(np.flatnonzero(perm == 37)[0])
    lo, hi = sh[3][p * nf], sh[3][(p + 1) * nf]
    lo0, hi0 = big[3][37 * nf], big[3][38 * nf]
    assert sh[1][lo:hi].tobytes() == big[1][lo0:hi0].tobytes()
    gen.close()


def test_hist_is_the_binning_of_the_draw():
    inp = T.make_inputs("free", 1000)
    tw, gen = mock.MockTwin(inp), mock.MockGenerator(inp)
    th = _scaled_rows(tw, "free", False)
    edges = np.concatenate([np.linspace(41.6, 43.0, 37), [43.0, 43.4]])        # a zero-width bin too
    h = gen.hist(th, edges, 5)
    z, L, fld, off = gen.draw(th, 5)
    want = mock.bin_sources(L, off, edges).reshape(h.shape)
    np.testing.assert_array_equal(h, want)
    assert h[..., 0].sum() > 0 and h[..., -1].sum() > 0
    np.testing.assert_array_equal(h.sum(axis=2), gen.counts(th, 5)[1])
    gen.close()


def _hat_cdf(x, nodes):
    """[len(x), len(nodes)]: integral up to x of every unit hat on `nodes`."""
    x = np.asarray(x)[:, None]
    n = nodes
    out = np.zeros((x.shape[0], n.size))
    dl = np.concatenate([[0.0], np.diff(n)])
    dr = np.concatenate([np.diff(n), [0.0]])
    with np.errstate(all="ignore"):
        left = np.where(dl > 0, np.clip(x - (n - dl), 0, dl) ** 2 / (2 * dl), 0.0)
        t = np.clip(x - n, 0, dr)
        right = np.where(dr > 0, t - t ** 2 / (2 * dr), 0.0)
    out = left + right
    return out


def test_a_million_source_mock_has_the_exact_marginals():
    inp = T.make_inputs("zevol", 2000, nf=1)
    tw, gen = mock.MockTwin(inp), mock.MockGenerator(inp)
    th = np.array([[42.4, 42.7, 42.2, -2.3, -2.7, -2.5, -1.4]])
    th[0, 3:6] += np.log10(1.0e6 / tw.means(th).sum())
    z, L, fld, off = gen.draw(th, 2026)
    n = z.size
    assert abs(n - 1.0e6) < 6000
    lam = tw.lam(th[0])[0]                                    # [j][k], every column on the same L nodes here
    Ln, zn = tw.logL[:, 0], tw.zarr
    wz, wL = mock.trapz_weights(zn), tw.wL[:, 0]
    Az = (wL[:, None] * lam).sum(axis=0)                      # the z marginal: sum_k Az[k] hat_k(z)
    AL = (lam * wz[None, :]).sum(axis=1)                      # the L marginal: sum_j AL[j] hat_j(L)
    for x, nodes, A, w in ((z, zn, Az, wz), (L, Ln, AL, wL)):
        pts = np.sort(np.concatenate([nodes, np.quantile(x, np.linspace(0.0005, 0.9995, 2000))]))
        F = _hat_cdf(pts, nodes) @ A / (A @ w)
        emp = np.searchsorted(np.sort(x), pts, side="right") / n
        D = np.max(np.abs(emp - F))
        assert D < 1.95 / np.sqrt(n), D                      # KS at p = 0.001 (D over a subset of points <= the KS D)
    gen.close()


def _fixcomp_model(cat_lists, **extra):
    from lumfuncmcmc_amd.model import LumFuncMCMC
    kw = dict(Flim=list(synth.FLIM), alpha=synth.ALPHA_C, Omega_0=list(synth.OMEGA_0), sch_al=synth.SCH_AL,
              sch_al_lims=synth.SCH_AL_LIMS, Lstar=synth.LSTAR, Lstar_lims=synth.LSTAR_LIMS, phistar=synth.PHISTAR,
              phistar_lims=synth.PHISTAR_LIMS, Lc=synth.LC, Lh=synth.LH, min_comp_frac=0.0, Flim_lims=synth.FLIM_LIMS,
              alpha_lims=synth.ALPHA_LIMS, fix_comp=True)
    kw.update(extra)
    return LumFuncMCMC(cat_lists["z"], lum=cat_lists["lum"], lum_e=cat_lists["lum_e"], field_ind=cat_lists["field_ind"], **kw)


def test_parameter_recovery_and_the_posterior_predictive_check():
    cat = synth.catalogue(5000, seed=21)
    fi = cat["field_ind"]
    base = _fixcomp_model({"z": synth.split_fields(cat["z"], fi), "lum": synth.split_fields(cat["lum"], fi),
                           "lum_e": synth.split_fields(cat["lum_e"], fi), "field_ind": fi}, nwalkers=32, nsteps=10)
    theta = np.array([42.6, -2.0, -1.5])
    m0 = base._mock_generator(True).counts(theta[None], 0)[0].sum()
    theta[1] += np.log10(2.0e4 / m0)
    mc = base.mock_catalogue(theta, seed=8080, device=True)
    assert mc["seed"] == 8080 and np.array_equal(mc["theta"], theta)
    n = int(mc["field_ind"][-1])
    assert abs(n - 2.0e4) < 5 * np.sqrt(2.0e4)
    assert [len(a) for a in mc["z"]] == list(np.diff(mc["field_ind"]))
    assert all((e == 0).all() for e in mc["lum_e"])
    again = base.mock_catalogue(theta, seed=8080, device=True)
    assert all(np.array_equal(a, b) for a, b in zip(mc["lum"], again["lum"]))
    host = base.mock_catalogue(theta, seed=8080, device=False)
    for a, b in zip(mc["lum"], host["lum"]):
        np.testing.assert_allclose(a, b, rtol=0, atol=1e-12)
    base.close()

    fit = _fixcomp_model(mc, nwalkers=64, nsteps=800)
    np.random.seed(123)
    fit.fit_model()
    s = fit.samples[:, :-1]
    med, sd = np.median(s, axis=0), np.std(s, axis=0)
    assert np.all(np.abs(med - theta) < 4 * sd), (med, sd, theta)

    np.random.seed(5)
    pp = fit.posterior_predictive(ndraws=100, seed=31)
    B = 20
    assert pp["edges"].shape == (B + 1,)
    assert pp["observed"].shape == (5, B + 2) and pp["replicated"].shape == (100, 5, B + 2)
    assert pp["percentiles"].shape == (3, 5, B + 2)
    np.testing.assert_array_equal(pp["observed"].sum(axis=1), np.diff(mc["field_ind"]))
    for k in ("p_upper", "p_lower", "p_upper_total", "p_lower_total"):
        assert np.all((pp[k] >= 0) & (pp[k] <= 1)), k
    tot = pp["replicated"].sum(axis=(1, 2))
    assert abs(tot.mean() - pp["expected"].sum(axis=1).mean()) < 5 * tot.std() / np.sqrt(tot.size) + 1e-9
    np.random.seed(5)
    again = fit.posterior_predictive(ndraws=100, seed=31)
    np.testing.assert_array_equal(again["replicated"], pp["replicated"])
    fit.close()


def test_every_refusal_names_the_problem_and_leaves_the_handle_usable():
    inp = T.make_inputs("fixcomp", 500)
    gen = mock.MockGenerator(inp)
    lib, h = gen._lib, gen._h
    th = synth.walkers("fixcomp", 2, seed=1)
    th[:, 1] = -4.0
    ref = gen.draw(th, 9)
    R = 2
    mean, cnt = np.empty(R * 5), np.empty(R * 5, dtype=np.int64)
    ip = lambda a: a.ctypes.data_as(capi._c_int64_p)                 # noqa: E731

    def refused(rc, pattern):
        assert rc == capi.LF_ERR_ARG
        msg = lib.lf_mock_last_error(h).decode()
        assert pattern in msg, msg

    refused(lib.lf_mock_counts(h, None, R, None, 1, capi._ptr(mean), ip(cnt)), "theta is NULL")
    refused(lib.lf_mock_counts(h, capi._ptr(th), 0, None, 1, capi._ptr(mean), ip(cnt)), "R must be")
    refused(lib.lf_mock_counts(h, capi._ptr(th), -3, None, 1, capi._ptr(mean), ip(cnt)), "R must be")
    edges = np.linspace(41.0, 44.0, mock.MAX_BINS + 2)
    hist = np.empty(R * 5 * (mock.MAX_BINS + 3), dtype=np.int64)
    refused(lib.lf_mock_hist(h, capi._ptr(th), R, None, 1, mock.MAX_BINS + 1, capi._ptr(edges), ip(hist)), "nbins")
    bad = th.copy()
    bad[1, 2] = np.inf
    refused(lib.lf_mock_counts(h, capi._ptr(bad), R, None, 1, capi._ptr(mean), ip(cnt)), "row 1")
    big = th.copy()
    big[0, 1] = 40.0
    refused(lib.lf_mock_counts(h, capi._ptr(big), R, None, 1, capi._ptr(mean), ip(cnt)), "row 0 field 0")
    refused(lib.lf_mock_draw(h, capi._ptr(big), R, None, 1, ip(np.ones(R * 5, dtype=np.int64)), capi._ptr(np.empty(10)),
                             capi._ptr(np.empty(10)), np.empty(10, dtype=np.int32).ctypes.data_as(ctypes.POINTER(ctypes.c_int32))),
            "row 0 field 0")
    with pytest.raises(mock.MockError, match="not finite"):
        gen.counts(bad, 1)
    after = gen.draw(th, 9)
    for a, b in zip(ref, after):
        assert a.tobytes() == b.tobytes()
    assert lib.lf_mock_create(None) is None
    assert "NULL" in lib.lf_mock_last_error(None).decode()
    gen.close()
