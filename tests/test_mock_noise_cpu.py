"""The observation step of the mock catalogues on the host (lumfuncmcmc_amd/mock.py: MockTwin.set_error_model, draw_noisy,
hist_noisy, error_model_from_catalogue): the sigma lookup against np.interp, sigma = 0 and a constant
table tied to what the mocks did before (hist, catalogue_lists(lum_err=...)) bit for bit, batch independence, the moments of
the noise, the default model from a catalogue, the refusals - and the point of the feature: at the true theta the count of
bright sources of a noisy catalogue lies inside the noisy replicates and above the noiseless ones."""
import numpy as np
import pytest

import lf_deconvlib as L
import lf_testlib as T
from lumfuncmcmc_amd import mock, synth

SEED = 20260229


def _twin(variant="fixcomp", n=300, **kw):
    inp = T.make_inputs(variant, n, **kw)
    return mock.MockTwin(inp), inp


def _rows(tw, variant, R, target, seed=5):
    th = synth.walkers(variant, R, seed=seed)
    phi = [3, 4, 5] if variant == "zevol" else [1]
    th[:, phi] += np.log10(target / tw.means(th).sum(axis=1))[:, None]
    return th


def _table(nf, M, lo=-16.6, hi=-15.4, seed=1):
    rng = np.random.default_rng(seed)
    nodes = np.sort(rng.uniform(lo, hi, M)) if M > 1 else np.array([0.5 * (lo + hi)])
    return nodes, rng.uniform(0.02, 0.4, (nf, M))


def test_sigma_lookup_is_np_interp_clamped():
    rng = np.random.default_rng(2)
    for M in (1, 2, 3, 17, 64):
        nodes, sig = _table(1, M, seed=M)
        t = np.concatenate([rng.uniform(-18.0, -14.0, 4000), nodes, [nodes[0] - 1e-13, nodes[-1] + 1e-13, -30.0, 5.0]])
        got = mock.sigma_lookup(nodes, sig[0], t)
        want = np.interp(t, nodes, sig[0])                      # (np.interp holds the end values outside the nodes)
        np.testing.assert_allclose(got, want, rtol=0, atol=4 * np.finfo(float).eps)
        assert np.all(got[t <= nodes[0]] == sig[0, 0]) and np.all(got[t >= nodes[-1]] == sig[0, -1])
        np.testing.assert_array_equal(mock.sigma_lookup(nodes, sig[0], nodes), sig[0])
    assert np.all(mock.sigma_lookup(np.array([-16.0]), np.array([0.3]), t) == 0.3)


def test_the_flux_of_a_mock_source_is_the_interpolant_the_issue_states():
    tw, inp = _twin()
    ld2n = mock.ld2_nodes(inp["DL_zarr"])
    np.testing.assert_array_equal(ld2n, np.log10(4.0 * np.pi * (3.086e24 * inp["DL_zarr"]) ** 2))
    rng = np.random.default_rng(4)
    z = np.concatenate([rng.uniform(tw.zarr[0], tw.zarr[-1], 500), tw.zarr])
    Lx = rng.uniform(41.0, 44.0, z.size)
    np.testing.assert_allclose(mock.log_flux(tw.zarr, ld2n, z, Lx), Lx - np.interp(z, tw.zarr, ld2n), rtol=0, atol=1e-13)


def test_an_all_zero_table_changes_nothing():
    for variant in ("free", "zevol"):
        tw, _ = _twin(variant)
        th = _rows(tw, variant, 3, 4000.0)
        nodes, sig = _table(tw.nf, 5)
        tw.set_error_model(nodes, np.zeros_like(sig))
        z, Lt, Lo, sg, fld, off = tw.draw_noisy(th, SEED)
        z0, L0, f0, o0 = tw.draw(th, SEED)
        assert Lt.size > 5000 and not sg.any()
        assert Lo.tobytes() == Lt.tobytes() == L0.tobytes() and z.tobytes() == z0.tobytes()
        np.testing.assert_array_equal(off, o0)
        edges = np.linspace(41.5, 43.5, 33)
        np.testing.assert_array_equal(tw.hist_noisy(th, edges, SEED), tw.hist(th, edges, SEED))


def test_a_constant_table_per_field_is_catalogue_lists_lum_err():
    tw, _ = _twin("fixcomp")
    th = _rows(tw, "fixcomp", 1, 3000.0)
    per = np.array([0.0, 0.1, 0.25, 0.3, 0.45])
    for M, rid in ((1, 0), (4, 12345)):
        nodes, _ = _table(tw.nf, M)
        tw.set_error_model(nodes, np.repeat(per[:, None], M, axis=1))
        z, Lt, Lo, sg, fld, off = tw.draw_noisy(th, SEED, row_ids=[rid])
        old = mock.catalogue_lists(z, Lt, fld, tw.nf, lum_err=per, seed=SEED, row_id=rid)
        assert np.concatenate(old["lum"]).tobytes() == Lo.tobytes()
        assert np.concatenate(old["lum_e"]).tobytes() == sg.tobytes()
        new = mock.observed_lists(z, Lt, Lo, sg, fld, tw.nf)
        for k in ("z", "lum", "lum_e", "lum_true"):
            assert all(np.array_equal(a, b) for a, b in zip(old[k], new[k])), k
        np.testing.assert_array_equal(old["field_ind"], new["field_ind"])


def test_a_row_does_not_depend_on_its_batch():
    tw, _ = _twin("zevol")
    th = _rows(tw, "zevol", 7, 800.0)
    rng = np.random.default_rng(3)
    rid = rng.integers(0, 1 << 62, 7)
    tw.set_error_model(*_table(tw.nf, 6))
    big = tw.draw_noisy(th, 77, rid)
    nf = tw.nf
    edges = np.linspace(41.0, 44.0, 13)
    hbig = tw.hist_noisy(th, edges, 77, rid)
    perm = rng.permutation(7)
    sh = tw.draw_noisy(th[perm], 77, rid[perm])
    for i in (0, 4, 6):
        one = tw.draw_noisy(th[i:i + 1], 77, rid[i:i + 1])
        lo, hi = big[5][i * nf], big[5][(i + 1) * nf]
        p = int(np.flatnonzero(perm == i)[0])
        slo, shi = sh[5][p * nf], sh[5][(p + 1) * nf]
        assert hi > lo
        for a, b, c in zip(one[:5], big[:5], sh[:5]):
            assert a.tobytes() == b[lo:hi].tobytes() == c[slo:shi].tobytes()
        np.testing.assert_array_equal(tw.hist_noisy(th[i:i + 1], edges, 77, rid[i:i + 1])[0], hbig[i])


def test_the_noise_has_zero_mean_and_unit_variance():
    tw, _ = _twin("free")
    th = _rows(tw, "free", 1, 2.0e4)
    nodes, sig = _table(tw.nf, 9)
    tw.set_error_model(nodes, sig)
    z, Lt, Lo, sg, fld, off = tw.draw_noisy(th, SEED)
    n = Lt.size
    assert 1.9e4 < n < 2.1e4 and sg.min() > 0
    assert np.unique(sg).size > n // 4                          # the flux dependence is there (the rest lie outside the nodes)
    r = (Lo - Lt) / sg
    print("noise moments over %d sources: mean %.4f (bound %.4f), var %.4f (1 +- %.4f)" % (n, r.mean(), 5 / np.sqrt(n), r.var(),
                                                                                          5 * np.sqrt(2.0 / n)))
    assert abs(r.mean()) < 5.0 / np.sqrt(n)
    assert abs(r.var() - 1.0) < 5.0 * np.sqrt(2.0 / n)


def test_error_model_from_catalogue_recovers_a_planted_law():
    rng = np.random.default_rng(8)
    nf, N, a, c = 3, 6000, 0.08, -16.0
    fi = np.array([0, 2500, 4500, 6000])
    logf = np.concatenate([np.sort(rng.uniform(-16.5, -15.0, n)) for n in np.diff(fi)])
    scale = np.repeat([1.0, 1.5, 0.5], np.diff(fi))
    sigma = scale * a * 10.0 ** (-(logf - c))
    nodes, val = mock.error_model_from_catalogue(logf, sigma, fi, nodes=16)
    assert nodes.shape == (16,) and val.shape == (nf, 16) and np.all(np.diff(nodes) > 0)
    n2, v2 = mock.error_model_from_catalogue(logf, sigma, fi, nodes=16)
    assert n2.tobytes() == nodes.tobytes() and v2.tobytes() == val.tobytes()             # deterministic
    # the law is monotone, so a bin's median sigma is the law at a flux inside the bin: within the bin's width of the node
    srt = np.sort(logf)
    cut = (np.arange(17) * N) // 16
    lo, hi = srt[cut[:-1]], srt[cut[1:] - 1]
    assert np.all((nodes >= lo) & (nodes <= hi))
    for f, s in enumerate((1.0, 1.5, 0.5)):
        assert np.all(val[f] <= s * a * 10.0 ** (-(lo - c)) * (1 + 1e-12)) and np.all(val[f] >= s * a * 10.0 ** (-(hi - c)) * (1 - 1e-12))
    # through the twin: sigma of a source at a node's flux is the node's value
    assert np.array_equal(mock.sigma_lookup(nodes, val[1], nodes), val[1])


def test_error_model_from_catalogue_empty_bins_empty_fields_and_merged_nodes():
    # field 0 only faint, field 1 only bright, field 2 empty: 4 bins of 3 sources
    logf = np.array([-16.9, -16.8, -16.7, -16.6, -16.5, -16.4, -15.6, -15.5, -15.4, -15.3, -15.2, -15.1])
    sigma = np.array([0.40, 0.41, 0.42, 0.30, 0.31, 0.32, 0.10, 0.11, 0.12, 0.05, 0.06, 0.07])
    fi = np.array([0, 6, 12, 12])
    nodes, val = mock.error_model_from_catalogue(logf, sigma, fi, nodes=4)
    np.testing.assert_array_equal(nodes, [-16.8, -16.5, -15.5, -15.2])
    np.testing.assert_array_equal(val[0], [0.41, 0.31, 0.31, 0.31])         # empty bins: the nearest filled bin of the field
    np.testing.assert_array_equal(val[1], [0.11, 0.11, 0.11, 0.06])
    np.testing.assert_array_equal(val[2], [0.41, 0.31, 0.11, 0.06])         # a field without sources: the pooled medians
    # equal distance: the lower bin
    fi2 = np.array([0, 3, 3, 12])
    logf2 = np.concatenate([[-16.9, -15.5, -15.1], np.delete(logf, [0, 7, 11])])
    sig2 = np.concatenate([[0.9, 0.5, 0.1], np.delete(sigma, [0, 7, 11])])
    _, v = mock.error_model_from_catalogue(logf2, sig2, fi2, nodes=4)
    assert v[0, 1] == 0.9 and v[0, 0] == 0.9 and v[0, 2] == 0.5 and v[0, 3] == 0.1
    # nodes that coincide are merged, and more nodes than sources are not made
    same = np.array([-16.0] * 9 + [-15.0, -14.9, -14.8])
    nodes, val = mock.error_model_from_catalogue(same, sigma, np.array([0, 12]), nodes=4)
    np.testing.assert_array_equal(nodes, [-16.0, -14.9])
    np.testing.assert_array_equal(val, [[np.median(sigma[:9]), 0.06]])
    nodes, val = mock.error_model_from_catalogue(logf[:3], sigma[:3], np.array([0, 3]), nodes=16)
    assert nodes.size == 3
    nodes, val = mock.error_model_from_catalogue(logf, sigma, fi, nodes=1)
    assert nodes.shape == (1,) and val.shape == (3, 1)
    with pytest.raises(ValueError, match="one catalogue"):
        mock.error_model_from_catalogue(logf, sigma[:-1], fi)
    with pytest.raises(ValueError, match="finite"):
        mock.error_model_from_catalogue(logf, -sigma, fi)


def test_the_model_class_builds_and_uses_the_model():
    cat = synth.catalogue(600, seed=17)
    fi = cat["field_ind"]
    rng = np.random.default_rng(5)
    cat["lum_e"] = rng.uniform(0.05, 0.3, 600)
    o = L.fixcomp_model(cat)
    nodes, sig = o.error_model(nodes=8)
    want = mock.error_model_from_catalogue(np.log10(o.flux), o.lum_e, fi, nodes=8)
    assert nodes.tobytes() == want[0].tobytes() and sig.tobytes() == want[1].tobytes() and sig.shape == (5, 8)
    want16 = o.error_model()[1]                                  # what "catalogue" means: the default of 16 nodes
    theta = np.array([synth.LSTAR, synth.PHISTAR, synth.SCH_AL])
    a = o.mock_catalogue(theta, seed=11, device=False)
    b = o.mock_catalogue(theta, seed=11, device=False, lum_err="catalogue")
    c = o.mock_catalogue(theta, seed=11, device=False, lum_err=o.error_model())
    d = o.mock_catalogue(theta, seed=11, device=False, lum_err=(0.1, 0.2, 0.1, 0.2, 0.1))      # five numbers: per field, as before
    assert sorted(b) == ["field_ind", "lum", "lum_e", "lum_true", "seed", "theta", "z"] == sorted(d)
    for f in range(5):
        assert np.array_equal(b["lum_true"][f], a["lum"][f]) and np.array_equal(b["z"][f], a["z"][f])
        assert np.array_equal(b["lum"][f], c["lum"][f]) and np.array_equal(b["lum_e"][f], c["lum_e"][f])
        assert np.all((b["lum_e"][f] >= want16[f].min() - 1e-15) & (b["lum_e"][f] <= want16[f].max() + 1e-15))
        assert np.all(d["lum_e"][f] == (0.1, 0.2, 0.1, 0.2, 0.1)[f])
    with pytest.raises(ValueError, match="catalogue"):
        o.mock_catalogue(theta, seed=11, device=False, lum_err="survey")
    o.close()


def test_refusals_name_the_problem():
    tw, inp = _twin()
    nodes, sig = _table(tw.nf, 4)
    for bad_nodes, bad_sig, pattern in (
            (np.linspace(-17, -15, 65), np.zeros((5, 65)), "M must be in 1..64"),
            (np.zeros(0), np.zeros((5, 0)), "M must be"),
            (nodes[::-1], sig, "node 1: logf_nodes must be finite and strictly ascending"),
            (np.array([-16.0, -16.0, -15.0, -14.0]), sig, "node 1"),
            (np.array([-16.0, np.nan, -15.0, -14.0]), sig, "node 1"),
            (nodes, sig[:4], "sigma must be (nf, M) = (5, 4)"),
            (nodes, np.where(np.arange(20).reshape(5, 4) == 14, -0.1, sig), "field 3 node 2: sigma must be finite and >= 0"),
            (nodes, np.where(np.arange(20).reshape(5, 4) == 5, np.inf, sig), "field 1 node 1")):
        with pytest.raises(mock.MockError) as e:
            tw.set_error_model(bad_nodes, bad_sig)
        assert pattern in str(e.value), str(e.value)
    th = _rows(tw, "fixcomp", 1, 100.0)
    with pytest.raises(mock.MockError, match="no error model is set"):
        tw.draw_noisy(th, 1)
    with pytest.raises(mock.MockError, match="no error model is set"):
        tw.hist_noisy(th, np.linspace(41, 44, 4), 1)
    bad = dict(inp)
    bad["DL_zarr"] = np.where(np.arange(inp["DL_zarr"].size) == 7, 0.0, inp["DL_zarr"])
    with pytest.raises(mock.MockError, match="DL_zarr"):
        mock.MockTwin(bad).set_error_model(nodes, sig)
    del bad["DL_zarr"]
    with pytest.raises(mock.MockError, match="DL_zarr"):
        mock.MockTwin(bad).set_error_model(nodes, sig)
    tw.set_error_model(nodes, sig)
    assert tw.draw_noisy(th, 1)[2].size > 0
    tw.set_error_model(None, None)                               # cleared
    with pytest.raises(mock.MockError, match="no error model is set"):
        tw.draw_noisy(th, 1)


PP_R, PP_SEED = 200, 4242            # replicates and their seed; the catalogue is section 3.18's profile mock (lf_deconvlib.EDD_*)


def test_noisy_replicates_hold_the_observed_bright_count_and_noiseless_ones_do_not():
    """Section 3.18's seeded mock (about 3000 sources, 0.25 dex) at the true theta, 200 replicates on the twin: the observed
    count above L* + 0.5 dex lies inside the 0.5 - 99.5 % range of the noisy replicates and above the 99.5 % point of the
    noiseless ones.  Confirmed on the CPU with these seeds before they were fixed here."""
    o, theta, mc = L.noisy_mock(L.EDD_N, L.EDD_ERR, L.EDD_SEED)
    tw = mock.MockTwin(o.kernel_inputs())
    o.close()
    cut = theta[0] + 0.5
    observed = int(sum((a >= cut).sum() for a in mc["lum"]))
    rows = np.repeat(theta[None], PP_R, axis=0)
    edges = np.array([30.0, cut, 60.0])
    tw.set_error_model(np.array([-16.0]), np.full((tw.nf, 1), L.EDD_ERR))
    z, Lt, Lo, sg, fld, off = tw.draw_noisy(rows, PP_SEED)       # one draw; hist_noisy and hist are its two binnings
    noisy = mock.bin_sources(Lo, off, edges).reshape(PP_R, tw.nf, 4)[:, :, 2].sum(axis=1)
    plain = mock.bin_sources(Lt, off, edges).reshape(PP_R, tw.nf, 4)[:, :, 2].sum(axis=1)
    np.testing.assert_array_equal(tw.hist_noisy(rows[:3], edges, PP_SEED)[:, :, 2].sum(axis=1), noisy[:3])
    np.testing.assert_array_equal(tw.hist(rows[:3], edges, PP_SEED)[:, :, 2].sum(axis=1), plain[:3])
    qn = np.percentile(noisy, (0.5, 99.5))
    qp = np.percentile(plain, 99.5)
    print("observed above L* + 0.5: %d; noisy replicates 0.5 - 99.5 %%: %.1f - %.1f; noiseless 99.5 %%: %.1f" % (observed, qn[0], qn[1], qp))
    assert qn[0] <= observed <= qn[1]
    assert observed > qp
