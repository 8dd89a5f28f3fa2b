"""The observation step of the mock catalogues on the device (lf_mock_set_error_model, lf_mock_draw_err, lf_mock_hist_err;
csrc/lf_mock_noise.h) against the NumPy twin on the goldens' grids: sources within 1e-12 (the bound of
tests/test_gpu_mock.py) and equal counts for every variant, both fix_sch_al and tables of 1, 2 and 64 nodes; every edge of the
launch shapes; the histogram equal to the twin's, exactly, under a precondition asserted on the twin; sigma = 0 and batch
independence bit for bit; the refusals; and the model class on both paths."""
import ctypes
import functools
import os

import numpy as np
import pytest

import lf_deconvlib as L
from lf_testlib import O
from lumfuncmcmc_amd import capi, mock, synth

pytestmark = pytest.mark.gpu
TOL = 1e-12
GOLDENS = {"free": "free_n50", "fixcomp": "fixcomp_n50", "zevol": "zevol_n800"}
SEED = 1234
EDGE_MARGIN = 1e-9


@functools.lru_cache(maxsize=None)
def _inputs(variant, fix_sch_al):
    gdir = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    inp = O.inputs_from_golden(np.load(os.path.join(gdir, GOLDENS[variant] + ".npz")), variant)
    inp["fix_sch_al"] = fix_sch_al
    return inp


def _scaled(tw, variant, fix_sch_al, targets, seed=5, field0=False):
    """rows of the prior box with phi* shifted so that the expected total (field0: the expected count of field 0) is
    targets[i]; a target of 0 puts L* so far below the grid that every node underflows"""
    th = synth.walkers(variant, len(targets), seed=seed, fix_sch_al=fix_sch_al)
    phi = [3, 4, 5] if variant == "zevol" else [1]
    m = tw.means(th)
    m = m[:, 0] if field0 else m.sum(axis=1)
    for i, t in enumerate(targets):
        if t > 0:
            th[i, phi] += np.log10(t / m[i])
        else:
            th[i, [0, 1, 2] if variant == "zevol" else [0]] = 20.0
    return th


def _table(tw, th, M, seed=SEED):
    """M nodes between the 3 % and 97 % points of the mock's own log fluxes (so sources fall on both sides of the table),
    sigma in 0 .. 0.4 dex with zero entries.  (The device's host layer and the twin each take log10 of the distance nodes
    with their own library: one ulp of 57, 7e-15, in the flux, times the table's steepest slope - 0.4 dex over a 64th of the
    span - times |n| < 5 stays inside the 1e-12 bound at this span; a table as steep over a fifth of it would not.)"""
    z, Lt, fld, off = tw.draw(th, seed)
    t = mock.log_flux(tw.zarr, mock.ld2_nodes(tw.dl_zarr), z, Lt)
    lo, hi = np.quantile(t, (0.03, 0.97))
    nodes = np.linspace(lo, hi, M) if M > 1 else np.array([0.5 * (lo + hi)])
    sig = np.random.default_rng(M).uniform(0.02, 0.4, (tw.nf, M))
    if M >= 5:
        sig[:, ::5] = 0.0                      # zero nodes between positive ones, the first node among them
    elif M > 1:
        sig[0, 0] = 0.0                        # field 0 rises from 0 (the goldens' summed tables have sources in field 0 only)
    else:
        sig[tw.nf - 1, 0] = 0.0                # one value per field: the last field has no noise
    assert (t < nodes[0]).sum() > 10 and (t > nodes[-1]).sum() > 10
    return nodes, sig


@pytest.mark.parametrize("fix_sch_al", [False, True])
@pytest.mark.parametrize("variant", ["free", "fixcomp", "zevol"])
def test_device_matches_the_twin(variant, fix_sch_al):
    inp = _inputs(variant, fix_sch_al)
    tw, gen = mock.MockTwin(inp), mock.MockGenerator(inp)
    th = _scaled(tw, variant, fix_sch_al, (3000.0, 300.0, 5.0, 0.0))
    rid = np.arange(100, 104, dtype=np.int64)
    try:
        for M in (1, 2, 64):
            nodes, sig = _table(tw, th, M)
            tw.set_error_model(nodes, sig)
            gen.set_error_model(nodes, sig)
            d = gen.draw_noisy(th, SEED, rid)
            h = tw.draw_noisy(th, SEED, rid)
            np.testing.assert_array_equal(d[5], h[5])                 # counts
            np.testing.assert_array_equal(d[4], h[4])
            assert d[5][-1] > 2500
            worst = [float(np.max(np.abs(a - b))) for a, b in zip(d[:4], h[:4])]
            print("%s fix_sch_al=%d M=%2d: %d sources, max |dev - twin| z %.2e L_true %.2e L_obs %.2e sigma %.2e"
                  % (variant, fix_sch_al, M, d[5][-1], *worst))
            for a, b in zip(d[:4], h[:4]):
                np.testing.assert_allclose(a, b, rtol=0, atol=TOL)
            zero = h[3] == 0.0
            assert (~zero).any() and zero.any() == (sig[np.unique(h[4])] == 0.0).any()
            assert d[2][zero].tobytes() == d[1][zero].tobytes()      # sigma = 0: L_obs is L_true bit for bit
            plain = gen.draw(th, SEED, rid)
            assert plain[0].tobytes() == d[0].tobytes() and plain[1].tobytes() == d[1].tobytes()
    finally:
        gen.close()


@pytest.mark.parametrize("variant", ["free", "fixcomp", "zevol"])
def test_draw_counts_at_the_edges_of_a_workgroup(variant):
    inp = _inputs(variant, False)
    tw, gen = mock.MockTwin(inp), mock.MockGenerator(inp)
    nf = tw.nf
    R = -(-5 // nf) + 1
    th = _scaled(tw, variant, False, (3000.0,) * R)
    cnt = np.resize(np.array([0, 1, 255, 256, 257], dtype=np.int64), R * nf).reshape(R, nf)
    assert set(cnt.ravel()) == {0, 1, 255, 256, 257}
    nodes, sig = _table(tw, th, 7)
    tw.set_error_model(nodes, sig)
    gen.set_error_model(nodes, sig)
    try:
        d = gen.draw_noisy(th, SEED, count=cnt)
        h = tw.draw_noisy(th, SEED, count=cnt)
        np.testing.assert_array_equal(d[5], h[5])
        np.testing.assert_array_equal(np.diff(d[5]), cnt.ravel())
        np.testing.assert_array_equal(d[4], h[4])
        for a, b in zip(d[:4], h[:4]):
            np.testing.assert_allclose(a, b, rtol=0, atol=TOL)
        one = gen.draw_noisy(th[:1], SEED, count=np.where(np.arange(nf) == 0, 1, 0))
        assert one[2].size == 1
    finally:
        gen.close()


@functools.lru_cache(maxsize=None)
def _hist_case(variant):
    """(inputs, rows, table, the twin's noisy draw): rows whose per-(row, field) counts cover every launch shape of
    lf_mock_hist_err, asserted here on the twin"""
    inp = _inputs(variant, False)
    tw = mock.MockTwin(inp)
    th = _scaled(tw, variant, False, (0.0, 100.0, 6000.0, 10000.0), seed=7, field0=True)
    nodes, sig = _table(tw, th, 64)
    tw.set_error_model(nodes, sig)
    drawn = tw.draw_noisy(th, SEED)
    n = np.diff(drawn[5])
    chunk = 4096
    assert (n[:tw.nf] == 0).all()                                        # counts of 0
    assert ((n > 0) & (n < 256)).any()                                   # less than one pass of the workgroup
    ragged = (n > chunk) & (n < 2 * chunk) & (n % 256 != 0)
    assert ragged.any()                                                  # two workgroups, the second's last pass ragged
    assert (n > 2 * chunk).any()                                         # more than two workgroups
    return inp, th, (nodes, sig), drawn


def _edges_clear_of_sources(Lobs, nbins):
    lo, hi = float(Lobs.min()), float(Lobs.max())
    edges = np.linspace(lo + 0.3, hi - 0.2, nbins + 1) if nbins > 1 else np.array([lo + 0.3, hi - 0.2])
    gap = np.min(np.abs(Lobs[:, None] - edges[None, :]), axis=1) if nbins == 1 else None
    if gap is None:
        i = np.clip(np.searchsorted(edges, Lobs), 1, nbins)
        gap = np.minimum(np.abs(Lobs - edges[i - 1]), np.abs(edges[i] - Lobs))
    return edges, float(gap.min())


@pytest.mark.parametrize("nbins", [1, 1022])
@pytest.mark.parametrize("variant", ["free", "fixcomp", "zevol"])
def test_hist_equals_the_twins_exactly(variant, nbins):
    inp, th, table, drawn = _hist_case(variant)
    Lobs, off = drawn[2], drawn[5]
    edges, gap = _edges_clear_of_sources(Lobs, nbins)
    print("%s nbins=%d: %d sources, nearest L_obs to an edge %.3e" % (variant, nbins, Lobs.size, gap))
    assert gap > EDGE_MARGIN                # the precondition: no source of the twin's within 1e-9 of an edge
    want = mock.bin_sources(Lobs, off, edges).reshape(len(th), -1, nbins + 2)
    assert want[..., 0].sum() > 0 and want[..., -1].sum() > 0
    gen = mock.MockGenerator(inp)
    try:
        gen.set_error_model(*table)
        got = gen.hist_noisy(th, edges, SEED)
        np.testing.assert_array_equal(got, want)
        np.testing.assert_array_equal(got.sum(axis=2), gen.counts(th, SEED)[1])
    finally:
        gen.close()


def test_an_all_zero_table_gives_lf_mock_hist_bit_for_bit():
    inp, th, (nodes, sig), _ = _hist_case("zevol")
    gen = mock.MockGenerator(inp)
    try:
        gen.set_error_model(nodes, np.zeros_like(sig))
        for edges in (np.linspace(41.0, 44.0, 2), np.linspace(41.5, 43.5, 1023), np.linspace(41.6, 43.0, 38)):
            a, b = gen.hist_noisy(th, edges, SEED), gen.hist(th, edges, SEED)
            assert a.tobytes() == b.tobytes() and a.sum() > 10000
        d = gen.draw_noisy(th[1:3], SEED)
        assert d[2].tobytes() == d[1].tobytes() and not d[3].any()
    finally:
        gen.close()


def test_a_row_does_not_depend_on_its_batch():
    inp = _inputs("zevol", False)
    tw, gen = mock.MockTwin(inp), mock.MockGenerator(inp)
    rng = np.random.default_rng(3)
    th = _scaled(tw, "zevol", False, tuple(rng.uniform(200.0, 2000.0, 64)), seed=9)
    rid = rng.integers(0, 1 << 62, 64)
    gen.set_error_model(*_table(tw, th[:4], 9))
    edges = np.linspace(41.5, 43.5, 41)
    nf = gen.nf
    try:
        big, hbig = gen.draw_noisy(th, 77, rid), gen.hist_noisy(th, edges, 77, rid)
        again, hagain = gen.draw_noisy(th, 77, rid), gen.hist_noisy(th, edges, 77, rid)
        for a, b in zip(big, again):
            assert a.tobytes() == b.tobytes()
        assert hbig.tobytes() == hagain.tobytes()
        perm = rng.permutation(64)
        sh, hsh = gen.draw_noisy(th[perm], 77, rid[perm]), gen.hist_noisy(th[perm], edges, 77, rid[perm])
        for i in (0, 37, 63):
            one = gen.draw_noisy(th[i:i + 1], 77, rid[i:i + 1])
            lo, hi = big[5][i * nf], big[5][(i + 1) * nf]
            p = int(np.flatnonzero(perm == i)[0])
            slo, shi = sh[5][p * nf], sh[5][(p + 1) * nf]
            assert hi > lo
            for a, b, c in zip(one[:5], big[:5], sh[:5]):
                assert a.tobytes() == b[lo:hi].tobytes() == c[slo:shi].tobytes()
            h1 = gen.hist_noisy(th[i:i + 1], edges, 77, rid[i:i + 1])
            assert h1[0].tobytes() == hbig[i].tobytes() == hsh[p].tobytes()
    finally:
        gen.close()


def test_every_refusal_names_the_problem_and_leaves_the_handle_usable():
    inp = _inputs("fixcomp", False)
    tw, gen = mock.MockTwin(inp), mock.MockGenerator(inp)
    lib, h, nf, S = gen._lib, gen._h, gen.nf, gen.S
    th = _scaled(tw, "fixcomp", False, (400.0, 40.0))
    R = 2
    ip = lambda a: a.ctypes.data_as(capi._c_int64_p)                 # noqa: E731
    i32 = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))  # noqa: E731
    P = capi._ptr

    def refused(rc, pattern):
        assert rc == capi.LF_ERR_ARG
        msg = lib.lf_mock_last_error(h).decode()
        assert pattern in msg, msg

    cnt = np.full(R * nf, 3, dtype=np.int64)
    buf = [np.empty(R * nf * 3) for _ in range(4)]
    fld = np.empty(R * nf * 3, dtype=np.int32)
    edges = np.linspace(41.0, 44.0, 5)
    hist = np.empty(R * nf * 6, dtype=np.int64)
    try:
        # no model yet
        refused(lib.lf_mock_draw_err(h, P(th), R, None, 1, ip(cnt), P(buf[0]), P(buf[1]), P(buf[2]), P(buf[3]), i32(fld)), "no error model")
        refused(lib.lf_mock_hist_err(h, P(th), R, None, 1, 4, P(edges), ip(hist)), "no error model")
        with pytest.raises(mock.MockError, match="no error model"):
            gen.hist_noisy(th, edges, 1)
        nodes = np.array([-16.5, -16.0, -15.5])
        sig = np.full((nf, 3), 0.2)
        dl = capi._f64(inp["DL_zarr"])
        set_ = lib.lf_mock_set_error_model
        refused(set_(h, 3, None, P(sig), P(dl)), "NULL")
        refused(set_(h, 3, P(nodes), None, P(dl)), "NULL")
        refused(set_(h, 3, P(nodes), P(sig), None), "NULL")
        refused(set_(h, 65, P(nodes), P(sig), P(dl)), "M must be in 0..64")
        refused(set_(h, -1, P(nodes), P(sig), P(dl)), "M must be in 0..64")
        refused(set_(h, 3, P(np.array([-16.5, -16.5, -15.5])), P(sig), P(dl)), "node 1: logf_nodes must be finite and strictly ascending")
        refused(set_(h, 3, P(np.array([-16.5, -16.0, np.inf])), P(sig), P(dl)), "node 2")
        bad = sig.copy()
        bad[nf - 1, 1] = -0.01
        refused(set_(h, 3, P(nodes), P(bad), P(dl)), "field %d node 1: sigma must be finite and >= 0" % (nf - 1))
        bad[nf - 1, 1], bad[0, 2] = 0.2, np.nan
        refused(set_(h, 3, P(nodes), P(bad), P(dl)), "field 0 node 2")
        for v in (0.0, -5.0, np.nan, np.inf):
            bdl = dl.copy()
            bdl[S - 2] = v
            refused(set_(h, 3, P(nodes), P(sig), P(bdl)), "dl_zarr[%d]" % (S - 2))
        # a refused model leaves none in place here (none was set), and the handle works
        refused(lib.lf_mock_hist_err(h, P(th), R, None, 1, 4, P(edges), ip(hist)), "no error model")
        gen.set_error_model(nodes, sig)
        ref = gen.draw_noisy(th, 9)
        assert ref[2].size > 300
        # the refusals of lf_mock_draw and lf_mock_hist
        refused(lib.lf_mock_draw_err(h, None, R, None, 1, ip(cnt), P(buf[0]), P(buf[1]), P(buf[2]), P(buf[3]), i32(fld)), "theta is NULL")
        refused(lib.lf_mock_draw_err(h, P(th), 0, None, 1, ip(cnt), P(buf[0]), P(buf[1]), P(buf[2]), P(buf[3]), i32(fld)), "R must be")
        refused(lib.lf_mock_draw_err(h, P(th), R, None, 1, None, P(buf[0]), P(buf[1]), P(buf[2]), P(buf[3]), i32(fld)), "count is NULL")
        refused(lib.lf_mock_draw_err(h, P(th), R, None, 1, ip(cnt), P(buf[0]), P(buf[1]), None, P(buf[3]), i32(fld)), "NULL")
        neg = cnt.copy()
        neg[nf + 1] = -1
        refused(lib.lf_mock_draw_err(h, P(th), R, None, 1, ip(neg), P(buf[0]), P(buf[1]), P(buf[2]), P(buf[3]), i32(fld)), "row 1 field 1")
        nonfin = th.copy()
        nonfin[1, 2] = np.inf
        refused(lib.lf_mock_hist_err(h, P(nonfin), R, None, 1, 4, P(edges), ip(hist)), "row 1")
        big = th.copy()
        big[0, 1] = 40.0
        refused(lib.lf_mock_hist_err(h, P(big), R, None, 1, 4, P(edges), ip(hist)), "row 0 field 0")
        refused(lib.lf_mock_draw_err(h, P(big), R, None, 1, ip(cnt), P(buf[0]), P(buf[1]), P(buf[2]), P(buf[3]), i32(fld)), "row 0 field 0")
        wide = np.linspace(41.0, 44.0, mock.MAX_BINS + 2)
        whist = np.empty(R * nf * (mock.MAX_BINS + 3), dtype=np.int64)
        refused(lib.lf_mock_hist_err(h, P(th), R, None, 1, mock.MAX_BINS + 1, P(wide), ip(whist)), "nbins")
        refused(lib.lf_mock_hist_err(h, P(th), R, None, 1, 0, P(edges), ip(hist)), "nbins")
        refused(lib.lf_mock_hist_err(h, P(th), R, None, 1, 4, None, ip(hist)), "NULL")
        refused(lib.lf_mock_hist_err(h, P(th), R, None, 1, 4, P(edges[::-1].copy()), ip(hist)), "edges must be finite and non-decreasing")
        with pytest.raises(mock.MockError, match="field 0 node 2"):
            gen.set_error_model(nodes, bad)
        after = gen.draw_noisy(th, 9)
        for a, b in zip(ref, after):
            assert a.tobytes() == b.tobytes()
        gen.set_error_model(None, None)                              # M = 0 clears
        with pytest.raises(mock.MockError, match="no error model"):
            gen.draw_noisy(th, 9)
    finally:
        gen.close()


def test_the_model_class_on_the_device_and_on_the_host():
    cat = synth.catalogue(400, seed=17)
    cat["lum_e"] = np.random.default_rng(5).uniform(0.05, 0.3, 400)
    o = L.fixcomp_model(cat)
    theta = np.array([synth.LSTAR, synth.PHISTAR, synth.SCH_AL])
    rng = np.random.default_rng(6)
    rows = theta[None] + rng.normal(0.0, 0.02, (50, 3))
    rows[:, 1] -= 1.0                                                # a tenth of the sources: the host path stays quick
    o.samples = np.concatenate([rows, -0.5 * rng.chisquare(3, 50)[:, None]], axis=1)
    try:
        kw = dict(ndraws=24, seed=31)
        np.random.seed(5)
        dev = o.posterior_predictive(device=True, noise="catalogue", **kw)
        np.random.seed(5)
        host = o.posterior_predictive(device=False, noise="catalogue", **kw)
        assert dev["noise"] == host["noise"] == "catalogue"
        want = o.error_model()
        for a, b, c in zip(dev["sigma_model"], host["sigma_model"], want):
            assert a.tobytes() == b.tobytes() == c.tobytes()
        np.testing.assert_array_equal(dev["replicated"], host["replicated"])
        np.testing.assert_array_equal(dev["observed"], host["observed"])
        np.testing.assert_allclose(dev["expected"], host["expected"], rtol=1e-12, atol=0)
        assert dev["replicated"].sum() > 20000
        # noise=None: the dict the method returned before the keyword (mock.predictive on the same rows), plus the two keys
        np.random.seed(5)
        plain = o.posterior_predictive(device=True, **kw)
        np.random.seed(5)
        prows = o._posterior_rows(24, 7.5)[:, :-1]
        old = mock.predictive(o._mock_generator(True), prows, np.linspace(np.min(o.lum), np.max(o.lum), 21), o.lum,
                              np.asarray(o.field_ind, dtype=np.int64), 31)
        assert plain["noise"] is None and plain["sigma_model"] is None
        assert sorted(plain) == sorted(list(old) + ["noise", "sigma_model"])
        for k, v in old.items():
            assert np.array_equal(plain[k], v), k
        assert not np.array_equal(plain["replicated"], dev["replicated"])
        pair = o.posterior_predictive(device=True, noise=want, **kw)
        assert pair["noise"] == "model"
        # mock_catalogue: the device adds the noise; the host path agrees to rounding
        a = o.mock_catalogue(theta, seed=8, device=True, lum_err="catalogue")
        b = o.mock_catalogue(theta, seed=8, device=False, lum_err="catalogue")
        c = o.mock_catalogue(theta, seed=8, device=True)
        np.testing.assert_array_equal(a["field_ind"], b["field_ind"])
        for f in range(o.nfields):
            assert a["lum_true"][f].tobytes() == c["lum"][f].tobytes()
            for k in ("z", "lum", "lum_e", "lum_true"):
                np.testing.assert_allclose(a[k][f], b[k][f], rtol=0, atol=TOL)
    finally:
        o.close()
