"""Mock catalogues of the cut process on the device (lf_mock_set_cut_band, lf_mock_draw_cut, lf_mock_hist_cut;
csrc/lf_mock_cut.h) against the NumPy twin on grids with their own lower edge per redshift column
(lf_cutlib.cut_inputs, S = 5 and S = 23): every candidate within 1e-12 (section 3.23's bound) with equal candidate counts in
both pieces, for every variant, both fix_sch_al and tables of 1, 2 and 64 nodes with zero entries; identical keep flags and
kept order under a precondition asserted on the twin; every edge of the launch shapes in both pieces; the histogram and the
kept totals equal to the twin's, exactly; batch independence and the all-zero table bit for bit; the refusals; the model class
on both paths."""
import ctypes
import functools

import numpy as np
import pytest

import lf_mockcutlib as K
from lumfuncmcmc_amd import capi, mock, synth

pytestmark = pytest.mark.gpu
TOL = 1e-12
SEED = 1234
EDGE_MARGIN = 1e-9


def _pair(variant, S, M, fix_sch_al=False):
    inp = K.inputs(variant, S, fix_sch_al)
    nodes, sig = K.table(M)
    return inp, K.arm(mock.MockTwin(inp), inp, nodes, sig), K.arm(mock.MockGenerator(inp), inp, nodes, sig)


def _agree(dev, host, gap):
    """candidates_cut of the device against the twin's: counts, fields, flags equal; values within TOL"""
    np.testing.assert_array_equal(dev[6], host[6])
    np.testing.assert_allclose(dev[7], host[7], rtol=1e-12, atol=0)
    np.testing.assert_array_equal(dev[4], host[4])
    worst = [float(np.max(np.abs(a - b))) if a.size else 0.0 for a, b in zip(dev[:4], host[:4])]
    for a, b in zip(dev[:4], host[:4]):
        np.testing.assert_allclose(a, b, rtol=0, atol=TOL)
    assert gap > EDGE_MARGIN, gap               # the precondition: no L_obs of the twin's within 1e-9 of its edge
    np.testing.assert_array_equal(dev[5], host[5])
    return worst


@pytest.mark.parametrize("fix_sch_al", [False, True])
@pytest.mark.parametrize("variant", ["free", "fixcomp", "zevol"])
def test_device_matches_the_twin(variant, fix_sch_al):
    rid = np.arange(100, 104, dtype=np.int64)
    for S, M in ((23, 1), (5, 2), (23, 64)):
        inp, tw, gen = _pair(variant, S, M, fix_sch_al)
        try:
            th = K.rows_for_means(tw, variant, fix_sch_al, (3000.0, 300.0, 5.0, 0.0), 0)
            host, gap = K.edge_gap(tw, th, SEED, rid)
            dev = gen.candidates_cut(th, SEED, rid)
            worst = _agree(dev, host, gap)
            print("%s fix_sch_al=%d S=%d M=%2d: %d + %d candidates, %d kept; max |dev - twin| z %.2e L_true %.2e L_obs %.2e sigma %.2e; "
                  "nearest L_obs to its edge %.2e" % (variant, fix_sch_al, S, M, host[6][..., 0].sum(), host[6][..., 1].sum(),
                                                      (host[5] != 0).sum(), *worst, gap))
            assert host[6][..., 0].sum() > 2500 and host[6][..., 1].sum() > 100
            d, h = mock.compact_cut(*dev), mock.compact_cut(*host)                # kept order: above, then below, in index order
            np.testing.assert_array_equal(d[5], h[5])
            for key in ("kept", "n_scattered_in", "n_candidates"):
                np.testing.assert_array_equal(d[6][key], h[6][key])
            assert 0 < h[6]["n_scattered_in"].sum() < h[6]["kept"].sum() < host[6].sum()
            full = gen.draw_cut(th, SEED, rid)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(full[:6], d[:6]))
            # piece "above": lf_mock_draw_err's true draws, bit for bit
            plain = gen.draw_noisy(th, SEED, rid, count=dev[6][..., 0])
            above = np.repeat(np.tile([True, False], dev[6].size // 2), dev[6].ravel())
            assert dev[0][above].tobytes() == plain[0].tobytes() and dev[1][above].tobytes() == plain[1].tobytes()
        finally:
            gen.close()


@functools.lru_cache(maxsize=None)
def _count_case(variant, piece):
    inp = K.inputs(variant, 23)
    nodes, sig = K.table(7)
    tw = K.arm(mock.MockTwin(inp), inp, nodes, sig)
    rid = np.arange(5, dtype=np.int64) + 50 * piece
    th = K.rows_for_counts(tw, variant, (0, 1, 255, 256, 257), piece, SEED, rid)
    host, gap = K.edge_gap(tw, th, SEED, rid)
    np.testing.assert_array_equal(host[6][:, 0, piece], [0, 1, 255, 256, 257])
    return inp, (nodes, sig), th, rid, host, gap


@pytest.mark.parametrize("piece", [0, 1])
@pytest.mark.parametrize("variant", ["free", "fixcomp", "zevol"])
def test_draw_counts_at_the_edges_of_a_workgroup(variant, piece):
    inp, table, th, rid, host, gap = _count_case(variant, piece)
    gen = K.arm(mock.MockGenerator(inp), inp, *table)
    try:
        _agree(gen.candidates_cut(th, SEED, rid), host, gap)
        for i in range(5):                                                       # each count alone in its launch
            one = gen.candidates_cut(th[i:i + 1], SEED, rid[i:i + 1])
            np.testing.assert_array_equal(one[6][0], host[6][i])
    finally:
        gen.close()


@functools.lru_cache(maxsize=None)
def _hist_case(variant):
    """rows whose candidate counts of field 0 cover every launch shape of lf_mock_hist_cut in each piece, asserted on the twin"""
    inp = K.inputs(variant, 23)
    nodes, sig = K.table(64)
    tw = K.arm(mock.MockTwin(inp), inp, nodes, sig)
    th = np.concatenate([K.rows_for_means(tw, variant, False, (0.0, 100.0, 6000.0, 10000.0), 0, seed=7),
                         K.rows_for_means(tw, variant, False, (100.0, 6000.0, 10000.0), 1, seed=8)])
    host = tw.candidates_cut(th, SEED)
    for p in range(2):
        n = host[6][:, 0, p]
        assert (n == 0).any() and ((n > 0) & (n < 256)).any() and (n > 2 * 4096).any()
        assert ((n > 4096) & (n < 2 * 4096) & (n % 256 != 0)).any()
    return inp, (nodes, sig), th, mock.compact_cut(*host)


@pytest.mark.parametrize("nbins", [1, 1022])
@pytest.mark.parametrize("variant", ["free", "fixcomp", "zevol"])
def test_hist_and_kept_totals_equal_the_twins_exactly(variant, nbins):
    inp, table, th, kept = _hist_case(variant)
    Lobs, off = kept[2], kept[5]
    lo, hi = float(Lobs.min()), float(Lobs.max())
    for shift in (0.30, 0.31, 0.32, 0.33):      # (edges of the test's choosing: the first set clear of the twin's sources)
        edges = np.linspace(lo + shift, hi - 0.2, nbins + 1)
        i = np.clip(np.searchsorted(edges, Lobs), 1, nbins)
        gap = float(np.minimum(np.abs(Lobs - edges[i - 1]), np.abs(edges[i] - Lobs)).min())
        if gap > EDGE_MARGIN:
            break
    print("%s nbins=%d: %d kept sources, nearest L_obs to a bin edge %.3e" % (variant, nbins, Lobs.size, gap))
    assert gap > EDGE_MARGIN                    # the precondition: no kept source of the twin's within 1e-9 of a bin edge
    want = mock.bin_sources(Lobs, off, edges).reshape(len(th), -1, nbins + 2)
    assert want[..., 0].sum() > 0 and want[..., -1].sum() > 0
    gen = K.arm(mock.MockGenerator(inp), inp, *table)
    try:
        got, tot = gen.hist_cut(th, edges, SEED)
        np.testing.assert_array_equal(got, want)
        np.testing.assert_array_equal(tot, kept[6]["kept"])
        np.testing.assert_array_equal(got.sum(axis=2), tot)
    finally:
        gen.close()


def test_an_all_zero_table_gives_lf_mock_hist_bit_for_bit():
    inp, (nodes, sig), th, _ = _hist_case("zevol")
    gen = K.arm(mock.MockGenerator(inp), inp, nodes, np.zeros_like(sig), H=1.0)
    try:
        for edges in (np.linspace(41.0, 44.0, 2), np.linspace(41.5, 43.5, 1023), np.linspace(41.6, 43.0, 38)):
            (a, tot), b = gen.hist_cut(th, edges, SEED), gen.hist(th, edges, SEED)
            assert a.tobytes() == b.tobytes() and a.sum() > 10000
            np.testing.assert_array_equal(tot, gen.counts(th, SEED)[1])
        d, p = gen.draw_cut(th[1:3], SEED), gen.draw(th[1:3], SEED)
        assert d[0].tobytes() == p[0].tobytes() and d[1].tobytes() == d[2].tobytes() == p[1].tobytes()
        assert not d[6]["n_cand"][..., 1].any() and not d[3].any()
    finally:
        gen.close()


def test_a_row_does_not_depend_on_its_batch():
    inp, tw, gen = _pair("zevol", 23, 64)
    rng = np.random.default_rng(3)
    th = K.rows_for_means(tw, "zevol", False, tuple(rng.uniform(200.0, 2000.0, 64)), 0, seed=9)
    rid = rng.integers(0, 1 << 62, 64)
    edges = np.linspace(41.5, 43.5, 41)
    nf = gen.nf
    try:
        big, hbig = gen.draw_cut(th, 77, rid), gen.hist_cut(th, edges, 77, rid)
        again, hagain = gen.draw_cut(th, 77, rid), gen.hist_cut(th, edges, 77, rid)
        for a, b in zip(big[:6], again[:6]):
            assert a.tobytes() == b.tobytes()
        assert hbig[0].tobytes() == hagain[0].tobytes() and hbig[1].tobytes() == hagain[1].tobytes()
        np.testing.assert_array_equal(hbig[1], big[6]["kept"])
        perm = rng.permutation(64)
        sh, hsh = gen.draw_cut(th[perm], 77, rid[perm]), gen.hist_cut(th[perm], edges, 77, rid[perm])
        for i in (0, 37, 63):
            one = gen.draw_cut(th[i:i + 1], 77, rid[i:i + 1])
            p = int(np.flatnonzero(perm == i)[0])
            lo, hi, slo, shi = big[5][i * nf], big[5][(i + 1) * nf], sh[5][p * nf], sh[5][(p + 1) * nf]
            assert hi > lo and one[6]["n_scattered_in"].sum() > 0
            for a, b, c in zip(one[:5], big[:5], sh[:5]):
                assert a.tobytes() == b[lo:hi].tobytes() == c[slo:shi].tobytes()
            for key in ("n_cand", "mean", "kept"):
                assert one[6][key][0].tobytes() == big[6][key][i].tobytes() == sh[6][key][p].tobytes()
            h1 = gen.hist_cut(th[i:i + 1], edges, 77, rid[i:i + 1])
            assert h1[0][0].tobytes() == hbig[0][i].tobytes() == hsh[0][p].tobytes()
            assert h1[1][0].tobytes() == hbig[1][i].tobytes() == hsh[1][p].tobytes()
    finally:
        gen.close()


def test_every_refusal_names_the_problem_and_leaves_the_handle_usable():
    inp = K.inputs("fixcomp", 5)
    nodes, sig = K.table(3)
    tw, gen = mock.MockTwin(inp), mock.MockGenerator(inp)
    lib, h, nf, S = gen._lib, gen._h, gen.nf, gen.S
    th = synth.walkers("fixcomp", 2, seed=5)
    R = 2
    ip = lambda a: a.ctypes.data_as(capi._c_int64_p)                 # noqa: E731
    i32 = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))  # noqa: E731
    P = capi._ptr
    lb = mock.band_grid(inp, 1.0)
    ipb = mock.band_integ_part(inp, lb)
    edges = np.linspace(41.0, 44.0, 5)
    hist, kept = np.empty(R * nf * 6, dtype=np.int64), np.empty(R * nf, dtype=np.int64)
    ncand, mean = np.empty(R * nf * 2, dtype=np.int64), np.empty(R * nf * 2)
    cap = 1 << 16
    buf = [np.empty(cap) for _ in range(4)]
    fld, keep = np.empty(cap, dtype=np.int32), np.empty(cap, dtype=np.int32)

    def refused(rc, pattern):
        assert rc == capi.LF_ERR_ARG
        msg = lib.lf_mock_last_error(h).decode()
        assert pattern in msg, msg

    def draw(theta=th, rows=R, c=cap, z=buf[0], k=keep, n=ncand):
        return lib.lf_mock_draw_cut(h, P(theta), rows, None, 1, c, P(z), P(buf[1]), P(buf[2]), P(buf[3]), i32(fld),
                                    i32(k) if k is not None else None, ip(n) if n is not None else None, P(mean), ip(kept))

    def hst(theta=th, nb=4, e=edges, k=kept):
        return lib.lf_mock_hist_cut(h, P(theta), R, None, 1, nb, P(e), ip(hist), ip(k) if k is not None else None)

    try:
        refused(lib.lf_mock_set_cut_band(h, P(lb), P(ipb)), "no error model")
        refused(draw(), "no error model")
        refused(hst(), "no error model")
        gen.set_error_model(nodes, sig)
        tw.set_error_model(nodes, sig)
        refused(draw(), "no cut band")
        refused(hst(), "no cut band")
        refused(lib.lf_mock_set_cut_band(h, None, P(ipb)), "logLb is NULL")
        refused(lib.lf_mock_set_cut_band(h, P(lb), None), "need integ_part_b")
        bad = lb.copy()
        bad[-1, 2] += 1e-9
        refused(lib.lf_mock_set_cut_band(h, P(bad), P(ipb)), "column 2: row S - 1 of logLb must equal row 0 of logL")
        bad = lb.copy()
        bad[2, 1] = bad[1, 1]
        refused(lib.lf_mock_set_cut_band(h, P(bad), P(ipb)), "column 1 node 2: the band's luminosity nodes must be finite and strictly")
        bad = lb.copy()
        bad[0, 3] = np.nan
        refused(lib.lf_mock_set_cut_band(h, P(bad), P(ipb)), "column 3 node 0")
        bad = ipb.copy()
        bad[1, 0, 0] = -1.0
        refused(lib.lf_mock_set_cut_band(h, P(lb), P(bad)), "field 1: integ_part_b must be finite and >= 0")
        with pytest.raises(mock.MockError, match=r"\(S, S\)"):
            gen.set_cut_band(lb[:-1], ipb)
        with pytest.raises(mock.MockError, match=r"\(nf, S, S\)"):
            gen.set_cut_band(lb, ipb[:1])
        refused(draw(), "no cut band")                                    # a refused band leaves none
        gen.set_cut_band(lb, ipb)
        tw.set_cut_band(lb, ipb)
        ref = gen.draw_cut(th, 9)
        want = tw.draw_cut(th, 9)
        np.testing.assert_array_equal(ref[5], want[5])
        assert ref[2].size > 10
        refused(draw(theta=None), "theta is NULL")
        refused(draw(rows=0), "R must be")
        refused(draw(n=None), "n_cand or mean is NULL")
        refused(draw(c=-1), "cap must be >= 0")
        refused(draw(k=None), "NULL")
        assert draw(c=0, k=None) == capi.LF_OK and ncand.sum() > 0      # cap = 0: the counts alone, no array is read
        nonfin = th.copy()
        nonfin[1, 2] = np.inf
        refused(hst(theta=nonfin), "row 1")
        big = th.copy()
        big[0, 1] = 40.0
        refused(hst(theta=big), 'row 0 field 0')
        refused(hst(theta=big), '(piece "above")')
        refused(draw(theta=big), '(piece "above")')
        wide = np.linspace(41.0, 44.0, mock.MAX_BINS + 2)
        refused(lib.lf_mock_hist_cut(h, P(th), R, None, 1, mock.MAX_BINS + 1, P(wide), ip(hist), ip(kept)), "nbins")
        refused(hst(nb=0), "nbins")
        refused(hst(k=None), "NULL")
        refused(hst(e=edges[::-1].copy()), "edges must be finite and non-decreasing")
        # piece "below" alone above the cap: a deep band under a steep faint end
        deep = mock.band_grid(inp, 6.0)
        gen.set_cut_band(deep, mock.band_integ_part(inp, deep))
        th2 = th.copy()
        th2[0, 2] = -2.9
        th2[0, 1] += np.log10(0.9 * mock.MAX_MEAN / tw.means(th2)[0, 0])
        refused(hst(theta=th2), 'row 0 field 0')
        refused(hst(theta=th2), '(piece "below")')
        gen.set_cut_band(lb, ipb)
        after = gen.draw_cut(th, 9)
        for a, b in zip(ref[:6], after[:6]):
            assert a.tobytes() == b.tobytes()
        gen.set_error_model(nodes, sig)                                   # a new error model clears the band
        with pytest.raises(mock.MockError, match="no cut band"):
            gen.draw_cut(th, 9)
    finally:
        gen.close()


def test_the_model_class_on_the_device_and_on_the_host():
    from test_mock_cut_cpu import _class_object
    o, theta = _class_object()
    try:
        kw = dict(ndraws=16, seed=31, noise="catalogue", cut=True)
        np.random.seed(5)
        dev = o.posterior_predictive(device=True, **kw)
        np.random.seed(5)
        host = o.posterior_predictive(device=False, **kw)
        np.testing.assert_array_equal(dev["replicated"], host["replicated"])
        np.testing.assert_array_equal(dev["replicated_kept"], host["replicated_kept"])
        np.testing.assert_array_equal(dev["replicated_kept"], dev["replicated_total"])
        np.testing.assert_allclose(dev["expected"], host["expected"], rtol=1e-12, atol=0)
        assert dev["cut"] is True and dev["replicated"].sum() > 20000
        np.random.seed(5)
        plain = o.posterior_predictive(device=True, ndraws=16, seed=31, noise="catalogue")
        assert "cut" not in plain and not np.array_equal(plain["replicated"], dev["replicated"])
        a = o.mock_catalogue(theta, seed=8, device=True, cut=True)
        b = o.mock_catalogue(theta, seed=8, device=False, cut=True)
        np.testing.assert_array_equal(a["field_ind"], b["field_ind"])
        np.testing.assert_array_equal(a["n_candidates"], b["n_candidates"])
        np.testing.assert_array_equal(a["n_scattered_in"], b["n_scattered_in"])
        assert a["n_scattered_in"].sum() > 0
        for f in range(o.nfields):
            for k in ("z", "lum", "lum_e", "lum_true"):
                np.testing.assert_allclose(a[k][f], b[k][f], rtol=0, atol=TOL)
    finally:
        o.close()
