"""The mocks binned in redshift and luminosity on the device (lf_mock_hist2, lf_mock_hist2_err, lf_mock_hist2_cut;
csrc/lf_mock_hist2.h).  The reference is the binning (mock.bin_sources2) of the device's OWN draw,
integer for integer - the twin's draws are only within 1e-12 of the device's and cannot decide a source at an edge.  Per
process and variant: the 2-D histogram, its marginal over redshift against the existing 1-D entry with the same seed, its
total against the counts (the kept counts of the cut process), and a second call.  Then the edges of a workgroup's chunk
through the explicit counts, the tile shapes (9 slots, a small odd tile, exactly 8192 slots, one long axis), edges taken from
drawn values, rows and fields without mass, the refusals, and the model class."""
import functools

import numpy as np
import pytest

import lf_mockcutlib as K
import lf_mockproblib as M
from lumfuncmcmc_amd import capi, mock, synth

pytestmark = pytest.mark.gpu
SEED = 1234
RID = np.array([100, 1 << 40, 7], dtype=np.int64)
VARIANTS = ("free", "fixcomp", "zevol")
C = mock.HIST_CHUNK


@functools.lru_cache(maxsize=None)
def _rows(variant):
    return M.scaled_rows(mock.MockTwin(M.edge_inputs(variant, 257)), variant, (3000.0, 300.0, 5.0))


def _armed(variant, inp=None):
    """a device generator on edge_inputs(variant, 257) with an error model and the band of the cut process"""
    inp = M.edge_inputs(variant, 257) if inp is None else inp
    return K.arm(mock.MockGenerator(inp), inp, *K.table(7))


def _drawn(gen, process, th, rid, count=None):
    """(z, L, offsets, totals [R, nf]) of the device's own draw of the process"""
    if process == "plain":
        z, L, fld, off = gen.draw(th, SEED, rid, count)
    elif process == "noisy":
        z, _, L, sg, fld, off = gen.draw_noisy(th, SEED, rid, count)
    else:
        z, _, L, sg, fld, off, info = gen.draw_cut(th, SEED, rid)
        return z, L, off, info["kept"]
    return z, L, off, np.diff(off).reshape(len(th), -1)


def _hist2(gen, process, th, ze, e, rid, count=None):
    if process == "plain":
        return gen.hist2(th, ze, e, SEED, rid, count), None
    if process == "noisy":
        return gen.hist2_noisy(th, ze, e, SEED, rid, count), None
    return gen.hist2_cut(th, ze, e, SEED, rid)


def _grid(z, L, nz, nl):
    return np.linspace(z.min() + 0.01, z.max() - 0.01, nz + 1), np.linspace(L.min() + 0.1, L.max() - 0.2, nl + 1)


def _check(gen, process, th, rid, ze, e, count=None):
    z, L, off, tot = _drawn(gen, process, th, rid, count)
    got, kept = _hist2(gen, process, th, ze, e, rid, count)
    assert got.shape == (len(th), gen.nf, len(ze) + 1, len(e) + 1) and got.dtype == np.int64
    np.testing.assert_array_equal(got, mock.bin_sources2(z, L, off, ze, e).reshape(got.shape))
    np.testing.assert_array_equal(got.sum(axis=(2, 3)), tot)
    if kept is not None:
        np.testing.assert_array_equal(kept, tot)
    return got, (z, L, off)


@pytest.mark.parametrize("process", ["plain", "noisy", "cut"])
@pytest.mark.parametrize("variant", VARIANTS)
def test_hist2_is_the_binning_of_the_devices_own_draw(variant, process):
    gen = _armed(variant)
    th = _rows(variant)
    try:
        z, L, off, tot = _drawn(gen, process, th, RID)
        ze, e = _grid(z, L, 10, 20)
        got, _ = _check(gen, process, th, RID, ze, e)
        one = {"plain": gen.hist, "noisy": gen.hist_noisy, "cut": lambda *a: gen.hist_cut(*a)[0]}[process](th, e, SEED, RID)
        np.testing.assert_array_equal(got.sum(axis=2), one)
        again, _ = _hist2(gen, process, th, ze, e, RID)
        assert again.tobytes() == got.tobytes()
        assert got.sum() > 3000 and got[:, :, 0].sum() > 0 and got[:, :, -1].sum() > 0 and got[..., 0].sum() > 0 and got[..., -1].sum() > 0
    finally:
        gen.close()


@pytest.mark.parametrize("variant", VARIANTS)
def test_the_cut_process_with_a_populated_band(variant):
    """grids with their own lower edge per redshift column (lf_mockcutlib.inputs): piece "below" has hundreds of candidates"""
    inp = K.inputs(variant, 23)
    tw = K.arm(mock.MockTwin(inp), inp, *K.table(64))
    th = K.rows_for_means(tw, variant, False, (3000.0, 6000.0, 300.0, 0.0), 0)
    rid = np.arange(100, 104, dtype=np.int64)
    gen = K.arm(mock.MockGenerator(inp), inp, *K.table(64))
    try:
        z, L, off, tot = _drawn(gen, "cut", th, rid)
        info = gen.draw_cut(th, SEED, rid)[6]
        assert info["n_cand"][..., 1].sum() > 100 and info["n_scattered_in"].sum() > 0 and (info["n_cand"][..., 0] > C).any()
        ze, e = _grid(z, L, 7, 11)
        got, _ = _check(gen, "cut", th, rid, ze, e)
        np.testing.assert_array_equal(got.sum(axis=2), gen.hist_cut(th, e, SEED, rid)[0])
        assert not got[3].any()
    finally:
        gen.close()


@pytest.mark.parametrize("process", ["plain", "noisy"])
def test_counts_at_the_edges_of_a_workgroups_chunk(process):
    gen = _armed("zevol")
    th = np.concatenate([_rows("zevol"), _rows("zevol")[:1]])
    rid = np.array([100, 1 << 40, 7, 8], dtype=np.int64)
    # per (row, field); a pair without sources first, in the middle and last
    count = np.array([[0, 1], [C - 1, C], [0, C + 1], [2 * C + 3, 0]], dtype=np.int64)
    try:
        z, L, off, tot = _drawn(gen, process, th, rid, count)
        np.testing.assert_array_equal(tot, count)
        ze, e = _grid(z, L, 6, 9)
        got, _ = _check(gen, process, th, rid, ze, e, count)
        assert not got[0, 0].any() and not got[2, 0].any() and not got[3, 1].any() and got[0, 1].sum() == 1
        for r in range(4):                                                      # each row alone in its launch
            one, _ = _hist2(gen, process, th[r:r + 1], ze, e, rid[r:r + 1], count[r:r + 1])
            assert one[0].tobytes() == got[r].tobytes()
    finally:
        gen.close()


@pytest.mark.parametrize("nz,nl", [(1, 1), (3, 5), (62, 126), (1022, 6)])
def test_tile_shapes(nz, nl):
    assert (nz + 2) * (nl + 2) <= mock.MAX_SLOTS2
    gen = _armed("zevol")
    th = _rows("zevol")
    try:
        for process in ("plain", "noisy", "cut"):
            z, L, off, tot = _drawn(gen, process, th, RID)
            ze, e = _grid(z, L, nz, nl)
            got, _ = _check(gen, process, th, RID, ze, e)
            assert got[:, :, 1:-1, 1:-1].sum() > 2000
    finally:
        gen.close()


def test_edges_taken_from_drawn_values_and_edges_off_the_data():
    gen = _armed("fixcomp")
    th = _rows("fixcomp")
    try:
        for process in ("plain", "noisy", "cut"):
            z, L, off, tot = _drawn(gen, process, th, RID)
            zs, Ls = np.sort(z[[5, 700]]), np.sort(L[[11, 900]])
            assert zs[0] < zs[1] and Ls[0] < Ls[1]
            got, _ = _check(gen, process, th, RID, zs, Ls)
            # a source on an edge is in the upper slot: slot 0 holds the sources strictly below the first edge
            assert got[:, :, 0].sum() == (z < zs[0]).sum() and got[:, :, 2].sum() == (z >= zs[1]).sum()
            assert got[..., 0].sum() == (L < Ls[0]).sum() and got[..., 2].sum() == (L >= Ls[1]).sum()
            assert got[:, :, 1].sum() == ((z >= zs[0]) & (z < zs[1])).sum() >= 1
            low, _ = _check(gen, process, th, RID, np.array([-2.0, -1.0]), np.array([1.0, 2.0, 3.0]))
            assert low[:, :, -1, -1].sum() == low.sum() == tot.sum()
            high, _ = _check(gen, process, th, RID, np.array([50.0, 60.0, 60.0]), np.array([90.0, 91.0]))
            assert high[:, :, 0, 0].sum() == high.sum() == tot.sum()
    finally:
        gen.close()


def test_a_field_and_a_row_without_mass_leave_their_tiles_zero():
    inp = dict(M.edge_inputs("fixcomp", 257))
    ip = np.array(inp["integ_part"], dtype=np.float64, copy=True)
    ip[1] = 0.0                                                                  # field 1 has no mass in any row
    inp["integ_part"] = ip
    tw = mock.MockTwin(inp)
    th = M.scaled_rows(tw, "fixcomp", (0.0, 3000.0, 0.0, 300.0, 0.0))
    gen = _armed("fixcomp", inp)
    try:
        mean, n = gen.counts(th, SEED)
        assert (mean[:, 1] == 0).all() and (mean[[0, 2, 4]] == 0).all() and (n[[1, 3], 0] > 0).all()
        for process in ("plain", "noisy", "cut"):
            z, L, off, tot = _drawn(gen, process, th, None)
            ze, e = _grid(z, L, 4, 6)
            got, _ = _check(gen, process, th, None, ze, e)
            assert not got[:, 1].any() and not got[[0, 2, 4]].any() and got[1, 0].sum() > 1000
    finally:
        gen.close()


def test_every_refusal_names_the_problem_and_leaves_the_handle_usable():
    inp = M.edge_inputs("fixcomp", 257)
    gen = mock.MockGenerator(inp)
    lib, h, nf = gen._lib, gen._h, gen.nf
    th = _rows("fixcomp")
    R = len(th)
    ip = lambda a: a.ctypes.data_as(capi._c_int64_p)                 # noqa: E731
    P = capi._ptr
    ze, e = np.linspace(2.0, 3.4, 4), np.linspace(41.8, 43.2, 6)
    hist, kept = np.empty(R * nf * mock.MAX_SLOTS2, dtype=np.int64), np.empty(R * nf, dtype=np.int64)
    long_ = np.linspace(0.0, 1.0, 4096)

    def refused(rc, pattern):
        assert rc == capi.LF_ERR_ARG
        msg = lib.lf_mock_last_error(h).decode()
        assert pattern in msg, msg

    def plain(nz=3, zed=ze, nl=5, ed=e, entry=None, count=None, theta=th):
        fn = entry or lib.lf_mock_hist2
        return fn(h, P(theta), R, None, SEED, ip(count) if count is not None else None, nz, P(zed), nl, P(ed), ip(hist))

    def cut(nz=3, zed=ze, nl=5, ed=e, k=kept):
        return lib.lf_mock_hist2_cut(h, P(th), R, None, SEED, nz, P(zed), nl, P(ed), ip(hist), ip(k) if k is not None else None)

    try:
        ref = gen.hist2(th, ze, e, SEED)
        assert ref.sum() > 3000
        refused(plain(nz=1, nl=2729, ed=long_), "8193 slots: the limit is 8192")                  # 3 x 2731
        refused(plain(nz=32, nl=239, ed=long_), "8194 slots: the limit is 8192")                  # 34 x 241, both axes in range
        assert plain(nz=62, zed=long_, nl=126, ed=long_) == capi.LF_OK                            # 64 x 128 = 8192
        refused(plain(nz=0), "nz must be in 1..1022")
        refused(plain(nl=0), "nl must be in 1..1022")
        refused(plain(nz=1023, zed=long_, nl=1), "nz must be in 1..1022")
        refused(plain(nz=1, nl=1023, ed=long_), "nl must be in 1..1022")
        bad = ze.copy()
        bad[2] = np.nan
        refused(plain(zed=bad), "z_edges must be finite and non-decreasing")
        bad = e.copy()
        bad[1] = np.inf
        refused(plain(ed=bad), "edges must be finite and non-decreasing")
        refused(plain(zed=ze[::-1].copy()), "z_edges must be finite and non-decreasing")
        refused(plain(ed=e[::-1].copy()), "edges must be finite and non-decreasing")
        refused(lib.lf_mock_hist2(h, P(th), R, None, SEED, None, 3, None, 5, P(e), ip(hist)), "NULL")
        refused(lib.lf_mock_hist2(h, None, R, None, SEED, None, 3, P(ze), 5, P(e), ip(hist)), "theta is NULL")
        refused(plain(count=np.full((R, nf), -1, dtype=np.int64)), "row 0 field 0: count out of range")
        nonfin = th.copy()
        nonfin[1, 0] = np.nan
        refused(plain(theta=nonfin), "row 1")
        refused(plain(entry=lib.lf_mock_hist2_err), "no error model")
        refused(cut(), "no error model")
        nodes, sig = K.table(7)
        gen.set_error_model(nodes, sig)
        assert plain(entry=lib.lf_mock_hist2_err) == capi.LF_OK
        refused(cut(), "no cut band")
        with pytest.raises(mock.MockError, match="no cut band"):
            gen.set_cut_band(None)
            gen.hist2_cut(th, ze, e, SEED)
        K.arm(gen, inp, nodes, sig)
        refused(cut(k=None), "NULL")
        refused(cut(nz=0), "nz must be")
        assert cut() == capi.LF_OK
        assert gen.hist2(th, ze, e, SEED).tobytes() == ref.tobytes()
    finally:
        gen.close()


def test_the_model_class_on_the_device_and_on_the_host():
    import lf_deconvlib as L
    cat = synth.catalogue(400, seed=17)
    cat["lum_e"] = np.random.default_rng(5).uniform(0.05, 0.3, 400)
    o = L.fixcomp_model(cat)
    theta = np.array([synth.LSTAR, synth.PHISTAR - 1.0, synth.SCH_AL])
    rng = np.random.default_rng(6)
    rows = theta[None] + rng.normal(0.0, 0.02, (50, 3))
    o.samples = np.concatenate([rows, -0.5 * rng.chisquare(3, 50)[:, None]], axis=1)
    try:
        for noise in (None, "catalogue"):
            kw = dict(ndraws=12, seed=31, noise=noise)
            np.random.seed(5)
            dev = o.posterior_predictive(device=True, z_edges="auto", **kw)
            np.random.seed(5)
            host = o.posterior_predictive(device=False, z_edges="auto", **kw)
            np.random.seed(5)
            old = o.posterior_predictive(device=True, **kw)
            np.testing.assert_array_equal(dev["observed_2d"], host["observed_2d"])
            assert dev["z_edges"].tobytes() == host["z_edges"].tobytes() == np.linspace(o.zmin, o.zmax, 11).tobytes()
            assert dev["replicated_2d"].shape == (12, o.nfields, 12, 22) and dev["replicated_2d"].sum() > 2000
            np.testing.assert_array_equal(dev["replicated_2d"].sum(axis=2), dev["replicated"])
            np.testing.assert_array_equal(dev["replicated_2d"].sum(axis=3), dev["replicated_z"])
            np.testing.assert_array_equal(dev["replicated_2d"].sum(axis=(2, 3)), dev["replicated_total"])
            assert sorted(set(dev) - set(old)) == sorted(set(host) - set(old)) and "deviance" in dev and "z_edges" not in old
            for k, v in old.items():                                             # the 1-D entries: the old path's integers
                assert np.array_equal(dev[k], v) if k != "sigma_model" else True, k
            np.testing.assert_array_equal(dev["p_deviance"], np.mean(dev["replicated_deviance"] >= dev["deviance"][None], axis=0))
    finally:
        o.close()


def test_the_model_class_under_the_cut():
    from test_mock_cut_cpu import _class_object
    o, theta = _class_object()
    try:
        kw = dict(ndraws=8, seed=31, noise="catalogue", cut=True)
        np.random.seed(5)
        dev = o.posterior_predictive(device=True, z_edges="auto", **kw)
        np.random.seed(5)
        host = o.posterior_predictive(device=False, z_edges="auto", **kw)
        np.random.seed(5)
        old = o.posterior_predictive(device=True, **kw)
        np.testing.assert_array_equal(dev["observed_2d"], host["observed_2d"])
        np.testing.assert_array_equal(dev["replicated_2d"].sum(axis=2), old["replicated"])
        np.testing.assert_array_equal(dev["replicated_kept"], old["replicated_kept"])
        np.testing.assert_array_equal(dev["replicated_2d"].sum(axis=(2, 3)), dev["replicated_kept"])
        assert dev["cut"] is True and dev["replicated_2d"].sum() > 5000
    finally:
        o.close()
