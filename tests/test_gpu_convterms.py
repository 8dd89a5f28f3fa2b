"""The wide, tiled, per-source-posterior and binned copies of the convolved likelihood's node loop (csrc/lf_deconv_wide.h,
csrc/lf_deconv_tile.h, csrc/lf_lumpost.h, csrc/lf_vefftrue.h), one source per block on the GPU against 40-digit values
(inputs, references, yardsticks and caps: tests/lf_convproblib.py; the probe: tests/conv_probe.hip, compiled once per module
with the library's own flags and loaded after the library).

The library's own tests hold these kernels against NumPy twins that restate them branch for branch, at 1e-12 of a sum over
a well-behaved catalogue.  Here each source's value is read on its own, on the edge lattice of DESIGN.md section 3.13 and on
every wide class table; each test prints its measured maximum of err / yardstick and the input at the maximum, then asserts it
against the cap: 4 x the figure of the same expression in NumPy binary64, never below 2.  DESIGN.md section 3.27 records the
figures."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import lf_convproblib as C
from lumfuncmcmc_amd import build, capi, deconv as D

P = C.P
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_dp = ctypes.POINTER(ctypes.c_double)
FILL = -777.0
TILED = (P.FIXCOMP, P.ZEVOL)
WIDE_KEYS = tuple(("wide", c) for c in range(5))


def _d(a):
    return None if a is None else a.ctypes.data_as(_dp)


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("conv_probe") / "conv_probe.so")
    subprocess.run([build.hipcc()] + build.CXXFLAGS + ["-fPIC", "-shared", "-o", so, os.path.join(ROOT, "tests", "conv_probe.hip")], check=True)
    capi.load()          # first: it brings in the process's one HIP runtime, which the probe must share
    lib = ctypes.CDLL(so)
    assert lib.cp_device_count() >= 1, "no GPU"
    assert [lib.cp_layout(k) for k in range(6)] == [P.D_SLOTS, 8, 2, 16, 32, 144]
    return lib


@pytest.fixture(scope="module")
def gprobe(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("grad_probe") / "grad_probe.so")
    subprocess.run([build.hipcc()] + build.CXXFLAGS + ["-fPIC", "-shared", "-o", so, os.path.join(ROOT, "tests", "grad_probe.hip")], check=True)
    capi.load()
    return ctypes.CDLL(so)


def model(variant):
    return C.L.f64([variant, 0, P.synth.SCH_AL, P.KAPPA] + list(P.PIVOT_SETS[0]) + [P.FLIM0, P.ALPHA0, C.PV])


def src_of(variant, s):
    return C.L.f64(np.stack([s["lum"], s["z"] if variant == P.ZEVOL else s["logf"], s["P"], s["logf"], s["U"], s["sigma"]]))


def nodes_of(x, lnw):
    return C.L.f64(np.concatenate([x, lnw]))


def check(name, case, got, where=None):
    fig, i = C.L.measure(case, got)
    cap = C.CAPS[name]
    at = "" if where is None else " at %s" % (where(i),)
    print("%-12s %-8s table %-12s device max err / yard %9.3f (cap %g)%s: got %.17g ref %.17g"
          % (name, P.VNAME[case["variant"]], case["key"], fig, cap, at, np.ravel(got)[i], case["ref"][0][i]))
    assert fig <= cap, (name, fig, cap, i)
    return fig


def where_of(case, per=1):
    s, n = case["src"], case["src"]["n"]

    def at(i):
        b, it = np.unravel_index(i // per, (len(case["rows"]), n))
        return "row %d source %d (sigma %.17g, lum %r, logf %r; %d rises)%s" % (b, it, s["sigma"][it], s["lum"][it], s["logf"][it], case["rises"][it],
                                                                              " item %d" % (i % per) if per > 1 else "")
    return at


# ---------------------------------------------------------------------------------------------- cp_wide
def run_wide(lib, variant, rows, s, cls, nodes=None, lnprob=None):
    R, n = len(rows), s["n"]
    lnp = np.full(R, -123.5) if lnprob is None else C.L.f64(lnprob)
    part, gpart = np.full((R, n), FILL), np.full((R, n, P.D_SLOTS), FILL)
    K = 0 if nodes is None else len(nodes) // 2
    rc = lib.cp_wide(_d(model(variant)), _d(C.L.f64(rows)), _d(lnp), R, _d(src_of(variant, s)), n, cls, _d(nodes), K, _d(part), _d(gpart))
    assert rc == 0, rc
    return part, gpart


def test_the_librarys_class_tables_have_the_twins_bits(probe):
    for c in range(5):
        out = np.zeros(2 * 144)
        K = probe.cp_table(c, _d(out))
        x, lnw = D.wide_table(c)
        assert K == len(x) == C.WIDE_K[c] and np.array_equal(out[:K], x) and np.array_equal(out[K:2 * K], lnw)
    assert probe.cp_table(5, _d(out)) == -1


@pytest.mark.parametrize("variant", C.VARIANTS)
def test_wide_items(probe, variant):
    used = {P.FREE: 4, P.FIXCOMP: 2, P.ZEVOL: 4}[variant]
    for key in WIDE_KEYS:
        c = C.case(variant, key)
        cd = c["delta"]
        s, rows = cd["src"], cd["rows"]
        R = len(rows)
        th = np.concatenate([rows, rows[:1]])
        part, gpart = run_wide(probe, variant, th, s, key[1], lnprob=[-123.5] * R + [-np.inf])
        assert np.all(part[R] == FILL) and np.all(gpart[R] == FILL), "a block of a row whose lnprob is -inf must leave at once"
        assert np.all(gpart[:R, :, used:] == FILL) and np.all(gpart[:R, :, :used] != FILL) and np.all(part[:R] != FILL)
        got = gpart[:R].copy()
        got[:, :, used:] = 0.0
        check("delta_wide", cd, part[:R].ravel(), where_of(cd))
        check("grad_wide", c["grad"], got.ravel(), where_of(cd, P.D_SLOTS))


@pytest.mark.parametrize("variant", C.VARIANTS)
def test_wide_value_slot_has_the_narrow_kernels_bits_for_the_same_table(probe, gprobe, variant):
    """at K <= 32 lf_deconv_wide_part runs deconv_source on the table lf_deconv_part would: the same bits, slot by slot; so do
    the table with a node of weight 0 first, in the middle and last, and each node twice"""
    import test_gpu_gradterms as T
    s0 = C.lattice(variant)
    s = C.thin(s0, np.flatnonzero(s0["sigma"] > 0.0))             # (the wide list holds no source with sigma = 0)
    rows = P.deconv_rows(variant)
    for K in (4, 32):
        x, lnw = D.gauss_hermite(K)
        tabs = [(x, lnw)] + ([C.with_dead_node(x, lnw, pos) for pos in (0, 2, 4)] + [C.twice(x, lnw)] if K == 4 else [])
        for xx, ll in tabs:
            nodes = nodes_of(xx, ll)
            want = T.run_deconv(gprobe, variant, rows, s, nodes, len(xx))
            got = run_wide(probe, variant, rows, s, -1, nodes)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (variant, K, len(xx))


# ---------------------------------------------------------------------------------------------- cp_tile
def run_tile(lib, variant, rows, lnp, s, nodes):
    nrows, n = len(rows), s["n"]
    part = np.full((nrows, n), FILL)
    rc = lib.cp_tile(_d(model(variant)), _d(C.L.f64(rows)), _d(C.L.f64(lnp)), nrows, _d(src_of(variant, s)), n, _d(nodes), len(nodes) // 2, _d(part))
    assert rc == 0, rc
    return part


@pytest.mark.parametrize("K", [4, 32])
@pytest.mark.parametrize("variant", TILED)
def test_tile_items(probe, variant, K):
    cd = C.case(variant, K)["delta"]
    s, rows = cd["src"], cd["rows"]
    R = len(rows)
    # nine rows: the four of the case, a dead one among them, the four again in another order - a tile of 8 and one of 1
    order = [0, 1, -1, 2, 3, 3, 2, 1, 0]
    th = np.array([rows[max(j, 0)] for j in order])
    lnp = np.array([-np.inf if j < 0 else -123.5 for j in order])
    part = run_tile(probe, variant, th, lnp, s, cd["nodes"])
    assert np.all(part[2] == FILL), "a dead row's slots are left alone"
    got = np.array([part[order.index(b)] for b in range(R)])
    check("tile_delta", cd, got.ravel(), where_of(cd))
    for j, b in enumerate(order):                                 # the same bits at any place of any tile
        assert b < 0 or np.array_equal(part[j], got[b]), j
    off = s["sigma"] == 0.0
    assert off.sum() >= 10 and np.all(got[:, off] == 0.0) and not np.any(np.signbit(got[:, off]))


@pytest.mark.parametrize("variant", TILED)
def test_a_tiles_row_does_not_depend_on_its_neighbours(probe, variant):
    """A row's slot has the same bits alone in its tile at every position (all 8 single-live masks), with only the first or
    only the last row of the tile dead, and at nrows = 1, 8, 9; a dead row keeps the fill; the table with a node of weight 0
    and with each node twice behaves as lf_deconv_part's"""
    cd = C.case(variant, 4)["delta"]
    s, rows, nodes = cd["src"], cd["rows"], cd["nodes"]
    row = rows[1]
    alone = run_tile(probe, variant, row[None], [-123.5], s, nodes)[0]                     # nrows = 1
    assert np.all(alone != FILL)
    eight = np.tile(row, (8, 1))
    for pos in range(8):
        lnp = np.full(8, -np.inf)
        lnp[pos] = -50.0 - pos
        part = run_tile(probe, variant, eight, lnp, s, nodes)
        assert np.array_equal(part[pos], alone), pos
        assert np.all(np.delete(part, pos, axis=0) == FILL), pos
    mixed = np.array([rows[j % len(rows)] for j in range(9)])
    full = run_tile(probe, variant, mixed, np.full(9, -1.0), s, nodes)                     # nrows = 9, all live
    assert np.array_equal(full[1], alone) and np.array_equal(full[5], alone)
    for dead in (0, 7):                                                                    # first-dead and last-dead masks
        lnp = np.full(8, -1.0)
        lnp[dead] = np.nan if dead else -np.inf
        part = run_tile(probe, variant, mixed[:8], lnp, s, nodes)                          # nrows = 8
        assert np.all(part[dead] == FILL) and np.array_equal(np.delete(part, dead, axis=0), np.delete(full[:8], dead, axis=0)), dead
    x, lnw = nodes[:4], nodes[4:]
    for pos in (0, 2, 4):
        got = run_tile(probe, variant, mixed, np.full(9, -1.0), s, nodes_of(*C.with_dead_node(x, lnw, pos)))
        assert np.array_equal(got, full), pos
    d8 = run_tile(probe, variant, mixed, np.full(9, -1.0), s, nodes_of(*C.twice(x, lnw)))
    on = s["sigma"] > 0.0
    assert np.all(np.abs(d8[:, on] - (full[:, on] + np.log(2.0))) <= 8 * P.U53 * (np.abs(full[:, on]) + 1.0))


# ---------------------------------------------------------------------------------------------- cp_lumpost
def run_lumpost(lib, variant, rows, s, nodes, wide):
    R, n = len(rows), s["n"]
    e1, e2 = np.full((R, n), FILL), np.full((R, n), FILL)
    rc = lib.cp_lumpost(_d(model(variant)), _d(C.L.f64(rows)), R, _d(src_of(variant, s)), n, int(wide), _d(nodes), len(nodes) // 2, _d(e1), _d(e2))
    assert rc == 0, rc
    return e1, e2


def _moment_checks(c, e1, e2, route):
    s = c["e1"]["src"]
    off = s["sigma"] == 0.0
    # a source with sigma = 0 is skipped: its slots are never written (the library's m1, m2 are zeroed before the first launch
    # and lf_lumpost_fold leaves them alone: exactly 0, 0 - tests/test_gpu_lumpost.py); here its (e1, e2) count as (0, 0)
    assert np.all(e1[:, off] == FILL) and np.all(e2[:, off] == FILL) and np.all(e1[:, ~off] != FILL) and np.all(e2[:, ~off] != FILL)
    g1, g2 = np.where(off, 0.0, e1), np.where(off, 0.0, e2)
    check("e1_" + route, c["e1"], g1.ravel(), where_of(c["e1"]))
    check("e2_" + route, c["e2"], g2.ravel(), where_of(c["e1"]))
    normal = (np.abs(g1) >= 2.0 ** -1022) & (g2 >= 2.0 ** -1022) & (g1 * g1 >= 2.0 ** -1022)
    assert normal.sum() > 0.5 * (~off).sum() * len(g1) and np.all(g2[normal] >= (g1 * g1)[normal])
    return g1, g2


@pytest.mark.parametrize("variant", C.VARIANTS)
def test_lumpost_items(probe, variant):
    for key in (4, 32) + WIDE_KEYS:
        c = C.case(variant, key)
        wide = isinstance(key, tuple)
        s, rows, nodes = c["e1"]["src"], c["e1"]["rows"], c["e1"]["nodes"]
        e1, e2 = run_lumpost(probe, variant, rows, s, nodes, wide)
        _moment_checks(c, e1, e2, "wide" if wide else "narrow")
        if not wide:                       # the same table handed in by the other route: the same bits
            w1, w2 = run_lumpost(probe, variant, rows, s, nodes, True)
            assert np.array_equal(w1, e1) and np.array_equal(w2, e2), (variant, key)
    # a node of weight 0 is skipped; each node twice: the same moments (p_k halves, every value comes twice)
    c = C.case(variant, 4)
    s, rows, nodes = c["e1"]["src"], c["e1"]["rows"], c["e1"]["nodes"]
    want = run_lumpost(probe, variant, rows, s, nodes, False)
    for pos in (0, 2, 4):
        got = run_lumpost(probe, variant, rows, s, nodes_of(*C.with_dead_node(nodes[:4], nodes[4:], pos)), False)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), pos
    t1, t2 = run_lumpost(probe, variant, rows, s, nodes_of(*C.twice(nodes[:4], nodes[4:])), False)
    on = s["sigma"] > 0.0
    for t, w_, cs in ((t1, want[0], c["e1"]), (t2, want[1], c["e2"])):
        assert np.all(np.abs(t[:, on] - w_[:, on]) <= 4.0 * cs["yard"].reshape(w_.shape)[:, on])


# ---------------------------------------------------------------------------------------------- cp_vefftrue
def run_vefft(lib, variant, rows, s, nodes, wide, edges, per=1, own=True, lnprob=None):
    R, n = len(rows), s["n"]
    K = len(nodes) // 2
    edges = C.L.f64(edges)
    nbin = edges.shape[-1] - 1
    nch = n // per
    assert edges.shape == ((nch, nbin + 1) if own else (nbin + 1,))
    lnp = np.full(R, -123.5) if lnprob is None else C.L.f64(lnprob)
    partial = np.full((nch, 16, nbin), FILL)
    rc = lib.cp_vefftrue(_d(model(variant)), _d(C.L.f64(rows)), _d(lnp), R, _d(src_of(variant, s)), n, per, int(wide), _d(nodes), K, _d(edges),
                         nbin, int(own), _d(partial))
    assert rc == 0, rc
    assert np.all(partial[:, R:] == FILL)
    return partial[:, :R]


@pytest.mark.parametrize("variant", C.VARIANTS)
def test_vefftrue_nodes(probe, variant):
    for key in (4, 32) + WIDE_KEYS:
        c = C.case(variant, key)["prod"]
        wide = isinstance(key, tuple)
        s, rows, nodes, K = c["src"], c["rows"], c["nodes"], c["K"]
        ed = C.node_edges(s, nodes[:K])
        part = run_vefft(probe, variant, rows, s, nodes, wide, ed)                 # [n][R][K]
        assert np.all(part != FILL)
        got = np.ascontiguousarray(part.transpose(1, 0, 2))
        name = "node_wide" if wide else "node_narrow"
        check(name, c, got.ravel(), where_of(c, K))
        # a source's sum over its nodes against the reference's, in the sum of the nodes' yardsticks
        ref, yard = c["ref"][0].reshape(got.shape), c["yard"].reshape(got.shape)
        ok = np.all(np.isfinite(ref), axis=2)
        err = np.abs((got.sum(axis=2) - ref.sum(axis=2)) - c["ref"][1].reshape(got.shape).sum(axis=2))[ok]
        fig = float(np.max(err / (yard.sum(axis=2)[ok] + K * P.U53 * np.abs(ref).sum(axis=2)[ok])))
        print("%-12s %-8s table %-12s a source's sum over its nodes: max err / yard %.3f (cap %g)" % (name, P.VNAME[variant], key, fig, C.CAPS[name]))
        assert ok.sum() > 0.8 * ok.size and fig <= C.CAPS[name]
        # a source with sigma = 0 is one node: the others' bins are exactly 0
        off = s["sigma"] == 0.0
        assert np.all(part[off][:, :, 1:] == 0.0) and np.all(part[off][:, :, 0] > 0.0)
        # the factor question: no +inf and no 0 where the 40-digit product is a finite normal number
        normal = np.isfinite(ref) & (np.abs(ref) >= 2.0 ** -1022) & (np.abs(ref) < 1e300)
        assert np.all(np.isfinite(got[normal]) & (got[normal] > 0.0)), (variant, key)
    # a node of weight 0 contributes exactly 0; it moves the others one lane up, so the butterfly adds the same positive
    # addends in another association: the sum moves by at most log2(64) = 6 roundings, the quotient by 8 x 2^-53 of itself
    c = C.case(variant, 4)["prod"]
    s, rows, nodes = c["src"], c["rows"], c["nodes"]
    on = s["sigma"] > 0.0
    want = run_vefft(probe, variant, rows, s, nodes, False, C.node_edges(s, nodes[:4]))
    for pos in (0, 2, 4):
        x, lnw = C.with_dead_node(nodes[:4], nodes[4:], pos)
        got = run_vefft(probe, variant, rows, s, nodes_of(x, lnw), False, C.node_edges(s, x))
        assert np.all(got[on][:, :, pos] == 0.0) and not np.any(np.signbit(got[on][:, :, pos])), pos
        rest = np.delete(got[on], pos, axis=2)
        fin = np.isfinite(want[on])
        assert np.array_equal(rest[~fin], want[on][~fin]) and np.all(np.abs(rest[fin] - want[on][fin]) <= 8 * P.U53 * want[on][fin]), pos


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("variant", C.VARIANTS)
def test_vefftrue_chunk_order(probe, variant, wide):
    """chunks of 2, 3, 63, 64, 65 and 257 sources equal the sums of the one-source partials in the documented order - wave,
    then batch, the lower half-wave's source before the upper's - bit for bit: two sources per wave at K = 32, one source in
    three passes at K = 144; a dead row's slots are left alone"""
    rows = np.concatenate([P.deconv_rows(variant)[:2], P.deconv_rows(variant)[:1]])
    lnp = [-123.5, -5.0, -np.inf]
    x, lnw = C.table(("wide", 4) if wide else 32)
    nodes = nodes_of(x, lnw)
    s = C.chunk_sources(variant, 257, wide)
    ed = C.node_edges(C.thin(s, [0]), x)[0]
    one = run_vefft(probe, variant, rows, s, nodes, wide, ed, per=1, own=False, lnprob=lnp)          # [257][3][K]
    assert np.all(one[:, 2] == FILL) and np.all(one[:, :2] != FILL)
    assert np.mean(one[s["sigma"] > 0.0][:, :2] > 0.0) > 0.5          # (every bin holds a node of every source; far tails underflow)
    for n in (2, 3, 63, 64, 65, 257):
        sub = C.thin(s, np.arange(n))
        got = run_vefft(probe, variant, rows, sub, nodes, wide, ed, per=n, own=False, lnprob=lnp)    # [1][3][K]
        assert np.all(got[0, 2] == FILL)
        assert np.array_equal(got[0, :2], C.chunk_sum(one[:n, :2], n)), (variant, wide, n)


def test_entry_points_refuse_counts_beyond_their_buffers(probe):
    s = C.thin(C.lattice(P.FIXCOMP), np.arange(4))
    rows = P.deconv_rows(P.FIXCOMP)
    nodes = nodes_of(*D.gauss_hermite(4))
    m, src, th, lp = model(P.FIXCOMP), src_of(P.FIXCOMP, s), C.L.f64(rows), np.full(4, -1.0)
    out = np.zeros(4096)
    assert probe.cp_wide(_d(m), _d(th), _d(lp), 17, _d(src), 4, 0, None, 0, _d(out), _d(out)) == -1
    assert probe.cp_wide(_d(m), _d(th), _d(lp), 4, _d(src), 4, -1, _d(nodes), 145, _d(out), _d(out)) == -1
    assert probe.cp_tile(_d(model(P.FREE)), _d(th), _d(lp), 4, _d(src), 4, _d(nodes), 4, _d(out)) == -1
    assert probe.cp_tile(_d(m), _d(th), _d(lp), 4, _d(src), 4, _d(nodes), 33, _d(out)) == -1
    assert probe.cp_lumpost(_d(m), _d(th), 4, _d(src), 4, 0, _d(nodes), 33, _d(out), _d(out)) == -1
    ed = np.array([1.0, 2.0, 2.0, 3.0, 4.0])
    assert probe.cp_vefftrue(_d(m), _d(th), _d(lp), 4, _d(src), 4, 1, 0, _d(nodes), 4, _d(ed), 4, 0, _d(out)) == -1       # edges that do not ascend
    assert probe.cp_vefftrue(_d(m), _d(th), _d(lp), 4, _d(src), 4, 3, 0, _d(nodes), 4, _d(np.arange(5.0)), 4, 0, _d(out)) == -1
    assert probe.cp_vefftrue(_d(m), _d(th), _d(lp), 4, _d(src), 4, 1, 0, _d(nodes), 4, _d(np.arange(1026.0)), 1025, 0, _d(out)) == -1
