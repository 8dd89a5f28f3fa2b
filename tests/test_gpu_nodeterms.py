"""Piece B's grid-node forms (csrc/lf_kernels.h), one node at a time on the GPU against 40-digit values (inputs, references,
yardsticks and caps: tests/lf_nodeproblib.py; the probe kernels: tests/node_probe.hip, compiled once per module with the
library's own flags).

Every other GPU test of this arithmetic looks at a sum over 10 201 nodes at rtol 2e-13 .. 1e-12, in which an error confined
to one clamp or one form switch averages out.  Here field_sum<NF>, field_sum_bright<NF>, walker_vmin and the quadratics
are called directly, and the inline expressions of gridsum_body<VARIANT, TW> - the Schechter factor of FREE and FIXCOMP, the
column and the row form of the z-evolving node - are read from partials that hold one node's value and exact zeros.
Each test prints its measured maximum of err / yardstick and the input at the maximum, then asserts it against the cap:
4 x the figure of the same expression in NumPy binary64, never below 2.  DESIGN.md section 3.25 records the figures."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import lf_nodeproblib as N
from lumfuncmcmc_amd import build

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_dp, _ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
FREE, FIXCOMP, ZEVOL = 0, 1, 2
FILL = -12345.0


def _d(a):
    return a.ctypes.data_as(_dp)


def _i(a):
    return a.ctypes.data_as(_ip)


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("node_probe") / "node_probe.so")
    subprocess.run([build.hipcc()] + build.CXXFLAGS + ["-fPIC", "-shared", "-o", so, os.path.join(ROOT, "tests", "node_probe.hip")], check=True)
    lib = ctypes.CDLL(so)
    assert lib.np_device_count() >= 1, "no GPU"
    return lib


def layout(lib):
    names = ("REC", "CA0", "V0", "FSTRIDE", "R_LSTAR", "R_C0", "R_C1", "R_Q", "R_ALPHAC", "Z_AL", "Z_C1", "MODE_SKIP", "ZCOLS")
    return {n: lib.np_layout(k) for k, n in enumerate(names)}


def check(name, case, got, x=None, cap=None):
    fig, i = N.measure(case, got)
    cap = N.CAPS[name] if cap is None else cap
    at = "" if x is None else " at input %r" % (x[i],)
    print("%-18s device max err / yard %9.3f (cap %g)%s: got %.17g ref %.17g" % (name, fig, cap, at, got[i], case["ref"][0][i]))
    assert fig <= cap, (name, fig, cap, i)
    return fig


# ---------------------------------------------------------------------------------------------- the node sum, called directly
def field_sum(lib, c, bright):
    n = len(c["aC"])
    y, vm = np.full(n, FILL), np.full(n, FILL)
    rc = lib.np_field_sum(c["nf"], int(bright), _d(N.f64(c["om0"])), _d(N.f64(c["aC"])), _d(N.f64(c["a3"])), _d(N.f64(c["a4"])),
                          _d(N.f64(c["cA"])), _d(N.f64(c["V"])), _d(y), _d(vm), n)
    assert rc == 0, rc
    return y, vm


def _where(c):
    return np.column_stack([c["aC"], c["a3"], c["a4"] * c["V"][:, 0], c["aC"] * c["a3"] + c["cA"][:, 0]])      # aC, a3, a4 V_0, num_0


@pytest.mark.parametrize("nf,zero_field", [(1, None), (2, None), (3, None), (4, None), (5, None), (6, None), (7, None), (8, None), (5, 2)])
def test_field_sum(probe, nf, zero_field):
    """field_sum<NF> on every element; field_sum_bright<NF> on the elements the kernels' gate hands it (alpha_C > 0 and a4 vmin >
    37.5), against the FULL formula, decay included: the claim that the decay factor is exactly 1.0 there."""
    c = N.case_field_sum(nf, zero_field)
    got, vm = field_sum(probe, c, False)
    assert np.array_equal(vm, N.vmin_of(c, nf)), "walker_vmin"
    check("field_sum", c, got, _where(c))
    # where d = 0 before the floor, the floor makes the exponent -inf-like and the node contributes exactly +0
    fl = c["kind"] == "floor"
    assert fl.sum() >= 20 and np.all(got[fl] == 0.0) and not np.any(np.signbit(got[fl]))
    g = N.sub(c, c["gate"])
    assert len(g["aC"]) > 100
    gotb, _ = field_sum(probe, g, True)
    check("field_sum_bright", g, gotb, _where(g))


def test_field_sum_special_values(probe):
    """non-finite node values, which the gridsum_body-driven entries cannot carry (0 x inf): a4 = +inf is a node brighter than
    any - the clamp makes it the bits of a4 V = 1e6 - a NaN log-flux contributes exactly +0 in the general form (both clamps
    are fmax(x, -750), which returns its other operand), and a4 = 0 gives exactly +0"""
    E = N._direct(1.0, [1.5, np.nan, 1.5, -2.0, 1.5, -2.0], [np.inf, 3.0, 0.0, np.inf, 1.0e6, 1.0e6], 0.0, 1.0, "special")
    got, _ = field_sum(probe, dict(E, nf=3, om0=N.om0_for(3)), False)
    assert got[1] == 0.0 and got[2] == 0.0 and not np.any(np.signbit(got[1:3]))
    assert got[0] == got[4] and got[3] == got[5] and 0.0 < got[3] < got[0] < N.OM0[:3].sum()


# ---------------------------------------------------------------------------------------------- the quadratics
def quad(lib, op, x):
    n = len(x)
    y = np.full((n, 3), FILL)
    rc = lib.np_quad(op, _d(N.f64(x)), _d(y), n)
    assert rc == 0, rc
    return y


def test_quad_coef(probe):
    """the reference's float64 operation order with contraction off: the NumPy twin's bits, and each coefficient against the
    quadratic through the three points at 40 digits"""
    c = N.case_quad_coef()
    got = quad(probe, 0, c["x"])
    for q, nm in enumerate("abc"):
        bad = np.where(got[:, q] != c["np"][q])[0]
        assert len(bad) == 0, (nm, bad[:10], got[bad[:10], q], c["np"][q][bad[:10]])
        check("quad_coef", {"ref": c["ref"][q], "yard": c["yard"][:, q]}, got[:, q], c["x"])


def test_quad_nofma(probe):
    c = N.case_quad_nofma()
    got = quad(probe, 1, c["x"])[:, 0]
    bad = np.where(got != c["np"])[0]
    assert len(bad) == 0, (bad[:10], got[bad[:10]], c["np"][bad[:10]], c["x"][bad[:10]])
    check("quad_nofma", c, got, c["x"])


def test_quad_comp(probe):
    c = N.case_quad_comp()
    got = quad(probe, 2, c["x"])[:, 0]
    fig = check("quad_comp", c, got, c["x"])
    assert fig <= 2.0, "the header claims ~1 ulp"


def test_quad_range(probe):
    """the contract: [mn, mx] contains the twin's values at lo, at hi and at the vertex where it lies strictly inside, and both
    ends are among those values"""
    c = N.case_quad_range()
    x = c["x"]
    got = quad(probe, 3, x)
    mn, mx = got[:, 0], got[:, 1]
    v0, v1, vv, zv, inside = N.np_quad_range(x[:, 0], x[:, 1], x[:, 2], x[:, 3], x[:, 4])
    ex = c["exact_vertex"]
    on_edge = ex & ((c["vert"] == 1.25) | (c["vert"] == 1.75))
    assert on_edge.sum() >= 50 and not inside[on_edge].any() and inside[ex & ~on_edge].all()      # the vertex exactly on lo or hi is not inside
    assert (x[:, 0] == 0.0).sum() >= 100
    vals = np.column_stack([v0, v1, np.where(inside, vv, v0)])
    assert np.all(mn <= vals.min(axis=1)) and np.all(mx >= vals.max(axis=1)), np.where((mn > vals.min(axis=1)) | (mx < vals.max(axis=1)))[0][:10]
    assert np.array_equal(mn, vals.min(axis=1)) and np.array_equal(mx, vals.max(axis=1))


# ---------------------------------------------------------------------------------------------- gridsum_body
def gridsum(lib, variant, TW, tw, nf, om0, S, cols, spec, G, PG, W, a3, a4, a4min, wrec, mode, B):
    nn = len(G)
    nch = (nn + 255) // 256
    part = np.full((B, nch), FILL)
    rc = lib.np_gridsum(variant, TW, tw, nf, _d(N.f64(om0)), S, int(cols), int(spec), _d(N.f64(G)), _d(N.f64(PG)), _d(N.f64(W)), _d(N.f64(a3)),
                        _d(N.f64(a4)), _d(N.f64(a4min)), nn, _d(N.f64(wrec)), _i(np.ascontiguousarray(mode, dtype=np.int32)), B, _d(part))
    assert rc == 0, rc
    return part


def with_skip(B, lay, k=None):
    """the walkers' modes: all MODE_FAST but one MODE_SKIP (outside the prior: its nodes are not evaluated)"""
    mode = np.zeros(B, dtype=np.int32)
    k = B // 2 if k is None else k
    mode[k] = lay["MODE_SKIP"]
    return mode, k


def check_grid(name, c, part, skip, B, nch, x=None):
    """every slot written; the MODE_SKIP walker exactly +0.0 in every chunk; the others against the reference"""
    assert not np.any(part == FILL), "a partial that was not written"
    assert np.all(part[skip] == 0.0) and not np.any(np.signbit(part[skip])), "MODE_SKIP"
    keep = np.ones((B, nch), dtype=bool)
    keep[skip] = False
    keep = keep.ravel()
    s = {"ref": (c["ref"][0][keep], c["ref"][1][keep]), "yard": c["yard"][keep]}
    return check(name, s, part.ravel()[keep], None if x is None else x[keep])


@pytest.mark.parametrize("variant", [FREE, FIXCOMP])
@pytest.mark.parametrize("TW,B", N.TILINGS)
def test_schechter_node_factor(probe, variant, TW, B):
    """fexp_c(fma(c1, G - L*, c0) - PG Q) of FREE and FIXCOMP.  FREE multiplies it with the node sum, which is made exactly 1.0:
    one field of Omega_0 = 2, alpha_C = 1, a3 = 0 and cA = 0 (num = 0, w = fma(0, rsqrt(1), 1) = 1), a4min vmin = 1000 (the
    bright form: 0.5 x 2 x 1)."""
    lay = layout(probe)
    nch = 260 if (TW, B) == N.TILINGS[0] else 24
    c = N.case_schechter(B, nch)
    rec = np.zeros((B, lay["REC"]))
    rec[:, lay["R_LSTAR"]], rec[:, lay["R_C0"]], rec[:, lay["R_C1"]], rec[:, lay["R_Q"]] = c["Ls"], c["c0"], c["c1"], c["Q"]
    rec[:, lay["R_ALPHAC"]], rec[:, lay["V0"]] = 1.0, 1.0
    nn = nch * 256
    mode, skip = with_skip(B, lay, B - 1)
    part = gridsum(probe, variant, TW, TW, 1, [2.0], 101, False, True, N.chunk_nodes(c["G"]), N.chunk_nodes(c["PG"]), N.one_hot_weights(nch),
                   np.zeros(nn), np.full(nn, 1000.0), np.full(nch, 1000.0), rec, mode, B)
    x = np.column_stack([np.repeat(c["c0"], nch), np.repeat(c["c1"], nch), np.repeat(c["Ls"], nch), np.tile(c["G"], B), c["arg"].ravel()])
    check_grid("schechter", c, part, skip, B, nch, x)
    # beyond both clamps: exactly +0 below -750, the value at 709 above it
    arg = c["arg"]
    low = (arg < -750.0)
    low[skip] = False
    assert np.all(part[low] == 0.0)
    if B == 31:
        assert low.sum() > 10 and c["n_edge_walkers"] >= 6
        assert part[3, 0] == part[2, 0] == part[5, 0] and np.isfinite(part[3, 0])          # c0 = 709 + 1 ulp, 709, 720 (Q = 0)


@pytest.mark.parametrize("TW,B,nf", [(16, 31, 5), (16, 17, 8), (4, 7, 1), (4, 5, 3)])
def test_gridsum_free_node_sum_and_bright_gate(probe, TW, B, nf):
    """the node sum through gridsum_body<LF_FREE>, whose own test a4min walker_vmin > 37.5 picks the form: against the full
    formula on both sides of 37.5, for the walker with the smallest num the boxes allow there"""
    lay = layout(probe)
    nch = 260 if B == 31 else 40
    c = N.case_gridsum_free(B, nch, nf)
    rec = np.zeros((B, lay["REC"]))
    rec[:, lay["R_ALPHAC"]] = c["w_aC"]
    for f in range(nf):
        rec[:, lay["CA0"] + lay["FSTRIDE"] * f] = c["w_cA"][:, f]
        rec[:, lay["V0"] + lay["FSTRIDE"] * f] = c["w_V"][:, f]
    mode, skip = with_skip(B, lay)
    assert skip != 0
    part = gridsum(probe, FREE, TW, TW, nf, c["om0"], 101, False, True, np.full(nch * 256, 42.0), np.ones(nch * 256), N.one_hot_weights(nch),
                   N.chunk_nodes(c["n_a3"]), N.chunk_nodes(c["n_a4"]), c["n_a4"], rec, mode, B)
    x = np.column_stack([c["aC"], c["a3"], c["a4"] * N.vmin_of(c, nf), c["gate"]])
    check_grid("gridsum_free_sum", c, part, skip, B, nch, x)
    # walker 0's first nodes straddle the gate
    g0 = c["gate"].reshape(B, nch)[0, :c["n_edge_nodes"]]
    assert g0.any() and not g0.all()


@pytest.mark.parametrize("cols", [True, False])
@pytest.mark.parametrize("TW,B,S", [(16, 31, 257), (16, 17, 129), (4, 7, 129), (4, 5, 128)])
def test_znode_forms(probe, TW, B, S, cols):
    """the z-evolving node: the column form (Q, E per (walker, column) in LDS, one exponential per node) on chunks that
    straddle one and two column boundaries and on the last, partial chunk (S = 257: one node; S = 129: one node; S = 128: the
    chunks are whole and end on a boundary), and the row form lnT_zevol<true> on the same lattice"""
    lay = layout(probe)
    c = N.case_znode(B, S, cols)
    nch = c["nch"]
    rec = np.zeros((B, lay["REC"]))
    rec[:, lay["Z_AL"]:lay["Z_C1"] + 1] = c["rec"]
    mode, skip = with_skip(B, lay, 1)
    part = gridsum(probe, ZEVOL, TW, TW, 1, [1.0], S, cols, True, c["G"], c["PG"], c["W"], c["a3"], c["a4"], np.zeros(nch), rec, mode, B)
    x = np.column_stack([np.repeat(np.arange(B), nch), np.tile(np.arange(nch), B), np.tile(c["col"], B), np.tile(c["G"][c["live"]], B)])
    check_grid("znode_cols" if cols else "znode_rows", c, part, skip, B, nch, x)
    if S == 257:
        lanes = c["live"] % 256
        assert set(lanes[:256].tolist()) == set(range(256))           # every lane position carried a value


def test_entry_points_refuse_what_they_cannot_run(probe):
    z = np.zeros(8)
    y = np.zeros(1)
    assert probe.np_field_sum(0, 0, _d(z), _d(z), _d(z), _d(z), _d(z), _d(z), _d(y), _d(y), 1) == -1
    assert probe.np_field_sum(9, 0, _d(z), _d(z), _d(z), _d(z), _d(z), _d(z), _d(y), _d(y), 1) == -1
    assert probe.np_quad(4, _d(z), _d(z), 1) == -1
    lay = layout(probe)
    rec, mode, part = np.zeros(lay["REC"]), np.zeros(1, dtype=np.int32), np.zeros(1)
    args = (_d(z), _d(z), _d(z), _d(z), _d(z), _d(z), 8, _d(rec), _i(mode), 1, _d(part))
    assert probe.np_gridsum(ZEVOL, 16, 16, 1, _d(z), 127, 1, 1, *args) == -1       # S below BLOCK / (ZCOLS - 1)
    assert probe.np_gridsum(ZEVOL, 16, 16, 1, _d(z), 128, 1, 1, *args) == -1       # nnodes != S * S
    assert probe.np_gridsum(FREE, 8, 8, 1, _d(z), 101, 0, 1, *args) == -1          # a tile height that is not instantiated
    assert probe.np_gridsum(FREE, 16, 17, 1, _d(z), 101, 0, 1, *args) == -1        # tw above TW
