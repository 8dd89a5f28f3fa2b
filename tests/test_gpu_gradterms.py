"""The completeness forms and the Lagrange basis of csrc/lf_grad.h, csrc/lf_deconv.h and csrc/lf_deconv_grad.h, and the
per-source / per-lattice-node contributions of lf_grad_part, lf_deconv_part and lf_deconv_grad_part, element by element on the
GPU against 40-digit values (inputs, references, yardsticks and caps: tests/lf_gradproblib.py; the probe:
tests/grad_probe.hip, compiled once per module with the library's own flags).

test_gpu_grad.py, test_gpu_deconv.py and test_gpu_deconv_grad.py compare whole-catalogue sums with the NumPy twins to 1e-12 of
the sum of the absolute contributions: an error of 1e-9 in the bright sources' branch of g', in the sources whose e^(-v) is 0
or in the nodes that raise the running maximum stays below that.  Here each test prints its measured maximum of err / yardstick
and the input at the maximum, then asserts it against the cap: 4 x the figure of the same expression in NumPy binary64, never
below 2.  DESIGN.md section 3.13 records the figures."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import lf_gradproblib as P
from lf_testlib import make_inputs
from lumfuncmcmc_amd import build

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_dp = ctypes.POINTER(ctypes.c_double)
FILL = -777.0
VARIANTS = (P.FREE, P.FIXCOMP, P.ZEVOL)


def _d(a):
    return None if a is None else a.ctypes.data_as(_dp)


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("grad_probe") / "grad_probe.so")
    subprocess.run([build.hipcc()] + build.CXXFLAGS + ["-fPIC", "-shared", "-o", so, os.path.join(ROOT, "tests", "grad_probe.hip")], check=True)
    lib = ctypes.CDLL(so)
    assert lib.gp_device_count() >= 1, "no GPU"
    return lib


def check(name, case, got, where=None, cap=None):
    fig, i = P.measure(case, got)
    cap = P.CAPS[name] if cap is None else cap
    at = "" if where is None else " at %s" % (where(i),)
    print("%-22s device max err / yard %9.3f (cap %g)%s: got %.17g ref %.17g" % (name, fig, cap, at, np.ravel(got)[i], case["ref"][0][i]))
    assert fig <= cap, (name, fig, cap, i)
    return fig


def comp(lib, which, aC, kappa, p, q, r):
    n = len(aC)
    assert n <= P.NMAX
    out = np.full((n, 3), -12345.0)
    rc = lib.gp_comp(which, _d(P.L.f64(aC)), _d(P.L.f64(kappa)), _d(None if p is None else P.L.f64(p)), _d(P.L.f64(q)), _d(P.L.f64(r)), _d(out), n)
    assert rc == 0, rc
    return out


# ---------------------------------------------------------------------------------------------- completeness forms, basis
def test_dgrad_comp_and_deconv_lcomp(probe):
    c = P.case_dgrad_comp()
    q = c["l"]
    got = comp(probe, 1, q["aC"], q["kappa"], None, q["y"], q["v"])
    at = lambda i: "aC %r y %r v %r (num %r)" % (q["aC"][i], q["y"][i], q["v"][i], q["num"][i])      # noqa: E731
    for j, k in enumerate(("l", "dF", "dC")):
        check("dgrad_comp_" + k, c[k], got[:, j], at)
    lc = comp(probe, 2, q["aC"], q["kappa"], None, q["y"], q["v"])
    check("deconv_lcomp", c["lcomp"], lc[:, 0], at)
    # the header's promise: dgrad_comp(...).l has deconv_lcomp's bits
    assert np.array_equal(got[:, 0], lc[:, 0]), np.where(got[:, 0] != lc[:, 0])[0][:10]
    # past the underflow of e^(-v) the weight w is exactly 0: dF is its second addend alone and has its sign
    with np.errstate(under="ignore"):
        dead = np.exp(-q["v"]) == 0.0
    assert dead.sum() >= 20 and np.all(np.sign(got[dead, 1]) == -np.sign(q["aC"][dead]))


def test_grad_comp(probe):
    c = P.case_grad_comp()
    q = c["l"]
    got = comp(probe, 0, q["aC"], q["kappa"], q["flim"], q["logf"], q["U"])
    at = lambda i: "Flim %r aC %r y %r" % (q["flim"][i], q["aC"][i], q["y"][i])      # noqa: E731
    for j, k in enumerate(("l", "dF", "dC")):
        check("grad_comp_" + k, c[k], got[:, j], at)


def test_grad_basis(probe):
    c = P.case_basis()
    n = len(c["z"])
    out = np.full((n, 3), -12345.0)
    rc = probe.gp_basis(_d(c["piv"]), _d(c["z"]), _d(out), n)
    assert rc == 0, rc
    check("grad_basis", c, out.ravel(), lambda i: "z %r pivots %s l_%d" % (c["z"][i // 3], c["piv"][i // 3], i % 3))
    at = c["z"][:, None] == c["piv"]                 # at a pivot: exactly 0 for the two others
    rows = at.any(axis=1)
    assert np.all(out[rows][~at[rows]] == 0.0)


# ---------------------------------------------------------------------------------------------- lf_grad_part
def run_grad_part(lib, c, with_dead_row=True):
    rows = c["rows"]
    v, fsa, n = c["variant"], c["fsa"], c["n"]
    th = np.ascontiguousarray(np.concatenate([rows, rows[:1]]) if with_dead_row else rows)
    lnp = np.full(len(th), -123.5)
    if with_dead_row:
        lnp[-1] = -np.inf
    a1 = c["z"] if v == P.ZEVOL else c["logf"]
    part = np.full((len(th), 2 * n, P.G_SLOTS), FILL)
    piv = P.L.f64(P.PIVOT_SETS[0])
    rc = lib.gp_grad_part(v, fsa, ctypes.c_double(P.synth.SCH_AL), ctypes.c_double(P.KAPPA), ctypes.c_double(P.OM0), _d(piv), _d(th), _d(lnp),
                          len(th), _d(c["lum"]), _d(a1), _d(c["P"]), _d(c["U"]), n, _d(c["lum"]), _d(c["P"]), _d(c["W"]), _d(a1), _d(c["U"]), n,
                          _d(part))
    assert rc == 0, rc
    return part


@pytest.mark.parametrize("fsa", [0, 1])
@pytest.mark.parametrize("variant", VARIANTS)
def test_grad_part_items(probe, variant, fsa):
    c = P.case_grad_part(variant, fsa)
    part = run_grad_part(probe, c)
    R, items, ns = c["shape"]
    n = c["n"]
    assert np.all(part[R] == FILL), "a block of a row whose lnprob is -inf must leave at once"
    assert np.all(part[:R, :, 7] == FILL) and np.all(part[:R, :, :7] != FILL)
    got = part[:R].copy()
    got[:, :, 7] = 0.0
    ref = c["ref"][0].reshape(c["shape"])

    def at(i):
        b, it, s = np.unravel_index(i, c["shape"])
        return "row %d %s %d slot %d (lum %r)" % (b, "source" if it < n else "node", it % n, s, c["lum"][it % n])
    check("grad_part_" + P.VNAME[variant], c, got.ravel(), at)
    # a node whose integrand is 0 in binary64 is skipped: every slot exactly +0
    dead = np.all(ref[:, n:, :] == 0.0, axis=2)
    assert dead.sum() >= 10 and np.all(got[:, n:, :][dead] == 0.0) and not np.any(np.signbit(got[:, n:, :][dead]))
    # a row's bits do not depend on the batch: the same rows without the dead one
    assert np.array_equal(run_grad_part(probe, c, with_dead_row=False), part[:R])


# ---------------------------------------------------------------------------------------------- deconvolution
def run_deconv(lib, variant, rows, s, nodes, K, dead_row=False, fsa=0):
    th = np.ascontiguousarray(np.concatenate([rows, rows[:1]]) if dead_row else rows)
    lnp = np.full(len(th), -123.5)
    if dead_row:
        lnp[-1] = -np.inf
    n = s["n"]
    a1 = s["z"] if variant == P.ZEVOL else s["logf"]
    part = np.full((len(th), n), FILL)
    gpart = np.full((len(th), n, P.D_SLOTS), FILL)
    piv = P.L.f64(P.PIVOT_SETS[0])
    nodes = P.L.f64(nodes)
    assert len(nodes) == 2 * K
    rc = lib.gp_deconv(variant, fsa, ctypes.c_double(P.synth.SCH_AL), ctypes.c_double(P.KAPPA), _d(piv), ctypes.c_double(P.FLIM0),
                       ctypes.c_double(P.ALPHA0), _d(th), _d(lnp), len(th), _d(s["lum"]), _d(a1), _d(s["P"]), _d(s["logf"]), _d(s["U"]),
                       _d(s["sigma"]), n, _d(nodes), K, _d(part), _d(gpart))
    assert rc == 0, rc
    return part, gpart


@pytest.mark.parametrize("K", [4, 32])
@pytest.mark.parametrize("variant", VARIANTS)
def test_deconv_items(probe, variant, K):
    c = P.case_deconv(variant, K)
    cd, cg = c["delta"], c["grad"]
    s, rows = cd["src"], cd["rows"]
    R, n = len(rows), s["n"]
    part, gpart = run_deconv(probe, variant, rows, s, cd["nodes"], K, dead_row=True)
    assert np.all(part[R] == FILL) and np.all(gpart[R] == FILL), "a block of a row whose lnprob is -inf must leave at once"
    used = {P.FREE: 4, P.FIXCOMP: 2, P.ZEVOL: 4}[variant]
    assert np.all(gpart[:R, :, used:] == FILL) and np.all(gpart[:R, :, :used] != FILL) and np.all(part[:R] != FILL)
    got = gpart[:R].copy()
    got[:, :, used:] = 0.0
    nm = P.VNAME[variant]

    def at(i):
        b, it = np.unravel_index(i, (R, n))
        return "row %d source %d (sigma %g, lum %r, logf %r; %d rises)" % (b, it, s["sigma"][it], s["lum"][it], s["logf"][it], cd["rises"][it])
    check("deconv_delta_" + nm, cd, part[:R].ravel(), at)
    check("deconv_grad_" + nm, cg, got.ravel(), lambda i: at(i // P.D_SLOTS) + " slot %d" % (i % P.D_SLOTS))
    # a sigma = 0 source: exactly +0 in every slot
    off = s["sigma"] == 0.0
    for a in (part[:R][:, off], got[:, off, :]):
        assert np.all(a == 0.0) and not np.any(np.signbit(a))


@pytest.mark.parametrize("variant", VARIANTS)
def test_a_node_of_zero_weight_is_skipped(probe, variant):
    """A node whose exponent is -inf is skipped by both kernels.  No source inside the model's domain produces one
    (lf_gradproblib's docstring), so the table gets one more node of weight 0 (ln w = -inf): first (m = -inf and s = 0 still),
    in the middle and last.  The bits are those of the table without it."""
    c = P.case_deconv(variant, 4)["delta"]
    s, rows, nodes = c["src"], c["rows"], c["nodes"]
    want = run_deconv(probe, variant, rows, s, nodes, 4)
    for pos in (0, 2, 4):
        n5 = np.concatenate([np.insert(nodes[:4], pos, 0.3), np.insert(nodes[4:], pos, -np.inf)])
        got = run_deconv(probe, variant, rows, s, n5, 5)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (variant, pos)
    # a node that ties the maximum (d == 0): the table's own nodes twice each give ln 2 more
    n8 = np.concatenate([np.repeat(nodes[:4], 2), np.repeat(nodes[4:], 2)])
    d8, g8 = run_deconv(probe, variant, rows, s, n8, 8)
    on = s["sigma"] > 0.0
    tol = 8 * P.U53 * (np.abs(want[0][:, on]) + 1.0)
    assert np.all(np.abs(d8[:, on] - (want[0][:, on] + np.log(2.0))) <= tol)


def test_free_value_slot_has_the_librarys_bits(probe):
    """The FREE value slot of lf_deconv_part for one source alone in its block is what the library adds for that source: on a
    one-source catalogue lf_lnprob_err_batch returns fl(lnprob + Delta_1) (one block, one source, the final sum of one
    element), so with the probe's Delta_1 the sum lnprob + Delta_1 has the library's bits.  Subtracting lnprob from the
    library's value instead would round a second time, at the size of lnprob; the forward sum asks for the same identity
    without that."""
    from lumfuncmcmc_amd.capi import LFContext
    K = 32
    nodes = np.zeros(2 * K)
    assert probe.gp_nodes(K, _d(nodes)) == 0
    inp = make_inputs("free", 1, seed=3, S=23, nf=1)
    lum = np.array([42.61])
    logf = np.array([np.log10(P.FLIM0) + 0.13 - 17.0])
    inp["lum"], inp["logf"] = lum, logf
    rows = np.array([[42.5, -2.0, -1.49, 2.72, 4.56], [42.1, -2.4, -1.2, 3.3, 2.0], [43.0, -3.0, -1.7, 1.5, 6.5]])
    ctx = LFContext(inp)
    try:
        probe.gp_kappa.restype, probe.gp_kappa.argtypes = ctypes.c_double, [ctypes.c_double]
        assert probe.gp_kappa(inp["fcmin"]) == P.KAPPA, "the context's kappa and the cases' differ"
        lp = ctx.lnprob_batch(rows)
        assert np.all(np.isfinite(lp))
        for sg in (0.05, 0.3):
            ctx.set_lum_err(np.array([sg]), K, unchecked=True)
            lib = ctx.lnprob_err_batch(rows)
            s = {"lum": lum, "z": np.array([1.5]), "logf": logf, "P": P.pow10(lum - 42.0), "U": P.pow10(logf + 17.0), "sigma": np.array([sg]), "n": 1}
            part, _ = run_deconv(probe, P.FREE, rows, s, nodes, K)
            print("sigma %g: Delta_1 %s, lnprob %s" % (sg, part[:, 0], lp))
            assert np.all(part[:, 0] != 0.0) and np.array_equal(lp + part[:, 0], lib)
    finally:
        ctx.close()


def test_entry_points_refuse_counts_beyond_their_buffers(probe):
    one = np.ones(4)
    assert probe.gp_comp(1, _d(one), _d(one), None, _d(one), _d(one), _d(np.zeros(12)), P.NMAX + 1) == -1
    assert probe.gp_comp(0, _d(one), _d(one), None, _d(one), _d(one), _d(np.zeros(12)), 4) == -1
    assert probe.gp_basis(_d(np.ones(12)), _d(one), _d(np.zeros(12)), 0) == -1
    c = P.case_deconv(P.FREE, 4)["delta"]
    with pytest.raises(AssertionError):
        run_deconv(probe, P.FREE, np.repeat(c["rows"], 3, axis=0), c["src"], c["nodes"], 4)            # 12 rows
