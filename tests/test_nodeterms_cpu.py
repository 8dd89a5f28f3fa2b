"""The element-wise probes of piece B's grid-node forms without a GPU: tests/node_probe.hip cross-compiles for gfx950 with
the library's flags and its kernels use no scratch; every generator of tests/lf_nodeproblib.py yields what it promises;
the NumPy twins stay within their caps against the 40-digit references on the full input sets (the reference alone must
pass before it judges a kernel), and the figures the caps of tests/test_gpu_nodeterms.py rest on are measured and printed."""
import math
import os

import numpy as np

import lf_isalib
import lf_nodeproblib as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "node_probe.hip")
NFS = [(nf, None) for nf in range(1, 9)] + [(5, 2)]
GRIDSUM_FREE = ((31, 260, 5), (17, 40, 8), (7, 40, 1), (5, 40, 3))
ZNODE = ((31, 257), (17, 129), (7, 129), (5, 128))


def test_probe_unit_compiles_for_gfx950_and_its_kernels_use_no_scratch():
    seen = {name: r["ScratchSize"] for name, r in lf_isalib.remarks(SRC, "-c").items() if "probe_" in name and "ScratchSize" in r}
    # the node sum, 4 quadratics, gridsum_body for 3 variants x 2 tile heights
    assert len(seen) == 11, sorted(seen)
    assert all(v == 0 for v in seen.values()), seen


def test_generator_never_leaves_the_domain():
    """(alpha_C, Flim, log f) inside the boxes, and the record values derived from the triple: num and a4 V go together"""
    aC, Fl, logf, kap = N.triples(3000, 7)
    box = np.arange(3000) % 3
    for k, ((alo, ahi), (flo, fhi)) in enumerate(N.BOXES):
        s = box == k
        assert aC[s].min() == alo and aC[s].max() == ahi and Fl[s].min() == flo and Fl[s].max() == fhi
    assert logf.min() >= N.LOGF_LO and logf.max() <= N.LOGF_HI
    assert set(np.round(kap, 12)) == set(round(N.kappa_of(f), 12) for f in N.FCMINS)
    assert abs(N.kappa_of(0.1) - 4.0 / 3.0) < 1e-15              # (the b = -sqrt((16 / 9) / alpha_C^2) of lf_problib)
    E = N.elements_from(aC, Fl, logf, kap)
    for f in (0, 3, 7):
        assert np.abs(N.tie_residual(E, f)).max() < 1e-13
        num = E["aC"] * E["a3"] + E["cA"][:, f]
        x = E["a4"] * E["V"][:, f]
        assert num.min() >= N.NUM_LO and num.max() <= N.NUM_HI and x.min() >= N.X_LO and x.max() <= N.X_HI
    # the cases' reachable elements too, and their unreachable ones are edges only
    for nf in (1, 8):
        c = N.case_field_sum(nf)
        assert np.abs(N.tie_residual(c)).max() < 1e-13
        assert not c["reach"][:c["n_edges"]].all() and c["reach"][c["n_edges"]:].all()
        assert len(c["aC"]) <= N.L.NMAX


def test_edge_lists_hit_what_they_claim():
    E = N.field_edges()
    kind, x = E["kind"], E["a4"] * E["V"][:, 0]
    num = E["aC"] * E["a3"] + E["cA"][:, 0]
    with np.errstate(divide="ignore", over="ignore"):
        d = 1.0 - np.exp(-x)
        t = np.log(0.5 * (1.0 + num / np.sqrt(1.0 + num * num))) / d
    # the clamp of -(a4 V): on both sides of -750 and on it
    s = kind == "clamp_x"
    assert np.any(-x[s] < -750.0) and np.any(-x[s] > -750.0) and np.any(x[s] == 750.0)
    assert set(np.round((x[s] - 750.0) / np.spacing(750.0)).astype(int)) >= {-1, 0, 1, 2}
    # the floor: d == 0 before it; the next doubles up are not floored
    assert (kind == "floor").sum() >= 20 and np.all(d[kind == "floor"] == 0.0)
    assert np.all(d[kind == "above_floor"] > 0.0) and np.all(d[kind == "above_floor"] > 1e-100)
    # the cancelling range
    s = kind == "cancel"
    assert x[s].min() == 1.0e-3 and x[s].max() == 1.0 and set(num[s]) == {-2.0, 0.0, 1.5, 8.0}
    # the clamp of ln fc / d: both sides of -750, the subnormal results, the normal ones
    s = kind == "clamp_t"
    assert np.any(t[s] < -750.0) and np.any(t[s] > -750.0) and np.any((t[s] > -745.0) & (t[s] < -708.4)) and np.any(t[s] > -700.0)
    te = np.array([float(N.mp.log(N.mp.mpf(1) / 2) / -N.mp.expm1(-N.mpf(v)) + 750) for v in x[s][-7:]])      # (exactly: the doubles next to the clamp)
    assert np.any(te < 0.0) and np.any(te > 0.0) and np.min(np.abs(te)) < 2e-13
    # the bright threshold: straddled within 2 ulp, up to 40, at the smallest num of the boxes
    s = kind == "bright"
    k = np.round((x[s] - 37.5) / np.spacing(37.5))
    assert set(k[np.abs(k) <= 2].astype(int)) == {-2, -1, 0, 1, 2} and x[s].min() == 30.0 and x[s].max() == 40.0
    assert np.any(x[s] > 37.5) and np.any(x[s] <= 37.5)
    aC, Fl, kap = N.smallest_num_bright()
    assert np.allclose(num[s], aC * np.log10(x[s]) - kap, atol=1e-12) and num[s].max() < -3.9
    assert np.all(np.abs(N.tie_residual(N.sub(dict(E, ref=(x, x), yard=x, np=x, gate=E["reach"]), s))) < 1e-13)
    # zeros of both signs, the largest |num|
    z = kind == "zero"
    assert np.all(num[z] == 0.0) and np.any(np.signbit(E["a3"][z])) and np.any(~np.signbit(E["a3"][z]))
    m = kind == "num_max"
    assert num[m].max() > 57.0 and num[m].min() < -29.0
    # Omega_f = 0 for one field, every NF
    assert N.om0_for(5, 2)[2] == 0.0 and np.all(N.om0_for(5, 2)[[0, 1, 3, 4]] > 0)
    # gridsum_body's gate: walker 0's edge nodes on both sides, within 2 ulp
    c = N.case_gridsum_free(17, 40, 8)
    xs = (c["a4"] * N.vmin_of(c, 8)).reshape(17, 40)[0, :c["n_edge_nodes"]]
    assert np.any(xs > 37.5) and np.any(xs <= 37.5) and np.min(np.abs(xs - 37.5)) <= 2 * np.spacing(37.5) and xs.min() < 30.5
    # the Schechter factor: arguments at both clamps of fexp_c, and PG Q large enough to underflow
    c = N.case_schechter(31, 260)
    a = c["arg"]
    assert np.any(a > 709.0) and np.any(a == 709.0) and np.any(a < -750.0) and np.any(a == -750.0) and np.any((a < -708.4) & (a > -745.0))
    assert np.any(c["ref"][0] == 0.0) and np.all(np.isfinite(c["ref"][0]))
    # the quadratics: the reference's pivots, pivots 1e-3 apart, z on a pivot, a = 0, the vertex on lo and on hi
    P = N.pivot_sets()
    assert tuple(P[0]) == N.PIVOTS and np.any(np.abs(np.diff(P, axis=1) - 1e-3) < 1e-12)
    q = N.case_quad_nofma()["x"]
    assert np.mean(np.isin(q[:, 3], P.ravel())) > 0.2
    r = N.case_quad_range()
    assert (r["x"][:, 0] == 0.0).sum() >= 100 and {1.25, 1.75} <= set(r["vert"][r["exact_vertex"]])


def test_layouts_put_one_weight_in_every_chunk_and_visit_every_lane():
    W = N.one_hot_weights(260)
    assert np.all(W.reshape(260, 256).sum(axis=1) == 1.0) and set(np.where(W == 1.0)[0] % 256) == set(range(256))
    lanes = np.where(W == 1.0)[0][:256] % 256
    assert set((lanes // 32).tolist()) == set(range(8))                       # both halves of all four waves
    for B, S in ZNODE:
        c = N.case_znode(B, S, True)
        nn = S * S
        assert len(c["G"]) == nn and c["W"].sum() == c["nch"] == (nn + 255) // 256
        first, last = np.arange(c["nch"]) * 256, np.minimum(np.arange(c["nch"]) * 256 + 255, nn - 1)
        ncols = last // S - first // S + 1
        assert ncols.max() <= 3                                               # ZCOLS
        assert (ncols.max() == 3) == (S == 129) and (nn % 256 != 0) == (S != 128)
        # the weighted node lies in its chunk, and in other columns than the chunk's first for some chunks
        assert np.array_equal(c["live"] // 256, np.arange(c["nch"]))
        rel = c["col"] - first // S
        assert set(rel.tolist()) >= ({0, 1, 2} if S == 129 else {0, 1})
    for TW, B in N.TILINGS:
        assert B % TW in (1, TW - 1)


def test_numpy_figures_behind_the_caps():
    """max err / yardstick of the NumPy twins against the 40-digit values, on the full input sets: the caps of the GPU tests are
    4 x these and never below 2 (lf_nodeproblib.CAPS holds them as constants; this test says when they have moved)"""
    figs = {}

    def put(name, case, got=None):
        f = N.measure(case, case["np"] if got is None else got)
        if name not in figs or f[0] > figs[name][0]:
            figs[name] = f
    for nf, zf in NFS:
        c = N.case_field_sum(nf, zf)
        put("field_sum", c)
        put("field_sum_bright", N.sub(c, c["gate"]))
    for B, nch, nf in GRIDSUM_FREE:
        put("gridsum_free_sum", N.case_gridsum_free(B, nch, nf))
    for TW, B in N.TILINGS:
        put("schechter", N.case_schechter(B, 260 if B == 31 else 24))
    for B, S in ZNODE:
        put("znode_cols", N.case_znode(B, S, True))
        put("znode_rows", N.case_znode(B, S, False))
    c = N.case_quad_coef()
    for q in range(3):
        put("quad_coef", {"ref": c["ref"][q], "yard": c["yard"][:, q]}, c["np"][q])
    put("quad_nofma", N.case_quad_nofma())
    put("quad_comp", N.case_quad_comp())
    for k, (fig, i) in figs.items():
        print("numpy %-18s max err / yard %12.3f at index %d   cap %g" % (k, fig, i, N.CAPS[k]))
    assert set(figs) == set(N.CAPS)
    for k, (fig, i) in figs.items():
        assert math.isfinite(fig), k
        assert fig <= N.CAPS[k], (k, fig)                # the twin within its cap: the reference alone passes
        # the constant is 4 x the figure measured when it was written (never below 2): it may not have drifted by more
        # than the last digit it was rounded to
        assert N.cap_from(fig) <= N.CAPS[k] * 1.05 and N.cap_from(fig) >= N.CAPS[k] * 0.8, (k, fig, N.CAPS[k])
