"""The element-wise probes of the device math without a GPU: tests/term_probe.hip cross-compiles for gfx950 with the
library's flags and its kernels use no scratch; every generator of tests/lf_problib.py yields what it promises; and the
NumPy binary64 figures that the caps of the GPU tests (tests/test_gpu_terms.py) rest on are measured and printed."""
import math
import os

import mpmath as mp
import numpy as np
import pytest

import lf_isalib
import lf_problib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "term_probe.hip")


def test_probe_unit_compiles_for_gfx950_and_its_kernels_use_no_scratch(tmp_path):
    seen = {name: r["ScratchSize"] for name, r in lf_isalib.remarks(SRC, "-c").items() if "probe_" in name and "ScratchSize" in r}
    # 11 unary, 3 free terms, 2 z-evolving, 6 table instantiations, cell, wave, group8, reduce
    assert len(seen) == 26, sorted(seen)
    assert all(v == 0 for v in seen.values()), seen


def _exact(x):
    return mp.mpf(float(x))


def test_reduction_boundaries_are_within_two_ulp_of_the_intended_points():
    mp.mp.dps = 40
    b = L.reduction_boundaries()
    assert len(b) > 1200 and b.min() < -740 and b.max() > 705
    for x in b[::7]:
        j2 = _exact(x) / L.STEP * 2                     # twice the index: an integer for both kinds of point
        assert abs(j2 - mp.nint(j2)) * L.STEP / 2 <= np.spacing(abs(x)), x
    c = L.case_fexp_t()
    pts = L.ulps_around(b)
    assert np.all(np.isin(pts, c["x"]))
    # the neighbours are 1 and 2 ulp away
    m = len(b)
    assert np.all(np.abs(pts[:m] - b) <= 2 * np.spacing(np.abs(b))) and np.all(pts[2 * m:3 * m] == b) and np.all(pts[:m] < pts[m:2 * m])
    assert np.isnan(c["x"]).sum() == 1 and c["zero"].sum() >= 7
    u = L.case_fexp_neg()["x"]
    assert u.min() == 0.0 and u.max() < 1.0e6 and np.any(u > 999999.0)


def test_log_and_rsqrt_inputs_cover_what_they_promise():
    c = L.case_flog_half()
    w = c["x"]
    # both ends of all 256 intervals in nine binades: the table index (bits 12..19 of the high word) changes between them
    hi = (w.view(np.int64) >> 32)
    j = (hi >> 12) & 0xff
    e = (hi >> 20) & 0x7ff
    for be in (1, 23, 511, 923, 1013, 1020, 1021, 1022, 1023):
        assert len(set(j[e == be])) == 256, be
    ends = L.mantissa_interval_ends((0,))
    assert np.all(np.diff(np.sort(ends))[::2] <= np.spacing(2.0))            # pairs one ulp apart
    assert 0 < c["exempt"].sum() < 0.01 * len(w) and np.all(w[c["exempt"]] < 2.0 ** -1022)
    assert {2.0, 1.0, 2.0 ** -1022, 0.0} <= set(w.tolist())
    up = L.case_flog_half_upper()["x"]
    assert up.min() == 1.0 and up.max() == 2.0 and np.nextafter(2.0, 0.0) in up
    s = L.case_frsqrt()["x"]
    assert s.min() >= L.FRSQRT_LO and s.max() <= L.FRSQRT_HI
    k = np.arange(-300, 500)
    assert np.all(np.isin(np.ldexp(1.0, 2 * k), s)) and np.all(np.isin(np.nextafter(np.ldexp(1.0, 2 * k), 0.0), s))


def test_term_inputs_pass_the_fast_screens_and_the_yardstick_is_finite():
    c = L.case_term_free()
    assert np.all(L.fast_screen(c["num"], c["u"])), np.where(~L.fast_screen(c["num"], c["u"]))[0][:10]
    assert np.all(np.isfinite(c["yard"])) and np.all(c["yard"] > 0)
    assert np.all(np.isfinite(c["ref"][0]))
    num, u, aC = c["num"], c["u"], c["aC"]
    assert num.min() < -1.0e4 and num.max() > 1.0e4 and np.any(num == 0.0) and np.any(np.signbit(num) & (num == 0.0))
    assert u.max() > 5.0e5 and np.all(u < 1.0e6) and aC.max() > 3000.0 and aC.min() < 1.1
    # the smallest admitted values are really at the edge: 10 % less fails the screen
    edge = np.arange(len(u))[::11]
    assert np.mean(~L.fast_screen(num[edge], 0.9 * u[edge])) > 0.9
    # what the reference was computed from is what the function forms: num = fma(alphaC, logf, cA)
    w = c["w"]
    assert np.array_equal(L.fma_exact(w[:20, 4], c["logf"][:20], w[:20, 8]), num[:20])
    k = L.case_term_careful()
    assert k["want_inf"][:k["n_edges"]].sum() >= 7 and not k["want_inf"][k["n_edges"]:].any()


def test_table_lanes_are_inside_the_margins_and_the_ties_are_exact():
    mp.mp.dps = 40
    gb = L.g_boundaries()
    assert len(gb) > 250
    for st, noexp in ((2, False), (4, True), (8, False)):
        c = L.case_table(st, noexp)
        x, wk, kind = c["x"], c["wk"], c["kind"]
        aC, cYH = wk[:, 0], wk[:, 3]
        assert np.all(np.diff(x, axis=1) >= 0)
        width = x[:, -1] - x[:, 0]
        assert np.all(aC * width <= L.G_MARGIN) and np.all(width <= L.H_MARGIN)
        assert np.any(aC * width > 0.99 * L.G_MARGIN) and np.any(width > 0.99 * L.H_MARGIN)
        assert set(c["npad"].tolist()) == set(range(st))
        for i in np.where(c["npad"] > 0)[0][:50]:
            assert np.all(x[i, st - c["npad"][i]:] == x[i, st - c["npad"][i] - 1])
        # centres inside the range the key tests admit
        numc = c["numc"]
        assert np.all(numc > L.G_LO + 2 * L.G_MARGIN) and np.all(numc < L.G_HI - 2 * L.G_MARGIN)
        assert np.all(x[:, 0] + cYH >= 2 * L.H_MARGIN)
        nlo, nhi = aC * x[:, 0] + wk[:, 1], aC * x[:, -1] + wk[:, 1]
        assert np.all(nlo > L.G_LO + 2 * L.G_MARGIN) and np.all(nhi < L.G_HI - 2 * L.G_MARGIN)
        assert c["pg"].min() == 0 and c["pg"].max() == len(L.GT) - 1 and np.all(np.diff(np.unique(c["pg"])) <= 3)
        if not noexp:
            ph = np.clip(np.floor(c["hx"]), 0, L.H_N - 1)
            assert set(ph.astype(int).tolist()) == set(range(L.H_N))
    c = L.case_table(4, False)
    full = c["npad"] == 0
    # g boundaries: the unpadded boundary lanes' centres are within 2 ulp (of x_c, times aC) of a boundary, on both sides
    sel = np.where((c["kind"] == 0) & full)[0]
    d = np.min(np.abs(c["numc"][sel][:, None] - gb[None, :]), axis=1)
    assert np.all(d <= 2 * 8.0 * np.spacing(16.5)) and np.any(d == 0.0)
    # h ties: H_INV (y_c - H_LO) is exactly an integer (kind 2) or an integer + 1/2 (kind 3), in exact arithmetic
    for kd, frac in ((2, 0), (3, mp.mpf(1) / 2)):
        for i in np.where((c["kind"] == kd) & full)[0]:
            v = (_exact(c["x"][i, 2]) + _exact(c["wk"][i, 3])) * int(L.H_INV)
            assert v - mp.floor(v) == frac, (i, v)
            assert float(v) == c["hx"][i]
            # and the device's own argument, x_c + cYs, is exact as well
            s = _exact(c["x"][i, 2]) + _exact(c["wk"][i, 2])
            assert mp.mpf(float(s)) == s
    assert np.any(np.signbit(c["numc"]) & (c["numc"] == 0.0)) or np.any(np.signbit(L.case_table(2, False)["numc"]) & (L.case_table(2, False)["numc"] == 0.0))


def test_cell_records_fill_their_radius():
    c = L.case_cells()
    assert set(c["nsrc"].tolist()) == {1, 4, 1000}
    cd = c["cd"]
    assert np.array_equal(cd[:, 1], c["nsrc"].astype(float))                  # S_0 = the number of sources
    # S_2 / S_0 <= rho^2, and the cells with all sources at +rho reach it
    r2 = cd[:, 3] / cd[:, 1] / c["rho"] ** 2
    assert np.all(r2 <= 1.0 + 1e-6) and np.any(r2 > 0.99)
    assert np.all(np.isfinite(c["yard"])) and np.all(c["yard"] > 0)


def test_reduction_vectors_are_exact_in_any_order():
    exact, seeded = L.reduction_vectors()
    assert exact.shape[1] == 64 and len(exact) >= 64 + 80 and len(seeded) >= 100
    assert np.array_equal(exact[:64] != 0, np.eye(64, dtype=bool))
    for v in exact:
        s = math.fsum(v)
        assert np.sum(v) == s and np.sum(v[::-1]) == s and np.sum(np.sort(np.abs(v)) * 0 + v[np.argsort(np.abs(v))]) == s


def test_numpy_figures_behind_the_caps():
    """max err / yardstick of the same expressions in plain NumPy binary64, against the 40-digit values: the caps of the GPU
    tests are 4 x these and never below 2 (lf_problib.CAPS holds them as constants; this test says when they have moved)."""
    cases = {
        "fexp_t": L.case_fexp_t(), "fexp_neg": L.case_fexp_neg(), "fexp_c": L.case_fexp_c(), "dexp": L.case_dexp(),
        "flog_half": L.case_flog_half(), "flog_half_upper": L.case_flog_half_upper(), "dlog": L.case_dlog(),
        "frsqrt": L.case_frsqrt(), "drsqrt": L.case_frsqrt(),
        "ln_fc_fast": L.case_ln_fc(), "ln_fc_careful": L.case_ln_fc(),
        "term_free_fast": L.case_term_free(), "term_free_noexp": L.case_term_free()["noexp"],
        "term_free_careful": L.case_term_careful(),
        "lnT_zevol": L.case_zevol()["lnT"], "v_zevol": L.case_zevol()["v"],
    }
    figs = {k: L.numpy_figure(k, c) for k, c in cases.items()}
    figs["table_terms"] = max(L.numpy_figure("table_terms", L.case_table(st, ne)) for st in (2, 4, 8) for ne in (False, True))
    figs["cell_sum"] = L.numpy_figure("cell_sum", L.case_cells())
    for k, (fig, i) in figs.items():
        print("numpy %-18s max err / yard %9.3f at index %d   cap %g" % (k, fig, i, L.CAPS[k]))
    for k, (fig, i) in figs.items():
        assert math.isfinite(fig), k
        # the constant is 4 x the figure measured when it was written (never below 2): it may not have drifted by more
        # than the last digit it was rounded to
        assert L.cap_from(fig) <= L.CAPS[k] * 1.05 and L.cap_from(fig) >= L.CAPS[k] * 0.8, (k, fig, L.CAPS[k])
