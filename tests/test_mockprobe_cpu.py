"""The element-wise probes of the mock catalogues' device functions without a GPU: tests/mock_probe.hip cross-compiles for
gfx950 with the library's flags and its kernels use no scratch; every generator of tests/lf_mockproblib.py yields what it
promises; the twin's cumulative sums meet the contract of csrc/lf_mock.h on every probe input; and the NumPy binary64
figures that the caps of tests/test_gpu_mockprobe.py rest on are measured and printed."""
import math
import os

import numpy as np
import pytest

import lf_isalib
import lf_mockproblib as M
from lumfuncmcmc_amd import mock

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "mock_probe.hip")


def test_probe_unit_compiles_for_gfx950_and_its_kernels_use_no_scratch():
    seen = {name: r for name, r in lf_isalib.remarks(SRC, "-c").items() if "probe_" in name and "ScratchSize" in r}
    assert len(seen) == 8, sorted(seen)          # cdf, search, hat, loggam, poisson, sigma, logflux, noise
    assert all(r["ScratchSize"] == 0 for r in seen.values()), seen
    lds = {name: r["LDS Size"] for name, r in seen.items()}
    assert sorted(lds.values()) == [0] * 7 + [2048], lds          # the one tile of mock_cdf


@pytest.mark.parametrize("n", M.LENGTHS)
def test_scan_inputs_and_the_twins_sums(n):
    """the inputs are what scan_inputs promises; on each, mock.scan meets (b) the error bound against the exact prefix sums
    and (c) the contract, and its total is the sum scan's carry"""
    X = M.scan_inputs(n)
    want = {"masses", "masses_b", "zeros", "decades", "decades_zeros", "subnormals"} | {"one_at_%d" % p for p in (0, 255, 256, n - 1) if p < n}
    assert set(X) == want
    for name, x in X.items():
        assert x.shape == (n,) and (x >= 0).all(), name
        if name.startswith("one_at_"):
            assert (x > 0).sum() == 1 and x[int(name[7:])] > 0
    if n >= 255:
        for name in ("masses", "masses_b", "decades_zeros", "subnormals"):
            assert (X[name] == 0).any() and (X[name] > 0).any(), name
        d = X["decades"]
        assert math.log10(d.max() / d.min()) > 290
        s = X["subnormals"]
        assert s.max() < 2.0 ** -1022 and s.max() > 0
    P = M.exact_prefixes(X["decades"][:50])
    assert [float(p) for p in P] == [math.fsum(X["decades"][:j + 1]) for j in range(len(P))]
    worst = 0.0
    for name, x in X.items():
        c, total = mock.scan(x)
        assert M.contract_violations(x, c) == (0, 0), name
        worst = max(worst, M.scan_error(x, c))
        assert abs(total - math.fsum(x)) <= (9 + (n - 1) // M.TILE) * M.U53 * M.SCAN_BOUND * math.fsum(x), name
    print("scan n = %4d  twin max err / ((9 + T) 2^-53 prefix) %.3f" % (n, worst))
    assert worst <= M.SCAN_BOUND


def test_the_sum_scan_alone_breaks_the_contract_and_the_bound_counts_its_tiles():
    """why the running maximum is there: without it the sums of real masses go down and step at zero masses (so the checks
    above can fail); and an error of more than 9 units needs the tiles the bound counts"""
    x = M.scan_inputs(4096)["masses"]
    c = mock.scan(x)[0]
    raw = np.empty_like(x)
    carry = 0.0
    for base in range(0, len(x), M.TILE):
        t = x[base:base + M.TILE].copy()
        d = 1
        while d < M.TILE:
            t[d:] = t[:-d] + t[d:]
            d <<= 1
        raw[base:base + M.TILE] = carry + t
        carry = carry + t[-1]
    dec, zst = M.contract_violations(x, raw)
    assert dec > 0 and zst > 0, (dec, zst)
    assert np.array_equal(c, np.maximum.accumulate(np.where(x > 0, raw, 0.0)))
    # on the raw sums bisection and the linear search part; on the stored ones, next to them, they agree.  (The raw sums
    # also show that first_above is the linear scan and not a bisection in disguise.)
    tr = M.search_thresholds(raw)
    assert np.array_equal(M.first_above(raw, tr), M.first_above_brute(raw, tr))
    assert (M.bisect_above(raw, tr) != M.first_above(raw, tr)).any()
    v, t, want = M.search_case(4096, "masses")
    assert np.array_equal(v, c) and np.array_equal(want, M.first_above_brute(v, t))
    assert np.array_equal(M.bisect_above(v, t), want)


@pytest.mark.parametrize("n", M.LENGTHS)
def test_search_cases_cover_their_thresholds_and_bisection_agrees_on_the_twins_sums(n):
    for kind in sorted(M.scan_inputs(n)):
        v, t, want = M.search_case(n, kind)
        assert len(t) == 5 * n + 5
        assert np.all(np.isin(v, t)) and np.all(np.isin(np.nextafter(v, np.inf), t)) and np.all(np.isin(np.nextafter(v, -np.inf), t))
        assert {0.0, -1.0, v[-1], np.inf} <= set(t.tolist()) and np.nextafter(v[-1], np.inf) in t
        assert want.min() >= 0 and want.max() < n
        # no threshold t >= 0 (a source's is u M >= 0) selects a node of zero mass (all-zero sums: the fallback's index 0)
        x = M.scan_inputs(n)[kind]
        if (x > 0).any():
            assert (x[want[t >= 0]] > 0).all(), kind
        else:
            assert (want == 0).all(), kind
        assert np.array_equal(M.bisect_above(v, t), want), kind
        if kind == "subnormals" and n >= 255:          # the sums and their ulp neighbours are themselves subnormal
            assert 0 < v[-1] < 2.0 ** -1022 and (np.diff(np.unique(t[np.isfinite(t) & (t >= 0)])) == 5e-324).any()
        if kind.startswith("one_at_"):                 # the pure step: every t in [0, 0.3) finds the one node with mass
            assert (want[(t >= 0) & (t < 0.3)] == int(kind[7:])).all()


def test_hat_inputs_and_order():
    c = M.case_hat()
    D = M.hat_designs()
    assert (D[:, 1] == 0).sum() >= 2 and (D[:, 2] == 0).sum() >= 2
    ratio = D[:, 1] / np.where(D[:, 2] > 0, D[:, 2], np.nan)
    assert np.nanmax(ratio) >= 1.0e6 and np.nanmin(ratio[ratio > 0]) <= 1.0e-6
    u, a, b = c["u"], c["a"], c["b"]
    assert u.min() == 0.0 and u.max() == 1.0 - M.U53 and M.U53 in u and (u < 1).all()
    for g in range(len(D)):
        ug, br = u[c["group"] == g], D[g, 1] / (D[g, 1] + D[g, 2])
        for p in M.ulps_around(br):
            assert p in ug or not 0.0 <= p < 1.0, (g, p)
        assert len(ug) >= 50
    assert np.all(np.isfinite(c["ref"][0])) and np.all(c["yard"] > 0)
    assert M.hat_order_violations(c, c["np"]) == (0, 0)


def test_loggam_sigma_logflux_and_noise_inputs():
    x = M.case_loggam()["x"]
    assert np.all(np.isin(np.arange(41) + 1.0, x)) and np.nextafter(7.0, 0.0) in x and np.nextafter(7.0, 8.0) in x
    assert np.all(np.isin(10.0 ** np.arange(1, 10), x)) and 2.0 ** 31 + 1.0 in x and x.min() >= 1.0
    S = M.case_sigma()
    assert sorted({len(c["nodes"]) for c in S}) == [1, 2, 64]
    for c in S:
        nodes, t = c["nodes"], c["t"]
        assert np.all(np.isin(M.ulps_around(nodes), t)) and t.min() < nodes[0] - 1 and t.max() > nodes[-1] + 1
        assert np.all(np.diff(nodes) > 0) and (c["sig"] >= 0).all()
    assert sum((c["sig"] == 0).any() and (c["sig"] > 0).any() for c in S) >= 4 and any((c["sig"] == 0).all() for c in S)
    F = M.case_logflux()
    assert [len(c["zarr"]) for c in F] == [2, 201]
    for c in F:
        zarr, z = c["zarr"], c["z"]
        assert np.all(np.isin(M.ulps_around(zarr), z)) and z.min() < zarr[0] and z.max() > zarr[-1]
    for c in M.case_noise():
        assert c["index"].max() == (1 << 32) - 1 and c["index"].min() == 0 and c["row_id"].max() >= (1 << 62) - 1
        assert set(c["field"].tolist()) == set(range(5)) and (c["u1"] < 1).all()
        assert np.all(np.isfinite(c["np"]))


def test_numpy_figures_behind_the_caps():
    """max err / yardstick of the same expressions in NumPy binary64 (mock.py), against the 40-digit values: the caps of the
    GPU tests are 4 x these and never below 2 (lf_mockproblib.CAPS holds them as constants; this test says when they have
    moved)."""
    figs = {"hat": M.numpy_figure("hat", M.case_hat()), "loggam": M.numpy_figure("loggam", M.case_loggam())}
    for name, cases in (("sigma", M.case_sigma()), ("logflux", M.case_logflux()), ("noise", M.case_noise())):
        figs[name] = M.worst(cases, [c["np"] for c in cases])
        M.NUMPY_FIGURES[name] = figs[name]
    for k, (fig, i) in figs.items():
        print("numpy %-8s max err / yard %9.5f at index %s   cap %g" % (k, fig, i, M.CAPS[k]))
    for k, (fig, i) in figs.items():
        assert math.isfinite(fig), k
        assert M.cap_from(fig) <= M.CAPS[k] * 1.05 and M.cap_from(fig) >= M.CAPS[k] * 0.8, (k, fig, M.CAPS[k])


def test_poisson_lists():
    assert len(M.POISSON_MEANS) == 12 and M.POISSON_DRAWS == 40000
    assert {5e-324, 10.0, 2.0 ** 31} <= set(M.POISSON_MEANS) and np.nextafter(10.0, 0.0) in M.POISSON_MEANS
    got = mock.poisson(np.array(M.POISSON_REFUSED), np.arange(4, dtype=np.int64), M.POISSON_FIELD, M.POISSON_SEED)
    assert (got == -1).all()
