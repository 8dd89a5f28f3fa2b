"""Inputs, references and yardsticks for the element-wise probes of the mock catalogues' device functions (csrc/lf_mock.h,
csrc/lf_mock_noise.h): the cumulative sums, the node search, the hat inversion, the Stirling series, the Poisson draws, the
error model's two interpolants and the noise.  No GPU here: tests/test_mockprobe_cpu.py checks that every generator yields
what it promises and measures the NumPy binary64 figures, tests/test_gpu_mockprobe.py runs the same cases through
tests/mock_probe.hip.

The rule is lf_problib's, unchanged.  A floating-point case is a dict: the input arrays, `ref` = the value at 40 digits from
the exact binary64 inputs as a (hi, lo) pair, `yard` = the unit the error is expressed in, `np` = the same expression in
NumPy binary64 (lumfuncmcmc_amd/mock.py).  Every yardstick follows from the number format and the formula; each case's
docstring says which terms it has.  The cap on the device's max err / yard is max(2, 4 x the NumPy figure).  No input is
exempt.  The cumulative sums, the search and the Poisson draws are compared exactly instead (bits, indices, draws)."""
import functools
import math
from fractions import Fraction

import mpmath as mp
import numpy as np

import lf_testlib as T
from lf_problib import NMAX, U53, cap_from, err_of, f64, measure, mpf, pair, ulp_of, ulps_around    # noqa: F401
from lumfuncmcmc_amd import mock, philox, synth

mp.mp.dps = 40

# Caps K on max err / yard, per probed function: max(2, 4 x the NumPy binary64 figure on the same inputs), the figures
# measured by tests/test_mockprobe_cpu.py::test_numpy_figures_behind_the_caps (which asserts that they still hold) on
# 2026-10-20; DESIGN.md section 3.11 has the device's figures next to them.
CAPS = {"hat": 2.05, "loggam": 5.07, "sigma": 2.0, "logflux": 2.0, "noise": 4.73}
NUMPY_FIGURES = {}


def numpy_figure(name, case):
    fig = measure(case, case["np"])
    NUMPY_FIGURES[name] = fig
    return fig


def _finish(case):
    assert len(case["yard"]) <= NMAX, len(case["yard"])
    return case


# ---------------------------------------------------------------------------------------------- the cumulative sums
LENGTHS = (1, 2, 255, 256, 257, 511, 512, 513, 4096)
TILE = mock.SCAN_TILE


@functools.lru_cache(None)
def _mass_pool():
    """Real masses, column after column: MockTwin.masses of a z-evolving row whose bright end underflows to exact zeros"""
    inp = T.make_inputs("zevol", 500, S=201, nf=2)
    th = synth.walkers("zevol", 4, seed=5)[1]
    return np.ascontiguousarray(np.swapaxes(mock.MockTwin(inp).masses(th), 1, 2)).ravel()


@functools.lru_cache(None)
def scan_inputs(n):
    """{name: n masses >= 0}: real masses (zeros included), all zeros, one positive value among zeros at 0, 255, 256 and
    n - 1, values spread over 300 decades, subnormals (multiples of 2^-1074, zeros among them)"""
    rng = np.random.default_rng(1000 + n)
    pool = _mass_pool()
    zb = np.flatnonzero(pool == 0.0)
    b0 = int(zb[zb > 20000][0]) - 100                      # a window that meets a column's zeros after 100 nodes with mass
    out = {"masses": pool[:n].copy(), "masses_b": pool[b0:b0 + n].copy(), "zeros": np.zeros(n)}
    for p in sorted({0, 255, 256, n - 1}):
        if p < n:
            x = np.zeros(n)
            x[p] = 0.3
            out["one_at_%d" % p] = x
    out["decades"] = 10.0 ** rng.uniform(-150.0, 150.0, n)
    dz = 10.0 ** rng.uniform(-150.0, 150.0, n)
    dz[rng.uniform(0, 1, n) < 0.3] = 0.0
    out["decades_zeros"] = dz
    out["subnormals"] = rng.integers(0, 1 << 20, n) * (rng.uniform(0, 1, n) < 0.8) * 5e-324
    return {k: f64(v) for k, v in out.items()}


def exact_prefixes(x):
    """the exact prefix sums of x as rationals (math.fsum(x[:j + 1]) is float() of entry j)"""
    out, s = [], Fraction(0)
    for v in x:
        s += Fraction(float(v))
        out.append(s)
    return out


def scan_error(x, c):
    """max over j of |c[j] - P[j]| / ((9 + T) 2^-53 P[j]), P the exact prefix sums and T = j // 256 the tiles before the
    element: a tile's scan is a tree 8 adds deep, the carry is added once, and the carry has taken T additions.  A prefix
    of 0 must be 0 exactly (ratio 0, else inf)."""
    worst = 0.0
    for j, (P, v) in enumerate(zip(exact_prefixes(x), c)):
        e = abs(Fraction(float(v)) - P)
        if P == 0:
            r = 0.0 if e == 0 else math.inf
        else:
            r = float(e / (P * Fraction((9 + j // TILE)) * Fraction(U53)))
        worst = max(worst, r)
    return worst


SCAN_BOUND = 1.0 + 1.0e-12          # "(9 + T) 2^-53 to first order": the second-order term is (9 + T) 2^-54 of it, < 3e-15


def contract_violations(x, c):
    """(steps where c decreases, nodes of zero mass with a step), along the last axis; c[-1] counts as 0"""
    x, c = np.asarray(x), np.asarray(c)
    step = np.diff(np.concatenate([np.zeros(c.shape[:-1] + (1,)), c], axis=-1), axis=-1)
    return int((step < 0).sum()), int(((x == 0) & (step != 0)).sum())


# ---------------------------------------------------------------------------------------------- the node search
def first_above(v, t):
    """The contract of mock_search, as a linear search states it: per t the first index with v > t, else the first with
    v >= v[-1].  For ANY v (monotone or not) the first index with v > t is the first at which the running maximum of v
    exceeds t, and the running maximum is non-decreasing, so one searchsorted on it finds that index; this is the linear
    search's answer, not a bisection of v (first_above_brute is the literal scan, tests/test_mockprobe_cpu.py compares
    the two on sums that do go down)."""
    v, t = np.asarray(v), np.asarray(t)
    out = np.searchsorted(np.maximum.accumulate(v), t, side="right")
    return np.where(out < len(v), out, int((v >= v[-1]).argmax()))


def first_above_brute(v, t):
    """first_above by comparing every entry with every threshold"""
    v, t = np.asarray(v), np.asarray(t)
    out = np.empty(len(t), dtype=np.int64)
    top = int((v >= v[-1]).argmax())
    step = max(1, (1 << 24) // len(v))
    for i in range(0, len(t), step):
        above = v[None, :] > t[i:i + step, None]
        out[i:i + step] = np.where(above.any(axis=1), above.argmax(axis=1), top)
    return out


def bisect_above(v, t):
    """mock_search's own bisection, restated for the CPU test of the twin's sums: it equals first_above where v is
    non-decreasing and may differ where it is not"""
    v, t = np.asarray(v), np.asarray(t)
    n = len(v)
    lo, hi = np.zeros(len(t), dtype=np.int64), np.full(len(t), n, dtype=np.int64)
    while (lo < hi).any():
        act = lo < hi
        mid = (lo + hi) >> 1
        up = act & (v[np.minimum(mid, n - 1)] > t)
        hi = np.where(up, mid, hi)
        lo = np.where(act & ~up, mid + 1, lo)
    none = lo >= n
    lo2, hi2 = np.zeros(len(t), dtype=np.int64), np.full(len(t), n - 1, dtype=np.int64)
    while (lo2 < hi2).any():
        act = lo2 < hi2
        mid = (lo2 + hi2) >> 1
        up = act & (v[mid] >= v[-1])
        hi2 = np.where(up, mid, hi2)
        lo2 = np.where(act & ~up, mid + 1, lo2)
    return np.where(none, lo2, lo)


def search_thresholds(v):
    """every entry of v and its neighbours at +-1 and +-2 ulps; 0, a negative t, the top, just above the top, +inf"""
    top = v[-1]
    return f64(np.concatenate([ulps_around(v), [0.0, -1.0, top, np.nextafter(top, np.inf), np.inf]]))


@functools.lru_cache(None)
def search_case(n, kind):
    """(v, t, want): v = mock.scan of scan_inputs(n)[kind], for every kind of scan_inputs(n)"""
    v = mock.scan(scan_inputs(n)[kind])[0]
    t = search_thresholds(v)
    return v, t, first_above(v, t)


# ---------------------------------------------------------------------------------------------- the hat inversion
def hat_designs():
    """(x0, a, b): ordinary nodes, the grid's two ends (a = 0, b = 0), width ratios 10^-6 .. 10^6, a seeded fill, and one
    design at whose branch point the uncapped root exceeds 1 (x would step back below x0 there)"""
    rng = np.random.default_rng(2001)
    D = [(1.5, 0.0037, 0.0037), (42.0, 0.0125, 0.0125), (1.16, 0.0, 0.0037), (1.9, 0.0037, 0.0), (41.0, 0.0, 0.0125),
         (43.5, 0.0125, 0.0), (1.0, 0.23056352117316764, 0.28900982527137853)]
    for k in range(1, 7):
        D += [(42.0, 10.0 ** -k, 1.0), (42.0, 1.0, 10.0 ** -k), (1.5, 3.0e-7 * 10.0 ** k, 3.0e-7)]
    D += [(rng.uniform(1.0, 44.0), rng.uniform(0.001, 0.1), rng.uniform(0.001, 0.1)) for _ in range(54)]
    return np.array(D)


@functools.lru_cache(None)
def case_hat():
    """mock_hat.  Per design a sorted list of u: 0, 2^-53, the branch point a / (a + b) and its neighbours at +-1 and +-2
    ulps, a uniform fill, 1 - 2^-53 (all in [0, 1)).  Reference: the exact inverse of the hat's distribution function at the
    binary64 inputs.  Yardstick: ulp of the result + 2^-53 w, w the width of the side taken - the formula forms x as
    x0 -+ w (1 - s) and the roundings of s and of 1 - s enter at the size of w, whatever is left after the cancellation
    against x0.  Within 4 ulps of the branch point either side's formula may be the one taken (both give x0 there): w is
    the larger width."""
    rng = np.random.default_rng(2002)
    X0, A, B, Uu, G, near = [], [], [], [], [], []
    for g, (x0, a, b) in enumerate(hat_designs()):
        br = a / (a + b)
        u = np.concatenate([[0.0, U53, 1.0 - U53], ulps_around(br), rng.uniform(0.0, 1.0, 50)])
        u = np.unique(u[(u >= 0.0) & (u < 1.0)])
        X0.append(np.full(len(u), x0)); A.append(np.full(len(u), a)); B.append(np.full(len(u), b)); Uu.append(u)
        G.append(np.full(len(u), g))
        near.append(np.abs(u - br) <= 4 * np.spacing(br))
    x0, a, b, u, g, near = (np.concatenate(v) for v in (X0, A, B, Uu, G, near))
    refs, w = [], np.empty(len(u))
    for i in range(len(u)):
        ma, mb, mu_ = mpf(a[i]), mpf(b[i]), mpf(u[i])
        ab = ma + mb
        if mu_ * ab < ma:
            refs.append(mpf(x0[i]) - ma * (1 - mp.sqrt(mu_ * ab / ma)))
            w[i] = a[i]
        else:
            refs.append(mpf(x0[i]) + mb * (1 - mp.sqrt((1 - mu_) * ab / mb)))
            w[i] = b[i]
    w = np.where(near, np.maximum(a, b), w)
    ref = pair(refs)
    return _finish({"x0": f64(x0), "a": f64(a), "b": f64(b), "u": f64(u), "group": g, "ref": ref, "yard": ulp_of(ref) + U53 * w,
                    "np": mock.hat_inverse(x0, a, b, u)})


def hat_order_violations(case, x):
    """(results outside [x0 - a, x0 + b] as rounded, decreases of x along a design's sorted u)"""
    out = int(((x < case["x0"] - case["a"]) | (x > case["x0"] + case["b"])).sum())
    same = np.diff(case["group"]) == 0
    assert np.all(np.diff(case["u"])[same] > 0)
    return out, int((np.diff(x)[same] < 0).sum())


# ---------------------------------------------------------------------------------------------- the Stirling series
@functools.lru_cache(None)
def case_loggam():
    """mock_loggam against mpmath.loggamma: x = k + 1 for k = 0 .. 40 (the arguments of small counts), both sides of 7 (where
    the recurrence starts), powers of ten up to 2^31 + 1, a seeded fill.  Yardstick: ulp of the result + 2^-53 times the
    terms the formula cancels: (x0 - 1/2) ln x0 and x0 of the series at x0 = x + n >= 7, and the n logarithms the
    recurrence takes off below 7."""
    rng = np.random.default_rng(2003)
    x = f64(np.concatenate([np.arange(41) + 1.0, ulps_around(7.0), [6.5, 6.999, 7.001, 7.5], 10.0 ** np.arange(1, 10),
                            [2.0 ** 31, 2.0 ** 31 + 1.0], rng.uniform(1.0, 50.0, 200), 10.0 ** rng.uniform(0.0, 9.33, 200)]))
    ref = pair([mp.loggamma(mpf(v)) for v in x])
    n = np.where(x < 7.0, np.floor(7.0 - x), 0.0)
    x0 = x + n
    cond = np.abs((x0 - 0.5) * np.log(x0)) + x0
    for k in range(1, 7):
        cond = cond + np.where(n >= k, np.abs(np.log(np.maximum(x0 - k, 1.0))), 0.0)
    with np.errstate(divide="ignore"):
        npv = mock.loggam(x)
    return _finish({"x": x, "ref": ref, "yard": ulp_of(ref) + U53 * cond, "np": npv})


# ---------------------------------------------------------------------------------------------- the Poisson draws
POISSON_DRAWS = 40000
POISSON_MEANS = (5e-324, 1e-300, 1e-3, 0.5, 5.0, float(np.nextafter(10.0, 0.0)), 10.0, float(np.nextafter(10.0, np.inf)), 37.0,
                 1.0e4, 1.0e6, 2.0 ** 31)
POISSON_REFUSED = (np.nan, -1.0, np.inf, 1.5 * 2.0 ** 31)
POISSON_FIELD, POISSON_SEED = 3, 20260101


def _pmf(mu, k):
    return np.exp(-mu + k * math.log(mu) - np.array([math.lgamma(x + 1.0) for x in k]))


def poisson_fit(k, mu):
    """Asserts that the draws k follow Poisson(mu): chi^2 against the exact pmf over mu +- 6 sd, neighbours merged until
    every class expects >= 5 draws (both tails go into their edge classes), p > 1e-4; where fewer than two classes are
    left (almost every draw is 0), the count of non-zero draws against n (1 - e^-mu) instead."""
    from scipy import stats
    n = len(k)
    sd = math.sqrt(mu)
    lo, hi = max(0, int(mu - 6 * sd) - 1), int(mu + 6 * sd) + 2
    support = np.arange(lo, hi)
    p = _pmf(mu, support.astype(np.float64))
    obs = np.bincount(np.clip(k - lo, 0, hi - lo - 1), minlength=hi - lo)[:hi - lo].astype(float)
    exp_, got, acc_e, acc_o = [], [], 0.0, 0.0
    for e, o in zip(n * p, obs):
        acc_e += e
        acc_o += o
        if acc_e >= 5.0:
            exp_.append(acc_e)
            got.append(acc_o)
            acc_e = acc_o = 0.0
    if exp_:
        exp_[-1] += acc_e
        got[-1] += acc_o
    exp_, got = np.array(exp_), np.array(got)
    exp_ *= got.sum() / exp_.sum()
    if len(exp_) < 2:
        assert abs((k > 0).sum() - n * (1.0 - math.exp(-mu))) < 5 * math.sqrt(n * mu) + 1, (mu, int((k > 0).sum()))
        return
    chi2 = float(((got - exp_) ** 2 / exp_).sum())
    assert stats.chi2.sf(chi2, len(exp_) - 1) > 1e-4, (mu, chi2, len(exp_))


# ---------------------------------------------------------------------------------------------- the error model
def _interp_ref(x, y, i, t):
    """y[i] + (t - x[i]) (y[i + 1] - y[i]) / (x[i + 1] - x[i]) at 40 digits; also |the second term|"""
    d = (mpf(t) - mpf(x[i])) * (mpf(y[i + 1]) - mpf(y[i])) / (mpf(x[i + 1]) - mpf(x[i]))
    return mpf(y[i]) + d, abs(float(d))


@functools.lru_cache(None)
def sigma_tables():
    """(nodes, sigma row) for M = 1, 2, 64: unevenly spaced nodes; ordinary rows, rows containing zeros, a row of zeros"""
    rng = np.random.default_rng(2004)
    out = []
    for M in (1, 2, 64):
        nodes = -17.5 + np.concatenate([[0.0], np.cumsum(rng.uniform(0.01, 0.09, M - 1))])
        rows = [rng.uniform(0.01, 0.3, M), np.zeros(M)]
        z = rng.uniform(0.01, 0.3, M)
        z[::3] = 0.0
        rows.append(z)
        z = rng.uniform(0.01, 0.3, M)
        z[M // 2:] = 0.0
        rows.append(z)
        out += [(f64(nodes), f64(r)) for r in rows]
    return out


@functools.lru_cache(None)
def case_sigma():
    """mock_sigma, one sub-case per table of sigma_tables(): t at every node and its neighbours at +-1 and +-2 ulps, below and
    above the table, a fill inside.  Reference: the exact piecewise-linear interpolant of the binary64 table, constant
    outside.  Yardstick: ulp of the result + 5 x 2^-53 |D|, D = (t - x_i) slope the interpolation's second term (five
    roundings: two differences, the quotient, t - x_i, the product), which the sum with sig_i can cancel where sigma falls;
    outside the table and at M = 1 the value is a table entry (D = 0: the yardstick is the ulp)."""
    rng = np.random.default_rng(2005)
    cases = []
    for nodes, sig in sigma_tables():
        M = len(nodes)
        t = f64(np.concatenate([ulps_around(nodes), [nodes[0] - 1.0, nodes[0] - 1e-9, -1.0e300, nodes[-1] + 1e-9, nodes[-1] + 1.0, 1.0e300],
                                rng.uniform(nodes[0] - 0.05, nodes[-1] + 0.05, 80)]))
        refs, D = [], np.zeros(len(t))
        for q, v in enumerate(t):
            if not v > nodes[0]:
                refs.append(mpf(sig[0]))
            elif v >= nodes[-1]:
                refs.append(mpf(sig[-1]))
            else:
                i = int(np.searchsorted(nodes, v, side="right")) - 1
                r, D[q] = _interp_ref(nodes, sig, i, v)
                refs.append(r)
        ref = pair(refs)
        cases.append(_finish({"nodes": nodes, "sig": sig, "t": t, "ref": ref, "yard": ulp_of(ref) + 5.0 * U53 * D,
                              "np": mock.sigma_lookup(nodes, sig, t)}))
    return cases


@functools.lru_cache(None)
def case_logflux():
    """mock_logflux for S = 2 and S = 201 (the synthetic survey's redshift nodes and distances): z at every node and its
    neighbours at +-1 and +-2 ulps, below zarr[0] and above zarr[S - 1] (the end intervals, continued), a fill.  Reference:
    L - ld2(z) with the exact linear interpolant.  Yardstick: ulp of the result + 2^-53 (|ld2| + 5 |D|): the rounding of
    ld2 = ld2n_i + D enters L - ld2 at the size of ld2 (about 58 against a result near -16), and D carries five roundings."""
    rng = np.random.default_rng(2006)
    inp = T.make_inputs("zevol", 500, S=201, nf=2)
    z201, l201 = f64(inp["zarr"]), mock.ld2_nodes(inp["DL_zarr"])
    cases = []
    for zarr, ld2n in ((z201[[0, -1]].copy(), l201[[0, -1]].copy()), (z201, l201)):
        S = len(zarr)
        z = f64(np.concatenate([ulps_around(zarr), [zarr[0] - 0.1, zarr[0] - 1e-12, 0.0, zarr[-1] + 1e-12, zarr[-1] + 0.1, 10.0],
                                rng.uniform(zarr[0], zarr[-1], 200)]))
        L = rng.uniform(41.0, 44.0, len(z))
        refs, cond = [], np.zeros(len(z))
        for q, v in enumerate(z):
            i = min(max(int(np.searchsorted(zarr, v, side="right")) - 1, 0), S - 2)
            ld2, d = _interp_ref(zarr, ld2n, i, v)
            refs.append(mpf(L[q]) - ld2)
            cond[q] = abs(float(ld2)) + 5.0 * d
        ref = pair(refs)
        cases.append(_finish({"zarr": zarr, "ld2n": f64(ld2n), "z": z, "L": f64(L), "ref": ref, "yard": ulp_of(ref) + U53 * cond,
                              "np": mock.log_flux(zarr, ld2n, z, L)}))
    return cases


# ---------------------------------------------------------------------------------------------- the noise
NOISE_SEEDS = (20261020, (1 << 63) + 5)


@functools.lru_cache(None)
def case_noise():
    """mock_noise, one sub-case per seed: (row_id, index, field) lists with the ends of each range.  Reference: philox.py's
    words of block (row_id, index, purpose 3, field), u53, then sqrt(-2 ln(1 - u1)) cos(2 pi u2) at 40 digits.  Yardstick: ulp
    of the result + 2^-53 R (2 pi u2), R the radius: the angle is formed with a rounded 2 pi and one rounded product, an
    error of up to 2^-53 of its size, which the cosine passes on at up to that size whatever the result's."""
    rng = np.random.default_rng(2007)
    cases = []
    for seed, n in zip(NOISE_SEEDS, (4000, 1000)):
        rid = np.concatenate([[0, 1, (1 << 32) - 1, 1 << 32, 1 << 40, (1 << 62) - 1], rng.integers(0, 1 << 62, n - 6)]).astype(np.int64)
        idx = np.concatenate([[0, 1, (1 << 32) - 1, 1 << 31, 255, 256], rng.integers(0, 1 << 32, n - 6)]).astype(np.uint32)
        fld = (np.arange(n) % 5).astype(np.int32)
        w = mock._words(rid, idx.astype(np.uint64), mock.NOISE_PURPOSE, fld, seed)
        u1, u2 = philox.u53(w[0], w[1]), philox.u53(w[2], w[3])
        R = [mp.sqrt(-2 * mp.log(1 - mpf(a))) for a in u1]
        ref = pair([r * mp.cos(2 * mp.pi * mpf(b)) for r, b in zip(R, u2)])
        yard = ulp_of(ref) + U53 * np.array([float(r) for r in R]) * (2.0 * math.pi * u2)
        npv = np.sqrt(-2.0 * np.log1p(-u1)) * np.cos(2.0 * np.pi * u2)
        cases.append(_finish({"row_id": rid, "index": idx, "field": fld, "seed": seed, "u1": u1, "u2": u2, "ref": ref, "yard": yard,
                              "np": npv}))
    return cases


def worst(cases, gots):
    """measure() over sub-cases: (the largest max err / yard, (sub-case, index))"""
    figs = [measure(c, g) for c, g in zip(cases, gots)]
    k = int(np.argmax([f[0] for f in figs]))
    return figs[k][0], (k, figs[k][1])


# ---------------------------------------------------------------------------------------------- entry-level cases at the tile edges
EDGE_GRIDS = [(v, S) for v in ("fixcomp", "zevol") for S in (255, 256, 257, 513)] + [("free", 256), ("free", 257)]
CONTRACT_GRIDS = (("zevol", 201), ("free", 101), ("fixcomp", 257), ("zevol", 513))


@functools.lru_cache(None)
def edge_inputs(variant, S):
    return T.make_inputs(variant, 500, S=S, nf=2)


def scaled_rows(tw, variant, targets, seed=5):
    """One row of the prior box per target, phi* shifted so that the row's expected total is the target; a target of 0
    puts L* so far below the grid that every node underflows (mean exactly 0)."""
    th = synth.walkers(variant, len(targets), seed=seed, nf=tw.nf)
    phi, lstar = ([3, 4, 5], [0, 1, 2]) if variant == "zevol" else ([1], [0])
    mean = tw.means(th).sum(axis=1)
    for i, t in enumerate(targets):
        if t > 0:
            th[i, phi] += np.log10(t / mean[i])
        else:
            th[i, lstar] = 20.0
    return th


def search_disagreements(v):
    """thresholds t = an entry of v at which mock_search's bisection and the linear search find different nodes"""
    return int((bisect_above(v, v) != first_above(v, v)).sum())
