"""The device functions of the mock catalogues (csrc/lf_mock.h, csrc/lf_mock_noise.h) element by element on the GPU: the
cumulative sums bit for bit against mock.scan, against exact prefix sums and against their contract; the node search
against a linear search at every entry of the sums and its ulp neighbours; the Poisson draws draw for draw against
mock.poisson and against the exact pmf; the hat inversion, the Stirling series, the error model's interpolants and the noise
against 40-digit values (inputs, references, yardsticks and caps: tests/lf_mockproblib.py; the probe kernels:
tests/mock_probe.hip, compiled once per module with the library's own flags).

Each test prints its measured figure, then asserts it.  DESIGN.md section 3.11 records the figures."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import lf_mockproblib as M
from lumfuncmcmc_amd import build, capi, mock

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_dp, _ip, _lp, _up = (ctypes.POINTER(t) for t in (ctypes.c_double, ctypes.c_int, ctypes.c_longlong, ctypes.c_uint))


def _d(a):
    return a.ctypes.data_as(_dp)


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("mock_probe") / "mock_probe.so")
    subprocess.run([build.hipcc()] + build.CXXFLAGS + ["-fPIC", "-shared", "-o", so, os.path.join(ROOT, "tests", "mock_probe.hip")], check=True)
    capi.load()          # first: it brings in the process's one HIP runtime (capi.load says why), which the probe must share
    lib = ctypes.CDLL(so)
    lib.mp_poisson.argtypes = [_dp, _lp, ctypes.c_int, ctypes.c_uint64, _lp, ctypes.c_int]
    lib.mp_noise.argtypes = [_lp, _up, _ip, ctypes.c_uint64, _dp, ctypes.c_int]
    assert lib.mp_device_count() >= 1, "no GPU"
    return lib


def check(name, fig, i, got, ref, cases, gots):
    """prints the figure and, since the device's library functions are not NumPy's, in how many elements the two differ"""
    cap = M.CAPS[name]
    differ = sum(int((g != c["np"]).sum()) for c, g in zip(cases, gots))
    print("%-8s device max err / yard %9.5f (cap %g) at index %s: got %.17g ref %.17g; %d of %d results differ from NumPy's"
          % (name, fig, cap, i, got, ref, differ, sum(len(g) for g in gots)))
    assert fig <= cap, (name, fig, cap, i)


# ---------------------------------------------------------------------------------------------- the cumulative sums
def device_cdf(lib, X):
    """mock_cdf of the rows of X, at most NMAX elements a call"""
    X = M.f64(X)
    narr, n = X.shape
    c, tot = np.full(X.shape, -12345.0), np.full(narr, -12345.0)
    per = max(1, M.NMAX // n)
    for i in range(0, narr, per):
        k = min(per, narr - i)
        assert k * n <= M.NMAX
        rc = lib.mp_cdf(_d(X[i:i + k]), k, n, _d(c[i:i + k]), _d(tot[i:i + k]))
        assert rc == 0, rc
    return c, tot


@pytest.mark.parametrize("n", M.LENGTHS)
def test_cumulative_sums(probe, n):
    X = M.scan_inputs(n)
    names = sorted(X)
    c, tot = device_cdf(probe, np.array([X[k] for k in names]))
    worst = 0.0
    for i, name in enumerate(names):
        want, wtot = mock.scan(X[name])
        assert c[i].tobytes() == want.tobytes(), (name, np.flatnonzero(c[i] != want)[:5])            # (a)
        assert tot[i] == wtot, name
        worst = max(worst, M.scan_error(X[name], c[i]))                                             # (b)
        assert M.contract_violations(X[name], c[i]) == (0, 0), name                                 # (c)
    print("scan n = %4d  device max err / ((9 + T) 2^-53 prefix) %.3f (bound 1)" % (n, worst))
    assert worst <= M.SCAN_BOUND


# ---------------------------------------------------------------------------------------------- the node search
def device_search(lib, v, t):
    v, t = M.f64(v), M.f64(t)
    out = np.full(len(t), -7, dtype=np.int32)
    for i in range(0, len(t), M.NMAX):
        k = min(M.NMAX, len(t) - i)
        rc = lib.mp_search(_d(v), len(v), _d(t[i:i + k]), out[i:i + k].ctypes.data_as(_ip), k)
        assert rc == 0, rc
    return out


@pytest.mark.parametrize("n", M.LENGTHS)
def test_node_search(probe, n):
    total = 0
    for kind in sorted(M.scan_inputs(n)):
        v, t, want = M.search_case(n, kind)
        got = device_search(probe, v, t)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (kind, bad[:5], t[bad[:5]], got[bad[:5]], want[bad[:5]])
        total += len(t)
    print("search n = %4d  %d arrays, %d thresholds, 0 differ from the linear search" % (n, len(M.scan_inputs(n)), total))


# ---------------------------------------------------------------------------------------------- the hat inversion
def test_hat_inversion(probe):
    c = M.case_hat()
    n = len(c["u"])
    got = np.full(n, -12345.0)
    assert probe.mp_hat(_d(c["x0"]), _d(c["a"]), _d(c["b"]), _d(c["u"]), _d(got), n) == 0
    fig, i = M.measure(c, got)
    check("hat", fig, i, got[i], c["ref"][0][i], [c], [got])
    assert M.hat_order_violations(c, got) == (0, 0)


def test_stirling_series(probe):
    c = M.case_loggam()
    n = len(c["x"])
    got = np.full(n, -12345.0)
    assert probe.mp_loggam(_d(c["x"]), _d(got), n) == 0
    fig, i = M.measure(c, got)
    check("loggam", fig, i, got[i], c["ref"][0][i], [c], [got])
    assert got[0] == 0.0 and got[1] == 0.0                      # x = 1 and x = 2: exactly 0


# ---------------------------------------------------------------------------------------------- the Poisson draws
def device_poisson(lib, mu, rid, f, seed):
    mu, rid = M.f64(mu), np.ascontiguousarray(rid, dtype=np.int64)
    k = np.full(len(mu), -99, dtype=np.int64)
    for i in range(0, len(mu), M.NMAX):
        m = min(M.NMAX, len(mu) - i)
        rc = lib.mp_poisson(_d(mu[i:i + m]), rid[i:i + m].ctypes.data_as(_lp), f, seed, k[i:i + m].ctypes.data_as(_lp), m)
        assert rc == 0, rc
    return k


@pytest.mark.parametrize("mu", M.POISSON_MEANS)
def test_poisson_draws(probe, mu):
    n = M.POISSON_DRAWS
    rid = np.arange(n, dtype=np.int64)
    k = device_poisson(probe, np.full(n, mu), rid, M.POISSON_FIELD, M.POISSON_SEED)
    want = mock.poisson(np.full(n, mu), rid, M.POISSON_FIELD, M.POISSON_SEED)
    bad = np.flatnonzero(k != want)
    print("poisson mean %-22r %d of %d draws differ from mock.poisson; device mean of the draws %.6g" % (mu, bad.size, n, k.mean()))
    assert (k >= 0).all()
    # a comparison that falls the other way through a one-ulp difference of a library function has probability of order
    # 1e-13 per draw: a mismatch is a finding
    assert bad.size == 0, (mu, bad[:5], k[bad[:5]], want[bad[:5]])
    M.poisson_fit(k, mu)


def test_poisson_refuses_what_it_must(probe):
    mu = np.array(M.POISSON_REFUSED + (0.0,))
    k = device_poisson(probe, mu, np.arange(len(mu)), M.POISSON_FIELD, M.POISSON_SEED)
    assert (k[:-1] == -1).all() and k[-1] == 0, k


# ---------------------------------------------------------------------------------------------- the error model, the noise
def test_sigma_lookup(probe):
    cases, gots = M.case_sigma(), []
    for c in cases:
        got = np.full(len(c["t"]), -12345.0)
        assert probe.mp_sigma(_d(c["nodes"]), _d(c["sig"]), len(c["nodes"]), _d(c["t"]), _d(got), len(got)) == 0
        gots.append(got)
    fig, (k, i) = M.worst(cases, gots)
    check("sigma", fig, (k, i), gots[k][i], cases[k]["ref"][0][i], cases, gots)


def test_log_flux(probe):
    cases, gots = M.case_logflux(), []
    for c in cases:
        got = np.full(len(c["z"]), -12345.0)
        assert probe.mp_logflux(_d(c["zarr"]), _d(c["ld2n"]), len(c["zarr"]), _d(c["z"]), _d(c["L"]), _d(got), len(got)) == 0
        gots.append(got)
    fig, (k, i) = M.worst(cases, gots)
    check("logflux", fig, (k, i), gots[k][i], cases[k]["ref"][0][i], cases, gots)


def test_noise(probe):
    cases, gots = M.case_noise(), []
    for c in cases:
        got = np.full(len(c["index"]), np.nan)
        rc = probe.mp_noise(c["row_id"].ctypes.data_as(_lp), c["index"].ctypes.data_as(_up), c["field"].ctypes.data_as(_ip), c["seed"],
                            _d(got), len(got))
        assert rc == 0
        assert np.all(np.isfinite(got))
        gots.append(got)
    fig, (k, i) = M.worst(cases, gots)
    check("noise", fig, (k, i), gots[k][i], cases[k]["ref"][0][i], cases, gots)
