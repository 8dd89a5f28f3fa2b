"""Chain diagnostics without a GPU: the exports, the window rule in C against integrated_time's own
lines, the NumPy twin of the device's direct sums against the FFT form, the edge conventions, split-R-hat and ESS against
literal NumPy, and every argument error (refused before a device is touched).

Bounds.  Twin ACF against the FFT form: 1e-12 absolute on the normalised curve - direct summation of n terms errs by about
sqrt(n) eps a[0] (2e-14 at n = 2e4), never more than n eps a[0] (2e-12); the FFT form's own error is of order eps log2(n); the
cases have n <= 2e4.  tau with equal windows: 2 (window + 1) 1e-12, the sum of window + 1 such terms, doubled.  Windows are
compared only where the host's own curve keeps every m <= window further than 1e-6 from m = c taus[m] (asserted per case)."""
import ctypes

import numpy as np
import pytest

from lf_diaglib import CASES, ar1, fft_acf, fft_window, rhat_numpy, shifted

F64P = ctypes.POINTER(ctypes.c_double)
I64P = ctypes.POINTER(ctypes.c_int64)


@pytest.fixture(scope="module")
def lib():
    from lumfuncmcmc_amd import build, capi
    build.build_library(verbose=False)
    return capi.load()


def _p(a):
    return a.ctypes.data_as(F64P)


def c_window(lib, acf, c, n):
    acf = np.ascontiguousarray(acf, dtype=np.float64)
    tau, win = ctypes.c_double(0.0), ctypes.c_int64(-1)
    rc = lib.lf_chain_window(_p(acf), len(acf), c, n, ctypes.byref(tau), ctypes.byref(win))
    return rc, tau.value, win.value


def test_exports_and_abi(lib):
    import os
    import re
    from lumfuncmcmc_amd import capi
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "lfmcmc.h")).read()
    declared = set(re.findall(r"\b(lf_[a-z_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    for name in ("lf_chain_diag", "lf_sampler_diag", "lf_ptsampler_diag", "lf_chain_window", "lf_diag_last"):
        assert name in declared and name in capi.EXPORTS and hasattr(lib, name), name
    assert lib.lf_abi_version() == 3


@pytest.mark.parametrize("seed", range(len(CASES)))
def test_window_rule_equals_integrated_time(lib, seed):
    from lumfuncmcmc_amd.sampler import chain_window, integrated_time
    x = ar1(seed)
    n = x.shape[1]
    acf = fft_acf(x)
    tau, win, margin = fft_window(acf)
    print("case %d: n %d window %d tau %.4f margin %.3g" % (seed, n, win, tau, margin))
    assert margin > 1e-6                                     # the precondition: the window does not hang on a rounding error
    assert tau == integrated_time(x.T)                       # the helper is integrated_time's lines
    rc, ctau, cwin = c_window(lib, acf, 5.0, n)
    assert rc == 0 and cwin == win
    assert abs(ctau - tau) <= 1e-15 * abs(tau)
    assert chain_window(acf, 5.0, n) == (tau, win)
    # fewer lags than the window needs: undecided, and decided again once they are there
    assert c_window(lib, acf[:win], 5.0, n)[0] == 1 and chain_window(acf[:win], 5.0, n) is None
    assert c_window(lib, acf[:win + 1], 5.0, n) == (0, ctau, win)


@pytest.mark.parametrize("seed", range(len(CASES)))
def test_twin_against_the_fft_form(seed):
    from lumfuncmcmc_amd.sampler import chain_diagnostics_twin
    x = ar1(seed)
    W, n = x.shape
    acf = fft_acf(x)
    tau, win, margin = fft_window(acf)
    assert margin > 1e-6
    nl = min(n, 512)
    r = chain_diagnostics_twin(x[:, :, None], nlags=nl)
    err = np.max(np.abs(r.acf[0] - acf[:nl]))
    print("case %d: twin ACF max abs err %.3g, tau %.6f vs %.6f" % (seed, err, r.tau[0], tau))
    assert err <= 1e-12
    assert r.window[0] == win
    assert abs(r.tau[0] - tau) <= 2 * (win + 1) * 1e-12
    assert r.ess[0] == W * n / r.tau[0]


def test_edge_conventions(lib):
    from lumfuncmcmc_amd.sampler import chain_diagnostics_twin, chain_window, integrated_time
    rs = np.random.RandomState(7)
    # n < 4
    x = rs.standard_normal((8, 3, 2))
    r = chain_diagnostics_twin(x)
    assert np.all(r.tau == 1.0) and np.all(r.window == 0) and np.all(r.ess == 8 * 3) and np.all(np.isnan(r.rhat))
    assert c_window(lib, np.zeros(1), 5.0, 3) == (0, 1.0, 0)
    # a constant series: a[0] = 0 for every walker, ACF 0, tau -1 -> 1.0
    x = np.full((8, 50, 1), 2.5)
    r = chain_diagnostics_twin(x, nlags=50)
    assert r.tau[0] == 1.0 == integrated_time(x[:, :, 0].T) and r.window[0] == 0 and np.all(r.acf == 0.0)
    assert c_window(lib, np.zeros(50), 5.0, 50) == (0, 1.0, 0)
    # one walker constant: left out of the sum, which is still divided by W
    x = 0.01 * rs.standard_normal((8, 400, 1)) + 43.0
    x[3] = 43.0
    r = chain_diagnostics_twin(x, nlags=400)
    ref = fft_acf(x[:, :, 0])
    assert np.max(np.abs(r.acf[0] - ref)) <= 1e-12 and abs(r.acf[0, 0] - 7.0 / 8.0) < 1e-15
    assert abs(r.tau[0] - integrated_time(x[:, :, 0].T)) <= 2 * (r.window[0] + 1) * 1e-12
    # c tau reached only deep in the chain (a slow drift, c = 50): past the first 512 lags, so the lags are doubled
    x = (np.linspace(0.0, 1.0, 600)[None, :] + 1e-3 * rs.standard_normal((4, 600)))[:, :, None]
    ref_tau, ref_win, margin = fft_window(fft_acf(x[:, :, 0]), c=50.0)
    assert ref_win > 512 and margin > 1e-6
    r = chain_diagnostics_twin(x, c=50.0)
    assert r.window[0] == ref_win
    assert abs(r.tau[0] - integrated_time(x[:, :, 0].T, c=50.0)) <= 2 * (ref_win + 1) * 1e-12
    # c tau never reached within n (sum(y) = 0 makes taus[n - 1] = 0 for a real chain, so only a curve can show it): n - 1
    ones = np.ones(40)
    assert c_window(lib, ones, 5.0, 40) == (0, 79.0, 39) and chain_window(ones, 5.0, 40) == (79.0, 39)
    assert c_window(lib, ones[:20], 5.0, 40)[0] == 1
    # t0 > 0 is the diagnostics of the tail; the lnprob column is one more series
    x = ar1(2)
    lnp = -0.5 * ((x - x.mean()) / 0.01) ** 2
    chain = np.stack([x, 2.0 * x + 1.0], axis=2)
    r = chain_diagnostics_twin(chain, lnprob=lnp, t0=100)
    tail = chain_diagnostics_twin(chain[:, 100:], lnprob=lnp[:, 100:])
    assert r.tau.shape == (3,) and r.n == x.shape[1] - 100
    for k in ("tau", "window", "ess", "rhat"):
        np.testing.assert_array_equal(getattr(r, k), getattr(tail, k))
    assert abs(r.tau[2] - integrated_time(lnp[:, 100:].T)) <= 2 * (r.window[2] + 1) * 1e-12
    assert abs(r.tau[0] - r.tau[1]) <= 2 * (r.window[0] + 1) * 1e-12           # an affine map of a series has its ACF


@pytest.mark.parametrize("seed", range(len(CASES)))
def test_rhat_and_ess(seed):
    from lumfuncmcmc_amd.sampler import chain_diagnostics_twin, split_rhat
    x = ar1(seed)
    y = shifted(x)
    want, want_shifted = rhat_numpy(x), rhat_numpy(y)
    print("case %d: R-hat %.4f, with the second half shifted %.4f" % (seed, want, want_shifted))
    assert want < 1.05 and want_shifted > 1.5               # conditions on the inputs, by the literal formula alone
    assert abs(split_rhat(x) - want) <= 1e-12 * want
    assert abs(split_rhat(y) - want_shifted) <= 1e-12 * want_shifted
    if x.shape[1] <= 5000:
        r = chain_diagnostics_twin(x[:, :, None])
        assert abs(r.rhat[0] - want) <= 1e-12 * want
        assert abs(r.ess[0] - x.size / r.tau[0]) <= 1e-12 * r.ess[0]
    # odd n: the halves are [0, h) and [n - h, n)
    assert abs(split_rhat(x[:, :-1]) - rhat_numpy(x[:, :-1])) <= 1e-12


def test_argument_errors_without_a_device(lib):
    from lumfuncmcmc_amd import capi
    W, steps, nd = 4, 10, 2
    chain = np.zeros((W, steps, nd))
    tau, ess, rhat = np.zeros(nd), np.zeros(nd), np.zeros(nd)
    win = np.zeros(nd, dtype=np.int64)

    def call(chain_=chain, W_=W, steps_=steps, nd_=nd, t0=0, t1=steps, c=5.0, tau_=tau, win_=win, ess_=ess, rhat_=rhat):
        return lib.lf_chain_diag(0, None if chain_ is None else _p(chain_), None, W_, steps_, nd_, t0, t1, c,
                                 None if tau_ is None else _p(tau_), None if win_ is None else win_.ctypes.data_as(I64P),
                                 None if ess_ is None else _p(ess_), None if rhat_ is None else _p(rhat_), None, 0)

    bad = [dict(chain_=None), dict(tau_=None), dict(win_=None), dict(ess_=None), dict(rhat_=None), dict(W_=0), dict(nd_=0),
           dict(t0=-1), dict(t1=steps + 1), dict(t0=5, t1=5), dict(t0=6, t1=5), dict(c=0.0), dict(c=-1.0), dict(c=float("nan"))]
    for kw in bad:
        assert call(**kw) == capi.LF_ERR_ARG, kw
    # the sampler entries: no sampler (a sampler that exists but has not been started is refused the same way; it takes a GPU
    # to make one - tests/test_gpu_diag.py)
    assert lib.lf_sampler_diag(None, 0, 5.0, 0, _p(tau), win.ctypes.data_as(I64P), _p(ess), _p(rhat)) == capi.LF_ERR_ARG
    assert lib.lf_ptsampler_diag(None, 0, 0, 5.0, 0, _p(tau), win.ctypes.data_as(I64P), _p(ess), _p(rhat)) == capi.LF_ERR_ARG
    t, w = ctypes.c_double(), ctypes.c_int64()
    acf = np.ones(8)
    assert lib.lf_chain_window(None, 8, 5.0, 8, ctypes.byref(t), ctypes.byref(w)) == capi.LF_ERR_ARG
    assert lib.lf_chain_window(_p(acf), 8, 5.0, 8, None, ctypes.byref(w)) == capi.LF_ERR_ARG
    assert lib.lf_chain_window(_p(acf), 8, 5.0, 8, ctypes.byref(t), None) == capi.LF_ERR_ARG
    assert lib.lf_chain_window(_p(acf), 8, 0.0, 8, ctypes.byref(t), ctypes.byref(w)) == capi.LF_ERR_ARG
    assert lib.lf_chain_window(_p(acf), 0, 5.0, 8, ctypes.byref(t), ctypes.byref(w)) == capi.LF_ERR_ARG
    assert lib.lf_chain_window(_p(acf), 8, 5.0, 0, ctypes.byref(t), ctypes.byref(w)) == capi.LF_ERR_ARG
    assert lib.lf_diag_last(None, None) == capi.LF_ERR_ARG
