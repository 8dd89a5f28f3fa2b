"""Chain diagnostics without a GPU: the exports, the window rule in C against integrated_time's own
lines, the NumPy twin of the device's direct sums against the FFT form, the edge conventions, split-R-hat and ESS against
literal NumPy, and every argument error (refused before a device is touched).

Bounds.  Twin ACF against the FFT form: 1e-12 absolute on the normalised curve - direct summation of n terms errs by about
sqrt(n) eps a[0] (2e-14 at n = 2e4), never more than n eps a[0] (2e-12); the FFT form's own error is of order eps log2(n); the
cases have n <= 2e4.  tau with equal windows: 2 (window + 1) 1e-12, the sum of window + 1 such terms, doubled.  Windows are
compared only where the host's own curve keeps every m <= window further than 1e-6 from m = c taus[m] (asserted per case).

The second half asserts everything tests/test_gpu_diag.py presupposes of its exact inputs and references (lf_diaglib.py):
on integer series whose range and half sums are divisible by their lengths the twin equals exact_acf bit for bit; on real
series it stays inside truth_bound of a direct sum in extended precision."""
import ctypes

import numpy as np
import pytest

import lf_diaglib as dl
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


# --------------------------------------------------------------------- what the device tests presuppose (lf_diaglib.py)
def _twin(x_int, **kw):
    from lumfuncmcmc_amd.sampler import chain_diagnostics_twin
    return chain_diagnostics_twin(np.asarray(x_int, dtype=np.float64)[:, :, None], **kw)


def _same(a, b):
    return a == b or (np.isnan(a) and np.isnan(b))


def test_lattice_series_are_exact_inputs():
    for n in dl.EXACT_N + [1, 2, 3]:
        x = dl.lattice(n, 3, n)
        h = n // 2
        assert x.dtype == np.int64 and x.shape == (3, n) and np.all(x.sum(axis=1) % n == 0)
        assert h == 0 or (np.all(x[:, :h].sum(axis=1) % h == 0) and np.all(x[:, n - h:].sum(axis=1) % h == 0))
        assert 30000 < x.min() and x.max() < 50000                   # sums and squares far below 2^53
        assert n < 4 or np.all(dl.exact_lag_sums(x, 1)[:, 0] > 0)    # no walker is constant by accident
        assert not np.array_equal(x, dl.lattice(n + 1, 3, n))        # the seed matters
    # exact_acf on a series small enough to do by hand: y = (-1, 1, 1, -1) and (-3, -1, 1, 3)
    x = np.array([[4, 6, 6, 4], [2, 4, 6, 8]], dtype=np.int64)
    np.testing.assert_array_equal(dl.exact_lag_sums(x, 5), [[4, -1, -2, 1, 0], [20, 5, -6, -9, 0]])
    want = [(1.0 + 1.0) / 2, (-1.0 / 4.0 + 5.0 / 20.0) / 2, (-2.0 / 4.0 + -6.0 / 20.0) / 2, (1.0 / 4.0 + -9.0 / 20.0) / 2, 0.0]
    np.testing.assert_array_equal(dl.exact_acf(x, 5), want)
    with pytest.raises(AssertionError):
        dl.exact_acf(x + np.array([[0, 0, 0, 1], [0, 0, 0, 0]]), 5)  # a sum that n does not divide is refused


def test_twin_equals_exact_acf_at_every_length():
    """Lists (a): bit for bit, whole lag tiles past n, for W = 1 and 3; and R-hat in the device's order of the halves."""
    for n in dl.EXACT_N:
        nl = dl.lags_past(n)
        assert nl % 512 == 0 and nl - 512 > n >= nl - 1024
        for W in (1, 3):
            x = dl.lattice(n, W, n)
            r = _twin(x, nlags=nl)
            want = dl.exact_acf(x, nl)
            np.testing.assert_array_equal(r.acf[0], want)
            assert np.all(want[n:] == 0.0) and want[0] == 1.0
            assert r.ess[0] == W * n / r.tau[0]
            assert abs(r.rhat[0] - rhat_numpy(x.astype(np.float64))) <= 1e-12 * r.rhat[0]


def test_twin_rhat_adds_the_halves_in_the_device_order():
    """lfd::split_rhat restated term by term on exact moments (integer means and sums of squares): the twin has its bits.
    n = 7, W = 3 is where adding all first halves before the second halves gives another last bit."""
    from lumfuncmcmc_amd.sampler import split_rhat
    for n, W in [(7, 3), (4, 1), (257, 2), (513, 3), (1100, 4), (300, 9)]:
        x = dl.lattice(n, W, n)
        h = n // 2
        sm = sv = 0.0
        mom = []
        for w in range(W):
            for half in (x[w, :h], x[w, n - h:]):
                m = int(half.sum()) // h
                mom.append((float(m), float(int(((half - m) ** 2).sum()))))
        for m, q in mom:
            sm += m
            sv += q / float(h - 1)
        gm, Wv = sm / (2 * W), sv / (2 * W)
        bs = 0.0
        for m, q in mom:
            bs += (m - gm) * (m - gm)
        want = float(np.sqrt((float(h - 1) / float(h) * Wv + bs / (2 * W - 1)) / Wv))
        assert split_rhat(x.astype(np.float64)) == want, (n, W)


def test_twin_equals_exact_acf_in_every_group_slot():
    """List (b): the D series of a batch are different series, each equal to its own exact curve."""
    nl = dl.lags_past(dl.GROUP_N)
    x = dl.group_series(max(dl.GROUP_D))
    assert x.shape == (9, dl.GROUP_W, dl.GROUP_N)
    curves = [dl.exact_acf(x[d], nl) for d in range(9)]
    for d in range(9):
        np.testing.assert_array_equal(_twin(x[d], nlags=nl).acf[0], curves[d])
        for e in range(d):
            assert not np.array_equal(curves[d][:dl.GROUP_N], curves[e][:dl.GROUP_N])


def test_drift_series_need_later_passes(lib):
    """List (c): under c = 50 the window lies past the first 512 lags, far from a rounding error, and the lags diag_run has
    computed when it decides are 1024, 1024, 1024 and 1536; the twin has the FFT form's window and the exact curve."""
    windows = {}
    for n in dl.DRIFT_N:
        x = dl.drift(n, 4, n)
        assert np.all(np.abs(x - 8 * np.arange(n)) <= 3 + n)         # 8 t + noise; the few adjusted elements moved by < n
        tau, win, margin = fft_window(fft_acf(x.astype(np.float64)), c=50.0)
        print("drift n %d: window %d tau %.4f margin %.3g -> %d lags" % (n, win, tau, margin, dl.passes(win, n)))
        windows[n] = win
        assert win > 512 and margin > 1e-6 and margin > 1.0
        assert dl.passes(win, n) == dl.DRIFT_LAGS[n]
        r = _twin(x, c=50.0)
        assert r.window[0] == win
        full = _twin(x, c=50.0, nlags=1536)
        want = dl.exact_acf(x, 1536)
        np.testing.assert_array_equal(full.acf[0], want)
        assert (full.tau[0], full.window[0]) == (r.tau[0], r.window[0])
        rc, ctau, cwin = c_window(lib, want[:min(n, 1536)], 50.0, n)  # the C rule on the exact curve: what the device must give
        assert rc == 0 and cwin == win and abs(ctau - r.tau[0]) <= 1e-15 * abs(ctau)
    assert windows == {600: 550, 700: 642, 1100: 1009, 1200: 1101}
    assert dl.passes(511, 600) == 512 and dl.passes(512, 600) == 1024 and dl.passes(1023, 1100) == 1024
    assert dl.passes(1024, 1100) == 1536 and dl.passes(1024, 3000) == 2048


def test_slice_arithmetic_and_pattern_curves():
    """List (d): W D 1024 doubles exceed 64 MiB, so a pass of 1024 lags takes two slices of 512; and the expected curve of
    the pattern chain equals exact_acf of the chain itself (shown on its first 23 walkers)."""
    W, D, n, nlags = dl.SLICE_SHAPE
    assert W * D * nlags * 8 > dl.SLICE_BYTES and dl.slices(W, D, nlags) == (512, 2)
    assert dl.slices(32, 3, 2048)[1] == 1 and dl.slices(W, D - 1, nlags) == (1024, 1)
    assert nlags == -(-n // 512) * 512 and n > 512                  # both slices hold lags below n
    pat = dl.slice_patterns()
    live, ratio = dl.exact_ratios(pat, nlags)
    assert list(live) == [True, True, True, True, False] and np.all(ratio[4] == 0.0)
    for d in range(D):
        idx = [dl.slice_pattern_of(w, d) for w in range(23)]
        np.testing.assert_array_equal(dl.slice_expected(pat, d, 23, nlags), dl.exact_acf(pat[idx], nlags))
        np.testing.assert_array_equal(_twin(pat[idx], nlags=nlags).acf[0], dl.exact_acf(pat[idx], nlags))
    full = dl.slice_expected(pat, 0, W, nlags)
    assert full[0] == sum(1.0 for w in range(W) if w % 5 != 4) / W and np.all(full[n:] == 0.0) and np.any(full[512:n] != 0.0)
    # one constant walker among 8: acf[0] is 7/8 exactly
    x = dl.lattice(300, 8, 400)
    x[3] = 40000
    want = dl.exact_acf(x, 512)
    assert want[0] == 7.0 / 8.0
    np.testing.assert_array_equal(_twin(x, nlags=512).acf[0], want)


def test_constant_series_and_short_series_on_the_twin():
    """List (f): a constant that is not representable centres to exactly 0 (the two-pass mean of a constant is exact), so
    a[0] = 0, the ACF is 0, tau 1.0 and window 0 - where the host's integrated_time, whose one-pass mean may miss the
    constant by an ulp, can return tau = n; and n < 4."""
    from lumfuncmcmc_amd.sampler import chain_diagnostics_twin, integrated_time
    host = {}
    for v in dl.CONSTANTS:
        assert float(np.float32(v)) != v                             # not a short binary fraction
        for n in dl.CONSTANT_N:
            x = np.full((3, n, 1), v)
            r = chain_diagnostics_twin(x, nlags=dl.lags_past(n))
            assert np.all(r.acf == 0.0) and r.tau[0] == 1.0 and r.window[0] == 0 and r.ess[0] == 3 * n, (v, n)
            host[(v, n)] = integrated_time(x[:, :, 0].T)
    print("host integrated_time on constants:", host)
    # either its mean hits the constant (a[0] = 0, tau 1.0) or misses it by an ulp: then y is a constant, acf[k] = (n - k) / n
    # and tau comes out as n
    assert all(t == 1.0 or abs(t - n) <= 1e-12 * n for (v, n), t in host.items())
    for n in (1, 2, 3):
        r = _twin(dl.lattice(n, 3, n), nlags=512)
        assert r.tau[0] == 1.0 and r.window[0] == 0 and np.isnan(r.rhat[0]) and np.all(r.acf == 0.0) and r.ess[0] == 3 * n
    # the widest ensemble the device takes, n = 4: the exact reference handles it
    x = dl.lattice(4, 65535, 4)
    want = dl.exact_acf(x, 4)
    assert want[0] == 1.0 and np.all(np.abs(want) <= 1.0)


def test_truth_and_its_bound_hold_the_twin():
    """List (g): the twin against direct sums in extended precision stays inside 2 ((n + 16) 2^-53 + S); so does the FFT
    form.  The figures are printed (DESIGN.md section 3.12 quotes them)."""
    from lumfuncmcmc_amd.sampler import chain_diagnostics_twin
    assert np.finfo(np.longdouble).eps <= 1.1e-19 or dl._extended() is None
    for name, x in dl.real_cases().items():
        W, n = x.shape
        truth, S = dl.truth_acf(x, n)
        bound = dl.truth_bound(n, S)
        assert bound <= 1e-12 and truth[0] == 1.0
        twin = np.max(np.abs(chain_diagnostics_twin(x[:, :, None], nlags=n).acf[0] - truth))
        fft = np.max(np.abs(fft_acf(x) - truth))
        print("%-22s W %2d n %4d S %.3g bound %.3g twin err / bound %.4f FFT err / bound %.4f" % (name, W, n, S, bound, twin / bound, fft / bound))
        assert twin <= bound and fft <= bound
    assert {x.shape[1] for x in dl.real_cases().values()} == {300, 1100, 1025}


def test_truth_in_mpmath_equals_truth_in_long_double(monkeypatch):
    """The fall-back of truth_acf (40 digits) on a short series, against the extended-precision form where there is one."""
    if dl._extended() is None:
        pytest.skip("no extended precision to compare with")
    x = ar1(0)[:2, :24]
    a, Sa = dl.truth_acf(x, 30)
    monkeypatch.setattr(dl, "_extended", lambda: None)
    b, Sb = dl.truth_acf(x, 30)
    assert np.max(np.abs(a - b)) <= 4e-16 and abs(Sa - Sb) <= 1e-18 + 1e-3 * Sb and np.all(b[24:] == 0.0)    # long double resolves S to about eps
