"""Chain diagnostics on the GPU (csrc/lf_diag.h) against the code as it stood: the FFT form of
sampler.integrated_time and NumPy.  Bounds as in tests/test_diag_cpu.py: ACF 1e-12 absolute, tau 2 (window + 1) 1e-12 with
equal windows (compared where the host's margin is above 1e-6), R-hat and ESS 1e-12 relative."""
import functools

import numpy as np
import pytest

import lf_diaglib as dl
from lf_diaglib import CASES, ar1, fft_acf, fft_window, rhat_numpy
from lf_testlib import make_inputs, synth

pytestmark = pytest.mark.gpu


def check_against_fft(chain, lnprob=None, t0=0, nlags=2048, what=""):
    from lumfuncmcmc_amd.sampler import chain_diagnostics
    W, steps, nd = chain.shape
    n = steps - t0
    r = chain_diagnostics(chain, lnprob=lnprob, t0=t0, nlags=nlags)
    series = [chain[:, t0:, d] for d in range(nd)] + ([lnprob[:, t0:]] if lnprob is not None else [])
    assert r.tau.shape == (len(series),)
    for d, x in enumerate(series):
        acf = fft_acf(x)
        tau, win, margin = fft_window(acf)
        k = min(n, nlags)
        err = np.max(np.abs(r.acf[d, :k] - acf[:k]))
        print("%s series %d: n %d ACF err %.3g window %d / %d margin %.3g tau %.6f / %.6f rhat %.5f ess %.1f"
              % (what, d, n, err, r.window[d], win, margin, r.tau[d], tau, r.rhat[d], r.ess[d]))
        assert err <= 1e-12
        assert np.all(r.acf[d, k:] == 0.0)
        if margin > 1e-6:
            assert r.window[d] == win
            want = tau if np.isfinite(tau) and tau > 0 else 1.0
            assert abs(r.tau[d] - want) <= 2 * (win + 1) * 1e-12
        want = rhat_numpy(x)
        assert abs(r.rhat[d] - want) <= 1e-12 * want
        assert abs(r.ess[d] - W * n / r.tau[d]) <= 1e-12 * r.ess[d]
    return r


@pytest.mark.parametrize("seed", range(len(CASES)))
def test_chain_diag_against_the_fft_form_seeded(seed):
    x = ar1(seed)
    tau, win, margin = fft_window(fft_acf(x))
    assert margin > 1e-6
    other = ar1((seed + 1) % 3)[:x.shape[0], :x.shape[1]] if seed != 1 else None
    if other is not None and other.shape == x.shape:
        chain = np.stack([x, other, 3.0 - x], axis=2)
    else:
        chain = x[:, :, None]
    check_against_fft(chain, what="AR(1) case %d" % seed)


def _real_chain(variant, steps, W=32, cap=None, seed=5):
    from lumfuncmcmc_amd.capi import LFContext
    from lumfuncmcmc_amd.sampler import DeviceEnsembleSampler
    ctx = LFContext(make_inputs(variant, 1000, seed=71))
    pos = synth.walkers(variant, W, seed=72)
    ds = DeviceEnsembleSampler(ctx, W, seed=seed, capacity=cap or steps)
    ds.run_mcmc(pos, steps)
    return ctx, ds, pos


@pytest.mark.parametrize("variant,steps", [("free", 2000), ("fixcomp", 500), ("zevol", 500)])
def test_chain_diag_against_the_fft_form_real_chain(variant, steps):
    ctx, ds, _ = _real_chain(variant, steps)
    check_against_fft(ds.chain, lnprob=ds.lnprobability, what=variant)
    check_against_fft(ds.chain, t0=steps // 4, what=variant + " tail")
    ds.close(); ctx.close()


def test_determinism_and_lag_independence():
    from lumfuncmcmc_amd.sampler import chain_diagnostics
    x = ar1(0)
    chain = np.stack([x, x * x], axis=2)
    a = chain_diagnostics(chain, nlags=2048)
    b = chain_diagnostics(chain, nlags=2048)
    for k in ("tau", "window", "ess", "rhat", "acf"):
        np.testing.assert_array_equal(getattr(a, k), getattr(b, k))
    small = chain_diagnostics(chain, nlags=256)
    np.testing.assert_array_equal(small.acf, a.acf[:, :256])
    np.testing.assert_array_equal(small.tau, a.tau)
    # whatever else is in the batch: the first series alone, and next to a lnprob column
    alone = chain_diagnostics(chain[:, :, :1], lnprob=chain[:, :, 1], nlags=2048)
    np.testing.assert_array_equal(alone.acf[0], a.acf[0])
    np.testing.assert_array_equal(alone.acf[1], a.acf[1])


def test_sampler_diag_equals_chain_diag_and_moves_nothing():
    from lumfuncmcmc_amd.sampler import DeviceEnsembleSampler, chain_diagnostics, integrated_time
    ctx, ds, pos = _real_chain("free", 600, cap=1000)
    with pytest.raises(Exception):
        DeviceEnsembleSampler(ctx, 32, seed=1, capacity=10).diagnostics()             # not started
    for t0 in (0, 150):
        on = ds.diagnostics(t0=t0, with_lnprob=True)
        off = chain_diagnostics(ds.chain, lnprob=ds.lnprobability, t0=t0)
        for k in ("tau", "window", "ess", "rhat"):
            np.testing.assert_array_equal(getattr(on, k), getattr(off, k))
        np.testing.assert_array_equal(ds.diagnostics(t0=t0).tau, on.tau[:-1])
    with pytest.raises(Exception):
        ds.diagnostics(t0=600)
    # get_autocorr_time: unchanged without the keyword, within the tolerance with it
    old = np.array([integrated_time(ds.chain[:, :, d].T) for d in range(ds.ndim)])
    np.testing.assert_array_equal(ds.get_autocorr_time(), old)
    np.testing.assert_array_equal(ds.acor, old)
    new = ds.get_autocorr_time(device=True)
    for d in range(ds.ndim):
        tau, win, margin = fft_window(fft_acf(ds.chain[:, :, d]))
        if margin > 1e-6:
            assert abs(new[d] - old[d]) <= 2 * (win + 1) * 1e-12
    # a diagnostics() call in the middle of a run changes nothing of the chain
    ds.run_mcmc(None, 400)
    plain = DeviceEnsembleSampler(ctx, 32, seed=5, capacity=1000)
    plain.run_mcmc(pos, 1000)
    np.testing.assert_array_equal(ds.chain, plain.chain)
    np.testing.assert_array_equal(ds.lnprobability, plain.lnprobability)
    np.testing.assert_array_equal(ds.naccepted, plain.naccepted)
    plain.close(); ds.close(); ctx.close()


def test_ptsampler_diag_equals_chain_diag():
    from lumfuncmcmc_amd.capi import LFContext
    from lumfuncmcmc_amd.sampler import DevicePTSampler, chain_diagnostics
    ctx = LFContext(make_inputs("fixcomp", 1000, seed=73))
    T, W, steps = 3, 32, 300
    pos = synth.walkers("fixcomp", T * W, seed=74).reshape(T, W, ctx.ndim)
    pt = DevicePTSampler(ctx, T, W, betas=[1.0, 0.5, 0.2], seed=9, capacity=450)
    pt.run_mcmc(pos, steps)
    for t in (0, T - 1):
        for t0 in (0, 70):
            on = pt.diagnostics(t, t0=t0, with_lnlike=True)
            off = chain_diagnostics(pt.chain[t], lnprob=pt.lnlikelihood[t], t0=t0)
            for k in ("tau", "window", "ess", "rhat"):
                np.testing.assert_array_equal(getattr(on, k), getattr(off, k))
    old = pt.get_autocorr_time()
    np.testing.assert_array_equal(old, pt.acor)
    assert pt.get_autocorr_time(device=True).shape == old.shape
    with pytest.raises(Exception):
        pt.diagnostics(T)
    pt.close(); ctx.close()


# ------------------------------------------------------------------------------------ exact sums at every tile edge
# Integer series (lf_diaglib.lattice, drift) leave the device nothing to round but a_w[k] / a_w[0], the walker sum and the
# division by W, so its curve must equal exact_acf bit for bit; tests/test_diag_cpu.py asserts what is presupposed here of
# the inputs, of exact_acf and of the twin.

def _raw(chain, lnprob=None, t0=0, t1=None, c=5.0, nlags=0):
    """lf_chain_diag itself over [t0, t1): (rc, tau, window, ess, rhat, acf, lags reported by lf_diag_last)."""
    import ctypes
    from lumfuncmcmc_amd import capi
    lib = capi.load()
    chain = np.ascontiguousarray(chain, dtype=np.float64)
    lnprob = None if lnprob is None else np.ascontiguousarray(lnprob, dtype=np.float64)
    W, steps, ndim = chain.shape
    D = ndim + (lnprob is not None)
    tau, ess, rhat = np.full(D, -7.0), np.full(D, -7.0), np.full(D, -7.0)
    window = np.full(D, -7, dtype=np.int64)
    acf = np.full((D, nlags), -7.0) if nlags else None
    rc = lib.lf_chain_diag(0, capi._ptr(chain), capi._ptr(lnprob), W, steps, ndim, t0, steps if t1 is None else t1, float(c),
                           capi._ptr(tau), window.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), capi._ptr(ess), capi._ptr(rhat),
                           capi._ptr(acf), nlags)
    ms, lags = ctypes.c_double(), ctypes.c_int64()
    if rc == capi.LF_OK:
        assert lib.lf_diag_last(ctypes.byref(ms), ctypes.byref(lags)) == capi.LF_OK
    return rc, tau, window, ess, rhat, acf, lags.value


def _c_window(acf, c, n):
    import ctypes
    from lumfuncmcmc_amd import capi
    acf = np.ascontiguousarray(acf, dtype=np.float64)
    tau, win = ctypes.c_double(), ctypes.c_int64()
    assert capi.load().lf_chain_window(capi._ptr(acf), len(acf), float(c), n, ctypes.byref(tau), ctypes.byref(win)) == 0
    return tau.value, win.value


def _as_chain(series):
    """(D, W, n) integers -> the (W, n, D) chain of doubles."""
    return np.ascontiguousarray(np.transpose(np.asarray(series), (1, 2, 0)), dtype=np.float64)


def _equals_twin(r, chain, lnprob=None, c=5.0):
    """window, ess and R-hat with the twin's bits, tau within 1e-15 relative (the figure of the C window rule)."""
    from lumfuncmcmc_amd.sampler import chain_diagnostics_twin
    t = chain_diagnostics_twin(chain, lnprob=lnprob, c=c)
    np.testing.assert_array_equal(r.window, t.window)
    np.testing.assert_array_equal(r.ess, t.ess)
    np.testing.assert_array_equal(r.rhat, t.rhat)
    assert np.all(np.abs(r.tau - t.tau) <= 1e-15 * np.abs(t.tau))


@pytest.mark.parametrize("n", dl.EXACT_N)
def test_exact_acf_at_every_length(n):
    """(a) n at and beside 4, 8, 64, 256, 512, 768 and 1024, W = 3, whole lag tiles asked for past n."""
    from lumfuncmcmc_amd.sampler import chain_diagnostics
    x = dl.lattice(n, 3, n)
    nl = dl.lags_past(n)
    chain = _as_chain(x[None])
    r = chain_diagnostics(chain, nlags=nl)
    np.testing.assert_array_equal(r.acf[0], dl.exact_acf(x, nl))
    assert np.all(r.acf[0, n:] == 0.0)
    _equals_twin(r, chain)


@functools.lru_cache(maxsize=None)
def _group_refs():
    x = dl.group_series(max(dl.GROUP_D))
    return x, [dl.exact_acf(x[d], dl.lags_past(dl.GROUP_N)) for d in range(len(x))]


@pytest.mark.parametrize("D,with_lnprob", [(D, l) for D in dl.GROUP_D for l in (False, True) if D - l >= 1])
def test_exact_acf_in_every_group_slot(D, with_lnprob):
    """(b) last groups of 1, 2, 3 and 4 live series, as parameters alone and with lnprob as the last series; every series
    is a different one, so a series in the wrong slot shows."""
    from lumfuncmcmc_amd.sampler import chain_diagnostics
    x, curves = _group_refs()
    chain = _as_chain(x[:D - with_lnprob])
    lnprob = x[D - 1].astype(np.float64) if with_lnprob else None
    r = chain_diagnostics(chain, lnprob=lnprob, nlags=dl.lags_past(dl.GROUP_N))
    assert r.acf.shape[0] == D
    for d in range(D):
        np.testing.assert_array_equal(r.acf[d], curves[d], err_msg="series %d of %d" % (d, D))
    _equals_twin(r, chain, lnprob)


@pytest.mark.parametrize("n", dl.DRIFT_N)
def test_later_passes_have_the_bits_of_one_pass(n):
    """(c) passes that start at k_lo = 512 and 1024 (c = 50 on a drift: the window lies past 512, for n = 1200 past 1024).
    lf_chain_diag hands out no lag a later pass computed (a call that asks for more than 512 lags computes them in its
    first pass), so the later passes are held by what they feed: tau = 2 sum_{k <= window} acf[k] - 1 of the call in passes
    has the bits of the C window rule on the exact curve, and of the calls that compute the same lags in one pass or split
    at 1024."""
    from lumfuncmcmc_amd.sampler import chain_diagnostics_twin
    x = dl.drift(n, 4, n)
    chain = _as_chain(x[None])
    want = dl.exact_acf(x, 1536)
    mmax = -(-n // 512) * 512
    rc, tau, window, ess, rhat, _, lags = _raw(chain, c=50.0)
    print("drift n %d: window %d tau %.6f, %d lags in passes" % (n, window[0], tau[0], lags))
    assert rc == 0 and lags == dl.DRIFT_LAGS[n]
    twin = chain_diagnostics_twin(chain, c=50.0)
    assert window[0] == twin.window[0] > 512
    assert (tau[0], window[0]) == _c_window(want[:n], 50.0, n)
    assert abs(tau[0] - twin.tau[0]) <= 1e-15 * twin.tau[0] and ess[0] == 4 * n / tau[0] and rhat[0] == twin.rhat[0]
    for nlags in (1536, 1024):
        rc, tau1, window1, ess1, rhat1, acf, lags = _raw(chain, c=50.0, nlags=nlags)
        assert rc == 0 and lags == max(min(nlags, mmax), dl.DRIFT_LAGS[n])
        np.testing.assert_array_equal(acf[0], want[:nlags])
        assert (tau1[0], window1[0], ess1[0], rhat1[0]) == (tau[0], window[0], ess[0], rhat[0])


def test_second_slice_of_a_pass():
    """(d) W D = 8200 series make a pass of 1024 lags two slices of 512: the second slice's lag offset and its use of the
    first slice's a[0].  Five patterns, one of them constant (a_w[0] = 0), walker w of series d taking (w + 2 d) % 5."""
    from lumfuncmcmc_amd.sampler import chain_diagnostics
    W, D, n, nlags = dl.SLICE_SHAPE
    assert dl.slices(W, D, nlags) == (512, 2)
    pat = dl.slice_patterns()
    idx = np.array([[dl.slice_pattern_of(w, d) for d in range(D)] for w in range(W)])
    chain = np.ascontiguousarray(np.transpose(pat[idx], (0, 2, 1)), dtype=np.float64)
    assert chain.shape == (W, n, D)
    r = chain_diagnostics(chain, nlags=nlags)
    for d in range(D):
        np.testing.assert_array_equal(r.acf[d], dl.slice_expected(pat, d, W, nlags), err_msg="series %d" % d)
    assert np.all(r.acf[:, n:] == 0.0) and np.all(np.isfinite(r.tau)) and np.all(np.isfinite(r.rhat))


def test_one_constant_walker_among_eight():
    from lumfuncmcmc_amd.sampler import chain_diagnostics
    x = dl.lattice(300, 8, 400)
    x[3] = 40000
    chain = _as_chain(x[None])
    r = chain_diagnostics(chain, nlags=512)
    assert r.acf[0, 0] == 7.0 / 8.0
    np.testing.assert_array_equal(r.acf[0], dl.exact_acf(x, 512))
    _equals_twin(r, chain)


def test_range_inside_the_chain():
    """(e) 0 < t0 < t1 < steps through lf_chain_diag itself (the Python wrapper always passes t1 = steps): everything outside
    [t0, t1) is NaN, and every output has the bits of the sliced chain's."""
    steps, t0, n = 700, 37, 513
    x = np.stack([dl.lattice(300 + d, 3, n) for d in range(3)])
    inner, lnp = _as_chain(x[:2]), x[2].astype(np.float64)
    chain, lnprob = np.full((3, steps, 2), np.nan), np.full((3, steps), np.nan)
    chain[:, t0:t0 + n], lnprob[:, t0:t0 + n] = inner, lnp
    got = _raw(chain, lnprob, t0=t0, t1=t0 + n, nlags=1536)
    want = _raw(inner, lnp, nlags=1536)
    assert got[0] == 0 and want[0] == 0 and got[6] == want[6] == 1024
    for g, w in zip(got[1:6], want[1:6]):
        assert not np.any(np.isnan(g))
        np.testing.assert_array_equal(g, w)
    for d in range(3):
        np.testing.assert_array_equal(got[5][d], dl.exact_acf(x[d], 1536))


@pytest.mark.parametrize("n", [1, 2, 3])
def test_fewer_than_four_steps(n):
    """(f) tau 1.0, window 0, R-hat NaN, ACF 0.0, no error."""
    rc, tau, window, ess, rhat, acf, lags = _raw(_as_chain(dl.lattice(n, 3, n)[None]), nlags=512)
    assert rc == 0 and lags == 0
    assert tau[0] == 1.0 and window[0] == 0 and ess[0] == 3.0 * n and np.isnan(rhat[0]) and np.all(acf == 0.0)


def test_constant_series_centre_to_zero():
    """(f) a constant that is not representable: the two-pass mean is the constant itself, so a[0] = 0 exactly."""
    from lumfuncmcmc_amd.sampler import chain_diagnostics
    for v in dl.CONSTANTS:
        for n in dl.CONSTANT_N:
            r = chain_diagnostics(np.full((3, n, 1), v), nlags=dl.lags_past(n))
            assert np.all(r.acf == 0.0) and r.tau[0] == 1.0 and r.window[0] == 0 and r.ess[0] == 3.0 * n, (v, n)


def test_widest_ensemble():
    """(f) W = 65535 is the grid's limit and is right; 65536 is refused."""
    from lumfuncmcmc_amd import capi
    x = dl.lattice(4, 65535, 4)
    rc, tau, window, ess, rhat, acf, lags = _raw(_as_chain(x[None]), nlags=4)
    want = dl.exact_acf(x, 4)
    assert rc == 0 and lags == 512
    np.testing.assert_array_equal(acf[0], want)
    assert (tau[0], window[0]) == _c_window(want, 5.0, 4) and ess[0] == 65535 * 4 / tau[0] and np.isfinite(rhat[0])
    assert _raw(np.zeros((65536, 4, 1)), nlags=4)[0] == capi.LF_ERR_ARG


@functools.lru_cache(maxsize=None)
def _truths():
    return {name: (x,) + dl.truth_acf(x, x.shape[1]) for name, x in dl.real_cases().items()}


@pytest.mark.parametrize("name", sorted(dl.real_cases()))
def test_real_series_against_extended_precision(name):
    """(g) direct sums in extended precision, bound 2 ((n + 16) 2^-53 + S) (lf_diaglib.truth_bound; the twin is held to it in
    tests/test_diag_cpu.py).  Measured on an MI355X, err / bound: see DESIGN.md section 3.12."""
    from lumfuncmcmc_amd.sampler import chain_diagnostics
    x, truth, S = _truths()[name]
    W, n = x.shape
    bound = dl.truth_bound(n, S)
    r = chain_diagnostics(x[:, :, None], nlags=n)
    err = np.max(np.abs(r.acf[0] - truth))
    print("%-22s W %2d n %4d S %.3g bound %.3g device err / bound %.4f" % (name, W, n, S, bound, err / bound))
    assert bound <= 1e-12 and err <= bound


def _fixcomp_model(nsteps=1000):
    from lumfuncmcmc_amd.model import LumFuncMCMC
    cat = synth.catalogue(1000, seed=81)
    fi = cat["field_ind"]
    return LumFuncMCMC(synth.split_fields(cat["z"], fi), lum=synth.split_fields(cat["lum"], fi),
                       lum_e=synth.split_fields(cat["lum_e"], fi), Flim=list(synth.FLIM), alpha=synth.ALPHA_C,
                       Omega_0=list(synth.OMEGA_0), sch_al=synth.SCH_AL, sch_al_lims=synth.SCH_AL_LIMS, Lstar=synth.LSTAR,
                       Lstar_lims=synth.LSTAR_LIMS, phistar=synth.PHISTAR, phistar_lims=synth.PHISTAR_LIMS, Lc=synth.LC,
                       Lh=synth.LH, nwalkers=32, nsteps=nsteps, min_comp_frac=0.0, field_ind=fi, fix_comp=True)


def test_fit_model_converged(caplog):
    """Fixed completeness, 1000 sources, 32 walkers, seeded, check_every = 200, max_steps = 20000; ntau = 50 and rtol = 0.01
    are emcee's numbers and stay."""
    import logging
    from lumfuncmcmc_amd.sampler import DeviceEnsembleSampler
    m = _fixcomp_model()
    np.random.seed(20261)
    tau = m.fit_model_converged(max_steps=20000, check_every=200)
    hist = m.tau_history
    for steps, t in hist:
        print("steps %6d  tau %s" % (steps, np.array2string(t, precision=2)))
    steps = hist[-1][0]
    ndim = m.start_pos.shape[1]
    assert m.converged
    assert steps > 50 * np.max(tau) and np.array_equal(tau, hist[-1][1])
    assert np.max(np.abs(hist[-1][1] - hist[-2][1]) / hist[-1][1]) < 0.01
    assert m.samples.shape[1] == ndim + 1 and m.chain.shape == (32, steps, ndim)
    burn = min(int(3 * np.max(tau)), steps // 2)
    assert m.samples.shape[0] == 32 * (steps - burn)
    np.testing.assert_array_equal(m.samples[:, :-1].reshape(32, steps - burn, ndim), m.chain[:, burn:])
    plain = DeviceEnsembleSampler(m.context(), 32, seed=m.sampler_seed, capacity=steps)
    plain.run_mcmc(m.start_pos, steps)
    np.testing.assert_array_equal(plain.chain, m.chain)
    np.testing.assert_array_equal(plain.lnprobability, m.sampler.lnprobability)
    plain.close()
    # too few steps allowed: it says so and goes on with the chain there is
    np.random.seed(20261)
    with caplog.at_level(logging.WARNING, logger=m.log.name):
        caplog.clear()
        m.fit_model_converged(max_steps=300, check_every=200)
    assert not m.converged and m.chain.shape[1] == 300 and [s for s, _ in m.tau_history] == [200, 300]
    assert any("not converged" in r.getMessage() for r in caplog.records)
    m.close()
