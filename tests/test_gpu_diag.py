"""Chain diagnostics on the GPU (csrc/lf_diag.h) against the code as it stood: the FFT form of
sampler.integrated_time and NumPy.  Bounds as in tests/test_diag_cpu.py: ACF 1e-12 absolute, tau 2 (window + 1) 1e-12 with
equal windows (compared where the host's margin is above 1e-6), R-hat and ESS 1e-12 relative."""
import numpy as np
import pytest

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
