"""fit_model_converged and fit_model_pt on the flux-error-convolved likelihood (the `likelihood` keyword; DESIGN.md section
3.20) on a noisy mock of about 3000 sources with 0.09 dex of noise at fixed completeness: the convergence-controlled fit sets
what it sets for the plain likelihood and its chain replays on the host, the Eddington shift has its sign (the convolved
chain's mean L* lies below the plain chain's on the same object), start="map" runs, and the tempered fit's evidence agrees with
the Laplace evidence of fit_model_map(likelihood="convolved") under the acceptance rule of tests/test_gpu_pt.py."""
import numpy as np
import pytest

import lf_deconvlib as L
from lf_replaylib import host_replay

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mock():
    o, theta, _ = L.noisy_mock(3000, 0.09, 11, deconvolve=True, deconvolve_tile=True, nsteps=1000)
    yield o, theta
    o.close()


def test_fit_model_converged_on_the_convolved_likelihood(mock):
    o, theta = mock
    np.random.seed(7)
    tau = o.fit_model_converged(max_steps=600, check_every=200, likelihood="convolved")
    steps = o.chain.shape[1]
    assert o.sampler_likelihood == "convolved" and o.sampler.likelihood == "convolved"
    assert o.chain.shape == (32, steps, 3) and steps in (400, 600) and o.samples.shape[1] == 4
    assert [s for s, _ in o.tau_history] == list(range(200, steps + 1, 200)) and np.array_equal(tau, o.tau_history[-1][1])
    assert np.all(np.isfinite(o.samples))
    # (start, seed, steps) reproduce the chain, over the convolved likelihood with the object's own context options
    ctx = o.context()
    chain, lnp, nacc = host_replay(ctx, o.start_pos, steps, o.sampler_seed, lnprob=ctx.lnprob_err_batch)
    np.testing.assert_array_equal(o.chain, chain)
    np.testing.assert_array_equal(o.sampler.lnprobability, lnp)
    np.testing.assert_array_equal(o.sampler.naccepted, nacc)
    conv_mean = o.samples[:, 0].mean()
    np.random.seed(7)
    o.fit_model_converged(max_steps=600, check_every=200, likelihood="plain")
    assert o.sampler_likelihood == "plain"
    plain_mean = o.samples[:, 0].mean()
    print("chain mean of L*: convolved %.4f, plain %.4f, truth %.4f" % (conv_mean, plain_mean, theta[0]))
    assert conv_mean < plain_mean


def test_fit_model_converged_from_the_map(mock):
    o, _ = mock
    np.random.seed(8)
    o.map_theta = None
    o.fit_model_converged(max_steps=200, check_every=100, start="map", likelihood="convolved")
    assert o.map_info["likelihood"] == "convolved" and o.map_info["converged"]
    assert o.chain.shape == (32, 200, 3) and np.all(np.isfinite(o.sampler.lnprobability))
    # the walkers started around the convolved maximum: the first step's lnprob is already close to it
    assert np.median(o.sampler.lnprobability[:, 0]) > o.map_lnprob - 20.0


def test_fit_model_pt_evidence_against_laplace(mock):
    o, _ = mock
    np.random.seed(2026)
    info = o.fit_model_map(nstarts=8, seed=3, likelihood="convolved")
    assert info["converged"] and np.isfinite(info["lnZ_laplace"]), info["lnZ_reason"]
    lnZ, dlnZ = o.fit_model_pt(likelihood="convolved")
    assert (o.lnZ, o.dlnZ) == (lnZ, dlnZ) and o.pt_sampler.likelihood == "convolved"
    print("lnZ %.4f +/- %.4f, Laplace %.4f, %d temperatures, Tmax %.3g" % (
        lnZ, dlnZ, info["lnZ_laplace"], o.pt_sampler.ntemps, 1.0 / o.pt_sampler.betas[-1]))
    assert abs(lnZ - info["lnZ_laplace"]) <= max(0.3, 3.0 * dlnZ), (lnZ, dlnZ, info["lnZ_laplace"])
    assert o.samples.shape[1] == 4 and np.all(np.isfinite(o.samples))
    # the beta = 1 chain's lnlike is the convolved likelihood of its positions
    ctx = o.context()
    last = o.pt_sampler.chain[0][:, -1]
    np.testing.assert_array_equal(ctx.lnprob_err_batch(last), o.pt_sampler.lnlikelihood[0][:, -1])
