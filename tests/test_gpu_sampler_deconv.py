"""The device samplers on the flux-error-convolved likelihood (lf_sampler_set_likelihood, lf_ptsampler_set_likelihood;
DESIGN.md section 3.20): the chain replays bit for bit on the host over ctx.lnprob_err_batch with the same "deconv_tile" on
the context - start given or left to the sampler, run or hand-sharded halves, one temperature or three - it is the plain
chain when every sigma is 0, the refusals leave the context usable, and the diagnostics see the chain where it is."""
import ctypes

import numpy as np
import pytest

from lf_replaylib import host_replay
from lf_testlib import make_inputs, synth

pytestmark = pytest.mark.gpu
N, STEPS, K = 300, 40, 4
CASES = [("fixcomp", 0), ("fixcomp", 1), ("zevol", 1), ("free", 0)]
NF = {"fixcomp": 5, "zevol": 5, "free": 2}              # (free: ndim = 3 + 2 + 1, so that 16 walkers are enough)


def seeded_sigma(n, seed):
    rng = np.random.default_rng(seed)
    sg = rng.uniform(0.0, 0.09, n)
    sg[rng.permutation(n)[:max(1, n // 10)]] = 0.0
    return sg


def context(variant, tile, sigma=None, seed=31):
    from lumfuncmcmc_amd.capi import LFContext
    ctx = LFContext(make_inputs(variant, N, seed=seed, S=23, nf=NF[variant]))
    ctx.set_lum_err(seeded_sigma(N, seed + 1) if sigma is None else sigma, K, unchecked=True)
    ctx.set_option("deconv_tile", tile)
    return ctx


def start(variant, W, seed=33):
    return synth.walkers(variant, W, seed=seed, nf=NF[variant])


@pytest.mark.parametrize("W", [16, 18])
@pytest.mark.parametrize("variant,tile", CASES)
def test_convolved_chain_replays_on_the_host(variant, tile, W):
    """halves of 8 and 9 rows; the start's lnprob given, and left to the sampler; a run in two pieces"""
    from lumfuncmcmc_amd.sampler import DeviceEnsembleSampler
    ctx = context(variant, tile)
    try:
        pos, seed = start(variant, W), 0xDEC0 + W
        chain, lnp, nacc = host_replay(ctx, pos, STEPS, seed, lnprob=ctx.lnprob_err_batch)
        assert 0 < nacc.sum() < W * STEPS
        plain = host_replay(ctx, pos, STEPS, seed)
        assert not np.array_equal(plain[1], lnp)
        for lnprob0 in (ctx.lnprob_err_batch(pos), None):
            ds = DeviceEnsembleSampler(ctx, W, seed=seed, capacity=STEPS, likelihood="convolved")
            ds.enqueue(pos, 15, lnprob0=lnprob0)
            ds.enqueue(None, STEPS - 15)
            ds.sync()
            np.testing.assert_array_equal(ds.chain, chain)
            np.testing.assert_array_equal(ds.lnprobability, lnp)
            np.testing.assert_array_equal(ds.naccepted, nacc)
            ds.close()
    finally:
        ctx.close()


@pytest.mark.parametrize("variant,tile", [("fixcomp", 1), ("zevol", 1), ("free", 0)])
def test_all_sigma_zero_is_the_plain_chain(variant, tile):
    from lumfuncmcmc_amd.sampler import DeviceEnsembleSampler
    ctx = context(variant, tile, sigma=np.zeros(N))
    try:
        pos, seed = start(variant, 18), 77
        a = DeviceEnsembleSampler(ctx, 18, seed=seed, capacity=STEPS)
        a.run_mcmc(pos, STEPS)
        b = DeviceEnsembleSampler(ctx, 18, seed=seed, capacity=STEPS, likelihood="convolved")
        b.run_mcmc(pos, STEPS)
        np.testing.assert_array_equal(a.chain, b.chain)
        np.testing.assert_array_equal(a.lnprobability, b.lnprobability)
        np.testing.assert_array_equal(a.naccepted, b.naccepted)
        assert 0 < a.naccepted.sum()
        a.close(); b.close()
    finally:
        ctx.close()


@pytest.mark.parametrize("variant,tile", [("fixcomp", 1), ("free", 0)])
def test_hand_sharded_halves_give_the_chain_of_run(variant, tile):
    """lf_sampler_half_eval on two ranges of the half, lf_sampler_half_accept on the whole: one GPU, torch's stream"""
    import torch
    from lumfuncmcmc_amd.sampler import DeviceEnsembleSampler
    ctx = context(variant, tile)
    try:
        W, seed = 18, 4242
        pos = start(variant, W)
        whole = DeviceEnsembleSampler(ctx, W, seed=seed, capacity=STEPS, likelihood="convolved")
        whole.run_mcmc(pos, STEPS)
        ds = DeviceEnsembleSampler(ctx, W, seed=seed, capacity=STEPS, likelihood="convolved")
        lib, half = ctx._lib, W // 2
        ctx._check(lib.lf_sampler_start(ds._h, ds._p(np.ascontiguousarray(pos)), None))
        buf = torch.full((half,), float("nan"), dtype=torch.float64, device="cuda")
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        for _ in range(STEPS):
            for h in (0, 1):
                for lo, hi in ((0, 4), (4, half)):
                    ctx._check(lib.lf_sampler_half_eval(ds._h, h, lo, hi, ctypes.c_void_p(buf.data_ptr()), stream))
                ctx._check(lib.lf_sampler_half_accept(ds._h, h, ctypes.c_void_p(buf.data_ptr()), stream))
        ds.sync()
        np.testing.assert_array_equal(ds.chain, whole.chain)
        np.testing.assert_array_equal(ds.lnprobability, whole.lnprobability)
        np.testing.assert_array_equal(ds.naccepted, whole.naccepted)
        whole.close(); ds.close()
    finally:
        ctx.close()


@pytest.mark.parametrize("variant,tile", [("fixcomp", 0), ("fixcomp", 1), ("zevol", 1)])
def test_tempered_chain_replays_on_the_host(variant, tile):
    """T = 3, W = 8 against sampler.PTSampler over ctx.lnprob_err_batch (tests/test_gpu_pt.py with the likelihood swapped); the
    start's lnlike given, and left to the sampler"""
    from lumfuncmcmc_amd.sampler import DevicePTSampler, PTSampler
    ctx = context(variant, tile)
    try:
        T, W, seed = 3, 8, 0xFEEDFACE12345
        betas = [1.0, 0.5, 0.2]
        pos = synth.walkers(variant, T * W, seed=64, nf=NF[variant]).reshape(T, W, ctx.ndim)
        host = PTSampler(T, W, ctx.ndim, ctx.lnprob_err_batch, betas=betas, seed=seed)
        host.run_mcmc(pos, STEPS)
        ll0 = ctx.lnprob_err_batch(pos.reshape(T * W, -1)).reshape(T, W)
        for lnlike0 in (ll0, None):
            dev = DevicePTSampler(ctx, T, W, betas=betas, seed=seed, capacity=STEPS, likelihood="convolved")
            dev.run_mcmc(pos, 12, lnlike0=lnlike0)
            dev.run_mcmc(None, STEPS - 12)
            np.testing.assert_array_equal(dev.chain, host.chain)
            np.testing.assert_array_equal(dev.lnlikelihood, host.lnlikelihood)
            np.testing.assert_array_equal(dev.naccepted, host.naccepted)
            np.testing.assert_array_equal(dev.nswap, host.nswap)
            dev.close()
        assert host.naccepted.sum() > 0
        plain = PTSampler(T, W, ctx.ndim, ctx.lnprob_batch, betas=betas, seed=seed)
        plain.run_mcmc(pos, 2)
        assert not np.array_equal(plain.lnlikelihood, host.lnlikelihood[:, :, :2])
    finally:
        ctx.close()


@pytest.mark.parametrize("variant,tile", [("fixcomp", 1), ("free", 0)])
def test_one_temperature_is_the_convolved_ensemble_chain(variant, tile):
    from lumfuncmcmc_amd.sampler import DeviceEnsembleSampler, DevicePTSampler
    ctx = context(variant, tile)
    try:
        W, seed = 16, 0x1234567890ABCDEF
        pos = start(variant, W)
        ds = DeviceEnsembleSampler(ctx, W, seed=seed, capacity=STEPS, likelihood="convolved")
        ds.run_mcmc(pos, STEPS)
        pt = DevicePTSampler(ctx, 1, W, betas=[1.0], seed=seed, capacity=STEPS, likelihood="convolved")
        pt.run_mcmc(pos[None], STEPS)
        np.testing.assert_array_equal(pt.chain[0], ds.chain)
        np.testing.assert_array_equal(pt.lnlikelihood[0], ds.lnprobability)
        np.testing.assert_array_equal(pt.naccepted[0], ds.naccepted)
        assert 0 < ds.naccepted.sum()
        pt.close(); ds.close()
    finally:
        ctx.close()


def test_refusals_leave_the_context_usable():
    """LF_ERR_ARG with a message: no errors set, after a step, a source-sharded context (skip_grid)"""
    from lumfuncmcmc_amd.capi import LF_ERR_ARG, LFContext, LFError
    from lumfuncmcmc_amd.sampler import DeviceEnsembleSampler, DevicePTSampler
    ctx = LFContext(make_inputs("fixcomp", N, seed=31, S=23))
    try:
        lib = ctx._lib
        W, pos = 16, start("fixcomp", 16)
        ds = DeviceEnsembleSampler(ctx, W, seed=1, capacity=STEPS)
        pt = DevicePTSampler(ctx, 1, W, betas=[1.0], seed=1, capacity=STEPS)
        for fn, h in ((lib.lf_sampler_set_likelihood, ds._h), (lib.lf_ptsampler_set_likelihood, pt._h)):
            assert fn(h, 1) == LF_ERR_ARG
            assert b"no luminosity errors set" in lib.lf_last_error(ctx._h)
        with pytest.raises(LFError, match="error -1.*no luminosity errors set"):
            DeviceEnsembleSampler(ctx, W, seed=1, capacity=STEPS, likelihood="convolved")
        with pytest.raises(LFError, match="error -1.*no luminosity errors set"):
            DevicePTSampler(ctx, 1, W, betas=[1.0], seed=1, capacity=STEPS, likelihood="convolved")
        ctx.set_lum_err(seeded_sigma(N, 2), K, unchecked=True)
        ctx.set_option("skip_grid", 1)
        for fn, h in ((lib.lf_sampler_set_likelihood, ds._h), (lib.lf_ptsampler_set_likelihood, pt._h)):
            assert fn(h, 1) == LF_ERR_ARG
            assert b"source-sharded" in lib.lf_last_error(ctx._h)
        ctx.set_option("skip_grid", 0)
        ok = ctx.lnprob_err_batch(pos)
        # between the start and the first step: taken; after a step: refused, either way
        ds.enqueue(pos, 0)
        ds.set_likelihood("convolved")
        ds.enqueue(None, 3)
        pt.run_mcmc(pos[None], 2)
        for fn, h, v in ((lib.lf_sampler_set_likelihood, ds._h, 0), (lib.lf_ptsampler_set_likelihood, pt._h, 1)):
            assert fn(h, v) == LF_ERR_ARG
            assert b"has taken a step" in lib.lf_last_error(ctx._h)
        with pytest.raises(LFError, match="error -1.*has taken a step"):
            ds.set_likelihood("plain")
        # the chain that switched after its start is the convolved one, and everything still works
        ds.enqueue(None, STEPS - 3)
        ds.sync()
        chain, lnp, nacc = host_replay(ctx, pos, STEPS, 1, lnprob=ctx.lnprob_err_batch)
        np.testing.assert_array_equal(ds.chain, chain)
        np.testing.assert_array_equal(ds.lnprobability, lnp)
        assert np.array_equal(ctx.lnprob_err_batch(pos), ok)
        ds.close(); pt.close()
    finally:
        ctx.close()


def test_diagnostics_on_the_convolved_chain():
    """lf_sampler_diag / lf_ptsampler_diag on the convolved chains equal lf_chain_diag on the chains read back (the criterion
    of tests/test_gpu_diag.py: every output the same bits)"""
    from lumfuncmcmc_amd.sampler import DeviceEnsembleSampler, DevicePTSampler, chain_diagnostics
    ctx = context("fixcomp", 1)
    try:
        W, steps = 16, 300
        pos = start("fixcomp", W)
        ds = DeviceEnsembleSampler(ctx, W, seed=5, capacity=steps, likelihood="convolved")
        ds.run_mcmc(pos, steps)
        for t0 in (0, 100):
            on = ds.diagnostics(t0=t0, with_lnprob=True)
            off = chain_diagnostics(ds.chain, lnprob=ds.lnprobability, t0=t0)
            for k in ("tau", "window", "ess", "rhat"):
                np.testing.assert_array_equal(getattr(on, k), getattr(off, k))
        pt = DevicePTSampler(ctx, 2, W, betas=[1.0, 0.5], seed=5, capacity=steps, likelihood="convolved")
        pt.run_mcmc(np.array([pos, start("fixcomp", W, seed=34)]), steps)
        for t in (0, 1):
            on = pt.diagnostics(t, with_lnlike=True)
            off = chain_diagnostics(pt.chain[t], lnprob=pt.lnlikelihood[t])
            for k in ("tau", "window", "ess", "rhat"):
                np.testing.assert_array_equal(getattr(on, k), getattr(off, k))
        ds.close(); pt.close()
    finally:
        ctx.close()
