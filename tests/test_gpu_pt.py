"""The parallel-tempered device sampler (lf_ptsampler_*): T = 1 is the ensemble sampler bit for bit, T > 1 replays bit for
bit on the host PTSampler over the same likelihood - also at the edges of lf_pt_swap's sort (pads, several passes, strided
loops, all of LDS, a half of one walker) - and fit_model_pt's evidence agrees with brute-force quadrature."""
import math

import numpy as np
import pytest

from lf_replaylib import fixcomp_model as _fixcomp_model, grid_lnint as _grid_lnint
from lf_testlib import make_inputs, synth

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("variant,n,W", [("free", 20000, 20), ("fixcomp", 3000, 16), ("zevol", 2000, 20)])
def test_one_temperature_is_the_ensemble_sampler(variant, n, W):
    from lumfuncmcmc_amd.capi import LFContext
    from lumfuncmcmc_amd.sampler import DeviceEnsembleSampler, DevicePTSampler
    ctx = LFContext(make_inputs(variant, n, seed=61))
    pos = synth.walkers(variant, W, seed=62)
    nsteps, seed = 20, 0x1234567890ABCDEF
    ds = DeviceEnsembleSampler(ctx, W, seed=seed, capacity=nsteps)
    ds.run_mcmc(pos, nsteps)
    pt = DevicePTSampler(ctx, 1, W, betas=[1.0], seed=seed, capacity=nsteps)
    pt.run_mcmc(pos[None], nsteps)
    assert pt.chain.shape == (1, W, nsteps, ctx.ndim)
    np.testing.assert_array_equal(pt.chain[0], ds.chain)
    np.testing.assert_array_equal(pt.lnlikelihood[0], ds.lnprobability)
    np.testing.assert_array_equal(pt.lnprobability[0], ds.lnprobability)
    np.testing.assert_array_equal(pt.naccepted[0], ds.naccepted)
    assert 0 < ds.acceptance_fraction.mean() < 1
    pt.close(); ds.close(); ctx.close()


def _assert_mean_lnlike(dev, host):
    """mean_lnlike against math.fsum(l) / W per temperature and step, l the W values of the (bit-equal) lnlikelihood.  The
    device adds the W numbers in an order of its own (64 lanes, then a butterfly); any recursive sum of W numbers is within
    (W - 1) 2^-53 sum|l_i| of the exact one (Higham, Accuracy and Stability of Numerical Algorithms, 4.2, first order), hence
    the mean within that over W."""
    T, W, S = host.lnlikelihood.shape
    assert dev.mean_lnlike.shape == (T, S)
    for t in range(T):
        for s in range(S):
            l = host.lnlikelihood[t, :, s]
            ref = math.fsum(l) / W
            bound = (W - 1) * 2.0 ** -53 * math.fsum(np.abs(l)) / W
            assert abs(dev.mean_lnlike[t, s] - ref) <= bound, (t, s, dev.mean_lnlike[t, s], ref, bound)


@pytest.mark.parametrize("variant,n", [("free", 20000), ("fixcomp", 2000)])
def test_device_chain_replays_on_the_host(variant, n):
    from lumfuncmcmc_amd.capi import LFContext
    from lumfuncmcmc_amd.sampler import DevicePTSampler, PTSampler
    ctx = LFContext(make_inputs(variant, n, seed=63))
    T, W, nsteps, seed = 3, 32, 30, 0xFEEDFACE12345
    betas = [1.0, 0.5, 0.2]
    pos = synth.walkers(variant, T * W, seed=64).reshape(T, W, ctx.ndim)
    dev = DevicePTSampler(ctx, T, W, betas=betas, seed=seed, capacity=nsteps)
    dev.run_mcmc(pos, 12)
    dev.run_mcmc(None, nsteps - 12)                       # continuing = one longer run
    host = PTSampler(T, W, ctx.ndim, ctx.lnprob_batch, betas=betas, seed=seed)
    host.run_mcmc(pos, nsteps)
    np.testing.assert_array_equal(dev.chain, host.chain)
    np.testing.assert_array_equal(dev.lnlikelihood, host.lnlikelihood)
    np.testing.assert_array_equal(dev.naccepted, host.naccepted)
    np.testing.assert_array_equal(dev.nswap, host.nswap)
    _assert_mean_lnlike(dev, host)
    assert dev.nswap.sum() > 0 and dev.tswap_acceptance_fraction.shape == (T - 1,)
    with pytest.raises(Exception):
        dev.run_mcmc(None, 1)                              # capacity exceeded is an error
    bad = pos.copy()
    bad[2, 5] = 99.0                                       # outside the prior: -inf at every temperature
    with pytest.raises(Exception, match="finite"):
        dev.run_mcmc(bad, 1)
    dev.close(); ctx.close()


# (T, W): Wp = the power of two >= W, 4096 / Wp runs of keys are sorted per pass, the kernel has 1024 threads
SWAP_EDGES = [
    (3, 20),        # pads: Wp = 32
    (64, 70),       # Wp = 128: 32 runs per pass, 63 pairs in two passes, the second partial
    (5, 1024),      # W = the thread count; 4 pairs fill exactly one pass
    (3, 2050),      # Wp = 4096: one run per pass, two passes, nearly half the slots are pads, strided loops
    (2, 4096),      # the maximum: all of LDS, no pads
    (2, 2),         # a half of one walker
]


@pytest.mark.parametrize("T,W", SWAP_EDGES)
def test_swap_replays_at_the_sort_edges(T, W):
    """lf_pt_swap against sampler.PTSampler (NumPy's stable argsort) over ctx.lnprob_batch: fixed completeness and fixed
    faint-end slope (ndim = 2), 2000 sources, 6 steps, a ladder close enough that every neighbouring pair swaps."""
    from lumfuncmcmc_amd.capi import LFContext
    from lumfuncmcmc_amd.sampler import DevicePTSampler, PTSampler, geometric_betas
    ctx = LFContext(make_inputs("fixcomp", 2000, seed=65, fix_sch_al=True))
    assert ctx.ndim == 2
    nsteps, seed = 6, 0xC0FFEE1234567
    betas = geometric_betas(64, 1e3) if T == 64 else geometric_betas(T, 4)
    pos = synth.walkers("fixcomp", T * W, seed=66, fix_sch_al=True).reshape(T, W, 2)
    dev = DevicePTSampler(ctx, T, W, betas=betas, seed=seed, capacity=nsteps)
    dev.run_mcmc(pos, nsteps)
    host = PTSampler(T, W, 2, ctx.lnprob_batch, betas=betas, seed=seed)
    host.run_mcmc(pos, nsteps)
    print("T %d W %d nswap %s" % (T, W, dev.nswap.tolist()))
    np.testing.assert_array_equal(dev.nswap, host.nswap)
    np.testing.assert_array_equal(dev.naccepted, host.naccepted)
    np.testing.assert_array_equal(dev.lnlikelihood, host.lnlikelihood)
    np.testing.assert_array_equal(dev.chain, host.chain)
    assert dev.nswap.shape == (T - 1,) and np.all(dev.nswap > 0)
    _assert_mean_lnlike(dev, host)
    dev.close(); ctx.close()


def test_evidence_agrees_with_quadrature():
    """Fixed completeness, fixed faint-end slope (theta = log L*, log phi*), 300 sources.  Quadrature: a 400 x 400 grid
    over the prior box finds the region within 40 nats of the peak; a box around it is refined (64, 128, ... cells a
    side) until halving the spacing moves lnZ by < 0.01; minus ln(box area).  fit_model_pt with its default ladder
    (Tmax from the data), 32 walkers per temperature, 1000 steps: within max(0.3, 3 dlnZ) nats."""
    np.random.seed(2026)
    m = _fixcomp_model(300, seed=71)
    ctx = m.context()
    box = m._theta_lims()
    assert box.shape == (2, 2)
    _, lp, x, y = _grid_lnint(ctx, box[:, 0], box[:, 1], 400)
    ix, iy = np.nonzero(lp > lp[np.isfinite(lp)].max() - 40.0)
    dx, dy = x[1] - x[0], y[1] - y[0]
    lo = np.maximum([x[ix.min()] - 3 * dx, y[iy.min()] - 3 * dy], box[:, 0])
    hi = np.minimum([x[ix.max()] + 3 * dx, y[iy.max()] + 3 * dy], box[:, 1])
    prev, n = None, 64
    while True:
        cur = _grid_lnint(ctx, lo, hi, n)[0]
        if prev is not None and abs(cur - prev) < 0.01:
            break
        assert n <= 2048, (prev, cur)
        prev, n = cur, 2 * n
    quad = cur - np.log(np.prod(box[:, 1] - box[:, 0]))
    lnZ, dlnZ = m.fit_model_pt()
    assert (m.lnZ, m.dlnZ) == (lnZ, dlnZ)
    print("lnZ %.4f +/- %.4f, quadrature %.4f (%d cells a side), %d temperatures, Tmax %.3g" % (
        lnZ, dlnZ, quad, n, m.pt_sampler.ntemps, 1.0 / m.pt_sampler.betas[-1]))
    assert abs(lnZ - quad) <= max(0.3, 3.0 * dlnZ), (lnZ, dlnZ, quad)
    assert m.samples.shape[1] == 3 and np.all(np.isfinite(m.samples))
    assert m.pt_sampler.chain.shape[:3] == (m.pt_sampler.ntemps, 32, 1000)
    m.close()


def test_fit_model_pt_refuses_several_ranks(monkeypatch):
    from lumfuncmcmc_amd.model import LumFuncMCMC
    m = _fixcomp_model(200, seed=72)
    monkeypatch.setattr(LumFuncMCMC, "_dist_state", staticmethod(lambda: (0, 2)))
    with pytest.raises(NotImplementedError):
        m.fit_model_pt(ntemps=2)
