"""Teardown: whatever the library allocates on the device goes when its owner is destroyed (csrc/lf_devmem.h).

One process, the public classes only.  A cycle makes a context of every variant, evaluates at two batch sizes (the workspace
regrows), switches the compressed catalogue on and off, runs a few steps of the device sampler and of the tempered one, draws
a mock catalogue and a histogram, and destroys everything.  After a warm-up cycle (the runtime's own pools and code objects
are then in place) ten more cycles must not lower the free device memory by more than the footprint of ONE cycle's objects
(measured in the warm-up cycle: free memory after it minus the lowest seen while its objects were alive).  The allowance is
derived, not tuned: a leak of an object set costs ten footprints over the ten cycles, the allocator's granularity well
under one.  A coarse guard - a leaked 4-byte word hides under it; that the host layer has no free of its own to forget is
what the structure of lfmcmc.hip guarantees.  Nothing here provokes an allocation failure."""
import numpy as np
import pytest

from lf_testlib import make_inputs, synth

pytestmark = pytest.mark.gpu

CYCLES = 10
N_SOURCES = {"free": 20000, "fixcomp": 3000, "zevol": 4000}
MOCK_ROWS = {}


def _cycle(note):
    """One set of objects of every variant, used and destroyed; note() is called while they are alive."""
    from lumfuncmcmc_amd import mock
    from lumfuncmcmc_amd.capi import LFContext
    from lumfuncmcmc_amd.sampler import DeviceEnsembleSampler, DevicePTSampler
    alive = []
    try:
        for k, variant in enumerate(("free", "fixcomp", "zevol")):
            inp = make_inputs(variant, N_SOURCES[variant], seed=71 + k)
            ctx = LFContext(inp, max_batch=64)
            alive.append(ctx)
            small, big = synth.walkers(variant, 16, seed=72), synth.walkers(variant, 300, seed=73)
            a = ctx.lnprob_batch(small)
            b = ctx.lnprob_batch(big)                          # (beyond max_batch and its double: the workspace regrows)
            assert np.isfinite(a).any() and np.isfinite(b).any()
            ctx.set_option("compress", 1)
            c = ctx.lnprob_batch(small)
            ctx.set_option("compress", 0)
            np.testing.assert_array_equal(ctx.lnprob_batch(small), a)
            np.testing.assert_allclose(c[np.isfinite(a)], a[np.isfinite(a)], rtol=1e-10)
            W = 2 * ctx.ndim
            ds = DeviceEnsembleSampler(ctx, W, seed=5, capacity=8)
            alive.append(ds)
            ds.run_mcmc(synth.walkers(variant, W, seed=74), 4)
            assert ds.chain.shape == (W, 4, ctx.ndim)
            pt = DevicePTSampler(ctx, 2, W, betas=[1.0, 0.5], seed=6, capacity=8)
            alive.append(pt)
            pt.run_mcmc(synth.walkers(variant, 2 * W, seed=75).reshape(2, W, ctx.ndim), 4)
            assert pt.chain.shape == (2, W, 4, ctx.ndim)
            gen = mock.MockGenerator(inp)
            alive.append(gen)
            if variant not in MOCK_ROWS:                       # four rows of the prior box, phi* shifted to ~5000 sources apiece
                th = synth.walkers(variant, 4, seed=76)
                phi = [3, 4, 5] if variant == "zevol" else [1]
                th[:, phi] += np.log10(5000.0 / mock.MockTwin(inp).means(th).sum(axis=1))[:, None]
                MOCK_ROWS[variant] = th
            th = MOCK_ROWS[variant]
            z, L, fld, off = gen.draw(th, 7)
            assert off[-1] == z.size > 0
            h = gen.hist(th, np.linspace(L.min(), L.max(), 21), 7)
            assert h.sum() == z.size
            note()
    finally:
        for o in reversed(alive):                              # samplers before their context
            o.close()


def test_ten_cycles_of_create_and_destroy_give_the_device_memory_back():
    import torch
    torch.cuda.init()
    torch.zeros(1).cuda()

    def free():
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info()[0]

    lowest = [free()]
    _cycle(lambda: lowest.__setitem__(0, min(lowest[0], free())))
    after_warmup = free()
    footprint = after_warmup - lowest[0]
    assert footprint > 0, "the warm-up cycle's objects took no device memory?"
    for _ in range(CYCLES):
        _cycle(lambda: None)
    end = free()
    print("footprint of one cycle %.1f MB, free memory after warm-up %.1f MB, after %d more cycles %.1f MB (lost %.2f MB)"
          % (footprint / 1e6, after_warmup / 1e6, CYCLES, end / 1e6, (after_warmup - end) / 1e6))
    assert after_warmup - end <= footprint, (after_warmup, end, footprint)
