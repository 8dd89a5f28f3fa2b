"""The flux-error-convolved likelihood on the device (csrc/lf_deconv.h, lf_set_lum_err, lf_lnprob_err_batch; DESIGN.md section
3.18) against its NumPy twin (lumfuncmcmc_amd/deconv.py, itself checked against 30-digit integration in
tests/test_deconv_cpu.py):

    |dev - (lnprob + Delta_twin)| <= 1e-12 (|lnprob| + sum_i |Delta_i|),   -inf pattern identical to lnprob's,

lnprob being the plain path's value of the same rows; then exact zeros, batch independence, the device form, the refusals and
the model classes on top of it."""
import os

import numpy as np
import pytest

import lf_deconvlib as L
from lf_testlib import O, make_inputs, synth
from lumfuncmcmc_amd import deconv as D

pytestmark = pytest.mark.gpu
TOL = 1e-12
ORDERS = sorted({D.ORDERS[0], D.DEFAULT_ORDER, 32})
GOLDENS = [("free_n50", "free"), ("free_n1000", "free"), ("fixcomp_n50", "fixcomp"), ("zevol_n800", "zevol")]
CH = D.CHUNK
FIELDS = {1: [(n,) for n in (1, CH - 1, CH, CH + 1)], 5: [(1, CH - 1, CH, CH + 1, 7)]}


def seeded_sigma(n, seed):
    """sigma in [0, 0.3], a tenth of the sources at exactly 0"""
    rng = np.random.default_rng(seed)
    sg = rng.uniform(0.0, 0.3, n)
    sg[rng.permutation(n)[:max(1, n // 10)]] = 0.0
    return sg


def check_case(inp, th, label, seed=1):
    from lumfuncmcmc_amd.capi import LFContext
    n = len(inp["lum"])
    sg = seeded_sigma(n, seed)
    ctx = LFContext(inp)
    worst = 0.0
    try:
        lp = ctx.lnprob_batch(th)
        fin = np.isfinite(lp)
        for K in ORDERS:
            ctx.set_lum_err(sg, K, unchecked=True)
            dev = ctx.lnprob_err_batch(th)
            tot, _, sabs = D.delta(inp, sg, th, K=K, terms=True)
            assert np.array_equal(np.isneginf(dev), np.isneginf(lp)) and not np.isnan(dev).any(), "%s K=%d: -inf pattern" % (label, K)
            err = np.abs(dev[fin] - (lp[fin] + tot[fin]))
            ratio = err / (np.abs(lp[fin]) + sabs[fin])
            w = float(ratio.max()) if ratio.size else 0.0
            print("deconv %-30s K=%2d rows %2d finite, max |dev - twin| / bound = %.3e" % (label, K, int(fin.sum()), w / TOL))
            assert w <= TOL, (label, K, w)
            worst = max(worst, w)
    finally:
        ctx.close()
    return worst


def rows37(inp, seed):
    nf = len(inp["field_ind"]) - 1
    th = synth.walkers(inp["variant"], 37, seed=seed, fix_sch_al=bool(inp["fix_sch_al"]), nf=nf)
    th[3, 0] = 39.5                      # outside the box
    th[20, 0] = 40.001                   # inside, but the bright sources underflow
    if inp["variant"] == "zevol":
        th[20, 0:3] = 40.001
    return th


@pytest.mark.parametrize("name,variant", GOLDENS)
def test_device_against_twin_goldens(golden_dir, name, variant):
    g = np.load(os.path.join(golden_dir, name + ".npz"))
    check_case(O.inputs_from_golden(g, variant), np.asarray(g["theta"], dtype=np.float64), name)


@pytest.mark.parametrize("variant", ["free", "fixcomp", "zevol"])
@pytest.mark.parametrize("nf", [1, 5])
def test_device_against_twin_chunk_edges(variant, nf):
    """1, chunk - 1, chunk and chunk + 1 sources in a field"""
    for sizes in FIELDS[nf]:
        inp = make_inputs(variant, int(sum(sizes)), seed=5 + sizes[0], S=23, nf=nf)
        inp["field_ind"] = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        check_case(inp, rows37(inp, 7)[:12], "%s nf=%d sizes=%s" % (variant, nf, sizes), seed=sizes[0])


@pytest.mark.parametrize("variant", ["free", "fixcomp", "zevol"])
def test_bits(variant):
    """sigma = 0 everywhere: lf_lnprob_batch's bits; a row alone, in its batch of 37 and in a permuted batch of 300, twice, and
    through the device entry point: the same bits"""
    import torch
    from lumfuncmcmc_amd.capi import LFContext
    inp = make_inputs(variant, 4500, seed=2, S=23)
    th = rows37(inp, 3)
    rng = np.random.default_rng(5)
    idx = rng.integers(0, 37, 300)
    idx[:37] = rng.permutation(37)
    ctx = LFContext(inp)
    try:
        lp = ctx.lnprob_batch(th)
        ctx.set_lum_err(np.zeros(4500))
        assert np.array_equal(ctx.lnprob_err_batch(th), lp)
        ctx.set_lum_err(seeded_sigma(4500, 4), 8, unchecked=True)
        e37 = ctx.lnprob_err_batch(th)
        assert np.array_equal(ctx.lnprob_err_batch(th), e37)
        assert np.array_equal(ctx.lnprob_err_batch(th[idx]), e37[idx])
        assert np.array_equal(np.array([ctx.lnprob_err_batch(th[i:i + 1])[0] for i in range(37)]), e37)
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            dev = ctx.lnprob_err_torch(torch.from_numpy(th).cuda())
        st.synchronize()
        assert np.array_equal(dev.cpu().numpy(), e37)
        assert np.isfinite(e37).sum() >= 30 and np.any(e37[np.isfinite(e37)] != lp[np.isfinite(e37)])
    finally:
        ctx.close()


def test_refusals():
    """LF_ERR_ARG with a message, nothing launched, the context stays usable"""
    from lumfuncmcmc_amd.capi import LFContext, LFError
    inp = make_inputs("free", 300, seed=4, S=23)
    th = rows37(inp, 9)
    ctx = LFContext(inp)
    try:
        with pytest.raises(LFError, match="error -1.*no luminosity errors set"):
            ctx.lnprob_err_batch(th)
        for bad, what in ((-0.01, "finite and >= 0"), (np.nan, "finite and >= 0")):
            sg = np.full(300, 0.02)
            sg[17] = bad
            with pytest.raises(LFError, match="error -1.*" + what):
                ctx.set_lum_err(sg)
        with pytest.raises(LFError, match="error -1.*not supported"):
            ctx.set_lum_err(np.full(300, 0.02), 7)
        with pytest.raises(LFError, match="error -1.*above 0.06 dex"):
            ctx.set_lum_err(np.full(300, 0.07), 12)
        with pytest.raises(LFError, match="no luminosity errors set"):
            ctx.lnprob_err_batch(th)
        ctx.set_lum_err(np.full(300, 0.05))
        ok = ctx.lnprob_err_batch(th)
        ctx.set_option("skip_grid", 1)
        with pytest.raises(LFError, match="error -1.*source-sharded"):
            ctx.lnprob_err_batch(th)
        ctx.set_option("skip_grid", 0)
        assert np.array_equal(ctx.lnprob_err_batch(th), ok)
    finally:
        ctx.close()
    # min_comp_frac = 0.5: the grid's columns have their own luminosity nodes
    inp["logL"] = inp["logL"].copy()
    inp["logL"][:, 5:] += 1e-3 * np.linspace(1, 0, inp["logL"].shape[0])[:, None]
    ctx = LFContext(inp)
    try:
        with pytest.raises(LFError, match="error -1.*min_comp_frac"):
            ctx.set_lum_err(np.full(300, 0.02))
    finally:
        ctx.close()


def test_class_surface_and_fit_model():
    """lnprob of a deconvolve=True object is the C entry's; a 32-walker, 20-step fit_model on a 1000-source noisy mock runs and
    its lnprobability is what re-evaluating the stored positions gives, bit for bit"""
    np.random.seed(5)
    o, theta, _ = L.noisy_mock(1000, 0.05, 11, deconvolve=True)
    try:
        assert o.deconvolve and o.deconvolve_order == D.DEFAULT_ORDER
        rows = o.get_init_walker_values(16)
        ctx = o.context()
        assert np.array_equal(o.lnprob_fix_comp(rows), ctx.lnprob_err_batch(rows))
        assert o.lnprob_fix_comp(theta) == ctx.lnprob_err_batch(theta)[0] != ctx.lnprob_batch(theta)[0]
        o.fit_model()
        assert o.chain.shape == (32, 20, 3)
        lnp = o.sampler.lnprobability
        again = ctx.lnprob_err_batch(o.chain.reshape(-1, 3)).reshape(32, 20)
        assert np.array_equal(lnp, again)
        assert o.samples.shape[1] == 4
    finally:
        o.close()


def test_eddington_profile_on_the_device():
    """the seeded profile of tests/test_deconv_cpu.py: the device's two maxima sit on the twin's grid points"""
    from lumfuncmcmc_amd.capi import LFContext
    from lumfuncmcmc_amd import grad as G
    inp, sigma, theta, rows = L.eddington_case()
    lp_t = G.lnprob_grad(inp, rows)[0]
    conv_t = lp_t + D.delta(inp, sigma, rows, K=D.DEFAULT_ORDER)
    ctx = LFContext(inp)
    try:
        ctx.set_lum_err(sigma, unchecked=True)
        lp_d, conv_d = ctx.lnprob_batch(rows), ctx.lnprob_err_batch(rows)
    finally:
        ctx.close()
    print("Eddington profile on the device: plain argmax %+.2f dex, convolved argmax %+.2f dex"
          % (L.EDD_GRID[int(np.argmax(lp_d))], L.EDD_GRID[int(np.argmax(conv_d))]))
    assert int(np.argmax(lp_d)) == int(np.argmax(lp_t)) and int(np.argmax(conv_d)) == int(np.argmax(conv_t))
