"""The convolved likelihood under a cut on the observed flux on the device (csrc/lf_deconv_cut.h, lf_set_cut_error_model,
lf_cut_term_batch) against its NumPy twin (deconv.cut_term, itself checked against 30-digit integration
in tests/test_deconv_cut_cpu.py):

    |dev - twin| <= 1e-12 sum_n |c_n phi Omega|   for Delta B alone,
    |dev - (lnprob + Delta_twin - Delta B_twin)| <= 1e-12 (|lnprob| + sum_i |Delta_i| + sum_n |c_n phi Omega|)   for the value,

then the -inf pattern, batch independence, a device sampler's chain and the refusals."""
import numpy as np
import pytest

import lf_cutlib as C
from lf_testlib import synth
from lumfuncmcmc_amd import deconv as D

pytestmark = pytest.mark.gpu
TOL = 1e-12
K = 8
# the nodes of a row: one below, at and one above a wave and a block of the kernel, and the whole list
LIMITS = [63, 64, 65, 255, 256, 257, 0]


def seeded_sigma(n, seed):
    rng = np.random.default_rng(seed)
    sg = rng.uniform(0.0, 0.04, n)
    sg[rng.permutation(n)[:max(1, n // 10)]] = 0.0
    return sg


def rows(inp, B, seed):
    nf = len(inp["field_ind"]) - 1
    th = synth.walkers(inp["variant"], B, seed=seed, fix_sch_al=bool(inp["fix_sch_al"]), nf=nf)
    if B > 3:
        th[3, 0] = 39.5                  # outside the box
    return th


def context(inp, model, sigma, limit=0, tile=0):
    from lumfuncmcmc_amd.capi import LFContext
    ctx = LFContext(inp)
    ctx.set_option("deconv_cut_limit", limit)
    ctx.set_cut_error_model(*model)
    ctx.set_lum_err(sigma, K)
    ctx.set_option("deconv_tile", tile)
    return ctx


def check(inp, model, limit, label):
    th = rows(inp, 9, seed=7)
    sg = seeded_sigma(len(inp["lum"]), 3)
    ctx = context(inp, model, sg, limit)
    try:
        info = ctx.cut_info()
        nl, H = D.cut_nodes(inp, *model, limit=limit)
        lp = ctx.lnprob_batch(th)
        fin = np.isfinite(lp)
        assert fin.sum() >= 4
        dev = ctx.cut_term_batch(th)
        tw, sabs = D.cut_term(inp, *model, th, terms=True, limit=limit)
        assert np.array_equal(np.isnan(dev), ~fin)
        r1 = np.abs(dev[fin] - tw[fin]) / sabs[fin]
        val = ctx.lnprob_err_batch(th)
        ref, _, sall = D.lnprob_err(inp, sg, th, K=K, terms=True, cut=model) if limit == 0 else \
            D.lnprob_err_cut(inp, sg, th, model, K=K, terms=True, limit=limit)
        assert np.array_equal(np.isneginf(val), np.isneginf(lp)) and not np.isnan(val).any()
        r2 = np.abs(val[fin] - ref[fin]) / (np.abs(lp[fin]) + sall[fin])
        print("cut %-28s nodes %s chunks %d: term %.3e value %.3e of the bound; Delta B %.4e of lnprob %.4e"
              % (label, info["nnodes"].tolist(), info["chunks"], r1.max() / TOL, r2.max() / TOL, tw[fin][0], lp[fin][0]))
        assert info["nnodes"].tolist() == [n["L"].size for n in nl] and np.allclose(info["H"], H, rtol=1e-15)
        assert info["chunks"] == sum(-(-n["L"].size // info["chunk"]) for n in nl)
        assert r1.max() <= TOL and r2.max() <= TOL
        assert np.all(np.abs(tw[fin]) > 0.0)
    finally:
        ctx.close()


@pytest.mark.parametrize("limit", LIMITS)
@pytest.mark.parametrize("variant", ["free", "fixcomp", "zevol"])
def test_term_and_value_against_twin_one_field(variant, limit):
    inp = C.cut_inputs(variant, n=200, S=5, nf=1)
    check(inp, C.flux_model(0.09), limit, "%s S=5 nf=1 limit %d" % (variant, limit))


@pytest.mark.parametrize("variant", ["free", "fixcomp", "zevol"])
def test_term_and_value_against_twin_five_fields(variant):
    """size_ln 101, five fields, one of them without sources, every field with its own errors"""
    inp = C.cut_inputs(variant, n=400, S=101, nf=5, empty_field=2)
    nodes, sig = C.flux_model(0.06, nf=5)
    sig = np.minimum(sig * np.array([1.0, 0.5, 1.2, 0.8, 1.5])[:, None], D.CUT_SIGMA_MAX)
    check(inp, (nodes, sig), 0, "%s S=101 nf=5" % variant)


def test_zero_errors_launch_nothing():
    inp = C.cut_inputs("fixcomp", n=200, S=5, nf=2)
    sg = seeded_sigma(200, 3)
    th = rows(inp, 5, seed=7)
    ctx = context(inp, C.const_model(0.0, nf=2), sg)
    try:
        assert ctx.cut_info()["chunks"] == 0
        fin = np.isfinite(ctx.lnprob_batch(th))
        assert np.all(ctx.cut_term_batch(th)[fin] == 0.0)
        ref = D.lnprob_err(inp, sg, th, K=K)
        assert np.all(np.abs(ctx.lnprob_err_batch(th)[fin] - ref[fin]) <= 1e-12 * np.abs(ref[fin]))
    finally:
        ctx.close()


def test_batch_independence():
    """a row has the same bits at B = 1, 37 and 300 (permuted), across two calls, through the device entry and with deconv_tile"""
    import torch
    inp = C.cut_inputs("fixcomp", n=300, S=23, nf=5)
    model = C.flux_model(0.09, nf=5)
    sg = seeded_sigma(300, 5)
    th = rows(inp, 300, seed=9)
    ctx = context(inp, model, sg)
    try:
        full = ctx.lnprob_err_batch(th)
        assert np.isfinite(full).sum() > 100
        np.testing.assert_array_equal(ctx.lnprob_err_batch(th), full)
        perm = np.random.default_rng(1).permutation(300)
        np.testing.assert_array_equal(ctx.lnprob_err_batch(th[perm]), full[perm])
        np.testing.assert_array_equal(ctx.lnprob_err_batch(th[:37]), full[:37])
        for r in (0, 5, 299):
            np.testing.assert_array_equal(ctx.lnprob_err_batch(th[r:r + 1]), full[r:r + 1])
        np.testing.assert_array_equal(ctx.lnprob_err_torch(torch.from_numpy(th).cuda()).cpu().numpy(), full)
        term = ctx.cut_term_batch(th)
        np.testing.assert_array_equal(ctx.cut_term_batch(th[perm]), term[perm])
        np.testing.assert_array_equal(ctx.cut_term_batch(th[7:8]), term[7:8])
        ctx.set_option("deconv_tile", 1)
        tiled = ctx.lnprob_err_batch(th)
        np.testing.assert_array_equal(ctx.lnprob_err_batch(th[perm]), tiled[perm])
        np.testing.assert_array_equal(ctx.lnprob_err_batch(th[:37]), tiled[:37])
        fin = np.isfinite(full)
        assert np.array_equal(np.isfinite(tiled), fin) and np.all(np.abs(tiled[fin] - full[fin]) <= 1e-12 * np.abs(full[fin]))
    finally:
        ctx.close()


def _class_object(**extra):
    from lf_deconvlib import fixcomp_model
    cat = synth.catalogue(400, seed=17)
    return fixcomp_model(cat, deconvolve=True, min_comp_frac=0.5, deconvolve_cut=True, deconvolve_order=12, **extra)


def test_sampler_chain_on_a_min_comp_frac_object():
    """16 walkers, 10 steps of the device sampler on the convolved likelihood of a min_comp_frac = 0.5 object: the stored lnprob
    is what lnprob_err_batch gives for the stored positions, bit for bit"""
    from lumfuncmcmc_amd.sampler import DeviceEnsembleSampler
    o = _class_object()
    try:
        ctx = o.context()
        assert ctx.cut_info()["chunks"] > 0
        rng = np.random.default_rng(4)
        pos = np.array([synth.LSTAR, synth.PHISTAR, synth.SCH_AL]) + 0.05 * rng.standard_normal((16, 3))
        assert np.isfinite(ctx.lnprob_err_batch(pos)).all()
        assert not np.array_equal(ctx.lnprob_err_batch(pos), ctx.lnprob_batch(pos))
        ds = DeviceEnsembleSampler(ctx, 16, seed=0xC07, capacity=10, likelihood="convolved")
        ds.enqueue(pos, 10)
        ds.sync()
        chain, lnp = np.array(ds.chain), np.array(ds.lnprobability)
        ds.close()
        flat = chain.reshape(-1, chain.shape[-1])
        np.testing.assert_array_equal(ctx.lnprob_err_batch(flat).reshape(lnp.shape), lnp)
        # the class's own value is the same entry
        assert o.lnprob_fix_comp(pos[0]) == ctx.lnprob_err_batch(pos[:1])[0]
    finally:
        o.close()


def test_lum_posterior_is_served_under_the_cut():
    o = _class_object()
    try:
        ctx = o.context()
        th = np.array([[synth.LSTAR, synth.PHISTAR, synth.SCH_AL]])
        m1, m2, used = ctx.lum_posterior(th)
        r1, r2, rused = D.lum_posterior(o.kernel_inputs(), np.asarray(o.lum_e), th, K=12)
        assert used == rused == 1
        assert np.all(np.abs(m1 - r1) <= 1e-10 * np.abs(r1) + 1e-15) and np.all(np.abs(m2 - r2) <= 1e-10 * np.abs(r2) + 1e-15)
    finally:
        o.close()


def test_refusals():
    from lumfuncmcmc_amd.capi import LFContext, LFError
    from lf_testlib import make_inputs
    inp = C.cut_inputs("fixcomp", n=100, S=5, nf=2)
    model = C.flux_model(0.09, nf=2)
    sg = np.full(100, 0.03)
    th = rows(inp, 3, seed=7)
    ctx = LFContext(inp)
    try:
        with pytest.raises(LFError, match="error -1.*min_comp_frac.*lf_set_cut_error_model"):
            ctx.set_lum_err(sg, K)
        with pytest.raises(LFError, match="0.30 dex"):
            ctx.set_cut_error_model(model[0], np.full((2, model[0].size), 0.31))
        with pytest.raises(LFError, match="nodes must increase"):
            ctx.set_cut_error_model(model[0][::-1].copy(), model[1])
        with pytest.raises(LFError, match="all 0"):
            ctx.set_cut_error_model(np.array([-17.0, -16.0]), np.array([[0.0, 0.1], [0.1, 0.1]]))
        with pytest.raises(LFError, match="finite"):
            ctx.set_cut_error_model(model[0], np.full((2, model[0].size), np.nan))
        with pytest.raises(LFError, match="no cut model"):
            ctx.cut_info()
        ctx.set_cut_error_model(*model)
        ctx.set_lum_err(sg, K)
        assert np.isfinite(ctx.lnprob_err_batch(th)).any()
        with pytest.raises(LFError, match="gradient of Delta B"):
            ctx.lnprob_err_grad(th)
        with pytest.raises(LFError, match="per-source volumes"):
            ctx.veff_true(th, np.linspace(41.0, 44.0, 7), 1.0, 1.0)
        with pytest.raises(LFError, match="before lf_set_lum_err"):
            ctx.set_cut_error_model(*model)
        assert np.isfinite(ctx.lnprob_err_batch(th)).any()             # (the context stays usable)
    finally:
        ctx.close()
    # the sharded options; a context without the cut
    ctx = LFContext(inp)
    try:
        ctx.set_option("skip_grid", 1)
        with pytest.raises(LFError, match="source-sharded"):
            ctx.set_cut_error_model(*model)
        ctx.set_option("skip_grid", 0)
        ctx.set_option("grid_share", 0 + 65536 * 2)
        with pytest.raises(LFError, match="source-sharded"):
            ctx.set_cut_error_model(*model)
    finally:
        ctx.close()
    ctx = LFContext(make_inputs("fixcomp", 100, S=5, nf=2))
    try:
        with pytest.raises(LFError, match="no cut on the observed flux"):
            ctx.set_cut_error_model(*model)
    finally:
        ctx.close()
    o = _class_object()
    try:
        with pytest.raises(NotImplementedError, match="gradient of Delta B"):
            o.fit_model_map(nstarts=2, likelihood="convolved")
        with pytest.raises(NotImplementedError, match="own volume"):
            o.veff_deconvolved()
    finally:
        o.close()
