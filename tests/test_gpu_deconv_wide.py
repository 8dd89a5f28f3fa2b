"""The wide rule of the flux-error-convolved likelihood on the device (csrc/lf_deconv_wide.h, option "deconv_wide"; DESIGN.md
section 3.21) against its NumPy twin (lumfuncmcmc_amd/deconv.py with wide=True, itself checked against 30-digit integration
in tests/test_deconv_wide_cpu.py), with the bounds of tests/test_gpu_deconv.py and tests/test_gpu_deconv_grad.py:

    |dev - (lnprob + Delta_twin)| <= 1e-12 (|lnprob| + sum_i |Delta_i|),   -inf pattern identical to lnprob's,
    |grad_dev - grad_twin| <= 1e-12 S_abs element-wise,   NaN pattern identical,

then what the option must leave alone (no source above the order's limit: the bits without it), batch independence, the device
entry, "deconv_tile", the refusal above the top edge, and the model classes, the MAP fit and the device sampler on top."""
import os

import numpy as np
import pytest

import lf_deconvlib as L
from lf_replaylib import host_replay
from lf_testlib import O, make_inputs, synth
from lumfuncmcmc_amd import deconv as D

pytestmark = pytest.mark.gpu
TOL = 1e-12
ORDERS = (4, 32)
GOLDENS = [("free_n50", "free"), ("fixcomp_n50", "fixcomp"), ("zevol_n800", "zevol")]
CH = D.WIDE_CHUNK
TOP = D.WIDE_SIGMA_MAX
VARIANTS = ["free", "fixcomp", "zevol"]


def mixed_sigma(n, seed):
    """sigma uniform in [0, top edge]: narrow and every class; a tenth of the sources at exactly 0"""
    rng = np.random.default_rng(seed)
    sg = rng.uniform(0.0, TOP, n)
    sg[rng.permutation(n)[:max(1, n // 10)]] = 0.0
    return sg


def rows37(inp, seed):
    nf = len(inp["field_ind"]) - 1
    th = synth.walkers(inp["variant"], 37, seed=seed, fix_sch_al=bool(inp["fix_sch_al"]), nf=nf)
    th[3, 0] = 39.5                      # outside the box
    th[20, 0] = 40.001                   # inside, but the bright sources underflow
    if inp["variant"] == "zevol":
        th[20, 0:3] = 40.001
    return th


def check_value(ctx, inp, th, sg, K, label):
    ctx.set_lum_err(sg, K, wide=True)
    lp, dev = ctx.lnprob_batch(th), ctx.lnprob_err_batch(th)
    fin = np.isfinite(lp)
    tot, _, sabs = D.delta(inp, sg, th, K=K, terms=True, wide=True)
    assert np.array_equal(np.isneginf(dev), np.isneginf(lp)) and not np.isnan(dev).any(), "%s K=%d: -inf pattern" % (label, K)
    ratio = np.abs(dev[fin] - (lp[fin] + tot[fin])) / (np.abs(lp[fin]) + sabs[fin])
    w = float(ratio.max()) if ratio.size else 0.0
    print("deconv wide %-34s K=%2d rows %2d finite, max |dev - twin| / bound = %.3e" % (label, K, int(fin.sum()), w / TOL))
    assert w <= TOL, (label, K, w)
    return dev


def check_grad(ctx, inp, th, sg, K, label):
    ctx.set_lum_err(sg, K, wide=True)
    val_d, g_d = ctx.lnprob_err_grad(th)
    assert np.array_equal(val_d, ctx.lnprob_err_batch(th)), "%s K=%d: the value differs from lnprob_err_batch" % (label, K)
    val_t, g_t, s_t = D.lnprob_err_grad(inp, sg, th, K=K, terms=True, wide=True)
    fin = np.isfinite(val_d)
    assert np.array_equal(fin, np.isfinite(val_t)) and np.all(val_d[~fin] == -np.inf), "%s K=%d: -inf pattern" % (label, K)
    assert np.array_equal(np.isnan(g_d), np.isnan(g_t)), "%s K=%d: NaN pattern" % (label, K)
    err, scale = np.abs(g_d[fin] - g_t[fin]), s_t[fin]
    assert np.all(err[scale == 0.0] == 0.0), "%s K=%d: an element without contributions is not 0" % (label, K)
    ratio = np.where(scale > 0.0, err / np.where(scale > 0.0, scale, 1.0), 0.0)
    w = float(np.max(ratio)) if ratio.size else 0.0
    print("deconv wide grad %-29s K=%2d rows %2d finite, max |dev - twin| / S_abs = %.3e" % (label, K, int(fin.sum()), w / TOL))
    assert w <= TOL, (label, K, w)


def check_case(inp, th, sg, label, grad=True):
    from lumfuncmcmc_amd.capi import LFContext
    ctx = LFContext(inp)
    try:
        for K in ORDERS:
            check_value(ctx, inp, th, sg, K, label)
            if grad:
                check_grad(ctx, inp, th, sg, K, label)
    finally:
        ctx.close()


@pytest.mark.parametrize("name,variant", GOLDENS)
def test_device_against_twin_goldens(golden_dir, name, variant):
    """value on the goldens' recorded rows, gradient on 37 seeded rows"""
    from lumfuncmcmc_amd.capi import LFContext
    g = np.load(os.path.join(golden_dir, name + ".npz"))
    inp = O.inputs_from_golden(g, variant)
    sg = mixed_sigma(len(inp["lum"]), 1)
    assert (sg > D.SIGMA_MAX).sum() >= 10
    ctx = LFContext(inp)
    try:
        for K in ORDERS:
            check_value(ctx, inp, np.asarray(g["theta"], dtype=np.float64), sg, K, name)
            check_grad(ctx, inp, rows37(inp, 11)[:12], sg, K, name)
    finally:
        ctx.close()


def edge_case(variant):
    """five fields holding 1, CH - 1, CH, CH + 1 and 0 wide sources, those of a field in one class: classes 4, 0, 1, 2 - class 3
    is empty and class 4 holds one source, at the top edge itself; the other sources are narrow, some at exactly 0"""
    wide = (1, CH - 1, CH, CH + 1, 0)
    sizes = (40, CH + 30, CH + 30, CH + 30, 30)
    inp = make_inputs(variant, int(sum(sizes)), seed=6, S=23, nf=5)
    fi = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    inp["field_ind"] = fi
    rng = np.random.default_rng(12)
    sg = rng.uniform(0.0, D.sigma_max(4), int(sum(sizes)))            # narrow under every order tested
    sg[::7] = 0.0
    lo_hi = {0: (TOP, TOP), 1: (0.0901, 0.10), 2: (0.1001, 0.15), 3: (0.1501, 0.20)}
    for f, nw in enumerate(wide):
        if nw:
            at = fi[f] + rng.permutation(sizes[f])[:nw]
            sg[at] = rng.uniform(*lo_hi[f], nw)
    cls = D.wide_class(sg, 32)
    assert [(cls == c).sum() for c in range(5)] == [CH - 1, CH, CH + 1, 0, 1]
    return inp, sg


@pytest.mark.parametrize("variant", VARIANTS)
def test_device_against_twin_chunk_edges(variant):
    inp, sg = edge_case(variant)
    check_case(inp, rows37(inp, 7)[:12], sg, "%s chunk edges" % variant)


@pytest.mark.parametrize("variant", VARIANTS)
def test_device_against_twin_every_source_wide(variant):
    inp = make_inputs(variant, 2 * CH + 40, seed=9, S=23, nf=2)
    sg = np.random.default_rng(3).uniform(0.0901, TOP, 2 * CH + 40)
    check_case(inp, rows37(inp, 5)[:12], sg, "%s all wide" % variant)


@pytest.mark.parametrize("variant", VARIANTS)
def test_bits(variant):
    """no source above the order's limit: the bits without the option; a row alone, in its batch of 37 and in a permuted batch of
    300, twice, and through the device entry: the same bits, value and gradient"""
    import torch
    from lumfuncmcmc_amd.capi import LFContext
    n = 1500
    inp = make_inputs(variant, n, seed=2, S=23)
    th = rows37(inp, 3)
    rng = np.random.default_rng(5)
    idx = rng.integers(0, 37, 300)
    idx[:37] = rng.permutation(37)
    ctx = LFContext(inp)
    try:
        narrow = np.minimum(mixed_sigma(n, 4), D.SIGMA_MAX)
        narrow[0] = D.SIGMA_MAX                                   # the limit itself stays with the order
        ctx.set_lum_err(narrow)
        off, goff = ctx.lnprob_err_grad(th)
        ctx.set_lum_err(narrow, wide=True)
        on, gon = ctx.lnprob_err_grad(th)
        assert np.array_equal(on, off) and np.array_equal(gon, goff, equal_nan=True)
        assert np.array_equal(ctx.lnprob_err_batch(th), off)
        sg = mixed_sigma(n, 4)
        ctx.set_lum_err(sg, 8, wide=True)
        e37, g37 = ctx.lnprob_err_grad(th)
        assert np.array_equal(ctx.lnprob_err_batch(th), e37)
        assert np.array_equal(ctx.lnprob_err_batch(th), e37)
        assert np.array_equal(ctx.lnprob_err_batch(th[idx]), e37[idx])
        assert np.array_equal(np.array([ctx.lnprob_err_batch(th[i:i + 1])[0] for i in range(37)]), e37)
        e300, g300 = ctx.lnprob_err_grad(th[idx])
        assert np.array_equal(e300, e37[idx]) and np.array_equal(g300, g37[idx], equal_nan=True)
        g1 = np.array([ctx.lnprob_err_grad(th[i:i + 1])[1][0] for i in range(37)])
        assert np.array_equal(g1, g37, equal_nan=True)
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            dev = ctx.lnprob_err_torch(torch.from_numpy(th).cuda())
            dval, dgrad = ctx.lnprob_err_grad_torch(torch.from_numpy(th).cuda())
        st.synchronize()
        assert np.array_equal(dev.cpu().numpy(), e37) and np.array_equal(dval.cpu().numpy(), e37)
        assert np.array_equal(dgrad.cpu().numpy(), g37, equal_nan=True)
        fin = np.isfinite(e37)
        assert fin.sum() >= 30 and np.any(e37[fin] != off[fin])
        # the unchecked order's sum of the same catalogue is another number
        ctx.set_lum_err(sg, 8, unchecked=True)
        assert np.all(ctx.lnprob_err_batch(th)[fin] != e37[fin])
    finally:
        ctx.close()


@pytest.mark.parametrize("variant", VARIANTS)
def test_deconv_tile(variant):
    """every source wide: "deconv_tile" changes no bit (the wide part runs per row either way); narrow and wide sources: the tile
    kernel's own rounding on the narrow part, twice the bound (tests/test_gpu_deconv_tile.py)"""
    from lumfuncmcmc_amd.capi import LFContext
    n = 900
    inp = make_inputs(variant, n, seed=13, S=23)
    th = rows37(inp, 4)
    ctx = LFContext(inp)
    try:
        for sg, exact in ((np.random.default_rng(8).uniform(0.0901, TOP, n), True), (mixed_sigma(n, 9), False)):
            ctx.set_lum_err(sg, wide=True)
            ctx.set_option("deconv_tile", 0)
            row = ctx.lnprob_err_batch(th)
            ctx.set_option("deconv_tile", 1)
            tile = ctx.lnprob_err_batch(th)
            ctx.set_option("deconv_tile", 0)
            fin = np.isfinite(row)
            assert np.array_equal(np.isneginf(tile), ~fin) and fin.sum() >= 30
            if exact or variant == "free":
                assert np.array_equal(tile, row)
            else:
                lp = ctx.lnprob_batch(th)
                _, _, sabs = D.delta(inp, sg, th, terms=True, wide=True)
                w2 = float((np.abs(tile[fin] - row[fin]) / (np.abs(lp[fin]) + sabs[fin])).max())
                print("deconv wide tile %s: max |tile - per-row| / (2 bound) = %.3e" % (variant, w2 / (2 * TOL)))
                assert w2 <= 2 * TOL
    finally:
        ctx.close()


def test_refusals():
    """the top edge is taken, the next double above it refused with the limit stated; without the option the order's refusal as it
    was; the context stays usable"""
    from lumfuncmcmc_amd.capi import LFContext, LFError
    inp = make_inputs("free", 300, seed=4, S=23)
    th = rows37(inp, 9)
    ctx = LFContext(inp)
    try:
        sg = np.full(300, 0.05)
        sg[17] = TOP
        ctx.set_lum_err(sg, wide=True)
        ok = ctx.lnprob_err_batch(th)
        sg[17] = np.nextafter(TOP, 1.0)
        with pytest.raises(LFError, match="error -1.*above 0.30 dex.*deconv_wide"):
            ctx.set_lum_err(sg, wide=True)
        with pytest.raises(LFError, match="error -1.*above 0.09 dex"):
            ctx.set_lum_err(sg)
        sg[17] = TOP
        ctx.set_lum_err(sg, wide=True)
        assert np.array_equal(ctx.lnprob_err_batch(th), ok)
        ctx.set_option("skip_grid", 1)
        with pytest.raises(LFError, match="error -1.*source-sharded"):
            ctx.lnprob_err_batch(th)
        ctx.set_option("skip_grid", 0)
        assert np.array_equal(ctx.lnprob_err_batch(th), ok)
    finally:
        ctx.close()


@pytest.fixture(scope="module")
def mock():
    """about 1000 sources with 0.15 dex of noise: every source is wide (class 1)"""
    o, theta, _ = L.noisy_mock(1000, 0.15, 11, deconvolve=True, deconvolve_wide=True, nsteps=200)
    yield o, theta
    o.close()


def test_model_map_fit(mock):
    o, theta = mock
    ctx = o.context()
    rows = o.get_init_walker_values(16)
    assert np.array_equal(o.lnprob_fix_comp(rows), ctx.lnprob_err_batch(rows))
    tw = D.lnprob_err(o.kernel_inputs(), np.array(o.lum_e), rows, wide=True)
    assert np.allclose(ctx.lnprob_err_batch(rows), tw, rtol=1e-10, atol=0.0)
    np.random.seed(4)
    info = o.fit_model_map(seed=3, likelihood="convolved")
    assert info["likelihood"] == "convolved" and info["converged"]
    assert o.map_lnprob == ctx.lnprob_err_batch(o.map_theta)[0]
    assert abs(o.map_theta[0] - theta[0]) < 0.3


def test_model_converged_fit_replays_on_the_host(mock):
    o, _ = mock
    np.random.seed(7)
    o.fit_model_converged(max_steps=100, check_every=50, likelihood="convolved")
    steps = o.chain.shape[1]
    assert o.sampler_likelihood == "convolved" and o.chain.shape == (32, steps, 3) and steps in (50, 100)
    ctx = o.context()
    chain, lnp, nacc = host_replay(ctx, o.start_pos, steps, o.sampler_seed, lnprob=ctx.lnprob_err_batch)
    np.testing.assert_array_equal(o.chain, chain)
    np.testing.assert_array_equal(o.sampler.lnprobability, lnp)
    np.testing.assert_array_equal(o.sampler.naccepted, nacc)
    assert 0 < nacc.sum() < 32 * steps
