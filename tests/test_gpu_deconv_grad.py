"""The gradient of the flux-error-convolved likelihood on the device (csrc/lf_deconv_grad.h, lf_lnprob_err_grad_batch; DESIGN.md
section 3.19) against its NumPy twin (lumfuncmcmc_amd/deconv.py: lnprob_err_grad, itself checked against 30-digit
differentiation in tests/test_deconv_grad_cpu.py):

    |grad_dev - grad_twin| <= 1e-12 S_abs   element-wise,   NaN pattern identical,   value bit-identical to lnprob_err_batch,

S_abs being the sum of the absolute values of all contributions to the element (the plain gradient's and the correction's);
then batch independence, the device form on a stream, the refusals, the options and the MAP fit of the model classes."""
import os

import numpy as np
import pytest

import lf_deconvlib as L
from lf_testlib import O, make_inputs, synth
from lumfuncmcmc_amd import deconv as D
from lumfuncmcmc_amd import mapfit

pytestmark = pytest.mark.gpu
TOL = 1e-12
ORDERS = (4, 32)
GOLDENS = [("free_n50", "free"), ("free_n1000", "free"), ("fixcomp_n50", "fixcomp"), ("zevol_n800", "zevol")]
CH = D.CHUNK
FIELDS = {1: [(n,) for n in (1, CH - 1, CH, CH + 1)], 5: [(1, CH - 1, CH, CH + 1, 7)]}
EDGE_ROWS = [0, 1, 2, 3, 4, 5, 11, 20, 21, 22, 23, 24]      # of rows37: the three that are not finite among them


def seeded_sigma(n, seed):
    """sigma uniform in [0, 0.09] dex, a tenth of the sources at exactly 0"""
    rng = np.random.default_rng(seed)
    sg = rng.uniform(0.0, 0.09, n)
    sg[rng.permutation(n)[:max(1, n // 10)]] = 0.0
    return sg


def rows37(inp, seed):
    """37 theta rows: prior-box draws (synth.walkers), two rows outside the box, one underflowing row."""
    nf = len(inp["field_ind"]) - 1
    th = synth.walkers(inp["variant"], 37, seed=seed, fix_sch_al=bool(inp["fix_sch_al"]), nf=nf)
    th[3, 0] = 39.5                      # outside the box (L* below 40)
    th[11, 1] = 5.5                      # outside the box (phi* above 5)
    th[20, 0] = 40.001                   # inside, but exp(-10^(lum - L*)) underflows for the bright sources
    if inp["variant"] == "zevol":
        th[20, 0:3] = 40.001
    return th


def twin_case(inp, th, sg, K, label):
    """the twin's (value, grad, S_abs), with what the cases are chosen for: finite gradients on every finite row, and the
    outside and underflowing rows not finite"""
    val, g, s = D.lnprob_err_grad(inp, sg, th, K=K, terms=True)
    fin = np.isfinite(val)
    assert np.all(np.isfinite(g[fin])) and np.all(np.isfinite(s[fin])), "%s: the twin's gradient of a finite row is not finite" % label
    assert np.isnan(g[~fin]).all()
    assert len(inp["lum"]) < 50 or (~fin).sum() >= 3, "%s: the outside and underflowing rows are not -inf" % label
    return val, g, s


def check_case(inp, th, label, seed=1):
    from lumfuncmcmc_amd.capi import LFContext
    sg = seeded_sigma(len(inp["lum"]), seed)
    ctx = LFContext(inp)
    worst = 0.0
    try:
        for K in ORDERS:
            ctx.set_lum_err(sg, K, unchecked=True)
            val_d, g_d = ctx.lnprob_err_grad(th)
            assert np.array_equal(val_d, ctx.lnprob_err_batch(th)), "%s K=%d: the value differs from lnprob_err_batch" % (label, K)
            val_t, g_t, s_t = twin_case(inp, th, sg, K, label)
            fin = np.isfinite(val_d)
            assert np.array_equal(fin, np.isfinite(val_t)) and np.all(val_d[~fin] == -np.inf), "%s K=%d: -inf pattern" % (label, K)
            assert np.array_equal(np.isnan(g_d), np.isnan(g_t)), "%s K=%d: NaN pattern" % (label, K)
            assert np.array_equal(np.isnan(g_d).all(axis=1), ~fin) and np.all(np.isfinite(g_d[fin])), "%s K=%d: NaN rows" % (label, K)
            err, scale = np.abs(g_d[fin] - g_t[fin]), s_t[fin]
            assert np.all(err[scale == 0.0] == 0.0), "%s K=%d: an element without contributions is not 0" % (label, K)
            ratio = np.where(scale > 0.0, err / np.where(scale > 0.0, scale, 1.0), 0.0)
            w = float(np.max(ratio)) if ratio.size else 0.0
            print("deconv grad %-34s K=%2d rows %2d finite, max |dev - twin| / S_abs = %.3e" % (label, K, int(fin.sum()), w))
            assert w <= TOL, (label, K, w, np.unravel_index(np.argmax(ratio), ratio.shape))
            worst = max(worst, w)
    finally:
        ctx.close()
    return worst


@pytest.mark.parametrize("name,variant", GOLDENS)
def test_device_against_twin_goldens(golden_dir, name, variant):
    inp = O.inputs_from_golden(np.load(os.path.join(golden_dir, name + ".npz")), variant)
    check_case(inp, rows37(inp, 11), name)


def edge_inputs(variant, nf, sizes, fsa):
    inp = make_inputs(variant, int(sum(sizes)), seed=5 + sizes[0], S=23, fix_sch_al=fsa, nf=nf)
    inp["field_ind"] = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return inp


@pytest.mark.parametrize("fsa", [False, True])
@pytest.mark.parametrize("variant", ["free", "fixcomp", "zevol"])
@pytest.mark.parametrize("nf", [1, 5])
def test_device_against_twin_chunk_edges(variant, nf, fsa):
    """1, chunk - 1, chunk and chunk + 1 sources in a field, in one field and in five, the slope free and fixed"""
    for sizes in FIELDS[nf]:
        inp = edge_inputs(variant, nf, sizes, fsa)
        check_case(inp, rows37(inp, 7)[EDGE_ROWS], "%s nf=%d fsa=%d sizes=%s" % (variant, nf, fsa, sizes), seed=sizes[0])


@pytest.mark.parametrize("variant", ["free", "fixcomp", "zevol"])
def test_bits(variant):
    """the value is lnprob_err_batch's, bit for bit, -inf rows stay -inf with NaN gradients; all sigma 0: the plain gradient's
    bits; a row alone, in its batch of 37 and in a permuted batch of 300, twice, and through the device entry point on a
    stream of its own: the same bits"""
    import torch
    from lumfuncmcmc_amd.capi import LFContext
    inp = make_inputs(variant, 4500, seed=2, S=23)
    th = rows37(inp, 3)
    rng = np.random.default_rng(5)
    idx = rng.integers(0, 37, 300)
    idx[:37] = rng.permutation(37)
    ctx = LFContext(inp)
    try:
        lp, gp = ctx.lnprob_grad(th)
        ctx.set_lum_err(np.zeros(4500))
        v0, g0 = ctx.lnprob_err_grad(th)
        assert np.array_equal(v0, lp) and np.array_equal(g0, gp, equal_nan=True)
        ctx.set_lum_err(seeded_sigma(4500, 4), 8, unchecked=True)
        e37 = ctx.lnprob_err_batch(th)
        v37, g37 = ctx.lnprob_err_grad(th)
        fin = np.isfinite(e37)
        assert np.array_equal(v37, e37) and np.all(v37[~fin] == -np.inf) and (~fin).sum() >= 3
        assert np.isnan(g37[~fin]).all() and np.isfinite(g37[fin]).all() and np.any(g37[fin] != gp[fin])
        again = ctx.lnprob_err_grad(th)
        assert np.array_equal(again[0], v37) and np.array_equal(again[1], g37, equal_nan=True)
        v300, g300 = ctx.lnprob_err_grad(th[idx])
        assert np.array_equal(v300, v37[idx]) and np.array_equal(g300, g37[idx], equal_nan=True)
        g1 = np.array([ctx.lnprob_err_grad(th[i:i + 1])[1][0] for i in range(37)])
        assert np.array_equal(g1, g37, equal_nan=True)
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            vd, gd = ctx.lnprob_err_grad_torch(torch.from_numpy(th).cuda())
        st.synchronize()
        assert np.array_equal(vd.cpu().numpy(), v37) and np.array_equal(gd.cpu().numpy(), g37, equal_nan=True)
    finally:
        ctx.close()


def test_refusals_and_options():
    """LF_ERR_ARG with a message, nothing launched, and the next correct call has the bits it had before; compress (ignored by
    the gradient: the value is lnprob_err_batch's under the same option, which takes its plain part from the compressed
    catalogue) and the kernels behind lnprob (persistent 0 / 2) do not change the gradient's bits"""
    from lumfuncmcmc_amd.capi import LFContext, LFError
    for variant in ("free", "zevol"):
        inp = make_inputs(variant, 4500, seed=4, S=23)
        th = rows37(inp, 9)
        ctx = LFContext(inp)
        try:
            with pytest.raises(LFError, match="error -1.*no luminosity errors set"):
                ctx.lnprob_err_grad(th)
            ctx.set_lum_err(seeded_sigma(4500, 6))
            v0, g0 = ctx.lnprob_err_grad(th)
            same = lambda r: np.array_equal(r[0], v0) and np.array_equal(r[1], g0, equal_nan=True)      # noqa: E731
            ctx.set_option("skip_grid", 1)
            with pytest.raises(LFError, match="error -1.*source-sharded"):
                ctx.lnprob_err_grad(th)
            ctx.set_option("skip_grid", 0)
            assert same(ctx.lnprob_err_grad(th))
            for key, val in (("compress", 1), ("compress", 0), ("persistent", 0), ("persistent", 2), ("persistent", 1)):
                ctx.set_option(key, val)
                v, g = ctx.lnprob_err_grad(th)
                assert np.array_equal(g, g0, equal_nan=True), (variant, key, val)
                assert np.array_equal(v, ctx.lnprob_err_batch(th)), (variant, key, val)
            ctx.set_option("grid_share", 1 + 65536 * 2)
            with pytest.raises(LFError, match="error -1.*source-sharded"):
                ctx.lnprob_err_grad(th)
            ctx.set_option("grid_share", 0)
            assert same(ctx.lnprob_err_grad(th)), (variant, "grid_share")
        finally:
            ctx.close()


def test_model_map_fit_under_deconvolve():
    """a mock of about 3000 sources with 0.09 dex of noise at fixed completeness: the convolved maximum, its covariance and
    Laplace evidence from fit_model_map(likelihood="convolved"); the plain maximum of the same object has the larger L*"""
    tol = 1e-6
    np.random.seed(3)
    o, truth, _ = L.noisy_mock(3000, 0.09, seed=3, deconvolve=True)
    try:
        r = dict(o.fit_model_map(nstarts=8, seed=1, tol=tol, likelihood="convolved"))
        assert r["converged"] and r["likelihood"] == "convolved", r
        inp, sigma = o.kernel_inputs(), np.array(o.lum_e)
        free = ~r["on_bound"]
        twin = lambda t: D.lnprob_err_grad(inp, sigma, t, K=o.deconvolve_order)      # noqa: E731
        _, g = twin(r["theta"])
        dec = mapfit.newton_decrement(g, mapfit.hessian(twin, r["theta"], r["box"]), free)
        print("MAP convolved: lnprob %.4f niter %d decrement (twin) %.3e on_bound %s lnZ_laplace %.4f %s"
              % (r["lnprob"], r["niter"], dec, r["on_bound"].tolist(), o.lnZ_laplace, r["lnZ_reason"]))
        assert dec <= 2 * tol
        assert np.allclose(o.map_cov, o.map_cov.T, rtol=1e-9, atol=0) and np.linalg.eigvalsh(0.5 * (o.map_cov + o.map_cov.T))[0] > 0
        assert np.isfinite(o.lnZ_laplace)
        assert o.map_lnprob >= o.lnprob_fix_comp(truth)
        pos = o.map_init_walkers(64, likelihood="convolved")
        assert pos.shape == (64, 3) and np.all(np.isfinite(o.lnprob_fix_comp(pos)))
        p = o.fit_model_map(nstarts=8, seed=1, tol=tol, likelihood="plain")
        print("    convolved %s\n    plain     %s\n    truth     %s" % (np.round(r["theta"], 4), np.round(p["theta"], 4), np.round(truth, 4)))
        assert p["converged"] and p["likelihood"] == "plain" and o.map_info["likelihood"] == "plain"
        assert p["theta"][0] > r["theta"][0]
        assert p["lnprob"] == o.context().lnprob_batch(p["theta"])[0]
    finally:
        o.close()
