"""The gradient of the cut's term on the device (csrc/lf_deconv_cut_grad.h, lf_cut_term_grad_batch, option "deconv_cut_grad";
DESIGN.md section 3.33) against its NumPy twin (deconv.cut_term_grad, lnprob_err_grad(cut=...), themselves checked against
30-digit differentiation in tests/test_deconv_cut_grad_cpu.py):

    |dev - twin| <= 1e-12 S_abs per element, S_abs the sum of the absolute values of the element's terms - the cut's nodes for
    lf_cut_term_grad_batch, the plain gradient's, Delta's and the cut's together for lf_lnprob_err_grad_batch,

an element without terms exactly 0, the values bit for bit those of the value entries, then the NaN pattern, batch independence,
the option, the model classes' MAP fit under the cut and the recovery of the truth from a mock of the cut process."""
import numpy as np
import pytest

import lf_cutlib as C
from lf_testlib import synth
from lumfuncmcmc_amd import deconv as D
from test_gpu_deconv_cut import K, LIMITS, TOL, context, rows, seeded_sigma

pytestmark = pytest.mark.gpu


def check(inp, model, limit, label, sg=None, wide=False):
    th = rows(inp, 9, seed=7)
    sg = seeded_sigma(len(inp["lum"]), 3) if sg is None else sg
    if wide:
        from lumfuncmcmc_amd.capi import LFContext
        ctx = LFContext(inp)
        ctx.set_option("deconv_cut_limit", limit)
        ctx.set_cut_error_model(*model)
        ctx.set_lum_err(sg, K, wide=True)
    else:
        ctx = context(inp, model, sg, limit)
    try:
        lp = ctx.lnprob_batch(th)
        fin = np.isfinite(lp)
        assert 4 <= fin.sum() < len(th)
        # lf_cut_term_grad_batch: Delta B and its gradient
        out, g = ctx.cut_term_grad(th)
        assert out.tobytes() == ctx.cut_term_batch(th).tobytes()
        tw, tg, ts = D.cut_term_grad(inp, *model, th, terms=True, limit=limit)
        assert np.array_equal(np.isnan(out), ~fin) and np.array_equal(np.isnan(g), np.repeat(~fin[:, None], g.shape[1], axis=1))
        has = ts[fin] > 0.0
        assert np.all(g[fin][~has] == 0.0) and has.any()
        r1 = (np.abs(g[fin] - tg[fin])[has] / ts[fin][has]).max()
        # lf_lnprob_err_grad_batch with the option: refused without it
        from lumfuncmcmc_amd.capi import LFError
        with pytest.raises(LFError, match="gradient of Delta B"):
            ctx.lnprob_err_grad(th)
        ctx.set_option("deconv_cut_grad", 1)
        val, gv = ctx.lnprob_err_grad(th)
        assert val.tobytes() == ctx.lnprob_err_batch(th).tobytes()
        rv, rg, rs = D.lnprob_err_grad(inp, sg, th, K=K, terms=True, wide=wide, cut=model, limit=limit)
        assert np.array_equal(np.isneginf(val), ~fin) and np.array_equal(np.isneginf(rv), ~fin) and not np.isnan(val).any()
        assert np.array_equal(np.isnan(gv), np.repeat(~fin[:, None], gv.shape[1], axis=1))
        assert np.array_equal(np.isnan(rg), np.isnan(gv))
        r2 = (np.abs(gv[fin] - rg[fin]) / rs[fin]).max()
        # the cut's part is in it: the same entry without the cut's nodes differs
        g0 = D.lnprob_err_grad(inp, sg, th, K=K, wide=wide)[1]
        assert np.any(np.abs(gv[fin] - g0[fin])[has] > 0.0)
        print("cut grad %-32s chunks %d: Delta B gradient %.3e, lnprob_err gradient %.3e of the bound"
              % (label, ctx.cut_info()["chunks"], r1 / TOL, r2 / TOL))
        assert r1 <= TOL and r2 <= TOL
    finally:
        ctx.close()


@pytest.mark.parametrize("limit", LIMITS)
@pytest.mark.parametrize("variant", ["free", "fixcomp", "zevol"])
def test_both_entries_against_twin_one_field(variant, limit):
    inp = C.cut_inputs(variant, n=200, S=5, nf=1)
    check(inp, C.flux_model(0.09), limit, "%s S=5 nf=1 limit %d" % (variant, limit))


@pytest.mark.parametrize("variant", ["free", "fixcomp", "zevol"])
def test_both_entries_against_twin_fixed_slope(variant):
    inp = C.cut_inputs(variant, n=200, S=5, nf=1, fix_sch_al=True)
    check(inp, C.flux_model(0.09), 0, "%s S=5 nf=1 fix_sch_al" % variant)


def five_field_model():
    nodes, sig = C.flux_model(0.06, nf=5)
    return nodes, np.minimum(sig * np.array([1.0, 0.5, 1.2, 0.8, 1.5])[:, None], D.CUT_SIGMA_MAX)


@pytest.mark.parametrize("variant", ["free", "fixcomp", "zevol"])
def test_both_entries_against_twin_five_fields(variant):
    """size_ln 101, five fields, one of them without sources, every field with its own errors: fields of several chunks, and
    the Flim_f elements take their field's chunks only"""
    inp = C.cut_inputs(variant, n=400, S=101, nf=5, empty_field=2)
    check(inp, five_field_model(), 0, "%s S=101 nf=5" % variant)


def test_with_the_wide_rule():
    inp = C.cut_inputs("free", n=200, S=5, nf=2)
    sg = seeded_sigma(200, 3)
    sg[::7] = 0.2                                    # above the order's limit: the wide rule's sources
    check(inp, C.flux_model(0.09, nf=2), 0, "free S=5 nf=2 deconv_wide", sg=sg, wide=True)


def test_zero_errors_launch_nothing():
    inp = C.cut_inputs("fixcomp", n=200, S=5, nf=2)
    sg = seeded_sigma(200, 3)
    th = rows(inp, 5, seed=7)
    ctx = context(inp, C.const_model(0.0, nf=2), sg)
    try:
        ctx.set_option("deconv_cut_grad", 1)
        assert ctx.cut_info()["chunks"] == 0
        fin = np.isfinite(ctx.lnprob_batch(th))
        out, g = ctx.cut_term_grad(th)
        assert np.all(out[fin] == 0.0) and np.all(g[fin] == 0.0) and np.isnan(g[~fin]).all() and (~fin).any()
        val, gv = ctx.lnprob_err_grad(th)
        rv, rg, rs = D.lnprob_err_grad(inp, sg, th, K=K, terms=True)
        assert val.tobytes() == ctx.lnprob_err_batch(th).tobytes()
        assert np.all(np.abs(gv[fin] - rg[fin]) <= TOL * rs[fin]) and np.isnan(gv[~fin]).all()
    finally:
        ctx.close()


@pytest.mark.parametrize("variant", ["fixcomp", "free"])
def test_batch_independence(variant):
    """a row's gradient has the same bits at B = 1, 37 and 300 (permuted), across two calls and through the device entry"""
    import torch
    if variant == "fixcomp":
        inp, model = C.cut_inputs("fixcomp", n=300, S=23, nf=5), C.flux_model(0.09, nf=5)
    else:
        inp, model = C.cut_inputs("free", n=300, S=23, nf=2), C.flux_model(0.09, nf=2)
    sg = seeded_sigma(300, 5)
    th = rows(inp, 300, seed=9)
    ctx = context(inp, model, sg)
    try:
        ctx.set_option("deconv_cut_grad", 1)
        same = lambda a, b: a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()      # noqa: E731
        perm = np.random.default_rng(1).permutation(300)
        for fn in (ctx.lnprob_err_grad, ctx.cut_term_grad):
            full = fn(th)
            assert np.isfinite(full[1]).all(axis=1).sum() > 100
            assert same(fn(th), full)
            p = fn(th[perm])
            assert same(p, (full[0][perm], full[1][perm]))
            assert same(fn(th[:37]), (full[0][:37], full[1][:37]))
            for r in (0, 5, 299):
                assert same(fn(th[r:r + 1]), (full[0][r:r + 1], full[1][r:r + 1]))
        full = ctx.lnprob_err_grad(th)
        v, g = ctx.lnprob_err_grad_torch(torch.from_numpy(th).cuda())
        assert same((v.cpu().numpy(), g.cpu().numpy()), full)
        assert full[0].tobytes() == ctx.lnprob_err_batch(th).tobytes()
    finally:
        ctx.close()


def test_the_option():
    import torch
    from lumfuncmcmc_amd.capi import LFContext, LFError
    from lf_testlib import make_inputs
    inp = C.cut_inputs("fixcomp", n=100, S=5, nf=2)
    model = C.flux_model(0.09, nf=2)
    sg = np.full(100, 0.03)
    th = rows(inp, 3, seed=7)
    ctx = context(inp, model, sg)
    try:
        with pytest.raises(LFError, match=r"lf_lnprob_err_grad_batch: not under a cut on the observed flux \(lf_set_cut_error_model\): "
                                          "the gradient of Delta B, the cut's change of the expected counts, is not provided"):
            ctx.lnprob_err_grad(th)
        with pytest.raises(LFError, match="lf_lnprob_err_grad_batch_device: .*gradient of Delta B"):
            ctx.lnprob_err_grad_torch(torch.from_numpy(th).cuda())
        before = ctx.lnprob_err_batch(th)
        assert np.isfinite(before).any()                              # (the context stays usable)
        dB, gB = ctx.cut_term_grad(th)                                # served whatever the option says
        assert np.isfinite(gB).any()
        ctx.set_option("deconv_cut_grad", 1)
        val, g = ctx.lnprob_err_grad(th)
        assert val.tobytes() == before.tobytes() and np.isfinite(g).any()
        ctx.set_option("deconv_cut_grad", 0)
        with pytest.raises(LFError, match="gradient of Delta B"):
            ctx.lnprob_err_grad(th)
        ctx.set_option("deconv_cut_grad", 7)                          # a flag: any value but 0
        again = ctx.lnprob_err_grad(th)
        assert again[1].tobytes() == g.tobytes()
    finally:
        ctx.close()
    # a context without a cut model: the option does nothing
    inp = make_inputs("fixcomp", 100, S=5, nf=2)
    ctx = LFContext(inp)
    try:
        ctx.set_lum_err(sg, K)
        off = ctx.lnprob_err_grad(th)
        ctx.set_option("deconv_cut_grad", 1)
        on = ctx.lnprob_err_grad(th)
        assert on[0].tobytes() == off[0].tobytes() and on[1].tobytes() == off[1].tobytes()
        with pytest.raises(LFError, match="no cut model set"):
            ctx.cut_term_grad(th)
    finally:
        ctx.close()


@pytest.mark.parametrize("kind", ["fixcomp", "free", "zevol"])
def test_the_classes_fit_the_maximum_under_the_cut(kind):
    from test_gpu_model_deconv_cut import model
    o = model(kind, deconvolve_cut_grad=True)
    try:
        ctx = o.context()
        assert ctx.cut_info()["chunks"] > 0
        info = o.fit_model_map(nstarts=4, seed=3, likelihood="convolved")
        assert info["converged"] and o.map_info["likelihood"] == "convolved"
        th = o.map_theta
        assert o.map_lnprob == ctx.lnprob_err_batch(th[None])[0]
        # the maximum, independently of the gradient: no step of a tenth of a sigma along a free coordinate goes up
        free = np.flatnonzero(~info["on_bound"])
        sd = np.sqrt(np.diag(o.map_cov))
        probe = np.repeat(th[None], 2 * free.size, axis=0)
        for i, e in enumerate(free):
            probe[2 * i, e] += 0.1 * sd[e]
            probe[2 * i + 1, e] -= 0.1 * sd[e]
        around = ctx.lnprob_err_batch(probe)
        print("MAP %s: lnprob %.6f after %d iterations, on_bound %s; largest lnprob a tenth of a sigma away %+.3e below"
              % (kind, o.map_lnprob, info["niter"], info["on_bound"].astype(int), o.map_lnprob - around.max()))
        assert free.size > 0 and np.all(sd[free] > 0.0) and np.all(around <= o.map_lnprob)
        np.random.seed(4)
        pos = o.map_init_walkers(likelihood="convolved")
        assert pos.shape == (o.nwalkers, ctx.ndim) and np.isfinite(ctx.lnprob_err_batch(pos)).all()
        np.random.seed(12)
        o.fit_model_converged(max_steps=20, check_every=10, start="map", likelihood="convolved")
        assert o.sampler_likelihood == "convolved" and o.chain.shape == (o.nwalkers, 20, ctx.ndim)
    finally:
        o.close()


RECOVERY_SEED = 8


def test_recovery_of_the_truth_from_a_mock_of_the_cut_process():
    """One seeded mock catalogue of the cut process of the fixed-completeness class (about 3000 kept sources), refitted under the
    cut: every free coordinate of the maximum lies within 4 sqrt(cov_ii) of the truth (DESIGN.md section 3.33 has the offsets)."""
    from lf_deconvlib import fixcomp_model
    kw = dict(deconvolve=True, min_comp_frac=0.5, deconvolve_cut=True, deconvolve_cut_grad=True, deconvolve_order=12,
              Flim=[synth.FLIM[0]] * 5)
    base = fixcomp_model(synth.catalogue(400, seed=17), **kw)
    try:
        theta0 = np.array([synth.LSTAR, synth.PHISTAR, synth.SCH_AL])
        probe = base.mock_catalogue(theta0, seed=1, cut=True)
        theta0[1] += np.log10(3000.0 / probe["field_ind"][-1])
        mc = base.mock_catalogue(theta0, seed=RECOVERY_SEED, cut=True)
        errors = base.deconvolve_cut_errors
    finally:
        base.close()
    n = int(mc["field_ind"][-1])
    assert 2500 < n < 3500, n
    o = fixcomp_model(mc, deconvolve_cut_errors=errors, **kw)
    try:
        info = o.fit_model_map(nstarts=4, seed=3, likelihood="convolved")
        assert info["converged"]
        free = ~info["on_bound"]
        off = (o.map_theta - theta0)[free] / np.sqrt(np.diag(o.map_cov))[free]
        print("recovery: %d sources, MAP %s, truth %s, offsets in sigma %s" % (n, np.round(o.map_theta, 4), np.round(theta0, 4),
                                                                              np.round(off, 2)))
        assert free.all() and np.all(np.abs(off) <= 4.0)
    finally:
        o.close()
