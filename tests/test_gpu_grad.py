"""The device gradient of lnprob (csrc/lf_grad.h, lf_lnprob_grad_batch) against its NumPy twin
(lumfuncmcmc_amd/grad.py, itself checked against 40-digit differentiation in tests/test_grad_cpu.py):

    |grad_dev - grad_twin| <= 1e-12 S_abs   element-wise,   NaN pattern identical,   lnprob bit-identical to lnprob_batch,

S_abs being the sum of the absolute values of all per-source and per-lattice-point contributions to the element; then batch
independence, the options, the device form, and the MAP fit of the model classes on top of it."""
import os

import numpy as np
import pytest

from lf_testlib import O, make_inputs, synth
from lumfuncmcmc_amd import grad as G
from lumfuncmcmc_amd import mapfit

pytestmark = pytest.mark.gpu
TOL = 1e-12
GOLDENS = [("free_n50", "free"), ("free_n1000", "free"), ("free_n1000_fsa", "free"), ("free_n300_mcf50", "free"),
           ("fixcomp_n50", "fixcomp"), ("fixcomp_n1000_fsa", "fixcomp"), ("zevol_n800", "zevol"), ("zevol_n1000_fsa", "zevol")]
SYNTH = [(v, n, nf) for v in ("free", "fixcomp", "zevol") for n in (1, 63, 257, 4500) for nf in ((1, 8) if v == "free" else (5,))]


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


def compare(lp_d, g_d, lp_b, g_t, s_t, label):
    """the device's (lnprob, gradient) of one call against lnprob_batch's value of the same rows (lp_b) and the twin's gradient
    and scale (g_t, s_t); returns the largest |dev - twin| / S_abs"""
    assert np.array_equal(lp_d, lp_b), "%s: lnprob of the gradient call differs from lnprob_batch" % label
    fin = np.isfinite(lp_b)
    assert np.array_equal(np.isnan(g_d), np.isnan(g_t)), "%s: NaN pattern" % label
    assert np.array_equal(np.isnan(g_d).all(axis=1), ~fin) and not np.isnan(g_d[fin]).any(), "%s: NaN rows" % label
    assert np.all(np.isfinite(g_d[fin])), "%s: a finite row with a non-finite gradient" % label
    err, scale = np.abs(g_d[fin] - g_t[fin]), s_t[fin]
    # (an element nothing contributes to - the Flim of a field without sources on a lattice of zero width - is exactly 0)
    assert np.all(err[scale == 0.0] == 0.0), "%s: an element without contributions is not 0" % label
    ratio = np.where(scale > 0.0, err / np.where(scale > 0.0, scale, 1.0), 0.0)
    worst = float(np.max(ratio)) if ratio.size else 0.0
    print("grad %-28s rows %2d finite, max |dev - twin| / S_abs = %.3e" % (label, int(fin.sum()), worst))
    assert worst <= TOL, (label, worst, np.unravel_index(np.argmax(ratio), ratio.shape))
    return worst


def check_case(inp, seed, label):
    from lumfuncmcmc_amd.capi import LFContext
    th = rows37(inp, seed)
    lp_t, g_t, s_t = G.lnprob_grad(inp, th, terms=True)
    ctx = LFContext(inp)
    try:
        lp_d, g_d = ctx.lnprob_grad(th)
        lp_b = ctx.lnprob_batch(th)
    finally:
        ctx.close()
    assert len(inp["lum"]) < 60 or (~np.isfinite(lp_b)).sum() >= 3, "%s: the outside and underflowing rows are not -inf" % label
    return compare(lp_d, g_d, lp_b, g_t, s_t, label)


@pytest.mark.parametrize("name,variant", GOLDENS)
def test_device_against_twin_goldens(golden_dir, name, variant):
    inp = O.inputs_from_golden(np.load(os.path.join(golden_dir, name + ".npz")), variant)
    check_case(inp, 11, name)


@pytest.mark.parametrize("variant,n,nf", SYNTH)
def test_device_against_twin_sizes(variant, n, nf):
    """wave and chunk edges (1, 63, 257 sources; 4500 = several blocks of 1024 per field), one field and eight"""
    for fsa in (False, True):
        inp = make_inputs(variant, n, seed=5 + n, S=23, fix_sch_al=fsa, nf=nf)
        check_case(inp, 7 + n, "%s n=%d nf=%d fsa=%d" % (variant, n, nf, fsa))


@pytest.mark.parametrize("variant", ["free", "fixcomp", "zevol"])
def test_batch_independence(variant):
    """a row alone, in its batch of 37 and in a permuted batch of 300: the same bits"""
    from lumfuncmcmc_amd.capi import LFContext
    inp = make_inputs(variant, 4500, seed=2, S=23)
    th = rows37(inp, 3)
    rng = np.random.default_rng(5)
    idx = rng.integers(0, 37, 300)
    idx[:37] = rng.permutation(37)
    ctx = LFContext(inp)
    try:
        _, g37 = ctx.lnprob_grad(th)
        _, g300 = ctx.lnprob_grad(th[idx])
        g1 = np.array([ctx.lnprob_grad(th[i:i + 1])[1][0] for i in range(37)])
    finally:
        ctx.close()
    assert np.array_equal(g37, g1, equal_nan=True)
    assert np.array_equal(g300, g37[idx], equal_nan=True)


def test_options():
    """compress is ignored; the kernels behind lnprob (persistent 0 / 2, fuse 0) do not change gradient bits; a context
    with skip_grid set refuses with LF_ERR_ARG and stays usable"""
    from lumfuncmcmc_amd.capi import LFContext, LFError
    for variant in ("free", "zevol"):
        inp = make_inputs(variant, 4500, seed=4, S=23)
        th = rows37(inp, 9)
        ctx = LFContext(inp)
        try:
            lp0, g0 = ctx.lnprob_grad(th)
            for key, val in (("compress", 1), ("compress", 0), ("persistent", 0), ("persistent", 2), ("persistent", 1), ("fuse", 0)):
                ctx.set_option(key, val)
                _, g = ctx.lnprob_grad(th)
                assert np.array_equal(g, g0, equal_nan=True), (variant, key, val)
            ctx.set_option("fuse", 1)
            ctx.set_option("skip_grid", 1)
            with pytest.raises(LFError, match="error -1"):
                ctx.lnprob_grad(th)
            ctx.set_option("skip_grid", 0)
            lp1, g1 = ctx.lnprob_grad(th)
            assert np.array_equal(g1, g0, equal_nan=True) and np.array_equal(lp1, lp0)
            ctx.set_option("grid_share", 1 + 65536 * 2)
            with pytest.raises(LFError, match="error -1"):
                ctx.lnprob_grad(th)
        finally:
            ctx.close()


def test_device_form_on_a_stream():
    import torch
    from lumfuncmcmc_amd.capi import LFContext
    inp = make_inputs("free", 4500, seed=6, S=23)
    th = rows37(inp, 13)
    ctx = LFContext(inp)
    try:
        lp_h, g_h = ctx.lnprob_grad(th)
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            lp_d, g_d = ctx.lnprob_grad_torch(torch.from_numpy(th).cuda())
        st.synchronize()
        assert np.array_equal(lp_d.cpu().numpy(), lp_h)
        assert np.array_equal(g_d.cpu().numpy(), g_h, equal_nan=True)
    finally:
        ctx.close()


def _model(variant, n=2000, cat=None):
    from lumfuncmcmc_amd.model import LumFuncMCMC, LumFuncMCMCz
    cat = synth.catalogue(n, seed=17) if cat is None else cat
    fi = cat["field_ind"]
    kw = dict(lum=synth.split_fields(cat["lum"], fi), lum_e=synth.split_fields(cat["lum_e"], fi), Flim=list(synth.FLIM),
              alpha=synth.ALPHA_C, Omega_0=list(synth.OMEGA_0), sch_al=synth.SCH_AL, sch_al_lims=synth.SCH_AL_LIMS,
              Lstar=synth.LSTAR, Lstar_lims=synth.LSTAR_LIMS, phistar=synth.PHISTAR, phistar_lims=synth.PHISTAR_LIMS,
              Lc=synth.LC, Lh=synth.LH, nwalkers=32, nsteps=100, field_ind=fi)
    zs = synth.split_fields(cat["z"], fi)
    if variant == "zevol":
        return LumFuncMCMCz(zs, **kw)
    return LumFuncMCMC(zs, Flim_lims=synth.FLIM_LIMS, alpha_lims=synth.ALPHA_LIMS, **kw)


def _mock_model(variant, n=2000):
    """A model object over a catalogue of about n sources DRAWN FROM THE MODEL (mock.py's NumPy twin) at known parameters,
    so that the posterior's maximum lies inside the prior box; returns (object, truth)."""
    base = _model(variant, n)
    if variant == "zevol":
        theta = np.array([42.6, 42.5, 42.4, -2.1, -2.0, -1.9, synth.SCH_AL])
        amp = slice(3, 6)
    else:
        # (a completeness curve that rises over a decade in flux, alpha_C = 2.5: 2000 sources then bound the slope from
        # both sides - with the instrument's sharp 4.56 too few of them sit on the rise, and the posterior stays open
        # towards steep slopes up to the prior's edge, where there is no Laplace evidence)
        theta = np.array([synth.LSTAR, synth.PHISTAR, synth.SCH_AL] + list(synth.FLIM) + [2.5])
        amp = slice(1, 2)
    m0 = base._mock_generator(False).counts(theta[None], 0)[0].sum()
    theta[amp] += np.log10(n / m0)
    mc = base.mock_catalogue(theta, seed=99, device=False)
    base.close()
    return _model(variant, cat={"z": np.concatenate(mc["z"]), "lum": np.concatenate(mc["lum"]),
                                "lum_e": np.concatenate(mc["lum_e"]) + 0.05, "field_ind": np.asarray(mc["field_ind"])}), theta


@pytest.mark.parametrize("variant", ["free", "zevol"])
def test_model_map_fit(variant):
    """fit_model_map on a synthetic catalogue of about 2000 sources drawn from the model (FREE: S = 101), then walkers around
    the maximum and a chain started there"""
    tol = 1e-6
    np.random.seed(3)
    o, truth = _mock_model(variant)
    try:
        r = o.fit_model_map(nstarts=16, seed=1, tol=tol)
        assert r["converged"], r
        inp = o.kernel_inputs()
        box = o._theta_lims()
        free = ~r["on_bound"]
        # the decrement again, with the twin's gradient at the device's maximum and the twin's Hessian
        twin = lambda t: G.lnprob_grad(inp, t)      # noqa: E731
        _, g = twin(r["theta"])
        dec = mapfit.newton_decrement(g, mapfit.hessian(twin, r["theta"], o.map_info["box"]), free)
        print("MAP %s: lnprob %.4f niter %d decrement (twin) %.3e on_bound %s lnZ_laplace %.4f %s"
              % (variant, r["lnprob"], r["niter"], dec, r["on_bound"].tolist(), o.lnZ_laplace, r["lnZ_reason"]))
        print("    theta %s\n    truth %s\n    sd    %s" % (np.round(r["theta"], 4), np.round(truth, 4), np.round(np.sqrt(np.diag(o.map_cov)), 4)))
        assert dec <= 2 * tol
        assert np.allclose(o.map_cov, o.map_cov.T, rtol=1e-9, atol=0) and np.linalg.eigvalsh(0.5 * (o.map_cov + o.map_cov.T))[0] > 0
        assert np.isfinite(o.lnZ_laplace)
        assert r["lnprob"] >= o.lnprob(truth)
        pos = o.map_init_walkers(64)
        assert pos.shape == (64, len(box)) and np.all(np.isfinite(o.lnprob(pos)))
        o.fit_model_converged(max_steps=200, check_every=100, start="map")
        assert o.chain.shape == (32, 200, len(box)) and np.all(np.isfinite(o.sampler.lnprobability))
    finally:
        o.close()
