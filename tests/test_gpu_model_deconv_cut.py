"""The model classes at the default min_comp_frac = 0.5 with deconvolve=True, deconvolve_cut=True:
fit_model, fit_model_converged(likelihood="convolved") and fit_model_pt(likelihood="convolved") run a few steps on the
fixed-completeness, the free-completeness and the z-evolving class, with the default error model read off the catalogue; every
chain's stored value is what the context's convolved entry, Delta B included, gives for the stored position."""
import numpy as np
import pytest

from lumfuncmcmc_amd import synth

pytestmark = pytest.mark.gpu
N = 400


def model(kind, **extra):
    from lumfuncmcmc_amd.model import LumFuncMCMC, LumFuncMCMCz
    cat = synth.catalogue(N, seed=21)
    fi = cat["field_ind"]
    # the synthetic catalogue's errors (0.05 dex) with a fifth of the sources at half of it: the default error model has structure
    lum_e = cat["lum_e"].copy()
    lum_e[::5] = 0.025
    kw = dict(lum=synth.split_fields(cat["lum"], fi), lum_e=synth.split_fields(lum_e, fi), Flim=list(synth.FLIM),
              alpha=synth.ALPHA_C, Omega_0=list(synth.OMEGA_0), sch_al=synth.SCH_AL, Lc=synth.LC, Lh=synth.LH, nwalkers=20,
              nsteps=20, min_comp_frac=0.5, field_ind=fi, deconvolve=True, deconvolve_cut=True, deconvolve_order=12)
    kw.update(extra)
    zs = synth.split_fields(cat["z"], fi)
    np.random.seed(5)
    if kind == "zevol":
        return LumFuncMCMCz(zs, **kw)
    return LumFuncMCMC(zs, fix_comp=(kind == "fixcomp"), Flim_lims=synth.FLIM_LIMS, alpha_lims=synth.ALPHA_LIMS,
                       Lstar=synth.LSTAR, Lstar_lims=synth.LSTAR_LIMS, phistar=synth.PHISTAR, phistar_lims=synth.PHISTAR_LIMS,
                       sch_al_lims=synth.SCH_AL_LIMS, **kw)


def check_values(ctx, pos, stored):
    """stored lnprob == lf_lnprob_err_batch of the positions, bit for bit; and the cut term is in it"""
    pos = pos.reshape(-1, pos.shape[-1])
    got = ctx.lnprob_err_batch(pos)
    np.testing.assert_array_equal(got, stored.reshape(-1))
    fin = np.isfinite(got)
    assert fin.any()
    dB = ctx.cut_term_batch(pos[fin][:4])
    assert np.all(np.isfinite(dB)) and np.all(dB != 0.0)


@pytest.mark.parametrize("kind", ["fixcomp", "free", "zevol"])
def test_the_three_fits_run_at_the_default_min_comp_frac(kind):
    o = model(kind)
    try:
        nodes, sig = o.deconvolve_cut_errors
        assert sig.shape == (o.nfields, nodes.size) and nodes.size > 1 and np.all(sig > 0.0)
        ctx = o.context()
        info = ctx.cut_info()
        assert info["chunks"] > 0 and np.all(info["nnodes"] > 0)
        ndim = ctx.ndim
        # fit_model: the batched host sampler on the convolved value
        np.random.seed(11)
        o.fit_model()
        assert o.samples.shape[1] == ndim + 1 and np.all(np.isfinite(o.samples))
        check_values(ctx, o.samples[:8, :ndim], o.samples[:8, ndim])
        # fit_model_converged: the device sampler on the convolved likelihood
        np.random.seed(12)
        o.fit_model_converged(max_steps=20, check_every=10, likelihood="convolved")
        assert o.sampler_likelihood == "convolved" and o.chain.shape == (20, 20, ndim)
        check_values(ctx, o.chain[:, -1], o.sampler.lnprobability[:, -1])
        # fit_model_pt: the tempered device sampler; the beta = 1 chain's lnlike is the convolved likelihood of its positions
        np.random.seed(13)
        lnZ, dlnZ = o.fit_model_pt(ntemps=3, likelihood="convolved")
        assert np.isfinite(lnZ) and o.pt_sampler.likelihood == "convolved"
        check_values(ctx, o.pt_sampler.chain[0][:, -1], o.pt_sampler.lnlikelihood[0][:, -1])
    finally:
        o.close()


def test_the_caller_may_pass_an_error_model_below_the_cut():
    nodes = np.array([-17.6, -17.0, -16.4, -15.8])
    sig = np.repeat(np.array([[0.2, 0.1, 0.05, 0.03]]), 5, axis=0)
    o = model("fixcomp", deconvolve_cut_errors=(nodes, sig))
    d = model("fixcomp")
    try:
        th = np.array([[synth.LSTAR, synth.PHISTAR, synth.SCH_AL]])
        a, b = o.context().cut_term_batch(th), d.context().cut_term_batch(th)
        assert np.isfinite(a).all() and np.isfinite(b).all() and a[0] != b[0]
        assert o.lnprob_fix_comp(th[0]) == o.context().lnprob_err_batch(th)[0]
    finally:
        o.close()
        d.close()
