"""Shared pieces of the tests of the flux-error-convolved likelihood (tests/test_deconv_cpu.py, tests/test_gpu_deconv.py):
the seeded noisy mock of the Eddington-bias check and its L* profile grid.  Test infrastructure only."""
import functools

import numpy as np

from lumfuncmcmc_amd import synth

EDD_SEED, EDD_N, EDD_ERR = 3, 3000, 0.25
EDD_GRID = np.linspace(-0.4, 0.4, 41)              # offsets from the true L*, 0.02 dex apart


def fixcomp_model(cat, **extra):
    from lumfuncmcmc_amd.model import LumFuncMCMC
    fi = np.asarray(cat["field_ind"])
    as_lists = lambda a: a if isinstance(a, list) else synth.split_fields(a, fi)      # noqa: E731
    kw = dict(lum=as_lists(cat["lum"]), lum_e=as_lists(cat["lum_e"]), Flim=list(synth.FLIM), alpha=synth.ALPHA_C,
              Omega_0=list(synth.OMEGA_0), sch_al=synth.SCH_AL, sch_al_lims=synth.SCH_AL_LIMS, Lstar=synth.LSTAR,
              Lstar_lims=synth.LSTAR_LIMS, phistar=synth.PHISTAR, phistar_lims=synth.PHISTAR_LIMS, Lc=synth.LC, Lh=synth.LH,
              nwalkers=32, nsteps=20, min_comp_frac=0.0, field_ind=fi, fix_comp=True, Flim_lims=synth.FLIM_LIMS,
              alpha_lims=synth.ALPHA_LIMS)
    kw.update(extra)
    return LumFuncMCMC(as_lists(cat["z"]), **kw)


def noisy_mock(n, lum_err, seed, **extra):
    """(model object over a mock of about n sources drawn at theta_true with Gaussian noise lum_err, theta_true, the mock)"""
    base = fixcomp_model(synth.catalogue(2000, seed=17))
    theta = np.array([synth.LSTAR, synth.PHISTAR, synth.SCH_AL])
    m0 = base._mock_generator(False).counts(theta[None], 0)[0].sum()
    theta[1] += np.log10(n / m0)
    mc = base.mock_catalogue(theta, seed=seed, device=False, lum_err=lum_err)
    base.close()
    return fixcomp_model(mc, **extra), theta, mc


@functools.lru_cache(maxsize=None)
def eddington_case():
    """(kernel inputs of the model over the seeded noisy mock, sigma[N], theta_true, the 41 profile rows)"""
    o, theta, _ = noisy_mock(EDD_N, EDD_ERR, EDD_SEED)
    inp = o.kernel_inputs()
    sigma = np.array(o.lum_e)
    rows = np.repeat(theta[None], EDD_GRID.size, axis=0)
    rows[:, 0] += EDD_GRID
    return inp, sigma, theta, rows
