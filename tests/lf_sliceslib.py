"""Model objects with a synthetic posterior for the tests of the 1/Veff points in redshift slices (test_veffslices_cpu.py,
test_gpu_veffslices.py).  No GPU needed to make them.  Test infrastructure only."""
import numpy as np

from lf_testlib import synth

PIVOTS = (1.20, 1.53, 1.86)


def _kw(cat, nboot, nbins, mcf):
    fi = cat["field_ind"]
    return dict(lum=synth.split_fields(cat["lum"], fi), lum_e=synth.split_fields(cat["lum_e"], fi), Flim=list(synth.FLIM),
                alpha=synth.ALPHA_C, Omega_0=list(synth.OMEGA_0), sch_al=synth.SCH_AL, nwalkers=32, nsteps=10, min_comp_frac=mcf,
                field_ind=fi, nboot=nboot, nbins=nbins)


def zmodel(n=2000, seed=11, nboot=20, nbins=25, mcf=0.0):
    """LumFuncMCMCz on synth's catalogue with a posterior cloud around a z-evolving truth: L* brightens by 0.5 dex and phi*
    drops by 0.7 dex across the pivots"""
    from lumfuncmcmc_amd.model import LumFuncMCMCz
    cat = synth.catalogue(n, seed=seed)
    m = LumFuncMCMCz(synth.split_fields(cat["z"], cat["field_ind"]), z1=PIVOTS[0], z2=PIVOTS[1], z3=PIVOTS[2], **_kw(cat, nboot, nbins, mcf))
    rng = np.random.default_rng(seed)
    m.samples = np.column_stack([rng.normal(42.3, 0.03, 300), rng.normal(42.5, 0.03, 300), rng.normal(42.8, 0.03, 300),
                                 rng.normal(-2.0, 0.03, 300), rng.normal(-2.3, 0.03, 300), rng.normal(-2.7, 0.03, 300),
                                 rng.normal(-1.5, 0.03, 300), rng.normal(-50.0, 2.0, 300)])
    return m


def model(n=2000, seed=7, nboot=20, nbins=25, mcf=0.0):
    """LumFuncMCMC (free completeness) with a posterior cloud around synth's single Schechter function"""
    from lumfuncmcmc_amd.model import LumFuncMCMC
    cat = synth.catalogue(n, seed=seed)
    m = LumFuncMCMC(synth.split_fields(cat["z"], cat["field_ind"]), sch_al_lims=synth.SCH_AL_LIMS, Lstar=synth.LSTAR,
                    Lstar_lims=synth.LSTAR_LIMS, phistar=synth.PHISTAR, phistar_lims=synth.PHISTAR_LIMS, Lc=synth.LC, Lh=synth.LH,
                    Flim_lims=synth.FLIM_LIMS, alpha_lims=synth.ALPHA_LIMS, **_kw(cat, nboot, nbins, mcf))
    rng = np.random.default_rng(seed)
    th = np.column_stack([rng.normal(42.6, 0.05, 300), rng.normal(-2.1, 0.05, 300), rng.normal(-1.5, 0.05, 300)] +
                         [rng.normal(f, 0.1, 300) for f in synth.FLIM] + [rng.normal(synth.ALPHA_C, 0.1, 300)])
    m.samples = np.column_stack([th, rng.normal(-100.0, 3.0, 300)])
    return m
