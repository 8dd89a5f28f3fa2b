"""What the device samplers on the flux-error-convolved likelihood promise before any GPU is touched:
the two C ABI entries in the header and the binding, the `likelihood` keyword of fit_model_converged / fit_model_pt on both
model classes, the constructor keyword deconvolve_tile, and the device samplers' own check of `likelihood`."""
import os
import re

import numpy as np
import pytest

from lumfuncmcmc_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_c_abi_entries():
    from lumfuncmcmc_amd import build, capi
    hdr = open(os.path.join(ROOT, "include", "lfmcmc.h")).read()
    assert re.search(r"int lf_sampler_set_likelihood\(lf_sampler \*s, int convolved\);", hdr)
    assert re.search(r"int lf_ptsampler_set_likelihood\(lf_ptsampler \*s, int convolved\);", hdr)
    assert "#define LF_ABI_VERSION 3" in hdr
    assert '"deconv_tile"' in hdr
    lib = capi.load()
    for n in ("lf_sampler_set_likelihood", "lf_ptsampler_set_likelihood"):
        assert n in capi.EXPORTS and hasattr(lib, n)
        # refused before any device is touched
        assert getattr(lib, n)(None, 1) == capi.LF_ERR_ARG
    assert "lf_deconv_tile.h" in " ".join(build.HEADERS)


def zevol_model(cat, **extra):
    from lumfuncmcmc_amd.model import LumFuncMCMCz
    fi = np.asarray(cat["field_ind"])
    sp = lambda a: synth.split_fields(a, fi)      # noqa: E731
    kw = dict(lum=sp(cat["lum"]), lum_e=sp(cat["lum_e"]), Flim=list(synth.FLIM), alpha=synth.ALPHA_C, Omega_0=list(synth.OMEGA_0),
              sch_al=synth.SCH_AL, sch_al_lims=synth.SCH_AL_LIMS, Lstar=synth.LSTAR, Lstar_lims=synth.LSTAR_LIMS,
              phistar=synth.PHISTAR, phistar_lims=synth.PHISTAR_LIMS, Lc=synth.LC, Lh=synth.LH, nwalkers=32, nsteps=20,
              min_comp_frac=0.0, field_ind=fi)
    kw.update(extra)
    return LumFuncMCMCz(sp(cat["z"]), **kw)


@pytest.mark.parametrize("make", ["fixcomp", "zevol"])
def test_likelihood_keyword_on_both_classes(make):
    import lf_deconvlib as L
    cat = synth.catalogue(300, seed=17)
    cat["lum_e"] = np.full(300, 0.05)
    model = L.fixcomp_model if make == "fixcomp" else zevol_model
    o = model(cat, deconvolve=True, deconvolve_tile=True)
    p = model(cat)
    try:
        assert o.deconvolve_tile is True and p.deconvolve_tile is False
        for name in ("fit_model_converged", "fit_model_pt"):
            with pytest.raises(NotImplementedError, match="deconvolve") as ei:
                getattr(o, name)()
            assert "likelihood=" in str(ei.value) and name in str(ei.value)
            for obj in (o, p):
                with pytest.raises(ValueError, match="likelihood"):
                    getattr(obj, name)(likelihood="bogus")
            with pytest.raises(ValueError, match="deconvolve=True"):
                getattr(p, name)(likelihood="convolved")
    finally:
        o.close()
        p.close()


def test_device_samplers_check_likelihood_first():
    """an unknown likelihood is a ValueError before the context or a library is touched: the context here is no context"""
    from lumfuncmcmc_amd.sampler import DeviceEnsembleSampler, DevicePTSampler
    with pytest.raises(ValueError, match="likelihood"):
        DeviceEnsembleSampler(None, 16, likelihood="bogus")
    with pytest.raises(ValueError, match="likelihood"):
        DevicePTSampler(None, 2, 16, likelihood=None)
