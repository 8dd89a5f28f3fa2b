"""Posterior LF bands without a GPU: the NumPy statement of lf_lumfunc_quantiles (lfbands.quantiles_host), the draws of
lf_percentiles against set_median_fit's, and the argument checks of the C entry (made before the device is touched)."""

import numpy as np
import pytest

from lf_testlib import synth
from lumfuncmcmc_amd import capi, hostsetup as hs, lfbands


def _model(n=1500, seed=7, fix_sch_al=False):
    from lumfuncmcmc_amd.model import LumFuncMCMC
    cat = synth.catalogue(n, seed=seed)
    fi = cat["field_ind"]
    m = LumFuncMCMC(synth.split_fields(cat["z"], fi), lum=synth.split_fields(cat["lum"], fi),
                    lum_e=synth.split_fields(cat["lum_e"], fi), Flim=list(synth.FLIM), alpha=synth.ALPHA_C,
                    Omega_0=list(synth.OMEGA_0), sch_al=synth.SCH_AL, sch_al_lims=synth.SCH_AL_LIMS, Lstar=synth.LSTAR,
                    Lstar_lims=synth.LSTAR_LIMS, phistar=synth.PHISTAR, phistar_lims=synth.PHISTAR_LIMS, Lc=synth.LC,
                    Lh=synth.LH, nwalkers=32, nsteps=10, min_comp_frac=0.0, field_ind=fi, Flim_lims=synth.FLIM_LIMS,
                    alpha_lims=synth.ALPHA_LIMS, fix_sch_al=fix_sch_al)
    rng = np.random.default_rng(seed)
    ndim = len(m._theta_lims())
    th = np.column_stack([rng.normal(42.6, 0.05, 600), rng.normal(-2.1, 0.05, 600)] +
                         ([] if fix_sch_al else [rng.normal(-1.5, 0.05, 600)]) +
                         [rng.normal(f, 0.1, 600) for f in synth.FLIM] + [rng.normal(synth.ALPHA_C, 0.1, 600)])
    assert th.shape[1] == ndim
    m.samples = np.column_stack([th, rng.normal(-100.0, 3.0, 600)])
    return m


@pytest.mark.parametrize("variant", ["free", "zevol"])
@pytest.mark.parametrize("method", ["linear", "median"])
def test_quantiles_host_is_the_full_matrix_numpy_statement(variant, method):
    rng = np.random.default_rng(3)
    R, P = 37, 1000
    logL = rng.uniform(40.5, 44.0, P)
    z = rng.uniform(1.1, 2.0, P) if variant == "zevol" else None
    if variant == "free":
        draws = np.column_stack([rng.normal(42.5, 0.2, R), rng.normal(-2.5, 0.3, R), rng.normal(-1.5, 0.3, R)])
        full = np.array([hs.true_lum_func(logL, d[2], d[0], d[1]) for d in draws])
    else:
        rows = np.column_stack([rng.normal(42.5, 0.1, (R, 3)), rng.normal(-2.5, 0.1, (R, 3)), rng.normal(-1.5, 0.2, R)])
        draws = lfbands.pack_draws("zevol", rows, pivots=(1.2, 1.53, 1.86))
        full = np.array([hs.schechter_z(logL, z, r[6], *r[:6], 1.2, 1.53, 1.86) for r in rows])
    q = (2.5, 16, 50, 84, 97.5)
    want = np.percentile(full, q, axis=0) if method == "linear" else np.median(full, axis=0)[None]
    got = lfbands.quantiles_host(variant, draws, logL, z=z, q=q, method=method, chunk=97)      # several chunks
    assert got.shape == want.shape
    np.testing.assert_array_equal(got, want)


def test_pack_draws_takes_alpha_from_the_object_when_it_is_fixed():
    rows = np.array([[42.0, -3.0, 2.5, 3.5, 99.0], [43.0, -2.0, 2.6, 3.6, 98.0]])
    np.testing.assert_array_equal(lfbands.pack_draws("free", rows, fix_sch_al=True, sch_al=-1.25),
                                  [[42.0, -3.0, -1.25], [43.0, -2.0, -1.25]])
    np.testing.assert_array_equal(lfbands.pack_draws("fixcomp", rows), rows[:, :3])


@pytest.mark.parametrize("fix_sch_al", [False, True])
def test_lf_percentiles_median_reproduces_set_median_fit_and_its_draws(fix_sch_al):
    m = _model(fix_sch_al=fix_sch_al)
    R = 57
    np.random.seed(11)
    got = m.lf_percentiles(method="median", ndraws=R, device=False)
    state_after = np.random.get_state()

    # set_median_fit's own draw loop and median (its VeffLF, which draws more numbers, is left out)
    np.random.seed(11)
    m2 = _model(fix_sch_al=fix_sch_al)
    m2.VeffLF = lambda *a, **k: None
    m2.set_median_fit(rndsamples=R)
    assert got.shape == (1, m.lum.size)
    np.testing.assert_array_equal(got[0], m2.medianLF)

    np.random.seed(11)
    n = len(m._select_samples(7.5, keep_lnprob=True))
    for _ in range(R):
        np.random.randint(0, n)
    want = np.random.get_state()
    assert state_after[0] == want[0] and state_after[2:] == want[2:]
    np.testing.assert_array_equal(state_after[1], want[1])


def test_lf_percentiles_linear_shape_and_order():
    m = _model()
    np.random.seed(5)
    out = m.lf_percentiles(percentiles=(16, 50, 84), logL=np.linspace(41, 44, 50), ndraws=40, device=False)
    assert out.shape == (3, 50)
    assert np.all(out[0] <= out[1]) and np.all(out[1] <= out[2])
    with pytest.raises(ValueError):
        m.lf_percentiles(method="nearest", device=False)


# ------------------------------------------------------------------------------------------------ the C entry's checks
@pytest.fixture(scope="module")
def lib():
    from lumfuncmcmc_amd import build
    build.build_library(verbose=False)
    return capi.load()


def test_the_entry_is_exported_and_the_abi_is_version_3(lib):
    assert lib.lf_abi_version() == 3 == capi.LF_ABI_VERSION
    for name in ("lf_lumfunc_quantiles", "lf_lumfunc_quantiles_ms"):
        assert hasattr(lib, name) and name in capi.EXPORTS


def _call(lib, variant=0, R=4, P=8, draws=True, logL=True, z=False, nq=1, q=(50.0,), method=0, out=True):
    p = capi._ptr
    d = np.zeros((max(R, 1), 7))
    L = np.full(max(P, 1), 42.0)
    qa = np.array(q, dtype=np.float64) if q is not None else None
    o = np.zeros(max(nq, 1) * max(P, 1))
    return lib.lf_lumfunc_quantiles(0, variant, R, p(d) if draws else None, P, p(L) if logL else None, p(L) if z else None, nq,
                                    p(qa) if qa is not None else None, method, p(o) if out else None, None)


@pytest.mark.parametrize("kw", [
    dict(R=0), dict(R=4097), dict(R=-1),
    dict(nq=0, q=()), dict(nq=33, q=tuple(range(33))),
    dict(q=(-1e-9,)), dict(q=(100.0000001,)), dict(q=(float("nan"),)), dict(nq=2, q=(50.0, float("nan"))),
    dict(draws=False), dict(logL=False), dict(out=False), dict(q=None), dict(variant=2, z=False),
    dict(variant=3), dict(variant=-1), dict(method=2), dict(method=-1),
    dict(method=1, nq=2, q=(50.0, 50.0)), dict(method=1, nq=0, q=None),
    dict(P=0), dict(P=-5),
])
def test_bad_arguments_are_refused_before_the_device_is_touched(lib, kw):
    assert _call(lib, **kw) == capi.LF_ERR_ARG


def test_wrapper_raises_lferror(lib):
    with pytest.raises(capi.LFError):
        capi.lumfunc_quantiles("free", np.zeros((4097, 3)), np.zeros(3))
