"""The device ensemble sampler replayed on the host, bit for bit, at every tile edge and through every form a half-step can
take - each case also says which kernel it ran (ctx.last_launch()) - and one check that shares no algorithm with the
replay: the sampler's stationary distribution against quadrature.

A half-ensemble is cut into tiles of 8 walkers (csrc/lf_tile.h: PTW).  A half-step runs as lf_free_step / lf_pers_step (one
launch: proposal in the prologue, accept by the tile's finishing workgroup), as lf_prepare + lf_free / lf_pers + lf_finalize
("fuse_step" 0), as lf_prepare + lf_main + lf_finalize ("persistent" 0, or no cells for the z-evolving variant), or as
lf_propose + the plain evaluation + lf_accept (enqueue_sharded).  The replay evaluates its proposals with the context's plain
call at the same options and the same batch size, the half."""
import numpy as np
import pytest

from lf_replaylib import fixcomp_model, host_replay, peak_box, refined_moments
from lf_testlib import make_inputs, synth

pytestmark = pytest.mark.gpu

NSTEPS = 8
SEED = 0x1234567890ABCDEF
LF_MAIN, LF_FREE, LF_PERS = 0, 2, 4          # last_launch()["kind"]
PERSISTENT = {"free": LF_FREE, "fixcomp": LF_PERS, "zevol": LF_PERS}


def _context(variant, n, fsa, nf=5, options=()):
    from lumfuncmcmc_amd.capi import LFContext
    ctx = LFContext(make_inputs(variant, n, seed=31, fix_sch_al=fsa, nf=nf))
    for key, value in options:
        ctx.set_option(key, value)
    return ctx


def _start(variant, W, fsa, nf=5, seed=32):
    pos = synth.walkers(variant, W, seed=seed + W, fix_sch_al=fsa, nf=nf)
    pos[1] = 99.0                                  # one walker starts outside the prior (-inf)
    return pos


def _assert_launch(ctx, kind, fused, rows, st=None):
    ll = ctx.last_launch()
    assert (ll["kind"], ll["fused"], ll["rows"]) == (kind, fused, rows), ll
    if st is not None:
        assert ll["st"] == st and ll["kernel"] == "lf_free<%d>" % st, ll
    return ll


def _assert_replay(ds, ctx, pos, nsteps, seed, kind, fused, st=None, a=2.0, lnprob0=None):
    """ds has run nsteps from pos: its launch is the one the case is meant for, and its chain is the replay's."""
    half = pos.shape[0] // 2
    _assert_launch(ctx, kind, fused, half, st)
    chain, lnps, nacc = host_replay(ctx, pos, nsteps, seed, a=a, lnprob0=lnprob0)
    # (the replay's proposals went through the plain call of the same kernel family at the same batch size)
    ll = ctx.last_launch()
    assert (ll["kind"], ll["rows"]) == (kind, half), ll
    assert ds.chain.shape == (pos.shape[0], nsteps, ctx.ndim)
    assert np.array_equal(ds.naccepted, nacc)
    assert np.array_equal(ds.chain, chain)
    assert np.array_equal(ds.lnprobability, lnps)
    assert 0 < ds.acceptance_fraction.mean() < 1
    return chain, lnps, nacc


def _run(ctx, pos, nsteps=NSTEPS, seed=SEED, a=2.0, lnprob0=None):
    from lumfuncmcmc_amd.sampler import DeviceEnsembleSampler
    ds = DeviceEnsembleSampler(ctx, pos.shape[0], a=a, seed=seed, capacity=nsteps)
    ds.run_mcmc(pos, nsteps, lnprob0=lnprob0)
    return ds


# ------------------------------------------------------------------------------------------------------------------ shapes
# ndim: free 9 / 8 (five fields) and 5 / 4 (one field), fixcomp 3 / 2, zevol 7 / 6 - every power of z from 1 to 8.
# W: 2 ndim (the smallest the class accepts: one partial tile), 18 (a half of 8 + 1), 256 (16 full tiles: the benchmark's
# shape), 258 (a half of 129), 1026 (a half of 513).
def _shape_cases():
    out = []
    for variant, nf in (("free", 5), ("free", 1), ("fixcomp", 5), ("zevol", 5)):
        for fsa in (False, True):
            nd = synth.ndim_of(variant, fsa, nf)
            out += [pytest.param(variant, nf, fsa, W, id="%s-nf%d-ndim%d-W%d" % (variant, nf, nd, W))
                    for W in sorted({2 * nd, 18, 256, 258, 1026})]
    return out


@pytest.mark.parametrize("variant,nf,fsa,W", _shape_cases())
def test_shapes_replay_on_the_default_path(variant, nf, fsa, W):
    """The one-launch half-step (lf_free_step<4> / lf_pers_step; the free variant hands over by polling at every W: a tile's
    partial sums are 32 slots, whatever the batch)."""
    ctx = _context(variant, 2500, fsa, nf)
    assert ctx.ndim == synth.ndim_of(variant, fsa, nf) and W >= 2 * ctx.ndim
    pos = _start(variant, W, fsa, nf)
    ds = _run(ctx, pos)
    _assert_replay(ds, ctx, pos, NSTEPS, SEED, PERSISTENT[variant], True, 4 if variant == "free" else None)
    ds.close(); ctx.close()


# ------------------------------------------------------------------------------------------------------------------- paths
# name -> (options, n, and per variant (kind, fused, st)).  "cells" 0: the free variant then reaches lf_free only from 8192
# sources and ~2000 work items (lf_main here), or when asked to ("persistent" 2: a row of its own, lf_free without cells); the
# z-evolving variant has no persistent kernel without its cells and takes lf_main; fixed completeness has no cells to lose.
# last_launch() tells neither the polling hand-over from the counting one nor lf_free_step from a plain fused lf_free: the
# "poll" 0 rows assert the kernel family of the default rows, and what they add is the replay through the other hand-over.
PATHS = {
    "default": ((), 2500, {"free": (LF_FREE, True, 4), "fixcomp": (LF_PERS, True, None), "zevol": (LF_PERS, True, None)}),
    "poll0": ((("poll", 0),), 2500, {"free": (LF_FREE, True, 4), "fixcomp": (LF_PERS, True, None), "zevol": (LF_PERS, True, None)}),
    "fuse_step0": ((("fuse_step", 0),), 2500,
                   {"free": (LF_FREE, False, 4), "fixcomp": (LF_PERS, False, None), "zevol": (LF_PERS, False, None)}),
    "persistent0": ((("persistent", 0),), 2500,
                    {"free": (LF_MAIN, False, None), "fixcomp": (LF_MAIN, False, None), "zevol": (LF_MAIN, False, None)}),
    "cells0": ((("cells", 0),), 2500,
               {"free": (LF_MAIN, False, None), "fixcomp": (LF_PERS, True, None), "zevol": (LF_MAIN, False, None)}),
    "cells0_persistent2": ((("cells", 0), ("persistent", 2)), 2500, {"free": (LF_FREE, True, 4)}),
    "free_st2": ((("free_st", 2),), 2500, {"free": (LF_FREE, True, 2)}),
    "free_st4": ((("free_st", 4),), 2500, {"free": (LF_FREE, True, 4)}),
}


def _path_cases(names):
    return [pytest.param(name, variant, W, id="%s-%s-W%d" % (name, variant, W))
            for name in names for variant in PATHS[name][2] for W in (18, 258)]


@pytest.mark.parametrize("name,variant,W", _path_cases(PATHS))
def test_forced_paths_replay(name, variant, W):
    options, n, expect = PATHS[name]
    kind, fused, st = expect[variant]
    ctx = _context(variant, n, False, options=options)
    pos = _start(variant, W, False)
    ds = _run(ctx, pos)
    _assert_replay(ds, ctx, pos, NSTEPS, SEED, kind, fused, st)
    ds.close(); ctx.close()


@pytest.mark.parametrize("variant,W", [pytest.param(v, W, id="%s-W%d" % (v, W)) for v in ("free", "fixcomp", "zevol") for W in (18, 258)])
def test_sharded_form_replays_on_one_rank(variant, W):
    """enqueue_sharded without a process group: it calls lf_sampler_half_eval (lf_propose, then the plain one-launch
    evaluation of the half) and lf_sampler_half_accept (lf_accept) itself, never lf_sampler_run.  last_launch() describes the
    evaluation only, which is what is asserted; that lf_propose and lf_accept ran follows from the entry points, not from it."""
    from lumfuncmcmc_amd.sampler import DeviceEnsembleSampler
    ctx = _context(variant, 2500, False)
    pos = _start(variant, W, False)
    ds = DeviceEnsembleSampler(ctx, W, seed=SEED, capacity=NSTEPS)
    ds.enqueue_sharded(pos, NSTEPS)
    ds.sync()
    _assert_replay(ds, ctx, pos, NSTEPS, SEED, PERSISTENT[variant], True, 4 if variant == "free" else None)
    ds.close(); ctx.close()


# --------------------------------------------------------------------------------------------------------------- arguments
VARIANTS = ["free", "fixcomp", "zevol"]


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("fsa", [False, True])
def test_stretch_scale(variant, fsa):
    """a = 1.3 through the one-launch half-step (the scale enters the proposal and, through z, the accept step's (ndim - 1)
    log z) and through lf_propose / lf_accept."""
    from lumfuncmcmc_amd.sampler import DeviceEnsembleSampler
    ctx = _context(variant, 2500, fsa)
    W = 18
    pos = _start(variant, W, fsa)
    ds = _run(ctx, pos, a=1.3)
    kind, st = PERSISTENT[variant], 4 if variant == "free" else None
    chain, _, _ = _assert_replay(ds, ctx, pos, NSTEPS, SEED, kind, True, st, a=1.3)
    assert not np.array_equal(chain, host_replay(ctx, pos, NSTEPS, SEED, a=2.0)[0])
    sh = DeviceEnsembleSampler(ctx, W, a=1.3, seed=SEED, capacity=NSTEPS)
    sh.enqueue_sharded(pos, NSTEPS)
    sh.sync()
    assert np.array_equal(sh.chain, ds.chain) and np.array_equal(sh.lnprobability, ds.lnprobability)
    assert np.array_equal(sh.naccepted, ds.naccepted)
    ds.close(); sh.close(); ctx.close()


@pytest.mark.parametrize("variant", VARIANTS)
def test_lnprob0_given(variant):
    """The start's lnprob as ctx.lnprob_batch gives it: the chain of a run started without it."""
    ctx = _context(variant, 2500, False)
    pos = _start(variant, 34, False)
    lp0 = ctx.lnprob_batch(pos)
    assert lp0[1] == -np.inf and np.isfinite(lp0).sum() == len(lp0) - 1
    a = _run(ctx, pos)
    b = _run(ctx, pos, lnprob0=lp0)
    assert np.array_equal(a.chain, b.chain) and np.array_equal(a.lnprobability, b.lnprobability)
    assert np.array_equal(a.naccepted, b.naccepted)
    _assert_replay(b, ctx, pos, NSTEPS, SEED, PERSISTENT[variant], True, lnprob0=lp0)
    a.close(); b.close(); ctx.close()


@pytest.mark.parametrize("variant", VARIANTS)
def test_continuing_is_one_longer_run(variant):
    from lumfuncmcmc_amd.sampler import DeviceEnsembleSampler
    ctx = _context(variant, 2500, False)
    pos = _start(variant, 34, False)
    ds = DeviceEnsembleSampler(ctx, 34, seed=SEED, capacity=NSTEPS)
    ds.run_mcmc(pos, 3)
    ds.run_mcmc(None, 5)
    _assert_replay(ds, ctx, pos, NSTEPS, SEED, PERSISTENT[variant], True)
    ds.close(); ctx.close()


@pytest.mark.parametrize("variant", VARIANTS)
def test_two_samplers_on_one_context(variant):
    """Two samplers of different seeds, starts and sizes alive on one context, a step of one enqueued after a step of the
    other: they share the context's workspace, its partial-sum slots and its tile counters, and each must still make its own
    chain."""
    from lumfuncmcmc_amd.sampler import DeviceEnsembleSampler
    ctx = _context(variant, 2500, False)
    W1, W2, s1, s2 = 258, 18, SEED, 987654321
    p1, p2 = _start(variant, W1, False), _start(variant, W2, False, seed=77)
    d1 = DeviceEnsembleSampler(ctx, W1, seed=s1, capacity=NSTEPS)
    d2 = DeviceEnsembleSampler(ctx, W2, seed=s2, capacity=NSTEPS)
    for it in range(NSTEPS):
        d1.enqueue(p1 if it == 0 else None, 1)
        d2.enqueue(p2 if it == 0 else None, 1)
    d1.sync(); d2.sync()
    _assert_launch(ctx, PERSISTENT[variant], True, W2 // 2)
    for ds, pos, seed in ((d1, p1, s1), (d2, p2, s2)):
        chain, lnps, nacc = host_replay(ctx, pos, NSTEPS, seed)
        assert np.array_equal(ds.chain, chain) and np.array_equal(ds.lnprobability, lnps)
        assert np.array_equal(ds.naccepted, nacc)
        assert 0 < ds.acceptance_fraction.mean() < 1
    d1.close(); d2.close(); ctx.close()


# ------------------------------------------------------------------------------------------- the stationary distribution
# Fixed completeness, fixed faint-end slope (theta = log L*, log phi*), 300 sources.  The reference is the posterior's mean and
# covariance by quadrature; the sampler runs 64 walkers from a ball around the grid's maximum, the first 20 tau are discarded
# and the effective sample size is chain_diagnostics'.  Criteria (thresholds of the estimators' own sampling error, at five
# standard errors): every mean within 5 sigma / sqrt(ESS), every variance ratio within 1 +- 5 sqrt(2 / ESS) (the standard
# error of a variance from ESS normal draws).  4000 steps: tau is 10 to 20 steps for this near-Gaussian 2-d posterior, so
# ESS = 64 (4000 - 20 tau) / tau is above 10 000 per parameter against the 2000 the check requires.
STAT_STEPS, STAT_W, STAT_SEED, STAT_MIN_ESS = 4000, 64, 20260117, 2000.0


def _zscores(chain, mean, cov):
    """(z of the means, z of the variance ratios, ESS, t0) of a chain (W, steps, 2) against the quadrature's moments."""
    from lumfuncmcmc_amd.sampler import chain_diagnostics
    tau0 = chain_diagnostics(chain).tau
    t0 = int(np.ceil(20.0 * tau0.max()))
    assert t0 < chain.shape[1] // 2, (tau0, t0)
    ess = chain_diagnostics(chain, t0=t0).ess
    flat = chain[:, t0:].reshape(-1, 2)
    sd = np.sqrt(np.diag(cov))
    zm = (flat.mean(axis=0) - mean) / (sd / np.sqrt(ess))
    zv = (flat.var(axis=0) / np.diag(cov) - 1.0) / np.sqrt(2.0 / ess)
    return zm, zv, ess, t0


@pytest.fixture(scope="module")
def posterior():
    m = fixcomp_model(300, seed=71)
    ctx = m.context()
    box = m._theta_lims()
    assert box.shape == (2, 2)
    lo, hi = peak_box(ctx, box)
    mean, cov, mode, cells = refined_moments(ctx, lo, hi)
    yield ctx, mean, cov, mode, cells
    m.close()


def _ball(mode, cov):
    rng = np.random.default_rng(5)
    return mode + 0.1 * np.sqrt(np.diag(cov)) * rng.normal(size=(STAT_W, 2))


def test_stationary_distribution_against_quadrature(posterior):
    ctx, mean, cov, mode, cells = posterior
    p0 = _ball(mode, cov)
    ds = _run(ctx, p0, nsteps=STAT_STEPS, seed=STAT_SEED)
    _assert_launch(ctx, LF_PERS, True, STAT_W // 2)
    zm, zv, ess, t0 = _zscores(ds.chain, mean, cov)
    print("quadrature (%d cells a side): mean %s sd %s; device sampler: t0 %d ESS %s z(mean) %s z(var) %s" % (
        cells, mean, np.sqrt(np.diag(cov)), t0, ess, zm, zv))
    assert np.all(ess >= STAT_MIN_ESS), ess
    assert np.all(np.abs(zm) <= 5.0), zm
    assert np.all(np.abs(zv) <= 5.0), zv
    ds.close()


def test_stationary_check_sees_a_wrong_exponent(posterior):
    """The same run with z^ndim in place of z^(ndim - 1) in the acceptance ratio (the host replay, over the same context):
    the criteria must fail, or the run above is too short to mean anything."""
    ctx, mean, cov, mode, cells = posterior
    chain, _, _ = host_replay(ctx, _ball(mode, cov), STAT_STEPS, STAT_SEED, exponent=ctx.ndim)
    zm, zv, ess, t0 = _zscores(chain, mean, cov)
    print("wrong exponent: t0 %d ESS %s z(mean) %s z(var) %s" % (t0, ess, zm, zv))
    assert np.all(ess >= STAT_MIN_ESS), ess
    assert max(np.abs(zm).max(), np.abs(zv).max()) > 5.0, (zm, zv)
