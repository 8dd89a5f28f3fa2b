"""The entries that read the catalogue through per-field tables of their own - lf_lnprob_grad_batch, lf_lnprob_err_batch,
lf_lnprob_err_grad_batch (narrow and wide chunk tables, the 8-row tile kernel) and lf_lum_posterior (slots, caller permutation) -
on the ragged catalogues of tests/lf_fuzzlib.py: empty fields in front, in the middle and behind, n < nf, one wide source alone in
a field, every source wide, every sigma 0.  tests/test_gpu_fuzz.py does this for lf_lnprob_batch alone.

No bound of its own: lnprob_batch against the oracle with compare_rows (the anchor), then the comparisons of
tests/test_gpu_grad.py (compare), tests/test_gpu_deconv_wide.py (check_value, check_grad) and tests/test_gpu_lumpost.py (check) -
1e-12 on the twins' own S_abs scales, -inf and NaN patterns identical - and the bits the entries promise.  Then the same under
the options that change how the plain value the convolved entries read is produced, a third of the seeds; and a convolved device
chain on four ragged catalogues against its host replay."""
import functools
import time

import numpy as np
import pytest

import lf_fuzzlib as F
from lf_replaylib import host_replay
from lf_testlib import O, compare_rows, synth
from lumfuncmcmc_amd import deconv as D
from lumfuncmcmc_amd import grad as G
from test_gpu_deconv_wide import check_grad, check_value
from test_gpu_grad import compare as compare_grad
from test_gpu_lumpost import check as check_lumpost

pytestmark = pytest.mark.gpu
RTOL = 1e-12                                    # lnprob_batch against the oracle, as tests/test_gpu_fuzz.py
CASES = F.all_params()
IDS = F.case_ids()
CROSS = [s for s in F.SEEDS if s % 3 == (s // 3) % 3]          # a third of the seeds, the variants in turn
TWIN = {"s": 0.0, "depth": 0}                   # seconds spent in the twins since a test last reset it


@functools.lru_cache(maxsize=None)
def case_of(i):
    return F.build(**CASES[i])


@pytest.fixture(scope="module", autouse=True)
def twins_once():
    """The checks borrowed above call the twins themselves, and the option crossing asks for the same results many times over: here
    every twin keeps what it returned for (inputs, arrays, keywords), for this module's tests only."""
    mp = pytest.MonkeyPatch()
    kept = {}

    def once(mod, name):
        fn = getattr(mod, name)

        def f(inp, *args, **kw):
            key = (name, id(inp), tuple(a.tobytes() if isinstance(a, np.ndarray) else a for a in args), tuple(sorted(kw.items())))
            if key not in kept:
                t0 = time.perf_counter()
                TWIN["depth"] += 1
                try:
                    kept[key] = fn(inp, *args, **kw)
                finally:
                    TWIN["depth"] -= 1
                if TWIN["depth"] == 0:
                    TWIN["s"] += time.perf_counter() - t0
            return kept[key]
        mp.setattr(mod, name, f)
    once(G, "lnprob_grad")
    for name in ("delta", "lnprob_err_grad", "lum_posterior"):
        once(D, name)
    yield
    mp.undo()


def entries_against_twins(ctx, inp, th, sg, K, label):
    """Every entry of the context as it stands (its options are the caller's) against its twin, the plain value taken from the
    same context: returns the bits (lnprob, its gradient, the convolved value, its gradient, m1, m2, n_used)."""
    lp = ctx.lnprob_batch(th)
    _, g_t, s_t = G.lnprob_grad(inp, th, terms=True)
    lp_d, g_d = ctx.lnprob_grad(th)
    compare_grad(lp_d, g_d, lp, g_t, s_t, label)                       # (the value: lnprob_batch's bits)
    err = check_value(ctx, inp, th, sg, K, label)
    check_grad(ctx, inp, th, sg, K, label)                             # (the value: lnprob_err_batch's bits)
    _, eg = ctx.lnprob_err_grad(th)
    m1, m2, used = check_lumpost(ctx, inp, th, sg, K, label)
    assert used == int(np.isfinite(lp).sum()), label
    return lp, g_d, err, eg, m1, m2, used


def same_bits(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_entries_on_a_ragged_catalogue(i):
    from lumfuncmcmc_amd.capi import LFContext
    inp, th, sg, K, label = case_of(i)
    TWIN["s"] = 0.0
    ref = O.lnprob_batch(inp, th)
    ctx = LFContext(inp)
    try:
        compare_rows(ctx.lnprob_batch(th), ref, inp, th, RTOL, label)
        lp, g, err, eg, m1, m2, used = entries_against_twins(ctx, inp, th, sg, K, label)
        if inp["variant"] != "free":
            # the 8-row tile kernel over the same narrow chunks: the bits of the per-row kernels; the gradient entry ignores it
            ctx.set_option("deconv_tile", 1)
            tile, (tv, tg) = ctx.lnprob_err_batch(th), ctx.lnprob_err_grad(th)
            ctx.set_option("deconv_tile", 0)
            assert np.array_equal(tile, err), "%s: deconv_tile changes bits" % label
            assert np.array_equal(tv, err) and np.array_equal(tg, eg, equal_nan=True), "%s: deconv_tile changes the gradient entry" % label
        if np.count_nonzero(sg) == 1 and used:
            j = int(np.flatnonzero(sg)[0])
            assert m1[j] != 0.0 and m2[j] > 0.0 and np.count_nonzero(m1) == 1 and np.count_nonzero(m2) == 1, label
        if not sg.any():
            assert np.array_equal(err, lp) and np.array_equal(eg, g, equal_nan=True), "%s: every sigma 0, not the plain bits" % label
        if np.all(sg <= D.sigma_max(K)):
            ctx.set_lum_err(sg, K, wide=False)
            ov, og = ctx.lnprob_err_grad(th)
            assert np.array_equal(ctx.lnprob_err_batch(th), err) and np.array_equal(ov, err) and np.array_equal(og, eg, equal_nan=True), \
                "%s: no source above the order's limit, deconv_wide changes bits" % label
            o1, o2, ou = ctx.lum_posterior(th)
            assert ou == used and np.array_equal(o1, m1, equal_nan=True) and np.array_equal(o2, m2, equal_nan=True), label
    finally:
        ctx.close()
    print("%s: twins %.2f s" % (label, TWIN["s"]))


# What each entry does under an option that changes how the plain value is produced (csrc/lfmcmc.hip: enqueue, family_check; the
# table of DESIGN.md section 3.24): every one ACCEPTS every one of these - the option reaches the plain value through the
# library's one lnprob path, the tables of the entry's own kernels do not depend on it.  (The refusals the entries do have,
# "skip_grid" and "grid_share", are those of tests/test_gpu_grad.py, test_gpu_deconv_wide.py and test_gpu_lumpost.py.)
# name -> (the settings, the settings that undo them, the variants it is crossed on, the kernel lnprob_batch must then report)
OPTIONS = {
    "compress": ([("compress", 1)], [("compress", 0)], F.VARIANTS, "lf_"),            # (FIXCOMP has nothing to compress)
    "geometry": ([("geometry", None)], [("geometry", -1)], F.VARIANTS, "lf_main"),
    "persistent, free_st 0": ([("persistent", 2), ("free_st", 0)], [("persistent", 1)], ("free",), "lf_free"),
    "persistent, free_st 2": ([("persistent", 2), ("free_st", 2)], [("persistent", 1), ("free_st", 0)], ("free",), "lf_free<2>"),
    "persistent, fuse 0": ([("persistent", 2), ("fuse", 0)], [("persistent", 1), ("fuse", 1)], ("free",), "lf_free"),
    # (cells are made for catalogues this small too, and FREE and ZEVOL then run the persistent kernels: without them, lf_main)
    "cells": ([("cells", 0)], [("cells", 1)], F.VARIANTS, {"free": "lf_main", "fixcomp": "lf_", "zevol": "lf_main"}),
}


@pytest.mark.parametrize("seed", CROSS)
def test_entries_under_the_options_of_the_plain_value(seed):
    from lumfuncmcmc_amd.capi import LFContext
    inp, th, sg, K, label = case_of(seed)
    TWIN["s"] = 0.0
    ref = O.lnprob_batch(inp, th)
    geo = int(np.random.default_rng(8000 + seed).integers(0, 9))
    ctx = LFContext(inp)
    try:
        before = entries_against_twins(ctx, inp, th, sg, K, label)
        for name, (on, off, variants, kernel) in OPTIONS.items():
            if inp["variant"] not in variants:
                continue
            what = "%s [%s]" % (label, name if name != "geometry" else "geometry %d" % geo)
            for key, val in on:
                ctx.set_option(key, geo if val is None else val)
            compare_rows(ctx.lnprob_batch(th), ref, inp, th, RTOL, what)
            launch = ctx.last_launch()
            kernel = kernel if isinstance(kernel, str) else kernel[inp["variant"]]
            assert launch["kernel"].startswith(kernel) and (name != "persistent, fuse 0" or not launch["fused"]), (what, launch)
            entries_against_twins(ctx, inp, th, sg, K, what)
            for key, val in off:
                ctx.set_option(key, val)
            assert same_bits(entries_against_twins(ctx, inp, th, sg, K, what + " undone"), before), "%s: other bits after the reset" % what
    finally:
        ctx.close()
    print("%s: twins %.2f s" % (label, TWIN["s"]))


@pytest.mark.parametrize("k", range(4), ids=["%s-%s" % (p["label"].replace(" ", ""), p["variant"]) for p in F.sampler_params()])
def test_convolved_chain_on_a_ragged_catalogue(k):
    """16 walkers, 3 steps, the wide rule on; fixed completeness: also with the tile kernel"""
    from lumfuncmcmc_amd.capi import LFContext
    from lumfuncmcmc_amd.sampler import DeviceEnsembleSampler
    p = F.sampler_params()[k]
    inp, _, sg, K, label = F.build(**p)
    W, steps, seed = 16, 3, 0xF022 + k
    pos = synth.walkers(p["variant"], W, seed=33 + k, fix_sch_al=p["fsa"], nf=len(p["sizes"]))
    ctx = LFContext(inp)
    try:
        ctx.set_lum_err(sg, K, wide=True)
        for tile in ((0,) if p["variant"] == "free" else (0, 1)):
            ctx.set_option("deconv_tile", tile)
            chain, lnp, nacc = host_replay(ctx, pos, steps, seed, lnprob=ctx.lnprob_err_batch)
            assert np.isfinite(lnp).any(), label
            ds = DeviceEnsembleSampler(ctx, W, seed=seed, capacity=steps, likelihood="convolved")
            try:
                ds.run_mcmc(pos, steps)
                np.testing.assert_array_equal(ds.chain, chain)
                np.testing.assert_array_equal(ds.lnprobability, lnp)
                np.testing.assert_array_equal(ds.naccepted, nacc)
            finally:
                ds.close()
    finally:
        ctx.close()
