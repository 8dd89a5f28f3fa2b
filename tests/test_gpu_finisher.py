"""Who finishes a tile of lf_free's polling hand-over (csrc/lf_tile.h, csrc/lf_free.h): the workgroup the
deal expects to end last, which keeps its own partial sums out of memory.  Only who adds changes, never the order of a sum: the
one launch gives the bits of the three launches (fuse = 0) and of the counter form (poll = 0), for every group size a launch can
have, and it leaves every slot empty for the launch after it."""
import numpy as np
import pytest

from lf_testlib import make_inputs, synth

pytestmark = pytest.mark.gpu

BATCHES = (1, 8, 9, 128, 192, 512, 520)
BMAX = max(BATCHES)


def _group_sizes(B, stride):
    """group size of every tile of a launch (lf_tile.h: tile_ranks)"""
    ntiles = (B + 7) // 8
    if ntiles > stride:
        return [8] * ntiles
    return [8 * ((stride - t + ntiles - 1) // ntiles) for t in range(ntiles)]


class _Case(object):
    """One FREE context and, per batch size, the three forms' lnprob - computed once, shared by the tests, never changed."""

    def __init__(self, n):
        from lumfuncmcmc_amd.capi import LFContext
        self.inp = make_inputs("free", n, seed=311)
        self.ctx = LFContext(self.inp, max_batch=64)
        self.ctx.set_option("persistent", 2)
        self.th = synth.walkers("free", BMAX, seed=312)
        self.ref = {}
        self.stride = {}

    def rows(self, B, hard):
        th = self.th[:B].copy()
        if hard:
            # one row on the careful path (10^(lum_max - L*) = 716: careful from 700, -inf from 745) and one outside the prior box
            th[B - 1, 0] = float(np.max(self.inp["lum"])) - np.log10(716.0)
            if B >= 2:
                th[0, 1] = 6.0
        return th

    def forms(self, B, hard):
        key = (B, hard)
        if key not in self.ref:
            ctx, th = self.ctx, self.rows(B, hard)
            one = ctx.lnprob_batch(th)
            ll = ctx.last_launch()
            assert ll["fused"] and ll["kernel"].startswith("lf_free"), ll
            self.stride[B] = ll["tile_stride"]
            ctx.set_option("fuse", 0)
            three = ctx.lnprob_batch(th)
            assert not ctx.last_launch()["fused"]
            ctx.set_option("fuse", 1)
            after_three = ctx.lnprob_batch(th)              # right behind a call that left sums in the buffers
            ctx.set_option("poll", 0)
            count = ctx.lnprob_batch(th)
            assert ctx.last_launch()["fused"]
            ctx.set_option("poll", 1)
            again = ctx.lnprob_batch(th)
            twice = ctx.lnprob_batch(th)
            for a in (one, three, after_three, count, again, twice):
                a.setflags(write=False)
            self.ref[key] = dict(one=one, three=three, after_three=after_three, count=count, again=again, twice=twice)
        return self.ref[key]


@pytest.fixture(scope="module", params=[1000, 40000])
def case(request):
    c = _Case(request.param)
    yield c
    c.ctx.close()


def test_the_kernel_and_the_group_sizes_are_the_ones_meant(case):
    sizes, mixed, looped = set(), False, False
    for B in BATCHES:
        case.forms(B, False)
        g = _group_sizes(B, case.stride[B])
        sizes |= set(g)
        mixed = mixed or (24 in g and 16 in g)
        looped = looped or (B + 7) // 8 > case.stride[B]
    if case.ctx.N == 1000:
        assert case.ctx.last_launch()["st"] == 4            # (cells of one source apiece)
    assert sizes == {8, 16, 24, 32}, sizes
    assert mixed and looped
    assert 1 in BATCHES and any(B % 8 for B in BATCHES if B > 8)      # one tile; a partial tile behind a full one


@pytest.mark.parametrize("B", BATCHES)
def test_one_launch_equals_three_launches_and_the_counter_form(case, B):
    r = case.forms(B, False)
    assert not np.isnan(r["one"]).any() and np.isfinite(r["one"]).sum() > 0.5 * B
    np.testing.assert_array_equal(r["one"], r["three"])
    np.testing.assert_array_equal(r["one"], r["count"])


@pytest.mark.parametrize("B", BATCHES)
def test_the_slots_are_left_empty(case, B):
    r = case.forms(B, False)
    np.testing.assert_array_equal(r["again"], r["twice"])
    np.testing.assert_array_equal(r["one"], r["twice"])
    np.testing.assert_array_equal(r["one"], r["after_three"])


@pytest.mark.parametrize("B", BATCHES)
def test_a_tile_with_a_careful_walker_keeps_the_counter(case, B):
    th = case.rows(B, True)
    case.ctx.set_option("count_forms", 1)                   # (the census: three launches)
    case.ctx.lnprob_batch(th)
    fc = case.ctx.form_counts()
    case.ctx.set_option("count_forms", 0)
    assert fc["careful"] > 0, fc
    r = case.forms(B, True)
    assert not np.isnan(r["one"]).any()
    if B >= 2:
        assert r["one"][0] == -np.inf
    for k in ("three", "count", "after_three", "again", "twice"):
        np.testing.assert_array_equal(r["one"], r[k])
    # the rows of the other tiles, and the careful walker's tile-mates, are the plain batch's
    plain = case.forms(B, False)["one"]
    keep = np.ones(B, dtype=bool)
    keep[B - 1] = False
    if B >= 2:
        keep[0] = False
    np.testing.assert_array_equal(r["one"][keep], plain[keep])


@pytest.mark.parametrize("B", BATCHES)
def test_a_row_alone_equals_the_row_in_its_batch(case, B):
    batch = case.forms(B, False)["one"]
    for i in sorted({0, B // 2, B - 1}):
        alone = case.ctx.lnprob_batch(case.th[i:i + 1])
        np.testing.assert_array_equal(alone, batch[i:i + 1])


def test_the_sampler_half_step_finishes_alike():
    """lf_free_step runs the same body; its finisher also accepts or rejects."""
    from lumfuncmcmc_amd.capi import LFContext
    from lumfuncmcmc_amd.sampler import DeviceEnsembleSampler
    inp = make_inputs("free", 40000, seed=321)
    chains = []
    for poll in (1, 0):
        ctx = LFContext(inp)
        ctx.set_option("persistent", 2)
        ctx.set_option("poll", poll)
        ds = DeviceEnsembleSampler(ctx, 32, seed=7, capacity=20)
        ds.run_mcmc(synth.walkers("free", 32, seed=322), 16)
        chains.append((ds.chain.copy(), ds.lnprobability.copy()))
        ll = ctx.last_launch()
        assert ll["fused"] and ll["kernel"].startswith("lf_free"), ll
        ds.close()
        ctx.close()
    assert np.isfinite(chains[0][1]).all()
    np.testing.assert_array_equal(chains[0][0], chains[1][0])
    np.testing.assert_array_equal(chains[0][1], chains[1][1])
