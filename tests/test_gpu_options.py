"""lf_set_option (include/lfmcmc.h) on one small FREE context: the thirteen options that are one number of the context take 1, 0
and their default again and leave lnprob's bits alone; unknown keys and out-of-range values are refused with the
messages the library has always given.  Needs a real MI355X: `pytest -m gpu`."""
import numpy as np
import pytest

from lf_testlib import make_inputs, synth
from lumfuncmcmc_amd.capi import LF_ERR_ARG, LF_OK, LFContext

pytestmark = pytest.mark.gpu

# key -> default
PLAIN = {"taper": 0, "fuse": 1, "fuse_step": 1, "poll": 1, "cells": 1, "tables": 1, "specialise": 1, "grid_shortcut": 1,
         "compress_grid": 1, "skip_grid": 0, "persistent": 1, "profile_every": 1, "profile_span": 1}
REFUSED = [("geometry", 99, "geometry must be -1 (auto) or an index below 9"),
           ("free_st", 3, "free_st must be 0 (auto), 2, 4 or 8"),
           ("walker_tile", 65, "walker_tile must be 0 (auto) .. 64"),
           ("grid_share", 1 + 65536 * 1, "grid_share must be part + 65536 * parts with part < parts")]


@pytest.fixture(scope="module")
def ctx():
    c = LFContext(make_inputs("free", 300, seed=7, S=23), device=0)
    yield c
    c.close()


def _set(ctx, key, value):
    rc = ctx._lib.lf_set_option(ctx._h, key.encode(), int(value))
    return rc, ctx._lib.lf_last_error(ctx._h).decode()


def test_plain_options_round_trip_and_leave_lnprob_alone(ctx):
    th = synth.walkers("free", 4, seed=31)
    before = ctx.lnprob_batch(th)
    assert np.isfinite(before).any()
    for key, default in PLAIN.items():
        for v in (1, 0, default):
            assert _set(ctx, key, v)[0] == LF_OK, (key, v)
    after = ctx.lnprob_batch(th)
    assert np.array_equal(before.view(np.int64), after.view(np.int64)), (before, after)


def test_an_option_changes_what_is_computed_while_it_is_set(ctx):
    """(the round trip above cannot tell a row wired to another member: skip_grid = 1 leaves piece B, a positive count, out of lnprob)"""
    th = synth.walkers("free", 4, seed=31)
    before = ctx.lnprob_batch(th)
    fin = np.isfinite(before)
    assert fin.any() and _set(ctx, "skip_grid", 1)[0] == LF_OK
    assert np.all(ctx.lnprob_batch(th)[fin] > before[fin])
    assert _set(ctx, "skip_grid", 0)[0] == LF_OK
    assert np.array_equal(ctx.lnprob_batch(th).view(np.int64), before.view(np.int64))


def test_unknown_key_is_refused_by_name(ctx):
    assert _set(ctx, "no_such_option", 1) == (LF_ERR_ARG, "unknown option no_such_option")


@pytest.mark.parametrize("key,value,message", REFUSED)
def test_out_of_range_value_is_refused_with_its_message(ctx, key, value, message):
    """(grid_share: part 1 of 1 part - a part that its parts do not have, like part 3 of 3)"""
    assert _set(ctx, key, value) == (LF_ERR_ARG, message)
    assert np.isfinite(ctx.lnprob_batch(synth.walkers("free", 4, seed=31))).any()       # (and the context still serves)
