"""Who finishes a tile of lf_free's polling hand-over (csrc/lf_hostprep.h: deal_finishers, behind lf_deal_finishers; csrc/lf_tile.h;
DESIGN.md section 3.4d) - host logic, no GPU: per group size the physical rank the deal loads most, recomputed here from the
table lf_deal_table returns; and the deal itself is the one it was before the finisher ranks came (the order of every sum, and
so the bits of lnprob, hang on it)."""
import ctypes
import json
import os

import numpy as np
import pytest

from lumfuncmcmc_amd import capi

VF, COST_BIN, COST_CELL, COST_YOUNGER = 32, 8, 3, 8      # (lf_layout.h; lf_hostprep.h: make_deal)
SHAPES = [(55, 17), (16, 0), (1, 1), (0, 17), (200, 40)]
SHARES = [(0, 1), (1, 2)]


def _table(nc, nb, part, parts):
    lib = capi.load()
    lib.lf_deal_table.restype = ctypes.c_int
    lib.lf_deal_table.argtypes = [ctypes.c_int] * 4 + [ctypes.POINTER(ctypes.c_int32), ctypes.c_int64]
    n = lib.lf_deal_table(nc, nb, part, parts, None, 0)
    assert n == 2 * (VF + 1) + nc + nb
    t = np.empty(n, dtype=np.int32)
    assert lib.lf_deal_table(nc, nb, part, parts, t.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), n) == n
    return t


@pytest.mark.parametrize("part,parts", SHARES)
@pytest.mark.parametrize("nc,nb", SHAPES)
def test_the_finisher_is_the_rank_the_deal_loads_most(nc, nb, part, parts):
    t = _table(nc, nb, part, parts)
    lst = t[2 * (VF + 1):]
    vcost = np.zeros(VF, dtype=np.int64)
    for v in range(VF):
        bins = lst[nc + t[VF + 1 + v]:nc + t[VF + 2 + v]]
        mine = [b for b in bins if not (parts > 1 and b % parts != part)]       # (a share's foreign bins cost nothing)
        vcost[v] = COST_CELL * (t[v + 1] - t[v]) + COST_BIN * len(mine)
    got = capi.deal_finishers(nc, nb, part, parts)
    assert len(got) == 4
    for g, fgroup in enumerate((8, 16, 24, 32)):
        # physical rank r serves the virtual ranks r, r + fgroup, ...; the group's younger half starts behind
        cost = np.array([vcost[r::fgroup].sum() + (COST_YOUNGER if r >= fgroup // 2 else 0) for r in range(fgroup)])
        want = int(np.flatnonzero(cost == cost.max()).max())                    # ties: the highest rank, the youngest
        assert got[g] == want, (fgroup, cost.tolist(), got)
        assert 0 <= got[g] < fgroup


@pytest.mark.parametrize("part,parts", SHARES)
@pytest.mark.parametrize("nc,nb", SHAPES)
def test_the_deal_table_is_what_it_was(nc, nb, part, parts):
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "deal_tables_before_finisher.json")) as f:
        before = json.load(f)["tables"]
    want = np.array(before["%d,%d,%d,%d" % (nc, nb, part, parts)], dtype=np.int32)
    got = _table(nc, nb, part, parts)
    assert got.dtype == want.dtype and got.tobytes() == want.tobytes()


def test_bad_arguments_are_refused():
    with pytest.raises(ValueError):
        capi.deal_finishers(5, 5, grid_part=3, grid_parts=3)
    with pytest.raises(ValueError):
        capi.deal_finishers(-1, 5)
