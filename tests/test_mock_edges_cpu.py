"""The mock catalogues' cumulative sums at the scan's tile edges, host side (lumfuncmcmc_amd/mock.py, csrc/lf_mock.h; DESIGN.md
section 3.11): the twin's stored sums meet the header's contract on real grids - they never decrease, they are flat across
nodes of zero mass, and bisection finds the node a linear search finds - its expected counts are piece B with one, two and
three tiles per column, and (row, field) pairs without sources leave the offsets and histograms of their neighbours alone.
No GPU; tests/test_gpu_mock_edges.py runs the same grids on the device."""
import numpy as np
import pytest

import lf_mockproblib as M
import lf_oracle as O
from lumfuncmcmc_amd import mock, synth


@pytest.mark.parametrize("variant,S", M.CONTRACT_GRIDS)
def test_the_stored_sums_meet_the_contract(variant, S):
    inp = M.edge_inputs(variant, S)
    tw = mock.MockTwin(inp)
    for r, th in enumerate(synth.walkers(variant, 4, seed=5, nf=tw.nf)):
        m = np.swapaxes(tw.masses(th), 1, 2)                     # [f][k][j]
        cdfL, cdfZ, mean = tw._cdfs(th)
        dec, zst = M.contract_violations(m, cdfL)
        dz, zz = M.contract_violations(mock.scan(m)[1], cdfZ)        # (the column totals are cdfZ's masses)
        dis = sum(M.search_disagreements(cdfL[f, k]) for f in range(tw.nf) for k in range(0, S, S // 8))
        dis += sum(M.search_disagreements(cdfZ[f]) for f in range(tw.nf))
        step = np.diff(np.concatenate([np.zeros(cdfL.shape[:-1] + (1,)), cdfL], axis=-1), axis=-1)
        print("%s S = %d row %d: %d steps down, %d zero-mass nodes with a step, %d thresholds where bisection differs (cdfZ: %d, %d);"
              " %d of %d nodes have a mass too small to raise their sum" % (variant, S, r, dec, zst, dis, dz, zz, ((m > 0) & (step == 0)).sum(), m.size))
        assert (dec, zst, dis, dz, zz) == (0, 0, 0, 0, 0)
        # the reported mean is the sum scan's carry, the last stored sum the largest prefix: two roundings of one exact sum,
        # the carry within (8 + T) 2^-53 of it (8 adds in a tile, T = (S - 1) // 256 carries) and every prefix within
        # (9 + T) 2^-53 - so they are within (17 + 2 T) 2^-53 of each other, to first order; nothing makes that one ulp
        T = (S - 1) // M.TILE
        assert np.all(np.abs(mean - cdfZ[:, -1]) <= (17 + 2 * T) * M.U53 * M.SCAN_BOUND * mean)


@pytest.mark.parametrize("variant,S", M.EDGE_GRIDS)
def test_expected_counts_are_piece_b_across_tiles(variant, S):
    inp = M.edge_inputs(variant, S)
    tw = mock.MockTwin(inp)
    th = M.scaled_rows(tw, variant, (3000.0, 300.0, 5.0))
    mean, cnt = tw.counts(th, seed=1234)
    pb = np.array([O.piece_b(inp, O.split_theta(inp, t)) for t in th])
    np.testing.assert_allclose(mean.sum(axis=1), pb, rtol=1e-12, atol=0)
    edges = np.linspace(41.6, 43.4, 20)
    h = tw.hist(th, edges, seed=1234)
    np.testing.assert_array_equal(h.sum(axis=2), cnt)


def test_pairs_without_sources_first_in_the_middle_and_last():
    inp = M.edge_inputs("zevol", 257)
    tw = mock.MockTwin(inp)
    th = M.scaled_rows(tw, "zevol", (0.0, 3000.0, 0.0, 5.0, 0.0))
    mean, cnt = tw.counts(th, seed=7)
    assert (mean[[0, 2, 4]] == 0).all() and (cnt[[0, 2, 4]] == 0).all() and cnt[1].min() > 1000
    z, L, fld, off = tw.draw(th, seed=7)
    np.testing.assert_array_equal(np.diff(off), cnt.ravel())
    np.testing.assert_array_equal(fld, np.repeat(np.tile(np.arange(2), 5), cnt.ravel()))
    alone = tw.draw(th[1:2], seed=7, row_ids=[1])
    np.testing.assert_array_equal(L[off[2]:off[4]], alone[1])
    h = tw.hist(th, np.linspace(41.6, 43.4, 20), seed=7)
    np.testing.assert_array_equal(h.sum(axis=2), cnt)
