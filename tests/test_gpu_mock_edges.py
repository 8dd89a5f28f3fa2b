"""The mock catalogues on the device at the scan's tile edges (lf_mock_*, csrc/lf_mock.h): grids of
S = 255, 256, 257 and 513 nodes per axis - a ragged single tile, exactly one tile, a carry into a ragged second tile, and
two carries - against the NumPy twin and against the oracle's own trapezoid sum; and (row, field) pairs without sources at
the start, in the middle and at the end of a batch.  tests/test_mock_edges_cpu.py holds the twin to the same grids."""
import numpy as np
import pytest

import lf_mockproblib as M
import lf_oracle as O
from lumfuncmcmc_amd import mock

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("variant,S", M.EDGE_GRIDS)
def test_device_matches_the_twin_and_piece_b_across_tiles(variant, S):
    inp = M.edge_inputs(variant, S)
    tw, gen = mock.MockTwin(inp), mock.MockGenerator(inp)
    th = M.scaled_rows(tw, variant, (3000.0, 300.0, 5.0))
    rid = np.array([100, 1 << 40, 7], dtype=np.int64)
    m_d, n_d = gen.counts(th, 1234, rid)
    m_h, n_h = tw.counts(th, 1234, rid)
    np.testing.assert_allclose(m_d, m_h, rtol=1e-12, atol=0)
    np.testing.assert_array_equal(n_d, n_h)
    zd, Ld, fd, od = gen.draw(th, 1234, rid)
    zh, Lh, fh, oh = tw.draw(th, 1234, rid)
    np.testing.assert_array_equal(od, oh)
    np.testing.assert_array_equal(fd, fh)
    np.testing.assert_allclose(zd, zh, rtol=0, atol=1e-12)
    np.testing.assert_allclose(Ld, Lh, rtol=0, atol=1e-12)
    # the independent reference for the carry: the oracle's trapezoid sum over the whole grid
    pb = np.array([O.piece_b(inp, O.split_theta(inp, t)) for t in th])
    np.testing.assert_allclose(m_d.sum(axis=1), pb, rtol=1e-12, atol=0)
    edges = np.linspace(41.6, 43.4, 20)
    h = gen.hist(th, edges, 1234, rid)
    np.testing.assert_array_equal(h.sum(axis=2), n_d)
    np.testing.assert_array_equal(h, mock.bin_sources(Ld, od, edges).reshape(h.shape))
    gen.close()


def test_pairs_without_sources_first_in_the_middle_and_last():
    inp = M.edge_inputs("zevol", 257)
    tw, gen = mock.MockTwin(inp), mock.MockGenerator(inp)
    th = M.scaled_rows(tw, "zevol", (0.0, 3000.0, 0.0, 5.0, 0.0))
    m_d, n_d = gen.counts(th, 7)
    m_h, n_h = tw.counts(th, 7)
    assert (m_d[[0, 2, 4]] == 0).all() and (n_d[[0, 2, 4]] == 0).all()
    np.testing.assert_array_equal(n_d, n_h)
    explicit = np.array([[0, 1], [255, 256], [0, 0], [257, 1], [1, 0]], dtype=np.int64)        # a source asked of a row without mass too
    for count in (None, explicit):
        zd, Ld, fd, od = gen.draw(th, 7, count=count)
        zh, Lh, fh, oh = tw.draw(th, 7, count=count)
        np.testing.assert_array_equal(od, oh)
        np.testing.assert_array_equal(np.diff(od), (n_d if count is None else count).ravel())
        np.testing.assert_array_equal(fd, fh)
        np.testing.assert_allclose(zd, zh, rtol=0, atol=1e-12)
        np.testing.assert_allclose(Ld, Lh, rtol=0, atol=1e-12)
    edges = np.linspace(41.6, 43.4, 20)
    h = gen.hist(th, edges, 7)
    zd, Ld, fd, od = gen.draw(th, 7)
    np.testing.assert_array_equal(h.sum(axis=2), n_d)
    assert (h[[0, 2, 4]] == 0).all()
    np.testing.assert_array_equal(h, mock.bin_sources(Ld, od, edges).reshape(h.shape))
    gen.close()
