"""veffd_partial_zmax's volume per (source, draw) against voltable.VolumeTable.eval, bit for bit and element by element
(tests/lf_volproblib.py has the cases and what makes them exact; tests/test_volterms_cpu.py holds the table to 40 digits and
asserts what the cases cover).

Every call has one source per bin, so values[r][i] is the weight of pair (i, r) itself, and 257 draws: lanes 0, 63, 64, 255 of
the first tile and lane 0 of a second.  Every row of every call is asserted, to the bit (a -0 for a +0 fails):
  * fcmin = 0 and flux = Flim: values = 2 fl(1 / fl(pref0 eval(D))), +0 where eval gives 0 - with c = 2^j exact and D on the
    lattice, with a generic fmin and D the one rounded product dist * (1 / sqrt(fmin)), and with fmin = 0 entries mixed in;
  * fcmin = 0.1: values = lf_veff_draws' with the per-source vol = eval(D).
Each case prints the count of elements on each search path and at each clamp (the host replay's)."""
import numpy as np
import pytest

import lf_volproblib as P
from lumfuncmcmc_amd import capi

pytestmark = pytest.mark.gpu

ALL = P.TABLES + ("one",)


def _bits_equal(got, want):
    got, want = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(want, dtype=np.float64)
    assert got.shape == want.shape
    assert not np.isnan(got).any() and not np.isnan(want).any()
    bad = got.view(np.int64) != want.view(np.int64)
    assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[:5].tolist(), got[bad][:5], want[bad][:5])


def _device(c, tab, fcmin):
    n = len(c["dist"])
    assert n <= P.MAXBIN and c["draws"].shape[0] == P.R
    out, v = capi.veff_draws_zmax_device(c["flux"], c["field"], c["dist"], P.PREF0, fcmin, np.arange(n), n, c["draws"], c["fmin"], tab, q=P.Q)
    assert v.shape == (P.R, n)
    _bits_equal(out, np.percentile(v, P.Q, axis=0))
    return v


@pytest.mark.parametrize("nf", [1, 8, 9, 16])
@pytest.mark.parametrize("name", ALL)
def test_exact_c_on_the_lattice_gives_evals_bits(name, nf):
    """both instantiations on both sides of VEFFZ_FEW, sources in field nf - 1; "one": the single record's clamps and sweep"""
    tab = P.table(name)[0]
    for call in range(len(P.chunks(name))):
        c = P.exact_case(name, nf, call)
        print(P.counts_line("%s nf %d call %d, on the lattice" % (name, nf, call), P.counts(tab, c["D"][c["on"]])))
        print(P.counts_line("%s nf %d call %d, every pair" % (name, nf, call), P.counts(tab, c["D"])))
        want = P.weight(tab, c["D"])
        assert (want[c["on"]] > 0).any() and (want == 0).any()
        _bits_equal(_device(c, tab, 0.0), want)


@pytest.mark.parametrize("nf", [1, 9])
@pytest.mark.parametrize("name", P.TABLES)
def test_a_generic_fmin_gives_evals_bits_at_the_rounded_product(name, nf):
    tab = P.table(name)[0]
    c = P.generic_case(name, nf)
    k = P.counts(tab, c["D"])
    print(P.counts_line("%s nf %d, generic fmin" % (name, nf), k))
    assert k["below_2pc"] >= 0.01 * k["n"]
    _bits_equal(_device(c, tab, 0.0), P.weight(tab, c["D"]))


@pytest.mark.parametrize("nf", [5, 12])
@pytest.mark.parametrize("name", P.TABLES)
def test_with_fcmin_the_values_are_lf_veff_draws_bits_at_evals_volumes(name, nf):
    tab = P.table(name)[0]
    for call in range(len(P.chunks(name))):
        c = P.fcmin_case(name, nf, call)
        print(P.counts_line("%s nf %d call %d, fcmin 0.1 (every row)" % (name, nf, call), P.counts(tab, c["lattice"])))
        n = len(c["dist"])
        vol = tab.eval(c["lattice"])
        want = capi.veff_draws_device(c["flux"], c["field"], vol, P.PREF0, 0.1, np.arange(n), n, c["draws"], q=P.Q)[1]
        assert np.all(want[:, vol > 0] > 0) and np.all(want[:, vol == 0] == 0) and (vol == 0).any() and np.isfinite(want).all()
        _bits_equal(_device(c, tab, 0.1), want)


@pytest.mark.parametrize("name", P.TABLES)
def test_rows_with_and_without_a_cut_and_a_source_at_distance_zero(name):
    """fmin = 0 in some (draw, field) entries: those pairs carry lf_veff_draws' full-volume bits, the others the table's; a
    source with dist = 0 under fmin = 0 (0 inf is NaN) is exactly +0 and moves no other value"""
    tab = P.table(name)[0]
    m = P.mixed_case(name)
    z = P.ZERO_DIST_SOURCE
    plain, zero = m["plain"], m["zero"]
    print(P.counts_line("%s, mixed rows" % name, P.counts(tab, zero["D"])))
    got_plain, got_zero = _device(plain, tab, 0.0), _device(zero, tab, 0.0)
    _bits_equal(got_plain, P.weight(tab, plain["D"]))
    _bits_equal(got_zero, P.weight(tab, zero["D"]))
    n = len(plain["dist"])
    full = capi.veff_draws_device(plain["flux"], plain["field"], float(tab.v_total), P.PREF0, 0.0, np.arange(n), n, plain["draws"], q=P.Q)[1]
    cut = (plain["fmin"] == 0.0)[:, plain["field"]]
    assert cut.any() and (~cut).any() and np.all(full > 0)
    _bits_equal(got_plain[cut], full[cut])
    assert np.all(got_zero[:, z].view(np.int64) == 0)                              # +0, not -0
    assert np.all(got_plain[:, z] > 0)
    _bits_equal(np.delete(got_zero, z, axis=1), np.delete(got_plain, z, axis=1))
