"""The volume table against 40 digits, and what the per-element device cases cover, without a GPU (tests/lf_volproblib.py;
DESIGN.md section 3.30).

The table: max |VolumeTable.eval - V40| / V_total over at most 120 lattice points per table is held to voltable.EPS_MAX - the
project's bound on a usable table - and to 4 x the table's own eps, so that VolumeTable.validate, whose yardstick shares
luminosity_distance and the Newton inverse with the table, cannot understate its error by more than the standing margin for
twins.  d_lo, d_hi (4 x 2^-53 relative: the rounding of DL's last product and of its factors) and V_total (EPS_MAX) are held
to the same reference; eval is non-decreasing over the whole lattice.

The coverage: lf_volproblib.search_path replays the kernel's search on the host - its volumes are VolumeTable.eval's bits on
every input used here - and the counts asserted below keep tests/test_gpu_volterms.py from passing on easy inputs: the
neighbour step on the standard table, the bisection on the uneven one, both paths on the three-node one, all 32 z pieces, both
outer clamps, volumes below 1e-9 of the total, and elements where each inner clamp acts."""
import mpmath as mp
import numpy as np
import pytest

import lf_volproblib as P
from lumfuncmcmc_amd import voltable

ALL = P.TABLES + ("one",)
NFS = (1, 8, 9, 16)
LANES = (0, 63, 64, 255, 256)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@pytest.mark.parametrize("name", ALL)
def test_the_lattice_holds_what_it_promises(name):
    tab = P.table(name)[0]
    L, p = P.lattice(name), P.parts(name)
    e = tab.edges()
    zb = tab.d_lo + np.arange(1, voltable.NPIECE) / tab.head[3]
    nodes = np.concatenate([tab.rec[:, 0], [tab.d_hi]])
    kept = nodes[np.isin(nodes, L)]
    assert len(zb) == 31 and np.isin(zb, e).all()
    for d in (zb, kept):                                                       # with both neighbouring doubles
        assert np.isin(d, L).all() and np.isin(np.nextafter(d, -np.inf), L).all() and np.isin(np.nextafter(d, np.inf), L).all()
    if name == "standard":
        assert len(L) <= P.MAXBIN and len(P.chunks(name)) == 1 and len(kept) >= 150
        assert kept[0] == tab.d_lo and kept[-1] == tab.d_hi
        assert np.diff(np.searchsorted(nodes, kept)).max() <= 12               # spread over the records: no gap above 12 of 2486
    else:
        assert len(kept) == len(nodes) and np.isin(e, L).all()
    for d in (0.5 * tab.d_lo, 2.0 * tab.d_hi, tab.d_lo, tab.d_hi, np.nextafter(tab.d_lo, 0.0), np.nextafter(tab.d_lo, np.inf),
              np.nextafter(tab.d_hi, 0.0), np.nextafter(tab.d_hi, np.inf)):
        assert d in L
    u_top = (np.nextafter(tab.d_hi, 0.0) - tab.head[0]) * tab.head[3]
    assert 32.0 - 1e-13 < u_top <= 32.0                                        # u rounds to 31.999... (or 32: the min() holds)
    assert len(p["small"]) == 14 and np.all(p["small"] > tab.d_lo) and p["small"].max() <= 1.0100001 * tab.d_lo
    assert np.isin(p["small"], L).all() and len(p["uniform"]) >= 150
    assert all(len(c) <= P.MAXBIN for c in P.chunks(name)) and sum(len(c) for c in P.chunks(name)) == len(L)
    assert tab.d_hi < 2.0 * tab.d_lo                                           # exact_case's off-lattice rows are at a clamp


@pytest.mark.parametrize("name", ALL)
def test_the_replay_of_the_search_gives_evals_bits_and_covers_the_paths(name):
    tab = P.table(name)[0]
    L = P.lattice(name)
    uni = np.random.default_rng(1).uniform(tab.d_lo, tab.d_hi, 20000)
    every = np.concatenate([L, uni, [np.nan, 0.0, np.inf]])
    s = P.search_path(tab, every)
    assert np.array_equal(_bits(s["V"]), _bits(tab.eval(every)))
    inside = s["outer"] == 0
    assert np.all(s["path"][inside] >= 0) and np.all(s["path"][~inside] == -1) and s["steps"].max() <= 31
    rk = tab.rec[s["k"][inside]]
    assert np.all((rk[:, 0] <= every[inside]) & (every[inside] < rk[:, 1]))       # the record found holds D
    c, cu = P.counts(tab, L), P.counts(tab, uni)
    print(P.counts_line(name + " lattice", c))
    print(P.counts_line(name + " 20000 uniform", cu))
    assert c["pieces"] == 32 and c["lower"] >= 3 and c["upper"] >= 3 and c["tiny"] >= 5 and c["below_2pc"] >= 14
    assert c["guess"] + c["neighbour"] + c["bisect"] == c["in_table"]
    if name == "standard":
        assert cu["guess"] == 20000                       # uniform D never leave the first guess: the edges do
        assert c["neighbour"] >= 0.2 * c["in_table"] and c["bisect"] == 0
        assert c["inner_lo"] >= 10 and c["inner_hi"] >= 10                    # both inner clamps act on this lattice
    elif name == "uneven":
        assert c["bisect"] >= 0.5 * c["in_table"] and cu["bisect"] >= 0.5 * 20000 and c["guess"] >= 1 and c["neighbour"] >= 1
        assert c["inner_lo"] >= 10 and c["inner_hi"] >= 10
    elif name == "three":
        assert len(tab.rec) == 2 and tab.head[5] == 0.0
        assert min(c["guess"], c["neighbour"]) >= 0.25 * c["in_table"] and min(cu["guess"], cu["neighbour"]) >= 0.25 * 20000
    else:
        assert len(tab.rec) == 1 and c["guess"] == c["in_table"]


@pytest.mark.parametrize("name", ALL)
def test_the_table_against_40_digits(name):
    tab, _, zmin, zmax = P.table(name)
    ref = P.ref40(name)
    d, v40 = P.ref_volumes(name)
    assert 100 <= len(d) <= P.NREF
    s = P.search_path(tab, d)
    assert len(set(s["piece"][s["outer"] == 0])) == 32 and (s["outer"] == -1).sum() >= 2 and (s["outer"] == 1).sum() >= 2
    ev = tab.eval(d)
    with mp.workdps(40):
        vt = mp.mpf(float(tab.v_total))
        err = np.array([float(abs(mp.mpf(float(e)) - v) / vt) for e, v in zip(ev, v40)])
        e_lo = float(abs(mp.mpf(float(tab.d_lo)) / ref.dl(zmin) - 1))
        e_hi = float(abs(mp.mpf(float(tab.d_hi)) / ref.dl(zmax) - 1))
        e_tot = float(abs(vt / ref.volume_to(zmax) - 1))
        # (d_lo and d_hi are rounded images: the reference's volume next to them is within a rounding of the clamp, not on it)
        assert v40[0] == 0 and d[0] == 0.5 * tab.d_lo and v40[-1] == ref.volume_to(zmax) and d[-1] == 2.0 * tab.d_hi
    i = int(np.argmax(err))
    print("%-8s %d records, %d points: max |eval - V40| / V_total %.3e at D = %.17g (eps %.3e, EPS_MAX %g); d_lo %.2e d_hi %.2e "
          "relative, V_total %.2e" % (name, len(tab.rec), len(d), err[i], d[i], tab.eps, voltable.EPS_MAX, e_lo, e_hi, e_tot))
    assert err.max() <= voltable.EPS_MAX
    assert err.max() <= 4.0 * tab.eps
    assert e_lo <= 4.0 * 2.0 ** -53 and e_hi <= 4.0 * 2.0 ** -53
    assert e_tot <= voltable.EPS_MAX


@pytest.mark.parametrize("name", ALL)
def test_eval_does_not_decrease_over_the_lattice(name):
    tab = P.table(name)[0]
    L = P.lattice(name)
    v = tab.eval(L)
    assert np.all(np.diff(L) > 0) and np.all(np.diff(v) >= 0)
    assert v[0] == 0.0 and v[-1] == tab.v_total and np.all(v[L > tab.d_lo] > 0)


def _on_lattice_counts(name, nf):
    tab = P.table(name)[0]
    tot = None
    for call in range(len(P.chunks(name))):
        c = P.exact_case(name, nf, call)
        k = P.counts(tab, c["D"][c["on"]])
        tot = k if tot is None else {key: (max(v, k[key]) if key in ("pieces", "max_steps") else v + k[key]) for key, v in tot.items()}
        assert c["on"].mean() >= 0.45 and all(c["on"][r].mean() >= 0.4 for r in LANES)
        assert (c["field"] == nf - 1).mean() >= 0.45 and set(c["field"]) == set(range(nf))
        cf = 1.0 / np.sqrt(c["fmin"])
        assert set(np.log2(cf).ravel()) <= {0.0, 1.0, 2.0, 3.0} and (nf == 1 or np.any(cf[:, 0] != cf[:, nf - 1]))
        assert np.any(cf[:-1] != cf[1:]) and (c["draws"][:, nf] > 0).any() and (c["draws"][:, nf] < 0).any()
        assert np.all(c["draws"][:, :nf] == c["draws"][0, :nf]) and np.array_equal(c["flux"], c["draws"][0, :nf][c["field"]])
    return tot


@pytest.mark.parametrize("name", ALL)
def test_the_exact_cases_reach_the_lattice_on_every_lane(name):
    """fmin = 4^-j: the device's D is the lattice's double on about half of the rows of every source - the rows of lanes 0,
    63, 64, 255 and of the second tile among them - and the paths of the lattice are all walked there"""
    for nf in NFS:
        k = _on_lattice_counts(name, nf)
        print(P.counts_line("%s nf %d, on the lattice" % (name, nf), k))
        assert k["pieces"] == 32 and k["lower"] >= 1 and k["upper"] >= 1 and k["tiny"] >= 1
        if name == "standard":
            assert k["neighbour"] >= 0.2 * k["in_table"] and k["inner_lo"] >= 1 and k["inner_hi"] >= 1
        elif name == "uneven":
            assert k["bisect"] >= 0.5 * k["in_table"]
        elif name == "three":
            assert min(k["guess"], k["neighbour"]) >= 0.25 * k["in_table"]


@pytest.mark.parametrize("name", P.TABLES)
def test_the_generic_and_mixed_cases_graze_the_lower_clamp(name):
    tab = P.table(name)[0]
    for nf in (1, 9):
        c = P.generic_case(name, nf)
        k = P.counts(tab, c["D"])
        print(P.counts_line("%s nf %d, generic fmin" % (name, nf), k))
        # the pairs tests/test_gpu_veffzmax.py moves away: at least 1 % of all, and both outer clamps
        assert k["below_2pc"] >= 0.01 * k["n"] and k["lower"] >= 0.05 * k["n"] and k["upper"] >= 0.02 * k["n"] and k["pieces"] == 32
        assert np.all((c["fmin"] >= 2.7e-17) & (c["fmin"] <= 3.3e-17))
        # the rounded product is not the quotient: the replay has to use the device's form
        q = c["dist"][None, :] / np.sqrt(c["fmin"])[:, c["field"]]
        assert (q != c["D"]).mean() > 0.1
    m = P.mixed_case(name)
    z = P.ZERO_DIST_SOURCE
    assert np.isnan(m["zero"]["D"][:, z]).all() and np.isinf(m["plain"]["D"][:, z]).all() and m["zero"]["dist"][z] == 0.0
    assert not np.isnan(np.delete(m["zero"]["D"], z, axis=1)).any()
    cut = m["plain"]["fmin"] == 0.0
    assert 0.2 < cut.mean() < 0.5 and cut[:, 2].all() and (~cut).any(axis=0)[[0, 1, 3, 4]].all()
    assert np.all(tab.eval(m["zero"]["D"][:, z]) == 0.0)
