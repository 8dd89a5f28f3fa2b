"""The element-wise probes of veffd_partial and of the bands' stage 1 without a GPU (tests/lf_postproblib.py; DESIGN.md section
3.28): every generator yields what it promises, the conditions on the references hold, the twins (veff.veff_draws,
lfbands.lf_values) go through the same `measure` as the device will and their figures are pinned to 1 %, and the stated order
of summation is replayed on the twin's per-source weights."""
import math

import numpy as np

import lf_postproblib as P
from lumfuncmcmc_amd import synth, veff


def test_the_draws_and_catalogues_cover_what_they_promise():
    d = P.veffd_draws()
    assert d.shape == (257, 17) and set(P.PROBE_ROWS) >= {0, 1, 63, 64, 127, 128, 191, 192, 254, 255, 256} and len(set(P.PROBE_ROWS)) == 12
    lo, hi = synth.FLIM_LIMS[0] * 1e-17, synth.FLIM_LIMS[1] * 1e-17
    rows = d[list(P.PROBE_ROWS)]
    assert {0.6, 4.56, 10.0} <= set(rows[:, 16]) and (rows[:, 16] < 0).any()
    for k, r in enumerate(rows):
        assert len(set(r[:16])) == 16 and r[:16].min() >= lo * (1 - 1e-15) and r[:16].max() <= hi * (1 + 1e-15)
        assert np.array_equal(np.sort(r[:16]), np.sort(rows[0, :16]))
        assert all(not np.array_equal(r[:16], q[:16]) for q in rows[:k])           # another permutation on every row
    fill = np.delete(d, list(P.PROBE_ROWS), axis=0)
    assert np.all(np.abs(fill[:, 16] - synth.ALPHA_C) < 0.6) and np.all(np.abs(fill[:, :16] / 1e-17 - np.tile(synth.FLIM, 4)[:16]) < 0.6)
    assert set(P.FCMINS) >= {synth.FCMIN, 0.0} and any(0.0 < f < 0.5 and f != synth.FCMIN for f in P.FCMINS)
    for fm in P.FCMINS:
        cat = P.veffd_catalogue(fm)
        assert len(cat["flux"]) <= 1024 and set(cat["field"]) == set(range(16))
        x = cat["flux"] / cat["flim_laid"]
        keep = ~cat["redrawn"]
        assert x[keep].min() <= 1.0000001e-3 and x.max() >= 0.9999999e3 and np.sum(x == 1.0) >= 12
        assert np.sum(cat["flux"] == np.nextafter(cat["flim_laid"], 0.0)) >= 12 and np.sum(cat["flux"] == np.nextafter(cat["flim_laid"], 1.0)) >= 12
        assert np.sum(cat["vol"] <= 0) == len(P.ZERO_VOL) and {0.0, -1.0} <= set(cat["vol"])
        assert not cat["redrawn"][cat["edge"]].any() or fm > 0
        print("fcmin %-4g: %d of %d sources drawn again (%.2f %%), by group %s" % (
            fm, cat["redrawn"].sum(), len(x), 100.0 * cat["redrawn"].mean(), [int(cat["redrawn"][cat["group"] == g].sum()) for g in range(6)]))
        # the condition on the lattice, per catalogue: at most 5 % drawn again (none where the rule does not apply)
        assert cat["redrawn"].sum() <= 0.05 * len(x) and (fm > 0 or not cat["redrawn"].any()), (fm, cat["redrawn"].sum())


def test_the_veffd_references_are_what_the_yardstick_assumes():
    for fm in P.FCMINS:
        for ps, c in P.case_veffd(fm).items():
            ref, n = c["ref"][0], len(c["yard"])
            assert n == 12 * P.PER_ROW - c["dropped"] and np.all(np.isfinite(ref)) and np.all(c["yard"] > 0)
            # an element is left out only on a source's partner row, and only with fcmin > 0: at most 5 % of the elements
            assert c["dropped"] <= 0.05 * 12 * P.PER_ROW and (fm > 0 or c["dropped"] == 0), (fm, c["dropped"])
            cat = P.veffd_catalogue(fm)
            own = cat["krow"][c["src"]] == c["k"]
            assert np.all(ref[c["zero"]] == 0.0) and np.all(ref[~c["zero"]] > np.finfo(float).tiny)
            assert c["zero"].sum() == (2 * len(P.ZERO_VOL) if ps else 0)
            for row in P.PROBE_ROWS:
                assert (c["row"][own] == row).sum() == P.PER_ROW // 2 and (c["row"] == row).sum() >= 0.8 * P.PER_ROW
            if ps:
                print("fcmin %-4g: %d elements of %d carry a reference, %d left out on a partner row" % (fm, n, 12 * P.PER_ROW, c["dropped"]))


def numpy_figures():
    figs = {}
    for fm in P.FCMINS:
        for ps, c in P.case_veffd(fm).items():
            for k, v in P.veffd_figures(c, c["np"]).items():
                if k not in figs or v[0] > figs[k][0]:
                    figs[k] = v + (P.veffd_where(c, v[1], fm) + " fcmin %g" % fm,)
    for k, n in (("bands_v3", 3), ("bands_v7", 7)):
        c = P.case_bands(n)
        fig, i = P.measure(c, c["np"])
        figs[k] = (fig, i, P.bands_where(c, i))
    return figs


def test_numpy_figures_behind_the_caps():
    """max err / yardstick of the twins through lf_postproblib.measure: the GPU tests' caps are max(2, 4 x these); a figure that
    has moved by more than 1 % from the recorded one fails here"""
    figs = numpy_figures()
    assert set(figs) == set(P.CAPS) == set(P.NUMPY_FIGS)
    for k, (fig, i, where) in figs.items():
        print("numpy %-12s max err / yard %10.4f (recorded %g, cap %g) at %s" % (k, fig, P.NUMPY_FIGS[k], P.CAPS[k], where))
    for k, (fig, i, where) in figs.items():
        assert math.isfinite(fig) and abs(fig / P.NUMPY_FIGS[k] - 1.0) <= 0.01, (k, fig, P.NUMPY_FIGS[k])
        assert abs(P.CAPS[k] / P.cap_from(P.NUMPY_FIGS[k]) - 1.0) <= 0.005, (k, P.CAPS[k])


def test_the_twin_keeps_zero_volumes_at_zero_and_sees_a_wrong_field_row():
    """vol <= 0 is exactly +0 in the twin, and the metric sees a Flim read from the next field's row (the draws' permutations
    are there for that) - on the twin, no device code is mutated here"""
    for fm in (synth.FCMIN, 0.0):
        c = P.case_veffd(fm)[True]
        assert np.all(c["np"][c["zero"]] == 0.0) and not np.signbit(c["np"][c["zero"]]).any()
        cat, d = P.veffd_catalogue(fm), P.veffd_draws()
        with np.errstate(all="ignore"):
            w = veff.veff_draws(cat["flux"], (cat["field"] + 1) % P.NF, cat["vol"], P.PREF0, fm, np.arange(P.N_SRC), P.N_SRC, d[list(P.PROBE_ROWS)])
        figs = P.veffd_figures(c, np.nan_to_num(w[c["k"], c["src"]], posinf=1e308))
        assert figs["veffd_w"][0] > 1e3 * P.CAPS["veffd_w"] and figs["veffd_w_neg"][0] > 1e3 * P.CAPS["veffd_w_neg"], figs


def test_the_underflow_sources_and_the_quantile_rows():
    d = P.veffd_draws()
    for fm in (synth.FCMIN, 0.3):
        u = P.underflow_sources(fm)
        n = len(u["flux"])
        with np.errstate(all="ignore"):
            w = veff.veff_draws(u["flux"], u["field"], u["vol"], P.PREF0, fm, np.arange(n), n, d)
        assert n == u["n_base"] + 8 and not np.isnan(w).any()
        inf = np.isinf(w[:, u["n_base"]:])
        assert np.all(w[:, u["n_base"]:][inf] > 0) and inf.sum(axis=0).min() > 50 and inf[:, -1].all() and (~inf).any()
    q = P.quantile_case()
    assert np.array_equal(q["count"], q["planned"]) and q["count"][0] == 0 and q["count"][-1] == P.R and q["draws"].shape == (P.R, P.NF + 1)


def test_the_summation_rule_replayed_on_the_twin():
    """lf_postproblib.replay_sums on the twin's per-source weights: every source of a bin is added exactly once (against fsum
    to n / 2 roundings of the sum), a chunk boundary changes the association (the rule is not the serial sum), and the bins
    have the sizes the rule is tested at"""
    o = P.order_case()
    sizes = np.bincount(o["bin_of"][(o["bin_of"] >= 0) & (o["bin_of"] < o["nbin"])], minlength=o["nbin"])
    assert tuple(sizes) == (2, 255, 256, 257, 513) and len(o["idx"]) == sum(sizes) + 6 and set(o["idx"]) == set(o["eligible"]) and len(o["eligible"]) > 400
    assert not np.array_equal(np.sort(o["bin_of"]), o["bin_of"])                    # shuffled: the stable sort decides
    moved = 0
    for fm in (synth.FCMIN, 0.0):
        tw = P.veffd_twin(fm, True)
        for k in (0, 9, 10):                                                            # rows 0, 255, 256
            w = tw[k][o["idx"]]
            got = P.replay_sums(w, o["bin_of"], o["nbin"], 256)
            for b in range(o["nbin"]):
                exact = math.fsum(w[o["bin_of"] == b])
                assert abs(got[b] - exact) <= 0.5 * sizes[b] * 2.0 ** -53 * exact, (fm, k, b)
            serial = P.replay_sums(w, o["bin_of"], o["nbin"], 1 << 20)
            assert np.array_equal(got[:3], serial[:3])                                  # up to one chunk: the serial sum
            moved += int(np.sum(got[3:] != serial[3:]))
    assert moved > 0


def test_the_band_lattices_cover_what_they_promise():
    for n in (3, 7):
        c = P.case_bands(n)
        Rn, Pn = c["draws"].shape[0], len(c["logL"])
        assert Rn <= 64 and Pn <= 512 and c["draws"].shape[1] == n and len(c["yard"]) == Rn * P.NPTS
        assert set(c["draws"][:, -1] + 1.0) == set(P.C1S)
        t = c["t"]
        assert t.min() <= -5.99 and 2.79 <= np.max(t[t < 2.81]) and t.max() > 2.845
        for r in range(Rn):
            tr = t[c["r"] == r]
            for x in (1.0, 10.0, 100.0, 700.0):                                        # both sides of every crossing
                assert (10.0 ** tr < x).any() and (10.0 ** tr > x).any() and np.min(np.abs(tr - math.log10(x))) < 1e-9
            if n == 3:
                assert (tr == 0.0).sum() >= 1 and np.sort(np.abs(tr[tr != 0.0]))[:2].max() <= np.spacing(c["draws"][r, 0])
        # the condition on the references: at most 5 % below the smallest normal number, each of them one whose yardstick is
        # below 2^-1074 - the absolute bound asks nothing that a correctly rounded evaluation cannot give
        assert 0 < c["sub"].sum() <= 0.05 * len(c["sub"]), c["sub"].sum()
        assert np.all(c["yard"][c["sub"]] <= 2.0 ** -1074) and np.all(np.isfinite(c["ref"][0])) and np.all(c["ref"][0][~c["sub"]] > 0)
        assert np.all(P.sub_errors(c, c["np"]) <= P.ABS_SUB)
        if n == 7:
            assert c["z"].min() == 1.1 and c["z"].max() == 2.0
            assert np.all(c["cancel"][c["r"] >= 6] <= 1e-3) and c["cancel"][c["r"] >= 6].max() > 5e-4


def test_the_band_metric_sees_a_wrong_record_slot():
    """bands_eval<7> with the record's last but one slot for alpha + 1, stated in NumPy: far beyond the cap"""
    from lumfuncmcmc_amd import lfbands
    c = P.case_bands(7)
    wrong = c["draws"].copy()
    wrong[:, 6] = wrong[:, 5] - 1.0
    with np.errstate(all="ignore"):
        v = lfbands.lf_values("zevol", wrong, c["logL"], c["z"])
    got = np.nan_to_num(P.bands_elements(c, v), nan=0.0, posinf=1e308)
    assert P.measure(c, got)[0] > 1e6 * P.CAPS["bands_v7"]
