"""veffd_partial<FCMIN> and stage 1 of lf_bands<3> / lf_bands<7> element by element against 40-digit references, through
their public entries (tests/lf_postproblib.py has the cases, yardsticks and caps, tests/test_postterms_cpu.py the twins'
figures): lf_veff_draws with one source per bin returns the weight itself, lf_lumfunc_quantiles
with values returns v[r][p].  Also the underflow side of the weights, veffd_quant on +inf values, and lf_veff_draws' order of
summation replayed addition by addition.  Every figure is printed before it is asserted."""
import numpy as np
import pytest

import lf_postproblib as P
from lumfuncmcmc_amd import capi, synth

pytestmark = pytest.mark.gpu


def _bits_equal(got, want):
    """the same bits, NaN where the other has NaN"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape
    gn, wn = np.isnan(got), np.isnan(want)
    np.testing.assert_array_equal(gn, wn)
    bad = got[~gn].view(np.int64) != want[~wn].view(np.int64)
    assert not bad.any(), (np.flatnonzero(bad)[:5], got[~gn][bad][:5], want[~wn][bad][:5])


_values = {}


def _one_per_bin(fcmin, per_source):
    """values[R][N_SRC] of the catalogue with one source per bin (one device call per configuration and process)"""
    key = (fcmin, per_source)
    if key not in _values:
        cat = P.veffd_catalogue(fcmin)
        out, v = capi.veff_draws_device(cat["flux"], cat["field"], cat["vol"] if per_source else P.VOL_ALL, P.PREF0, fcmin,
                                        np.arange(P.N_SRC), P.N_SRC, P.veffd_draws(), q=P.Q)
        v.setflags(write=False)
        _values[key] = (out, v)
    return _values[key]


@pytest.mark.parametrize("per_source", [True, False], ids=["per-source", "shared"])
@pytest.mark.parametrize("fcmin", P.FCMINS)
def test_veffd_weights_element_by_element_against_40_digits(fcmin, per_source):
    """w_i(d_r) on the twelve probe rows (rows 0 .. 256 of two tiles; alpha 0.6, 4.56, 10 and their negatives; sixteen
    distinct Flim in another permutation per row) for up to 170 sources each, f / Flim 1e-3 .. 1e3 with f = Flim, f = ftau and
    their neighbours: max err / yard within max(2, 4 x veff.veff_draws' figure) - alpha > 0 at fcmin 0.1 and 0: twin 1.358
    on 2026-10-20, cap 5.43; alpha > 0 at fcmin 0.3: 5.009, cap 20.0; alpha < 0, under the yardstick with the 1 / d terms:
    1.543, cap 6.17 (lf_postproblib.CAPS).  vol <= 0 gives exactly +0."""
    c = P.case_veffd(fcmin)[per_source]
    got = P.veffd_elements(c, _one_per_bin(fcmin, per_source)[1])
    vol = "per source" if per_source else "shared"
    for al in sorted(set(P.GROUP_ALPHAS)):
        m = dict(c)
        m["exempt"] = np.array([P.probe_alpha(k) != al for k in c["k"]])
        fig, i = P.measure(m, got)
        name = P.cap_name(fcmin, al)
        print("veffd_w alpha %-5g fcmin %-4g vol %-10s device max err / yard %9.3f (cap %g) at %s: got %.17g ref %.17g" %
              (al, fcmin, vol, fig, P.CAPS[name], P.veffd_where(c, i, fcmin), got[i], c["ref"][0][i]))
    assert np.all(got[c["zero"]] == 0.0) and not np.signbit(got[c["zero"]]).any()
    for name, (fig, i) in P.veffd_figures(c, got).items():
        assert fig <= P.CAPS[name], (name, fig, P.veffd_where(c, i, fcmin))


@pytest.mark.parametrize("fcmin", [synth.FCMIN, 0.3])
def test_underflowing_sources_are_inf_where_the_twins_are_and_touch_nothing_else(fcmin):
    """8 sources whose fc^(1/d) is subnormal or 0: +inf exactly where veff.veff_draws has +inf, never a NaN, and the other 56
    sources' values have the bits of the call without the 8"""
    from lumfuncmcmc_amd import veff
    u, d = P.underflow_sources(fcmin), P.veffd_draws()
    n, nb = len(u["flux"]), u["n_base"]
    _, v = capi.veff_draws_device(u["flux"], u["field"], u["vol"], P.PREF0, fcmin, np.arange(n), n, d, q=P.Q)
    _, v0 = capi.veff_draws_device(u["flux"][:nb], u["field"][:nb], u["vol"][:nb], P.PREF0, fcmin, np.arange(nb), nb, d, q=P.Q)
    with np.errstate(all="ignore"):
        tw = veff.veff_draws(u["flux"], u["field"], u["vol"], P.PREF0, fcmin, np.arange(n), n, d)
    print("fcmin %g: +inf per underflowing source, device %s twin %s" % (fcmin, np.isinf(v[:, nb:]).sum(axis=0), np.isinf(tw[:, nb:]).sum(axis=0)))
    assert not np.isnan(v).any() and not np.isnan(v0).any() and np.all(v >= 0.0)
    np.testing.assert_array_equal(np.isinf(v), np.isinf(tw))
    assert np.isinf(v[:, nb:]).any() and np.isfinite(v[:, nb:]).any()
    _bits_equal(v[:, :nb], v0)


def test_quantiles_of_bins_with_inf_rows_are_numpys_bit_for_bit():
    """veffd_quant on values with 0, 1, 41, 128, 129, 216, 256 and 257 of 257 rows +inf: np.percentile / np.median of the
    device's own values, bit for bit, NaN where NumPy has NaN (inf - inf in its _lerp)"""
    q = P.quantile_case()
    n = len(q["flux"])
    out, v = capi.veff_draws_device(q["flux"], q["field"], P.VOL_ALL, P.PREF0, synth.FCMIN, np.arange(n), n, q["draws"], q=P.Q)
    med, v2 = capi.veff_draws_device(q["flux"], q["field"], P.VOL_ALL, P.PREF0, synth.FCMIN, np.arange(n), n, q["draws"],
                                     method=capi.LF_Q_MEDIAN)
    count = np.isinf(v).sum(axis=0)
    print("+inf rows per bin: device %s planned %s\nout =\n%s\nmedian = %s" % (count, q["planned"], out, med))
    assert not np.isnan(v).any() and np.array_equal(count, q["planned"])
    _bits_equal(v2, v)
    with np.errstate(all="ignore"):
        want, wmed = np.percentile(v, P.Q, axis=0), np.median(v, axis=0)[None]
    _bits_equal(out, want)
    _bits_equal(med, wmed)
    assert np.isnan(want).any() and np.isinf(want).any() and np.isfinite(want[:, 0]).all() and np.all(wmed[0, 4:] == np.inf)


@pytest.mark.parametrize("per_source", [True, False], ids=["per-source", "shared"])
@pytest.mark.parametrize("fcmin", [synth.FCMIN, 0.0])
def test_the_order_of_summation_is_the_stated_one(fcmin, per_source):
    """The sources regrouped into bins of 2, 255, 256, 257 and 513, shuffled: values[r][b] has the bits of the one-source values
    added in sorted order within chunks of lf_veff_draws_chunk() from 0.0, the chunks' sums then added in chunk order from 0.0
    (lf_postproblib.replay_sums, a loop over Python floats) - on rows 0, 255 and 256"""
    o, cat = P.order_case(), P.veffd_catalogue(fcmin)
    one = _one_per_bin(fcmin, per_source)[1]
    idx = o["idx"]
    out, v = capi.veff_draws_device(cat["flux"][idx], cat["field"][idx], cat["vol"][idx] if per_source else P.VOL_ALL, P.PREF0, fcmin,
                                    o["bin_of"], o["nbin"], P.veffd_draws(), q=P.Q)
    C = capi.veff_draws_chunk()
    assert C == 256
    for r in P.ORDER_ROWS:
        want = P.replay_sums(one[r][idx], o["bin_of"], o["nbin"], C)
        print("fcmin %g row %d: device %s replay %s" % (fcmin, r, v[r], want))
        assert np.all(np.isfinite(want)) and np.all(want > 0)
        _bits_equal(v[r], want)
    with np.errstate(all="ignore"):
        _bits_equal(out, np.percentile(v, P.Q, axis=0))


@pytest.mark.parametrize("np_rec", [3, 7])
def test_bands_values_element_by_element_against_40_digits(np_rec):
    """bands_eval<3> / bands_eval<7> from the record as the device receives it: t = logL - L* from -6 to 2.8 and where 10^t
    crosses 1, 10, 100 and 700, alpha + 1 in {-2.5, -1, -0.5, 0, 0.5, 1.5}, and for the z-evolving record quadratics that cancel to
    below 1e-3 of their largest term.  max err / yard within max(2, 4 x lfbands.lf_values' figure) (twin 0.552 / 0.745 on
    2026-10-20: caps 2.21 / 2.98); a point whose 40-digit value is below the smallest normal number within 4 x 2^-1074."""
    c = P.case_bands(np_rec)
    _, v = capi.lumfunc_quantiles(c["variant"], c["draws"], c["logL"], z=c["z"], q=(16.0, 50.0, 84.0), values=True)
    got = P.bands_elements(c, v)
    name = "bands_v%d" % np_rec
    fig, i = P.measure(c, got)
    sub = P.sub_errors(c, got)
    print("%s device max err / yard %7.3f (cap %g) at %s: got %.17g ref %.17g; %d points below the smallest normal number, max |err| %g x 2^-1074" %
          (name, fig, P.CAPS[name], P.bands_where(c, i), got[i], c["ref"][0][i], len(sub), sub.max() / P.TINY))
    assert np.all(sub <= P.ABS_SUB), sub / P.TINY
    assert fig <= P.CAPS[name], (fig, P.bands_where(c, i))
