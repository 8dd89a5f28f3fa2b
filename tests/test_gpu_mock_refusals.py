"""The order in which the nine mock entries of the C ABI refuse (lf_mock_draw, _draw_err, _draw_cut, lf_mock_hist, _hist_err,
_hist_cut, lf_mock_hist2, _hist2_err, _hist2_cut; DESIGN.md sections 3.11, 3.23, 3.32, 3.35).  Every case passes two faults at
once and asserts on the whole message of the one that is checked first, that the return is LF_ERR_ARG, and that no array the
call could write to was touched.  After the handle, every entry checks R, then a NULL theta, then a theta that is not finite;
then, each in its own order:
    lf_mock_draw       NULL count, count out of range, NULL outputs (only when the total is above 0)
    lf_mock_draw_err   no error model, then as lf_mock_draw
    lf_mock_hist       nbins, "edges or hist is NULL", the edges' order
    lf_mock_hist_err   no error model, then as lf_mock_hist
    lf_mock_hist_cut   no error model, no band, nbins, "edges, hist or kept is NULL", the edges' order
    lf_mock_draw_cut   no error model, no band, "n_cand or mean is NULL", cap < 0, NULL outputs (only when cap > 0)
    lf_mock_hist2*     no error model (_err, _cut), no band (_cut), nz < 1, nl < 1, the slot count, nz and nl above their limit,
                       NULL arguments, z_edges' order, edges' order, count out of range
Every refusal comes before the first launch: the file runs no kernel.  One row on lf_mockcutlib's smallest inputs."""
import ctypes

import numpy as np
import pytest

import lf_mockcutlib as K
from lumfuncmcmc_amd import capi, mock, synth

pytestmark = pytest.mark.gpu
VARIANT, S, SEED = "fixcomp", 23, 1234
NF = K.NF
FILL = -77                    # what every output array holds before a call
NO_MODEL = "no error model is set (lf_mock_set_error_model)"
NO_BAND = "no cut band is set (lf_mock_set_cut_band, after lf_mock_set_error_model)"
R_MSG, TH_NULL, TH_NAN = "R must be >= 1", "theta is NULL", "row 0: theta is not finite"
NBINS = "nbins must be in 1..%d" % mock.MAX_BINS
NZ, NL = "nz must be in 1..%d" % mock.MAX_BINS, "nl must be in 1..%d" % mock.MAX_BINS
ORDER = "edges must be finite and non-decreasing"
COUNT_RANGE = "row 0 field 0: count out of range"


@pytest.fixture(scope="module")
def gens():
    """the three states of a generator: no error model, a model without a band, model and band"""
    inp = K.inputs(VARIANT, S)
    nodes, sig = K.table(7)
    g = {"none": mock.MockGenerator(inp), "model": mock.MockGenerator(inp), "armed": K.arm(mock.MockGenerator(inp), inp, nodes, sig)}
    g["model"].set_error_model(nodes, sig)
    yield g
    for v in g.values():
        v.close()


def _call(gen, entry, **o):
    """One call of `entry` with good arguments but for the overrides `o`; a value of None passes NULL.  Returns (rc, message,
    the arrays the call might have written)."""
    th = synth.walkers(VARIANT, 1, seed=5, nf=NF)
    if isinstance(o.get("theta"), str):               # "nan"
        o["theta"] = np.full_like(th, np.nan)
    good = np.linspace(40.0, 45.0, 4096)              # long enough for any bin count a case passes
    cap = o.get("cap", 6)
    args = {"theta": th, "R": 1, "count": np.array([[2, 1]], dtype=np.int64), "nbins": 5, "edges": good, "nz": 3, "z_edges": good - 38.0,
            "nl": 5, "cap": cap, "hist": np.full(NF * 5 * 7, FILL, dtype=np.int64), "kept": np.full(NF, FILL, dtype=np.int64),
            "n_cand": np.full(2 * NF, FILL, dtype=np.int64), "mean": np.full(2 * NF, float(FILL))}
    for k in ("z", "L", "Lobs", "sg"):
        args[k] = np.full(6, float(FILL))
    for k in ("fld", "keep"):
        args[k] = np.full(6, FILL, dtype=np.int32)
    if o.pop("outputs", "") is None:
        o.update({k: None for k in ("z", "L", "Lobs", "sg", "fld", "keep")})
    args.update(o)
    a = dict(args)
    P = lambda k: capi._ptr(a[k])                                                                     # noqa: E731
    I = lambda k: a[k].ctypes.data_as(capi._c_int64_p) if a[k] is not None else None                   # noqa: E731
    J = lambda k: a[k].ctypes.data_as(ctypes.POINTER(ctypes.c_int32)) if a[k] is not None else None    # noqa: E731
    head = (gen._h, P("theta"), a["R"], None, SEED)
    tail = {"lf_mock_draw": lambda: (I("count"), P("z"), P("L"), J("fld")),
            "lf_mock_draw_err": lambda: (I("count"), P("z"), P("L"), P("Lobs"), P("sg"), J("fld")),
            "lf_mock_draw_cut": lambda: (a["cap"], P("z"), P("L"), P("Lobs"), P("sg"), J("fld"), J("keep"), I("n_cand"), P("mean"), I("kept")),
            "lf_mock_hist": lambda: (a["nbins"], P("edges"), I("hist")),
            "lf_mock_hist_err": lambda: (a["nbins"], P("edges"), I("hist")),
            "lf_mock_hist_cut": lambda: (a["nbins"], P("edges"), I("hist"), I("kept")),
            "lf_mock_hist2": lambda: (I("count"), a["nz"], P("z_edges"), a["nl"], P("edges"), I("hist")),
            "lf_mock_hist2_err": lambda: (I("count"), a["nz"], P("z_edges"), a["nl"], P("edges"), I("hist")),
            "lf_mock_hist2_cut": lambda: (a["nz"], P("z_edges"), a["nl"], P("edges"), I("hist"), I("kept"))}[entry]()
    rc = getattr(gen._lib, entry)(*head, *tail)
    outs = [a[k] for k in ("hist", "kept", "n_cand", "mean", "z", "L", "Lobs", "sg", "fld", "keep") if a[k] is not None]
    return rc, gen._lib.lf_mock_last_error(gen._h).decode(), outs


REV = np.linspace(45.0, 40.0, 4096)                   # edges in falling order
NEG = np.array([[-1, 1]], dtype=np.int64)
BIG = mock.MAX_BINS + 1

# (entry, the generator's state, the two faults, the message of the one checked first)
CASES = []
FIRST = {"lf_mock_draw": ("none", {"count": None}), "lf_mock_draw_err": ("none", {}), "lf_mock_draw_cut": ("none", {}),
         "lf_mock_hist": ("none", {"nbins": 0}), "lf_mock_hist_err": ("none", {}), "lf_mock_hist_cut": ("none", {}),
         "lf_mock_hist2": ("none", {"nz": 0}), "lf_mock_hist2_err": ("none", {}), "lf_mock_hist2_cut": ("none", {})}
for _e, (_s, _f) in FIRST.items():                    # the head all nine share, each against the entry's own first check
    CASES += [(_e, _s, {"R": 0, "theta": None}, R_MSG), (_e, _s, {"R": -3, "theta": "nan"}, R_MSG),
              (_e, _s, dict(_f, theta=None), TH_NULL), (_e, _s, dict(_f, theta="nan"), TH_NAN)]
CASES += [
    ("lf_mock_draw", "none", {"count": None, "outputs": None}, "count is NULL"),
    ("lf_mock_draw", "none", {"count": NEG, "outputs": None}, COUNT_RANGE),
    ("lf_mock_draw", "none", {"z": None, "fld": None}, "z, logL or field is NULL"),
    ("lf_mock_draw_err", "none", {"count": None}, NO_MODEL),
    ("lf_mock_draw_err", "none", {"count": NEG}, NO_MODEL),
    ("lf_mock_draw_err", "none", {"outputs": None}, NO_MODEL),
    ("lf_mock_draw_err", "model", {"count": None, "outputs": None}, "count is NULL"),
    ("lf_mock_draw_err", "model", {"count": NEG, "outputs": None}, COUNT_RANGE),
    ("lf_mock_draw_err", "model", {"Lobs": None, "sg": None}, "z, logL_true, logL_obs, sigma or field is NULL"),
    ("lf_mock_hist", "none", {"nbins": 0, "hist": None}, NBINS),
    ("lf_mock_hist", "none", {"nbins": BIG, "edges": None}, NBINS),
    ("lf_mock_hist", "none", {"nbins": 0, "edges": REV}, NBINS),
    ("lf_mock_hist", "none", {"hist": None, "edges": REV}, "edges or hist is NULL"),
    ("lf_mock_hist_err", "none", {"nbins": 0}, NO_MODEL),
    ("lf_mock_hist_err", "none", {"hist": None}, NO_MODEL),
    ("lf_mock_hist_err", "none", {"edges": REV}, NO_MODEL),
    ("lf_mock_hist_err", "model", {"nbins": 0, "edges": None}, NBINS),
    ("lf_mock_hist_err", "model", {"nbins": BIG, "edges": REV}, NBINS),
    ("lf_mock_hist_err", "model", {"hist": None, "edges": REV}, "edges or hist is NULL"),
    ("lf_mock_hist_cut", "none", {"nbins": 0}, NO_MODEL),
    ("lf_mock_hist_cut", "none", {"kept": None}, NO_MODEL),
    ("lf_mock_hist_cut", "model", {"edges": REV}, NO_BAND),
    ("lf_mock_hist_cut", "model", {"nbins": 0}, NO_BAND),
    ("lf_mock_hist_cut", "model", {"kept": None}, NO_BAND),
    ("lf_mock_hist_cut", "armed", {"nbins": 0, "kept": None}, NBINS),
    ("lf_mock_hist_cut", "armed", {"nbins": BIG, "edges": REV}, NBINS),
    ("lf_mock_hist_cut", "armed", {"kept": None, "edges": REV}, "edges, hist or kept is NULL"),
    ("lf_mock_hist_cut", "armed", {"hist": None, "edges": REV}, "edges, hist or kept is NULL"),
    ("lf_mock_draw_cut", "none", {"n_cand": None}, NO_MODEL),
    ("lf_mock_draw_cut", "none", {"cap": -1}, NO_MODEL),
    ("lf_mock_draw_cut", "model", {"n_cand": None}, NO_BAND),
    ("lf_mock_draw_cut", "model", {"cap": -1}, NO_BAND),
    ("lf_mock_draw_cut", "model", {"outputs": None}, NO_BAND),
    ("lf_mock_draw_cut", "armed", {"n_cand": None, "cap": -1}, "n_cand or mean is NULL"),
    ("lf_mock_draw_cut", "armed", {"mean": None, "outputs": None}, "n_cand or mean is NULL"),
    ("lf_mock_draw_cut", "armed", {"cap": -1, "outputs": None}, "cap must be >= 0"),
    ("lf_mock_draw_cut", "armed", {"z": None, "kept": None}, "z, logL_true, logL_obs, sigma, field, keep or kept is NULL"),
    ("lf_mock_hist2", "none", {"nz": 0, "hist": None}, NZ),
    ("lf_mock_hist2", "none", {"nz": 0, "nl": 0}, NZ),
    ("lf_mock_hist2", "none", {"nl": 0, "hist": None}, NL),
    ("lf_mock_hist2", "none", {"nl": 0, "nz": BIG}, NL),
    ("lf_mock_hist2", "none", {"nz": 1, "nl": 2729, "edges": None}, "(nz + 2) * (nl + 2) = 8193 slots: the limit is %d" % mock.MAX_SLOTS2),
    ("lf_mock_hist2", "none", {"nz": BIG, "nl": 1, "z_edges": None}, NZ),
    ("lf_mock_hist2", "none", {"nz": 1, "nl": BIG, "hist": None}, NL),
    ("lf_mock_hist2", "none", {"z_edges": None, "edges": REV}, "z_edges, edges or hist is NULL"),
    ("lf_mock_hist2", "none", {"hist": None, "z_edges": REV}, "z_edges, edges or hist is NULL"),
    ("lf_mock_hist2", "none", {"z_edges": REV, "edges": REV}, "z_" + ORDER),
    ("lf_mock_hist2", "none", {"edges": REV, "count": NEG}, ORDER),
    ("lf_mock_hist2", "none", {"z_edges": REV, "count": NEG}, "z_" + ORDER),
    ("lf_mock_hist2_err", "none", {"nz": 0}, NO_MODEL),
    ("lf_mock_hist2_err", "none", {"hist": None}, NO_MODEL),
    ("lf_mock_hist2_err", "none", {"count": NEG}, NO_MODEL),
    ("lf_mock_hist2_err", "model", {"nz": 0, "hist": None}, NZ),
    ("lf_mock_hist2_err", "model", {"edges": REV, "count": NEG}, ORDER),
    ("lf_mock_hist2_cut", "none", {"nz": 0}, NO_MODEL),
    ("lf_mock_hist2_cut", "model", {"nz": 0}, NO_BAND),
    ("lf_mock_hist2_cut", "model", {"kept": None}, NO_BAND),
    ("lf_mock_hist2_cut", "model", {"edges": REV}, NO_BAND),
    ("lf_mock_hist2_cut", "armed", {"nz": 0, "kept": None}, NZ),
    ("lf_mock_hist2_cut", "armed", {"nl": 0, "kept": None}, NL),
    ("lf_mock_hist2_cut", "armed", {"kept": None, "z_edges": REV}, "z_edges, edges, hist or kept is NULL"),
    ("lf_mock_hist2_cut", "armed", {"z_edges": REV, "edges": REV}, "z_" + ORDER),
]


@pytest.mark.parametrize("entry,state,faults,message", CASES,
                         ids=["%02d-%s-%s-%s" % (i, c[0][8:], c[1], "+".join(sorted(c[2]))) for i, c in enumerate(CASES)])
def test_the_earlier_of_two_faults_is_the_one_named(gens, entry, state, faults, message):
    rc, msg, outs = _call(gens[state], entry, **dict(faults))
    assert rc == capi.LF_ERR_ARG
    assert msg == "%s: %s" % (entry, message)
    for a in outs:
        assert (a == FILL).all()


def test_a_single_fault_of_every_rank_is_refused_too(gens):
    """the later fault of each pair above, alone: it is a fault, so the pairs decide an order"""
    for entry, state, faults, message in [
            ("lf_mock_draw", "none", {"outputs": None}, "z, logL or field is NULL"),
            ("lf_mock_hist", "none", {"edges": REV}, ORDER),
            ("lf_mock_hist_err", "model", {"edges": REV}, ORDER),
            ("lf_mock_hist_cut", "armed", {"edges": REV}, ORDER),
            ("lf_mock_draw_cut", "armed", {"outputs": None}, "z, logL_true, logL_obs, sigma, field, keep or kept is NULL"),
            ("lf_mock_hist2", "none", {"count": NEG}, COUNT_RANGE),
            ("lf_mock_hist2_err", "model", {"count": NEG}, COUNT_RANGE),
            ("lf_mock_hist2_cut", "armed", {"edges": REV}, ORDER)]:
        rc, msg, outs = _call(gens[state], entry, **dict(faults))
        assert rc == capi.LF_ERR_ARG and msg == "%s: %s" % (entry, message)
        assert all((a == FILL).all() for a in outs)


def test_the_good_arguments_are_good():
    """_call's defaults pass every check (with a count of zero sources and cap 0 nothing is launched past the masses)"""
    inp = K.inputs(VARIANT, S)
    gen = K.arm(mock.MockGenerator(inp), inp, *K.table(7))
    try:
        zero = np.zeros((1, NF), dtype=np.int64)
        for entry in ("lf_mock_draw", "lf_mock_draw_err"):
            rc, msg, outs = _call(gen, entry, count=zero)
            assert rc == capi.LF_OK and msg == "" and all((a == FILL).all() for a in outs)
    finally:
        gen.close()
