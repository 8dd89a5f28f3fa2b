"""The device math of csrc/lf_math.h and the per-term forms, table lookups, cells and reductions of csrc/lf_kernels.h,
element by element on the GPU against 40-digit values (inputs, references, yardsticks and caps: tests/lf_problib.py; the
probe kernels: tests/term_probe.hip, compiled once per module with the library's own flags).

Every other GPU test of this arithmetic looks at lnprob, a sum of 1e3 .. 1e6 terms in which an error confined to one table
interval, one reduction boundary or one piece averages out.  Here each test prints its measured maximum of err / yardstick
and the input at the maximum, then asserts it against the cap: 4 x the figure of the same expression in NumPy binary64,
never below 2.  DESIGN.md section 3.13 records the figures."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import lf_problib as L
from test_tables_cpu import g_eval, horner
from lumfuncmcmc_amd import build

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_dp, _ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
OPS = {n: i for i, n in enumerate(("fexp_t", "fexp_neg", "fexp_c", "flog_half", "flog_half_upper", "frsqrt", "ln_fc_fast",
                                   "ln_fc_careful", "dexp", "dlog", "drsqrt"))}
LIBRARY_ULP = 2.0      # the device library documents 1 ulp for exp, log and rsqrt in binary64; + the metric's half unit of a second rounding


def _d(a):
    return a.ctypes.data_as(_dp)


def _i(a):
    return a.ctypes.data_as(_ip)


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("term_probe") / "term_probe.so")
    subprocess.run([build.hipcc()] + build.CXXFLAGS + ["-fPIC", "-shared", "-o", so, os.path.join(ROOT, "tests", "term_probe.hip")], check=True)
    lib = ctypes.CDLL(so)
    assert lib.tp_device_count() >= 1, "no GPU"
    return lib


def unary(lib, name, x):
    x = L.f64(x)
    assert len(x) <= L.NMAX
    y = np.full(len(x), -12345.0)
    rc = lib.tp_unary(OPS[name], _d(x), _d(y), len(x))
    assert rc == 0, (name, rc)
    return y


def check(name, case, got, x=None, cap=None):
    fig, i = L.measure(case, got)
    cap = L.CAPS[name] if cap is None else cap
    at = "" if x is None else " at input %r" % (x[i],)
    print("%-18s device max err / yard %9.3f (cap %g)%s: got %.17g ref %.17g" % (name, fig, cap, at, got[i], case["ref"][0][i]))
    assert fig <= cap, (name, fig, cap, i)
    return fig


# ---------------------------------------------------------------------------------------------- unary
def test_exp_family(probe):
    for name, case in (("fexp_t", L.case_fexp_t()), ("fexp_neg", L.case_fexp_neg()), ("fexp_c", L.case_fexp_c())):
        got = unary(probe, name, case["x"])
        fig = check(name, case, got, case["x"])
        if name != "fexp_neg":
            assert fig <= 2.0, "the header claims ~1 ulp"
        if name == "fexp_t":
            # At the ends of the reduction intervals, |r| = ln2/512, the only systematic part of the error is the dropped
            # r^5/120, at most 0.35 ulp and odd in r: over both ends the signed error averages to zero, the roundings
            # with it.  A mean beyond that 0.35 is a wrong coefficient, which the maximum over all inputs can hide.
            x = case["x"]
            with np.errstate(invalid="ignore"):
                fr = x / float(L.STEP) - np.floor(x / float(L.STEP))
                ends = (np.abs(fr - 0.5) < 1e-6) & (np.abs(x) < 700.0) & (np.abs(x) > 1e-3)
                signed = ((got - case["ref"][0]) - case["ref"][1]) / case["yard"]
            assert ends.sum() > 3000
            print("fexp_t             mean signed error at the %d interval ends: %+.3f ulp" % (ends.sum(), signed[ends].mean()))
            assert abs(signed[ends].mean()) <= 0.35
        if "zero" in case:           # beyond the underflow point the result is exactly +0
            z = got[case["zero"]]
            assert np.all(z == 0.0) and not np.any(np.signbit(z)), name
    c = L.case_dexp()
    check("dexp", c, unary(probe, "dexp", c["x"]), c["x"], cap=LIBRARY_ULP)


def test_log_family(probe):
    for name, case in (("flog_half", L.case_flog_half()), ("flog_half_upper", L.case_flog_half_upper())):
        check(name, case, unary(probe, name, case["x"]), case["x"])
    c = L.case_dlog()
    check("dlog", c, unary(probe, "dlog", c["x"]), c["x"], cap=LIBRARY_ULP)


def test_rsqrt(probe):
    c = L.case_frsqrt()
    fig = check("frsqrt", c, unary(probe, "frsqrt", c["x"]), c["x"])
    assert fig <= 2.0, "the header claims ~1 ulp"
    check("drsqrt", c, unary(probe, "drsqrt", c["x"]), c["x"], cap=LIBRARY_ULP)


def test_ln_fc(probe):
    c = L.case_ln_fc()
    check("ln_fc_fast", c, unary(probe, "ln_fc_fast", c["x"]), c["x"])
    check("ln_fc_careful", c, unary(probe, "ln_fc_careful", c["x"]), c["x"])


# ---------------------------------------------------------------------------------------------- terms
def term_free(lib, form, w, lum, logf, P, U):
    n = len(logf)
    y = np.full(n, -12345.0)
    rc = lib.tp_term_free(form, _d(L.f64(w)), _d(L.f64(lum)), _d(L.f64(logf)), _d(L.f64(P)), _d(L.f64(U)), _d(y), n)
    assert rc == 0, rc
    return y


def test_term_free_fast_and_noexp(probe):
    c = L.case_term_free()
    n = len(c["logf"])
    one = np.ones(n)
    got = term_free(probe, 0, c["w"], 42.0 * one, c["logf"], one, c["U"])
    check("term_free_fast", c, got, np.column_stack([c["num"], c["u"]]))
    # the careful form on the same inputs, for the record: its argument alphaC (logf - lF) is a different rounding of num, so
    # it is compared on its own inputs below
    ne = c["noexp"]
    sel = ne["sel"]
    got = term_free(probe, 1, c["w"][sel], 42.0 * one[sel], c["logf"][sel], one[sel], c["U"][sel])
    check("term_free_noexp", ne, got, c["num"][sel])


def test_term_free_careful(probe):
    c = L.case_term_careful()
    got = term_free(probe, 2, c["w"], c["lum"], c["logf"], c["P"], c["U"])
    want = c["want_inf"]
    # each of the five conditions, on both sides of LF_UNDERFLOW
    assert np.all(got[want] == -np.inf), np.where(want & (got != -np.inf))[0]
    assert np.all(np.isfinite(got[~want])), np.where(~want & ~np.isfinite(got))[0]
    num = c["w"][:, 4] * (c["logf"] - c["w"][:, 5])
    check("term_free_careful", c, got, np.column_stack([num, c["U"] * c["w"][:, 6], c["w"][:, 7]]))


def test_lnT_zevol(probe):
    c = L.case_zevol()
    n = len(c["lum"])
    for fast in (1, 0):
        y = np.full(2 * n, -12345.0)
        rc = probe.tp_zevol(fast, _d(c["w"]), _d(c["lum"]), _d(c["z"]), _d(c["z2"]), _d(y), n)
        assert rc == 0, rc
        lnT, v = y[0::2], y[1::2]
        if fast:
            check("v_zevol", c["v"], v, c["lum"])
            check("lnT_zevol", c["lnT"], lnT, c["lum"])
        else:            # the device library's exp has no clamp: beyond the clamps it gives inf and 0
            keep = ~c["clamped"]
            sub = lambda k: {"ref": (c[k]["ref"][0][keep], c[k]["ref"][1][keep]), "yard": c[k]["yard"][keep]}      # noqa: E731
            check("v_zevol", sub("v"), v[keep], c["lum"][keep])
            check("lnT_zevol", sub("lnT"), lnT[keep], c["lum"][keep])
            assert v[0] == np.inf and v[1] == 0.0


# ---------------------------------------------------------------------------------------------- tables and cells
def run_table(lib, st, noexp, wk, x, npad):
    n = len(npad)
    s, coef = np.full(n, -12345.0), np.zeros((n, 20))
    rc = lib.tp_table(st, int(noexp), _d(L.f64(wk)), _d(L.f64(x)), _i(np.ascontiguousarray(npad, dtype=np.int32)), _d(s), _d(coef), n)
    assert rc == 0, rc
    return s, coef


_GROW = {r.tobytes(): i for i, r in enumerate(L.GT)}
_HROW = {r.tobytes(): i for i, r in enumerate(L.HT)}


@pytest.mark.parametrize("noexp", [False, True])
@pytest.mark.parametrize("st", [2, 4, 8])
def test_table_lookup_and_terms(probe, st, noexp):
    c = L.case_table(st, noexp)
    n = len(c["npad"])
    got, coef = run_table(probe, st, noexp, c["wk"], c["x"], c["npad"])
    # the device's piece choice: the coefficient rows it loaded, looked up in the tables
    pg = np.array([_GROW.get(np.ascontiguousarray(coef[i, :8]).tobytes(), -1) for i in range(n)])
    assert np.all(pg >= 0), "coefficients that are no row of G_TABLE"
    # ... equals the NumPy lookup of tests/test_tables_cpu.py: that piece's polynomial at the centre reproduces g_eval bit
    # for bit, in the half of the table that the sign of the centre selects (g_eval does not return its index; two
    # neighbouring pieces differ in the last bits wherever both are valid, so only at a shared end can they agree by chance)
    q = np.where(pg >= L.G_NPOS, pg - L.G_NPOS, pg)
    vlo = np.ldexp(1.0 + (q & ((1 << L.G_BITS) - 1)) / (1 << L.G_BITS), q >> L.G_BITS)
    numc = c["numc"]
    t = np.where(pg >= L.G_NPOS, -numc, numc) + (1.0 - vlo)
    mz = (numc == 0.0) & np.signbit(numc)
    # -0.0: the sign bit selects the negative half (its first piece, valid at 0 by its margin); NumPy's `<` the positive
    assert np.all(pg[mz] == L.G_NPOS)
    same = (horner(L.GT[pg], t) == g_eval(numc, numc)) & ((pg >= L.G_NPOS) == (numc < 0))
    bad = np.where(~same & ~mz)[0]
    assert len(bad) == 0, (bad[:10], pg[bad[:10]], numc[bad[:10]], t[bad[:10]])
    if not noexp:
        ph = np.array([_HROW.get(np.ascontiguousarray(coef[i, 8:16]).tobytes(), -1) for i in range(n)])
        assert np.all(ph >= 0), "coefficients that are no row of H_TABLE"
        hx = c["hx"]
        fl = np.clip(np.floor(hx), 0, L.H_N - 1).astype(int)
        tie = (hx == np.floor(hx)) & (hx >= 1) & (hx <= L.H_N - 1)
        ok = (ph == fl) | (tie & (ph == fl - 1))
        # (hx is rounded for the seeded lanes: within an ulp of an integer either neighbour is the floor of the exact value)
        near = (c["kind"] == 5) & (np.abs(hx - np.rint(hx)) <= 4 * np.spacing(np.abs(hx)))
        ok |= near & (np.abs(ph - fl) <= 1)
        assert np.all(ok), (np.where(~ok)[0][:10], ph[~ok][:10], hx[~ok][:10])
        assert tie.sum() >= 100 and set(ph[c["kind"] == 3]) >= set(range(1, L.H_N - 1))
    # the value, whichever piece was chosen
    check("table_terms", c, got, np.column_stack([c["numc"], c["x"][:, st // 2] + c["wk"][:, 3] + L.H_LO, c["npad"]]))


def _rn(v):
    """one rounding of a 40-digit value"""
    return float(v)


@pytest.mark.parametrize("noexp", [False, True])
@pytest.mark.parametrize("st", [2, 4, 8])
def test_table_terms_padding(probe, st, noexp):
    """npad copies of the last source change the lane's sum by one rounding of the sum and no more: on the padded lanes of
    case_table, S_p (npad = p) is the correctly rounded S_0 - p last, S_0 the same slots with npad = 0 and `last` the term of
    slot ST - 1 (the probe's second output).  Lanes whose ST slots all hold one source: every accumulator adds equal rounded
    products, or is fma(p, q, L) with L = rnd(p q), which is rnd(2 L + e) = 2 L because |e| <= ulp(L) / 2; so S_0 = ST L
    exactly, S_p is (ST - p) L rounded once, and a lane wholly past the end of its chunk (npad = ST) gives exactly 0."""
    mpf = L.mpf
    c = L.case_table(st, noexp)
    pad = np.where(c["npad"] > 0)[0]
    assert len(pad) > 500
    x, wk, p = c["x"][pad], c["wk"][pad], c["npad"][pad]
    s0, co = run_table(probe, st, noexp, wk, x, np.zeros(len(pad), dtype=np.int32))
    sp, cp = run_table(probe, st, noexp, wk, x, p)
    last = co[:, 19]
    assert np.array_equal(last, cp[:, 19]) and np.all(last < 0.0)
    want = np.array([_rn(mpf(a) - int(k) * mpf(b)) for a, k, b in zip(s0, p, last)])
    assert np.array_equal(sp, want), np.where(sp != want)[0][:10]
    # one source in every slot
    idx = np.arange(0, len(c["npad"]), 5)
    x1 = np.repeat(c["x"][idx, st // 2][:, None], st, 1)
    s0, co = run_table(probe, st, noexp, c["wk"][idx], x1, np.zeros(len(idx), dtype=np.int32))
    last = co[:, 19]
    assert np.array_equal(s0, st * last)
    for k in range(1, st + 1):
        sp, _ = run_table(probe, st, noexp, c["wk"][idx], x1, np.full(len(idx), k, dtype=np.int32))
        assert np.array_equal(sp, np.array([_rn((st - k) * mpf(b)) for b in last])), k
    assert np.all(sp == 0.0)                 # k = ST: "8 t - 8 t"


def test_cell_sum(probe):
    c = L.case_cells()
    n = len(c["nsrc"])
    y = np.full(n, -12345.0)
    rc = probe.tp_cell(_d(c["wk"]), _d(c["cd"]), _d(y), n)
    assert rc == 0, rc
    check("cell_sum", c, y, np.column_stack([c["wk"][:, 0], c["cd"][:, 0], c["nsrc"]]))


# ---------------------------------------------------------------------------------------------- reductions
def _fsum_rows(a):
    return np.array([math.fsum(r) for r in a])


def test_wave_sums(probe):
    exact, seeded = L.reduction_vectors()
    x = np.ascontiguousarray(np.concatenate([exact, seeded]))
    nv = len(x)
    a, b = np.full(nv, -12345.0), np.full(nv, -12345.0)
    rc = probe.tp_wave(_d(x), _d(a), _d(b), nv)
    assert rc == 0, rc
    ne = len(exact)
    want = _fsum_rows(x)
    for name, got in (("wave_sum_dpp", a), ("wave_sum", b)):
        assert np.array_equal(got[:ne], want[:ne]), (name, np.where(got[:ne] != want[:ne])[0][:10])      # one-hot: each lane once
        bound = 63 * L.U53 * np.sum(np.abs(x[ne:]), axis=1)
        r = np.abs(got[ne:] - want[ne:]) / bound
        print("%-14s max err / ((n - 1) 2^-53 sum|x|) = %.4f" % (name, r.max()))
        assert np.all(r <= 1.0), (name, r.max())


def test_group8(probe):
    exact, seeded = L.reduction_vectors()
    x = np.ascontiguousarray(np.concatenate([exact, seeded]))
    nv = len(x)
    rng = np.random.default_rng(5)
    xi = rng.integers(0, 2 ** 31 - 1, (nv, 64)).astype(np.int32)
    xi[:64] = np.eye(64, dtype=np.int32) << (np.arange(64) % 31)[None, :]
    ys, yo = np.full((nv, 64), -12345.0), np.zeros((nv, 64), dtype=np.int32)
    rc = probe.tp_group8(_d(x), _i(xi), _d(ys), _i(yo), nv)
    assert rc == 0, rc
    want_or = np.repeat(np.bitwise_or.reduce(xi.reshape(nv, 8, 8), axis=2), 8, axis=1)
    assert np.array_equal(yo, want_or)
    g = x.reshape(nv, 8, 8)
    want = np.repeat(np.array([[math.fsum(q) for q in r] for r in g]), 8, axis=1)
    ne = len(exact)
    assert np.array_equal(ys[:ne], want[:ne])                 # every lane of a group holds the group's total
    bound = np.repeat(7 * L.U53 * np.sum(np.abs(g), axis=2), 8, axis=1)[ne:]
    r = np.abs(ys[ne:] - want[ne:]) / bound
    print("group8_sum     max err / (7 2^-53 sum|x|) = %.4f" % r.max())
    assert np.all(r <= 1.0)
    # all eight lanes of a group hold the same bits
    assert np.array_equal(ys.reshape(nv, 8, 8), np.repeat(ys.reshape(nv, 8, 8)[:, :, :1], 8, axis=2))


@pytest.mark.parametrize("indexed", [False, True])
def test_reduce_store(probe, indexed):
    exact, seeded = L.reduction_vectors(256)
    rows = np.concatenate([exact, seeded])
    rng = np.random.default_rng(6)
    worst = 0.0
    for nw in range(1, 17):
        ncase = 6
        pick = rng.integers(0, len(rows), (ncase, nw))
        pick[0] = np.arange(nw) * 16 + 15                      # one-hot rows: column 16 w + 15 of walker w
        pick[1] = np.arange(nw)
        pick[2] = len(exact) - 1                               # the lane-weighted row
        red = np.ascontiguousarray(rows[pick])                 # [ncase][nw][256]
        is_exact = pick < len(exact)
        stride, chunk, w0, nout = 3, 1, 2, 3 * 40
        widx = np.ascontiguousarray(rng.permutation(38)[:nw], dtype=np.int32) if indexed else None
        out = np.full((ncase, nout), -777.0)
        rc = probe.tp_reduce(_d(red), nw, _d(out), nout, stride, w0, chunk, _i(widx) if indexed else None, ncase)
        assert rc == 0, (nw, rc)
        slot = (widx if indexed else w0 + np.arange(nw)) * stride + chunk
        want = np.array([[math.fsum(r) for r in cs] for cs in red])
        got = out[:, slot]
        assert np.array_equal(got[is_exact], want[is_exact]), (nw, np.where(is_exact & (got != want)))
        bound = 255 * L.U53 * np.sum(np.abs(red), axis=2)
        r = np.abs(got - want)[~is_exact] / bound[~is_exact]
        worst = max(worst, r.max() if r.size else 0.0)
        assert np.all(r <= 1.0), (nw, r.max())
        rest = np.ones(nout, dtype=bool)
        rest[slot] = False
        assert np.all(out[:, rest] == -777.0), "reduce_store wrote outside its slots (nw = %d)" % nw
    print("reduce_store   max err / (255 2^-53 sum|x|) = %.4f" % worst)
    # an index past the end is refused by the entry point, not run
    bad = np.array([1000], dtype=np.int32)
    out = np.zeros((1, 120))
    assert probe.tp_reduce(_d(np.zeros((1, 1, 256))), 1, _d(out), 120, 3, 0, 1, _i(bad), 1) == -1


# ---------------------------------------------------------------------------------------------- special values
def test_special_values(probe):
    nan, inf = np.nan, np.inf
    # NaN: fexp_t and fexp_neg pass it on; fexp_c's clamp, fmin(fmax(x, -750), 709), returns its other operand for a NaN,
    # so fexp_c(NaN) = fexp_t(-750) = +0 (lf_math.h says so)
    assert np.isnan(unary(probe, "fexp_t", [nan])[0]) and np.isnan(unary(probe, "fexp_neg", [nan])[0])
    y = unary(probe, "fexp_c", [nan, -inf, inf, -750.0, 709.0, np.nextafter(709.0, inf)])
    assert y[0] == 0.0 and not np.signbit(y[0]) and y[1] == 0.0 and y[2] == y[4] == y[5] and np.isfinite(y[2]) and y[3] == 0.0
    # exact +0 beyond the underflow point, the last subnormal before it, 1 at +-0
    y = unary(probe, "fexp_t", [-745.14, -1.0e5, -(2.0 ** 22), -745.13, 0.0, -0.0, 2.0 ** 22])
    assert np.all(y[:3] == 0.0) and not np.any(np.signbit(y[:3])) and y[3] == 5e-324 and y[4] == 1.0 and y[5] == 1.0 and y[6] == inf
    y = unary(probe, "fexp_neg", [0.0, 37.5, 745.14, 999999.9])
    assert y[0] == 1.0 and 1.0 - y[1] == 1.0 and y[2] == 0.0 and y[3] == 0.0
    # flog_half: w = 0 is finite, about -710; w = 2 gives 0 to a rounding; subnormal w finite
    y = unary(probe, "flog_half", [0.0, 2.0, 1.0, 5e-324, 2.0 ** -1023])
    assert -711.0 < y[0] < -709.0 and abs(y[1]) <= 3.1e-16 and abs(y[2] + L.LN2) <= 3.1e-16 and np.all(np.isfinite(y[3:]))
    # flog_half_upper(2) is nudged one ulp down: the value of 2 - 1 ulp, -1.1e-16, not 0 and not the next interval's entry
    y = unary(probe, "flog_half_upper", [2.0, np.nextafter(2.0, 0.0), 1.0])
    assert y[0] == y[1] and -3.4e-16 < y[0] < 0.0 and abs(y[2] + L.LN2) <= 3.1e-16
    # ln fc: 0 at both zeros gives -ln 2; frsqrt of powers of four is exact
    y = unary(probe, "ln_fc_fast", [0.0, -0.0])
    assert np.all(np.abs(y + L.LN2) <= 3.1e-16)
    k = np.arange(-300, 500, 7)
    assert np.array_equal(unary(probe, "frsqrt", np.ldexp(1.0, 2 * k)), np.ldexp(1.0, -k))
