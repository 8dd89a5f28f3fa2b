"""Inputs, 40-digit references and yardsticks for the element-wise probes of the device math (csrc/lf_math.h) and of the
per-term forms, table lookups, cells and reductions of csrc/lf_kernels.h.  No GPU here: tests/test_terms_cpu.py checks that
every generator yields what it promises and measures the NumPy binary64 figures, tests/test_gpu_terms.py runs the same
cases through tests/term_probe.hip.

A case is a dict: the input arrays (what the probe's entry point takes), `ref` = the value at 40 digits from the exact
binary64 inputs as a (hi, lo) pair of doubles, `yard` = the unit the error is expressed in, `np` = the same expression in
plain NumPy binary64 (the reference's arithmetic, correctly rounded), `exempt` = inputs the function is documented not to
accept (asserted finite, never more than 1 % of a list).  Every yardstick follows from the number format and the formula:
none comes from the code under test.  The cap on the device's max err / yard is 4 x the NumPy figure and never below 2
(a hand-written primitive gets about 2 ulp where NumPy's has 1/2; fma only removes roundings)."""
import functools
import math
import os
import re

import mpmath as mp
import numpy as np

from test_tables_cpu import C as TC, G as GT, H as HT, g_eval, g_ref, h_eval, h_ref

mp.mp.dps = 40
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lumfuncmcmc_amd", "csrc")
U53 = 2.0 ** -53
LN2 = math.log(2.0)
LN10 = 2.302585092994045684
LNLN10 = 0.834032445247955959
LF_UNDERFLOW = 745.13321910194122
NMAX = 20000                      # no entry point gets more elements than this
G_MARGIN, H_MARGIN, H_LO, H_INV = TC["G_MARGIN"], TC["H_MARGIN"], TC["H_LO"], TC["H_INV"]
G_LO, G_HI = TC["G_NUM_LO"], TC["G_NUM_HI"]
G_ERR, H_ERR = TC["G_TABLE_MAX_REL_ERR"], TC["H_TABLE_MAX_REL_ERR"]
G_NPOS, G_BITS, H_N = int(TC["G_NPOS"]), int(TC["G_BITS"]), int(TC["H_N"])
_src = open(os.path.join(CSRC, "lf_kernels.h")).read()
CELL_RHO_G, CELL_RHO_H = (float(x) for x in re.search(r"CELL_RHO_G = ([0-9.e-]+), CELL_RHO_H = ([0-9.e-]+);", _src).groups())
CELL_REC = 10
LNOM0 = math.log(121.9 * 0.85 * 3600)       # ln Omega_0 of a field of the synthetic survey (synth.OMEGA_0)

# Caps K on max err / yard, per probed function: max(2, 4 x the NumPy binary64 figure on the same inputs), the figures
# measured by tests/test_terms_cpu.py::test_numpy_figures_behind_the_caps (which asserts that they still hold) on
# 2026-10-17; DESIGN.md section 3.13 has the device's figures next to them.
CAPS = {
    # (dexp, dlog, drsqrt: for the record only - the device library's versions are asserted against its documented 1 ulp)
    "fexp_t": 2.56, "fexp_neg": 2.67, "fexp_c": 2.62, "dexp": 2.56,
    "flog_half": 3.93, "flog_half_upper": 2.89, "dlog": 3.93,
    "frsqrt": 5.5, "drsqrt": 5.5,
    "ln_fc_fast": 10.9, "ln_fc_careful": 10.9,
    "term_free_fast": 10.1, "term_free_noexp": 10.1, "term_free_careful": 7.83,
    "lnT_zevol": 2.84, "v_zevol": 2.23,
    "table_terms": 2.0, "cell_sum": 2.0,
}
NUMPY_FIGURES = {}                # filled by numpy_figure(): name -> (max err / yard, index)


def cap_from(numpy_figure):
    return max(2.0, 4.0 * numpy_figure)


# ---------------------------------------------------------------------------------------------- helpers
def f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def mpf(x):
    return mp.mpf(float(x))


def pair(vals):
    """40-digit values -> (hi, lo) doubles; values beyond the format's range become +-inf / 0 with lo = 0"""
    hi = np.array([float(v) for v in vals])
    lo = np.array([float(v - mp.mpf(h)) if math.isfinite(h) else 0.0 for v, h in zip(vals, hi)])
    return hi, lo


def err_of(got, ref):
    """|got - ref| with ref a (hi, lo) pair; NaN where one is NaN and the other is not, 0 where both are the same inf / NaN"""
    hi, lo = ref
    got = f64(got)
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.abs((got - hi) - lo)
    same = (got == hi) | (np.isnan(got) & np.isnan(hi))
    return np.where(same & ~np.isfinite(hi), 0.0, e)


def ulp_of(ref):
    """unit in the last place of the reference; 2^-1074 for subnormal (and zero) results"""
    with np.errstate(invalid="ignore"):
        return np.where(np.isfinite(ref[0]), np.spacing(np.abs(np.where(np.isfinite(ref[0]), ref[0], 1.0))), 1.0)


def ulps_around(x, ks=(-2, -1, 0, 1, 2)):
    """x and its neighbours k units in the last place away"""
    out = []
    for k in ks:
        v = np.array(x, dtype=np.float64, copy=True)
        for _ in range(abs(k)):
            v = np.nextafter(v, np.inf if k > 0 else -np.inf)
        out.append(v)
    return np.concatenate([np.atleast_1d(o) for o in out])


def measure(case, got):
    """(max err / yard, index of the maximum) over the case's comparable inputs; exempt inputs must be finite, and no
    input is left out otherwise: a NaN where none is expected counts as an infinite error"""
    got = f64(got)
    ex = case.get("exempt", np.zeros(got.shape, dtype=bool))
    assert np.all(np.isfinite(got[ex])), "non-finite result on an exempt input"
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = err_of(got, case["ref"]) / case["yard"]
    ratio = np.where(np.isnan(ratio), np.inf, ratio)
    ratio[ex] = 0.0
    i = int(np.argmax(ratio))
    return float(ratio[i]), i


def numpy_figure(name, case):
    fig = measure(case, case["np"])
    NUMPY_FIGURES[name] = fig
    return fig


def _finish(case):
    n = len(case["yard"])
    assert n <= NMAX, n
    ex = case.get("exempt")
    if ex is not None:
        assert ex.sum() < 0.01 * n, (ex.sum(), n)
    return case


def fma_exact(a, b, c):
    """round(a b + c), one rounding (what the device's fma gives), through 40-digit arithmetic"""
    r = np.array([float(mpf(x) * mpf(y) + mpf(z)) for x, y, z in zip(a, b, c)])
    # (40-digit numbers have no signed zero: an exact zero takes the sign IEEE gives it, -0 only from (-0) + (-0))
    return np.where(r == 0.0, f64(a) * f64(b) + f64(c), r)


# ---------------------------------------------------------------------------------------------- exp
STEP = mp.log(2) / 256


def reduction_boundaries(jmax_dense=300, xlo=-745.0, xhi=709.7):
    """The arguments where fexp_t's reduction changes its table entry, (j + 1/2) ln2/256, and where its remainder is 0,
    j ln2/256: the nearest double and its neighbours +-1, +-2 ulp; every j up to jmax_dense and a geometric ladder beyond"""
    js = set(range(-jmax_dense, jmax_dense + 1))
    j = jmax_dense
    while j * float(STEP) < max(-xlo, xhi):
        js.update((j, -j, j + 1, -j - 1))
        j = int(j * 1.37) + 1
    js.update((int(xhi / float(STEP)) - 1, int(xlo / float(STEP)) + 1))          # and the last ones inside the range
    pts = []
    for j in sorted(js):
        for h in (0, mp.mpf(1) / 2):
            x = float((j + h) * STEP)
            if xlo <= x <= xhi and not (j == 0 and h == 0):
                pts.append(x)
    return np.array(pts)


def _exp_ref(x, lo=None, hi=None):
    out = []
    for v in x:
        if math.isnan(v):
            out.append(mp.nan)
            continue
        if lo is not None:
            v = min(max(v, lo), hi)
        out.append(mp.exp(mpf(v)) if math.isfinite(v) else (mp.inf if v > 0 else mp.mpf(0)))
    return out


def _exp_pair(x, **kw):
    """the correctly rounded result is what the format can hold: 0 below 2^-1075, inf above the largest double"""
    vals = _exp_ref(x, **kw)
    big = mp.mpf(2) ** 1024 - mp.mpf(2) ** 970
    vals = [mp.inf if (not mp.isnan(v) and v >= big) else v for v in vals]
    hi = np.array([float(v) for v in vals])
    lo = np.array([float(v - mp.mpf(h)) if (math.isfinite(h) and mp.isfinite(v)) else 0.0 for v, h in zip(vals, hi)])
    return hi, lo


@functools.lru_cache(None)
def case_fexp_t():
    rng = np.random.default_rng(101)
    b = reduction_boundaries()
    edges = np.concatenate([
        [0.0, -0.0], [s * v for s in (1, -1) for v in (5e-324, 2.0 ** -1022, 1e-300, 1e-20, 2.0 ** -54, 2.0 ** -30, 1e-3)],
        ulps_around(b),
        np.linspace(-LF_UNDERFLOW, -708.4, 600), rng.uniform(-LF_UNDERFLOW, -708.4, 600),      # subnormal results
        ulps_around(-LF_UNDERFLOW), [-745.14, -745.2, -746.0, -750.0, -1000.0, -1.0e5, -(2.0 ** 22)],
        ulps_around(709.782712893384), [709.78, 709.7, 709.0, 709.79, 710.0, 720.0, 2.0 ** 22], [np.nan]])
    fill = np.concatenate([rng.uniform(-745.0, 709.7, 4000), rng.normal(0, 1, 2000), rng.uniform(-40, 40, 2000)])
    x = f64(np.concatenate([edges, fill]))
    ref = _exp_pair(x)
    with np.errstate(over="ignore", under="ignore"):
        npv = np.exp(x)
    return _finish({"x": x, "ref": ref, "yard": ulp_of(ref), "np": npv, "n_edges": len(edges), "boundaries": b,
                    "zero": x <= -745.14})


@functools.lru_cache(None)
def case_fexp_neg():
    """u in [0, 1e6): the screen of prepare_lane (u_max V < 1.0e6)"""
    rng = np.random.default_rng(102)
    b = reduction_boundaries(xlo=0.0, xhi=745.0)
    edges = np.concatenate([[0.0, 5e-324, 1e-300, 2.0 ** -60, 1e-17, 1e-9], ulps_around(b), ulps_around(37.5),
                            np.linspace(37.0, 38.0, 101), ulps_around(LF_UNDERFLOW), np.linspace(744.0, 746.0, 201),
                            [1.0e3, 1.0e4, 1.0e5, 999999.9, np.nextafter(1.0e6, 0.0)]])
    fill = 10.0 ** rng.uniform(-6.0, 2.9, 5000)
    u = f64(np.concatenate([edges, fill]))
    ref = _exp_pair(-u)
    # the header's own term: the one-constant reduction adds u * 1.1e-16 relative
    yard = ulp_of(ref) + u * 1.1e-16 * np.abs(ref[0])
    with np.errstate(under="ignore"):
        npv = np.exp(-u)
    return _finish({"x": u, "ref": ref, "yard": yard, "np": npv, "zero": u >= 745.14})


@functools.lru_cache(None)
def case_fexp_c():
    rng = np.random.default_rng(103)
    t = case_fexp_t()
    x = f64(np.concatenate([ulps_around(-750.0, (-1, 0, 1)), ulps_around(709.0, (-1, 0, 1)), [np.inf, -np.inf, 1e300, -1e300, 710.0, -751.0],
                            t["x"][:t["n_edges"]][~np.isnan(t["x"][:t["n_edges"]])][::3], rng.uniform(-760.0, 715.0, 3000), [np.nan]]))
    ref = _exp_pair(x, lo=-750.0, hi=709.0)
    with np.errstate(under="ignore", invalid="ignore"):
        npv = np.exp(np.clip(x, -750.0, 709.0))
    # NaN: fmax / fmin return their other operand, so the clamp turns NaN into -750 and the result is +0 (pinned by
    # test_special_values); it is exempt from the comparison with exp
    ex = np.isnan(x)
    ref = (np.where(ex, 0.0, ref[0]), np.where(ex, 0.0, ref[1]))
    npv = np.where(ex, 0.0, npv)
    return _finish({"x": x, "ref": ref, "yard": ulp_of(ref), "np": npv, "exempt": ex})


def case_dexp():
    c = dict(case_fexp_t())
    return c


# ---------------------------------------------------------------------------------------------- log
def mantissa_interval_ends(binades):
    """both ends of the 256 table intervals of the mantissa and the doubles next to them inside, in each binade"""
    j = np.arange(256)
    m = np.concatenate([1.0 + j / 256.0, np.nextafter(1.0 + j / 256.0, 2.0), np.nextafter(1.0 + (j + 1) / 256.0, 0.0),
                        np.nextafter(np.nextafter(1.0 + (j + 1) / 256.0, 0.0), 0.0)])
    return np.concatenate([np.ldexp(m, e) for e in binades])


def _log_half_pair(w):
    return pair([mp.log(mpf(v) / 2) if v > 0 else mp.mpf(-710) for v in w])


@functools.lru_cache(None)
def case_flog_half():
    """w in (0, 2].  Subnormal w (and 0) are outside the contract: flog_half's callers pass w = 1 + num / sqrt(1 + num^2)
    (>= 1 / (2 num^2) in exact arithmetic, or exactly 0 after the cancellation for num < -1e8), and the FAST screen of
    prepare_lane, -2 ln(2 (1 + |num|)) (1 + 1 / x) + ln Omega_0 > -700, keeps |num| < e^350: w is 0 or above 1e-304."""
    rng = np.random.default_rng(104)
    tiny = 2.0 ** -1022
    edges = np.concatenate([mantissa_interval_ends((-1022, -1000, -512, -100, -10, -3, -2, -1, 0)),
                            [2.0, 1.0, np.nextafter(1.0, 0.0), np.nextafter(1.0, 2.0), np.nextafter(2.0, 0.0), tiny, np.nextafter(tiny, 1.0)],
                            [0.0, 5e-324, 1e-310, 2.0 ** -1023, np.nextafter(tiny, 0.0)]])
    fill = np.ldexp(rng.uniform(1.0, 2.0, 4000), rng.integers(-1022, 1, 4000))
    w = f64(np.concatenate([edges, fill]))
    ex = w < tiny
    ref = _log_half_pair(w)
    with np.errstate(divide="ignore"):
        npv = np.where(ex, -710.0, np.log(0.5 * w))
    return _finish({"x": w, "ref": ref, "yard": U53 * np.maximum(np.abs(ref[0]), LN2), "np": npv, "exempt": ex})


@functools.lru_cache(None)
def case_flog_half_upper():
    rng = np.random.default_rng(105)
    w = f64(np.concatenate([mantissa_interval_ends((0,)), [2.0, np.nextafter(2.0, 0.0), 1.0], rng.uniform(1.0, 2.0, 3000)]))
    ref = _log_half_pair(w)
    return _finish({"x": w, "ref": ref, "yard": U53 * np.maximum(np.abs(ref[0]), LN2), "np": np.log(0.5 * w)})


def case_dlog():
    """the device library's log on flog_half's inputs (it takes subnormals; 0 is replaced by the smallest one)"""
    c = dict(case_flog_half())
    x = np.where(c["x"] <= 0.0, 5e-324, c["x"])
    ref = pair([mp.log(mpf(v)) for v in x])
    c.update(x=x, ref=ref, yard=U53 * np.maximum(np.abs(ref[0]), LN2), np=np.log(x), exempt=np.zeros(len(x), dtype=bool))
    return c


# ---------------------------------------------------------------------------------------------- rsqrt
# What frsqrt's callers can pass.  ln_fc_fast, term_free_noexp, field_sum_bright: s = 1 + num^2 in [1, inf).
# term_free_fast: s d^2 with d = 1 - e^(-u); the FAST screen of prepare_lane keeps ln fc_lo (1 + 1 / u) + ln Omega_0 above
# -700 with ln fc_lo <= -0.693, so u > 0.693 / (700 + ln Omega_0) > 9e-4 for any solid angle (ln Omega_0 < 27 even in
# square arcseconds over the whole sky), d > 9e-4 and s d^2 > 8e-7; for negative num, 2 ln(2 (1 + |num|)) < 700 + ln
# Omega_0 bounds s < e^730 < 1e305.  field_sum (grid nodes, not screened) floors d at 1e-100: s d^2 >= 1e-200.
# So: [1e-200, 1e305], all of it normal.
FRSQRT_LO, FRSQRT_HI = 1.0e-200, 1.0e305


@functools.lru_cache(None)
def case_frsqrt():
    rng = np.random.default_rng(106)
    k = np.arange(-332, 506)
    p4 = np.ldexp(1.0, 2 * k)
    s = f64(np.concatenate([ulps_around(p4, (-1, 0, 1)), [FRSQRT_LO, FRSQRT_HI, 1.0, 2.0, 3.0], 10.0 ** rng.uniform(-200, 305, 8000),
                            rng.uniform(1.0, 4.0, 4000), 1.0 + rng.uniform(-30, 30, 2000) ** 2]))
    s = s[(s >= FRSQRT_LO) & (s <= FRSQRT_HI)]
    ref = pair([1 / mp.sqrt(mpf(v)) for v in s])
    return _finish({"x": s, "ref": ref, "yard": ulp_of(ref), "np": 1.0 / np.sqrt(s)})


# ---------------------------------------------------------------------------------------------- ln fc and the free term
def _w_of(num):
    """1 + num / sqrt(1 + num^2) at 40 digits, without the cancellation for negative num"""
    x = mpf(num)
    s = mp.sqrt(1 + x * x)
    return 1 + x / s if x >= 0 else 1 / (s * (s - x))


def yard_E(ref_hi, w, d):
    """E = 2^-53 (|ref| (1 + 1/d) + 1 / (w d)): one rounding of the result and of 1/d, and the two cancellations the
    formula carries, 1 + num / sqrt(1 + num^2) (a rounding of w is 2^-53 absolute, 2^-53 / w in ln w) and 1 - e^(-u)"""
    return U53 * (np.abs(ref_hi) * (1.0 + 1.0 / d) + 1.0 / (w * d))


def np_ln_fc(num):
    return np.log(0.5 * (1.0 + num / np.sqrt(1.0 + num * num)))


def g_boundaries():
    """num where |num| + 1 crosses from one piece of g to the next, inside the range the key tests admit"""
    out = []
    for q in range(1, G_NPOS + 1):
        v = 2.0 ** (q >> G_BITS) * (1.0 + (q & ((1 << G_BITS) - 1)) / (1 << G_BITS))
        for s in (1.0, -1.0):
            n = s * (v - 1.0)
            if G_LO + 2 * G_MARGIN < n < G_HI - 2 * G_MARGIN:
                out.append(n)
    return np.array(sorted(out))


@functools.lru_cache(None)
def case_ln_fc():
    rng = np.random.default_rng(107)
    num = f64(np.concatenate([[0.0, -0.0, 5e-324, -5e-324, 1e-300, -1e-300, 1e-17, -1e-17, 1.0, -1.0, 30.0, -30.0, -1.6e4, 1.0e6],
                              ulps_around(g_boundaries(), (-1, 0, 1)), rng.uniform(-30, 30, 4000),
                              -10.0 ** rng.uniform(0, 4.2, 3000), 10.0 ** rng.uniform(0, 6, 2000)]))
    ws = [_w_of(v) for v in num]
    ref = pair([mp.log(w / 2) for w in ws])
    w = np.array([float(v) for v in ws])
    return _finish({"x": num, "ref": ref, "yard": yard_E(ref[0], w, 1.0), "np": np_ln_fc(num)})


def fast_screen(num, u, lnom0=LNOM0):
    """The FAST screens of prepare_lane (lf_kernels.h) on the completeness part, restated in NumPy with the field's extremes
    replaced by the one source: single-precision lower bound of ln fc, times 1 + 1 / x, plus ln Omega_0, above SAFE = -700,
    and f / f_tau below 1e6.  (The Schechter part's screen, lbT, does not enter term_free_fast.)"""
    f32 = np.float32
    an = np.maximum(-num, 0.0).astype(f32)
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        lo = np.where(num >= 0.0, f32(-0.6932), f32(-2.00002) * f32(0.69314724) * np.log2(f32(2.0) * (f32(1.0) + an) * f32(1.000001)) - f32(0.01)).astype(f32)
        x = u.astype(f32) * f32(0.999999)
        lnom = lnom0 + (lo * (f32(1.0) + f32(1.000001) / x)).astype(np.float64)
    return (lnom > -700.0) & (u < 1.0e6)


def u_min_for(num, lnom0=LNOM0):
    """the smallest f / f_tau the screen lets through for this num (double arithmetic, then 2 % on top)"""
    lo = np.where(num >= 0.0, -0.6932, -2.00002 * 0.69314724 * np.log2(2.0 * (1.0 + np.maximum(-num, 0.0)) * 1.000001) - 0.01)
    return 1.02 * 1.000001 / ((-700.0 - lnom0) / lo - 1.0) / 0.999999


@functools.lru_cache(None)
def case_term_free():
    """term_free_fast over what MODE_FAST admits.  Elements: WFree (9 doubles), logf, U; num = fma(alphaC, logf, cA) and
    u = U V are what the function forms from them, and the reference takes exactly those products of the binary64 inputs."""
    rng = np.random.default_rng(108)
    n = 6000
    aC = np.concatenate([rng.uniform(1.0, 7.0, n // 2), 10.0 ** rng.uniform(0.0, math.log10(4000.0), n - n // 2)])   # default box, widened box
    Flim = rng.uniform(1.0, 6.0, n)
    tgt = np.concatenate([rng.uniform(-30, 30, n // 3), -10.0 ** rng.uniform(-3, 4.2, n // 3), 10.0 ** rng.uniform(-3, 4.2, n - 2 * (n // 3))])
    rng.shuffle(tgt)
    lF = np.log10(1.0e-17 * Flim)
    logf = lF + tgt / aC
    # exact zeros of both signs and the doubles next to them: alphaC = 2, lF = -16.5 (cA = 33 exactly), and lF = 0 with logf = -0.0
    k = 8
    aC[:k] = 2.0
    lF[:k] = [-16.5, -16.5, -16.5, 0.0, 0.0, 0.0, -16.5, -16.5]
    logf[:k] = [-16.5, np.nextafter(-16.5, 0.0), np.nextafter(-16.5, -20.0), -0.0, 5e-324, -5e-324, -16.0, -17.0]
    cA = -aC * lF
    num = fma_exact(aC, logf, cA)
    b = -np.sqrt((16.0 / 9.0) / (aC * aC))
    V = 1.0 / (Flim * 10.0 ** b)
    umin = u_min_for(num)
    frac = rng.uniform(0, 1, n)
    u_t = umin * (1.0e6 * 0.99 / umin) ** (frac ** 2)                 # from the smallest admitted value up to 1e6, denser at the bottom
    u_t[::11] = umin[::11]
    u_t[5::11] = rng.uniform(30.0, 45.0, len(u_t[5::11]))               # around 37.5, where 1 - e^(-u) becomes exactly 1
    U = u_t / V
    u = U * V                                                           # the function's own product: one rounding of the exact product
    ws = [_w_of(v) for v in num]
    us = [mpf(a) * mpf(c) for a, c in zip(U, V)]
    ds = [1 - mp.exp(-v) for v in us]
    refs = [mp.log(w / 2) / d for w, d in zip(ws, ds)]
    ref = pair(refs)
    w, d = np.array([float(v) for v in ws]), np.array([float(v) for v in ds])
    W = np.zeros((n, 9))
    W[:, 0], W[:, 1], W[:, 2], W[:, 3], W[:, 4], W[:, 5], W[:, 6], W[:, 7], W[:, 8] = 42.6, LNOM0, -1.2, 0.25, aC, lF, V, LNOM0, cA
    npv = np_ln_fc(num) / (1.0 - np.exp(-u))
    pos = num >= 0.0
    refn = pair([mp.log(w_ / 2) for w_ in ws])
    return _finish({"w": f64(W), "logf": f64(logf), "U": f64(U), "num": num, "u": u, "wtrue": w, "dtrue": d, "ref": ref,
                    "yard": yard_E(ref[0], w, d), "np": npv, "aC": aC,
                    "noexp": {"sel": pos, "ref": (refn[0][pos], refn[1][pos]), "yard": yard_E(refn[0][pos], w[pos], 1.0),
                              "np": np_ln_fc(num[pos])}})


@functools.lru_cache(None)
def case_term_careful():
    """term_free_careful: each of its five -inf conditions on its own, on both sides of LF_UNDERFLOW; `want_inf` says which
    side.  The finite results are lnOm - lnom0 = (lnom0 + ln fc / d) - lnom0: the yardstick is E plus the two roundings at
    the size of lnom0 + ln fc / d."""
    rows = []          # (Lstar, c0f, c1, Q, aC, lF, V, lnom0, lum, logf, P, U, want_inf)
    T = LF_UNDERFLOW

    def row(c0f=0.0, lnom0=0.0, P=0.0, logf=0.0, U=50.0, lum=42.0, want=False):
        rows.append((42.0, c0f, 0.0, 1.0, 1.0, 0.0, 1.0, lnom0, lum, logf, P, U, want))

    for side, want in ((T + 0.01, True), (T - 0.01, False), (np.nextafter(T, 1e3), True), (T, False)):
        row(P=side, c0f=800.0, want=want)                                        # 1: v = P Q > T (lnT - lnom0 = 800 - v > -T)
    for side, want in ((-T - 0.2, True), (-T + 0.2, False)):
        row(c0f=side + 13.0, lnom0=13.0, logf=40.0, want=want)                   # 2: lnT - lnom0 < -T; lnOm = 13, term > -T
    # 3: lnOm < -T: ln fc(0) / d = -ln2 / d = -T -+ 0.05 at small u, lnT - lnom0 = +100 keeps the sum above -T
    for tgt, want in ((T + 0.05, True), (T - 0.05, False)):
        u = -math.log1p(-LN2 / tgt)
        row(c0f=100.0, U=u, want=want)
    for side, want in ((-345.2, True), (-345.0, False)):                         # 4: the sum alone: -400 + (-345.x)
        u = -math.log1p(-LN2 / -side)
        row(c0f=-400.0, U=u, want=want)
    row(logf=np.nan, want=True)                                                  # 5: NaN
    row(lum=np.nan, c0f=1.0, want=True)
    rows[-1] = rows[-1][:2] + (1.0,) + rows[-1][3:]                              # (c1 = 1 so that lum enters)
    row(want=False)
    a = np.array(rows, dtype=np.float64)
    # a seeded fill of ordinary sources: the inputs of term_free_fast with benign Schechter parts
    t = case_term_free()
    m = 1500
    W = np.concatenate([np.column_stack([a[:, 0], a[:, 1], a[:, 2], a[:, 3], a[:, 4], a[:, 5], a[:, 6], a[:, 7], np.zeros(len(a))]), t["w"][:m]])
    lum = np.concatenate([a[:, 8], np.full(m, 42.3)])
    logf = np.concatenate([a[:, 9], t["logf"][:m]])
    P = np.concatenate([a[:, 10], np.full(m, 2.0)])
    U = np.concatenate([a[:, 11], t["U"][:m]])
    want = np.concatenate([a[:, 12] > 0, np.zeros(m, dtype=bool)])
    aC, lF, V, lnom0 = W[:, 4], W[:, 5], W[:, 6], W[:, 7]
    num = aC * (logf - lF)                 # the careful form's own argument: the rounded difference times alphaC, rounded
    ws, ds, refs = [], [], []
    for i in range(len(num)):
        if want[i]:
            ws.append(mp.mpf(1)); ds.append(mp.mpf(1)); refs.append(-mp.inf)
            continue
        w_ = _w_of(num[i])
        d_ = 1 - mp.exp(-(mpf(U[i]) * mpf(V[i])))
        ws.append(w_); ds.append(d_); refs.append(mp.log(w_ / 2) / d_)
    ref = pair(refs)
    w, d = np.array([float(v) for v in ws]), np.array([float(v) for v in ds])
    with np.errstate(invalid="ignore"):
        yard = yard_E(np.where(want, 0.0, ref[0]), w, d) + 2.0 * U53 * (np.abs(lnom0) + np.abs(np.where(want, 0.0, ref[0])))
        npv = np.where(want, -np.inf, (lnom0 + np_ln_fc(num) / (1.0 - np.exp(-(U * V)))) - lnom0)
    return _finish({"w": f64(W), "lum": f64(lum), "logf": f64(logf), "P": f64(P), "U": f64(U), "want_inf": want, "ref": ref,
                    "yard": yard, "np": npv, "n_edges": len(a)})


# ---------------------------------------------------------------------------------------------- the z-evolving term
@functools.lru_cache(None)
def case_zevol():
    """lnT_zevol: Ls = (aL z2 + bL z) + cL and ph likewise, each operation rounded (the reference's order), t = lum - Ls,
    v = exp(ln10 t), lnT = fma(c1, t, fma(ln10, ph, lnln10)) - v.  References from the binary64 inputs; the yardsticks carry
    the roundings of the quadratic, which the exponential amplifies: dt = 2^-53 (|aL z2| + 2 |aL z2 + bL z| + 2 |Ls| + |t|)."""
    rng = np.random.default_rng(109)
    n = 4000
    z = rng.uniform(1.16, 1.90, n)
    z2 = z * z
    L = rng.uniform(42.0, 43.5, (3, n))
    ph3 = rng.uniform(-3.5, -1.5, (3, n))
    z1, zm, z3 = 1.20, 1.53, 1.86

    def quad(y1, y2, y3):
        a = ((y3 - y1) + (y2 - y1) * (z1 - z3) / (zm - z1)) / (z3 * z3 - z1 * z1 + (zm * zm - z1 * z1) * (z1 - z3) / (zm - z1))
        b = (y2 - y1 - a * (zm * zm - z1 * z1)) / (zm - z1)
        return a, b, y1 - a * z1 * z1 - b * z1
    aL, bL, cL = quad(*L)
    aP, bP, cP = quad(*ph3)
    c1 = LN10 * (rng.uniform(-3.0, 1.0, n) + 1.0)
    lum = rng.uniform(41.0, 44.5, n)
    # the clamps of fexp_c (grid nodes are not screened): ln10 t beyond 709 and below -750
    lum[:4] = [42.0 + 400.0, 42.0 - 400.0, 42.0 + 308.0, 42.0 - 323.5]
    aL[:4] = bL[:4] = 0.0
    cL[:4] = 42.0
    Wz = np.column_stack([aL, bL, cL, aP, bP, cP, c1, np.zeros(n)])
    Ls = [mpf(a) * mpf(q) + mpf(b) * mpf(x) + mpf(c) for a, b, c, x, q in zip(aL, bL, cL, z, z2)]
    Ph = [mpf(a) * mpf(q) + mpf(b) * mpf(x) + mpf(c) for a, b, c, x, q in zip(aP, bP, cP, z, z2)]
    ts = [mpf(l) - s for l, s in zip(lum, Ls)]
    clamp = lambda e: min(max(e, mp.mpf(-750)), mp.mpf(709))      # noqa: E731
    vs = [mp.exp(clamp(mp.mpf(LN10) * t)) for t in ts]
    lnT = [mpf(c) * t + (mp.mpf(LN10) * p + mp.mpf(LNLN10)) - v for c, t, p, v in zip(c1, ts, Ph, vs)]
    rv, rT = pair(vs), pair(lnT)
    t = np.array([float(x) for x in ts])
    Lsd, Phd = np.array([float(x) for x in Ls]), np.array([float(x) for x in Ph])

    def dq(a, b, s):
        return U53 * (np.abs(a * z2) + 2.0 * np.abs(a * z2 + b * z) + 2.0 * np.abs(s))
    dt = dq(aL, bL, Lsd) + U53 * np.abs(t)
    yv = ulp_of(rv) + np.abs(rv[0]) * (LN10 * dt + U53 * np.abs(LN10 * t))
    inner = np.abs(LN10 * Phd) + LNLN10
    yT = np.abs(c1) * dt + LN10 * dq(aP, bP, Phd) + U53 * (2.0 * inner + 2.0 * np.abs(c1 * t) + np.abs(rT[0])) + yv
    with np.errstate(over="ignore"):
        Ln = (aL * z2 + bL * z) + cL
        Pn = (aP * z2 + bP * z) + cP
        tn = lum - Ln
        vn = np.exp(np.clip(LN10 * tn, -750.0, 709.0))
        Tn = (c1 * tn + (LN10 * Pn + LNLN10)) - vn
    clamped = np.abs(LN10 * t) > 700.0
    return _finish({"w": f64(Wz), "lum": f64(lum), "z": f64(z), "z2": f64(z2), "clamped": clamped,
                    "v": {"ref": rv, "yard": yv, "np": vn}, "lnT": {"ref": rT, "yard": yT, "np": Tn}, "yard": yv})


# ---------------------------------------------------------------------------------------------- tables
def g_prime_over_g(num, gref):
    """|g'(num) / g(num)|, g' = 1 / (s^2 (s + num)), s = sqrt(1 + num^2)"""
    s = np.sqrt(1.0 + num * num)
    sn = np.where(num >= 0, s + num, 1.0 / (s - num))
    return 1.0 / (s * s * sn) / np.abs(gref)


def h_prime_over_h(y):
    """|h'(y) / h(y)| = ln10 10^y e^(-10^y) / (1 - e^(-10^y)) <= ln10"""
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        e = 10.0 ** y
        return np.where(e > 700.0, 0.0, LN10 * e * np.exp(-e) / -np.expm1(-e))


def lane_designs():
    """Lane centres (aC, cA, cYH, x_c) of the table probes, edge lists first.  cYs = cYH - 1 / (2 H_INV) as lf_prepare makes it.
    `kind`: 0 g boundary (+-1 ulp of x_c), 1 zero and tiny num, 2 h tie (H_INV (y - H_LO) an integer), 3 h half-integer,
    4 first / last pieces, 5 seeded fill.  With aC a power of two, lF = -16.5 and b = -1/2 every product is exact."""
    rng = np.random.default_rng(110)
    D = []
    lF, cY = -16.5, 17.0
    for nb in g_boundaries():
        aC = 8.0
        xc = lF + nb / aC
        for x in ulps_around(xc, (-1, 0, 1)):
            D.append((aC, -aC * lF, cY - H_LO, x, 0))
    for x in (lF, np.nextafter(lF, 0.0), np.nextafter(lF, -20.0)):
        D.append((2.0, 33.0, cY - H_LO, x, 1))
    for x in (-0.0, 0.0, 5e-324, -5e-324):                # lF = 0: cA = -0.0, so that num = -0.0 can come out of the fma
        D.append((2.0, -0.0, 2.0, x, 1))
    for m in range(1, H_N + 4):
        D.append((4.0, 66.0, cY - H_LO, m / H_INV - 19.5, 2))
        D.append((4.0, 66.0, cY - H_LO, (m + 0.5) / H_INV - 19.5, 3))
    # first and last pieces: g at num in [0, 1/32), just below G_HI - 2 margins, just above G_LO + 2 margins; h at its low end and tail
    for nb, yh in ((0.01, 2.0), (-0.01, 2.0), (G_HI - 2.01 * G_MARGIN, 4.5), (G_LO + 2.01 * G_MARGIN, 1.0), (1.0, 2.0001 * H_MARGIN),
                   (2.0, 1.0 / H_INV - 1e-9), (3.0, 4.11), (3.0, 4.2), (3.0, 9.0)):
        xc = lF + nb / 8.0
        D.append((8.0, 132.0, yh - xc, xc, 4))
    n = 1500
    aC = np.concatenate([rng.uniform(1.0, 7.0, n // 2), 10.0 ** rng.uniform(0, math.log10(4000.0), n - n // 2)])
    lFr = rng.uniform(-17.0, -16.2, n)
    nc = np.concatenate([rng.uniform(G_LO + 2.1 * G_MARGIN, G_HI - 2.1 * G_MARGIN, n - 400), rng.uniform(-1.0, 1.0, 400)])
    yh = rng.uniform(2.1 * H_MARGIN, 5.0, n)
    for i in range(n):
        xc = lFr[i] + nc[i] / aC[i]
        D.append((aC[i], -aC[i] * lFr[i], yh[i] - xc, xc, 5))
    return np.array(D)


@functools.lru_cache(None)
def case_table(st, noexp):
    """Lanes of ST flux neighbours around each design centre (x[ST / 2] = x_c), as wide as the key tests allow
    (aC width <= G_MARGIN, width <= H_MARGIN) or narrower, every npad in 0 .. ST-1 (padded slots: copies of the last source).
    NOEXP lanes are shifted to where the form is taken: y >= log10(37.5), h = 1 to 2^-54."""
    rng = np.random.default_rng(111 + 10 * st + int(noexp))
    D = lane_designs()
    n = len(D)
    aC, cA, cYH, xc, kind = D[:, 0].copy(), D[:, 1].copy(), D[:, 2].copy(), D[:, 3].copy(), D[:, 4].astype(int)
    if noexp:
        cYH = np.maximum(cYH, (1.58 + H_MARGIN - H_LO) - xc)
    Wd = np.minimum(G_MARGIN / aC, H_MARGIN) * (1.0 - 1e-9)
    Wd = Wd * np.where(rng.uniform(0, 1, n) < 0.5, 1.0, rng.uniform(0, 1, n))
    alpha = rng.choice([0.0, 1.0, 0.5, 0.3], n)
    # the key tests admit a lane when ALL its sources are inside the tables with room for the margins: at the ends of the
    # range the lane lies on the inner side of its centre
    n0 = aC * xc + cA
    alpha = np.where((xc + cYH < 3.1 * H_MARGIN) | (n0 < G_LO + 3.1 * G_MARGIN), 0.0, np.where(n0 > G_HI - 3.1 * G_MARGIN, 1.0, alpha))
    c = st // 2
    x = np.zeros((n, st))
    for i in range(n):
        below = np.sort(rng.uniform(-alpha[i] * Wd[i], 0.0, c))
        above = np.sort(rng.uniform(0.0, (1.0 - alpha[i]) * Wd[i], st - c - 1))
        if c:
            below[0] = -alpha[i] * Wd[i]
        if st - c - 1:
            above[-1] = (1.0 - alpha[i]) * Wd[i]
        x[i] = np.concatenate([xc[i] + below, [xc[i]], xc[i] + above])
    x = np.sort(x, axis=1)
    x[:, c] = xc                                           # (a tiny centre may have been rounded away by the offsets)
    x = np.sort(x, axis=1)
    keep = x[:, c] == xc
    npad = np.arange(n) % st
    npad[~keep] = 0
    for i in range(n):
        if npad[i]:
            x[i, st - npad[i]:] = x[i, st - npad[i] - 1]
    # a padded lane's centre slot may now hold the copy: the design's centre is whatever slot ST / 2 holds
    xc = x[:, c].copy()
    wk = np.column_stack([aC, cA, cYH - 0.5 / H_INV, cYH])
    numc = fma_exact(aC, xc, cA)
    # per-source arguments at 40 digits from the binary64 inputs, references, yardstick
    ref_sum, abs_sum, cond = [], np.zeros(n), np.zeros(n)
    num = np.zeros((n, st))
    y = np.zeros((n, st))
    for i in range(n):
        tot = mp.mpf(0)
        for k in range(st - npad[i]):
            nm = mpf(aC[i]) * mpf(x[i, k]) + mpf(cA[i])
            yy = mpf(x[i, k]) + mpf(cYH[i]) + mp.mpf(H_LO)
            num[i, k], y[i, k] = float(nm), float(yy)
            g = g_ref(nm)
            h = h_ref(yy)
            term = g * h
            tot += term
            gf = float(g)
            # roundings of the affine maps, amplified: sc = +-cA + (1 - v_lo) is rounded at the size of cA, t = sa x + sc
            # at the size of the piece; dy at the size of cYH
            cg = float(g_prime_over_g(np.float64(num[i, k]), gf)) * U53 * (abs(cA[i]) + 2.0 * (abs(num[i, k]) + 1.0))
            ch = 0.0 if noexp else float(h_prime_over_h(np.float64(y[i, k]))) * U53 * (abs(cYH[i]) + abs(x[i, k]) + 2.0 * abs(y[i, k] - H_LO))
            abs_sum[i] += abs(float(term))
            cond[i] += abs(float(term)) * (cg + ch)
        for k in range(st - npad[i], st):
            num[i, k], y[i, k] = num[i, st - npad[i] - 1], y[i, st - npad[i] - 1]
        ref_sum.append(tot)
    ref = pair(ref_sum)
    # table error of both factors, the conditioning above, 2 x 8 roundings of the two Horner chains, the product, the ST
    # adds and the padding's fma
    yard = abs_sum * (G_ERR + (0.0 if noexp else H_ERR) + U53 * (18 + st)) + cond
    nck = np.repeat(numc[:, None], st, 1)
    gp = g_eval(num.ravel(), nck.ravel()).reshape(n, st)
    hp = np.ones((n, st)) if noexp else h_eval(y.ravel(), np.repeat(y[:, c:c + 1], st, 1).ravel()).reshape(n, st)
    live = np.arange(st)[None, :] < (st - npad)[:, None]
    npv = np.sum(np.where(live, gp * hp, 0.0), axis=1)
    # The pieces the NumPy lookup picks, restated from test_tables_cpu.g_eval (which does not return its index) for ONE
    # use: tests/test_terms_cpu.py checks with it that the lanes reach every piece.  The device's choice is not compared
    # with this copy but with g_eval itself (tests/test_gpu_terms.py).
    v = np.abs(numc) + 1.0
    hi = (v.view(np.int64) >> 32) & (0xffffffff << (20 - G_BITS))
    pg = (hi >> (20 - G_BITS)) - (0x3ff << G_BITS) + np.where(numc < 0, G_NPOS, 0)
    hx = H_INV * (xc + cYH)                          # exact for the tie designs (checked by the CPU test)
    return _finish({"wk": f64(wk), "x": f64(x), "npad": npad.astype(np.int32), "kind": kind, "numc": numc, "pg": pg, "hx": hx,
                    "ref": ref, "yard": yard, "np": npv, "st": st, "noexp": noexp, "abs_sum": abs_sum})


@functools.lru_cache(None)
def case_cells():
    """Cell records {x_c, S_0 .. S_8}: 1, 4 and 1000 sources at offsets filling rho = min(CELL_RHO_H, CELL_RHO_G / aC) (and all
    at +rho), midpoints at the designs' centres; the power sums are formed at 40 digits and rounded once."""
    rng = np.random.default_rng(112)
    D = lane_designs()
    sel = np.concatenate([np.where(D[:, 4] == k)[0][::s] for k, s in ((0, 9), (1, 1), (2, 5), (3, 9), (4, 1), (5, 12))])
    D = D[sel]
    n = len(D)
    aC, cA, cYH, xc = D[:, 0], D[:, 1], D[:, 2], D[:, 3]
    nsrc = np.array([1, 4, 4][:3] * (n // 3 + 1))[:n]
    nsrc[rng.choice(n, 8, replace=False)] = 1000
    rho = np.minimum(CELL_RHO_H, CELL_RHO_G / aC) * (1.0 - 1e-9)
    cd = np.zeros((n, CELL_REC))
    refs, abs_sum, cond, npv = [], np.zeros(n), np.zeros(n), np.zeros(n)
    numc = fma_exact(aC, xc, cA)
    for i in range(n):
        off = rng.uniform(-rho[i], rho[i], nsrc[i])
        if i % 4 == 1:
            off[:] = rho[i]
        if nsrc[i] == 1 and i % 2 == 0:
            off[:] = 0.0
        xs = xc[i] + off                                   # the sources are doubles
        d = [mpf(v) - mpf(xc[i]) for v in xs]
        cd[i, 0] = xc[i]
        for j in range(9):
            cd[i, 1 + j] = float(mp.fsum(v ** j for v in d))
        tot = mp.mpf(0)
        nums, ys = np.zeros(nsrc[i]), np.zeros(nsrc[i])
        for k, v in enumerate(xs):
            nm = mpf(aC[i]) * mpf(v) + mpf(cA[i])
            yy = mpf(v) + mpf(cYH[i]) + mp.mpf(H_LO)
            nums[k], ys[k] = float(nm), float(yy)
            term = g_ref(nm) * h_ref(yy)
            tot += term
            abs_sum[i] += abs(float(term))
        gm = float(g_ref(mpf(numc[i])))
        cond[i] = abs_sum[i] * (float(g_prime_over_g(np.float64(numc[i]), gm)) * U53 * (abs(cA[i]) + 2.0 * (abs(numc[i]) + 1.0)) +
                                float(h_prime_over_h(np.float64(ys.mean()))) * U53 * (abs(cYH[i]) + abs(xc[i]) + 8.0))
        refs.append(tot)
        yc = np.full(nsrc[i], float(mpf(xc[i]) + mpf(cYH[i]) + mp.mpf(H_LO)))
        npv[i] = np.sum(g_eval(nums, np.full(nsrc[i], numc[i])) * h_eval(ys, yc))
    ref = pair(refs)
    # tables, dropped orders (< 1e-16, tests/test_tables_cpu.py::test_cell_truncation_bound), and the roundings of cell_sum:
    # two Taylor shifts (2 x 14), the product series (8), the dot product with the power sums (9), the sums' own rounding (1)
    yard = abs_sum * (G_ERR + H_ERR + 1.0e-16 + U53 * 46) + cond
    wk = np.column_stack([aC, cA, cYH - 0.5 / H_INV, cYH])
    return _finish({"wk": f64(wk), "cd": f64(cd), "nsrc": nsrc, "ref": ref, "yard": yard, "np": npv, "rho": rho, "aC": aC})


# ---------------------------------------------------------------------------------------------- reductions
@functools.lru_cache(None)
def reduction_vectors(width=64):
    """(exact, seeded): vectors whose sum is exact in any order (one-hot, small integers, mixed powers of two within 50
    binades), and seeded doubles to be checked against math.fsum with (n - 1) 2^-53 sum|x|"""
    rng = np.random.default_rng(113)
    onehot = np.eye(width) * 3.0
    ints = rng.integers(-1000, 1000, (40, width)).astype(np.float64)
    pw = np.ldexp(rng.choice([-1.0, 1.0, 3.0, -5.0], (40, width)), rng.integers(-20, 20, (40, width)))
    lanes = np.tile(np.arange(1.0, width + 1.0), (1, 1)) ** 2                    # lane-dependent weights: a lane counted twice shows
    exact = np.concatenate([onehot, ints, pw, lanes])
    seeded = np.concatenate([rng.normal(0, 1, (60, width)), 10.0 ** rng.uniform(-8, 8, (30, width)) * rng.choice([-1, 1], (30, width)),
                             -rng.uniform(0.5, 800.0, (30, width))])
    return f64(exact), f64(seeded)
