"""Inputs, 40-digit references and yardsticks for the element-wise probes of two post-fit kernels through their public
entries: veffd_partial<FCMIN> (csrc/lf_veffdraws.h, entry lf_veff_draws) and stage 1 of lf_bands<3> / lf_bands<7>
(bands_eval, csrc/lf_bands.h, entry lf_lumfunc_quantiles with values), in tests/lf_gradproblib.py's format and under its
rules.  No GPU here: tests/test_postterms_cpu.py checks the generators, measures the NumPy binary64 figures behind the caps
(the twins veff.veff_draws and lfbands.lf_values) and replays the summation rule on the twin; tests/test_gpu_postterms.py
runs the same cases on the device.  DESIGN.md section 3.28.

A case holds the exact binary64 inputs, `ref` (hi, lo) from mpmath at 40 digits (80 where the Fleming curve cancels), `yard`,
`np` (the twin's values at the same elements) and the elements' places: with one source per bin values[r][b] of lf_veff_draws
is w_b(d_r) itself (0.0 + (0.0 + w) = w), and values=True of lf_lumfunc_quantiles returns v[r][p].  Only some (row, source) /
(record, point) pairs carry a reference; the others are computed and ignored.  Yardsticks, from the formula and the format:

  veffd_partial's weight w = 1 / (pref0 fc^(1/d) vol):  lf_gradproblib.case_veff's,
      2^-53 |w| (1 + 1 / fc) (1 + |ln fc / d|)    (the last factor for fcmin > 0 only)
    - 0.5 (1 + num / sqrt(1 + num^2)) cancels for num << 0, which 1 / fc carries, and a relative error of fc is raised to the
    power 1 / d.  The kernel's extra quotient ((1 / (pref0 vol)) / fc against veff_weights' 1 / ((pref0 fc) vol)) and the
    product Flim * knee that forms ftau cost a constant number of roundings: they show in the figure, not in the yardstick.
    On the rows with alpha < 0 (not case_veff's ground: there fc -> 1 for f << Flim while 1 / d grows) two more terms of the
    same formula are added, (1 / d) (1 + |ln fc / d|) inside the bracket: see case_veffd.

  bands_eval<3>: v = rec1 10^(t c1) exp(-10^t), t = logL - rec0, c1 = rec2 (the record as the device receives it):
      2^-53 |v| (3 + ln10 |t c1| + 10^t (1 + ln10 |t|))
    - 3: the two transcendental results and the two products (1 + 1 + 1/2 + 1/2);  ln10 |t c1|: the rounded product t c1 is
    the exponent of the first power, d ln(10^x) = ln10 dx;  10^t: the rounded 10^t is the exponent of exp, d ln(exp(-y)) =
    -dy = -10^t (dy / y);  10^t ln10 |t|: a relative rounding of t moves 10^t by ln10 |t| of itself.
  bands_eval<7>: rec0 -> L*(z) = aL z z + bL z + cL and rec1 -> ln10 10^(phi*(z)), phi*(z) the same with the phi coefficients:
      the above with 5 for 3 (exp10(phi*)'s result, the product with ln10 and ln10's own rounding), plus
      2^-53 |v| ln10 ((|c1| + 10^t) (|aL z z| + |bL z| + |cL|) + (|aphi z z| + |bphi z| + |cphi|))
    - every addend of a quadratic is rounded at its own magnitude, and d ln v / d L* = -ln10 (c1 - 10^t), d ln v / d phi* = ln10.
  A point whose 40-digit value is below the smallest normal number is held absolutely, |dev - ref| <= 4 x 2^-1074, and left
  out of the relative figure (`sub`).

Caps on max err / yard: max(2, 4 x the twin's figure on the same elements), CAPS below."""
import functools
import math

import numpy as np

import lf_gradproblib as GP
from lumfuncmcmc_amd import hostsetup as hs, lfbands, synth, veff

mp, mpf, U53, _case, measure, cap_from = GP.mp, GP.mpf, GP.U53, GP._case, GP.measure, GP.cap_from
MLN10 = GP.MLN10
TINY = GP.TINY
TINY_NORMAL = float(np.finfo(np.float64).tiny)
ABS_SUB = 4.0 * TINY                   # the absolute bound of a point below TINY_NORMAL

# The twins' figures (max err / yard of veff.veff_draws and lfbands.lf_values), measured on the CPU by
# tests/test_postterms_cpu.py::test_numpy_figures_behind_the_caps on 2026-10-20, which fails when one moves by more than 1 %;
# CAPS = max(2, 4 x figure).  DESIGN.md section 3.28 has the device's figures next to them.
# "veffd_w": the probe rows with alpha > 0 at fcmin = synth.FCMIN and 0, what the fits use; "veffd_w_x": the same rows at the
# added fcmin 0.3, whose figure one element sets (alpha 0.6, f / Flim 1e-3, w = 1e218: d = 1 - exp(-f / ftau) cancels, which
# case_veff's yardstick does not carry) - a cap of its own keeps it from loosening the others; "veffd_w_neg": alpha < 0, under
# the yardstick with the two further terms (case_veffd).
NUMPY_FIGS = {"veffd_w": 1.358, "veffd_w_x": 5.009, "veffd_w_neg": 1.543, "bands_v3": 0.552, "bands_v7": 0.745}
CAPS = {"veffd_w": 5.43, "veffd_w_x": 20.0, "veffd_w_neg": 6.17, "bands_v3": 2.21, "bands_v7": 2.98}

# ---------------------------------------------------------------------------------------------- lf_veff_draws
PREF0 = GP.VEFF_PREF0
NF = 16                                # VEFFD_MAXF
R = 257                                # row 256: lane 0 of a second tile, 255 idle lanes behind it
N_SRC = 1020                           # one bin each (nbin <= 1024)
PER_ROW = 170                          # referenced sources per probe row
# the probe rows; rows k and k + 6 of this list share alpha and the 170 sources they are referenced on (100: mid-wave, no edge)
PROBE_ROWS = (0, 1, 63, 64, 127, 128, 191, 192, 254, 255, 256, 100)
# a negative alpha is inside lf_veff_draws' accepted domain (finite and non-zero: lfmcmc.hip), so are all fcmin (no check;
# fcmin > 0 selects the modified curve): one more in (0, 0.5)
GROUP_ALPHAS = (0.6, -4.56, -0.6, 10.0, 4.56, -10.0)
FCMINS = (synth.FCMIN, 0.0, 0.3)
UNDERFLOW_RULE = -600.0                # ln fc / d below this: fc^(1/d) has no relative accuracy to speak of (case_veff)
VOL_ALL = 1.0e6
ZERO_VOL = {7: 0.0, 23: -1.0, 500: 0.0, 1001: -3.5e5}
Q = (0.0, 16.0, 50.0, 84.0, 100.0)


def probe_alpha(k):
    return GROUP_ALPHAS[k % 6]


def filler_draws(nf, nrows, seed=100):
    """draws of tests/test_gpu_veffdraws.py's kind: N(synth.FLIM, 0.1) (the five fields repeated) and N(synth.ALPHA_C, 0.1),
    clipped into the prior box"""
    rng = np.random.default_rng(seed + nf)
    flim0 = [synth.FLIM[f % len(synth.FLIM)] for f in range(nf)]
    cols = [np.clip(rng.normal(f, 0.1, nrows), *synth.FLIM_LIMS) * 1.0e-17 for f in flim0]
    return np.ascontiguousarray(np.column_stack(cols + [np.clip(rng.normal(synth.ALPHA_C, 0.1, nrows), *synth.ALPHA_LIMS)]))


@functools.lru_cache(None)
def veffd_draws():
    """[R][NF + 1]: filler rows, and the twelve probe rows - sixteen distinct Flim log-spread over the prior box, another
    permutation on every row (a transposed or shifted read of the [field][lane] table lands on another value), and the
    group's alpha"""
    rng = np.random.default_rng(230)
    d = filler_draws(NF, R)
    spread = np.geomspace(synth.FLIM_LIMS[0], synth.FLIM_LIMS[1], NF) * 1.0e-17
    perms = []
    for k, r in enumerate(PROBE_ROWS):
        while True:
            p = rng.permutation(NF)
            if not any(np.array_equal(p, q) for q in perms):
                break
        perms.append(p)
        d[r, :NF] = spread[p]
        d[r, NF] = probe_alpha(k)
    d.setflags(write=False)
    return d


def _fleming_mp(f, fl, alpha, fcmin):
    """(fc of the plain curve, 1 / d) at the working precision"""
    a = mpf(alpha)
    num = a * mp.log10(mpf(f) / mpf(fl))
    fc = (1 + num / mp.sqrt(1 + num * num)) / 2
    if not fcmin:
        return fc, mp.mpf(1)
    aa = (2 * mpf(fcmin) - 1) ** 2
    ftau = mpf(fl) * mp.mpf(10) ** (-mp.sqrt(abs(aa / (1 - aa)) / (a * a)))
    return fc, 1 / (1 - mp.exp(-mpf(f) / ftau))


@functools.lru_cache(None)
def veffd_catalogue(fcmin):
    """N_SRC sources, one per bin.  Source i: group g = i % 6, place j = i // 6 in the group, field j % 16 (every field used);
    its flux is laid out against the Flim of its field on probe row g (j < 85) or g + 6 (j >= 85): f = Flim, f = ftau (the
    twin's, at synth.FCMIN for the plain curve) and the two neighbouring doubles of each, both ends 1e-3 and 1e3, then f / Flim
    log-uniform over 1e-3 .. 1e3.  lf_gradproblib.case_veff's rule: with fcmin > 0 a flux whose ln fc / d < -600 on the row it is
    laid out against is drawn again from [0.1, 1e3] Flim (`redrawn`).  It is referenced on the other row of its group too, whose
    Flim for the field may be up to the whole prior box higher: where it underflows there by the same rule the flux is kept and
    that one element carries no reference (case_veffd's `dropped`)."""
    rng = np.random.default_rng(231 + int(round(100 * fcmin)))
    d = veffd_draws()
    half = PER_ROW // 2
    i = np.arange(N_SRC)
    g, j = i % 6, i // 6
    field = j % NF
    krow = g + 6 * (j // half)
    flim = d[np.array(PROBE_ROWS)[krow], field]
    alpha = np.array([probe_alpha(k) for k in krow])
    jj = j % half
    ftau = np.array([hs.inverse_fleming(fl, al, fcmin or synth.FCMIN) for fl, al in zip(flim, alpha)])
    flux = flim * 10.0 ** rng.uniform(-3.0, 3.0, N_SRC)
    edge = {0: flim, 1: np.nextafter(flim, 0.0), 2: np.nextafter(flim, 1.0), 3: ftau, 4: np.nextafter(ftau, 0.0),
            5: np.nextafter(ftau, 1.0), 6: flim * 1.0e-3, 7: flim * 1.0e3}
    for e, v in edge.items():
        flux = np.where(jj == e, v, flux)
    redrawn = np.zeros(N_SRC, dtype=bool)
    if fcmin:
        for s in range(N_SRC):
            while True:
                fc, ex = _fleming_mp(flux[s], flim[s], alpha[s], fcmin)
                if mp.log(fc) * ex > UNDERFLOW_RULE:
                    break
                flux[s] = 10.0 ** rng.uniform(-1.0, 3.0) * flim[s]
                redrawn[s] = True
    vol = rng.uniform(1.0e5, 5.0e6, N_SRC)
    for s, v in ZERO_VOL.items():
        vol[s] = v
    out = {"flux": GP.L.f64(flux), "field": field.astype(np.int64), "vol": GP.L.f64(vol), "group": g, "krow": krow, "edge": jj < len(edge),
           "redrawn": redrawn, "flim_laid": flim}
    for v in out.values():
        v.setflags(write=False)
    return out


def veffd_pairs():
    """(k, rows, src): the probe row's place k in PROBE_ROWS [12][170], its row in the draws, and the referenced sources"""
    k = np.repeat(np.arange(12), PER_ROW).reshape(12, PER_ROW)
    src = np.array([np.arange(kk % 6, N_SRC, 6) for kk in range(12)])
    return k, np.array(PROBE_ROWS)[k], src


@functools.lru_cache(None)
def case_veffd(fcmin):
    """{per_source_vol: case} for one fcmin: ref / yard / np over the referenced (row, source) elements of veffd_pairs(), flat;
    `k`, `row`, `src` say where each is.  A source with vol <= 0 has the reference 0 and must be exactly +0 (`zero`).  `dropped`:
    the elements on a source's partner row that underflow by the redraw rule (see veffd_catalogue).  Yardstick: case_veff's on
    the rows with alpha > 0; on those with alpha < 0, which case_veff's was not made for, two more terms of the same formula -
    fc within 1e-4 of 1 is rounded at 2^-53 of itself and raised to 1 / d, and d = 1 - exp(-f / ftau) cancels for f << ftau, a
    relative 2^-53 / d of the exponent: 2^-53 |w| ((1 + 1 / fc) (1 + |ln fc / d|) + (1 / d) (1 + |ln fc / d|))."""
    cat, d = veffd_catalogue(fcmin), veffd_draws()
    k2, _, src2 = veffd_pairs()
    refs = {True: [], False: []}
    yard = {True: [], False: []}
    ks, srcs, dropped = [], [], 0
    with mp.workdps(80):          # (1 + num / sqrt(1 + num^2) loses 2 log10 |num| digits for num << 0)
        for a in range(12):
            r = PROBE_ROWS[a]
            for s in src2[a]:
                fc, ex = _fleming_mp(cat["flux"][s], d[r, cat["field"][s]], d[r, NF], fcmin)
                l = abs(mp.log(fc) * ex)
                if fcmin and -l <= UNDERFLOW_RULE:
                    assert a != cat["krow"][s]
                    dropped += 1
                    continue
                cond = (1 + 1 / fc) * ((1 + l) if fcmin else 1)
                if fcmin and d[r, NF] < 0:
                    cond += ex * (1 + l)
                base = 1 / (mpf(PREF0) * fc ** ex)
                ks.append(a)
                srcs.append(s)
                for ps in (True, False):
                    v = mpf(cat["vol"][s]) if ps else mpf(VOL_ALL)
                    if v <= 0:
                        refs[ps].append(mp.mpf(0))
                        yard[ps].append(TINY)
                    else:
                        w = base / v
                        refs[ps].append(+w)
                        yard[ps].append(float(mp.mpf(U53) * w * cond))
    k, src = np.array(ks), np.array(srcs)
    out = {}
    for ps in (True, False):
        tw = veffd_twin(fcmin, ps)
        out[ps] = _case(refs[ps], np.array(yard[ps]), tw[k, src], k=k, row=np.array(PROBE_ROWS)[k], src=src, dropped=dropped,
                        zero=(cat["vol"][src] <= 0) if ps else np.zeros(k.size, dtype=bool), fcmin=fcmin, per_source=ps)
    return out


@functools.lru_cache(None)
def veffd_twin(fcmin, per_source):
    """veff.veff_draws' weight of every source under the twelve probe rows, [12][N_SRC] (one bin per source: 0 + w is w)"""
    cat, d = veffd_catalogue(fcmin), veffd_draws()
    with np.errstate(all="ignore"):
        w = veff.veff_draws(cat["flux"], cat["field"], cat["vol"] if per_source else VOL_ALL, PREF0, fcmin, np.arange(N_SRC), N_SRC,
                            d[list(PROBE_ROWS)])
    w.setflags(write=False)
    return w


def cap_name(fcmin, alpha):
    """the cap an element is held by: "veffd_w" for alpha > 0 at the fcmin the fits use (synth.FCMIN and 0), "veffd_w_x" for
    alpha > 0 at the added fcmin, "veffd_w_neg" for alpha < 0"""
    return "veffd_w_neg" if alpha < 0 else "veffd_w" if fcmin in (synth.FCMIN, 0.0) else "veffd_w_x"


def veffd_figures(case, got):
    """{cap_name: (max err / yard, element)} of the elements `got` of one case, by the sign of alpha"""
    neg = np.array([probe_alpha(k) < 0 for k in case["k"]])
    out = {}
    for al, mask in ((1.0, ~neg), (-1.0, neg)):
        c = dict(case)
        c["exempt"] = ~mask
        out[cap_name(case["fcmin"], al)] = measure(c, got)
    return out


def veffd_elements(case, values):
    """the case's elements out of values[R][N_SRC]"""
    return np.asarray(values)[case["row"], case["src"]]


def veffd_where(case, i, fcmin):
    """the input at element i, for the printed figures"""
    cat, d = veffd_catalogue(fcmin), veffd_draws()
    s, r = int(case["src"][i]), int(case["row"][i])
    fl = d[r, cat["field"][s]]
    return "row %d alpha %g field %d Flim %.6e f / Flim %.9g vol %s" % (r, d[r, NF], cat["field"][s], fl, cat["flux"][s] / fl,
                                                                           ("%.6g" % cat["vol"][s]) if case["per_source"] else "shared")


# ---------------------------------------------------------------------------------------------- the underflow side
def _twin_w(flux, flim, alpha, fcmin, vol=VOL_ALL):
    with np.errstate(all="ignore"):
        return 1.0 / (PREF0 * hs.fleming(np.asarray(flux, dtype=np.float64), flim, alpha, fcmin) * vol)


def _flux_for(target, flim, alpha, fcmin):
    """the flux below Flim at which ln(fc^(1/d)) of the twin's curve is `target` (it rises with the flux)"""
    def lnp(x):
        fc, ex = _fleming_mp(x * flim, flim, alpha, fcmin)
        return mp.log(fc) * ex
    lo, hi = 1.0e-6, 1.0
    for _ in range(60):
        mid = math.sqrt(lo * hi)
        lo, hi = (mid, hi) if lnp(mid) < target else (lo, mid)
    return lo * flim


@functools.lru_cache(None)
def underflow_sources(fcmin):
    """8 sources in fields 0 .. 7 whose fc^(1/d) under the nominal filler draw is subnormal (ln = -712, -716, -730, -741) or 0
    (ln = -760, -1000, -5000, and f / Flim = 1e-20: d = 0, the exponent +inf); under the actual rows they cross between the
    three.  And 56 of veffd_catalogue(fcmin)'s sources, which the 8 must leave alone."""
    nom = np.array([synth.FLIM[f % len(synth.FLIM)] * 1.0e-17 for f in range(NF)] + [synth.ALPHA_C])
    targets = (-712.0, -716.0, -730.0, -741.0, -760.0, -1000.0, -5000.0)
    flux = [_flux_for(t, nom[f], nom[NF], fcmin) for f, t in enumerate(targets)] + [1.0e-20 * nom[7]]
    cat = veffd_catalogue(fcmin)
    base = np.arange(0, N_SRC, 18)[:56]
    return {"flux": np.concatenate([cat["flux"][base], flux]), "field": np.concatenate([cat["field"][base], np.arange(8)]),
            "vol": np.concatenate([cat["vol"][base], np.full(8, 7.0e5)]), "n_base": len(base)}


@functools.lru_cache(None)
def quantile_case(fcmin=synth.FCMIN):
    """One source per bin under R rows that differ in Flim alone (alpha = 10, Flim a shuffled geometric ramp over the prior
    box, the same for every field): a source is +inf on exactly the rows whose Flim is above its threshold.  `count` +inf rows
    per bin as the twin has them: none, 1, 41, 128, 129, 216, 256 and all 257."""
    rng = np.random.default_rng(233)
    ramp = np.geomspace(synth.FLIM_LIMS[0], synth.FLIM_LIMS[1], R) * 1.0e-17
    ramp = ramp[rng.permutation(R)]
    draws = np.ascontiguousarray(np.column_stack([np.tile(ramp[:, None], (1, NF)), np.full(R, 10.0)]))

    def count(f):
        return int(np.isinf(_twin_w(f, ramp, 10.0, fcmin)).sum())

    def edge(kk):                        # the largest flux with at least kk rows +inf
        lo, hi = 1.0e-22, 1.0e-15
        for _ in range(80):
            mid = math.sqrt(lo * hi)
            lo, hi = (mid, hi) if count(mid) >= kk else (lo, mid)
        return lo
    counts = (0, 1, 41, 128, 129, 216, 256, 257)
    flux = []
    for kk in counts:                    # the middle of the fluxes that have exactly kk rows +inf
        flux.append(2.0 * edge(1) if kk == 0 else 0.5 * edge(R) if kk == R else math.sqrt(edge(kk + 1) * edge(kk)))
    flux = np.array(flux)
    got = np.array([count(f) for f in flux])
    return {"flux": flux, "field": np.arange(len(flux)) % NF, "draws": draws, "count": got, "planned": np.array(counts)}


# ---------------------------------------------------------------------------------------------- the order of summation
ORDER_BINS = (2, 255, 256, 257, 513)
ORDER_ROWS = (0, 255, 256)


@functools.lru_cache(None)
def order_case():
    """The regrouped call: `idx` [1283 + 6] places in veffd_catalogue's sources, shuffled, with bin_of giving bins of 2, 255,
    256, 257 and 513 sources, and 6 sources outside [0, nbin), which are dropped.  A source is laid out for the two rows of its
    group only and may underflow to +inf on another row, where a sum would say nothing: `idx` takes the sources whose twin
    weight stays below 1e6 on ORDER_ROWS at every fcmin and volume form (each once, then again at random)."""
    rng = np.random.default_rng(234)
    ks = [PROBE_ROWS.index(r) for r in ORDER_ROWS]
    ok = np.ones(N_SRC, dtype=bool)
    for fm in FCMINS:
        for ps in (True, False):
            ok &= np.all(veffd_twin(fm, ps)[ks] < 1.0e6, axis=0)
    elig = np.flatnonzero(ok)
    m = sum(ORDER_BINS) + 6
    idx = np.concatenate([elig, rng.choice(elig, m - len(elig), replace=True)])
    bin_of = np.concatenate([np.full(c, b) for b, c in enumerate(ORDER_BINS)] + [[-1, -7, len(ORDER_BINS), len(ORDER_BINS) + 3, -1, 2 ** 20]])
    p = rng.permutation(m)
    return {"idx": idx[p], "bin_of": bin_of[p].astype(np.int64), "nbin": len(ORDER_BINS), "eligible": elig}


def replay_sums(w, bin_of, nbin, chunk):
    """lf_veff_draws' order of summation, stated: the sources of a bin in input order (the stable sort), cut into chunks of
    `chunk`; within a chunk acc = 0.0, acc += w; then s = 0.0, s += acc in chunk order.  Python floats: binary64, one rounding
    per addition, no pairwise regrouping."""
    out = np.zeros(nbin)
    w = [float(v) for v in w]
    for b in range(nbin):
        members = [i for i, bb in enumerate(bin_of) if bb == b]
        s = 0.0
        for c0 in range(0, len(members), chunk):
            acc = 0.0
            for i in members[c0:c0 + chunk]:
                acc += w[i]
            s += acc
        out[b] = s
    return out


# ---------------------------------------------------------------------------------------------- bands_eval
C1S = (-2.5, -1.0, -0.5, 0.0, 0.5, 1.5)                  # alpha + 1; alpha = c1 - 1 is exact, and so is the host's alpha + 1
T_LIN = np.linspace(-6.0, 2.8, 23)
T_CROSS = (0.0, 1.0, 2.0, math.log10(700.0))             # 10^t crosses 1, 10, 100, 700
NPTS = len(T_LIN) + 3 * len(T_CROSS)
B3_GROUPS = ((42.5, -1.0), (40.25, 4.0), (44.75, -0.6))  # (L*, phi*) of the NP = 3 records; six alpha + 1 each (see case_bands3)
PIV = (1.2, 1.53, 1.86)


def _lattice_logl(lstar_of, zs):
    """logL of the NPTS points of one record group: L* + t, and at each crossing the double nearest to L* + t with its two
    neighbours (t = 0: logL = L* itself, t = -+1 ulp of L*)"""
    out = []
    for i, t in enumerate(T_LIN):
        out.append(float(lstar_of(zs[i]) + mpf(t)))
    for c, t in enumerate(T_CROSS):
        for j, step in enumerate((0, -1, 1)):
            x = np.float64(float(lstar_of(zs[len(T_LIN) + 3 * c + j]) + mpf(t)))
            out.append(float(x if step == 0 else np.nextafter(x, np.inf * step)))
    return np.array(out)


def _bands_ref(pref_mp, t, c1, extra, const):
    """(v, yard) at 40 digits: v = pref 10^(t c1) exp(-10^t)"""
    p10 = mp.exp(MLN10 * t)
    v = pref_mp * mp.exp(MLN10 * t * c1) * mp.exp(-p10)
    return v, float(mp.mpf(U53) * abs(v) * (const + MLN10 * abs(t * c1) + p10 * (1 + MLN10 * abs(t)) + extra))


def _finish_bands(refs, yard, npv, **kw):
    c = _case(refs, yard, npv, **kw)
    c["sub"] = np.array([abs(v) < mpf(TINY_NORMAL) for v in refs])
    c["exempt"] = c["sub"]
    return c


@functools.lru_cache(None)
def case_bands3():
    """lf_bands<3>: 18 draws (L*, phi*, alpha) - B3_GROUPS x C1S - and 3 x NPTS points; record r is referenced on its group's
    points.  The reference starts from the record as the device receives it: {L*, ln10 * pow(10, phi*) in the host's binary64,
    alpha + 1}."""
    draws = np.array([[ls, ph, c1 - 1.0] for ls, ph in B3_GROUPS for c1 in C1S])
    logL = np.concatenate([_lattice_logl(lambda z, ls=ls: mpf(ls), np.zeros(NPTS)) for ls, _ in B3_GROUPS])
    rr = np.repeat(np.arange(len(draws)), NPTS)
    pp = np.concatenate([np.arange(NPTS) + NPTS * (r // len(C1S)) for r in range(len(draws))])
    refs, yard = [], []
    for r, p in zip(rr, pp):
        ls, ph, al = draws[r]
        rec1 = GP.L.LN10 * math.pow(10.0, ph)
        v, y = _bands_ref(mpf(rec1), mpf(logL[p]) - mpf(ls), mpf(al + 1.0), 0, 3)
        refs.append(v)
        yard.append(y)
    npv = lfbands.lf_values("free", draws, logL)[rr, pp]
    return _finish_bands(refs, yard, npv, draws=GP.L.f64(draws), logL=GP.L.f64(logL), z=None, r=rr, p=pp, variant="free",
                         t=np.array([logL[p] - draws[r, 0] for r, p in zip(rr, pp)]))


def _quad_mp(co, z):
    z = mpf(z)
    adds = [mpf(co[0]) * z * z, mpf(co[1]) * z, mpf(co[2])]
    return sum(adds), sum(abs(a) for a in adds), max(abs(a) for a in adds)


@functools.lru_cache(None)
def case_bands7():
    """lf_bands<7>: 12 records {aL, bL, cL, aphi, bphi, cphi, alpha}, NPTS points of its own each (P = 12 NPTS), z in [1.1, 2.0].
    Records 0 .. 5: the quadratics through ordinary pivot values (hostsetup.get_quad_coef), z over the whole range.  Records
    6 .. 11: L*(z) = 2e4 (z - z0)^2 + 42.5 and phi*(z) = 2e3 (z - z0)^2 + 4 written out as coefficients, z within 0.02 of z0:
    a z^2 + b z + c cancels to below 1e-3 of its largest term (`cancel`: the ratio per element).  logL = L*(z) + t from the
    40-digit L*(z)."""
    rng = np.random.default_rng(235)
    nrec = 12
    recs, zs = [], []
    for r in range(nrec):
        c1 = C1S[r % 6]
        if r < 6:
            lp = 42.5 + rng.uniform(-0.4, 0.4, 3)
            pp_ = (-3.0 if r == 0 else 4.0) + rng.uniform(-0.5, 0.5, 3)
            co = list(hs.get_quad_coef(*lp, *PIV)) + list(hs.get_quad_coef(*pp_, *PIV))
            z = rng.uniform(1.1, 2.0, NPTS)
            z[0], z[1] = 1.1, 2.0
        else:
            z0 = 1.15 + 0.16 * (r - 6)
            co = [2.0e4, -2.0 * 2.0e4 * z0, 2.0e4 * z0 * z0 + 42.5, 2.0e3, -2.0 * 2.0e3 * z0, 2.0e3 * z0 * z0 + 4.0]
            z = np.clip(z0 + rng.uniform(-0.02, 0.02, NPTS), 1.1, 2.0)
        recs.append([float(v) for v in co] + [c1 - 1.0])
        zs.append(z)
    draws = np.array(recs)
    z = np.concatenate(zs)
    logL = np.concatenate([_lattice_logl(lambda zz, r=r: _quad_mp(draws[r, 0:3], zz)[0], zs[r]) for r in range(nrec)])
    rr = np.repeat(np.arange(nrec), NPTS)
    pp = np.arange(nrec * NPTS)
    refs, yard, cancel, ts = [], [], [], []
    for r, p in zip(rr, pp):
        lstar, ml, big = _quad_mp(draws[r, 0:3], z[p])
        lphi, mphi, bigp = _quad_mp(draws[r, 3:6], z[p])
        c1 = mpf(draws[r, 6] + 1.0)
        t = mpf(logL[p]) - lstar
        extra = MLN10 * ((abs(c1) + mp.exp(MLN10 * t)) * ml + mphi)
        v, y = _bands_ref(MLN10 * mp.exp(MLN10 * lphi), t, c1, extra, 5)
        refs.append(v)
        yard.append(y)
        cancel.append(float(max(abs(lstar) / big, abs(lphi) / bigp)))
        ts.append(float(t))
    npv = lfbands.lf_values("zevol", draws, logL, z)[rr, pp]
    return _finish_bands(refs, yard, npv, draws=GP.L.f64(draws), logL=GP.L.f64(logL), z=GP.L.f64(z), r=rr, p=pp, variant="zevol",
                         t=np.array(ts), cancel=np.array(cancel))


def case_bands(np_rec):
    return case_bands3() if np_rec == 3 else case_bands7()


def bands_elements(case, v):
    return np.asarray(v)[case["r"], case["p"]]


def bands_where(case, i):
    r, p = int(case["r"][i]), int(case["p"][i])
    s = "record %d %s logL %.17g t %.6g" % (r, np.array2string(case["draws"][r], precision=8), case["logL"][p], case["t"][i])
    return s + ("" if case["z"] is None else " z %.17g" % case["z"][p])


def sub_errors(case, got):
    """|got - ref| at the elements below the smallest normal number"""
    return GP.L.err_of(got, case["ref"])[case["sub"]]
