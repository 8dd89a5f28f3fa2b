"""Inputs, 40-digit references and yardsticks for the element-wise probes of the four copies of the convolved likelihood's
node loop: deconv_source on the wide tables (csrc/lf_deconv_wide.h), lf_deconv_tile, lumpost_source (csrc/lf_lumpost.h) and
the lanes-on-nodes form of lf_vefftrue_part, in tests/lf_gradproblib.py's format and under its rules.  No GPU here:
tests/test_convterms_cpu.py measures the NumPy binary64 figures behind the caps and shows that the metric sees a subtle
error; tests/test_gpu_convterms.py runs the same cases through tests/conv_probe.hip.

Everything comes from lf_gradproblib.deconv_item_mp, which forms a source's node exponents at 40 digits.  Yardsticks
(section 3.13's convention: 2^-53 x the addends' magnitude x (1 + A), A the largest magnitude among the exponent's addends
over the nodes with p_k >= 2^-53):

  Delta_i:            2^-53 (|Delta_i| + 1 + A)                     (lf_gradproblib's)
  the gradient slots: 2^-53 (sum_k p_k |q_k|) (1 + A)               (lf_gradproblib's)
  e1 = sum p_k d_k:   2^-53 (1 + A) sum_k p_k |d_k|
  e2 = sum p_k d_k^2: 2^-53 (1 + A) sum_k p_k d_k^2
  a node's product p_k exp(-l_k) / (pref0 vol):  its own value x 2^-53 (1 + A_k + |l_k|), A_k the larger of A and of node k's
                      own exponent addends (a node of negligible p_k does not enter A, but its own product carries its own
                      t em_k); l_k enters the exponent whether or not the code under test forms it there.  A sum over a
                      source's nodes: the sum of the nodes' yardsticks.

Inputs: the edge lattice deconv_sources(variant) under deconv_rows(variant) for K = 4 and 32 - every source of the sigma x
flux lattice, a fifth of the seeded fill, the prior's far corner - and per wide class (48, 72, 96, 120 and 144 nodes: 48, 8,
32, 56 and 16 in the last 64-lane pass) sources at sigma just above 0.09, just above the class's lower edge and on its upper
edge, each at fluxes from 1.5 dex below Flim to 2 dex above, a bright-end source and the far corner.  The class tables are
deconv.wide_table's here; the GPU tests take lfh::wide_table's from the probe and assert that the two have the same bits.

The cap of a form is 4 x its NumPy figure and never below 2 (lf_problib.cap_from); CAPS holds the figures measured by
tests/test_convterms_cpu.py::test_numpy_figures_behind_the_caps, which asserts that they still hold."""
import functools

import numpy as np

import lf_gradproblib as P
from lumfuncmcmc_amd import deconv as D

L = P.L
mp, mpf, U53, TINY = P.mp, P.mpf, P.U53, P.TINY
FREE, FIXCOMP, ZEVOL = P.FREE, P.FIXCOMP, P.ZEVOL
VARIANTS = (FREE, FIXCOMP, ZEVOL)
PV = 3.7e5                         # pref0 vol of the binned form: any positive number, not a power of two
WIDE_K = tuple(p * D.WIDE_NPANEL for p in D.WIDE_PANELS)
SQRT2 = float(np.sqrt(2.0))        # 1.41421356237309504880 rounded: the kernels' literal

# max(2, 4 x the NumPy binary64 figure), measured on 2026-10-20; DESIGN.md section 3.27 has the device's figures next to them
CAPS = {"delta_wide": 10.4, "grad_wide": 2.0, "tile_delta": 11.2, "e1_narrow": 5.68, "e2_narrow": 6.21, "e1_wide": 2.0, "e2_wide": 2.0,
        "node_narrow": 53.4, "node_wide": 41.8}


def thin(s, idx):
    idx = np.asarray(idx)
    out = {k: (v[idx] if k != "n" else len(idx)) for k, v in s.items()}
    return out


@functools.lru_cache(None)
def lattice(variant):
    """deconv_sources(variant) thinned: the 100 sources of the sigma x flux lattice, every fifth of the 99 seeded ones, the corner"""
    s = P.deconv_sources(variant)
    return thin(s, np.concatenate([np.arange(100), np.arange(100, 199, 5), [199]]))


def wide_sigmas(cls):
    lo = np.nextafter(D.SIGMA_MAX, 1.0)
    own = lo if cls == 0 else np.nextafter(D.WIDE_EDGES[cls - 1], 1.0)
    return sorted({float(lo), float(own), float(D.WIDE_EDGES[cls])})


@functools.lru_cache(None)
def wide_sources(variant, cls):
    rng = np.random.default_rng(230 + 10 * variant + cls)
    sg = wide_sigmas(cls)
    ys = (-1.5, -0.6, 0.0, 0.7, 2.0)
    yt = np.concatenate([np.repeat(ys, len(sg)), [0.5, 2.0]])
    n = len(yt)
    sig = np.concatenate([np.tile(sg, len(ys)), [sg[-1], sg[-1]]])
    lum = np.concatenate([42.5 + rng.uniform(-1.0, 0.8, n - 2), [44.6, 45.4]])
    logf = (np.log10(P.FLIM0) + yt) - 17.0
    z = rng.uniform(1.16, 1.90, n)
    return {"lum": L.f64(lum), "z": L.f64(z), "logf": L.f64(logf), "P": P.pow10(lum - 42.0), "U": P.pow10(logf + 17.0),
            "sigma": L.f64(sig), "n": n}


def table(key):
    """(x, lnw) of K = 4 or 32 (Gauss-Hermite) or of ("wide", class)"""
    return D.wide_table(key[1]) if isinstance(key, tuple) else D.gauss_hermite(key)


def sources(variant, key):
    return wide_sources(variant, key[1]) if isinstance(key, tuple) else lattice(variant)


def l0_mp(variant, th, s, i):
    """l at the catalogued flux of source i under row th"""
    _, _, _, flim, aC = P._row_parts(variant, False, th)
    if variant != FREE:
        flim, aC = P.FLIM0, P.ALPHA0
    flim, aC, kap = mpf(flim), mpf(aC), mpf(P.KAPPA)
    y0 = mpf(s["logf"][i]) + 17 - mp.log10(flim)
    v0 = mpf(s["U"][i]) * mp.exp(P.MLN10 * kap / aC) / flim
    return P.comp_mp(aC, y0, v0, kap)[0]


def item_mp(variant, th, s, i, x, lnw):
    """deconv_item_mp's tuple for source i (sigma > 0) and the four more: e1, e2 with their yardsticks, the per-node products
    p_k exp(-l_k) / PV with theirs"""
    Dl, yD, slots, ys, p, a, f = P.deconv_item_mp(variant, th, s, i, x, lnw, full=True)
    u, A = mp.mpf(U53), f["A"]
    dl = f["dl"]
    e1 = sum(pk * d for pk, d in zip(p, dl))
    e2 = sum(pk * d * d for pk, d in zip(p, dl))
    y1 = float(u * (1 + A) * sum(pk * abs(d) for pk, d in zip(p, dl)))
    y2 = float(u * (1 + A) * e2)
    prod = [pk * mp.exp(-lk) / mpf(PV) if pk > 0 else mp.mpf(0) for pk, lk in zip(p, f["l"])]
    yp = [float(u * v * (1 + max(A, ak) + abs(lk))) for v, lk, ak in zip(prod, f["l"], f["adds"])]
    return {"delta": Dl, "ydelta": yD, "slots": slots, "yslots": ys, "e1": e1, "y1": y1, "e2": e2, "y2": y2, "prod": prod, "yprod": yp,
            "p": p, "a": a}


def twin(variant, th, s, x, lnw):
    """the NumPy twins on these sources under one row: Delta_i, the gradient slots, (e1, e2), the per-node products / PV [K][n]"""
    inp = P.deconv_inp(variant, s)
    with np.errstate(all="ignore"):
        dl = D._row_terms(inp, s["sigma"], th, x, lnw)
        g = P.deconv_slots_from_twin(variant, th, D._row_grad_terms(inp, s["sigma"], th, x, lnw)[1])
        e1, e2, _ = D._row_terms(inp, s["sigma"], th, x, lnw, moments=True)
        r = D._row_terms(inp, s["sigma"], th, x, lnw, nodes="product")[3] / PV
    return dl, g, e1, e2, r


@functools.lru_cache(None)
def case(variant, key):
    """Cases "delta" [R][n], "grad" [R][n][4], "e1", "e2" [R][n], "prod" [R][n][K] for sources(variant, key) under the rows of
    deconv_rows(variant) against table(key).  A source with sigma = 0: Delta_i, e1 and e2 exactly 0 and one node, the first, of
    product exp(-l(f_i)) / PV.  `rises` [n] under row 0 as lf_gradproblib.case_deconv has them."""
    s, rows = sources(variant, key), P.deconv_rows(variant)
    x, lnw = table(key)
    K, n, R = len(x), s["n"], len(P.deconv_rows(variant))
    names = ("delta", "grad", "e1", "e2", "prod")
    ref = {k: [] for k in names}
    yard = {"delta": np.full((R, n), TINY), "grad": np.full((R, n, P.D_SLOTS), TINY), "e1": np.full((R, n), TINY),
            "e2": np.full((R, n), TINY), "prod": np.full((R, n, K), TINY)}
    npv = {k: np.zeros(v.shape) for k, v in yard.items()}
    rises, lmin = np.zeros(n, dtype=int), np.zeros(n)
    for b, th in enumerate(rows):
        for i in range(n):
            if s["sigma"][i] == 0.0:
                for k in ("delta", "e1", "e2"):
                    ref[k].append(mp.mpf(0))
                ref["grad"] += [mp.mpf(0)] * P.D_SLOTS
                l0 = l0_mp(variant, th, s, i)
                v = mp.exp(-l0) / mpf(PV)
                ref["prod"] += [v] + [mp.mpf(0)] * (K - 1)
                yard["prod"][b, i, 0] = float(mp.mpf(U53) * v * (1 + abs(l0)))
                continue
            it = item_mp(variant, th, s, i, x, lnw)
            ref["delta"].append(it["delta"]), ref["e1"].append(it["e1"]), ref["e2"].append(it["e2"])
            ref["grad"] += it["slots"]
            ref["prod"] += it["prod"]
            yard["delta"][b, i], yard["e1"][b, i], yard["e2"][b, i] = it["ydelta"], it["y1"], it["y2"]
            yard["grad"][b, i] = np.maximum(it["yslots"], TINY)
            yard["prod"][b, i] = np.maximum(it["yprod"], TINY)
            if b == 0:
                af = np.array([float(v) for v in it["a"]])
                rises[i] = 1 + int(np.sum(af[1:] > np.maximum.accumulate(af)[:-1]))
        npv["delta"][b], npv["grad"][b], npv["e1"][b], npv["e2"][b], r = twin(variant, th, s, x, lnw)
        npv["prod"][b] = r.T
    base = {"rows": rows, "src": s, "nodes": L.f64(np.concatenate([x, lnw])), "K": K, "variant": variant, "rises": rises, "key": key}
    return {k: P._case(ref[k], yard[k].ravel(), npv[k].ravel(), **base) for k in names}


def node_edges(s, x):
    """[n][K + 1] edges, source by source at the midpoints between its own node luminosities lum + (sqrt(2) sigma) x_k (rounded
    as vefft_node rounds: one product, one sum), so that bin k holds node k alone; a source with sigma = 0: its one node in
    bin 0.  Asserted here: strictly ascending, and searchsorted puts every node into its own bin."""
    K = len(x)
    ed = np.empty((s["n"], K + 1))
    for i in range(s["n"]):
        s2 = SQRT2 * s["sigma"][i]
        Lk = s["lum"][i] + s2 * np.asarray(x)
        if s["sigma"][i] == 0.0:
            ed[i] = s["lum"][i] + (np.arange(K + 1) - 0.5) * 1.0e-3
            assert np.searchsorted(ed[i], s["lum"][i], side="right") - 1 == 0
            continue
        h = Lk[1] - Lk[0]
        ed[i] = np.concatenate([[Lk[0] - h], 0.5 * (Lk[:-1] + Lk[1:]), [Lk[-1] + h]])
        assert np.array_equal(np.searchsorted(ed[i], Lk, side="right") - 1, np.arange(K)), i
    assert np.all(np.diff(ed, axis=1) > 0.0)
    return ed


def with_dead_node(x, lnw, pos):
    """the table with one more node of weight 0 (ln w = -inf) before node pos, its x between its neighbours'"""
    K = len(x)
    xn = x[0] - 0.25 if pos == 0 else (x[-1] + 0.25 if pos == K else 0.5 * (x[pos - 1] + x[pos]))
    return np.insert(x, pos, xn), np.insert(lnw, pos, -np.inf)


def twice(x, lnw):
    """each node twice: every second node ties the running maximum (d == 0); Delta_i grows by ln 2, p_k halves"""
    return np.repeat(x, 2), np.repeat(lnw, 2)


@functools.lru_cache(None)
def chunk_sources(variant, n, wide):
    """n sources of ONE luminosity and sigma - so of the same node luminosities: against node_edges of the first every bin
    holds one node of every source - with fluxes over the lattice's range and their own redshifts; narrow: every seventh has
    sigma = 0"""
    rng = np.random.default_rng(240 + n)
    yt = np.tile(np.linspace(-1.5, 2.0, 20), n // 20 + 1)[:n]
    logf = (np.log10(P.FLIM0) + yt) - 17.0
    lum = np.full(n, 42.6)
    sg = np.full(n, 0.2 if wide else 0.05)
    if not wide:
        sg[3::7] = 0.0
    return {"lum": L.f64(lum), "z": L.f64(rng.uniform(1.16, 1.90, n)), "logf": L.f64(logf), "P": P.pow10(lum - 42.0),
            "U": P.pow10(logf + 17.0), "sigma": L.f64(sg), "n": n}


def chunk_sum(one, n):
    """lf_vefftrue_part's documented order on the one-source partials one[n][...]: wave w takes sources 64 w .. 64 w + 63, then
    64 (w + 4) .., each in source order (the lower half-wave's before the upper's) into its own histogram from 0; the block
    stores ((w0 + w1) + w2) + w3"""
    hist = [np.zeros(one.shape[1:]) for _ in range(4)]
    for w in range(4):
        for base in range(64 * w, n, 256):
            for j in range(base, min(base + 64, n)):
                hist[w] = hist[w] + one[j]
    return ((hist[0] + hist[1]) + hist[2]) + hist[3]


# ---------------------------------------------------------------------------------------------- the loop restated, for mutations
def loop_numpy(variant, th, s, x, lnw, mutate=None):
    """deconv._row_terms's loop restated for ONE use: tests/test_convterms_cpu.py asserts that it gives the twin's bits with
    mutate = None, then applies one mutation and asserts that the metric sees it.  Returns (Delta_i [n], e1, e2, products / PV
    [K][n]).  mutate: "e1_no_rescale" (e1's numerator not rescaled when the maximum rises), "e2_delta" (e2 formed with delta),
    "fc_catalogued" (a node's completeness taken at the catalogued flux), "first64" (the softmax normalised over the first 64
    nodes only), "tile_l0" (l(f_i) taken at v = U, without 10^(kappa / alpha_C) / Flim: the tile form with a wrong l0)."""
    Ls, _, al, flim, aC = P._row_parts(variant, False, th)
    if variant != FREE:
        flim, aC = P.FLIM0, P.ALPHA0
    lum, sigma = s["lum"], s["sigma"]
    n, K = len(lum), len(x)
    LN10 = P.LN10
    c1l = LN10 * (al + 1.0)
    with np.errstate(all="ignore"):
        if variant == ZEVOL:
            ls = P.G._basis(s["z"], P.PIVOT_SETS[0])
            t = np.exp(LN10 * (lum - ls.T @ np.asarray(Ls, dtype=float)))
        else:
            t = 10.0 ** (lum - 42.0) * np.exp(LN10 * (42.0 - Ls))
        U = 10.0 ** (s["logf"] + 17.0)
        Fl = np.full(n, float(flim))
        y0 = (s["logf"] + 17.0) - np.log10(Fl)
        v0 = U * (np.exp(LN10 * P.KAPPA / aC) / Fl)
        l0 = D._lcomp(y0, U if mutate == "tile_l0" else v0, aC)
        s2 = np.sqrt(2.0) * sigma
        m, acc = np.full(n, -np.inf), np.zeros(n)
        num = np.zeros((2, n))
        ak, bk = np.empty((K, n)), np.empty((K, n))
        for k in range(K):
            dl = s2 * x[k]
            em = np.expm1(LN10 * dl)
            lc = D._lcomp(y0 + dl, v0 * (em + 1.0), aC)
            sch = c1l * dl - t * em
            a = lnw[k] + (sch + (lc - l0))
            ak[k] = a
            bk[k] = a - l0 if mutate == "fc_catalogued" else lnw[k] + (sch - l0)
            if mutate == "first64" and k >= 64:
                continue
            skip = a == -np.inf
            d = a - m
            e = np.exp(-np.abs(d))
            up = d > 0.0
            acc_n = np.where(up, acc * e + 1.0, acc + e)
            for j, q in enumerate((dl, dl if mutate == "e2_delta" else dl * dl)):
                risen = num[j] + q if (mutate == "e1_no_rescale" and j == 0) else num[j] * e + q
                num[j] = np.where(skip, num[j], np.where(up, risen, num[j] + e * q))
            acc = np.where(skip, acc, acc_n)
            m = np.where(skip, m, np.where(up, a, m))
        on = sigma > 0.0
        Dl = np.where(on, m + np.log(acc), 0.0)
        e1, e2 = (np.where(on, num[j] / acc, 0.0) for j in range(2))
        r = np.where((ak == -np.inf) | ~(acc > 0.0), 0.0, np.exp(bk - m) / acc)
        r = np.where(on, r, 0.0)
        r[0] = np.where(on, r[0], np.exp(-l0))
    return Dl, e1, e2, r / PV
