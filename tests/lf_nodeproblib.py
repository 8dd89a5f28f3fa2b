"""Inputs, 40-digit references, yardsticks and NumPy twins for the element-wise probes of piece B's grid-node forms
(csrc/lf_kernels.h: field_sum<NF>, field_sum_bright<NF>, walker_vmin, the Schechter node factor of FREE and FIXCOMP, the
column and the row form of the z-evolving node in gridsum_body, quad_coef, quad_nofma, quad_comp, quad_range).  No GPU here:
tests/test_nodeterms_cpu.py checks that every generator yields what it promises and measures the NumPy binary64 figures,
tests/test_gpu_nodeterms.py runs the same cases through tests/node_probe.hip.  Conventions: tests/lf_problib.py (a case is
a dict of input arrays, `ref` a (hi, lo) pair from 40 digits, `yard`, `np`; the cap is 4 x the NumPy figure, never below 2).

Inputs are the walker-record and node values themselves (c0, c1, L*, Q, F_CA, F_V, Omega_0, G, PG, a3, a4), not theta: the
probes test the node arithmetic, and prepare_lane, which makes the records, is out of scope.

Domain of the node sum.  A record follows from (alpha_C, Flim, fcmin) as prepare_lane makes it - lF = log10(1e-17 Flim),
b = -kappa / alpha_C with kappa = sqrt(fc_ratio), V = 1 / (Flim 10^b), cA = -alpha_C lF - and a node from log f: a3 = log f,
a4 = 10^(log f + 17).  So num = alpha_C (log f - lF) and a4 V = (f / Flim) 10^(kappa / alpha_C) are tied:
log10(a4 V) = (num + kappa) / alpha_C.  (alpha_C, Flim) run over the default prior box and the boxes of
test_compress_with_a_non_default_prior_box, fcmin over {0.01, 0.1, 0.45}, log f over [-19, -11.5]: the lattice has
log L in [40, 46] and log10(4 pi D_L^2) between 57.9 and 58.4 over the survey's redshifts.  Over that domain a4 V lies in
[1.1e-3, 1e14] and num in [-30, 59].  The edge lists go beyond it where the code has a branch there (the floor of d, the
clamps): those elements are marked `reach = False` and held to the same cap."""
import functools
import math

import mpmath as mp
import numpy as np

import lf_problib as L
from lf_problib import LN10, LNLN10, U53, cap_from, f64, measure, mpf, pair, ulp_of, ulps_around  # noqa: F401

mp.mp.dps = 40
MAXF = 8
TINY = 2.0 ** -1074
SQARCSEC = 42545170296.152206
# Omega_0 / sqarcsec of the synthetic survey's five fields (synth.OMEGA_0) and three more of the same size
OM0 = np.array([v * 0.85 * 3600 / SQARCSEC for v in (121.9, 122.2, 116.0, 147.3, 118.7, 130.1, 109.4, 125.0)])
BOXES = (((1.0, 7.0), (1.0, 6.0)), ((0.6, 10.0), (0.5, 9.0)), ((3.0, 5.0), (2.0, 4.0)))       # (alpha_C, Flim)
FCMINS = (0.01, 0.1, 0.45)
LOGF_LO, LOGF_HI = -19.0, -11.5
NUM_LO, NUM_HI, X_LO, X_HI = -30.0, 59.0, 1.1e-3, 1.0e14
BRIGHT = 37.5

# Caps K on max err / yard: max(2, 4 x the NumPy binary64 figure on the same inputs), the figures measured by
# tests/test_nodeterms_cpu.py::test_numpy_figures_behind_the_caps (which asserts that they still hold) on 2026-10-20;
# DESIGN.md section 3.25 has the device's figures next to them.
CAPS = {
    "field_sum": 4.66, "field_sum_bright": 4.46, "gridsum_free_sum": 4.91,
    "schechter": 41.8, "znode_cols": 2.5, "znode_rows": 2.5,
    "quad_coef": 57.6, "quad_nofma": 4.38,
    # (quad_comp: the plain evaluation cancels; the GPU test also holds the function to the 2 ulp of its header)
    "quad_comp": 2.09e6,
}


def kappa_of(fcmin):
    a = (2.0 * fcmin - 1.0) ** 2
    return math.sqrt(abs(a / (1.0 - a)))


# ---------------------------------------------------------------------------------------------- the node sum
def record_of(aC, Flim, kappa):
    """(cA, V) of one (walker, field) as prepare_lane forms them (lf_kernels.h), in NumPy"""
    b = -np.sqrt(kappa * kappa / (aC * aC))
    lF = np.log10(1.0e-17 * Flim)
    return -aC * lF, 1.0 / (Flim * 10.0 ** b)


def node_of(logf):
    """(a3, a4) of a node as grid_tables forms them (lf_hostprep.h)"""
    return logf, np.power(10.0, logf + 17.0)


def triples(n, seed):
    """(alpha_C, Flim[n][MAXF], log f, kappa): seeded, box by box and fcmin by fcmin, log f denser near Flim"""
    rng = np.random.default_rng(seed)
    aC, Fl, kap = np.zeros(n), np.zeros((n, MAXF)), np.zeros(n)
    for i in range(n):
        (alo, ahi), (flo, fhi) = BOXES[i % 3]
        aC[i] = rng.uniform(alo, ahi) if i % 5 else (alo, ahi)[(i // 5) % 2]
        Fl[i] = rng.uniform(flo, fhi, MAXF)
        if i % 7 == 0:
            Fl[i, 0], Fl[i, -1] = flo, fhi
        kap[i] = kappa_of(FCMINS[(i // 3) % 3])
    logf = np.where(rng.uniform(0, 1, n) < 0.5, rng.uniform(LOGF_LO, LOGF_HI, n), np.log10(1.0e-17 * Fl[:, 0]) + rng.normal(0, 0.5, n))
    return aC, Fl, np.clip(logf, LOGF_LO, LOGF_HI), kap


def elements_from(aC, Fl, logf, kap):
    cA, V = record_of(aC[:, None], Fl, kap[:, None])
    a3, a4 = node_of(logf)
    return {"aC": f64(aC), "a3": f64(a3), "a4": f64(a4), "cA": f64(cA), "V": f64(V), "kappa": f64(kap),
            "reach": np.ones(len(aC), dtype=bool)}


def _direct(aC, a3, a4, cA, V, kind):
    """elements given by their record and node values; every field gets the same (cA, V)"""
    aC, a3, a4, cA, V = np.broadcast_arrays(f64(aC), f64(a3), f64(a4), f64(cA), f64(V))
    n = len(aC)
    return {"aC": f64(aC), "a3": f64(a3), "a4": f64(a4), "cA": f64(np.repeat(cA[:, None], MAXF, 1)), "V": f64(np.repeat(V[:, None], MAXF, 1)),
            "kappa": np.full(n, np.nan), "reach": np.zeros(n, dtype=bool), "kind": np.array([kind] * n)}


def _cat(parts):
    out = {}
    for k in parts[0]:
        out[k] = np.concatenate([p[k] for p in parts])
    return out


def x_at_exponent(t):
    """a4 V at which ln fc / d = t for num = 0 (ln fc = -ln 2): d = ln2 / |t|"""
    return -np.log1p(-L.LN2 / np.abs(t))


def smallest_num_bright():
    """the walker of the boxes with the smallest num at a given a4 V: num = alpha_C log10(a4 V) - kappa is smallest for the
    smallest alpha_C and the largest kappa (a4 V > 1); Flim does not enter (Flim = 1: lF = -17)"""
    return 0.6, 1.0, kappa_of(0.01)


@functools.lru_cache(None)
def field_edges():
    """The edge lists of the node sum, by kind.  Direct elements take num = fma(aC, a3, cA) with aC = 1, a3 = the wanted num,
    cA = 0, and a4 V = a4 with V = 1, so that the products the function forms are exactly the listed values."""
    P = []
    nums = np.array([0.0, -3.0, 2.0])
    # a4 V at the -750 clamp +-0, 1, 2 ulp
    x = ulps_around(750.0)
    P.append(_direct(1.0, np.repeat(nums, len(x)), np.tile(x, 3), 0.0, 1.0, "clamp_x"))
    # a4 V < 2^-54: e^(-x) rounds to 1, d = 0 before the floor 1e-100 acts; and the first values above (at 2^-54 itself
    # e^(-x) is a hair above the midpoint of 1 - 2^-53 and 1: an exponential good to 1 ulp may give either)
    x = np.array([0.0, 5e-324, 1e-300, 1e-100, 1e-20, 2.0 ** -60, 2.0 ** -55])
    P.append(_direct(1.0, np.repeat(nums, len(x)), np.tile(x, 3), 0.0, 1.0, "floor"))
    x = np.array([2.0 ** -53, np.nextafter(2.0 ** -53, 1.0), 2.0 ** -52, 1e-12, 1e-8, 1e-5])
    P.append(_direct(1.0, np.repeat(nums, len(x)), np.tile(x, 3), 0.0, 1.0, "above_floor"))
    # a4 V in [1e-3, 1]: 1 - e^(-x) cancels one to three digits and exp(ln fc / d) amplifies the loss
    x = 10.0 ** np.linspace(-3.0, 0.0, 61)
    nn = np.array([-2.0, 0.0, 1.5, 8.0])
    P.append(_direct(1.0, np.repeat(nn, len(x)), np.tile(x, 4), 0.0, 1.0, "cancel"))
    # ln fc / d at the -750 clamp, and through the subnormal results down to it
    x750 = x_at_exponent(750.0)
    x = np.concatenate([x_at_exponent(np.linspace(690.0, 760.0, 141)), ulps_around(x750), x750 * (1.0 + np.array([-400.0, 400.0]) * 2.0 ** -52)])
    P.append(_direct(1.0, 0.0, x, 0.0, 1.0, "clamp_t"))
    # a4min vmin at 37.5 +-0, 1, 2 ulp and up to 40 (and down to 30), for the smallest num the boxes allow at that flux
    aC, Fl, kap = smallest_num_bright()
    cA, V = record_of(aC, Fl, kap)
    xw = np.concatenate([ulps_around(BRIGHT), np.linspace(30.0, 40.0, 41)])
    a4 = xw / V
    for k in range(5):                       # the product the kernel forms, a4 * V, is to be the listed value where a double allows
        a4 = np.where(a4 * V < xw, np.nextafter(a4, np.inf), np.where(a4 * V > xw, np.nextafter(a4, 0.0), a4))
    e = _direct(aC, np.log10(a4) - 17.0, a4, cA, V, "bright")
    e["kappa"][:] = kap
    e["reach"][:] = True
    P.append(e)
    # num = 0 of both signs, and the largest |num| of the boxes with the a4 V that goes with it
    P.append(_direct(1.0, [0.0, -0.0, 0.0, -0.0], [0.5, 0.5, 50.0, 50.0], [0.0, -0.0, -0.0, 0.0], 1.0, "zero"))
    for aC, Fl, lf, fc in ((10.0, 0.5, LOGF_HI, 0.01), (10.0, 9.0, LOGF_LO, 0.45), (10.0, 9.0, LOGF_LO, 0.01), (7.0, 1.0, LOGF_HI, 0.1)):
        e = elements_from(np.array([aC]), np.full((1, MAXF), Fl), np.array([lf]), np.array([kappa_of(fc)]))
        e["kind"] = np.array(["num_max"])
        P.append(e)
    return _cat(P)


def field_reference(E, nf, om0):
    """(ref pair, yard, numpy twin) of sum_f Omega_f fc_f^(1 / (1 - e^(-a4 V_f))), fc = (1 + num / sqrt(1 + num^2)) / 2,
    num = aC a3 + cA_f, from the exact binary64 inputs.  Yardstick: the free term's E = 2^-53 (|t| (1 + 1/d) + 1 / (w d)) is
    the error of the exponent t = ln fc / d; the exponential turns it into a relative error of v = e^t, which has a
    rounding of its own (one ulp: the unit of the format where v is subnormal); summed with the weights Omega_f, plus one
    rounding of the running sum per field (2^-53 of the sum, or the format's unit 2^-1074 where the sum is subnormal)."""
    n = len(E["aC"])
    tot, yard = [], np.zeros(n)
    for i in range(n):
        s = mp.mpf(0)
        y = 0.0
        for f in range(nf):
            num = mpf(E["aC"][i]) * mpf(E["a3"][i]) + mpf(E["cA"][i, f])
            x = mpf(E["a4"][i]) * mpf(E["V"][i, f])
            v = mp.mpf(0)
            if x > 0:
                d = -mp.expm1(-x)
                w = _w_mp(num)
                t = mp.log(w / 2) / d
                if t > -800:
                    v = mp.exp(t)
                    vf = float(v)
                    if vf > 0.0:
                        y += om0[f] * (vf * U53 * float(abs(t) * (1 + 1 / d) + 1 / (w * d)) + float(np.spacing(vf)))
            s += mpf(om0[f]) * v
        tot.append(s)
        yard[i] = y
    ref = pair(tot)
    yard = yard + nf * np.maximum(U53 * np.abs(ref[0]), TINY)
    return ref, yard, np_field_sum(E, nf, om0)


def _w_mp(x):
    s = mp.sqrt(1 + x * x)
    return 1 + x / s if x >= 0 else 1 / (s * (s - x))


def np_field_sum(E, nf, om0):
    """the reference's statements (VmaxLumFunc.py:118-127, :141; lumfuncmcmc.py:375) on the record values, in binary64; num is
    the one product-and-sum the function forms (as lf_problib.case_term_free takes it)"""
    s = np.zeros(len(E["aC"]))
    with np.errstate(all="ignore"):
        for f in range(nf):
            num = L.fma_exact(E["aC"], E["a3"], E["cA"][:, f])
            fc = 0.5 * (1.0 + num / np.sqrt(1.0 + num * num))
            d = 1.0 - np.exp(-(E["a4"] * E["V"][:, f]))
            s = s + om0[f] * fc ** (1.0 / d)
    return s


def vmin_of(E, nf):
    return np.min(E["V"][:, :nf], axis=1)


def om0_for(nf, zero_field=None):
    om0 = OM0[:nf].copy()
    if zero_field is not None:
        om0[zero_field] = 0.0
    return om0


@functools.lru_cache(None)
def case_field_sum(nf, zero_field=None, nfill=500):
    """every edge and a seeded fill, for one NF; `gate` marks the elements the kernels hand to field_sum_bright
    (alpha_C > 0 and a4 vmin > 37.5: all nodes of a chunk are at least as bright as its faintest)"""
    E = field_edges()
    n_edges = len(E["aC"])
    F = elements_from(*triples(nfill, 200 + nf))
    F["kind"] = np.array(["fill"] * nfill)
    E = _cat([E, F])
    om0 = om0_for(nf, zero_field)
    ref, yard, npv = field_reference(E, nf, om0)
    gate = (E["aC"] > 0.0) & (E["a4"] * vmin_of(E, nf) > BRIGHT)
    return dict(E, nf=nf, om0=om0, ref=ref, yard=yard, np=npv, gate=gate, n_edges=n_edges)


def sub(case, sel):
    """the case restricted to the elements `sel`"""
    out = dict(case)
    for k in ("aC", "a3", "a4", "cA", "V", "kappa", "reach", "kind", "yard", "np", "gate"):
        if k in case:
            out[k] = case[k][sel]
    out["ref"] = (case["ref"][0][sel], case["ref"][1][sel])
    return out


def tie_residual(E, f=0):
    """log10(a4 V) - (num + kappa) / alpha_C of the reachable elements: 0 up to roundings when num and a4 V go together"""
    r = E["reach"]
    num = E["aC"][r] * E["a3"][r] + E["cA"][r, f]
    return np.log10(E["a4"][r] * E["V"][r, f]) - (num + E["kappa"][r]) / E["aC"][r]


# ---------------------------------------------------------------------------------------------- gridsum_body: layouts
def lane_of(c, nlive=256):
    """the lane of chunk c that carries the weight: 37 is odd, so 256 consecutive chunks visit every lane"""
    return (37 * c + 5) % 256 % nlive


def chunk_nodes(vals, nnodes=None):
    """per-chunk values -> per-node arrays: every lane of chunk c holds vals[c]"""
    nch = len(vals)
    out = np.repeat(f64(vals), 256)
    return out[:nch * 256 if nnodes is None else nnodes]


def one_hot_weights(nch, nnodes=None):
    nnodes = nch * 256 if nnodes is None else nnodes
    W = np.zeros(nnodes)
    for c in range(nch):
        W[c * 256 + lane_of(c, min(256, nnodes - c * 256))] = 1.0
    return W


# (TW, B): tiles of TW walkers and a last one of TW - 1, or of 1
TILINGS = ((16, 31), (16, 17), (4, 7), (4, 5))


# ---------------------------------------------------------------------------------------------- the Schechter node factor
def np_schechter(c0, c1, Ls, Q, G, PG):
    with np.errstate(all="ignore"):
        return np.exp(np.clip((c1 * (G - Ls) + c0) - PG * Q, -750.0, 709.0))


@functools.lru_cache(None)
def case_schechter(B, nch):
    """walkers (c0, c1, L*, Q) x nodes (G, PG): exp(clamp(c1 (G - L*) + c0 - PG Q)), the clamps [-750, 709] of fexp_c being part
    of the function.  Walkers: phistar in [-9, 2], alpha in [-3, 1], L* in [40, 47] (the widest boxes), Q = 10^(42 - L*);
    nodes: G in [40, 46], PG = 10^(G - 42).  Edge walkers c1 = 0, Q in {0, 1}: the argument is c0 - PG Q, and the edge nodes
    carry PG at both clamps and through the subnormal results; c0 = 709 +- 1 ulp needs no node.  The argument reaches -750
    inside the domain (PG Q up to 1e6) and +709 only outside it (it stays below 38)."""
    rng = np.random.default_rng(300 + B)
    c0 = LNLN10 + LN10 * rng.uniform(-9.0, 2.0, B)
    c1 = LN10 * (rng.uniform(-3.0, 1.0, B) + 1.0)
    Ls = rng.uniform(40.0, 47.0, B)
    Q = 10.0 ** (42.0 - Ls)
    ew = [(0.0, 0.0, 42.0, 1.0), (0.0, 0.0, 42.0, 0.0), (709.0, 0.0, 42.0, 0.0), (np.nextafter(709.0, 1e3), 0.0, 42.0, 0.0),
          (np.nextafter(709.0, 0.0), 0.0, 42.0, 0.0), (720.0, 0.0, 42.0, 0.0), (-750.0, 0.0, 42.0, 0.0), (np.nextafter(-750.0, 0.0), 0.0, 42.0, 0.0),
          (1459.0, 0.0, 42.0, 1.0), (5.0, LN10 * 1.5, 40.0, 100.0)][:max(1, B - 4)]
    for k, e in enumerate(ew):
        c0[k], c1[k], Ls[k], Q[k] = e
    G = rng.uniform(40.0, 46.0, nch)
    PG = 10.0 ** (G - 42.0)
    en = np.concatenate([ulps_around(750.0), ulps_around(L.LF_UNDERFLOW), np.linspace(700.0, 760.0, 25), [0.0, 1e-300, 1.0, 1.0e6]])[:nch // 2]
    PG[:len(en)] = en
    with np.errstate(divide="ignore"):
        G[:len(en)] = np.clip(42.0 + np.log10(en), 40.0, 46.0)
    ref, arg = [], np.zeros((B, nch))
    for w in range(B):
        for c in range(nch):
            a = mpf(c1[w]) * (mpf(G[c]) - mpf(Ls[w])) + mpf(c0[w]) - mpf(PG[c]) * mpf(Q[w])
            arg[w, c] = float(a)
            ref.append(mp.exp(min(max(a, mp.mpf(-750)), mp.mpf(709))))
    ref = _round_pair(ref)
    hi = ref[0].reshape(B, nch)
    # 2^-53 |ref| (1 + |argument|); where the result is subnormal the format's own unit
    yard = U53 * hi * (1.0 + np.abs(arg))
    yard = np.where(hi >= 2.0 ** -1022, yard, np.maximum(yard, TINY))
    npv = np_schechter(c0[:, None], c1[:, None], Ls[:, None], Q[:, None], G[None, :], PG[None, :])
    return {"c0": c0, "c1": c1, "Ls": Ls, "Q": Q, "G": G, "PG": PG, "arg": arg, "ref": (hi.ravel(), ref[1]), "yard": yard.ravel(),
            "np": npv.ravel(), "B": B, "nch": nch, "n_edge_walkers": len(ew), "n_edge_nodes": len(en)}


def _round_pair(vals):
    """pair() for results of an exponential: below 2^-1075 the format holds 0"""
    return pair([mp.mpf(0) if v < mp.mpf(2) ** -1075 else v for v in vals])


# ---------------------------------------------------------------------------------------------- the node sum through gridsum_body
@functools.lru_cache(None)
def case_gridsum_free(B, nch, nf):
    """walkers (alpha_C, Flim[nf], fcmin) x nodes (log f), with c0 = c1 = Q = 0 so that the Schechter factor is fexp_c(0) = 1.0
    exactly and the partial is the node sum, in whichever form gridsum_body's own test a4min vmin > 37.5 selects (a4min of
    a chunk of copies is the node's a4).  Walker 0 is the one with the smallest num at a given a4 V, and the first nodes
    put its a4 vmin at 37.5 +-0, 1, 2 ulp and from 30 to 40: a threshold below 37.5 drops a decay factor that is not 1."""
    aC, Fl, logf, kap = triples(max(B, nch), 400 + B + nf)
    aC, Fl, kap = aC[:B].copy(), Fl[:B].copy(), kap[:B].copy()
    aC[0], Fl[0], kap[0] = smallest_num_bright()
    cA, V = record_of(aC[:, None], Fl, kap[:, None])
    vmin0 = np.min(V[0, :nf])
    xw = np.concatenate([ulps_around(BRIGHT), np.linspace(30.0, 40.0, 21)])[:nch // 2]
    a4e = xw / vmin0
    logf = logf[:nch].copy()
    logf[:len(xw)] = np.log10(a4e) - 17.0
    a3, a4 = node_of(logf)
    a4[:len(xw)] = a4e
    W, C = np.meshgrid(np.arange(B), np.arange(nch), indexing="ij")
    W, C = W.ravel(), C.ravel()
    E = {"aC": aC[W], "a3": a3[C], "a4": a4[C], "cA": cA[W], "V": V[W], "kappa": kap[W],
         "reach": np.ones(len(W), dtype=bool)}
    om0 = om0_for(nf)
    ref, yard, npv = field_reference(E, nf, om0)
    gate = (E["aC"] > 0.0) & (E["a4"] * vmin_of(E, nf) > BRIGHT)
    return dict(E, w_aC=aC, w_cA=cA, w_V=V, n_a3=a3, n_a4=a4, nf=nf, om0=om0, ref=ref, yard=yard, np=npv, gate=gate, B=B, nch=nch,
                n_edge_nodes=len(xw))


# ---------------------------------------------------------------------------------------------- the quadratics
PIVOTS = (1.20, 1.53, 1.86)


def np_quad_coef(y1, y2, y3, z1, z2, z3):
    """getQuadCoef, lumfuncmcmc_z.py:40-42, in the reference's operation order (NumPy does not contract)"""
    with np.errstate(all="ignore"):
        z1s, z2s, z3s = z1 * z1, z2 * z2, z3 * z3
        a = ((y3 - y1) + (y2 - y1) * (z1 - z3) / (z2 - z1)) / (z3s - z1s + (z2s - z1s) * (z1 - z3) / (z2 - z1))
        b = (y2 - y1 - a * (z2s - z1s)) / (z2 - z1)
        c = y1 - a * z1s - b * z1
    return a, b, c


def np_quad_nofma(a, b, c, z, z2):
    return (a * z2 + b * z) + c


def np_quad_range(a, b, c, lo, hi):
    """the values the contract names: at lo, at hi, and at the vertex where it lies strictly inside (NaN where not)"""
    v0, v1 = np_quad_nofma(a, b, c, lo, lo * lo), np_quad_nofma(a, b, c, hi, hi * hi)
    with np.errstate(all="ignore"):
        zv = -b / (2.0 * a)
        inside = (a != 0.0) & (zv > lo) & (zv < hi)
        vv = np.where(inside, np_quad_nofma(a, b, c, zv, zv * zv), np.nan)
    return v0, v1, vv, zv, inside


@functools.lru_cache(None)
def pivot_sets():
    """the reference's pivots, the survey's ends, pivots 1e-3 apart, and unequal gaps"""
    return np.array([PIVOTS, (1.16, 1.53, 1.90), (1.529, 1.530, 1.531), (1.20, 1.201, 1.86), (0.5, 2.0, 3.5), (1.20, 1.85, 1.86)])


@functools.lru_cache(None)
def case_quad_coef(n=1500):
    """L* and phi* values across the boxes on every pivot set.  Reference: the quadratic through the three points at 40
    digits.  Yardstick: 2^-53 x the coefficient's Lagrange sum of absolute terms, sum_i |y_i| |m_i| / |prod_(j != i) (z_i -
    z_j)| (m_i = 1, z_j + z_k, z_j z_k for a, b, c), times 1 + max|z| / min|dz|: the squares z_i^2 are rounded at the size
    of z^2 and then subtracted."""
    rng = np.random.default_rng(500)
    P = pivot_sets()
    piv = P[np.arange(n) % len(P)]
    y = np.where((np.arange(n) % 2 == 0)[:, None], rng.uniform(40.0, 47.0, (n, 3)), rng.uniform(-9.0, 2.0, (n, 3)))
    y[:6] = 42.5                                    # a constant: a = b = 0 exactly
    y[6:12] = np.array([41.0, 42.0, 43.0])          # (a straight line on the equidistant sets)
    X = np.column_stack([y, piv])
    refs = [[], [], []]
    yard = np.zeros((n, 3))
    for i in range(n):
        ys, zs = [mpf(v) for v in y[i]], [mpf(v) for v in piv[i]]
        co = [mp.mpf(0)] * 3
        ab = [0.0] * 3
        for k in range(3):
            j, m = (k + 1) % 3, (k + 2) % 3
            den = (zs[k] - zs[j]) * (zs[k] - zs[m])
            for q, mult in enumerate((mp.mpf(1), -(zs[j] + zs[m]), zs[j] * zs[m])):
                co[q] += ys[k] * mult / den
                ab[q] += float(abs(ys[k] * mult / den))
        amp = 1.0 + np.max(np.abs(piv[i])) / np.min(np.abs(np.diff(np.sort(piv[i]))))
        for q in range(3):
            refs[q].append(co[q])
            yard[i, q] = U53 * ab[q] * amp
    ref = [pair(r) for r in refs]
    a, b, c = np_quad_coef(*[X[:, k] for k in range(6)])
    return {"x": f64(X), "ref": ref, "yard": yard, "np": (a, b, c)}


def _quad_inputs(seed, n):
    """(a, b, c) from np_quad_coef of L* and phi* values across the boxes, z over and beyond the pivots' range"""
    k = case_quad_coef()
    a, b, c = (np.resize(v, n) for v in k["np"])
    piv = np.resize(k["x"][:, 3:], (n, 3))
    rng = np.random.default_rng(seed)
    z = rng.uniform(1.0, 2.1, n)
    on = np.arange(n) % 4 == 0                      # z on a pivot
    z[on] = piv[on, (np.arange(n)[on] // 4) % 3]
    return a, b, c, z, piv


@functools.lru_cache(None)
def case_quad_nofma(n=3000):
    a, b, c, z, _ = _quad_inputs(501, n)
    z2 = z * z
    ref = pair([mpf(p) * mpf(s) + mpf(q) * mpf(x) + mpf(r) for p, q, r, x, s in zip(a, b, c, z, z2)])
    yard = U53 * (np.abs(a * z2) + np.abs(b * z) + np.abs(c))
    X = np.column_stack([a, b, c, z, z2, np.zeros(n)])
    return {"x": f64(X), "ref": ref, "yard": yard, "np": np_quad_nofma(a, b, c, z, z2)}


@functools.lru_cache(None)
def case_quad_comp(n=3000):
    a, b, c, z, _ = _quad_inputs(502, n)
    ref = pair([mpf(p) * mpf(x) * mpf(x) + mpf(q) * mpf(x) + mpf(r) for p, q, r, x in zip(a, b, c, z)])
    X = np.column_stack([a, b, c, z, np.zeros(n), np.zeros(n)])
    return {"x": f64(X), "ref": ref, "yard": ulp_of(ref), "np": np_quad_nofma(a, b, c, z, z * z)}


@functools.lru_cache(None)
def case_quad_range(n=2000):
    """(a, b, c, lo, hi): coefficients across the boxes with the survey's redshift ranges; a = 0; the vertex exactly on lo
    or on hi (a = 1/2^k, b = -2 a lo: -b / (2 a) = lo without a rounding) and one ulp inside"""
    a, b, c, z, piv = _quad_inputs(503, n)
    rng = np.random.default_rng(504)
    lo = rng.uniform(1.0, 1.5, n)
    hi = lo + 10.0 ** rng.uniform(-3.0, 0.0, n)
    k = np.arange(n)
    a[k % 10 == 1] = 0.0
    ex = k % 10 == 2
    a[ex] = np.ldexp(1.0, -(k[ex] % 7)) * np.where(k[ex] % 4 < 2, 1.0, -1.0)
    lo[ex], hi[ex] = 1.25, 1.75
    vert = np.select([k % 40 == 2, k % 40 == 12, k % 40 == 22, k % 40 == 32], [1.25, 1.75, np.nextafter(1.25, 2.0), np.nextafter(1.75, 0.0)], 1.5)
    b[ex] = -2.0 * a[ex] * vert[ex]
    X = np.column_stack([a, b, c, lo, hi, np.zeros(n)])
    return {"x": f64(X), "exact_vertex": ex, "vert": vert}


# ---------------------------------------------------------------------------------------------- the z-evolving node
def zgrid(S):
    """the column-major S x S lattice of the z-evolving context: node = k S + j, a3 = z_k, a4 = z_k^2 (lf_hostprep.h)"""
    z = np.linspace(1.16, 1.90, S)
    col = np.arange(S * S) // S
    return z, col


@functools.lru_cache(None)
def case_znode(B, S, cols):
    """walkers (aL .. cP, c1) x chunks of the S x S lattice, one weighted node per chunk: exp(clamp(lnT)), lnT = c1 (G - L*(z)) +
    ln10 phi*(z) + ln ln10 - v with L*(z) = aL z2 + bL z + cL from the binary64 (z, z2) of the node's column.  The column form
    takes v = PG 10^(42 - L*(z)) from the node's PG, the row form v = 10^(G - L*(z)) from its G: each is referred to its own
    inputs.  Yardstick: that of lnT_zevol (lf_problib.case_zevol: the roundings of the two quadratics at the size of their
    terms, amplified by c1 and by v) as a relative error of the result, plus the result's own ulp.
    S = 257: 259 chunks, each over one column boundary, the last of one node; S = 129: chunks over two boundaries."""
    rng = np.random.default_rng(600 + B + S)
    nn = S * S
    nch = (nn + 255) // 256
    z, col = zgrid(S)
    y = rng.uniform(41.0, 44.0, (B, 3))
    p = rng.uniform(-5.0, -1.0, (B, 3))
    aL, bL, cL = np_quad_coef(y[:, 0], y[:, 1], y[:, 2], *PIVOTS)
    aP, bP, cP = np_quad_coef(p[:, 0], p[:, 1], p[:, 2], *PIVOTS)
    c1 = LN10 * (rng.uniform(-3.0, 1.0, B) + 1.0)
    Gc = rng.uniform(40.0, 45.0, nch)
    G = chunk_nodes(Gc, nn)
    PG = 10.0 ** (G - 42.0)
    Wt = one_hot_weights(nch, nn)
    live = np.where(Wt == 1.0)[0]
    assert len(live) == nch
    zc = z[col[live]]
    z2c = zc * zc
    refs, yard, npv = [], np.zeros((B, nch)), np.zeros((B, nch))
    for w in range(B):
        for c in range(nch):
            Ls = mpf(aL[w]) * mpf(z2c[c]) + mpf(bL[w]) * mpf(zc[c]) + mpf(cL[w])
            Ph = mpf(aP[w]) * mpf(z2c[c]) + mpf(bP[w]) * mpf(zc[c]) + mpf(cP[w])
            t = mpf(Gc[c]) - Ls
            v = mpf(PG[live[c]]) * mp.exp(mp.mpf(LN10) * (42 - Ls)) if cols else mp.exp(mp.mpf(LN10) * t)
            lnT = mpf(c1[w]) * t + (mp.mpf(LN10) * Ph + mp.mpf(LNLN10)) - v
            r = mp.exp(min(max(lnT, mp.mpf(-750)), mp.mpf(709)))
            refs.append(r)
            Lsd, Phd, td, vd = float(Ls), float(Ph), float(t), float(v)

            def dq(a, b, s):
                return U53 * (abs(a * z2c[c]) + 2.0 * abs(a * z2c[c] + b * zc[c]) + 2.0 * abs(s))
            dt = dq(aL[w], bL[w], Lsd) + U53 * abs(td)
            yv = float(np.spacing(vd)) + vd * (LN10 * dt + U53 * abs(LN10 * td))
            inner = abs(LN10 * Phd) + LNLN10
            yT = abs(c1[w]) * dt + LN10 * dq(aP[w], bP[w], Phd) + U53 * (2.0 * inner + 2.0 * abs(c1[w] * td) + abs(float(lnT))) + yv
            rf = float(r)
            yard[w, c] = max(rf * yT + float(np.spacing(rf)), TINY)
    with np.errstate(all="ignore"):
        Ln = (aL[:, None] * z2c[None, :] + bL[:, None] * zc[None, :]) + cL[:, None]
        Pn = (aP[:, None] * z2c[None, :] + bP[:, None] * zc[None, :]) + cP[:, None]
        tn = Gc[None, :] - Ln
        vn = PG[live][None, :] * np.exp(np.clip(LN10 * (42.0 - Ln), -750.0, 709.0)) if cols else np.exp(np.clip(LN10 * tn, -750.0, 709.0))
        npv = np.exp(np.clip((c1[:, None] * tn + (LN10 * Pn + LNLN10)) - vn, -750.0, 709.0))
    rec = np.column_stack([aL, bL, cL, aP, bP, cP, c1])
    return {"rec": rec, "G": G, "PG": PG, "W": Wt, "a3": z[col], "a4": z[col] * z[col], "S": S, "B": B, "nch": nch, "live": live,
            "col": col[live], "ref": _round_pair(refs), "yard": yard.ravel(), "np": npv.ravel()}
