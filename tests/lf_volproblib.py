"""Inputs, host replay and 40-digit reference for the per-element check of veffd_partial_zmax's volume evaluation
(csrc/lf_veffdraws.h, entry lf_veff_draws_zmax) against voltable.VolumeTable.eval.  No GPU here: tests/test_volterms_cpu.py
holds the table to the 40-digit reference and asserts what the cases cover; tests/test_gpu_volterms.py runs the cases on the
device.  DESIGN.md section 3.30.

What makes a per-element, bit-exact check possible (each derived from the kernel's text and asserted by the tests):
  * one source per bin (nbin = n <= 1024): values[r][i] = 0.0 + (0.0 + w) is the weight of pair (i, r) itself;
  * the host forms c = 1 / sqrt(fmin), so fmin = 4^-j gives c = 2^j exactly and dist = D 2^-j makes the device's D = dist c the
    intended double; for a generic fmin the device's D is the one rounded product dist * (1.0 / sqrt(fmin)) - not the quotient
    dist / sqrt(fmin);
  * fcmin = 0 and flux = Flim of the source's field: log10(1) = 0, fc = 0.5 for any alpha, and the weight is
    2 fl(1 / fl(pref0 V)) - what the host forms from VolumeTable.eval(D);
  * fcmin > 0: lf_veff_draws with the per-source vol = VolumeTable.eval(D) forms the same 1 / (pref0 vol) on the host and the
    same fc on the device (fmin constant per field over the draws of such a call, so that D is per source).

The tables: "standard" (tests/test_gpu_veffzmax.py's catalogue: 2486 evenly spaced node records), "uneven" (its bisection test's
nodes 1 + rng^3: the arithmetic guess of the record is off by many), "three" (dV/dz on {1, 1.5, 2}: two records, no spacing to
guess from) and "one" (dV/dz on {1, 2}: a single record; the clamps and a sweep).

The reference (Ref40) restates the definitions in mpmath at 40 digits and shares no code with cosmology.py, veff.py or
voltable.py: E(z) from the cosmology's density parameters taken as exact doubles, the comoving integral by mp.quad, the closed
branch of the transverse distance, DL = (1 + z) D_M, DL^-1 by mp.findroot (Newton, started at the table's z pieces), and V =
the exact integral of the piecewise-linear interpolant of dV/dz, its nodes taken as exact doubles, from zmin to
min(zmax, DL^-1(D))."""
import functools

import mpmath as mp
import numpy as np

from lumfuncmcmc_amd import hostsetup as hs, synth, veff, voltable
from lumfuncmcmc_amd.cosmology import cosmo

PREF0 = sum(synth.OMEGA_0) / hs.SQARCSEC
R = 257                                # rows reach lanes 0, 63, 64, 255 and lane 0 of a second tile
MAXBIN = 1024                          # sources per call: one bin each
TABLES = ("standard", "uneven", "three")
NODE_EDGES_STANDARD = 240              # node edges kept of the standard table's 2487 (the issue asks for at least 150)
N_UNIFORM = 300
N_UNIFORM_STANDARD = 160               # its lattice is one call of at most MAXBIN sources
SMALL = tuple(10.0 ** -e for e in range(15, 1, -1))      # d_lo (1 + 1e-15 .. 1e-2): the small-volume side
NREF = 120                             # 40-digit points per table, at most
Q = (0.0, 16.0, 50.0, 84.0, 100.0)


# ---------------------------------------------------------------------------------------------- the tables
@functools.lru_cache(None)
def table(name):
    """(VolumeTable, dVdzf, zmin, zmax), built and validated as the package does"""
    if name == "standard":
        cat = synth.catalogue(3000, seed=11)
        dVdzf = hs.distance_tables(cat["z"], cosmo)["dVdzf"]
        zmin, zmax = float(cat["z"].min()), float(cat["z"].max())
    else:
        zmin, zmax = 1.2, 1.85
        if name == "uneven":
            x = np.unique(np.concatenate([[1.0, 2.0], 1.0 + np.random.default_rng(31).random(900) ** 3]))
        else:
            x = np.array({"three": [1.0, 1.5, 2.0], "one": [1.0, 2.0]}[name])
        dVdzf = hs.LinearInterp(x, np.asarray(cosmo.differential_comoving_volume(x)))
    tab = voltable.require(voltable.build(cosmo, dVdzf, zmin, zmax))
    for a in (tab.head, tab.zc, tab.rec):
        a.setflags(write=False)
    return tab, dVdzf, zmin, zmax


def _with_neighbours(d):
    d = np.asarray(d, dtype=np.float64)
    return np.concatenate([d, np.nextafter(d, -np.inf), np.nextafter(d, np.inf)])


@functools.lru_cache(None)
def parts(name):
    """The lattice of one table by kind, {kind: D}: `zb` the 31 boundaries of the z pieces with both neighbouring doubles,
    `node` the node images D_k (all of them; of the standard table NODE_EDGES_STANDARD spread over the records, the first and
    the last included) with both neighbours - D_0 = d_lo and D_K = d_hi among them, and with d_hi's lower neighbour the largest
    D of the table, where u rounds to 32 or just below -, `outer` 0.5 d_lo and 2 d_hi, `small` d_lo (1 + 1e-15 .. 1e-2), and
    `uniform` N_UNIFORM values uniform in the table (N_UNIFORM_STANDARD in the standard one)."""
    tab = table(name)[0]
    zb = tab.d_lo + np.arange(1, voltable.NPIECE) / tab.head[3]                 # VolumeTable.edges()' own expression
    nodes = np.concatenate([tab.rec[:, 0], [tab.d_hi]])
    if name == "standard":
        nodes = nodes[np.unique(np.round(np.linspace(0, len(nodes) - 1, NODE_EDGES_STANDARD)).astype(np.int64))]
    rng = np.random.default_rng(300 + len(tab.rec))
    nuni = N_UNIFORM_STANDARD if name == "standard" else N_UNIFORM
    out = {"zb": _with_neighbours(zb), "node": _with_neighbours(nodes), "outer": np.array([0.5 * tab.d_lo, 2.0 * tab.d_hi]),
           "small": tab.d_lo * (1.0 + np.array(SMALL)), "uniform": rng.uniform(tab.d_lo, tab.d_hi, nuni)}
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(None)
def lattice(name):
    """every D of parts(name), sorted, each once"""
    d = np.unique(np.concatenate(list(parts(name).values())))
    d.setflags(write=False)
    return d


def chunks(name):
    """the lattice in calls of at most MAXBIN sources; every call gets an interleaved share of the sorted lattice, so that each
    spans the whole table"""
    d = lattice(name)
    ncall = -(-len(d) // MAXBIN)
    return [d[c::ncall] for c in range(ncall)]


# ---------------------------------------------------------------------------------------------- the kernel's search, replayed
def search_path(tab, D):
    """veffd_partial_zmax's evaluation of V(D), statement by statement, on the host.  Per element: `outer` -1 at the lower
    clamp (D <= d_lo, NaN), +1 at the upper (D >= d_hi), 0 between them; for the elements between them `piece` (the z piece),
    `path` 0 where the record guessed from z holds D, 1 where its neighbour does, 2 where the records were bisected, `steps`
    of the bisection, `k` the record, `inner` -1 / +1 where the raw quadratic lay below c0_k / above c0_k+1 so that a clamp
    acted (0: it did not); -1 in `piece`, `path`, `k` outside the table.  `V`: the volume."""
    D = np.asarray(D, dtype=np.float64).ravel()
    head, zc, rec = tab.head, tab.zc, tab.rec
    K = len(rec)
    n = D.size
    outer = np.where(D >= head[1], 1, np.where(D > head[0], 0, -1))
    out = {"outer": outer, "V": np.where(outer == 1, head[2], 0.0)}
    for key in ("piece", "path", "k"):
        out[key] = np.full(n, -1, dtype=np.int64)
    out["inner"] = np.zeros(n, dtype=np.int64)
    out["steps"] = np.zeros(n, dtype=np.int64)
    m = outer == 0
    if not m.any():
        return out
    d = D[m]
    u = (d - head[0]) * head[3]
    p = np.minimum(u.astype(np.int64), voltable.NPIECE - 1)
    t = u - p
    q = zc[p]
    z = q[:, voltable.DEG]
    for j in range(voltable.DEG - 1, -1, -1):
        z = z * t + q[:, j]
    g = np.floor((z - head[4]) * head[5]) + 1.0
    k0 = np.minimum(np.maximum(g, 0.0), K - 1.0).astype(np.int64)
    miss0 = (d < rec[k0, 0]) | (d >= rec[k0, 1])
    k1 = np.where(d < rec[k0, 0], np.maximum(k0 - 1, 0), np.minimum(k0 + 1, K - 1))
    miss1 = (d < rec[k1, 0]) | (d >= rec[k1, 1])
    lo, hi = np.zeros(d.size, dtype=np.int64), np.full(d.size, K - 1, dtype=np.int64)     # the last k with D_k <= D
    steps = np.zeros(d.size, dtype=np.int64)
    while True:
        act = lo < hi
        if not act.any():
            break
        mid = lo + (hi - lo + 1) // 2
        le = rec[mid, 0] <= d
        lo = np.where(act & le, mid, lo)
        hi = np.where(act & ~le, mid - 1, hi)
        steps += act
    k = np.where(~miss0, k0, np.where(~miss1, k1, lo))
    rk = rec[k]
    dz = z - rk[:, 2]
    raw = rk[:, 3] + (rk[:, 5] + rk[:, 6] * dz) * dz
    out["piece"][m] = p
    out["path"][m] = np.where(~miss0, 0, np.where(~miss1, 1, 2))
    out["steps"][m] = np.where(miss0 & miss1, steps, 0)
    out["k"][m] = k
    out["inner"][m] = np.where(raw < rk[:, 3], -1, np.where(raw > rk[:, 4], 1, 0))
    out["V"][m] = np.minimum(np.maximum(raw, rk[:, 3]), rk[:, 4])
    return out


def counts(tab, D):
    """what a case covers, for the printed line and the coverage assertions: elements on each search path, at each outer
    clamp, where an inner clamp acted, with 0 < V < 1e-9 V_total and 0 < V < 2 % of V_total, and the z pieces hit"""
    s = search_path(tab, D)
    V, vt = s["V"], tab.v_total
    return {"n": int(s["outer"].size), "in_table": int((s["outer"] == 0).sum()), "guess": int((s["path"] == 0).sum()),
            "neighbour": int((s["path"] == 1).sum()), "bisect": int((s["path"] == 2).sum()), "lower": int((s["outer"] == -1).sum()),
            "upper": int((s["outer"] == 1).sum()), "inner_lo": int((s["inner"] == -1).sum()), "inner_hi": int((s["inner"] == 1).sum()),
            "tiny": int(((V > 0) & (V < 1e-9 * vt)).sum()), "below_2pc": int(((V > 0) & (V < 0.02 * vt)).sum()),
            "pieces": int(len(set(s["piece"][s["outer"] == 0]))), "max_steps": int(s["steps"].max())}


def counts_line(what, c):
    return ("%s: %d elements, %d in the table - guess %d, neighbour %d, bisection %d (at most %d steps); lower clamp %d, upper %d; "
            "inner clamp acted below %d, above %d; 0 < V < 1e-9 V_total %d, 0 < V < 2 %% %d; %d z pieces" %
            (what, c["n"], c["in_table"], c["guess"], c["neighbour"], c["bisect"], c["max_steps"], c["lower"], c["upper"], c["inner_lo"],
             c["inner_hi"], c["tiny"], c["below_2pc"], c["pieces"]))


def weight(tab, D):
    """the weight of a pair at fc = 0.5 from VolumeTable.eval: 2 fl(1 / fl(pref0 V)), +0 without a volume"""
    D = np.asarray(D, dtype=np.float64)
    V = tab.eval(D.ravel()).reshape(D.shape)
    w = np.zeros(D.shape)
    w[V > 0] = 2.0 * (1.0 / (PREF0 * V[V > 0]))
    return w


def device_D(dist, fmin, field):
    """the device's D of every (draw, source): dist times the host's c = 1 / sqrt(fmin), one rounded product; fmin = 0 gives
    c = +inf, and a dist of 0 under it NaN"""
    with np.errstate(divide="ignore", invalid="ignore"):
        c = 1.0 / np.sqrt(np.asarray(fmin, dtype=np.float64))
        return np.asarray(dist, dtype=np.float64)[None, :] * c[:, np.asarray(field, dtype=np.int64)]


# ---------------------------------------------------------------------------------------------- the cases
def _fields(n, nf, rng):
    """half of the sources in the last field, the others over all of them"""
    field = rng.integers(0, nf, n)
    field[rng.random(n) < 0.5] = nf - 1
    return field


def _flims(nf):
    return np.geomspace(2.0e-17, 4.0e-17, nf) if nf > 1 else np.array([3.0e-17])


def _alphas(rng):
    """both signs, |alpha| in 3 .. 6"""
    return rng.uniform(3.0, 6.0, R) * np.where(rng.random(R) < 0.5, -1.0, 1.0)


def exact_case(name, nf, call=0):
    """fcmin = 0, flux = Flim, c = 2^j exactly.  j(r, f) = f % 3 + b(r, f) with random bits b, so that neighbouring lanes and
    fields hold different c; source i carries dist = D_i 2^-(f_i % 3 + b_i) with a bit b_i of its own and is on its lattice
    value D_i on the rows with b(r, f_i) = b_i - on the others D is 2 D_i (above the table: d_hi < 2 d_lo is asserted) or
    D_i / 2 (below it).  Flim is the same in every draw; alpha varies in size and sign."""
    tab = table(name)[0]
    Dl = chunks(name)[call]
    assert tab.d_hi < 2.0 * tab.d_lo
    n = len(Dl)
    rng = np.random.default_rng(1000 * nf + 10 * len(tab.rec) + call)
    field = _fields(n, nf, rng)
    b = rng.integers(0, 2, (R, nf))
    bi = rng.integers(0, 2, n)
    j = (np.arange(nf) % 3)[None, :] + b
    dist = Dl * 2.0 ** -(field % 3 + bi)
    fmin = 4.0 ** -j.astype(np.float64)
    flim = _flims(nf)
    draws = np.ascontiguousarray(np.column_stack([np.tile(flim, (R, 1)), _alphas(rng)]))
    D = device_D(dist, fmin, field)
    on = b[:, field] == bi[None, :]
    assert np.array_equal(D[on], np.broadcast_to(Dl, D.shape)[on])                   # the intended doubles, exactly
    assert np.all((D[~on] >= tab.d_hi) | (D[~on] <= tab.d_lo))
    return {"flux": flim[field], "field": field, "dist": dist, "fmin": fmin, "draws": draws, "D": D, "on": on, "lattice": Dl}


def generic_case(name, nf):
    """fcmin = 0, flux = Flim, fmin in [2.7e-17, 3.3e-17] per (draw, field) and generic luminosities: the draws move a source's
    D by 5 % either way, so the targets (D at 3e-17) are laid around d_lo (0.93 .. 1.1 d_lo: the pairs that graze the lower
    clamp), through the table, around d_hi, and a few far outside"""
    tab = table(name)[0]
    n = MAXBIN
    rng = np.random.default_rng(2000 * nf + len(tab.rec))
    field = _fields(n, nf, rng)
    kind = rng.random(n)
    target = np.where(kind < 0.35, rng.uniform(0.93 * tab.d_lo, 1.1 * tab.d_lo, n),
                      np.where(kind < 0.85, rng.uniform(tab.d_lo, tab.d_hi, n), rng.uniform(0.93 * tab.d_hi, 1.1 * tab.d_hi, n)))
    target[:4] = [0.5 * tab.d_lo, 2.0 * tab.d_hi, 0.94 * tab.d_lo, 1.07 * tab.d_hi]
    lum = np.log10(4.0 * np.pi * (target * veff.MPC_CM_EXACT) ** 2 * 3.0e-17)
    dist = veff.source_distance_scale(lum)
    fmin = rng.uniform(2.7e-17, 3.3e-17, (R, nf))
    flim = _flims(nf)
    draws = np.ascontiguousarray(np.column_stack([np.tile(flim, (R, 1)), _alphas(rng)]))
    return {"flux": flim[field], "field": field, "dist": dist, "fmin": fmin, "draws": draws, "D": device_D(dist, fmin, field)}


def fcmin_case(name, nf, call=0):
    """fcmin = 0.1: fmin = 4^-(f % 3) constant per field over the draws, so that D = dist 2^(f % 3) is the lattice value of
    the source in every row; Flim and alpha vary per draw, the flux is generic"""
    tab = table(name)[0]
    Dl = chunks(name)[call]
    n = len(Dl)
    rng = np.random.default_rng(3000 * nf + 10 * len(tab.rec) + call)
    field = _fields(n, nf, rng)
    dist = Dl * 2.0 ** -(field % 3)
    fmin = np.tile(4.0 ** -(np.arange(nf) % 3).astype(np.float64), (R, 1))
    draws = np.ascontiguousarray(np.column_stack([rng.uniform(2.0e-17, 4.0e-17, (R, nf)), rng.uniform(3.0, 6.0, R)]))
    D = device_D(dist, fmin, field)
    assert np.array_equal(D, np.broadcast_to(Dl, D.shape))
    return {"flux": rng.uniform(2.0e-17, 9.0e-17, n), "field": field, "dist": dist, "fmin": fmin, "draws": draws, "D": D, "lattice": Dl}


ZERO_DIST_SOURCE = 517


def mixed_case(name, nf=5):
    """generic_case with fmin = 0 in a third of the (draw, field) entries - every entry of field 2 among them -, and the
    source ZERO_DIST_SOURCE moved into field 2 (`plain`) and then given dist = 0 (`zero`): 0 inf is NaN under every draw"""
    c = generic_case(name, nf)
    rng = np.random.default_rng(4000 + len(table(name)[0].rec))
    fmin = np.where(rng.random(c["fmin"].shape) < 0.2, 0.0, c["fmin"])
    fmin[:, 2] = 0.0
    field = c["field"].copy()
    field[ZERO_DIST_SOURCE] = 2
    flux = _flims(nf)[field]
    dist0 = c["dist"].copy()
    dist0[ZERO_DIST_SOURCE] = 0.0
    plain = dict(c, flux=flux, field=field, fmin=fmin, D=device_D(c["dist"], fmin, field))
    return {"plain": plain, "zero": dict(plain, dist=dist0, D=device_D(dist0, fmin, field))}


# ---------------------------------------------------------------------------------------------- 40 digits
class Ref40(object):
    """DL, DL^-1 and V at 40 digits for (cosmo, dVdzf, zmin, zmax); every method under mp.workdps(40)"""

    def __init__(self, dVdzf, zmin, zmax, cos=cosmo):
        with mp.workdps(40):
            f = mp.mpf
            self.o_r = f(cos.Ogamma0) + f(cos.Onu0)
            self.o_m, self.o_k, self.o_de, self.dh = f(cos.Om0), f(cos.Ok0), f(cos.Ode0), f(cos.hubble_distance)
            assert self.o_k < 0                                      # the closed branch
            self.s = mp.sqrt(-self.o_k)
            self.zmin, self.zmax = f(zmin), f(zmax)
            self.i_min = mp.quad(self.inv_e, [0, self.zmin])
            self.x = [f(v) for v in dVdzf.x]
            self.y = [f(v) for v in dVdzf.y]
            self.xd = np.asarray(dVdzf.x, dtype=np.float64)
            cum = [f(0)]
            for i in range(1, len(self.x)):
                cum.append(cum[-1] + (self.y[i] + self.y[i - 1]) / 2 * (self.x[i] - self.x[i - 1]))
            self.cum = cum
            self.f_min = self._prim(self.zmin)

    def inv_e(self, z):
        a = 1 + z
        return 1 / mp.sqrt(self.o_r * a ** 4 + self.o_m * a ** 3 + self.o_k * a ** 2 + self.o_de)

    def _chi(self, z):
        """s times the comoving integral: the argument of the sine"""
        return self.s * (self.i_min + mp.quad(self.inv_e, [self.zmin, z]))

    def dl(self, z):
        with mp.workdps(40):
            z = mp.mpf(z)
            return (1 + z) * self.dh / self.s * mp.sin(self._chi(z))

    def dl_inverse(self, D, z0):
        with mp.workdps(40):
            D = mp.mpf(D)

            def f(z):
                return (1 + z) * self.dh / self.s * mp.sin(self._chi(z)) - D

            def df(z):
                chi = self._chi(z)
                return self.dh / self.s * mp.sin(chi) + (1 + z) * self.dh * mp.cos(chi) * self.inv_e(z)

            return mp.findroot(f, mp.mpf(z0), solver="newton", df=df)

    def _prim(self, t):
        """the integral of the interpolant from its first node to t"""
        hi = min(max(int(np.searchsorted(self.xd, float(t))), 1), len(self.x) - 1)
        if self.x[hi - 1] > t:                                       # float(t) rounded across a node
            hi -= 1
        elif hi + 1 < len(self.x) and self.x[hi] < t:
            hi += 1
        lo = hi - 1
        yt = self.y[lo] + (self.y[hi] - self.y[lo]) / (self.x[hi] - self.x[lo]) * (t - self.x[lo])
        return self.cum[lo] + (self.y[lo] + yt) / 2 * (t - self.x[lo])

    def volume_to(self, z):
        with mp.workdps(40):
            z = min(self.zmax, mp.mpf(z))
            return self._prim(z) - self.f_min if z > self.zmin else mp.mpf(0)

    def volume(self, D, z0):
        return self.volume_to(self.dl_inverse(D, z0))


@functools.lru_cache(None)
def ref40(name):
    _, dVdzf, zmin, zmax = table(name)
    return Ref40(dVdzf, zmin, zmax)


@functools.lru_cache(None)
def ref_points(name):
    """at most NREF of the lattice's D: every z-piece boundary, 36 node images across the range, the small-volume points, both
    clamps and their inner neighbours, a value inside every z piece, and uniform values up to NREF"""
    tab, p = table(name)[0], parts(name)
    nz = voltable.NPIECE - 1
    nodes = p["node"][:len(p["node"]) // 3]
    pick = nodes[np.unique(np.round(np.linspace(0, len(nodes) - 1, 36)).astype(np.int64))]
    d = np.unique(np.concatenate([p["zb"][:nz], pick, p["small"], p["outer"], [tab.d_lo, tab.d_hi, np.nextafter(tab.d_lo, np.inf),
                                                                                np.nextafter(tab.d_hi, 0.0)]]))
    uni = p["uniform"]
    L = lattice(name)
    piece = search_path(tab, L)["piece"]
    inside = [L[piece == q][(piece == q).sum() // 2] for q in range(voltable.NPIECE)]   # a value inside every z piece first
    d = np.unique(np.concatenate([d, inside]))
    d = np.unique(np.concatenate([d, uni[~np.isin(uni, d)][:NREF - len(d)]]))
    assert len(d) <= NREF and np.isin(d, lattice(name)).all()
    return d


@functools.lru_cache(None)
def ref_volumes(name):
    """(D, V40 as mpf) on ref_points(name)"""
    tab, ref = table(name)[0], ref40(name)
    d = ref_points(name)
    z0 = tab.redshift(np.clip(d, tab.d_lo, tab.d_hi))
    return d, [ref.volume(float(x), float(z)) for x, z in zip(d, z0)]
