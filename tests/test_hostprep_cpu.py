"""The host's derivation of the tables the kernels read (csrc/lf_hostprep.h), without a GPU.

tests/hostprep_shim.cpp is compiled with the host's g++ and no ROCm include path - that it compiles is the check that the
header is host-only - and called through ctypes with descriptors filled the way capi.LFContext fills them.  Every assertion
follows from a table's definition (a permutation is a permutation, a trapezoid weight integrates, a chunk table covers every
source once), not from the code under test; the bounds are those of the number format: 1 ulp where the same C library
evaluates the same expression, n 2^-52 relative for a sum of n terms accumulated in extended precision."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

from lf_testlib import make_inputs
from lumfuncmcmc_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lumfuncmcmc_amd", "csrc")
EPS = 2.0 ** -52
MAXF = 8
# sources per chunk of every table the host layer makes: st * 256 for the launch geometries of lf_main, st * 512 for lf_free
CHUNK_SIZES = sorted({st * 256 for st in (8, 2, 6, 4)} | {st * 512 for st in (2, 4, 8)})
SIZES = (0, 37, 1000, 5003)          # (none a multiple of a chunk size)
_dp, _ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("hostprep") / "hostprep_shim.so")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-shared", "-fPIC", "-o", so, os.path.join(ROOT, "tests", "hostprep_shim.cpp")],
                   check=True)
    lib = ctypes.CDLL(so)
    lib.hp_const.restype = ctypes.c_double
    lib.hp_get_d.restype = lib.hp_get_i.restype = ctypes.c_int64
    lib.hp_get_d.argtypes = [ctypes.c_int, _dp]
    lib.hp_get_i.argtypes = [ctypes.c_int, _ip]
    lib.hp_chunks.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_double]
    return lib


def slot_d(lib, i):
    a = np.empty(lib.hp_get_d(i, None))
    lib.hp_get_d(i, a.ctypes.data_as(_dp))
    return a


def slot_i(lib, i):
    a = np.empty(lib.hp_get_i(i, None), dtype=np.int32)
    lib.hp_get_i(i, a.ctypes.data_as(_ip))
    return a


def inputs(variant, n, special=None):
    """special: 'empty' (field 2 has no source), 'nan' (FREE: one NaN flux)"""
    inp = make_inputs(variant, n, seed=11 + n)
    if variant == "free":
        inp["logf"] = capi.log_flux(inp["lum"], inp["DLz"])
    if special == "empty":
        fi = np.array(inp["field_ind"]).copy()
        fi[2] = fi[3]
        inp["field_ind"] = fi
    if special == "nan":
        inp["logf"] = inp["logf"].copy()
        inp["logf"][n // 3] = np.nan
    return inp


def desc_of(inp):
    """An lf_desc of the inputs, as capi.LFContext fills it; returns (desc, the arrays it points into)"""
    f64 = lambda a: np.ascontiguousarray(a, dtype=np.float64)      # noqa: E731
    fi = np.ascontiguousarray(inp["field_ind"], dtype=np.int64)
    keep = {"fi": fi, "lum": f64(inp["lum"]), "logL": f64(inp["logL"]), "zarr": f64(inp["zarr"]), "omega0": f64(inp["Omega_0"])}
    d = capi.LfDesc()
    d.variant = capi.VARIANTS[inp["variant"]]
    d.fix_sch_al = 1 if inp.get("fix_sch_al", False) else 0
    d.nf, d.S, d.N = len(fi) - 1, keep["logL"].shape[0], keep["lum"].shape[0]
    if inp["variant"] == "free":
        keep.update(logf=f64(inp["logf"]), volume_part=f64(inp["volume_part"]), dl_zarr=f64(inp["DL_zarr"]))
    else:
        keep.update(om_arr=f64(inp["Om_arr"]), integ_part=f64(inp["integ_part"]))
        if inp["variant"] == "zevol":
            keep["z"] = f64(inp["z"])
        else:
            keep["flim0"] = f64(inp["Flim0"])
            d.alpha0 = float(inp["alpha0"])
    for k in ("logf", "z", "om_arr", "volume_part", "dl_zarr", "integ_part", "flim0", "lum", "omega0", "logL", "zarr"):
        setattr(d, k, capi._ptr(keep.get(k)))
    d.field_ind = fi.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
    d.sch_al0, d.fcmin = float(inp.get("sch_al0", 0.0)), float(inp.get("fcmin", 0.1))
    for i, name in enumerate(capi.LIM_ORDER):
        d.lims[i][0], d.lims[i][1] = float(inp["lims"][name][0]), float(inp["lims"][name][1])
    for i in range(3):
        d.pivots[i] = float(inp["pivots"][i])
    return d, keep


def within_ulp(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    both_nan = np.isnan(got) & np.isnan(want)
    with np.errstate(invalid="ignore"):
        return bool(np.all(both_nan | (got == want) | (np.abs(got - want) <= np.spacing(np.abs(want)))))


def _log(v):
    return math.log(v) if v > 0.0 else (-math.inf if v == 0.0 else math.nan)


CASES = [(v, n, None) for v in ("free", "fixcomp", "zevol") for n in SIZES] + \
        [(v, 1000, "empty") for v in ("free", "fixcomp", "zevol")] + [("free", 1000, "nan")]


@pytest.mark.parametrize("variant,n,special", CASES)
def test_catalogue_tables(shim, variant, n, special):
    inp = inputs(variant, n, special)
    d, keep = desc_of(inp)
    perm = np.empty(n, dtype=np.int64)
    lum, a1, P, U = (np.empty(n) for _ in range(4))
    fields, scal = np.zeros((17, MAXF)), np.zeros(3)
    shim.hp_catalogue(ctypes.byref(d), perm.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), *(capi._ptr(a) for a in (lum, a1, P, U, fields, scal)))
    fi = keep["fi"]
    assert sorted(perm.tolist()) == list(range(n))
    key = {"free": keep.get("logf"), "zevol": keep.get("z")}.get(variant)
    for f in range(d.nf):
        lo, hi = int(fi[f]), int(fi[f + 1])
        assert np.all((perm[lo:hi] >= lo) & (perm[lo:hi] < hi))                 # every source stays in its field
        if key is not None:                                                       # non-decreasing in the key, NaNs last
            k = key[perm[lo:hi]]
            nn = int(np.sum(~np.isnan(k)))
            assert not np.isnan(k[:nn]).any() and np.isnan(k[nn:]).all() and np.all(np.diff(k[:nn]) >= 0)
        assert fields[0, f] == hi - lo
    if key is None:
        assert np.array_equal(perm, np.arange(n))
    pl = keep["lum"][perm]
    np.testing.assert_array_equal(lum, pl)
    if variant == "free":
        lf = keep["logf"][perm]
        want = (lf, [math.pow(10.0, x - 42.0) for x in pl], [math.nan if math.isnan(x) else math.pow(10.0, x + 17.0) for x in lf])
    elif variant == "fixcomp":
        want = ([_log(x) for x in keep["om_arr"][perm]], [math.pow(10.0, x - 42.0) for x in pl], np.zeros(n))
    else:
        z = keep["z"][perm]
        want = (z, [_log(x) for x in keep["om_arr"][perm]], z * z)
    for got, w in zip((a1, P, U), want):
        assert within_ulp(got, w)
    # the per-field sums of the closed-form part, against math.fsum of the same terms
    for f in range(d.nf):
        lo, hi = int(fi[f]), int(fi[f + 1])
        m = hi - lo
        terms = {9: pl[lo:hi] - 42.0, 10: P[lo:hi] if variant != "zevol" else [], 11: a1[lo:hi] if variant == "fixcomp" else (P[lo:hi] if variant == "zevol" else []),
                 12: a1[lo:hi] if variant == "zevol" else [], 13: U[lo:hi] if variant == "zevol" else []}
        for row, t in terms.items():
            s = math.fsum(float(x) for x in t)
            assert abs(fields[row, f] - s) <= m * EPS * abs(s), (row, f, fields[row, f], s)
    assert scal[2] == {"free": 3 + d.nf + 1, "fixcomp": 3, "zevol": 7}[variant]
    if key is not None and n and special != "nan":
        assert scal[0] == np.min(key)


def grid(shim, d, gridq=1, zcols=1, collapse=1):
    flags = shim.hp_grid(ctypes.byref(d), gridq, zcols, collapse)
    names = ("G", "PG", "W", "a3", "a4", "L", "wL", "ck", "Dk", "nodes4", "zcol", "a4min", "nodes8", "rec")
    g = {k: slot_d(shim, i) for i, k in enumerate(names)}
    g["zgrid_cols"], g["binned"] = flags & 1, flags >> 1
    return g


trapz = getattr(np, "trapezoid", None) or np.trapz


def test_free_trapezoid_weights_integrate(shim):
    inp = inputs("free", 1000)
    d, keep = desc_of(inp)
    S = d.S
    g = grid(shim, d)
    assert g["G"].size == S * S and g["L"].size == S and g["binned"] == 1          # a separable grid: factors and flux bins
    assert grid(shim, d, gridq=0)["binned"] == 0
    logL, z = keep["logL"], keep["zarr"]
    for h in (np.ones((S, S)), np.exp(-0.7 * (logL - 42.0)) * (1.0 + 0.3 * z[None, :] ** 2)):
        want = trapz(trapz(h * keep["volume_part"][None, :], logL, axis=0), z)
        got = math.fsum(g["W"] * h.ravel())
        assert abs(got - want) <= S * S * EPS * abs(want), (got, want)
    # the records lf_free reads: node min(g, nn - 1) again, pads with W = 0, slot 5 = the smallest a4 of the node's chunk of 64
    nn = S * S
    n8 = g["nodes8"].reshape(-1, 8)
    assert n8.shape[0] == (nn + 63) // 64 * 64
    src = np.minimum(np.arange(n8.shape[0]), nn - 1)
    for col, k in enumerate(("G", "PG", "W", "a3", "a4")):
        want = g[k][src]
        if k == "W":
            want = np.where(np.arange(n8.shape[0]) < nn, want, 0.0)
        np.testing.assert_array_equal(n8[:, col], want)
    for ch in range(n8.shape[0] // 64):
        assert np.all(n8[ch * 64:(ch + 1) * 64, 5] == np.min(g["a4"][ch * 64:min(nn, (ch + 1) * 64)]))
    assert np.all(n8[:, 6:] == 0.0)
    np.testing.assert_array_equal(g["a4min"], [np.min(g["a4"][c * 256:(c + 1) * 256]) for c in range((nn + 255) // 256)])


def test_fixcomp_grid_collapses_to_its_row_sums(shim):
    d, keep = desc_of(inputs("fixcomp", 300))
    S = d.S
    lattice, rows = grid(shim, d, collapse=0), grid(shim, d)
    assert lattice["G"].size == S * S and rows["G"].size == S
    np.testing.assert_array_equal(lattice["G"], keep["logL"].ravel())                # the lattice comes back
    np.testing.assert_array_equal(rows["G"], keep["logL"][:, 0])
    want = np.array([math.fsum(r) for r in lattice["W"].reshape(S, S)])
    assert np.all(np.abs(rows["W"] - want) <= S * S * EPS * np.abs(want))
    for g in (lattice, rows):                                                         # lf_pers's records
        nn = g["G"].size
        n4 = g["nodes4"].reshape(-1, 4)
        assert n4.shape[0] == (nn + 63) // 64 * 64
        src = np.minimum(np.arange(n4.shape[0]), nn - 1)
        np.testing.assert_array_equal(n4[:, 0], g["G"][src])
        np.testing.assert_array_equal(n4[:, 1], g["PG"][src])
        np.testing.assert_array_equal(n4[:, 2], np.where(np.arange(n4.shape[0]) < nn, g["W"][src], 0.0))
        assert np.all(n4[:, 3] == 0.0)
        np.testing.assert_array_equal(g["zcol"].reshape(S, 2), np.stack([keep["zarr"], keep["zarr"] ** 2], axis=1))


def test_zevol_grid_is_stored_by_columns(shim):
    d, _ = desc_of(inputs("zevol", 800))
    S = d.S
    cols, rows = grid(shim, d), grid(shim, d, zcols=0)
    assert cols["zgrid_cols"] == 1 and rows["zgrid_cols"] == 0
    for k in ("G", "PG", "W", "a3", "a4"):
        np.testing.assert_array_equal(cols[k].reshape(S, S), rows[k].reshape(S, S).T)   # node k S + j holds what j S + k held
    np.testing.assert_array_equal(cols["nodes4"].reshape(-1, 4)[:S * S, 3], np.arange(S * S) // S)


def radii():
    """CELL_RHO_G, CELL_RHO_H, ZCELL_RHO, ZCELL_X1, ZCELL_X2, CELL_M, ZCELL_M as lf_kernels.h states them"""
    src = open(os.path.join(CSRC, "lf_kernels.h")).read()
    pat = r"CELL_RHO_G = ([0-9.e-]+), CELL_RHO_H = ([0-9.e-]+);.*ZCELL_RHO = ([0-9.e-]+), ZCELL_X1 = ([0-9.e-]+), ZCELL_X2 = ([0-9.e-]+);"
    orders = [re.search(r"constexpr int %s = (\d+);" % k, src).group(1) for k in ("CELL_M", "ZCELL_M")]
    return np.array([float(v) for v in list(re.search(pat, src, re.S).groups()) + orders])


def margins():
    src = open(os.path.join(CSRC, "lf_tables.h")).read()
    return tuple(float.fromhex(re.search(r"%s = (0x[0-9a-fp.+-]+)" % k, src).group(1)) for k in ("G_MARGIN", "H_MARGIN"))


@pytest.mark.parametrize("variant,n,special", [c for c in CASES if c[0] != "fixcomp"] + [("fixcomp", 5003, None)])
def test_chunk_tables(shim, variant, n, special):
    d, keep = desc_of(inputs(variant, n, special))
    fi = keep["fi"]
    gm, hm = margins()
    KS, scale = int(shim.hp_const(6)), shim.hp_const(7)
    for size in CHUNK_SIZES:
        for lane_w in ((0,) if variant == "fixcomp" else (0, size // 512 if size % 512 == 0 else size // 256)):
            shim.hp_chunks(ctypes.byref(d), size, lane_w, gm, hm)
            st, ln, fl, keys = (slot_i(shim, i) for i in range(4))
            x, x0 = slot_d(shim, 0), slot_d(shim, 1)[0]
            keys = keys.reshape(-1, KS)
            seen = np.zeros(n, dtype=np.int64)
            for s, l, f, k in zip(st, ln, fl, keys):
                assert 0 < l <= size and fi[f] <= s and s + l <= fi[f + 1]          # a chunk lies in one field
                seen[s:s + l] += 1
                xs = x[s:s + l]
                if lane_w == 0 or not np.all(np.isfinite(xs)):
                    assert k[0] == -1                                               # keys that fail every test
                elif k[0] != -1:
                    assert np.all(k[0] <= (xs - x0) * scale) and np.all((xs - x0) * scale <= k[1])
            assert np.all(seen == 1)                                                # every source exactly once
            assert len(st) == sum(-(-int(fi[f + 1] - fi[f]) // size) for f in range(d.nf))


@pytest.mark.parametrize("variant,n,special", [c for c in CASES if c[0] != "fixcomp" and c[1] > 0])
def test_cells(shim, variant, n, special):
    inp = inputs(variant, n, special)
    d, keep = desc_of(inp)
    fi = keep["fi"]
    rad = radii()
    built = shim.hp_cells(ctypes.byref(d), capi._ptr(rad))
    if special == "nan":
        assert not built                                      # a field with a non-finite flux: no cells
        return
    assert built
    free = variant == "free"
    M = int(rad[5 if free else 6])
    rec = slot_d(shim, 0).reshape(-1, M + 2)
    x = slot_d(shim, 1)
    st, ln, fl = (slot_i(shim, i) for i in range(3))
    kk = slot_i(shim, 3)
    cc_fstart = kk[2 * MAXF:]
    rho = min(rad[1], rad[0] / inp["lims"]["alpha"][1]) if free else slot_d(shim, 2)[0]
    assert 0.0 < rho <= (rad[1] if free else rad[2])
    assert np.all(ln <= (64 if free else 256)) and np.all(st[1:] == st[:-1] + ln[:-1]) and st[0] == 0 and st[-1] + ln[-1] == rec.shape[0]
    for f in range(d.nf):
        lo, hi = int(fi[f]), int(fi[f + 1])
        cells = np.concatenate([np.arange(s, s + l) for s, l, ff in zip(st, ln, fl) if ff == f] or [np.zeros(0, dtype=int)])
        r = rec[cells]
        if free:
            assert np.sum(r[:, 1]) == hi - lo                                       # S_0: the sources of the field, each once
            assert len(cells) % 64 == 0                                             # padded to whole chunks of 64 cells ...
            pads = r[:, 1] == 0
            assert np.all(r[pads, 1:] == 0.0)                                       # ... by cells whose sums are all 0
            at = lo
            for c in r[~pads]:                                                      # a cell: a run of neighbours no wider than 2 rho
                run = x[at:at + int(c[1])]
                assert run[-1] - run[0] <= 2.0 * rho and c[0] == 0.5 * (run[0] + run[-1])
                at += int(c[1])
            assert at == hi
            assert cc_fstart[f + 1] - cc_fstart[f] == len(cells) // 64
            if hi > lo:
                x0 = np.min(x)                                                      # the keys' origin: the faintest source of all
                assert kk[f] <= (x[lo] - x0) * 2.0 ** 20 and (x[hi - 1] - x0) * 2.0 ** 20 <= kk[MAXF + f]
        else:
            zs = keep["z"]
            order = lo + np.argsort(zs[lo:hi], kind="stable")
            want = math.fsum(math.pow(10.0, v - 42.0) for v in keep["lum"][order])
            assert abs(math.fsum(r[:, 1]) - want) <= max(hi - lo, 1) * EPS * want
            # |d| <= rho for every source of a cell (the midpoint is the middle of its extremes): S_2 <= rho^2 S_0
            assert np.all(r[:, 3] <= rho * rho * r[:, 1] * (1.0 + 8 * EPS))
            assert np.all((r[:, 0] >= x[lo] if hi > lo else True)) and np.all(r[:, 0] <= x[hi - 1] if hi > lo else True)
    if free:
        assert np.all(np.diff(cc_fstart) >= 0) and cc_fstart[-1] == len(st)
