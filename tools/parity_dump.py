"""What a build of the library computes, dumped for a bit-for-bit comparison with another build (a refactor of the host layer:
the tables that reach the device must not change by one bit).
    python tools/parity_dump.py dump  OUT.npz [--root TREE] [--sizes small|bench|all]   (needs the GPU; one process per dump)
    python tools/parity_dump.py create OUT.json [--root TREE] [--reps 5]                 (times lf_create, 10^6 sources)
    python tools/parity_dump.py compare A.npz B.npz                                      (no GPU)
--root: the checkout whose lumfuncmcmc_amd (and liblfmcmc.so) is loaded; default: the one this file is in.  Inputs and theta
rows come from the seeded generators of THIS checkout's tests/lf_testlib.py either way, so both dumps see the same bytes.
Per case: lnprob_batch, lnprob_pieces, the census of term forms (count_forms on) and lf_last_launch for 256 theta rows drawn in
and a little outside the prior box.  The census is the sensitive part: a changed chunk key, chunk order or cell shows there
even when lnprob agrees to the last bit.  compare: np.array_equal on the raw bytes (-inf and NaN patterns count)."""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = {"small": {"free": [50, 200, 1000, 10000], "fixcomp": [50, 300, 1000], "zevol": [800, 1000]},
         "bench": {"free": [1000000], "fixcomp": [1000000], "zevol": [1000000]}}
ROWS = 256


def thetas(ctx, variant, fsa, seed):
    """Half near the truth (the tests' walkers), half uniform over the prior box widened by 2 % on every side."""
    from lumfuncmcmc_amd import synth
    rng = np.random.default_rng(seed)
    box = ctx.prior_box()
    w = box[:, 1] - box[:, 0]
    wide = rng.uniform(box[:, 0] - 0.02 * w, box[:, 1] + 0.02 * w, size=(ROWS // 2, ctx.ndim))
    return np.ascontiguousarray(np.vstack([synth.walkers(variant, ROWS // 2, seed=seed, fix_sch_al=fsa), wide]))


def record(out, name, ctx, th):
    """count_forms off (the persistent kernels of FIXCOMP / ZEVOL run), then on (lf_main's census)"""
    ctx.set_option("count_forms", 0)
    out[name + "/lnprob"] = ctx.lnprob_batch(th)
    out[name + "/launch"] = np.array(sorted(ctx.last_launch().items()), dtype=object).astype(str)
    ctx.set_option("count_forms", 1)
    out[name + "/lnprob_census"] = ctx.lnprob_batch(th)
    a, b = ctx.lnprob_pieces(th)
    out[name + "/pieceA"], out[name + "/pieceB"] = a, b
    out[name + "/forms"] = np.array(list(ctx.form_counts().values()), dtype=np.int64)
    out[name + "/launch_census"] = np.array(sorted(ctx.last_launch().items()), dtype=object).astype(str)
    ctx.set_option("count_forms", 0)


def context(variant, n, fsa=False, env=None):
    from lf_testlib import make_inputs
    from lumfuncmcmc_amd.capi import LFContext
    for k in env or ():
        os.environ[k] = "1"
    try:
        return LFContext(make_inputs(variant, n, seed=1000 + n % 997, fix_sch_al=fsa))
    finally:
        for k in env or ():
            del os.environ[k]


def dump(path, sizes):
    out = {}
    for variant in ("free", "fixcomp", "zevol"):
        for n in sizes[variant]:
            tag = "%s_n%d" % (variant, n)
            for fsa in (False, True):
                ctx = context(variant, n, fsa)
                th = thetas(ctx, variant, fsa, seed=n + 7)
                record(out, "%s_fsa%d" % (tag, fsa), ctx, th)
                ctx.close()
            if n < 1000:
                continue
            switch = {"fixcomp": "LF_NO_COLLAPSE_GRID", "zevol": "LF_NO_ZGRID_COLS", "free": "LF_NO_GRIDQ"}[variant]
            ctx = context(variant, n, env=[switch])
            th = thetas(ctx, variant, False, seed=n + 7)
            record(out, "%s_%s" % (tag, switch), ctx, th)
            ctx.close()
            ctx = context(variant, n)
            for g in range(9):
                ctx.set_option("geometry", g)
                record(out, "%s_geometry%d" % (tag, g), ctx, th)
            ctx.set_option("geometry", -1)
            if variant == "free":
                for cells in (0, 1):
                    for short in (0, 1):
                        for pers in (0, 2):
                            for st in ((2, 4, 8) if pers else (0,)):
                                ctx.set_option("cells", cells)
                                ctx.set_option("grid_shortcut", short)
                                ctx.set_option("persistent", pers)
                                ctx.set_option("free_st", st)
                                record(out, "%s_cells%d_short%d_pers%d_st%d" % (tag, cells, short, pers, st), ctx, th)
                for k, v in (("cells", 1), ("grid_shortcut", 1), ("persistent", 1), ("free_st", 0)):
                    ctx.set_option(k, v)
                ctx.set_option("grid_share", 1 + 65536 * 3)
                record(out, tag + "_gridshare1of3", ctx, th)
                ctx.set_option("grid_share", 0 + 65536 * 1)
            if variant != "fixcomp":
                ctx.set_option("compress", 1)
                record(out, tag + "_compress", ctx, th)
            ctx.close()
            print("%s: %d arrays so far" % (tag, len(out)), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    np.savez(path, **out)
    print("wrote %s: %d arrays" % (path, len(out)))


def create(path, reps):
    from lf_testlib import make_inputs
    from lumfuncmcmc_amd.capi import LFContext
    res = {}
    for variant in ("free", "zevol"):
        inp = make_inputs(variant, 1000000, seed=3)
        LFContext(inp).close()                                  # (the runtime's own start-up is not lf_create's)
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            ctx = LFContext(inp)
            ts.append(time.perf_counter() - t0)
            ctx.close()
        res[variant] = ts
        print(variant, " ".join("%.4f" % t for t in ts), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    json.dump(res, open(path, "w"))


def compare(pa, pb):
    a, b = np.load(pa), np.load(pb)
    bad = sorted(set(a.files) ^ set(b.files))
    for k in sorted(set(a.files) & set(b.files)):
        x, y = a[k], b[k]
        if x.shape != y.shape or x.dtype != y.dtype or x.tobytes() != y.tobytes():
            bad.append(k)
    print("%d arrays in %s, %d in %s: %d differ" % (len(a.files), pa, len(b.files), pb, len(bad)))
    for k in bad:
        print("  DIFFERS", k)
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["dump", "create", "compare"])
    ap.add_argument("paths", nargs="+")
    ap.add_argument("--root", default=HERE)
    ap.add_argument("--sizes", default="all", choices=["small", "bench", "all"])
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    if a.mode == "compare":
        return compare(*a.paths)
    for p in (os.path.join(HERE, "tests"), os.path.join(HERE, "oracle"), os.path.abspath(a.root)):
        sys.path.insert(0, p)
    from lumfuncmcmc_amd import capi, synth  # noqa: F401       (the root's, before lf_testlib puts its own checkout in front)
    print("library:", capi.LIB_PATH, flush=True)
    if a.mode == "create":
        return create(a.paths[0], a.reps)
    sizes = SIZES[a.sizes] if a.sizes != "all" else {v: SIZES["small"][v] + SIZES["bench"][v] for v in SIZES["small"]}
    return dump(a.paths[0], sizes)


if __name__ == "__main__":
    sys.exit(main())
