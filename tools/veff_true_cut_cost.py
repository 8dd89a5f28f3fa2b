"""Cost of the deconvolved 1/Veff points under the cut (csrc/lf_vefftrue_cut.h) next to the plain
lf_veff_true call (section 3.26), in one process.

A context without the cut model needs a grid with one set of luminosity nodes, a context with it a grid with an edge per
column, so there are two contexts over the same sources, the same sigma and the same rows: `plain` (tests/lf_testlib.py:
make_inputs) and `cut` (tests/lf_cutlib.py: cut_inputs, the 1/flux error model, option "deconv_cut_veff").  One warm-up call of
each on two rows - the cut context's makes the table of 1 / g, timed by events of its own (lf_veff_true_cut_ms) - then the two
calls alternate `reps` times, timed by a host clock around the synchronous calls: medians with min and max.  lf_veff_true_ms
gives the device time of the node kernel (part), which is where the extra 8-byte load per node shows.  One JSON line per N.

    python tools/veff_true_cut_cost.py [--rows 200] [--order 32] [--bins 50] [--reps 5] [--sizes 100000,1000000] [--out FILE.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=200)
    ap.add_argument("--order", type=int, default=32)
    ap.add_argument("--bins", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="100000,1000000")
    ap.add_argument("--variant", default="free")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import numpy as np
    import lf_cutlib as C
    from lf_testlib import make_inputs
    from lumfuncmcmc_amd import capi, deconv, synth, veff

    res = []
    K = a.order
    for n in [int(s) for s in a.sizes.split(",")]:
        plain_inp = make_inputs(a.variant, n, seed=11)
        S, nf = len(plain_inp["zarr"]), len(plain_inp["field_ind"]) - 1
        cut_inp = C.cut_inputs(a.variant, n=n, S=S, nf=nf, seed=11)
        sigma = np.random.default_rng(3).uniform(0.2, 1.0, n) * deconv.sigma_max(K)
        th = synth.walkers(a.variant, a.rows, seed=2, nf=nf)
        edges = veff.luminosity_bins(plain_inp["lum"], a.bins)[0]
        plain = capi.LFContext(plain_inp, device=0)
        cut = capi.LFContext(cut_inp, device=0)
        cut.set_cut_error_model(*C.flux_model(0.09, nf=nf))
        cut.set_option("deconv_cut_veff", 1)
        for ctx in (plain, cut):
            ctx.set_lum_err(sigma, K)
            ctx.set_profiling(1)
            ctx.veff_true(th[:2], edges, 3.1e-5, 2.7e6)
        info = cut.veff_true_cut_info()
        tp, tc, mp, mc = [], [], [], []
        for _ in range(a.reps):
            for ctx, t, ms in ((plain, tp, mp), (cut, tc, mc)):
                t0 = time.perf_counter()
                out, _, used = ctx.veff_true(th, edges, 3.1e-5, 2.7e6)
                t.append(time.perf_counter() - t0)
                ms.append(capi.veff_true_ms()[0])
                assert used > 0 and np.all(np.isfinite(out))
        r = {"variant": a.variant, "N": n, "S": S, "rows": a.rows, "K": K, "bins": a.bins,
             "plain_s": round(float(np.median(tp)), 5), "plain_s_min_max": [round(min(tp), 5), round(max(tp), 5)],
             "cut_s": round(float(np.median(tc)), 5), "cut_s_min_max": [round(min(tc), 5), round(max(tc), 5)],
             "plain_part_ms": round(float(np.median(mp)), 3), "cut_part_ms": round(float(np.median(mc)), 3),
             "table_ms": round(info["ms"], 3), "table_slots": info["slots"], "table_bytes": info["bytes"],
             "table_dropped": info["dropped"], "table_erfc_terms_at_most": info["slots"] * S}
        print(json.dumps(r), flush=True)
        res.append(r)
        plain.close()
        cut.close()
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
