"""Time of one lf_veff_true call (csrc/lf_vefftrue.h) and its node terms per second, next to
lf_lum_posterior's rate - the same node loop without the binning - on the same context in the same process.

Both calls are synchronous with host pointers, so they are timed by a host clock around them: the rows' plain lnprob, the
kernels, and the copies in and out - what a user waits for.  One warm-up call of each on two rows, then the two calls alternate
`reps` times: medians with min and max.  lf_veff_true_ms gives the device times of the node kernel, the chunk sums and the
quantiles of the last call (hipEvents, summed over the row groups; taken under lf_set_profiling, which this tool sets: the
event pairs around every launch are part of what is timed).  Node terms: (sources with sigma > 0) x (used rows) x K.
One JSON line per (variant, N).

    python tools/veff_true_cost.py [--rows 200] [--order 32] [--bins 50] [--reps 5] [--sizes 1000000,100000]
                                   [--variants free,zevol] [--out FILE.json]"""
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
    ap.add_argument("--sizes", default="1000000,100000")
    ap.add_argument("--variants", default="free,zevol")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import numpy as np
    from lf_testlib import make_inputs
    from lumfuncmcmc_amd import capi, deconv, synth, veff

    res = []
    K = a.order
    for variant in a.variants.split(","):
        for n in [int(s) for s in a.sizes.split(",")]:
            inp = make_inputs(variant, n, seed=1)
            sigma = np.random.default_rng(3).uniform(0.2, 1.0, n) * deconv.sigma_max(K)
            th = synth.walkers(variant, a.rows, seed=2)
            edges = veff.luminosity_bins(inp["lum"], a.bins)[0]
            ctx = capi.LFContext(inp, device=0)
            ctx.set_lum_err(sigma, K)
            ctx.set_profiling(1)                                       # (lf_veff_true_ms: the stages are stamped only then)
            ctx.veff_true(th[:2], edges, 3.1e-5, 2.7e6)                # (warm-up: the code objects and the context's workspace)
            ctx.lum_posterior(th[:2])
            tv, tl, ms = [], [], []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                out, values, used = ctx.veff_true(th, edges, 3.1e-5, 2.7e6)
                tv.append(time.perf_counter() - t0)
                ms.append(capi.veff_true_ms())
                t0 = time.perf_counter()
                m1, m2, used_l = ctx.lum_posterior(th)
                tl.append(time.perf_counter() - t0)
            assert used == used_l > 0 and np.all(np.isfinite(out)) and np.all(np.isfinite(m1))
            terms = n * used * K
            sv, sl = float(np.median(tv)), float(np.median(tl))
            r = {"variant": variant, "N": n, "rows": a.rows, "rows_used": used, "K": K, "bins": a.bins, "node_terms": terms,
                 "veff_true_s": round(sv, 5), "veff_true_s_min_max": [round(min(tv), 5), round(max(tv), 5)],
                 "veff_true_terms_per_s": round(terms / sv, 1),
                 "stage_ms_part_reduce_quantiles": [round(float(v), 3) for v in np.median(np.array(ms), axis=0)],
                 "lum_posterior_s": round(sl, 5), "lum_posterior_s_min_max": [round(min(tl), 5), round(max(tl), 5)],
                 "lum_posterior_terms_per_s": round(terms / sl, 1), "rate_over_lum_posterior": round(sl / sv, 4)}
            print(json.dumps(r), flush=True)
            res.append(r)
            ctx.close()
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
