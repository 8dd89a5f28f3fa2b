"""Time of one lf_lum_posterior call (csrc/lf_lumpost.h) and its node terms per second, next to
lf_deconv_part's rate on the same context from the same run.

The call is synchronous with host pointers, so it is timed by a host clock around it: the rows' plain lnprob, the kernels over
all (source, row, node) terms, and the copies of theta in and of m1, m2 out - what a user waits for.  One warm-up call on two rows, then the
median over `reps`.  Node terms: (sources with sigma > 0) x (used rows) x K.  For comparison, per context, lf_deconv_part's time
as tools/deconv_cost.py takes it: lf_lnprob_err_batch_device minus lf_lnprob_batch_device between hipEvents, 128 rows, median.
With --twin the NumPy twin's time per row at the smallest size.  One JSON line per (variant, N).

    python tools/lum_posterior_cost.py [--rows 200] [--order 32] [--reps 5] [--sizes 1000000,100000] [--variants free,zevol]
                                       [--twin] [--out FILE.json]"""
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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="1000000,100000")
    ap.add_argument("--variants", default="free,zevol")
    ap.add_argument("--twin", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import numpy as np
    import torch
    from lf_testlib import make_inputs
    from lumfuncmcmc_amd import capi, deconv, synth
    torch.set_num_threads(1)

    def event_us(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3

    res = []
    K = a.order
    sizes = [int(s) for s in a.sizes.split(",")]
    for variant in a.variants.split(","):
        for n in sizes:
            inp = make_inputs(variant, n, seed=1)
            sigma = np.random.default_rng(3).uniform(0.2, 1.0, n) * deconv.sigma_max(K)
            th = synth.walkers(variant, a.rows, seed=2)
            ctx = capi.LFContext(inp, device=0)
            ctx.set_lum_err(sigma, K)
            ctx.lum_posterior(th[:2])                     # (warm-up: the code objects and the workspace, which does not depend on R)
            t = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                m1, m2, used = ctx.lum_posterior(th)
                t.append(time.perf_counter() - t0)
            assert used > 0 and np.all(np.isfinite(m1)) and np.all(m2 > 0.0)
            call_s = float(np.median(t))
            terms = n * used * K
            # lf_deconv_part on the same context: convolved minus plain, 128 rows between events
            thd = torch.from_numpy(synth.walkers(variant, 128, seed=2)).cuda()
            calls = {"plain": lambda: ctx.lnprob_torch(thd), "err": lambda: ctx.lnprob_err_torch(thd)}
            for fn in calls.values():
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            tt = {k: [] for k in calls}
            for _ in range(11):
                for k, fn in calls.items():
                    tt[k].append(event_us(fn))
            part_us = float(np.median(tt["err"]) - np.median(tt["plain"]))
            fin = int(np.isfinite(ctx.lnprob_batch(thd.cpu().numpy())).sum())
            r = {"variant": variant, "N": n, "rows": a.rows, "rows_used": used, "K": K, "call_s": round(call_s, 5),
                 "call_s_min_max": [round(min(t), 5), round(max(t), 5)], "node_terms": terms,
                 "terms_per_s": round(terms / call_s, 1), "deconv_part_us_128_rows": round(part_us, 2),
                 "deconv_part_terms_per_s": round(n * fin * K / (part_us * 1e-6), 1) if part_us > 0 else None}
            r["rate_over_deconv_part"] = round(r["terms_per_s"] / r["deconv_part_terms_per_s"], 4) if r["deconv_part_terms_per_s"] else None
            if a.twin and n == min(sizes):
                t0 = time.perf_counter()
                deconv.lum_posterior(inp, sigma, th[:2], K=K)
                r["twin_s_per_row"] = round((time.perf_counter() - t0) / 2.0, 4)
            print(json.dumps(r), flush=True)
            res.append(r)
            ctx.close()
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
