"""Device time of one flux-error-convolved batch (lf_lnprob_err_batch_device, which includes its own plain lnprob) next to the
plain lnprob of the same rows and to the NumPy twin on one host core, for FREE and ZEVOL at the default order; and the
gradient leg: lf_lnprob_err_grad_batch_device (the plain gradient, the value and the correction's gradient) next to the plain
lf_lnprob_grad_batch_device.  Warm-up, then hipEvents (torch.cuda.Event) on the stream around every single call, the median
over `reps` calls, all in one process.

    python tools/deconv_cost.py [--rows 128] [--reps 21] [--sizes 1000000,100000] [--twin-rows 1] [--map-fit 100000] [--out FILE.json]

Prints one JSON line per (variant, N): median us per call of each, the correction's own time, the node terms per second and
the share of the fp64 vector peak they stand for at FLOPS_PER_NODE counted flops per node term (DESIGN.md sections 3.18, 3.19).
--map-fit N: then the wall time of one fit_model_map(likelihood="convolved") (8 starts) on a noisy mock of about N sources at
fixed completeness, and of the plain fit of the same object, as one more JSON line."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

PEAK_FP64_VECTOR = 78.6e12      # MI355X, fp64 vector peak of the data sheet (half the fp32 vector rate)
# per node term, as written in lf_deconv.h: expm1, exp, expm1 and log / log1p of the device library at about 40 fp64 operations
# each, a square root and two divisions at about 15, and 25 multiplies, adds and compares around them
FLOPS_PER_NODE = 4 * 40 + 3 * 15 + 25


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=128)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--sizes", default="1000000,100000")
    ap.add_argument("--twin-rows", type=int, default=1)
    ap.add_argument("--map-fit", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from lf_testlib import make_inputs
    from lumfuncmcmc_amd import capi, deconv, synth
    torch.set_num_threads(1)
    K = deconv.DEFAULT_ORDER
    res = []
    for variant in ("free", "zevol"):
        for n in (int(s) for s in a.sizes.split(",")):
            inp = make_inputs(variant, n, seed=1)
            sigma = np.random.default_rng(3).uniform(0.0, deconv.SIGMA_MAX, n)
            ctx = capi.LFContext(inp, device=0)
            ctx.set_lum_err(sigma, K)
            th_h = synth.walkers(variant, a.rows, seed=2)
            th = torch.from_numpy(th_h).cuda()

            def timed(fn):
                for _ in range(3):
                    fn()
                torch.cuda.synchronize()
                t = []
                for _ in range(a.reps):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    fn()
                    e1.record()
                    torch.cuda.synchronize()
                    t.append(e0.elapsed_time(e1) * 1e3)
                return float(np.median(t))

            us_lnprob = timed(lambda: ctx.lnprob_torch(th))
            us_err = timed(lambda: ctx.lnprob_err_torch(th))
            us_grad = timed(lambda: ctx.lnprob_grad_torch(th))
            us_err_grad = timed(lambda: ctx.lnprob_err_grad_torch(th))
            us_lnprob_after = timed(lambda: ctx.lnprob_torch(th))
            ctx.close()
            t0 = time.perf_counter()
            deconv.delta(inp, sigma, th_h[:a.twin_rows], K=K)
            twin_s = (time.perf_counter() - t0) / a.twin_rows
            nodes = float(n) * K * a.rows
            own = max(us_err - us_lnprob, 1e-9)
            r = {"variant": variant, "N": n, "rows": a.rows, "K": K, "lnprob_us": round(us_lnprob, 2), "err_us": round(us_err, 2),
                 "correction_us": round(own, 2), "ratio": round(us_err / us_lnprob, 2), "twin_s_per_row_one_core": round(twin_s, 3),
                 "node_terms_per_s": float("%.4g" % (nodes / (own * 1e-6))),
                 "fp64_vector_peak_share": round(nodes * FLOPS_PER_NODE / (own * 1e-6) / PEAK_FP64_VECTOR, 4),
                 "grad_us": round(us_grad, 2), "err_grad_us": round(us_err_grad, 2),
                 "err_grad_over_err": round(us_err_grad / us_err, 3), "lnprob_us_after": round(us_lnprob_after, 2)}
            print(json.dumps(r), flush=True)
            res.append(r)
    if a.map_fit > 0:
        import lf_deconvlib
        np.random.seed(3)
        o, truth, _ = lf_deconvlib.noisy_mock(a.map_fit, deconv.SIGMA_MAX, seed=3, deconvolve=True)
        o.fit_model_map(nstarts=8, seed=1, likelihood="plain")                  # (warm-up: the context, the tables)
        t0 = time.perf_counter()
        p = dict(o.fit_model_map(nstarts=8, seed=1, likelihood="plain"))
        t1 = time.perf_counter()
        c = dict(o.fit_model_map(nstarts=8, seed=1, likelihood="convolved"))
        t2 = time.perf_counter()
        r = {"map_fit_N": len(o.lum), "K": o.deconvolve_order, "nstarts": 8, "plain_s": round(t1 - t0, 3), "convolved_s": round(t2 - t1, 3),
             "plain_niter": p["niter"], "convolved_niter": c["niter"], "plain_converged": p["converged"],
             "convolved_converged": c["converged"], "plain_Lstar": round(float(p["theta"][0]), 5),
             "convolved_Lstar": round(float(c["theta"][0]), 5), "true_Lstar": round(float(truth[0]), 5)}
        o.close()
        print(json.dumps(r), flush=True)
        res.append(r)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
