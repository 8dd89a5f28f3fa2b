"""Device time of one flux-error-convolved batch (lf_lnprob_err_batch_device, which includes its own plain lnprob) next to the
plain lnprob of the same rows and to the NumPy twin on one host core, for FREE and ZEVOL at the default order; and the
gradient leg: lf_lnprob_err_grad_batch_device (the plain gradient, the value and the correction's gradient) next to the plain
lf_lnprob_grad_batch_device.  Warm-up, then hipEvents (torch.cuda.Event) on the stream around every single call, the median
over `reps` calls, all in one process.

    python tools/deconv_cost.py [--rows 128] [--reps 21] [--sizes 1000000,100000] [--twin-rows 1] [--map-fit 100000] [--out FILE.json]
    python tools/deconv_cost.py --tile [--rows 128] [--reps 21] [--sizes 1000000,100000] [--walkers 256] [--converged 100000]

Prints one JSON line per (variant, N): median us per call of each, the correction's own time, the node terms per second and
the share of the fp64 vector peak they stand for at FLOPS_PER_NODE counted flops per node term (DESIGN.md sections 3.18, 3.19).
--map-fit N: then the wall time of one fit_model_map(likelihood="convolved") (8 starts) on a noisy mock of about N sources at
fixed completeness, and of the plain fit of the same object, as one more JSON line.
--tile: instead, the row-tiled correction kernel (context option "deconv_tile") against the per-row
kernels on FIXCOMP and ZEVOL by the same method, the two alternated call by call in one process: median and quartiles of both
at every size with K = 32, at the smallest size with K = 12 as well, and the verdict - the tile kernel counts as faster only
when its median lies below the per-row median by more than the sum of the two interquartile ranges; then the wall time of a
convolved device-sampler half-step at --walkers walkers with the option off and on, and with --converged N one
fit_model_converged(likelihood="convolved") on a noisy mock of about N sources."""
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


def quartiles(t):
    import numpy as np
    q1, med, q3 = (float(x) for x in np.percentile(t, [25, 50, 75]))
    return {"median_us": round(med, 2), "q1_us": round(q1, 2), "q3_us": round(q3, 2), "iqr_us": round(q3 - q1, 2)}


def tile_runs(a):
    import numpy as np
    import torch
    from lf_testlib import make_inputs
    from lumfuncmcmc_amd import capi, deconv, synth
    from lumfuncmcmc_amd.sampler import DeviceEnsembleSampler
    torch.set_num_threads(1)
    sizes = [int(s) for s in a.sizes.split(",")]
    res = []

    def event_us(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3

    for variant in ("fixcomp", "zevol"):
        for n in sizes:
            inp = make_inputs(variant, n, seed=1)
            sigma = np.random.default_rng(3).uniform(0.0, deconv.SIGMA_MAX, n)
            ctx = capi.LFContext(inp, device=0)
            th_h = synth.walkers(variant, a.rows, seed=2)
            th = torch.from_numpy(th_h).cuda()
            for K in ([deconv.DEFAULT_ORDER, 12] if n == min(sizes) else [deconv.DEFAULT_ORDER]):
                ctx.set_lum_err(sigma, K, unchecked=True)
                out, t = {}, {0: [], 1: []}
                for tile in (0, 1):
                    ctx.set_option("deconv_tile", tile)
                    for _ in range(3):
                        out[tile] = ctx.lnprob_err_torch(th)
                torch.cuda.synchronize()
                t_plain = [event_us(lambda: ctx.lnprob_torch(th)) for _ in range(a.reps)]
                for _ in range(a.reps):
                    for tile in (0, 1):
                        ctx.set_option("deconv_tile", tile)
                        t[tile].append(event_us(lambda: ctx.lnprob_err_torch(th)))
                o0, o1 = out[0].cpu().numpy(), out[1].cpu().numpy()
                fin = np.isfinite(o0)
                q0, q1 = quartiles(t[0]), quartiles(t[1])
                r = {"variant": variant, "N": n, "rows": a.rows, "K": K, "lnprob": quartiles(t_plain), "per_row": q0, "tile": q1,
                     "tile_over_per_row": round(q1["median_us"] / q0["median_us"], 4),
                     "faster": bool(q1["median_us"] < q0["median_us"] - (q0["iqr_us"] + q1["iqr_us"])),
                     "same_inf_pattern": bool(np.array_equal(fin, np.isfinite(o1))),
                     "max_rel_diff": float(np.max(np.abs(o0[fin] - o1[fin]) / np.abs(o0[fin]))) if fin.any() else 0.0}
                print(json.dumps(r), flush=True)
                res.append(r)
            if n == min(sizes):
                # one convolved half-step of the device sampler: wall time around `steps` steps that end in a synchronise
                ctx.set_lum_err(sigma, deconv.DEFAULT_ORDER)
                W, steps = a.walkers, 10
                pos = synth.walkers(variant, W, seed=4)
                r = {"variant": variant, "N": n, "walkers": W, "K": deconv.DEFAULT_ORDER, "steps_timed": steps}
                for tile in (0, 1):
                    ctx.set_option("deconv_tile", tile)
                    ds = DeviceEnsembleSampler(ctx, W, seed=1, capacity=4 * steps, likelihood="convolved")
                    ds.enqueue(pos, steps)
                    torch.cuda.synchronize()
                    t = []
                    for _ in range(3):
                        t0 = time.perf_counter()
                        ds.enqueue(None, steps)
                        torch.cuda.synchronize()
                        t.append((time.perf_counter() - t0) / (2 * steps) * 1e6)
                    ds.close()
                    r["half_step_us_tile%d" % tile] = [round(x, 1) for x in sorted(t)]
                print(json.dumps(r), flush=True)
                res.append(r)
            ctx.close()
    if a.converged > 0:
        import lf_deconvlib
        for tile in (False, True):
            np.random.seed(3)
            o, truth, _ = lf_deconvlib.noisy_mock(a.converged, deconv.SIGMA_MAX, seed=3, deconvolve=True, deconvolve_tile=tile, nsteps=1000)
            o.context().lnprob_err_batch(o.get_init_walker_values(16))           # (warm-up: the context, the tables)
            t0 = time.perf_counter()
            o.fit_model_converged(likelihood="convolved")
            dt = time.perf_counter() - t0
            r = {"converged_fit_N": len(o.lum), "K": o.deconvolve_order, "deconvolve_tile": tile, "walkers": o.nwalkers,
                 "steps": int(o.chain.shape[1]), "converged": bool(o.converged), "wall_s": round(dt, 3),
                 "max_tau": round(float(np.max(o.tau_history[-1][1])), 2), "chain_mean_Lstar": round(float(o.samples[:, 0].mean()), 5),
                 "true_Lstar": round(float(truth[0]), 5)}
            o.close()
            print(json.dumps(r), flush=True)
            res.append(r)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=128)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--sizes", default="1000000,100000")
    ap.add_argument("--twin-rows", type=int, default=1)
    ap.add_argument("--map-fit", type=int, default=0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--tile", action="store_true")
    ap.add_argument("--walkers", type=int, default=256)
    ap.add_argument("--converged", type=int, default=0)
    a = ap.parse_args()
    if a.tile:
        return tile_runs(a)
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
