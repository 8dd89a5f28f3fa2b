"""Cost of the integrated-LF bands: the device time of lf_bands_integ (lf_lumfunc_integral_quantiles,
three quantiles) at (R, P) = (200, 10^4), (1000, 10^4), (200, 10^6), and alongside, in the same run, lf_lumfunc_quantiles
(lf_bands, the differential LF) on the same shape and the wall time of the host twin (lfintegrals.quantiles_host).
Prints one JSON line.

   python tools/integrals_cost.py [--reps 5] [--host-max 250000000] [--variant free]

kernel_ms is the device time of the launch alone (hipEvents around it), the best of `reps`; wall times are
time.perf_counter around the call, transfers included.  The host twin is timed once, and only on shapes of at most
--host-max values (it evaluates every loop to the slowest element's trip count: about 1.3 x 10^6 values per second: minutes at 2 x 10^8).
The draws spread alpha over [-3, 1] and the limits logLmin - logL* over about [-3.5, 3.5], so a wave meets all three
branches of Gamma(a, x).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lumfuncmcmc_amd import capi, lfbands, lfintegrals      # noqa: E402

Q = (16.0, 50.0, 84.0)
SHAPES = ((200, 10 ** 4), (1000, 10 ** 4), (200, 10 ** 6))
PIV = (1.2, 1.53, 1.86)


def inputs(variant, R, P):
    rng = np.random.default_rng(R + P)
    lmin = rng.uniform(39.0, 46.0, P)
    if variant == "free":
        return np.column_stack([rng.normal(42.5, 0.3, R), rng.normal(-2.5, 0.4, R), rng.uniform(-3.0, 1.0, R)]), lmin, None
    rows = np.column_stack([rng.normal(42.5, 0.15, (R, 3)), rng.normal(-2.5, 0.15, (R, 3)), rng.uniform(-3.0, 1.0, R)])
    return lfbands.pack_draws("zevol", rows, pivots=PIV), lmin, rng.uniform(1.1, 2.0, P)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-max", type=int, default=250000000)
    ap.add_argument("--variant", default="free", choices=("free", "zevol"))
    a = ap.parse_args()
    res = {"tool": "integrals_cost", "variant": a.variant, "numpy": np.__version__, "cpus": len(os.sched_getaffinity(0))}
    d, lmin, z = inputs(a.variant, 8, 64)
    capi.lumfunc_integral_quantiles(a.variant, 0, d, lmin, z=z, q=Q)               # warm-up: initialises HIP
    for R, P in SHAPES:
        draws, lmin, z = inputs(a.variant, R, P)
        r = {}
        for kind, k in lfintegrals.KINDS.items():
            kms, walls = [], []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                capi.lumfunc_integral_quantiles(a.variant, k, draws, lmin, z=z, q=Q)
                walls.append(time.perf_counter() - t0)
                kms.append(capi.lumfunc_integral_quantiles_ms())
            r["integ_%s_kernel_ms" % kind] = min(kms)
            r["integ_%s_wall_s" % kind] = min(walls)
        kms = []
        for _ in range(a.reps):
            capi.lumfunc_quantiles(a.variant, draws, lmin, z=z, q=Q)
            kms.append(capi.lumfunc_quantiles_ms())
        r["bands_kernel_ms"] = min(kms)
        if R * P <= a.host_max:
            t0 = time.perf_counter()
            lfintegrals.quantiles_host(a.variant, "lumdens", draws, lmin, z=z, q=Q)
            r["host_twin_lumdens_wall_s"] = time.perf_counter() - t0
        else:
            r["host_twin_lumdens_wall_s"] = "not run: %d values > --host-max" % (R * P)
        res["R%d_P%d" % (R, P)] = r
    print(json.dumps(res))


if __name__ == "__main__":
    main()
