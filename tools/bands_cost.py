"""Cost of the posterior LF bands: the median step of LumFuncMCMC.set_median_fit on the host and on
the device (lf_lumfunc_quantiles, LF_Q_MEDIAN) at N = 10^6 sources, R = 200 and 1000 draws, and lf_percentiles with five
quantiles.  Prints one JSON line.

   python tools/bands_cost.py [--n 1000000] [--host-r 200] [--device-only]

The median step is set_median_fit without its 1/Veff estimate (the same in both paths): the draws, R TrueLumFunc
evaluations over the catalogue and their median.  Wall times are time.perf_counter around the call, transfers included;
kernel_ms is the device time of the lf_bands launch alone (hipEvents around it, lf_lumfunc_quantiles_ms), the best of
`reps`.  --host-r lists the R at which the host path is timed (its R x N float64 matrix is 8 GB at R = 1000).
fp64 work per call: R N evaluations of LN10 10^phi* 10^(t (alpha + 1)) exp(-10^t), three transcendentals each
(exp10, exp10, exp) plus 6 plain operations; the lower bound divides that by the MI355X's fp64 vector rate.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lumfuncmcmc_amd import capi, synth            # noqa: E402
from lumfuncmcmc_amd.model import LumFuncMCMC       # noqa: E402

FP64_VECTOR_OPS = 256 * 4 * 16 * 2.4e9       # fp64 VALU lane-operations per second: 256 CUs x 4 SIMDs x 16 lanes x 2.4 GHz
OPS_PER_TRANSCENDENTAL = 20                  # estimate for the device library's fp64 exp / exp10 (range reduction + degree-~11 polynomial + scaling)


def model(n):
    cat = synth.catalogue(n, seed=20241016)
    fi = cat["field_ind"]
    m = LumFuncMCMC(synth.split_fields(cat["z"], fi), lum=synth.split_fields(cat["lum"], fi),
                    lum_e=synth.split_fields(cat["lum_e"], fi), Flim=list(synth.FLIM), alpha=synth.ALPHA_C,
                    Omega_0=list(synth.OMEGA_0), sch_al=synth.SCH_AL, sch_al_lims=synth.SCH_AL_LIMS, Lstar=synth.LSTAR,
                    Lstar_lims=synth.LSTAR_LIMS, phistar=synth.PHISTAR, phistar_lims=synth.PHISTAR_LIMS, Lc=synth.LC,
                    Lh=synth.LH, nwalkers=100, nsteps=10, min_comp_frac=0.0, field_ind=fi, Flim_lims=synth.FLIM_LIMS,
                    alpha_lims=synth.ALPHA_LIMS)
    rng = np.random.default_rng(1)
    th = np.column_stack([rng.normal(42.6, 0.05, 5000), rng.normal(-2.1, 0.05, 5000), rng.normal(-1.5, 0.05, 5000)] +
                         [rng.normal(f, 0.1, 5000) for f in synth.FLIM] + [rng.normal(synth.ALPHA_C, 0.1, 5000)])
    m.samples = np.column_stack([th, rng.normal(-100.0, 3.0, 5000)])
    m.VeffLF = lambda *a, **k: None             # the median step only
    m.log.setLevel("WARNING")
    return m


def mem_available():
    """bytes the host can still give (the host path holds the R x N matrix, its list of rows and numpy's copy)"""
    try:
        for line in open("/proc/meminfo"):
            if line.startswith("MemAvailable:"):
                return int(line.split()[1]) * 1024
    except OSError:
        pass
    return 0


def median_step(m, R, device):
    np.random.seed(3)
    t0 = time.perf_counter()
    m.set_median_fit(rndsamples=R, device=device)
    return time.perf_counter() - t0, m.medianLF.copy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--host-r", type=int, nargs="*", default=[200])
    ap.add_argument("--device-only", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    m = model(a.n)
    res = {"tool": "bands_cost", "n": a.n, "numpy": np.__version__, "cpus": len(os.sched_getaffinity(0))}
    median_step(m, 8, True)                     # warm-up: context-free lf_lumfunc_quantiles initialises HIP
    for R in (200, 1000):
        walls, kms = [], []
        for _ in range(a.reps):
            w, dev = median_step(m, R, True)
            walls.append(w)
            kms.append(capi.lumfunc_quantiles_ms())
        evals = R * a.n
        ops = evals * (3 * OPS_PER_TRANSCENDENTAL + 6)
        r = {"device_median_wall_s": min(walls), "device_median_kernel_ms": min(kms),
             "evaluations": evals, "transcendentals": 3 * evals, "fp64_ops_estimate": ops,
             "fp64_lower_bound_ms": ops / FP64_VECTOR_OPS * 1e3}
        if R in a.host_r and not a.device_only and mem_available() < 3 * 8 * evals:
            r["host_median_wall_s"] = "not run: needs %.0f GB of host memory" % (3 * 8 * evals / 1e9)
        elif R in a.host_r and not a.device_only:
            w, host = median_step(m, R, False)
            r["host_median_wall_s"] = w
            r["max_rel_diff_vs_host"] = float(np.max(np.abs(dev - host) / np.maximum(np.abs(host), 1e-300)))
        res["median_R%d" % R] = r
        np.random.seed(4)
        kms = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            m.lf_percentiles(percentiles=(2.5, 16, 50, 84, 97.5), ndraws=R, device=True)
            w = time.perf_counter() - t0
            kms.append(capi.lumfunc_quantiles_ms())
        res["percentiles5_R%d" % R] = {"wall_s": w, "kernel_ms": min(kms)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
