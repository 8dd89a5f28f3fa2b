"""Cost of the chain diagnostics on the device (lf_chain_diag, csrc/lf_diag.h) on one MI355X, against
what the code did before for the same answer: the chain copied to the host and sampler.integrated_time per parameter.

Cases: W = 256 walkers, ndim = 5 and 8, n = 10^4 and 10^5 steps of a seeded AR(1) chain with tau ~ 50 and ~ 500
(rho = (tau - 1) / (tau + 1)).  Per case:
  device_kernel_ms   the diagnostics' kernels (hipEvents around every bracket of launches, lf_diag_last), median of --reps calls
                     after one warm-up call;
  device_wall_ms     wall time of lf_chain_diag, which first uploads the chain from the host - a copy the samplers' own entries
                     (lf_sampler_diag, lf_ptsampler_diag) do not make;
  lags               lags per series the window rule needed; fma = n x lags x W x ndim; bound_ms = fma at the fp64 vector peak
                     (78.6 TFLOP/s = 39.3e12 FMA/s); frac_of_bound = bound_ms / device_kernel_ms;
  host_read_ms       the chain's bytes from device memory to pageable host memory (what lf_sampler_read moves);
  host_acor_ms       get_autocorr_time's loop (integrated_time per parameter, one FFT pair per walker) on --host-walkers of the
                     256 walkers, scaled to 256 (its cost is linear in the walkers);
  ratio              (host_read_ms + host_acor_ms) / device_kernel_ms.
Writes one JSON document to --out and prints it.

    python tools/diag_cost.py [--reps 3] [--host-walkers 32] [--out profiles/r07_diag_cost.json]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from lumfuncmcmc_amd import capi                                        # noqa: E402
from lumfuncmcmc_amd.sampler import chain_diagnostics, integrated_time   # noqa: E402

PEAK_FMA = 78.6e12 / 2.0


def ar1_chain(W, n, ndim, tau, seed):
    from scipy.signal import lfilter
    rho = (tau - 1.0) / (tau + 1.0)
    e = np.random.RandomState(seed).standard_normal((W, n, ndim))
    e[:, 1:] *= np.sqrt(1.0 - rho * rho)
    x = lfilter([1.0], [1.0, -rho], e, axis=1)
    return np.ascontiguousarray(0.01 * x + 40.0 + np.arange(ndim))


def diag_last():
    ms, lags = ctypes.c_double(), ctypes.c_int64()
    assert capi.load().lf_diag_last(ctypes.byref(ms), ctypes.byref(lags)) == 0
    return ms.value, lags.value


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-walkers", type=int, default=32)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    W = 256
    cases = []
    for ndim in (5, 8):
        for n in (10 ** 4, 10 ** 5):
            for tau in (50.0, 500.0):
                chain = ar1_chain(W, n, ndim, tau, seed=len(cases))
                chain_diagnostics(chain)                                  # warm-up
                kms, wall = [], []
                for _ in range(args.reps):
                    t0 = time.perf_counter()
                    r = chain_diagnostics(chain)
                    wall.append((time.perf_counter() - t0) * 1e3)
                    k, lags = diag_last()
                    kms.append(k)
                dev = torch.from_numpy(chain).cuda()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                back = dev.cpu()
                read_ms = (time.perf_counter() - t0) * 1e3
                del dev
                hw = min(args.host_walkers, W)
                sub = back.numpy()[:hw]
                t0 = time.perf_counter()
                host_tau_sub = np.array([integrated_time(sub[:, :, d].T) for d in range(ndim)])
                acor_ms = (time.perf_counter() - t0) * 1e3 * W / hw
                fma = float(n) * lags * W * ndim
                kmed = float(np.median(kms))
                c = {"W": W, "ndim": ndim, "n": n, "tau_target": tau, "device_tau_max": float(r.tau.max()),
                     "device_window_max": int(r.window.max()), "host_tau_max_of_%d_walkers" % hw: float(host_tau_sub.max()),
                     "lags": int(lags), "device_kernel_ms": kmed, "device_kernel_ms_min": float(np.min(kms)),
                     "device_wall_ms": float(np.median(wall)), "fma": fma, "bound_ms": fma / PEAK_FMA * 1e3,
                     "frac_of_bound": fma / PEAK_FMA * 1e3 / kmed, "host_read_ms": read_ms, "host_acor_ms": acor_ms,
                     "host_walkers_timed": hw, "ratio": (read_ms + acor_ms) / kmed, "reps": args.reps}
                print(json.dumps(c), flush=True)
                cases.append(c)
    doc = {"what": "chain diagnostics: device (lf_chain_diag) against chain read-back + integrated_time on the host",
           "device": torch.cuda.get_device_name(0), "peak_fma_per_s": PEAK_FMA, "cases": cases}
    if args.out:
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
