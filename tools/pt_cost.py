"""Cost of the parallel-tempered device sampler at N = 10^6 sources (free completeness).  Prints one
JSON line and writes it to --out.

   python tools/pt_cost.py [--n 1000000] [--steps 40] [--out profiles/r05_pt_cost.json]

For T x W in {1024, 2048} walkers (T = 8 temperatures): evaluations per second of a running chain (T W per step; 60 steps
of burn-in first, then `steps` steps, wall time between two synchronisations), against back-to-back lf_lnprob_batch_device
calls on T W / 2-row blocks of the chain's own positions (2 `steps` calls, the same number of rows).  The swap kernel's
per-step cost comes from a rocprofv3 kernel trace of this script (lf_pt_swap's mean duration)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from lumfuncmcmc_amd import synth                              # noqa: E402
from lumfuncmcmc_amd.capi import LFContext                     # noqa: E402
from lumfuncmcmc_amd.sampler import DevicePTSampler, geometric_betas     # noqa: E402
from lf_testlib import make_inputs                             # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--ntemps", type=int, default=8)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    ctx = LFContext(make_inputs("free", args.n, seed=20241016))
    T, K = args.ntemps, args.steps
    res = {"n": args.n, "variant": "free", "ntemps": T, "steps": K, "cases": []}
    for TW in (1024, 2048):
        W = TW // T
        pt = DevicePTSampler(ctx, T, W, betas=geometric_betas(T, 1e3), seed=5, capacity=60 + K)
        pt.run_mcmc(synth.walkers("free", TW, seed=6).reshape(T, W, ctx.ndim), 60)
        t0 = time.perf_counter()
        pt.enqueue(None, K)
        pos, _, _ = pt.sync()
        dt = time.perf_counter() - t0
        swaps = pt.tswap_acceptance_fraction.tolist()
        pt.close()
        th = torch.from_numpy(np.ascontiguousarray(pos.reshape(TW, ctx.ndim))).cuda()
        halves = [th[:TW // 2].contiguous(), th[TW // 2:].contiguous()]
        out = torch.empty(TW // 2, dtype=torch.float64, device=th.device)
        for i in range(10):
            ctx.lnprob_torch(halves[i & 1], out)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for i in range(2 * K):
            ctx.lnprob_torch(halves[i & 1], out)
        torch.cuda.synchronize()
        db = time.perf_counter() - t1
        chain_rate, plain_rate = TW * K / dt, TW * K / db
        res["cases"].append({"T": T, "W": W, "rows_per_half": TW // 2, "pt_evals_per_s": chain_rate,
                             "pt_ms_per_step": dt / K * 1e3, "plain_evals_per_s": plain_rate,
                             "plain_ms_per_two_blocks": db / K * 1e3, "ratio": chain_rate / plain_rate,
                             "tswap_acceptance": swaps})
    ctx.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
