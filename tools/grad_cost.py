"""Device time of one gradient batch (lf_lnprob_grad_batch_device) next to one plain lnprob evaluation of the same rows, with
hipEvents (torch.cuda.Event) around `reps` back-to-back calls each; the gradient call includes its own lnprob evaluation.

    python tools/grad_cost.py [--rows 128] [--reps 20] [--sizes 1000000,100000] [--out FILE.json]

Prints one JSON line per (variant, N): us per call of each and their ratio."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=128)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sizes", default="1000000,100000")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from lf_testlib import make_inputs
    from lumfuncmcmc_amd import capi, synth
    res = []
    for variant in ("free", "zevol"):
        for n in (int(s) for s in a.sizes.split(",")):
            inp = make_inputs(variant, n, seed=1)
            ctx = capi.LFContext(inp, device=0)
            th = torch.from_numpy(synth.walkers(variant, a.rows, seed=2)).cuda()

            def timed(fn):
                for _ in range(3):
                    fn()
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.reps):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                return e0.elapsed_time(e1) * 1e3 / a.reps

            us_lnprob = timed(lambda: ctx.lnprob_torch(th))
            us_grad = timed(lambda: ctx.lnprob_grad_torch(th))
            ctx.close()
            r = {"variant": variant, "N": n, "rows": a.rows, "lnprob_us": round(us_lnprob, 2), "grad_us": round(us_grad, 2),
                 "ratio": round(us_grad / us_lnprob, 2)}
            print(json.dumps(r), flush=True)
            res.append(r)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
