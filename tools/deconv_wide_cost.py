"""Device time of the wide rule's kernel (csrc/lf_deconv_wide.h) next to lf_deconv_part's, from one run:
a catalogue of which the stated share of sources has sigma above the order's limit (uniform up to 0.30 dex), the others at or
below it.  Three calls are alternated, each between hipEvents on the stream, the median over `reps`:

    plain     lf_lnprob_batch_device
    narrow    lf_lnprob_err_batch_device with the wide sources' sigma set to 0 and the option off
    both      lf_lnprob_err_batch_device with the option on: the same narrow launches (the narrow kernel finds sigma = 0 for the
              wide sources either way) plus lf_deconv_wide_part

so narrow - plain is lf_deconv_part's time over the narrow sources (K = 32 node terms each) and both - narrow is
lf_deconv_wide_part's over the wide ones (48 to 144 node terms each, by class).  One JSON line per (variant, N).

    python tools/deconv_wide_cost.py [--rows 128] [--reps 21] [--sizes 1000000,100000] [--share 0.2] [--out FILE.json]"""
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
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--sizes", default="1000000,100000")
    ap.add_argument("--share", type=float, default=0.2)
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
    K = deconv.DEFAULT_ORDER
    nodes = np.array([p * deconv.WIDE_NPANEL for p in deconv.WIDE_PANELS])
    for variant in ("free", "zevol"):
        for n in (int(s) for s in a.sizes.split(",")):
            inp = make_inputs(variant, n, seed=1)
            rng = np.random.default_rng(3)
            sigma = rng.uniform(0.0, deconv.SIGMA_MAX, n)
            wide = rng.random(n) < a.share
            sigma[wide] = rng.uniform(np.nextafter(deconv.SIGMA_MAX, 1.0), deconv.WIDE_SIGMA_MAX, int(wide.sum()))
            cls = deconv.wide_class(sigma, K)
            terms_wide = int(nodes[cls[cls >= 0]].sum())
            terms_narrow = int(((cls < 0) & (sigma > 0.0)).sum()) * K
            th = torch.from_numpy(synth.walkers(variant, a.rows, seed=2)).cuda()
            ctx_n, ctx_b = capi.LFContext(inp, device=0), capi.LFContext(inp, device=0)
            ctx_n.set_lum_err(np.where(wide, 0.0, sigma), K)
            ctx_b.set_lum_err(sigma, K, wide=True)
            calls = {"plain": lambda: ctx_n.lnprob_torch(th), "narrow": lambda: ctx_n.lnprob_err_torch(th),
                     "both": lambda: ctx_b.lnprob_err_torch(th)}
            for _ in range(3):
                for fn in calls.values():
                    fn()
            torch.cuda.synchronize()
            t = {k: [] for k in calls}
            for _ in range(a.reps):
                for k, fn in calls.items():
                    t[k].append(event_us(fn))
            med = {k: float(np.median(v)) for k, v in t.items()}
            t_narrow, t_wide = med["narrow"] - med["plain"], med["both"] - med["narrow"]
            r = {"variant": variant, "N": n, "rows": a.rows, "K": K, "share_wide": round(float(wide.mean()), 4),
                 "median_us": {k: round(v, 2) for k, v in med.items()},
                 "narrow_us": round(t_narrow, 2), "wide_us": round(t_wide, 2),
                 "narrow_node_terms": terms_narrow * a.rows, "wide_node_terms": terms_wide * a.rows,
                 "mean_nodes_per_wide_source": round(terms_wide / max(1, int(wide.sum())), 2),
                 "narrow_terms_per_s": round(terms_narrow * a.rows / (t_narrow * 1e-6), 1) if t_narrow > 0 else None,
                 "wide_terms_per_s": round(terms_wide * a.rows / (t_wide * 1e-6), 1) if t_wide > 0 else None}
            r["wide_over_narrow_rate"] = (round(r["wide_terms_per_s"] / r["narrow_terms_per_s"], 4)
                                          if r["narrow_terms_per_s"] and r["wide_terms_per_s"] else None)
            print(json.dumps(r), flush=True)
            res.append(r)
            ctx_n.close()
            ctx_b.close()
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
