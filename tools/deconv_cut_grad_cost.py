"""Device time of the cut's gradient (csrc/lf_deconv_cut_grad.h): one convolved value-and-gradient batch
(lf_lnprob_err_grad_batch_device, option "deconv_cut_grad" = 1) on a context whose grid has its own luminosity nodes per
column, with the cut model's tables and with a cut model of sigma = 0 (no tables: nothing of lf_deconv_cut.h or
lf_deconv_cut_grad.h is launched).  Three warm-up calls, then hipEvents (torch.cuda.Event) on the stream around every single
call, the median of `reps` calls, the two contexts alternated call by call in one process.  The launches of one call run one
after the other on one stream, so the time of the cut's kernels - the value's lf_deconv_cut_part and the gradient's two - is
the difference of the two medians; the value's share is tools/deconv_cut_cost.py's figure.

    python tools/deconv_cut_grad_cost.py [--rows 128] [--reps 21] [--nsrc 100000] [--size-ln 101] [--out profiles/deconv_cut_grad_cost.json]

One child process per variant, each under its own time limit; the first that fails ends the run.  One JSON line per variant."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

VARIANTS = ("free", "fixcomp", "zevol")


def child(a):
    import numpy as np
    import torch
    import lf_cutlib
    from lumfuncmcmc_amd import capi, deconv, synth
    torch.set_num_threads(1)
    K, nf = deconv.DEFAULT_ORDER, 5
    inp = lf_cutlib.cut_inputs(a.child, n=a.nsrc, S=a.size_ln, nf=nf, seed=1)
    sigma = np.random.default_rng(3).uniform(0.0, deconv.SIGMA_MAX, a.nsrc)
    model = lf_cutlib.flux_model(0.09, nf=nf)
    th = torch.from_numpy(synth.walkers(a.child, a.rows, seed=2)).cuda()
    ctx = {}
    for name, m in (("without", lf_cutlib.const_model(0.0, nf=nf)), ("with", model)):
        c = capi.LFContext(inp, device=0)
        c.set_cut_error_model(*m)
        c.set_lum_err(sigma, K)
        c.set_option("deconv_cut_grad", 1)
        ctx[name] = c
    info = ctx["with"].cut_info()
    assert ctx["without"].cut_info()["chunks"] == 0 and info["chunks"] > 0

    def event_us(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3

    for c in ctx.values():
        for _ in range(3):
            c.lnprob_err_grad_torch(th)
            c.lnprob_err_torch(th)
    torch.cuda.synchronize()
    t = {"without": [], "with": [], "value_without": [], "value_with": []}
    for _ in range(a.reps):
        for name in ("without", "with"):
            t[name].append(event_us(lambda: ctx[name].lnprob_err_grad_torch(th)))
        for name in ("without", "with"):
            t["value_" + name].append(event_us(lambda: ctx[name].lnprob_err_torch(th)))
    q = {k: [float(x) for x in np.percentile(v, [25, 50, 75])] for k, v in t.items()}
    own = q["with"][1] - q["without"][1]
    value = q["value_with"][1] - q["value_without"][1]
    r = {"variant": a.child, "N": a.nsrc, "rows": a.rows, "K": K, "fields": nf, "size_ln": a.size_ln, "reps": a.reps,
         "cut_nodes_per_row": int(info["nnodes"].sum()), "cut_blocks_per_row": int(info["chunks"]),
         "delta_node_terms_per_row": int(np.count_nonzero(sigma > 0.0)) * K,
         "grad_call_without_cut_us": [round(x, 2) for x in q["without"]], "grad_call_with_cut_us": [round(x, 2) for x in q["with"]],
         "cut_kernels_us": round(own, 2), "cut_share_of_call": round(own / q["with"][1], 4),
         "value_call_cut_kernel_us": round(value, 2), "cut_grad_kernels_us": round(own - value, 2)}
    for c in ctx.values():
        c.close()
    print(json.dumps(r), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=128)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--nsrc", type=int, default=100000)
    ap.add_argument("--size-ln", type=int, default=101)
    ap.add_argument("--limit-s", type=int, default=240, help="time limit of one variant's child process")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, choices=VARIANTS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    res = []
    for v in VARIANTS:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", v, "--rows", str(a.rows), "--reps", str(a.reps),
               "--nsrc", str(a.nsrc), "--size-ln", str(a.size_ln)]
        p = subprocess.run(cmd, timeout=a.limit_s, capture_output=True, text=True)       # (a timeout or a failure ends the run)
        if p.returncode != 0:
            sys.stderr.write(p.stdout + p.stderr)
            sys.exit("deconv_cut_grad_cost: the %s step ended with status %d: nothing more is started" % (v, p.returncode))
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1]
        print(line, flush=True)
        res.append(json.loads(line))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
