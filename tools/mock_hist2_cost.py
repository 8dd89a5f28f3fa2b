"""Cost of the mocks binned in redshift and luminosity (lf_mock_hist2; csrc/lf_mock_hist2.h) beside the
histogram in luminosity alone (lf_mock_hist, the same rows and seed) and beside the only other way to the same numbers: draw
every source, copy it to the host and call np.histogram2d there.  One MI355X, one process.

One box: ZEVOL at S = 201, R = 200 posterior-like rows, the default grid of posterior_predictive(z_edges="auto") - 10 bins in
redshift, 20 in logL - and expected counts of 10^5 and 10^6 sources per replicate.  Per size: hist2, then hist, alternating
`reps` times between hipEvents (tools/mock_noise_cost.py: _pair; the calls are synchronous, the events sit on the null stream
the library launches on), then the draw path on `--draw-rows` of the rows (every source is 24 bytes on the host: all 200 rows
of 10^6 sources would be 4.8 GB), by a host clock, scaled to R rows.  The two histograms are checked against each other
(marginal over redshift) and against the draw path's on the rows it ran.  Prints one JSON line and writes it to --out.

    python tools/mock_hist2_cost.py [--reps 5] [--rows 200] [--draw-rows 8] [--sizes 100000,1000000] [--out profiles/mock_hist2_cost.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import lf_testlib as T                # noqa: E402
from lumfuncmcmc_amd import mock      # noqa: E402
from mock_cost import _rows           # noqa: E402
from mock_noise_cost import _pair     # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rows", type=int, default=200)
    ap.add_argument("--draw-rows", type=int, default=8)
    ap.add_argument("--sizes", default="100000,1000000")
    ap.add_argument("--variant", default="zevol")
    ap.add_argument("--S", type=int, default=201)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    torch.cuda.init()
    res = {"device": torch.cuda.get_device_name(0), "variant": a.variant, "S": a.S, "rows": a.rows, "cases": {}}
    inp = T.make_inputs(a.variant, 2000, S=a.S)
    tw, gen = mock.MockTwin(inp), mock.MockGenerator(inp)
    zarr = np.asarray(inp["zarr"], dtype=np.float64)
    ze, e = np.linspace(zarr[0], zarr[-1], 11), np.linspace(41.6, 43.6, 21)
    res["nz"], res["nl"] = ze.size - 1, e.size - 1
    for n in [int(s) for s in a.sizes.split(",")]:
        th = _rows(tw, a.variant, a.rows, float(n), seed=3)
        few = th[:a.draw_rows]
        h2, h1 = gen.hist2(th, ze, e, 1), gen.hist(th, e, 1)                     # warm-up of both shapes; the check
        assert np.array_equal(h2.sum(axis=2), h1)
        two, one, ratio = _pair(lambda: gen.hist2(th, ze, e, 1), lambda: gen.hist(th, e, 1), a.reps)     # ratio: hist / hist2
        tdraw = []
        for _ in range(max(1, min(a.reps, 3))):
            t0 = time.perf_counter()
            z, L, fld, off = gen.draw(few, 1)
            got = np.empty((len(few), gen.nf, ze.size + 1, e.size + 1), dtype=np.int64)
            zb, eb = np.concatenate([[-np.inf], ze, [np.inf]]), np.concatenate([[-np.inf], e, [np.inf]])
            for s in range(len(off) - 1):
                got[s // gen.nf, s % gen.nf] = np.histogram2d(z[off[s]:off[s + 1]], L[off[s]:off[s + 1]], bins=(zb, eb))[0]
            tdraw.append(time.perf_counter() - t0)
        # (np.histogram2d closes its last bin on the right; no source sits at +inf, so the slots are bin_sources2's)
        assert np.array_equal(got, h2[:len(few)])
        scale = a.rows / float(len(few))
        res["cases"]["n%d" % n] = {
            "sources": int(h1.sum()), "hist2": two, "hist": one, "hist2_over_hist": 1.0 / ratio,
            "draw_copy_histogram2d_ms_scaled": 1.0e3 * float(np.median(tdraw)) * scale, "draw_rows_timed": len(few),
            "draw_path_over_hist2": 1.0e3 * float(np.median(tdraw)) * scale / two["event_ms_median"]}
    gen.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
