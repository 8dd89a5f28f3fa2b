"""Cost of the mocks' observation step (lf_mock_draw_err, lf_mock_hist_err; csrc/lf_mock_noise.h)
beside the noiseless kernels, on one MI355X and in one process.

Cases (the sizes of section 3.11 and tools/mock_cost.py): one mock of ~10^6 expected sources for FREE at S = 101 and ZEVOL at
S = 201 - MockGenerator.draw beside draw_noisy (counts + draw, the copy of the sources to the host included: 20 MB without,
36 MB with the two extra columns); R = 200 rows of ~10^6 sources each for ZEVOL - hist beside hist_noisy.  Every call sits
between hipEvents (torch.cuda.Event on the null stream the library launches on); medians over --reps calls, the two kernels
of a pair alternating.  The error model has 16 nodes across the mock's own fluxes, sigma 0.05 .. 0.4 dex.
Prints one JSON line at the end and writes it to --out when given.

    python tools/mock_noise_cost.py [--reps 10] [--out profiles/mock_noise_cost.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import lf_testlib as T                # noqa: E402
from lumfuncmcmc_amd import mock      # noqa: E402
from mock_cost import _events, _rows  # noqa: E402


def _pair(plain, noisy, reps):
    """the two calls alternating, `reps` of each: (plain figures, noisy figures, ratio of the event medians)"""
    a, b = [], []
    for _ in range(reps):
        a.append(_events(plain, 1))
        b.append(_events(noisy, 1))
    fold = lambda v: {"event_ms_median": float(np.median([x["event_ms_median"] for x in v])),                 # noqa: E731
                      "event_ms_min": float(np.min([x["event_ms_min"] for x in v])),
                      "wall_ms_median": float(np.median([x["wall_ms_median"] for x in v])), "reps": reps}
    fa, fb = fold(a), fold(b)
    return fa, fb, fb["event_ms_median"] / fa["event_ms_median"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    torch.cuda.init()
    res = {"device": torch.cuda.get_device_name(0), "cases": {}}
    for variant, S in (("free", 101), ("zevol", 201)):
        inp = T.make_inputs(variant, 2000, S=S)
        tw, gen = mock.MockTwin(inp), mock.MockGenerator(inp)
        th = _rows(tw, variant, 1, 1.0e6, seed=3)
        z, L, _, _ = gen.draw(th, 1)                          # warm-up; its fluxes place the nodes
        t = mock.log_flux(tw.zarr, mock.ld2_nodes(inp["DL_zarr"]), z, L)
        nodes = np.linspace(*np.quantile(t, (0.05, 0.95)), 16)
        sig = np.repeat(np.linspace(0.4, 0.05, 16)[None], gen.nf, axis=0)
        gen.set_error_model(nodes, sig)
        gen.draw_noisy(th, 1)
        n = int(gen.counts(th, 7)[1].sum())
        p, q, ratio = _pair(lambda: gen.draw(th, 7), lambda: gen.draw_noisy(th, 7), a.reps)
        res["cases"]["draw_%s_S%d" % (variant, S)] = {"sources": n, "lf_mock_draw": p, "lf_mock_draw_err": q, "ratio": ratio}
        print(variant, S, "draw", n, p, q, "ratio %.3f" % ratio, flush=True)
        if variant == "zevol":
            R = 200
            rows = _rows(tw, variant, R, 1.0e6, seed=11)
            edges = np.linspace(float(inp["logL"].min()), 43.5, 21)
            gen.hist(rows[:2], edges, 1)
            gen.hist_noisy(rows[:2], edges, 1)
            h = gen.hist(rows, edges, 5)
            p, q, ratio = _pair(lambda: gen.hist(rows, edges, 5), lambda: gen.hist_noisy(rows, edges, 5), max(3, a.reps // 3))
            res["cases"]["hist_%s_S%d_R%d" % (variant, S, R)] = {"sources": int(h.sum()), "lf_mock_hist": p, "lf_mock_hist_err": q,
                                                                 "ratio": ratio}
            print(variant, S, "hist R=%d" % R, int(h.sum()), p, q, "ratio %.3f" % ratio, flush=True)
        gen.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
