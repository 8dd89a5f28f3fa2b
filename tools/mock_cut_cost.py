"""Cost of the cut process's mocks (lf_mock_hist_cut, lf_mock_draw_cut; csrc/lf_mock_cut.h) beside the
observation step without the cut (lf_mock_hist_err, lf_mock_draw_err), on one MI355X and in one process.

Cases: grids with their own lower edge per redshift column (tests/lf_cutlib.cut_inputs) for FREE at S = 101 and ZEVOL at S = 201,
R = 200 rows of ~10^5 expected sources above the edge each - hist_noisy beside hist_cut - and one row of ~10^6 - draw_noisy
beside draw_cut (counts, draw, the copy of the candidates to the host and the compaction there included).  Constant error
models of 0.09 and 0.30 dex: the band is 7.5 sigma deep, so they bound the band's share of the candidates.  Every call sits
between hipEvents (torch.cuda.Event on the null stream the library launches on); medians over --reps calls, the two calls of a
pair alternating (tools/mock_noise_cost.py: _pair).  Also printed: the band's candidates per source scattered in.
Prints one JSON line at the end and writes it to --out when given.

    python tools/mock_cut_cost.py [--reps 10] [--out profiles/mock_cut_cost.json]
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

import lf_cutlib as C                 # noqa: E402
from lumfuncmcmc_amd import mock      # noqa: E402
from mock_cost import _rows           # noqa: E402
from mock_noise_cost import _pair     # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    torch.cuda.init()
    res = {"device": torch.cuda.get_device_name(0), "cases": {}}
    edges = np.linspace(40.5, 44.5, 41)
    for variant, S in (("free", 101), ("zevol", 201)):
        inp = C.cut_inputs(variant, n=2000, S=S, nf=5)
        tw, gen = mock.MockTwin(inp), mock.MockGenerator(inp)
        for sg in (0.09, 0.30):
            nodes, sig = C.const_model(sg, nf=5)
            gen.set_error_model(nodes, sig)
            lb = mock.band_grid(inp, mock.cut_depth(sig))
            gen.set_cut_band(lb, None if variant == "free" else mock.band_integ_part(inp, lb))
            many, one = _rows(tw, variant, 200, 1.0e5, seed=3), _rows(tw, variant, 1, 1.0e6, seed=3)
            info = gen.draw_cut(one, 1)[6]                      # warm-up of every shape timed below
            gen.draw_noisy(one, 1), gen.hist_noisy(many, edges, 1), gen.hist_cut(many, edges, 1)
            h = _pair(lambda: gen.hist_noisy(many, edges, 1), lambda: gen.hist_cut(many, edges, 1), a.reps)
            d = _pair(lambda: gen.draw_noisy(one, 1), lambda: gen.draw_cut(one, 1), a.reps)
            res["cases"]["%s_S%d_sigma%.2f" % (variant, S, sg)] = {
                "hist_noisy": h[0], "hist_cut": h[1], "hist_ratio": h[2], "draw_noisy": d[0], "draw_cut": d[1], "draw_ratio": d[2],
                "candidates": [int(v) for v in info["n_cand"].sum(axis=(0, 1))], "kept": int(info["kept"].sum()),
                "band_candidates_per_source_scattered_in": float(info["n_cand"][..., 1].sum() / max(int(info["n_scattered_in"].sum()), 1))}
        gen.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
