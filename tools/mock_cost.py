"""Cost of mock catalogues (lf_mock_*, csrc/lf_mock.h) on one MI355X, and of the NumPy twin.

Cases: one mock of ~10^6 expected sources (lf_mock_counts + lf_mock_draw, as MockGenerator.draw makes them) for FREE at
S = 101 and ZEVOL at S = 201; lf_mock_hist for R = 200 posterior-like rows of ~10^6 sources each (2 x 10^8 draws).
Device figures: hipEvents (torch.cuda.Event on the null stream the library launches on) around each synchronous call -
they include the calls' small host <-> device copies, and for draw the 20 MB copy of the sources back to the host.  Host
figures: wall time of MockTwin for the same cases; for hist, `--host-rows` rows (default 2) scaled to R = 200.
Prints one JSON line at the end and writes it to --out when given.

    python tools/mock_cost.py [--reps 10] [--host-rows 2] [--out profiles/r06_mock_cost.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

import lf_testlib as T                # noqa: E402
from lumfuncmcmc_amd import mock, synth   # noqa: E402


def _rows(tw, variant, R, target, seed):
    th = synth.walkers(variant, R, seed=seed)
    phi = [3, 4, 5] if variant == "zevol" else [1]
    m = tw.means(th).sum(axis=1)
    th[:, phi] += np.log10(target / m)[:, None]
    return th


def _events(fn, reps):
    import torch
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append((a.elapsed_time(b), (time.perf_counter() - t0) * 1e3))
    ev, wall = np.array(out).T
    return {"event_ms_median": float(np.median(ev)), "event_ms_min": float(ev.min()), "wall_ms_median": float(np.median(wall)),
            "reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host-rows", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    torch.cuda.init()
    res = {"device": torch.cuda.get_device_name(0), "cases": {}}
    for variant, S in (("free", 101), ("zevol", 201)):
        inp = T.make_inputs(variant, 2000, S=S)
        tw, gen = mock.MockTwin(inp), mock.MockGenerator(inp)
        th = _rows(tw, variant, 1, 1.0e6, seed=3)
        gen.draw(th, 1)                                       # warm-up (first launch, allocations)
        n = int(gen.counts(th, 7)[1].sum())
        dev = _events(lambda: gen.draw(th, 7), a.reps)
        t0 = time.perf_counter()
        tw.draw(th, 7)
        host_ms = (time.perf_counter() - t0) * 1e3
        res["cases"]["draw_%s_S%d" % (variant, S)] = {"sources": n, "device": dev, "host_twin_ms": host_ms}
        print(variant, S, "draw", n, dev, "twin %.0f ms" % host_ms, flush=True)
        if variant == "zevol":
            R = 200
            rows = _rows(tw, variant, R, 1.0e6, seed=11)
            edges = np.linspace(float(inp["logL"].min()), 43.5, 21)
            gen.hist(rows[:2], edges, 1)
            h = gen.hist(rows, edges, 5)
            dev = _events(lambda: gen.hist(rows, edges, 5), max(3, a.reps // 3))
            hr = max(1, a.host_rows)
            t0 = time.perf_counter()
            tw.hist(rows[:hr], edges, 5)
            host_ms = (time.perf_counter() - t0) * 1e3 * R / hr
            res["cases"]["hist_%s_S%d_R%d" % (variant, S, R)] = {"sources": int(h.sum()), "device": dev,
                                                                 "host_twin_ms_scaled": host_ms, "host_rows_timed": hr}
            print(variant, S, "hist R=%d" % R, int(h.sum()), dev, "twin %.0f ms (scaled from %d rows)" % (host_ms, hr), flush=True)
        gen.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
