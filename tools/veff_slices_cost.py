"""Device time of the sliced 1/Veff bootstrap (lf_veff_slices) next to the unsliced lf_veff.

Per catalogue size N (synth.catalogue, five fields), with S equal-count redshift slices, nbin luminosity bins and nboot
resamples:
  * lf_veff_slices: the device time of its two kernels (veffs_partial + veffs_reduce, hipEvents: lf_veff_slices_ms) and the
    whole call (a host clock around it: the sort, the uploads, the weights, the kernels, the copies out);
  * lf_veff on the same catalogue, bins and resample count: the whole call only - it has no device timer, and its kernels are
    timed here by the difference between a call with nboot resamples and one with nbin = 0 (weights and copies alone), both on
    the host clock; what is compared with lf_veff_slices_ms is that difference.
The two alternate `reps` times in this process after one warm-up each; medians with min and max, and the ratios.  One JSON
line per size.

    python tools/veff_slices_cost.py [--sizes 100000,1000000] [--slices 5] [--bins 25] [--nboot 100] [--reps 7] [--out FILE.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _med(v):
    import numpy as np
    return [round(float(np.median(v)), 4), round(float(min(v)), 4), round(float(max(v)), 4)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="100000,1000000")
    ap.add_argument("--slices", type=int, default=5)
    ap.add_argument("--bins", type=int, default=25)
    ap.add_argument("--nboot", type=int, default=100)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import numpy as np
    from lumfuncmcmc_amd import capi, hostsetup as hs, synth, veff
    from lumfuncmcmc_amd.cosmology import cosmo
    pref0 = sum(synth.OMEGA_0) / hs.SQARCSEC
    res = []
    for n in [int(s) for s in a.sizes.split(",")]:
        cat = synth.catalogue(n, seed=11)
        t = hs.distance_tables(cat["z"], cosmo)
        zmin, zmax = cat["z"].min(), cat["z"].max()
        flux = 10 ** cat["lum"] / (4.0 * np.pi * (hs.MPC_CM * np.asarray(cosmo.luminosity_distance(cat["z"]))) ** 2)
        flim = 1.0e-17 * np.repeat(synth.FLIM, np.diff(cat["field_ind"]))
        idx = veff.luminosity_bins(cat["lum"], a.bins)[3]
        edges = veff.slice_edges(cat["z"], a.slices)
        so = veff.slice_index(cat["z"], edges)
        vol = veff.slice_volumes(t["dVdzf"], edges, so, zmax)
        vol_all = float(veff.comoving_volume(t["dVdzf"], zmin, zmax))

        def sliced():
            t0 = time.perf_counter()
            capi.veff_slices(flux, flim, vol, pref0, synth.ALPHA_C, synth.FCMIN, so, a.slices, idx, a.bins, nboot=a.nboot, seed=7)
            return time.perf_counter() - t0, capi.veff_slices_ms()

        def plain(nbin):
            t0 = time.perf_counter()
            capi.veff_device(flux, flim, vol_all, pref0, synth.ALPHA_C, synth.FCMIN, bin_of=idx if nbin else None, nbin=nbin,
                             nboot=a.nboot if nbin else 0, seed=7)
            return time.perf_counter() - t0

        sliced(), plain(a.bins), plain(0)
        w_new, k_new, w_old, w_base = [], [], [], []
        for _ in range(a.reps):
            w, k = sliced()
            w_new.append(w), k_new.append(k)
            w_old.append(plain(a.bins))
            w_base.append(plain(0))
        k_old = [1.0e3 * (x - y) for x, y in zip(w_old, w_base)]
        r = {"N": n, "slices": a.slices, "bins": a.bins, "nboot": a.nboot, "reps": a.reps, "gathers": int((so >= 0).sum()) * a.nboot,
             "veff_slices_kernels_ms_med_min_max": _med(k_new), "veff_slices_call_s_med_min_max": _med(w_new),
             "veff_call_s_med_min_max": _med(w_old), "veff_bins_ms_by_difference_med_min_max": _med(k_old),
             "kernels_ratio_slices_over_veff": round(float(np.median(k_new) / np.median(k_old)), 3),
             "call_ratio_slices_over_veff": round(float(np.median(w_new) / np.median(w_old)), 3)}
        print(json.dumps(r), flush=True)
        res.append(r)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
