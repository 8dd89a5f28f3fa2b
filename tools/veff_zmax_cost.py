"""Cost of z_max per source and draw in the marginalised 1/Veff points (lf_veff_draws_zmax).

Per (N, R), with nbin bins and the synthetic catalogue's five fields, min_comp_frac = 0.5:
  * stage 1 (the per-chunk sums, hipEvents: lf_veff_draws_ms) of lf_veff_draws_zmax against lf_veff_draws' stage 1 on the same
    catalogue and draws with the volumes at the first draw's cut - the two calls alternate `reps` times in this process after
    one warm-up each; medians with min and max, and their ratio;
  * the whole call (a host clock around it: the sort, the uploads, the three stages, the copies out; the table is built
    before) against the only exact route there was before: per draw max_redshift + comoving_volume on the host, then one
    lf_veff call - timed for `host_draws` draws and scaled to R.
With --shift it also reports, for the seeded synthetic catalogue of --shift-n sources and a chain scattered around the truth
(Flim and alpha_C with sigma 0.1), how far volumes="per_draw" moves the 16 / 50 / 84 % values and var_comp of every bin from
volumes="fixed".  One JSON line per measurement.

    python tools/veff_zmax_cost.py [--sizes 100000,1000000] [--draws 200,4096] [--bins 50] [--reps 5] [--host-draws 3] [--shift [--shift-host]] [--no-cost]
                                   [--out FILE.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def _med(v):
    import numpy as np
    return [round(float(np.median(v)), 4), round(float(min(v)), 4), round(float(max(v)), 4)]


def cost(a, res):
    import numpy as np
    from lumfuncmcmc_amd import capi, hostsetup as hs, synth, veff, voltable
    from lumfuncmcmc_amd.cosmology import cosmo
    roots = hs.completeness_roots(synth.FLIM_LIMS, synth.ALPHA_LIMS, 0.1, 0.5, 41)
    pref0 = sum(synth.OMEGA_0) / hs.SQARCSEC
    rng = np.random.default_rng(1)
    Rmax = max(a.draws)
    draws = np.column_stack([np.clip(rng.normal(f, 0.1, Rmax), *synth.FLIM_LIMS) * 1.0e-17 for f in synth.FLIM] +
                            [np.clip(rng.normal(synth.ALPHA_C, 0.1, Rmax), *synth.ALPHA_LIMS)])
    fmin = roots.ev(draws[:, :5] / 1.0e-17, draws[:, 5][:, None])
    for n in a.sizes:
        cat = synth.catalogue(n, seed=11)
        t = hs.distance_tables(cat["z"], cosmo)
        zmin, zmax = cat["z"].min(), cat["z"].max()
        flux = 10 ** cat["lum"] / (4.0 * np.pi * (hs.MPC_CM * np.asarray(cosmo.luminosity_distance(cat["z"]))) ** 2)
        field = np.repeat(np.arange(5), np.diff(cat["field_ind"]))
        idx = veff.luminosity_bins(cat["lum"], a.bins)[3]
        t0 = time.perf_counter()
        tab = voltable.build(cosmo, t["dVdzf"], zmin, zmax)
        t_table = time.perf_counter() - t0
        dist = veff.source_distance_scale(cat["lum"])
        vol0 = veff.comoving_volume(t["dVdzf"], zmin, np.minimum(zmax, veff.max_redshift(10 ** cat["lum"], fmin[0][field], cosmo)))
        for R in a.draws:
            d, f = draws[:R], fmin[:R]
            D = dist[None, :] / np.sqrt(f[:min(R, 16)][:, field])
            between = float(np.mean((D > tab.d_lo) & (D < tab.d_hi)))
            capi.veff_draws_zmax_device(flux, field, dist, pref0, 0.1, idx, a.bins, d[:2], f[:2], tab)
            capi.veff_draws_device(flux, field, vol0, pref0, 0.1, idx, a.bins, d[:2])
            s_new, s_old, w_new, w_old = [], [], [], []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                capi.veff_draws_zmax_device(flux, field, dist, pref0, 0.1, idx, a.bins, d, f, tab)
                w_new.append(time.perf_counter() - t0)
                s_new.append(capi.veff_draws_ms()[0])
                t0 = time.perf_counter()
                capi.veff_draws_device(flux, field, vol0, pref0, 0.1, idx, a.bins, d)
                w_old.append(time.perf_counter() - t0)
                s_old.append(capi.veff_draws_ms()[0])
            th = []
            for r in range(a.host_draws):
                t0 = time.perf_counter()
                vol = veff.comoving_volume(t["dVdzf"], zmin, np.minimum(zmax, veff.max_redshift(10 ** cat["lum"], f[r][field], cosmo)))
                capi.veff_device(flux, d[r][:5][field], vol, pref0, d[r][5], 0.1, bin_of=idx, nbin=a.bins, nboot=1, boot_idx=None, seed=1,
                                 device=0)
                th.append(time.perf_counter() - t0)
            r = {"N": n, "R": R, "bins": a.bins, "nodes": int(len(tab.rec)), "eps_T": tab.eps, "table_build_s": round(t_table, 3),
                 "pairs_between_the_clamps": round(between, 4),
                 "stage1_zmax_ms_med_min_max": _med(s_new), "stage1_veff_draws_ms_med_min_max": _med(s_old),
                 "stage1_ratio": round(float(np.median(s_new) / np.median(s_old)), 3),
                 "call_zmax_s_med_min_max": _med(w_new), "call_veff_draws_s_med_min_max": _med(w_old),
                 "host_route_s_per_draw": round(float(np.median(th)), 4), "host_route_s_scaled_to_R": round(float(np.median(th)) * R, 2),
                 "host_route_over_call": round(float(np.median(th)) * R / float(np.median(w_new)), 1)}
            print(json.dumps(r), flush=True)
            res.append(r)


def shift(a, res):
    import numpy as np
    from lumfuncmcmc_amd import synth
    from lumfuncmcmc_amd.model import LumFuncMCMC
    cat = synth.catalogue(a.shift_n)
    fi = cat["field_ind"]
    m = LumFuncMCMC(synth.split_fields(cat["z"], fi), lum=synth.split_fields(cat["lum"], fi), lum_e=synth.split_fields(cat["lum_e"], fi),
                    Flim=list(synth.FLIM), alpha=synth.ALPHA_C, Omega_0=list(synth.OMEGA_0), sch_al=synth.SCH_AL,
                    sch_al_lims=synth.SCH_AL_LIMS, Lstar=synth.LSTAR, Lstar_lims=synth.LSTAR_LIMS, phistar=synth.PHISTAR,
                    phistar_lims=synth.PHISTAR_LIMS, Lc=synth.LC, Lh=synth.LH, nwalkers=32, nsteps=10, min_comp_frac=0.5, field_ind=fi,
                    Flim_lims=synth.FLIM_LIMS, alpha_lims=synth.ALPHA_LIMS, nboot=20, nbins=25)
    rng = np.random.default_rng(7)
    th = np.column_stack([rng.normal(42.6, 0.05, 400), rng.normal(-2.1, 0.05, 400), rng.normal(-1.5, 0.05, 400)] +
                         [rng.normal(f, 0.1, 400) for f in synth.FLIM] + [rng.normal(synth.ALPHA_C, 0.1, 400)])
    m.samples = np.column_stack([th, rng.normal(-100.0, 3.0, 400)])
    out = {}
    for v in ("fixed", "per_draw"):
        np.random.seed(2024)
        out[v] = m.veff_percentiles(ndraws=200, device=not a.shift_host, volumes=v)
    f, p = out["fixed"], out["per_draw"]
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(f["percentiles"] > 0, p["percentiles"] / f["percentiles"] - 1.0, 0.0)
        sd = np.where(f["var_comp"] > 0, np.sqrt(p["var_comp"] / f["var_comp"]), 1.0)
    r = {"shift_N": a.shift_n, "draws": 200, "Lavg": [round(float(x), 3) for x in f["Lavg"]],
         "rel_shift_16": [round(float(x), 5) for x in rel[0]], "rel_shift_50": [round(float(x), 5) for x in rel[1]],
         "rel_shift_84": [round(float(x), 5) for x in rel[2]], "sd_comp_ratio": [round(float(x), 4) for x in sd]}
    print(json.dumps(r), flush=True)
    res.append(r)
    m.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="100000,1000000")
    ap.add_argument("--draws", default="200,4096")
    ap.add_argument("--bins", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-draws", type=int, default=3)
    ap.add_argument("--shift", action="store_true")
    ap.add_argument("--shift-n", type=int, default=20000)
    ap.add_argument("--shift-host", action="store_true", help="the shift on the host twin (no GPU needed)")
    ap.add_argument("--no-cost", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    a.sizes = [int(s) for s in a.sizes.split(",")]
    a.draws = [int(s) for s in a.draws.split(",")]
    res = []
    if not a.no_cost:
        cost(a, res)
    if a.shift:
        shift(a, res)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
