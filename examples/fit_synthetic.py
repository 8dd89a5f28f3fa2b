#!/usr/bin/env python
"""End to end on the MI355X path, the way run_lumfuncmcmc.py drives the reference
(run_lumfuncmcmc.py:230-323), without astropy / emcee / corner:

    catalogue file -> per-field lists -> LumFuncMCMC -> fit_model (device-resident sampler)
    -> set_median_fit (median LF + 1/Veff estimate) -> the reference's output tables.

    python examples/fit_synthetic.py [--nsrc 20000] [--nwalkers 64] [--nsteps 300] [--fix-comp] [--until-converged] [--map]
                                     [--integrals] [--pt] [--deconvolve [--deconvolve-tile] [--deconvolve-wide] [--deconvolve-cut] [--deconvolved-lums FILE]]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from lumfuncmcmc_amd import synth, tableio                      # noqa: E402
from lumfuncmcmc_amd.cosmology import cosmo                     # noqa: E402
from lumfuncmcmc_amd.model import LumFuncMCMC                   # noqa: E402


def write_catalogue(path, n, seed):
    """A synthetic catalogue in the driver's input format (Field, ID, z, OIII_flux, OIII_flux_e)."""
    cat = synth.catalogue(n, seed=seed)
    dl = cosmo.luminosity_distance(cat["z"])
    flux17 = 10 ** cat["lum"] / (4.0 * np.pi * (dl * 3.086e24) ** 2) / 1.0e-17
    names = np.array(["AEGIS", "COSMOS", "GOODSN", "GOODSS", "UDS"])
    field = np.concatenate([np.full(int(cat["field_ind"][f + 1] - cat["field_ind"][f]), names[f]) for f in range(5)])
    with open(path, "w") as f:
        f.write("Field ID z OIII_flux OIII_flux_e\n")
        for i in range(n):
            f.write("%s %d %r %r %r\n" % (field[i], i, float(cat["z"][i]), float(flux17[i]), float(0.1 * flux17[i])))


def write_integrals(LFmod, path):
    """The 16 / 50 / 84 % posterior values of n(>Lc) and rho(>Lc) (lf_integrals): one row, or for the
    z-evolving model one row per z of lf_integrals's default mesh."""
    cols, labels = [], []
    if hasattr(LFmod, "z1"):
        cols.append(np.linspace(LFmod.zmin, LFmod.zmax, 100))
        labels.append("z")
    for kind, name in (("number", "n"), ("lumdens", "rho")):
        np.random.seed(4)                                    # the same draws for both kinds
        band = LFmod.lf_integrals(kind=kind)
        cols += list(band)
        labels += ["%s_gt_Lc_%02d" % (name, p) for p in (16, 50, 84)]
    tableio.write_fixed_width_two_line(path, cols, labels, formats={l: ("%0.4f" if l == "z" else "%0.6e") for l in labels})


def write_veff_band(LFmod, path, volumes="fixed"):
    """The 1/Veff points with the band the completeness posterior gives them (veff_percentiles) next
    to the bootstrap error of the catalogue alone.  volumes "per_draw": z_max per source and draw (section 3.29)."""
    np.random.seed(4)
    band = LFmod.veff_percentiles(percentiles=(16, 50, 84), volumes=volumes)
    labels = ["Luminosity", "BinLF", "BinLFErr", "BinLF_16", "BinLF_50", "BinLF_84", "BinLFErrComp"]
    tableio.write_fixed_width_two_line(path, [band["Lavg"], LFmod.lfbinorig, np.sqrt(LFmod.var)] + list(band["percentiles"]) +
                                       [np.sqrt(band["var_comp"])], labels)


def write_veff_slices(LFmod, out, tag, S):
    """The 1/Veff points of S equal-count redshift slices, one table per slice in VeffLF's format, with the model averaged over
    the slice (veff_slices)"""
    np.random.seed(5)
    res = LFmod.veff_slices(z_edges=S, percentiles=(16, 50, 84))
    labels = ["Luminosity", "BinLF", "BinLFErr", "Model_16", "Model_50", "Model_84"]
    for s in range(S):
        path = os.path.join(out, "VeffLF_%s_z%.3f-%.3f.dat" % (tag, res["z_edges"][s], res["z_edges"][s + 1]))
        tableio.write_fixed_width_two_line(path, [res["Lavg"][s], res["lf"][s], np.sqrt(res["var"][s])] + list(res["model"][:, s]), labels)


def write_deconvolved_lums(LFmod, path):
    """the per-source posterior of the true luminosity (deconvolved_luminosities) as a table, and the mean shift of the faintest
    and the brightest tenth of the catalogue"""
    res = LFmod.deconvolved_luminosities()
    n = len(LFmod.lum)
    tableio.write_fixed_width_two_line(path, [np.arange(n), LFmod.lum, LFmod.lum_e, res["lum_true"], res["lum_true_e"]],
                                       ["ID", "lum", "lum_e", "lum_true", "lum_true_e"],
                                       formats={l: ("%d" if l == "ID" else "%0.5f") for l in ("ID", "lum", "lum_e", "lum_true", "lum_true_e")})
    order = np.argsort(LFmod.lum)
    k = max(1, n // 10)
    print("deconvolved luminosities over %d draws: mean shift %+.4f dex in the faintest tenth, %+.4f dex in the brightest"
          % (res["n_used"], np.mean(res["shift"][order[:k]]), np.mean(res["shift"][order[-k:]])))


def print_veff_deconvolved(LFmod):
    """the deconvolved 1/Veff points (veff_deconvolved) next to the plain ones"""
    np.random.seed(6)
    res = LFmod.veff_deconvolved(percentiles=(16, 50, 84))
    print("1/Veff points over %d draws: Lavg, plain dn/dlogL, deconvolved 16 / 50 / 84 %%" % res["n_used"])
    for b in range(len(res["Lavg"])):
        print("  %8.4f  %12.5e  %12.5e %12.5e %12.5e" % ((res["Lavg"][b], LFmod.lfbinorig[b]) + tuple(res["percentiles"][:, b])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nsrc", type=int, default=20000)
    ap.add_argument("--nwalkers", type=int, default=64)
    ap.add_argument("--nsteps", type=int, default=300)
    ap.add_argument("--fix-comp", action="store_true")
    ap.add_argument("--until-converged", action="store_true",
                    help="run until steps > 50 tau and tau has settled (fit_model_converged, at most 10 x nsteps steps; "
                         "DESIGN.md section 3.12) instead of exactly --nsteps steps")
    ap.add_argument("--map", action="store_true",
                    help="maximum a posteriori fit first (fit_model_map; DESIGN.md section 3.14): prints the best fit with "
                         "sqrt(diag(cov)) next to the medians and the Laplace evidence; with --until-converged the walkers "
                         "start in a Gaussian ball around the maximum")
    ap.add_argument("--integrals", action="store_true",
                    help="also write the 16 / 50 / 84 %% posterior values of the number density n(>Lc) [Mpc^-3] and the "
                         "luminosity density rho(>Lc) [erg s^-1 Mpc^-3] (lf_integrals; DESIGN.md section 3.16)")
    ap.add_argument("--veff-band", action="store_true",
                    help="also write the 1/Veff points with their 16 / 50 / 84 %% band over the completeness posterior and "
                         "sqrt(var_comp) (veff_percentiles; DESIGN.md section 3.17; not with --fix-comp)")
    ap.add_argument("--veff-volumes", choices=("fixed", "per_draw"), default="fixed",
                    help="with --veff-band: the sources' volumes at the current Flim and alpha for every draw (fixed), or out to "
                         "the z_max of each draw's own flux cut (per_draw; DESIGN.md section 3.29)")
    ap.add_argument("--veff-slices", type=int, default=0, metavar="S",
                    help="also write the 1/Veff points of S equal-count redshift slices, one VeffLF table per slice, with the model "
                         "averaged over the slice (veff_slices; DESIGN.md section 3.36)")
    ap.add_argument("--deconvolve", action="store_true",
                    help="fit the likelihood convolved with the catalogue's flux errors (Eddington-bias correction, deconvolve=True; "
                         "DESIGN.md section 3.18; errors above 0.09 dex are refused; --until-converged and --pt run the device "
                         "samplers on the convolved likelihood, DESIGN.md section 3.20, a plain run the host sampler; with --map the "
                         "convolved and the plain maximum are both found and the difference of their L*, the catalogue's Eddington "
                         "shift, is printed; DESIGN.md section 3.19)")
    ap.add_argument("--deconvolve-tile", action="store_true",
                    help="with --deconvolve and --fix-comp: the correction by tiles of rows (deconvolve_tile=True; DESIGN.md section "
                         "3.20; no effect with free completeness)")
    ap.add_argument("--deconvolve-wide", action="store_true",
                    help="with --deconvolve: errors above 0.09 dex, up to 0.30 dex, are integrated by the wide rule instead of "
                         "being refused (deconvolve_wide=True; DESIGN.md section 3.21)")
    ap.add_argument("--deconvolve-cut", action="store_true",
                    help="with --deconvolve: fit at min_comp_frac = 0.5, the classes' default, with the cut on the observed flux "
                         "modelled (deconvolve_cut=True; DESIGN.md section 3.31); with --map the gradient of the cut's term is "
                         "served too (deconvolve_cut_grad=True; DESIGN.md section 3.33) and the convolved and the plain maximum "
                         "are printed side by side, as without the cut; with --veff-deconvolved the points take the catalogued volume per "
                         "node (deconvolve_cut_veff=True; DESIGN.md section 3.34)")
    ap.add_argument("--deconvolved-lums", metavar="FILE", default="",
                    help="with --deconvolve: every source's posterior mean and spread of its TRUE luminosity over 200 posterior "
                         "draws (deconvolved_luminosities; DESIGN.md section 3.22) written to FILE: ID, lum, lum_e, lum_true, "
                         "lum_true_e")
    ap.add_argument("--veff-deconvolved", action="store_true",
                    help="with --deconvolve: print the deconvolved 1/Veff points - the sources' posteriors of the true luminosity "
                         "binned with the completeness at the true flux, 16 / 50 / 84 %% over 200 posterior draws - next to the "
                         "plain ones (veff_deconvolved; DESIGN.md section 3.26)")
    ap.add_argument("--predictive-noise", choices=("none", "catalogue"), default=None,
                    help="posterior predictive check of the luminosity histogram over 200 posterior draws (posterior_predictive; "
                         "DESIGN.md sections 3.11, 3.23), p-values per field printed: `none` bins the replicates' true "
                         "luminosities (the comparison for a plain fit), `catalogue` their observed ones under the catalogue's own "
                         "error model (the comparison for --deconvolve)")
    ap.add_argument("--predictive-z", nargs="?", type=int, const=10, default=None, metavar="NZ",
                    help="the posterior predictive check in redshift as well (posterior_predictive(z_edges=...); DESIGN.md section "
                         "3.35): NZ equal redshift bins over [zmin, zmax] (default 10).  Prints N(z) observed beside the replicates' "
                         "16/50/84 %% band and the deviance p-value per field; with --predictive-cut the replicates are those of the "
                         "cut process, with --predictive-noise their luminosities carry the noise asked for there")
    ap.add_argument("--predictive-cut", action="store_true",
                    help="with --deconvolve-cut: the posterior predictive check against replicates of the cut process the fit "
                         "models - sources scattered in and out across the grid's lower edge included - under the fit's own error "
                         "model (posterior_predictive(cut=True); DESIGN.md section 3.32); the faintest bins are printed as well")
    ap.add_argument("--pt", action="store_true",
                    help="parallel-tempered fit and the evidence by thermodynamic integration (fit_model_pt; DESIGN.md section "
                         "3.10) instead of fit_model")
    ap.add_argument("--out", default="LFMCMCOut")
    ap.add_argument("--compress", action="store_true", help="compressed catalogue and grid (DESIGN.md section 3.5)")
    args = ap.parse_args()
    if args.veff_band and args.fix_comp:
        ap.error("--veff-band needs the completeness parameters in the fit: not with --fix-comp")
    if args.deconvolved_lums and not args.deconvolve:
        ap.error("--deconvolved-lums needs --deconvolve")
    if args.veff_deconvolved and not args.deconvolve:
        ap.error("--veff-deconvolved needs --deconvolve")
    if args.deconvolve_cut and not args.deconvolve:
        ap.error("--deconvolve-cut needs --deconvolve (DESIGN.md section 3.31)")
    if args.pt and args.until_converged:
        ap.error("--pt and --until-converged are two fits: choose one")
    os.makedirs(args.out, exist_ok=True)
    cpath = os.path.join(args.out, "synthetic_catalogue.dat")
    write_catalogue(cpath, args.nsrc, seed=5)

    z, flux, flux_e, field_names, field_ind, _ = tableio.read_input_catalogue(cpath, "OIII", list(synth.FLIM), synth.ALPHA_C)
    t0 = time.time()
    LFmod = LumFuncMCMC(z, flux=flux, flux_e=flux_e, Flim=list(synth.FLIM), alpha=synth.ALPHA_C, line_name="OIII",
                        Omega_0=list(synth.OMEGA_0), nbins=50, nboot=100, sch_al=synth.SCH_AL,
                        sch_al_lims=synth.SCH_AL_LIMS, Lstar=synth.LSTAR, Lstar_lims=synth.LSTAR_LIMS,
                        phistar=synth.PHISTAR, phistar_lims=synth.PHISTAR_LIMS, Lc=synth.LC, Lh=synth.LH,
                        nwalkers=args.nwalkers, nsteps=args.nsteps, fix_sch_al=False, fix_comp=args.fix_comp,
                        min_comp_frac=0.5 if args.deconvolve_cut else 0.0, Flim_lims=synth.FLIM_LIMS, alpha_lims=synth.ALPHA_LIMS,
                        field_names=field_names, field_ind=field_ind, compress=args.compress, deconvolve=args.deconvolve,
                        deconvolve_tile=args.deconvolve_tile, deconvolve_wide=args.deconvolve_wide,
                        deconvolve_cut=args.deconvolve_cut, deconvolve_cut_grad=args.deconvolve_cut and args.map,
                        deconvolve_cut_veff=args.deconvolve_cut and args.veff_deconvolved)
    print("setup %.2f s for %d sources" % (time.time() - t0, len(LFmod.lum)))
    np.random.seed(3)
    plain_map = None
    if args.map and args.deconvolve:
        plain_map = dict(LFmod.fit_model_map(seed=7, likelihood="plain"))
        LFmod.fit_model_map(seed=7, likelihood="convolved")
    elif args.map:
        LFmod.fit_model_map(seed=7)
    like = "convolved" if args.deconvolve else None
    if args.until_converged:
        LFmod.fit_model_converged(start="map" if args.map else "box", likelihood=like)
        print("converged: %s after %d steps; tau per parameter %s" % (LFmod.converged, LFmod.tau_history[-1][0],
                                                                     np.array2string(LFmod.tau_history[-1][1], precision=1)))
    elif args.pt:
        LFmod.fit_model_pt(likelihood=like)
        print("lnZ = %.3f +/- %.3f (thermodynamic integration over %d temperatures)" % (LFmod.lnZ, LFmod.dlnZ, LFmod.pt_sampler.ntemps))
    else:
        LFmod.fit_model()
    LFmod.set_median_fit()

    names = LFmod.get_param_names() + ["Ln Prob"]
    tag = "synthetic_nw%d_ns%d" % (args.nwalkers, args.nsteps)
    tableio.write_fixed_width_two_line(os.path.join(args.out, "fitposterior_%s.dat" % tag),
                                       list(LFmod.samples.T), names)
    tableio.write_fixed_width_two_line(os.path.join(args.out, "bestfitLF_%s.dat" % tag),
                                       [LFmod.lum, LFmod.lum_e, LFmod.medianLF], ["Luminosity", "Luminosity_Err", "MedianLF"])
    tableio.write_fixed_width_two_line(os.path.join(args.out, "VeffLF_%s.dat" % tag),
                                       [LFmod.Lavg, LFmod.lfbinorig, np.sqrt(LFmod.var)], ["Luminosity", "BinLF", "BinLFErr"])
    percentiles = [5, 16, 50, 84, 95]
    labels = ["Line"] + [n + "_%02d" % p for n in names[:-1] for p in percentiles]
    LFmod.table = [["OIII"] + [0.0] * (len(labels) - 1)]
    LFmod.add_fitinfo_to_table(percentiles)
    tableio.write_fixed_width_two_line(os.path.join(args.out, "%s.dat" % tag), [np.array([v]) for v in LFmod.table[-1]],
                                       labels, formats={l: ("%s" if l == "Line" else "%0.3f") for l in labels})
    med = np.median(LFmod.samples[:, :-1], axis=0)
    print("posterior medians:", dict(zip(names[:-1], np.round(med, 3))))
    if args.map:
        sd = np.sqrt(np.diag(LFmod.map_cov))
        print("MAP (converged: %s; on a bound: %s):" % (LFmod.map_info["converged"], [n for n, b in zip(names, LFmod.map_info["on_bound"]) if b]))
        for n, t, e, m in zip(names[:-1], LFmod.map_theta, sd, med):
            print("  %-22s %9.4f +/- %.4f   (median %9.4f)" % (n, t, e, m))
        print("lnprob at the maximum %.4f; lnZ_laplace %.4f %s" % (LFmod.map_lnprob, LFmod.lnZ_laplace, LFmod.map_info["lnZ_reason"]))
        if plain_map is not None:
            print("maximum of the plain likelihood (converged: %s): %s" % (plain_map["converged"], np.round(plain_map["theta"], 4)))
            print("maximum of the convolved likelihood: %s" % np.round(LFmod.map_theta, 4))
            print("Eddington shift of L* (plain - convolved): %+.4f dex" % (plain_map["theta"][0] - LFmod.map_theta[0]))
    if args.integrals:
        write_integrals(LFmod, os.path.join(args.out, "integrals_%s.dat" % tag))
    if args.deconvolved_lums:
        write_deconvolved_lums(LFmod, args.deconvolved_lums)
    if args.veff_deconvolved:
        print_veff_deconvolved(LFmod)
    if args.predictive_noise:
        pp = LFmod.posterior_predictive(seed=11, noise=None if args.predictive_noise == "none" else "catalogue")
        bright = pp["edges"].size // 2
        print("posterior predictive check (noise: %s), per field: observed total, median replicated total, P(rep >= obs), and the "
              "same for the brighter half of the bins" % pp["noise"])
        for f in range(pp["nf"]):
            ob, rb = pp["observed"][f, bright:].sum(), pp["replicated"][:, f, bright:].sum(axis=1)
            print("  field %d: %6d %8.1f %.3f   bright: %6d %8.1f %.3f" % (f, pp["observed_total"][f], np.median(pp["replicated_total"][:, f]),
                                                                         pp["p_upper_total"][f], ob, np.median(rb), np.mean(rb >= ob)))
    if args.predictive_cut:
        pp = LFmod.posterior_predictive(seed=11, cut=True)
        print("posterior predictive check against the cut process, per field: observed total, median replicated total, "
              "P(rep >= obs), and the same for the two faintest bins")
        for f in range(pp["nf"]):
            ob, rb = pp["observed"][f, 1:3].sum(), pp["replicated"][:, f, 1:3].sum(axis=1)
            print("  field %d: %6d %8.1f %.3f   at the cut: %6d %8.1f %.3f" % (f, pp["observed_total"][f],
                                                                              np.median(pp["replicated_total"][:, f]),
                                                                              pp["p_upper_total"][f], ob, np.median(rb), np.mean(rb >= ob)))
    if args.predictive_z:
        noise = "catalogue" if args.predictive_noise == "catalogue" else None
        pp = LFmod.posterior_predictive(seed=11, cut=args.predictive_cut, noise=noise,
                                        z_edges=np.linspace(LFmod.zmin, LFmod.zmax, args.predictive_z + 1))
        print("posterior predictive check in (z, logL) (noise: %s%s), per field: N(z) observed | 16 / 50 / 84 %% of the replicates, "
              "bin by bin, then the deviance, P(D_rep >= D_obs) and the observed sources in cells no replicate fills"
              % (pp["noise"], ", cut process" if args.predictive_cut else ""))
        for f in range(pp["nf"]):
            for b in range(1, args.predictive_z + 1):
                lo, mid, hi = pp["percentiles_z"][:, f, b]
                print("  field %d  z %.3f-%.3f: %6d | %8.1f %8.1f %8.1f" % (f, pp["z_edges"][b - 1], pp["z_edges"][b], pp["observed_z"][f, b],
                                                                       lo, mid, hi))
            print("  field %d  deviance %.1f  p_deviance %.3f  in empty cells %d (of %d empty)"
                  % (f, pp["deviance"][f], pp["p_deviance"][f], pp["observed_in_empty"][f], pp["n_empty_cells"][f]))
    if args.veff_band:
        write_veff_band(LFmod, os.path.join(args.out, "veffband_%s.dat" % tag), volumes=args.veff_volumes)
    if args.veff_slices:
        write_veff_slices(LFmod, args.out, tag, args.veff_slices)
    print("wrote", sorted(os.listdir(args.out)))
    LFmod.close()


if __name__ == "__main__":
    main()
