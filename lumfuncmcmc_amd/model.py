"""LumFuncMCMC / LumFuncMCMCz: the reference's class surface over the HIP boundary.

Constructor keywords, attribute names and method names are those of the reference
(lumfuncmcmc.py:73-79, lumfuncmcmc_z.py:119-125) so that its drivers
(run_lumfuncmcmc.py:245-256, run_lumfuncmcmc_z.py:218-229) construct these classes unchanged.
What differs is underneath: setup comes from hostsetup.py (own cosmology, no astropy), and
`lnprob` / `lnprob_fix_comp` do not evaluate anything in Python - they hand theta to
liblfmcmc.so (one row, or a whole half-ensemble at once) and return what the GPU computed.
There is no NumPy fallback: without the library or a GPU the call raises.
"""
import logging
import time

import numpy as np

from . import hostsetup as hs
from . import lfbands
from . import lfintegrals
from . import mock
from . import veff
from .cosmology import cosmo as _cosmo
from .capi import LFContext
from .sampler import DeviceEnsembleSampler, DevicePTSampler, EnsembleSampler, default_ntemps, integrated_time, tmax_from_box

TrueLumFunc = hs.true_lum_func       # module-level names the reference exports (lumfuncmcmc.py:25)
schechter_z = hs.schechter_z         # lumfuncmcmc_z.py:45
getQuadCoef = hs.get_quad_coef       # lumfuncmcmc_z.py:26
Omega = hs.omega                     # lumfuncmcmc.py:47


class _Base(object):
    """State and behaviour shared by the two model classes."""

    _logger_name = 'lumfuncmcmc'
    device = 0
    compress = False               # True: piece A from the compressed catalogue (csrc/lf_compress.h), opt-in
    shard = "walkers"              # several ranks (torch.distributed, one process per GPU): "walkers" = every rank holds
                                   # the catalogue and evaluates a slice of each half-ensemble (all-gather of lnprob);
                                   # "sources" = every rank holds 1/world of the catalogue and of the grid and evaluates
                                   # every walker (all-reduce of lnprob) - for ensembles too small to split by walker

    @staticmethod
    def _check_shard(shard):
        if shard not in ("walkers", "sources"):
            raise ValueError("shard must be 'walkers' or 'sources', not %r" % (shard,))
        return shard

    # ------------------------------------------------------------------ setup (host, once)
    def _common_init(self, z, flux, flux_e, lum, lum_e):
        self.z = np.concatenate(z)
        self.zmin, self.zmax = min(self.z), max(self.z)
        self._ctx, self._ctx_key = None, None
        self.lnprob_fn = None          # optional override (lumfuncmcmc_amd.dist.ShardedLnProb)

    def setDLdVdz(self):
        """lumfuncmcmc.py:180-202."""
        t = hs.distance_tables(self.z)
        self.DL, self.DLf, self.dVdzf = t["DL"], t["DLf"], t["dVdzf"]
        self._zint, self._DLarr = t["zint"], t["DLarr"]
        roots = self._setup_roots()
        self.minlumf = []
        for ii in range(self.nfields):
            if self.min_comp_frac <= 0.001:
                minlum = np.zeros_like(self._DLarr)
            else:
                minlum = np.log10(4.0 * np.pi * (self._DLarr * hs.MPC_CM) ** 2 * roots[ii])
            self.minlumf.append(hs.LinearInterp(self._zint, minlum))

    def _fluxes_and_lums(self, flux, flux_e, lum, lum_e):
        """lumfuncmcmc.py:165-173."""
        if flux is not None:
            self.flux = 1.0e-17 * np.concatenate(flux)
            self.flux_e = 1.0e-17 * np.concatenate(flux_e) if flux_e is not None else None
        else:
            self.lum, self.lum_e = np.concatenate(lum), np.concatenate(lum_e)
            self.getFluxes()
        if lum is None:
            self.getLumin()

    def getLumin(self):
        self.lum, self.lum_e = hs.lum_from_flux(self.flux, self.flux_e, self.DL)

    def getFluxes(self):
        self.flux, self.flux_e = hs.flux_from_lum(self.lum, self.lum_e, self.DL)

    def defineFlimOmArr(self):
        self.Flims_arr, self.Omega_0_arr = hs.field_arrays(self.Flim, self.Omega_0, self.field_ind)

    def getFlim(self):
        for ii in range(self.nfields):
            self.Flims_arr[self.field_ind[ii]:self.field_ind[ii + 1]] = self.Flim[ii]

    def setOmegaLz(self, size=501):
        """lumfuncmcmc.py:204-215.  Only the fixed-completeness likelihoods read these splines, so
        the free-completeness class builds them on first use."""
        self._Omegaf = hs.omega_splines(self.DLf, self.zmin, self.zmax, self.Lc, self.Lh, self.Omega_0,
                                        self.Flim, self.alpha, self.fcmin, size=size)

    @property
    def Omegaf(self):
        if getattr(self, "_Omegaf", None) is None:
            self.setOmegaLz()
        return self._Omegaf

    def setlnsimple(self, need_integ=True):
        """lumfuncmcmc.py:217-235."""
        g = hs.integration_grid(self.size_ln, self.zmin, self.zmax, np.min(self.lum), self.Lh, self.DLf,
                                self.dVdzf, self.minlumf, self.Omegaf if need_integ else None)
        self.zarr, self.DL_zarr, self.volume_part = g["zarr"], g["DL_zarr"], g["volume_part"]
        self.zarr_rep, self.logL = g["zarr_rep"], g["logL"]
        self.logLi = self.logL[-1]
        self._integ_part = g["integ_part"]
        self.Om_arr = hs.omega(self.lum, self.z, self.DLf, self.Omega_0_arr, 1.0e-17 * self.Flims_arr,
                               self.alpha, self.fcmin)
        self._DLz = self.DLf(self.z)

    @property
    def integ_part(self):
        if self._integ_part is None:
            self._integ_part = [self.volume_part * self.Omegaf[ii].ev(self.logL[ii], self.zarr_rep)
                                for ii in range(self.nfields)]
        return self._integ_part

    def setup_logging(self):
        self.log = logging.getLogger(self._logger_name)
        if not len(self.log.handlers):
            handler = logging.StreamHandler()
            handler.setFormatter(logging.Formatter('[%(levelname)s - %(asctime)s] %(message)s'))
            handler.setLevel(logging.INFO)
            self.log.setLevel(logging.DEBUG)
            self.log.addHandler(handler)

    # ------------------------------------------------------------------ the boundary
    def _variant(self):
        raise NotImplementedError

    def _lims(self):
        return {"Lstar": self.Lstar_lims, "phistar": self.phistar_lims, "sch_al": self.sch_al_lims,
                "Flim": getattr(self, "Flim_lims", [1.0, 6.0]), "alpha": getattr(self, "alpha_lims", [1.0, 7.0])}

    def kernel_inputs(self):
        """The arrays the C ABI takes (include/lfmcmc.h), under the reference's attribute names."""
        v = self._variant()
        inp = {"variant": v, "fix_sch_al": bool(self.fix_sch_al), "sch_al0": float(self.sch_al),
               "field_ind": np.asarray(self.field_ind, dtype=np.int64), "lum": self.lum, "z": self.z,
               "DLz": self._DLz, "Omega_0": np.asarray(self.Omega_0, dtype=np.float64),
               "Om_arr": self.Om_arr, "Flim0": np.asarray(self._Flim0, dtype=np.float64),
               "alpha0": float(self._alpha0), "logL": self.logL[-1], "zarr": self.zarr,
               "DL_zarr": self.DL_zarr, "volume_part": self.volume_part, "fcmin": self.fcmin,
               "lims": self._lims(), "pivots": (getattr(self, "z1", 1.2), getattr(self, "z2", 1.53),
                                                getattr(self, "z3", 1.86)),
               "integ_part": None}
        if v != "free":
            inp["integ_part"] = np.array(self.integ_part)
        return inp

    @staticmethod
    def _dist_state():
        """(rank, world) of the default torch.distributed group, (0, 1) when there is none."""
        try:
            import torch.distributed as tdist
            if tdist.is_available() and tdist.is_initialized():
                return tdist.get_rank(), tdist.get_world_size()
        except ImportError:
            pass
        return 0, 1

    def context(self):
        """The device context for the current (variant, fixed-parameter) configuration.  With shard == "sources"
        and several ranks it holds this rank's 1/world of the catalogue and of the integration grid: its lnprob is a
        partial sum that only means something after the all-reduce (fit_model does that)."""
        rank, world = self._dist_state()
        by_source = self.shard == "sources" and world > 1
        key = (self._variant(), bool(self.fix_sch_al), float(self.sch_al) if self.fix_sch_al else None,
               (rank, world) if by_source else None)
        if self._ctx is None or self._ctx_key != key:
            if self._ctx is not None:
                self._ctx.close()
            inp = self.kernel_inputs()
            if by_source:
                from .dist import shard_sources
                inp = shard_sources(inp, rank, world)
            self._ctx = LFContext(inp, device=self.device, max_batch=max(8, getattr(self, "nwalkers", 100) // 2))
            if by_source:
                self._ctx.set_option("grid_share", rank + 65536 * world)
            if self.compress:
                self._ctx.set_option("compress", 1)
            if self.deconvolve:
                if self.deconvolve_cut:
                    self._ctx.set_cut_error_model(*self.deconvolve_cut_errors)
                    if self.deconvolve_cut_grad:
                        self._ctx.set_option("deconv_cut_grad", 1)
                    if self.deconvolve_cut_veff:
                        self._ctx.set_option("deconv_cut_veff", 1)
                self._ctx.set_lum_err(self.lum_e, self.deconvolve_order, unchecked=self.deconvolve_unchecked,
                                       wide=self.deconvolve_wide)
            if self.deconvolve_tile:
                self._ctx.set_option("deconv_tile", 1)
            self._ctx_key = key
        return self._ctx

    # ------------------------------------------------------------------ flux-error-convolved likelihood
    deconvolve = False             # True: lnprob is the likelihood convolved with the sources' lum_e (csrc/lf_deconv.h), opt-in
    deconvolve_order = None        # its Gauss-Hermite order (None: the library's default)
    deconvolve_unchecked = False   # True: lum_e above the order's validated range is taken as it is
    deconvolve_tile = False        # True: the context option "deconv_tile" (csrc/lf_deconv_tile.h; no effect with free completeness)
    deconvolve_wide = False        # True: lum_e above the order's range, up to 0.30 dex, by the wide rule (csrc/lf_deconv_wide.h)

    deconvolve_cut = False         # True: the cut on the observed flux of min_comp_frac > 0.001 is modelled (csrc/lf_deconv_cut.h)
    deconvolve_cut_errors = None   # its error model (nodes (M,), sigma (nf, M)); None: the one this catalogue shows (error_model())
    deconvolve_cut_grad = False    # True: the gradient of the cut's term is served too (csrc/lf_deconv_cut_grad.h): MAP fits under the cut
    deconvolve_cut_veff = False    # True: veff_deconvolved is served under the cut, by the catalogued volume per node (csrc/lf_vefftrue_cut.h)

    def _init_deconvolve(self, deconvolve, deconvolve_order, deconvolve_tile=False, deconvolve_wide=False, deconvolve_cut=False,
                         deconvolve_cut_errors=None, deconvolve_cut_grad=False, deconvolve_cut_veff=False):
        from . import deconv
        self.deconvolve, self.deconvolve_order = bool(deconvolve), deconvolve_order
        self.deconvolve_tile, self.deconvolve_wide = bool(deconvolve_tile), bool(deconvolve_wide)
        self.deconvolve_cut = bool(deconvolve_cut)
        self.deconvolve_cut_grad = bool(deconvolve_cut_grad)
        self.deconvolve_cut_veff = bool(deconvolve_cut_veff)
        if self.deconvolve_cut_veff and not self.deconvolve_cut:
            raise ValueError("deconvolve_cut_veff=True needs deconvolve_cut=True: it is the cut's catalogued volume per node that "
                             "it divides the deconvolved 1/Veff points by")
        if self.deconvolve_cut_grad and not self.deconvolve_cut:
            raise ValueError("deconvolve_cut_grad=True needs deconvolve_cut=True: it is the gradient of Delta B, the cut's change "
                             "of the expected counts, that it adds")
        if self.deconvolve_cut and not self.min_comp_frac > 0.001:
            raise ValueError("deconvolve_cut=True needs min_comp_frac > 0.001: with min_comp_frac <= 0.001 there is no cut on the "
                             "observed flux, and deconvolve=True alone is the model")
        if deconvolve_cut and not self.deconvolve:
            raise ValueError("deconvolve_cut=True needs deconvolve=True: it is the convolved likelihood's expected counts that the "
                             "cut on the observed flux changes")
        if not self.deconvolve:
            return
        if self.lum_e is None:
            raise ValueError("deconvolve=True needs lum_e (or flux_e): the sources' errors are what the likelihood is convolved with")
        if self.min_comp_frac > 0.001 and not self.deconvolve_cut:
            raise ValueError("deconvolve=True needs min_comp_frac <= 0.001: a cut on the observed flux would change the "
                             "expected counts, which the convolved likelihood leaves as they are (deconvolve_cut=True adds "
                             "that change)")
        if self.deconvolve_cut:
            # The error model at the TRUE flux.  The default is read off the catalogue, which has no sources below the cut:
            # there it continues as a constant (the faintest node's value).  A caller who knows the errors below the cut
            # passes (nodes, sigma) with nodes there.
            nodes, sig = self.error_model() if deconvolve_cut_errors is None else deconvolve_cut_errors
            self.deconvolve_cut_errors = deconv.check_cut_error_model(nodes, sig, self.nfields)
        if self.shard != "walkers":
            raise NotImplementedError("deconvolve=True is not implemented for shard='sources'")
        K = deconv.DEFAULT_ORDER if deconvolve_order is None else int(deconvolve_order)
        if K not in deconv.ORDERS:
            raise ValueError("deconvolve_order must be one of %s" % (deconv.ORDERS,))
        self.deconvolve_order = K
        sg = deconv.check_sigma(self.lum_e, len(self.lum), K, self.deconvolve_unchecked or self.deconvolve_wide)
        if self.deconvolve_wide:
            deconv.wide_class(sg, K)                 # (refuses lum_e above the wide rule's top edge)

    def _evaluate(self, theta):
        th = np.asarray(theta, dtype=np.float64)
        scalar = th.ndim == 1
        if self.deconvolve and self.lnprob_fn is None:
            out = self.context().lnprob_err_batch(th)
            return float(out[0]) if scalar else out
        if self.lnprob_fn is not None:
            out = np.asarray(self.lnprob_fn(np.atleast_2d(th)))
        else:
            out = self.context().lnprob_batch(th)
            rank, world = self._dist_state()
            if self.shard == "sources" and world > 1:
                # this rank's context holds 1/world of every field's sources and of the grid: its lnprob is a partial sum -
                # the ranks' sum is the value (every rank calls this with the same theta, as every collective requires)
                import torch
                import torch.distributed as tdist
                t = torch.from_numpy(np.ascontiguousarray(np.atleast_1d(out), dtype=np.float64))
                if tdist.get_backend() == "nccl":
                    t = t.to("cuda:%d" % self.device)
                tdist.all_reduce(t, op=tdist.ReduceOp.SUM)
                out = t.cpu().numpy()
        return float(out[0]) if scalar else out

    # ------------------------------------------------------------------ sampling
    def _theta_lims(self):
        raise NotImplementedError

    def get_init_walker_values(self, num=None):
        """Uniform in the prior box from numpy's global state (lumfuncmcmc.py:426-446)."""
        lims = self._theta_lims()
        if num is None:
            num = self.nwalkers
        if getattr(self, "diff_rand", True):
            u = np.random.rand(num, len(lims))
        else:
            u = np.random.rand(num)[:, np.newaxis]
        return u * (lims[:, 1] - lims[:, 0]) + lims[:, 0]

    def _lnprob_name(self):
        return 'lnprob'

    def fit_model(self):
        """Run the ensemble sampler on the batched boundary and collect `self.samples`
        (lumfuncmcmc.py:479-513): same log lines, burn-in = min(int(3 tau), nsteps//2), samples =
        post-burn-in chain flattened with lnprob as last column."""
        self.log.info('Fitting Schechter model to true luminosity function using emcee')
        pos = self.get_init_walker_values()
        ndim = pos.shape[1]
        start = time.time()
        # With torch.distributed initialised (one process per GPU) every rank runs the same sampler on the same
        # ensemble: start positions and the sampler's seed come from rank 0 (each process has its own numpy state).
        seed = int(np.random.randint(0, 2 ** 31 - 1))
        rank, world = self._dist_state()
        if world > 1:
            import torch.distributed as tdist
            box = [pos, seed]
            tdist.broadcast_object_list(box, src=0)
            pos, seed = box
        self.start_pos, self.sampler_seed = np.array(pos), seed       # (start, seed) reproduce the chain
        if self.deconvolve and (world > 1 or self.lnprob_fn is not None):
            raise NotImplementedError("fit_model with deconvolve=True runs on one GPU and cannot use lnprob_fn")
        if self.lnprob_fn is None and getattr(self, "device_sampler", True) and not self.deconvolve:
            # the whole stretch move runs on the device (theta never leaves HBM).  With several ranks every half-step
            # is sharded - by walker (all-gather of lnprob, RCCL) or by source (all-reduce), see `shard` - and
            # accepted on every rank.
            sampler = DeviceEnsembleSampler(self.context(), self.nwalkers, seed=seed, capacity=self.nsteps)
            if world > 1:
                sampler.enqueue_sharded(pos, self.nsteps, shard=self.shard)
                sampler.sync()
            else:
                sampler.run_mcmc(pos, self.nsteps)
        elif world > 1:
            # host sampler over a sharded callable (lnprob_fn = dist.ShardedLnProb): the ranks must propose the same
            # moves, so the random stream is seeded from rank 0's draw, not from each process's global state
            sampler = EnsembleSampler(self.nwalkers, ndim, getattr(self, self._lnprob_name()), vectorize=True, seed=seed)
            sampler.run_mcmc(pos, self.nsteps)
        else:
            sampler = EnsembleSampler(self.nwalkers, ndim, getattr(self, self._lnprob_name()), vectorize=True)
            sampler.run_mcmc(pos, self.nsteps, rstate0=np.random.get_state())
        elapsed = time.time() - start
        self.log.info("Total time taken: %0.2f s" % elapsed)
        self.log.info("Time taken per step per walker: %0.2f ms" % (elapsed / (self.nsteps) * 1000. / self.nwalkers))
        tau = np.max(sampler.acor)
        burnin_step = int(tau * 3)
        if burnin_step > self.nsteps // 2:
            burnin_step = self.nsteps // 2
        self.log.info("Mean acceptance fraction: %0.2f" % (np.mean(sampler.acceptance_fraction)))
        self.log.info("AutoCorrelation Steps: %i, Number of Burn-in Steps: %i" % (np.round(tau), burnin_step))
        new_chain = np.zeros((self.nwalkers, self.nsteps, ndim + 1))
        new_chain[:, :, :-1] = sampler.chain
        self.chain = sampler.chain
        new_chain[:, :, -1] = sampler.lnprobability
        self.samples = new_chain[:, burnin_step:, :].reshape((-1, ndim + 1))
        self.sampler = sampler
        self.log.info("Shape of self.samples")
        self.log.info(self.samples.shape)
        self.log.info("Median lnprob: %.5f; Max lnprob: %.5f" % (np.median(sampler.lnprobability),
                                                                np.amax(sampler.lnprobability)))

    def fit_model_converged(self, max_steps=None, check_every=None, ntau=50, rtol=0.01, start="box", likelihood=None):
        """fit_model that runs until the chain is long enough instead of for a number of steps guessed beforehand: one
        device sampler with room for max_steps (default 10 * self.nsteps) runs check_every steps at a time (default
        max(100, self.nsteps // 10)) and asks the chain where it is for its autocorrelation times
        (DeviceEnsembleSampler.diagnostics).  It stops when
            steps > ntau * max(tau)   and   max |tau - tau_prev| / tau < rtol
        - emcee's documented recipe, with its numbers 50 and 0.01 - or at max_steps with a warning.  The chain is read back
        once, at the end.  Sets what fit_model sets (samples, chain, sampler, start_pos, sampler_seed; burn-in =
        min(int(3 max tau), steps // 2) with the device's tau) plus self.converged and self.tau_history = [(steps, tau), ...];
        returns the last tau.  One GPU, device sampler only.  start="map": the walkers start in a Gaussian ball around the
        maximum a posteriori (map_init_walkers; fit_model_map runs first when it has not) instead of the prior box.
        likelihood: what the device sampler samples, with fit_model_map's semantics - None (the plain likelihood; an object made
        with deconvolve=True refuses and asks for the choice), "convolved" (deconvolve=True only: the flux-error-convolved
        likelihood) or "plain" (also under deconvolve=True); start="map" uses the same one.
        self.sampler_likelihood records which one ran."""
        if start not in ("box", "map"):
            raise ValueError('start must be "box" or "map"')
        likelihood = self._map_likelihood(likelihood, "fit_model_converged does")
        rank, world = self._dist_state()
        if world > 1:
            raise NotImplementedError("fit_model_converged runs on one GPU: diagnostics across several ranks are not implemented")
        if self.lnprob_fn is not None:
            raise NotImplementedError("fit_model_converged runs the device sampler: it cannot use lnprob_fn")
        max_steps = int(10 * self.nsteps if max_steps is None else max_steps)
        check_every = int(max(100, self.nsteps // 10) if check_every is None else check_every)
        if max_steps < 1 or check_every < 1:
            raise ValueError("max_steps and check_every must be positive")
        self.log.info('Fitting Schechter model to true luminosity function until the chain has converged')
        if start == "map" and (getattr(self, "map_theta", None) is None or getattr(self, "map_info", {}).get("likelihood", likelihood) != likelihood):
            self.fit_model_map(likelihood=likelihood)
        pos = self.get_init_walker_values() if start == "box" else self.map_init_walkers(likelihood=likelihood)
        ndim = pos.shape[1]
        start = time.time()
        seed = int(np.random.randint(0, 2 ** 31 - 1))
        self.start_pos, self.sampler_seed = np.array(pos), seed       # (start, seed, steps) reproduce the chain
        self.sampler_likelihood = likelihood
        sampler = DeviceEnsembleSampler(self.context(), self.nwalkers, seed=seed, capacity=max_steps, likelihood=likelihood)
        steps, tau, tau_prev = 0, None, None
        self.converged, self.tau_history = False, []
        while steps < max_steps and not self.converged:
            k = min(check_every, max_steps - steps)
            sampler.enqueue(pos if steps == 0 else None, k)
            steps += k
            tau_prev, tau = tau, sampler.diagnostics().tau
            self.tau_history.append((steps, tau.copy()))
            self.converged = bool(tau_prev is not None and steps > ntau * np.max(tau)
                                  and np.max(np.abs(tau - tau_prev) / tau) < rtol)
        if not self.converged:
            self.log.warning("fit_model_converged: not converged after max_steps = %d steps (max tau %.1f, needs more than "
                             "%d tau): going on with the chain there is" % (max_steps, np.max(tau), ntau))
        sampler.sync()
        elapsed = time.time() - start
        self.log.info("Total time taken: %0.2f s" % elapsed)
        self.log.info("Time taken per step per walker: %0.2f ms" % (elapsed / steps * 1000. / self.nwalkers))
        taumax = np.max(tau)
        burnin_step = int(taumax * 3)
        if burnin_step > steps // 2:
            burnin_step = steps // 2
        self.log.info("Mean acceptance fraction: %0.2f" % (np.mean(sampler.acceptance_fraction)))
        self.log.info("AutoCorrelation Steps: %i, Number of Burn-in Steps: %i" % (np.round(taumax), burnin_step))
        new_chain = np.zeros((self.nwalkers, steps, ndim + 1))
        new_chain[:, :, :-1] = sampler.chain
        self.chain = sampler.chain
        new_chain[:, :, -1] = sampler.lnprobability
        self.samples = new_chain[:, burnin_step:, :].reshape((-1, ndim + 1))
        self.sampler = sampler
        self.log.info("Shape of self.samples")
        self.log.info(self.samples.shape)
        self.log.info("Median lnprob: %.5f; Max lnprob: %.5f" % (np.median(sampler.lnprobability),
                                                                np.amax(sampler.lnprobability)))
        return tau

    # ------------------------------------------------------------------ maximum a posteriori (mapfit.py)
    def _map_likelihood(self, likelihood, who="fit_model_map and map_init_walkers do"):
        """Which likelihood fit_model_map / map_init_walkers maximise and fit_model_converged / fit_model_pt sample: None (the
        plain one; refused under deconvolve=True, where the choice has to be stated), "plain" or "convolved" (needs
        deconvolve=True; DESIGN.md sections 3.19 and 3.20)."""
        if likelihood is None:
            if self.deconvolve:
                raise NotImplementedError("%s not choose a likelihood for deconvolve=True: "
                                          'pass likelihood="convolved" (the flux-error-convolved one, lnprob\'s) or '
                                          'likelihood="plain"' % who)
            return "plain"
        if likelihood not in ("plain", "convolved"):
            raise ValueError('likelihood must be None, "plain" or "convolved", got %r' % (likelihood,))
        if likelihood == "convolved" and not self.deconvolve:
            raise ValueError('likelihood="convolved" needs an object made with deconvolve=True')
        return likelihood

    def _grad_fn(self, likelihood=None):
        """The batched (lnprob, gradient) callable of the current configuration: the device's (LFContext.lnprob_grad, or
        LFContext.lnprob_err_grad for the convolved likelihood)."""
        likelihood = self._map_likelihood(likelihood)
        rank, world = self._dist_state()
        if world > 1:
            raise NotImplementedError("the gradient runs on one GPU: source- or walker-sharded gradients are not implemented")
        if self.lnprob_fn is not None:
            raise NotImplementedError("the gradient comes from the device context: it cannot use lnprob_fn")
        if likelihood == "convolved" and self.deconvolve_cut and not self.deconvolve_cut_grad:
            raise NotImplementedError("the convolved likelihood's gradient is not implemented under deconvolve_cut=True: the "
                                      "gradient of Delta B, the cut's change of the expected counts, is missing (fit_model, "
                                      "fit_model_converged and fit_model_pt sample it without a gradient)")
        return self.context().lnprob_err_grad if likelihood == "convolved" else self.context().lnprob_grad

    def fit_model_map(self, nstarts=16, seed=None, tol=1e-6, likelihood=None):
        """Maximum a posteriori fit: box-constrained Newton iterations from nstarts draws of get_init_walker_values' box
        (seed: a RandomState of its own instead of numpy's global one; a start with -inf lnprob is drawn again), every
        iteration one batched gradient call on the device (mapfit.maximise).  For fixed completeness the context is
        lnprob_fix_comp's, as in fit_model.  Sets map_theta, map_lnprob, map_hessian, map_cov = (-H)^-1 (over the
        coordinates not held at a bound: rows and columns of a held coordinate are 0) and lnZ_laplace (NaN when a
        coordinate is on its bound or -H is not positive definite: map_info["lnZ_reason"] says which); returns them in a
        dict with converged, on_bound, niter and decrement.  likelihood: None (the plain likelihood; an object made with
        deconvolve=True refuses and asks for the choice), "convolved" (deconvolve=True only: the flux-error-convolved
        likelihood, LFContext.lnprob_err_grad) or "plain" (also under deconvolve=True: the two maxima side by side give the
        catalogue's Eddington shift); map_info["likelihood"] records which one ran.  Under deconvolve_cut=True (min_comp_frac >
        0.001) the convolved likelihood's gradient needs deconvolve_cut_grad=True, which adds the gradient of Delta B (DESIGN.md
        section 3.33); without it the call refuses."""
        from . import mapfit
        likelihood = self._map_likelihood(likelihood)
        f = self._grad_fn(likelihood)
        box = self._theta_lims()
        rs = np.random.RandomState(seed) if seed is not None else np.random
        draw = lambda n: rs.rand(n, len(box)) * (box[:, 1] - box[:, 0]) + box[:, 0]    # noqa: E731
        starts = draw(int(nstarts))
        for _ in range(100):
            bad = ~np.isfinite(f(starts)[0])
            if not bad.any():
                break
            starts[bad] = draw(int(bad.sum()))
        # (the z-evolving prior excludes the bounds of L and phi - lnprob is -inf on them: work a hair inside)
        r = mapfit.maximise(f, box, starts, tol=tol, inset=1.0e-9 if self._variant() == "zevol" else 0.0)
        H = r["hessian"]
        free = ~r["on_bound"]
        cov = np.zeros_like(H)
        try:
            cov[np.ix_(free, free)] = np.linalg.inv(-H[np.ix_(free, free)])
        except np.linalg.LinAlgError:
            cov[:] = np.nan
        lnZ, why = mapfit.laplace_evidence(r["lnprob"], H, box, on_bound=r["on_bound"])
        self.map_theta, self.map_lnprob, self.map_hessian, self.map_cov, self.lnZ_laplace = r["theta"], r["lnprob"], H, cov, lnZ
        self.map_info = {"theta": r["theta"], "lnprob": r["lnprob"], "hessian": H, "cov": cov, "lnZ_laplace": lnZ,
                         "lnZ_reason": why, "converged": r["converged"], "on_bound": r["on_bound"], "niter": r["niter"],
                         "decrement": r["decrement"], "box": r["box"], "likelihood": likelihood}
        self.log.info("MAP fit: lnprob %.5f after %d iterations (%sconverged), Laplace lnZ %.3f %s"
                      % (r["lnprob"], r["niter"], "" if r["converged"] else "NOT ", lnZ, why))
        return self.map_info

    def map_init_walkers(self, num=None, scale=1.0, likelihood=None):
        """Start positions drawn from N(map_theta, scale^2 map_cov) (numpy's global state, like get_init_walker_values)
        instead of the prior box; a row outside the box or with a lnprob that is not finite is drawn again, so every walker
        starts with a finite lnprob.  A coordinate held at a bound has no variance in map_cov: it is scattered into the box
        by |N(0, (1e-3 width)^2)| so that the ensemble is not degenerate there.  likelihood: whose lnprob has to be finite
        (as in fit_model_map; "convolved" under deconvolve_cut=True needs deconvolve_cut_grad=True, as there)."""
        if getattr(self, "map_theta", None) is None:
            raise RuntimeError("map_init_walkers: call fit_model_map first")
        if not np.all(np.isfinite(self.map_cov)):
            raise RuntimeError("map_init_walkers: map_cov is not finite")
        num = self.nwalkers if num is None else int(num)
        box = self._theta_lims()
        f = self._grad_fn(likelihood)
        held = self.map_info["on_bound"]
        cov = 0.5 * (self.map_cov + self.map_cov.T) * scale ** 2

        def draw(n):
            x = np.random.multivariate_normal(self.map_theta, cov, size=n, check_valid="ignore")
            if held.any():
                into = np.where(self.map_theta[held] < 0.5 * (box[held, 0] + box[held, 1]), 1.0, -1.0)
                x[:, held] += into * np.abs(np.random.randn(n, int(held.sum()))) * 1.0e-3 * (box[held, 1] - box[held, 0])
            return x

        pos = draw(num)
        for _ in range(200):
            bad = np.any((pos < box[:, 0]) | (pos > box[:, 1]), axis=1)
            ok = ~bad
            if ok.any():
                bad[ok] = ~np.isfinite(f(pos[ok])[0])
            if not bad.any():
                return pos
            pos[bad] = draw(int(bad.sum()))
        raise RuntimeError("map_init_walkers: could not draw %d walkers with finite lnprob around the maximum" % num)

    def fit_model_pt(self, ntemps=None, Tmax=None, betas=None, fburnin=0.1, likelihood=None):
        """Parallel-tempered fit (DevicePTSampler, sampler.py) and the Bayesian evidence of this model by thermodynamic
        integration, for comparing the models the classes offer.  self.nwalkers walkers per temperature, self.nsteps
        steps; every temperature starts from get_init_walker_values (a start with -inf lnprob is drawn again).  Ladder:
        `betas`, or geometric up to Tmax (None: tmax_from_box on the prior box) over ntemps temperatures (None:
        default_ntemps(Tmax)).  Sets self.samples from the beta = 1 chain as fit_model does, and self.pt_sampler,
        self.lnZ, self.dlnZ (fburnin: the leading fraction of steps the estimator leaves out).  likelihood: as in
        fit_model_converged - the starts' lnlike, Tmax from the box and the tempered target are all the chosen likelihood's."""
        likelihood = self._map_likelihood(likelihood, "fit_model_pt does")
        rank, world = self._dist_state()
        if world > 1:
            raise NotImplementedError("fit_model_pt runs on one GPU: parallel tempering over several ranks is not implemented")
        if self.lnprob_fn is not None:
            raise NotImplementedError("fit_model_pt runs the device sampler: it cannot use lnprob_fn")
        self.log.info('Fitting Schechter model with parallel tempering (evidence by thermodynamic integration)')
        ctx = self.context()
        lnlike = ctx.lnprob_err_batch if likelihood == "convolved" else ctx.lnprob_batch
        lims = self._theta_lims()
        if betas is not None:
            ntemps = len(betas)
        else:
            if Tmax is None:
                Tmax = tmax_from_box(lnlike, lims)
            if ntemps is None:
                ntemps = default_ntemps(Tmax)
        W, ndim = self.nwalkers, len(lims)
        pos = np.array([self.get_init_walker_values() for _ in range(ntemps)])
        ll = lnlike(pos.reshape(-1, ndim)).reshape(ntemps, W)
        for _ in range(100):
            bad = ~np.isfinite(ll)
            if not bad.any():
                break
            fresh = self.get_init_walker_values(int(bad.sum()))
            pos[bad] = fresh
            ll[bad] = lnlike(fresh)
        else:
            raise RuntimeError("fit_model_pt: no finite start in 100 draws of the prior box")
        seed = int(np.random.randint(0, 2 ** 31 - 1))
        self.start_pos, self.sampler_seed = pos.copy(), seed
        start = time.time()
        self.sampler_likelihood = likelihood
        sampler = DevicePTSampler(ctx, ntemps, W, betas=betas, Tmax=Tmax, seed=seed, capacity=self.nsteps, likelihood=likelihood)
        sampler.run_mcmc(pos, self.nsteps, lnlike0=ll)
        elapsed = time.time() - start
        self.log.info("Total time taken: %0.2f s" % elapsed)
        self.log.info("Time taken per step per walker: %0.2f ms" % (elapsed / (self.nsteps) * 1000. / (W * ntemps)))
        chain, lnp = sampler.chain[0], sampler.lnlikelihood[0]
        tau = max(integrated_time(chain[:, :, d].T) for d in range(ndim))
        burnin_step = int(tau * 3)
        if burnin_step > self.nsteps // 2:
            burnin_step = self.nsteps // 2
        self.log.info("Mean acceptance fraction: %0.2f" % (np.mean(sampler.acceptance_fraction[0])))
        self.log.info("AutoCorrelation Steps: %i, Number of Burn-in Steps: %i" % (np.round(tau), burnin_step))
        new_chain = np.zeros((W, self.nsteps, ndim + 1))
        new_chain[:, :, :-1] = chain
        self.chain = chain
        new_chain[:, :, -1] = lnp
        self.samples = new_chain[:, burnin_step:, :].reshape((-1, ndim + 1))
        self.pt_sampler = sampler
        self.log.info("Shape of self.samples")
        self.log.info(self.samples.shape)
        self.log.info("Median lnprob: %.5f; Max lnprob: %.5f" % (np.median(lnp), np.amax(lnp)))
        self.lnZ, self.dlnZ = sampler.thermodynamic_integration_log_evidence(fburnin)
        self.log.info("Temperatures: %d, Tmax %.4g; swap acceptance %.2f-%.2f" % (
            ntemps, 1.0 / sampler.betas[-1], np.min(sampler.tswap_acceptance_fraction, initial=1.0),
            np.max(sampler.tswap_acceptance_fraction, initial=0.0)))
        self.log.info("ln evidence: %.4f +/- %.4f" % (self.lnZ, self.dlnZ))
        return self.lnZ, self.dlnZ

    def _select_samples(self, lnprobcut, keep_lnprob):
        """Rows within lnprobcut of the maximum, doubling the cut until a quarter survive
        (lumfuncmcmc.py:548-553)."""
        nsamples = []
        while len(nsamples) < len(self.samples) // 4:
            sel = self.samples[:, -1] > (np.max(self.samples[:, -1], axis=0) - lnprobcut)
            nsamples = self.samples[sel, :] if keep_lnprob else self.samples[sel, :-1]
            lnprobcut *= 2.0
        self.log.info("Shape of nsamples (with a lnprobcut applied)")
        self.log.info(nsamples.shape)
        return nsamples

    def _posterior_rows(self, ndraws, lnprobcut):
        """ndraws random rows of the selected samples, drawn as set_median_fit draws them: _select_samples, then one
        np.random.randint per draw (numpy's global stream is consumed identically)."""
        nsamples = self._select_samples(lnprobcut, keep_lnprob=True)
        return np.array([nsamples[np.random.randint(0, nsamples.shape[0]), :] for _ in np.arange(ndraws)])

    def _band_device(self, device):
        return self._ctx is not None if device is None else bool(device)

    def deconvolved_luminosities(self, ndraws=200, lnprobcut=7.5, device=None):
        """Every source's posterior of its TRUE log-luminosity under the flux-error-convolved model, marginalised over
        ndraws random posterior draws (taken as lf_percentiles takes them; at most 4096): DESIGN.md section 3.22.  Returns a
        dict: lum_true = self.lum + shift, lum_true_e = sqrt(max(m2 - shift^2, 0)) - the spread of the mixture over the draws
        - shift = m1, the mean of (true - catalogued) in dex, and n_used, the draws whose plain lnprob is finite (0: NaN for
        every source with lum_e > 0); a source with lum_e = 0 keeps its luminosity with spread 0.  Needs deconvolve=True.
        device=True: the GPU (lf_lum_posterior), False: NumPy (deconv.lum_posterior); None = the GPU when this object
        already holds a device context.  self.lum and the tables are not touched."""
        if not self.deconvolve:
            raise ValueError("deconvolved_luminosities needs an object made with deconvolve=True")
        from . import deconv
        rows = self._posterior_rows(ndraws, lnprobcut)[:, :-1]
        if self._band_device(device):
            m1, m2, used = self.context().lum_posterior(rows)
        else:
            m1, m2, used = deconv.lum_posterior(self.kernel_inputs(), np.asarray(self.lum_e, dtype=np.float64), rows,
                                                K=self.deconvolve_order, wide=self.deconvolve_wide)
        with np.errstate(invalid="ignore"):
            spread = np.sqrt(np.maximum(m2 - m1 * m1, 0.0))
        return {"lum_true": np.asarray(self.lum, dtype=np.float64) + m1, "lum_true_e": spread, "shift": m1, "n_used": int(used)}

    def veff_deconvolved(self, percentiles=(16, 50, 84), ndraws=200, lnprobcut=7.5, method="linear", device=None, min_vol_frac=0.0):
        """The deconvolved 1/Veff points: per posterior draw, every source's posterior of its TRUE
        luminosity under the flux-error-convolved model, binned on VeffLF's bins with the completeness at the true flux, and
        the percentiles of every bin over the draws whose plain lnprob is finite (ndraws random draws, taken as lf_percentiles
        takes them; at most 4096).  Returns a dict: Lavg (nbins,), percentiles (nq, nbins) and values (ndraws, nbins; NaN for an
        unused draw) in dn/dlogL like lfbinorig, n_used, and var_post = np.var(values of the used draws, axis=0, ddof=1) - the
        posterior part of the points' variance; NaN when fewer than two draws are used (no variance can be formed).  Needs deconvolve=True (whose min_comp_frac <= 0.001 makes the volume one
        scalar).  device=True: the GPU (lf_veff_true), False: NumPy (deconv.veff_true_quantiles); None = the GPU when this
        object already holds a device context.  self.lum, var and lfbinorig are not touched.
        Under deconvolve_cut=True (min_comp_frac > 0.001) it needs deconvolve_cut_veff=True: every node's weight is then divided
        by g, the part of the survey volume in which its true luminosity is catalogued under the cut (deconvolve_cut_errors'
        model), nodes with g = 0 or g < min_vol_frac are dropped, and the dict gains n_dropped, the
        number of dropped (source, node) pairs."""
        if not self.deconvolve:
            raise ValueError("veff_deconvolved needs an object made with deconvolve=True")
        if self.deconvolve_cut and not self.deconvolve_cut_veff:
            raise NotImplementedError("veff_deconvolved is not implemented under deconvolve_cut=True: with min_comp_frac > 0.001 "
                                      "every source has its own volume (a z_max per source), and the deconvolved points take one")
        from . import deconv
        lfbands._method(method)
        rows = self._posterior_rows(ndraws, lnprobcut)[:, :-1]
        edges, Lavg, dL, _ = veff.luminosity_bins(self.lum, self.nbins)
        vol = float(veff.comoving_volume(self.dVdzf, self.zmin, self.zmax))
        pref0 = sum(self.Omega_0) / hs.SQARCSEC
        cut = self.deconvolve_cut_errors if self.deconvolve_cut else None
        if cut is None and min_vol_frac != 0.0:
            raise ValueError("min_vol_frac needs an object made with deconvolve_cut=True, deconvolve_cut_veff=True")
        dropped = None
        if self._band_device(device):
            ctx = self.context()
            out, values, used = ctx.veff_true(rows, edges, pref0, vol, q=percentiles, method=lfbands.METHODS[method],
                                              min_vol_frac=min_vol_frac)
            if cut is not None:
                dropped = ctx.veff_true_cut_info()["dropped"]
        else:
            sg = np.asarray(self.lum_e, dtype=np.float64)
            out, values, used = deconv.veff_true_quantiles(self.kernel_inputs(), sg, rows, edges, pref0, vol, q=percentiles, method=method,
                                                           K=self.deconvolve_order, wide=self.deconvolve_wide, cut=cut,
                                                           min_vol_frac=min_vol_frac)
            if cut is not None:
                dropped = deconv.cut_volume_table(self.kernel_inputs(), sg, cut, K=self.deconvolve_order, wide=self.deconvolve_wide,
                                                  min_vol_frac=min_vol_frac)[1]
        values = values / dL
        ok = ~np.all(np.isnan(values), axis=1)
        res = {"Lavg": Lavg, "percentiles": out / dL, "values": values, "n_used": int(used),
               "var_post": np.var(values[ok], axis=0, ddof=1) if ok.sum() > 1 else np.full(self.nbins, np.nan)}
        if dropped is not None:
            res["n_dropped"] = int(dropped)
        return res

    def _mock_generator(self, device):
        """MockGenerator (GPU) or MockTwin (NumPy) over this object's unsharded kernel_inputs(); device=None = the GPU when
        this object already holds a context.  The device generator is kept for the object's configuration."""
        if not self._band_device(device):
            return mock.MockTwin(self.kernel_inputs())
        key = (self._variant(), bool(self.fix_sch_al), float(self.sch_al) if self.fix_sch_al else None, self.device)
        if getattr(self, "_mock", None) is None or self._mock_key != key:
            self._mock = mock.MockGenerator(self.kernel_inputs(), device=self.device)
            self._mock_key = key
        return self._mock

    def error_model(self, nodes=16):
        """The error model this catalogue shows: (log10 flux nodes (M,), sigma (nf, M)) from
        mock.error_model_from_catalogue on log10(self.flux), self.lum_e and self.field_ind."""
        with np.errstate(divide="ignore", invalid="ignore"):
            logf = np.log10(np.asarray(self.flux, dtype=np.float64))
        return mock.error_model_from_catalogue(logf, self.lum_e, self.field_ind, nodes=nodes)

    def _noise_model(self, spec):
        """(nodes, sigma) of "catalogue" (self.error_model()) or of a (nodes, sigma) pair."""
        if isinstance(spec, str):
            if spec != "catalogue":
                raise ValueError("the error model must be \"catalogue\" or a (nodes, sigma) pair, got %r" % (spec,))
            return self.error_model()
        nodes, sigma = spec
        return mock.check_error_model(nodes, sigma, self.nfields)

    def _cut_model(self, spec, keyword):
        """(nodes, sigma) of the error model of a cut mock: `spec` as _noise_model takes it; None on a deconvolve_cut=True
        object: its deconvolve_cut_errors, so that the mock and the likelihood use one model."""
        if not self.min_comp_frac > 0.001:
            raise ValueError("cut=True needs min_comp_frac > 0.001: with min_comp_frac <= 0.001 the grid has one lower edge for "
                             "all redshifts, at min(lum), and there is no cut on the observed flux to draw")
        if spec is None and self.deconvolve_cut:
            return self.deconvolve_cut_errors
        pair = isinstance(spec, (tuple, list)) and len(spec) == 2 and np.ndim(spec[1]) == 2
        if not (isinstance(spec, str) or pair):
            raise ValueError("cut=True needs a flux-dependent error model: %s=\"catalogue\" or a (nodes, sigma) pair (a "
                             "deconvolve_cut=True object supplies its deconvolve_cut_errors by default), got %r" % (keyword, spec))
        return self._noise_model(spec)

    def _set_cut_process(self, gen, model):
        """the error model and the band of the cut process on a generator"""
        from . import deconv
        inp = self.kernel_inputs()
        gen.set_error_model(*model)
        H = mock.cut_depth(model[1], deconv.CUT_T)
        if not H > 0.0:
            raise ValueError("cut=True needs an error model with sigma > 0 somewhere: without errors no source crosses the cut")
        logLb = mock.band_grid(inp, H)
        gen.set_cut_band(logLb, None if inp["variant"] == "free" else mock.band_integ_part(inp, logLb))

    def mock_catalogue(self, theta, seed=None, device=None, lum_err=None, cut=False):
        """One catalogue drawn from the model at `theta`: the Poisson process whose likelihood
        lnprob evaluates, on this object's integration grid.  Returns the per-field lists both constructors take - z, lum,
        lum_e (zeros), field_ind - plus theta and seed.  seed=None draws one from numpy's global state (as fit_model does);
        device=True the GPU, False NumPy, None the GPU when this object already holds a device context (one GPU; with
        several ranks call it on one).  lum_err (dex; a scalar or one value per field): Gaussian measurement noise of that
        width is added to the drawn luminosities after detection - the model deconvolve=True fits -
        from a Philox stream of its own, on the host for both generators; lum_e is then filled and lum_true holds the
        noiseless values.  None: the output is what it was without the keyword, bit for bit.  lum_err="catalogue" (this
        catalogue's self.error_model()) or a (nodes, sigma) pair: the width is a function of the field and of the source's
        true log10 flux (section 3.23), lum_e holds every source's own sigma, and on the device path the noise is added on
        the GPU (the same stream and expression: the NumPy path agrees to the rounding of the device's cos and log1p).

        cut=True (needs min_comp_frac > 0.001 and a flux-dependent error model, by default the
        deconvolve_cut_errors of a deconvolve_cut=True object): a catalogue of the process deconvolve_cut=True models.  Sources
        are also drawn below the grid's lower edge, every source is observed with sigma at its true flux, and only those
        whose observed luminosity reaches the edge of their redshift column are returned (per field: those from above the
        edge, then those scattered in).  The lists also hold lum_true, n_candidates and n_scattered_in (per field: the
        sources drawn, and the returned ones whose lum_true lies below their edge).  cut=False: nothing changes."""
        if seed is None:
            seed = int(np.random.randint(0, 2 ** 31 - 1))
        theta = np.asarray(theta, dtype=np.float64).ravel()
        if cut:
            model = self._cut_model(lum_err, "lum_err")
            gen = self._mock_generator(device)
            self._set_cut_process(gen, model)
            z, lum, lobs, sg, fld, _, info = gen.draw_cut(theta[None], seed)
            out = mock.observed_lists(z, lum, lobs, sg, fld, self.nfields)
            out["n_candidates"], out["n_scattered_in"] = info["n_candidates"][0].copy(), info["n_scattered_in"][0].copy()
            out["theta"], out["seed"] = theta.copy(), int(seed)
            return out
        gen = self._mock_generator(device)
        # (a pair's sigma is two-dimensional, (nf, M): a sequence of two numbers stays one value per field)
        if isinstance(lum_err, str) or (isinstance(lum_err, (tuple, list)) and len(lum_err) == 2 and np.ndim(lum_err[1]) == 2):
            gen.set_error_model(*self._noise_model(lum_err))
            z, lum, lobs, sg, fld, _ = gen.draw_noisy(theta[None], seed)
            out = mock.observed_lists(z, lum, lobs, sg, fld, self.nfields)
        else:
            z, lum, fld, _ = gen.draw(theta[None], seed)
            out = mock.catalogue_lists(z, lum, fld, self.nfields, lum_err=lum_err, seed=seed)
        out["theta"], out["seed"] = theta.copy(), int(seed)
        return out

    def posterior_predictive(self, edges=None, ndraws=200, lnprobcut=7.5, seed=None, device=None, noise=None, cut=False,
                             z_edges=None):
        """Posterior predictive check of the observed luminosities per field: ndraws posterior rows (drawn as
        set_median_fit draws them), one mock catalogue each, binned in logL with `edges` (default: 20 equal bins over
        [min(lum), max(lum)]) by searchsorted(edges, x, side="right") - slot 0 below edges[0], slot B + 1 at or above
        edges[B].  Returns a dict: edges, observed [nf, B + 2], replicated [R, nf, B + 2], expected [R, nf] (the mocks'
        expected counts), percentiles (16, 50, 84) of replicated, p_upper = mean(rep >= obs) and p_lower = mean(rep <= obs)
        per bin, and the same for the per-field totals (observed_total, replicated_total, p_upper_total, p_lower_total).
        seed and device as mock_catalogue.

        noise: which luminosities of the replicates are binned.  None: the noiseless ones - the
        result without the keyword, bit for bit.  That is the right comparison for a plain fit (deconvolve=False), whose
        likelihood takes the catalogued luminosities for the true ones.  "catalogue" (self.error_model()) or a
        (nodes, sigma) pair: the replicates' observed luminosities, L_true + sigma n.  A deconvolve=True (or
        deconvolve_wide=True) posterior describes the true luminosities; the catalogue holds the observed ones, so its
        replicates are to be compared with the catalogue under noise="catalogue" - without it the check reports a
        bright-end excess that is only the Eddington bias the fit removed.  The dict also holds `noise` (None, "catalogue"
        or "model") and `sigma_model` (None or the (nodes, sigma) used).

        cut=True (as in mock_catalogue): the replicates are catalogues of the cut process - what a
        deconvolve_cut=True fit models, sources scattered in and out across the grid's lower edge included.  The dict then
        also holds `replicated_kept` [R, nf] and cut = True; `expected` stays the count above the edge before the observation
        (B; the cut process expects B + Delta B).  noise=None then means the object's deconvolve_cut_errors.

        z_edges: None - the check in logL alone, the result without the keyword, key for key and bit
        for bit.  An array of redshift edges, or "auto" (10 equal bins over [zmin, zmax]): the replicates are binned in
        (z, logL) as well - redshift slots as the logL slots, searchsorted(z_edges, z, side="right"); the replicates'
        redshifts carry no noise - and the dict gains z_edges, observed_2d [nf, nz + 2, B + 2], replicated_2d
        [R, nf, nz + 2, B + 2], percentiles_2d, p_upper_2d, p_lower_2d per cell, the N(z) marginal per field observed_z,
        replicated_z, percentiles_z, p_upper_z, p_lower_z, and one omnibus statistic per field, so that nobody has to pick
        among nz x B p-values: deviance = D(observed), D(h) = 2 sum_cells [m - h + h ln(h / m)] with m the replicates' mean
        of the cell (cells with m = 0 are left out: n_empty_cells counts them and observed_in_empty the observed sources
        in them), replicated_deviance [R, nf] and p_deviance = mean(replicated_deviance >= deviance).  The entries in logL
        alone are then the 2-D histogram's marginal: the same integers as without z_edges for the same seed.  noise= and
        cut= keep their meaning."""
        model = self._cut_model(noise, "noise") if cut else None
        rows = self._posterior_rows(ndraws, lnprobcut)[:, :-1]
        if edges is None:
            edges = np.linspace(np.min(self.lum), np.max(self.lum), 21)
        if seed is None:
            seed = int(np.random.randint(0, 2 ** 31 - 1))
        gen = self._mock_generator(device)
        if cut:
            self._set_cut_process(gen, model)
        elif noise is not None:
            model = self._noise_model(noise)
            gen.set_error_model(*model)
        fi = np.asarray(self.field_ind, dtype=np.int64)
        if z_edges is None:
            out = mock.predictive(gen, rows, edges, self.lum, fi, seed, noisy=noise is not None, cut=cut)
        else:
            if isinstance(z_edges, str):
                if z_edges != "auto":
                    raise ValueError("z_edges must be None, \"auto\" or an array of redshift edges, got %r" % (z_edges,))
                z_edges = np.linspace(self.zmin, self.zmax, 11)
            out = mock.predictive2(gen, rows, z_edges, edges, self.z, self.lum, fi, seed, noisy=noise is not None, cut=cut)
        out["noise"] = ("model" if cut else None) if noise is None else ("catalogue" if isinstance(noise, str) else "model")
        out["sigma_model"] = model
        if cut:
            out["cut"] = True
        return out

    def add_fitinfo_to_table(self, percentiles, start_value=1, lnprobcut=7.5):
        """Percentiles of each parameter into the last row of self.table (lumfuncmcmc.py:653-667)."""
        nsamples = self._select_samples(lnprobcut, keep_lnprob=False)
        n = len(percentiles)
        for i, per in enumerate(percentiles):
            for j, v in enumerate(np.percentile(nsamples, per, axis=0)):
                self.table[-1][(i + start_value + j * n)] = v

    def _veff(self, sum_Omega, zmaxval, device):
        if device is None:
            device = self._ctx is not None
        if device:
            vol = veff.comoving_volume(self.dVdzf, self.zmin, zmaxval)
            self.phifunc, self.Lavg, self.lfbinorig, self.var = veff.veff_device(
                self.lum, self.flux, 1.0e-17 * self.Flims_arr, vol, sum_Omega, self.alpha, self.fcmin,
                nboot=self.nboot, nbin=self.nbins, device=self.device)
            return
        self.phifunc = veff.lumfunc_weights(self.flux, self.dVdzf, sum_Omega, self.zmin, zmaxval,
                                            1.0e-17 * self.Flims_arr, self.alpha, self.fcmin)
        self.Lavg, self.lfbinorig, self.var = veff.boot_err_log(self.lum, self.phifunc, self.nboot, self.nbins)

    def _veff_or_skip(self):
        try:
            self.VeffLF()
        except NotImplementedError as e:
            self.log.warning("skipping the 1/Veff estimate: %s" % e)
            self.Lavg = self.lfbinorig = self.var = None

    SLICE_NODES = 8                # Gauss-Legendre nodes per redshift slice of veff_slices' model band

    def veff_slices(self, z_edges="auto", bins="common", device=None, model=True, percentiles=(16, 50, 84), ndraws=200, lnprobcut=7.5):
        """The 1/Veff points in redshift slices, next to the model averaged over the same slices (DESIGN.md section 3.36;
        VmaxLumFunc.zEvolSteps).  z_edges: S + 1 increasing redshifts inside [zmin, zmax], an integer S for S equal-count
        slices (veff.slice_edges), or "auto" = 5.  A source's volume runs from its slice's lower edge to the upper edge or to
        its own z_max (VeffLF's), whichever is lower; every slice is resampled on its own, nboot times.  bins="common": the
        luminosity bins of the whole catalogue for every slice; "slice": each slice's own, as the reference has them.
        Returns a dict: z_edges (S + 1,), Lavg (S, nbins), lf, var (S, nbins) in dn/dlogL like lfbinorig and var, counts
        (S, nbins), n_slice (S,), seed (the bootstrap's, drawn from numpy's global state), and with model=True also model
        (len(percentiles), S, nbins): the percentiles over ndraws posterior draws (taken as lf_percentiles takes them) of the
        model LF at Lavg, averaged over the slice with the weight dV/dz - for LumFuncMCMC, which has no z dependence,
        lf_percentiles at Lavg.  device=True: the GPU (lf_veff_slices, a fixed order of summation), False: NumPy; None = the
        GPU when this object already holds a device context.  self.Lavg, self.lfbinorig and self.var are not touched."""
        if isinstance(z_edges, str):
            if z_edges != "auto":
                raise ValueError("z_edges must be 'auto', a number of slices or the edges themselves, not %r" % (z_edges,))
            z_edges = 5
        edges = veff.slice_edges(self.z, z_edges) if np.ndim(z_edges) == 0 else np.asarray(z_edges, dtype=np.float64)
        if edges[0] < self.zmin or edges[-1] > self.zmax:
            raise ValueError("z_edges must lie inside [zmin, zmax] = [%r, %r]" % (self.zmin, self.zmax))
        slice_of = veff.slice_index(self.z, edges)
        S = edges.size - 1
        vol = veff.slice_volumes(self.dVdzf, edges, slice_of, self._veff_zmaxval())
        dev = self._band_device(device)
        seed = int(np.random.randint(0, 2 ** 31 - 1))
        run = veff.veff_slices_device if dev else veff.veff_slices_host
        _, Lavg, lf, var, counts, n_slice = run(self.lum, self.flux, 1.0e-17 * self.Flims_arr, vol, slice_of, S, sum(self.Omega_0),
                                                self.alpha, self.fcmin, nboot=self.nboot, nbin=self.nbins, bins=bins, seed=seed,
                                                **({"device": self.device} if dev else {}))
        out = {"z_edges": edges, "Lavg": Lavg, "lf": lf, "var": var, "counts": counts, "n_slice": n_slice, "seed": seed}
        if model:
            nobin = np.isnan(Lavg)                                  # (bins="slice": a slice without bins)
            band = self._slice_band(edges, np.where(nobin, 0.0, Lavg), percentiles, ndraws, lnprobcut, dev)
            band[:, nobin] = np.nan
            out["model"] = band
        return out

    def _slice_band(self, edges, Lavg, percentiles, ndraws, lnprobcut, dev):
        """(nq, S, nbins): without a z dependence the slice average is the model itself"""
        band = self.lf_percentiles(percentiles=percentiles, logL=Lavg.ravel(), ndraws=ndraws, lnprobcut=lnprobcut, device=dev)
        return band.reshape((band.shape[0],) + Lavg.shape)

    def close(self):
        # (a device sampler holds its context's handle: it goes first; what it read back stays on it)
        for s in (getattr(self, "sampler", None), getattr(self, "pt_sampler", None)):
            if hasattr(s, "close"):
                s.close()
        if self._ctx is not None:
            self._ctx.close()
            self._ctx = None
        if getattr(self, "_mock", None) is not None:
            self._mock.close()
            self._mock = None


class LumFuncMCMC(_Base):
    """Single-Schechter fit with free or fixed completeness parameters (lumfuncmcmc.py:72)."""

    def __init__(self, z, flux=None, flux_e=None, Flim=[2.35, 3.12, 2.20, 2.86, 2.85], Flim_lims=[1.0, 6.0],
                 alpha=3.5, alpha_lims=[1.0, 6.0], line_name="OIII",
                 line_plot_name=r'[OIII] $\lambda 5007$', lum=None, lum_e=None,
                 Omega_0=[100.0, 100.0, 100.0, 100.0, 100.0], nbins=50,
                 nboot=100, sch_al=-1.6, sch_al_lims=[-3.0, 1.0], Lstar=42.5, Lstar_lims=[40.0, 45.0],
                 phistar=-3.0, phistar_lims=[-8.0, 5.0], Lc=40.0, Lh=46.0, nwalkers=100, nsteps=1000,
                 fix_sch_al=False, fcmin=0.1, fix_comp=False, min_comp_frac=0.5,
                 field_names=None, field_ind=None, diff_rand=True, device=0, compress=False, shard="walkers",
                 deconvolve=False, deconvolve_order=None, deconvolve_tile=False, deconvolve_wide=False,
                 deconvolve_cut=False, deconvolve_cut_errors=None, deconvolve_cut_grad=False, deconvolve_cut_veff=False):
        self._common_init(z, flux, flux_e, lum, lum_e)
        self.device = device
        self.compress = bool(compress)
        self.shard = self._check_shard(shard)
        self.fcmin, self.min_comp_frac = fcmin, min_comp_frac
        self.Flim, self.Flim_lims = Flim, Flim_lims
        self.fields, self.nfields = field_names, len(self.Flim)
        self.field_ind = field_ind
        self.alpha, self.alpha_lims = alpha, alpha_lims
        self.line_name, self.line_plot_name = line_name, line_plot_name
        self.Lc, self.Lh = Lc, Lh
        self.Omega_0 = Omega_0
        self.nbins, self.nboot = nbins, nboot
        self.sch_al, self.sch_al_lims = sch_al, sch_al_lims
        self.Lstar, self.Lstar_lims = Lstar, Lstar_lims
        self.phistar, self.phistar_lims = phistar, phistar_lims
        self.nwalkers, self.nsteps = nwalkers, nsteps
        self.fix_sch_al, self.fix_comp = fix_sch_al, fix_comp
        self.all_param_names = ['Lstar', 'phistar', 'sch_al', 'Flim', 'alpha']
        self.diff_rand = diff_rand
        self._Flim0, self._alpha0 = list(Flim), alpha          # the fixed completeness of this object
        self.defineFlimOmArr()
        self.getRoot()
        self.setDLdVdz()
        self._fluxes_and_lums(flux, flux_e, lum, lum_e)
        self._Omegaf = None
        self.roots_ln = self.rootsf.ev(self.Flim, self.alpha)
        self.allind = np.arange(len(self.lum))
        self.size_ln = 201 if self.fix_comp else 101
        self.setlnsimple(need_integ=bool(self.fix_comp))
        self.setup_logging()
        self._init_deconvolve(deconvolve, deconvolve_order, deconvolve_tile, deconvolve_wide, deconvolve_cut, deconvolve_cut_errors,
                              deconvolve_cut_grad, deconvolve_cut_veff)

    def getRoot(self, size=201):
        self.rootsf = hs.completeness_roots(self.Flim_lims, self.alpha_lims, self.fcmin, self.min_comp_frac, size)

    def _setup_roots(self):
        return self.rootsf.ev(self.Flim, self.alpha)

    def _variant(self):
        return "fixcomp" if self.fix_comp else "free"

    def _lnprob_name(self):
        return 'lnprob_fix_comp' if self.fix_comp else 'lnprob'

    def set_parameters_from_list(self, input_list):
        """theta -> named attributes (lumfuncmcmc.py:320-337); kept for the post-processing code,
        the kernels unpack theta themselves."""
        self.Lstar, self.phistar = input_list[0], input_list[1]
        k = 2
        if not self.fix_sch_al:
            self.sch_al = input_list[2]
            k = 3
        if not self.fix_comp:
            self.Flim, self.alpha = input_list[k:k + self.nfields], input_list[k + self.nfields]

    def lnprob(self, theta):
        """log posterior, completeness free (lumfuncmcmc.py:395-409).  theta: (ndim,) -> float, or
        (B, ndim) -> (B,) in one device call."""
        if self.fix_comp:
            raise ValueError("this object was built with fix_comp=True: call lnprob_fix_comp")
        return self._evaluate(theta)

    def lnprob_fix_comp(self, theta):
        """log posterior, completeness fixed (lumfuncmcmc.py:411-424)."""
        if not self.fix_comp:
            raise ValueError("this object was built with fix_comp=False (S=101 grid): call lnprob")
        return self._evaluate(theta)

    def _theta_lims(self):
        lims = [self.Lstar_lims, self.phistar_lims]
        if not self.fix_sch_al:
            lims.append(self.sch_al_lims)
        if not self.fix_comp:
            lims += [self.Flim_lims] * self.nfields + [self.alpha_lims]
        return np.array(lims, dtype=np.float64)

    def get_param_names(self):
        names = [r'$\log L_*$', r'$\log \phi_*$']
        if not self.fix_sch_al:
            names += [r'$\alpha$']
        if not self.fix_comp:
            names += [r'$F_{{\rm 50},%d}$' % (i) for i in range(self.nfields)] + [r'$\alpha_C$']
        return names

    def get_params(self):
        vals = [self.Lstar, self.phistar]
        if not self.fix_sch_al:
            vals += [self.sch_al]
        if not self.fix_comp:
            vals += list(self.Flim) + [self.alpha]
        self.nfreeparams = len(vals)
        return vals

    def set_median_fit(self, rndsamples=200, lnprobcut=7.5, device=False):
        """Median model LF over random posterior draws, then the 1/Veff estimate (lumfuncmcmc.py:527-567).  device=True
        takes the rndsamples TrueLumFunc evaluations and their median on the GPU (lf_lumfunc_quantiles, LF_Q_MEDIAN); the
        draws, the median Flim / alpha and VeffLF are the same either way."""
        nsamples = self._select_samples(lnprobcut, keep_lnprob=True)
        Flims, alphas = np.zeros((rndsamples, self.nfields)), np.zeros(rndsamples)
        lf, recs = [], []
        for i in np.arange(rndsamples):
            ind = np.random.randint(0, nsamples.shape[0])
            self.set_parameters_from_list(nsamples[ind, :])
            Flims[i], alphas[i] = self.Flim, self.alpha
            if device:
                recs.append((self.Lstar, self.phistar, self.sch_al))
            else:
                lf.append(TrueLumFunc(self.lum, self.sch_al, self.Lstar, self.phistar))
        if device:
            self.medianLF = lfbands.quantiles_device(self._variant(), recs, self.lum, method="median", device=self.device)[0]
        else:
            self.medianLF = np.median(np.array(lf), axis=0)
        self.Flim, self.alpha = list(np.median(Flims, axis=0)), np.median(alphas)
        self._veff_or_skip()

    def lf_percentiles(self, percentiles=(16, 50, 84), logL=None, ndraws=200, lnprobcut=7.5, method="linear", device=None):
        """Percentiles over ndraws random posterior draws of the model LF at logL (default: every source, self.lum):
        (nq, P), np.percentile's rule ("linear") or np.median's ("median": one row, percentiles ignored).  The draws are
        taken as set_median_fit takes them.  device=True: the GPU (lf_lumfunc_quantiles), False: NumPy; None = the GPU
        when this object already holds a device context."""
        lfbands._method(method)
        rows = self._posterior_rows(ndraws, lnprobcut)
        recs = lfbands.pack_draws(self._variant(), rows, fix_sch_al=self.fix_sch_al, sch_al=self.sch_al)
        logL = self.lum if logL is None else np.asarray(logL, dtype=np.float64)
        return lfbands.quantiles(self._variant(), recs, logL, q=percentiles, method=method, device=self._band_device(device),
                                 device_index=self.device)

    def lf_integrals(self, kind="lumdens", logLmin=None, percentiles=(16, 50, 84), ndraws=200, lnprobcut=7.5, method="linear",
                     device=None):
        """Percentiles over ndraws random posterior draws of the integrated LF above each logLmin (default [self.Lc]):
        kind "number" = n(>L) [Mpc^-3], "lumdens" = rho(>L) [erg s^-1 Mpc^-3] (lfintegrals).
        Returns (nq, P).  Draws, lnprobcut, method and device as lf_percentiles."""
        lfbands._method(method)
        lfintegrals._kind(kind)
        rows = self._posterior_rows(ndraws, lnprobcut)
        recs = lfbands.pack_draws(self._variant(), rows, fix_sch_al=self.fix_sch_al, sch_al=self.sch_al)
        logLmin = np.atleast_1d(np.asarray(self.Lc if logLmin is None else logLmin, dtype=np.float64)).ravel()
        return lfintegrals.quantiles(self._variant(), kind, recs, logLmin, q=percentiles, method=method,
                                     device=self._band_device(device), device_index=self.device)

    def veff_percentiles(self, percentiles=(16, 50, 84), ndraws=200, lnprobcut=7.5, method="linear", device=None, volumes="fixed"):
        """The 1/Veff points marginalised over the completeness posterior: the binned 1/Veff LF of
        the catalogue under the Flim and alpha of each of ndraws random posterior draws (taken as lf_percentiles takes
        them), on the bins of VeffLF.  Returns a dict: Lavg (nbins,), percentiles (nq, nbins) and values (ndraws, nbins) in
        dn/dlogL like lfbinorig, and var_comp = np.var(values, axis=0, ddof=1) - the completeness part of the points'
        variance, to be added to the bootstrap self.var by whoever wants a total (self.var, Flim and alpha are not
        touched).  The volumes are VeffLF's: shared by all sources for min_comp_frac <= 0.001 (exact); otherwise
        volumes="fixed" takes each source's volume out to the z_max of the object's CURRENT Flim and alpha and holds it
        over the draws, volumes="per_draw" ends it at the z_max of each draw's own flux cut, the root of
        fleming = min_comp_frac at the draw's Flim and alpha (on the device from a validated table
        of the volume, on the host by one inversion per source and draw).  method and device as lf_percentiles."""
        if self.fix_comp:
            raise ValueError("this object was built with fix_comp=True: there is no completeness posterior to marginalise over")
        if volumes not in ("fixed", "per_draw"):
            raise ValueError("volumes must be 'fixed' or 'per_draw', not %r" % (volumes,))
        lfbands._method(method)
        rows = self._posterior_rows(ndraws, lnprobcut)
        k = 2 if self.fix_sch_al else 3                        # theta's layout: set_parameters_from_list
        draws = np.column_stack([1.0e-17 * rows[:, k:k + self.nfields], rows[:, k + self.nfields]])
        self.getFlim()
        field = np.repeat(np.arange(self.nfields), np.diff(self.field_ind))
        _, Lavg, dL, idx = veff.luminosity_bins(self.lum, self.nbins)
        pref0 = sum(self.Omega_0) / hs.SQARCSEC
        dev = self._band_device(device)
        if volumes == "per_draw" and self.min_comp_frac > 0.001:
            fmin = self.rootsf.ev(rows[:, k:k + self.nfields], rows[:, k + self.nfields][:, None])
            table = self._volume_table() if dev else None
            out, values = veff.veff_draws_zmax_quantiles(self.lum, self.flux, field, fmin, self.zmin, self.zmax, self.dVdzf, _cosmo,
                                                         pref0, self.fcmin, idx, self.nbins, draws, q=percentiles, method=method,
                                                         device=dev, device_index=self.device, table=table)
        else:                                                  # without a flux cut the roots are 0: the shared volume is exact
            if self.min_comp_frac <= 0.001:
                zmaxval = self.zmax
            else:
                root = self.rootsf.ev(self.Flims_arr, self.alpha)
                zmaxval = np.minimum(self.zmax, veff.max_redshift(10 ** self.lum, root, _cosmo))
            vol = veff.comoving_volume(self.dVdzf, self.zmin, zmaxval)
            out, values = veff.veff_draws_quantiles(self.flux, field, vol, pref0, self.fcmin, idx, self.nbins,
                                                    draws, q=percentiles, method=method, device=dev, device_index=self.device)
        values = values / dL
        return {"Lavg": Lavg, "percentiles": out / dL, "values": values,
                "var_comp": np.var(values, axis=0, ddof=1) if len(values) > 1 else np.zeros(self.nbins)}

    def _volume_table(self):
        """The device's table of the volume out to a luminosity distance (voltable), built and validated once per
        (zmin, zmax); refused when it misses the 1e-13 of V_total it is documented to hold."""
        from . import voltable
        key = (float(self.zmin), float(self.zmax))
        if getattr(self, "_voltable", None) is None or self._voltable[0] != key:
            self._voltable = (key, voltable.require(voltable.build(_cosmo, self.dVdzf, self.zmin, self.zmax)))
        return self._voltable[1]

    def VeffLF(self, device=None):
        """1/Veff weights per source and the binned LF with bootstrap errors (lumfuncmcmc.py:515-525).  device=True
        runs weights, binning and bootstrap on the GPU (lf_veff; resamples drawn with Philox instead of numpy's global
        state), False on the host; None = the GPU when this object already holds a device context."""
        self._veff(sum(self.Omega_0), self._veff_zmaxval(), device)

    def _veff_zmaxval(self):
        """Where a source's volume ends: zmax, or its own z_max under the flux cut of min_comp_frac, clipped to zmax"""
        self.getFlim()
        if self.min_comp_frac <= 0.001:
            return self.zmax
        root = self.rootsf.ev(self.Flims_arr, self.alpha)
        return np.minimum(self.zmax, veff.max_redshift(10 ** self.lum, root, _cosmo))

    def triangle_plot(self, outname, lnprobcut=7.5, imgtype='png'):
        """lumfuncmcmc.py:604-651.  The figure itself (corner + matplotlib) is outside the scope of this build; what the
        drivers write AFTER it is not: with configLF's default output_dict they call this right after fit_model()
        (run_lumfuncmcmc.py:291-293) and then read medianLF, Lavg, lfbinorig, var.  So everything the reference's
        add_subplots computes on the way (:576-603: median LF over random posterior draws, median Flim / alpha, roots_ln,
        VeffLF) is computed here, the skipped figure is logged, and the finished chain is kept."""
        self.set_median_fit(lnprobcut=lnprobcut)
        self.roots_ln = self.rootsf.ev(self.Flim, self.alpha)
        self.log.warning("triangle_plot: %s.%s not drawn (plotting is outside the scope of this build); "
                         "medianLF, Flim, alpha, roots_ln and the 1/Veff estimate are set as the figure's code would set them" % (outname, imgtype))


class LumFuncMCMCz(_Base):
    """Schechter fit whose log L* and log phi* are quadratics in z through three pivots
    (lumfuncmcmc_z.py:118); completeness is always fixed in this class."""

    _logger_name = 'lumfuncmcmc_z'

    def __init__(self, z, flux=None, flux_e=None, Flim=[2.35, 3.12, 2.20, 2.86, 2.85],
                 alpha=3.5, line_name="OIII",
                 line_plot_name=r'[OIII] $\lambda 5007$', lum=None, lum_e=None,
                 Omega_0=[100.0, 100.0, 100.0, 100.0, 100.0], nbins=50,
                 nboot=100, sch_al=-1.6, sch_al_lims=[-3.0, 1.0], Lstar=42.5, Lstar_lims=[41.0, 45.0],
                 phistar=-3.0, phistar_lims=[-8.0, 5.0], Lc=40.0, Lh=46.0, nwalkers=100, nsteps=1000,
                 fcmin=0.1, min_comp_frac=0.5, field_names=None,
                 field_ind=None, z1=1.20, z2=1.53, z3=1.86, fix_sch_al=False, device=0, compress=False, shard="walkers",
                 deconvolve=False, deconvolve_order=None, deconvolve_tile=False, deconvolve_wide=False,
                 deconvolve_cut=False, deconvolve_cut_errors=None, deconvolve_cut_grad=False, deconvolve_cut_veff=False):
        self._common_init(z, flux, flux_e, lum, lum_e)
        self.device = device
        self.compress = bool(compress)
        self.shard = self._check_shard(shard)
        self.z1, self.z2, self.z3 = z1, z2, z3
        self.fcmin, self.min_comp_frac = fcmin, min_comp_frac
        self.Flim = Flim
        self.fields, self.nfields = field_names, len(self.Flim)
        self.field_ind = field_ind
        self.alpha = alpha
        self.line_name, self.line_plot_name = line_name, line_plot_name
        self.Lc, self.Lh = Lc, Lh
        self.Omega_0 = Omega_0
        self.fix_sch_al = fix_sch_al
        self.nbins, self.nboot = nbins, nboot
        self.sch_al, self.sch_al_lims = sch_al, sch_al_lims
        self.Lstar, self.Lstar_lims = Lstar, Lstar_lims
        self.phistar, self.phistar_lims = phistar, phistar_lims
        # six draws from the global state, as the reference makes before anything else (:206-207)
        self.L1, self.L2, self.L3 = np.random.uniform(self.Lstar_lims[0] + 0.5, self.Lstar_lims[-1] - 0.5, 3)
        self.phi1, self.phi2, self.phi3 = np.random.uniform(self.phistar_lims[0] + 3, self.phistar_lims[-1] - 3, 3)
        self.nwalkers, self.nsteps = nwalkers, nsteps
        self._Flim0, self._alpha0 = list(Flim), alpha
        self.getRoot()
        self.defineFlimOmArr()
        self.setDLdVdz()
        self._fluxes_and_lums(flux, flux_e, lum, lum_e)
        self._Omegaf = None
        self.allind = np.arange(len(self.lum))
        self.size_ln = 201
        self.setlnsimple(need_integ=True)
        self.setup_logging()
        self._init_deconvolve(deconvolve, deconvolve_order, deconvolve_tile, deconvolve_wide, deconvolve_cut, deconvolve_cut_errors,
                              deconvolve_cut_grad, deconvolve_cut_veff)

    def getRoot(self):
        """Per-field flux at which the completeness equals min_comp_frac (lumfuncmcmc_z.py:292-297);
        only read when min_comp_frac > 0.001."""
        self.roots_ln = np.zeros(self.nfields)
        if self.min_comp_frac > 0.001:
            from scipy.optimize import fsolve
            for i in range(self.nfields):
                self.roots_ln[i] = fsolve(lambda x: hs.fleming(x, 1.0e-17 * self.Flim[i], self.alpha, self.fcmin)
                                          - self.min_comp_frac, [1.0e-17 * self.Flim[i]])[0]

    def _setup_roots(self):
        return self.roots_ln

    def defineFlimOmArr(self):
        _Base.defineFlimOmArr(self)
        self.roots_arr = np.zeros(self.field_ind[-1])
        for ii in range(self.nfields):
            self.roots_arr[self.field_ind[ii]:self.field_ind[ii + 1]] = self.roots_ln[ii]

    def _variant(self):
        return "zevol"

    def set_parameters_from_list(self, input_list):
        self.L1, self.L2, self.L3 = input_list[0], input_list[1], input_list[2]
        self.phi1, self.phi2, self.phi3 = input_list[3], input_list[4], input_list[5]
        if not self.fix_sch_al:
            self.sch_al = input_list[6]

    def lnprob(self, theta):
        """log posterior (lumfuncmcmc_z.py:378-392).  theta: (ndim,) -> float or (B, ndim) -> (B,)."""
        return self._evaluate(theta)

    def _theta_lims(self):
        lims = [self.Lstar_lims] * 3 + [self.phistar_lims] * 3
        if not self.fix_sch_al:
            lims.append(self.sch_al_lims)
        return np.array(lims, dtype=np.float64)

    def get_init_walker_values(self, num=None):
        lims = self._theta_lims()
        if num is None:
            num = self.nwalkers
        return np.random.rand(num, len(lims)) * (lims[:, 1] - lims[:, 0]) + lims[:, 0]

    def get_param_names(self):
        names = [r'$\log {\rm{L}}1_*$', r'$\log {\rm{L}}2_*$', r'$\log {\rm{L}}3_*$',
                 r'$\log \phi1_*$', r'$\log \phi2_*$', r'$\log \phi3_*$']
        if not self.fix_sch_al:
            names += [r'$\alpha$']
        return names

    def get_params(self):
        vals = [self.L1, self.L2, self.L3, self.phi1, self.phi2, self.phi3]
        if not self.fix_sch_al:
            vals += [self.sch_al]
        self.nfreeparams = len(vals)
        return vals

    def set_median_fit(self, lnprobcut=7.5, zlen=100, Llen=100):
        """Median-parameter LF surface on a (z, L) mesh, then the 1/Veff estimate (lumfuncmcmc_z.py:480-513)."""
        nsamples = self._select_samples(lnprobcut, keep_lnprob=False)
        self.Lout = np.linspace(min(self.lum) - 0.2, max(self.lum) + 0.2, Llen)
        self.zout = np.linspace(self.zmin, self.zmax, zlen)
        self.medianLF = np.zeros((zlen, Llen))
        self.set_parameters_from_list(np.percentile(nsamples, 50.0, axis=0))
        for i in np.arange(zlen):
            self.medianLF[i] = schechter_z(self.Lout, self.zout[i], self.sch_al, self.L1, self.L2, self.L3,
                                           self.phi1, self.phi2, self.phi3, self.z1, self.z2, self.z3)
        self._veff_or_skip()

    def lf_percentiles(self, percentiles=(16, 50, 84), logL=None, z=None, ndraws=200, lnprobcut=7.5, method="linear",
                       device=None):
        """Posterior band of the z-evolving LF: percentiles over ndraws random posterior draws (taken as
        LumFuncMCMC.set_median_fit takes them) on the (z, logL) mesh - by default set_median_fit's (zout, Lout, 100 x 100).
        Returns (nq, len(z), len(logL)).  method and device as LumFuncMCMC.lf_percentiles."""
        lfbands._method(method)
        if logL is None:
            logL = np.linspace(min(self.lum) - 0.2, max(self.lum) + 0.2, 100)
        if z is None:
            z = np.linspace(self.zmin, self.zmax, 100)
        logL, z = np.asarray(logL, dtype=np.float64).ravel(), np.asarray(z, dtype=np.float64).ravel()
        rows = self._posterior_rows(ndraws, lnprobcut)
        recs = lfbands.pack_draws("zevol", rows, fix_sch_al=self.fix_sch_al, sch_al=self.sch_al, pivots=(self.z1, self.z2, self.z3))
        Lp = np.tile(logL, z.size)
        zp = np.repeat(z, logL.size)
        out = lfbands.quantiles("zevol", recs, Lp, z=zp, q=percentiles, method=method, device=self._band_device(device),
                                device_index=self.device)
        return out.reshape(out.shape[0], z.size, logL.size)

    def lf_integrals(self, kind="lumdens", logLmin=None, z=None, percentiles=(16, 50, 84), ndraws=200, lnprobcut=7.5,
                     method="linear", device=None):
        """Posterior band of the integrated z-evolving LF, n(>L; z) or rho(>L; z): percentiles over ndraws random
        posterior draws at the redshifts z (default: 100 values across [zmin, zmax]) above logLmin (default self.Lc; a
        scalar is broadcast over z, an array pairs with z).  Returns (nq, len(z)).  Otherwise as
        LumFuncMCMC.lf_integrals."""
        lfbands._method(method)
        lfintegrals._kind(kind)
        if z is None:
            z = np.linspace(self.zmin, self.zmax, 100)
        z = np.atleast_1d(np.asarray(z, dtype=np.float64)).ravel()
        logLmin = np.asarray(self.Lc if logLmin is None else logLmin, dtype=np.float64)
        logLmin = np.ascontiguousarray(np.broadcast_to(logLmin.ravel() if logLmin.ndim else logLmin, z.shape))
        rows = self._posterior_rows(ndraws, lnprobcut)
        recs = lfbands.pack_draws("zevol", rows, fix_sch_al=self.fix_sch_al, sch_al=self.sch_al, pivots=(self.z1, self.z2, self.z3))
        return lfintegrals.quantiles("zevol", kind, recs, logLmin, z=z, q=percentiles, method=method,
                                     device=self._band_device(device), device_index=self.device)

    def VeffLF(self, device=None):
        """lumfuncmcmc_z.py:470-478 (device: see LumFuncMCMC.VeffLF)."""
        self._veff(sum(self.Omega_0), self._veff_zmaxval(), device)

    def _veff_zmaxval(self):
        if self.min_comp_frac <= 0.001:
            return self.zmax
        return np.minimum(self.zmax, veff.max_redshift(10 ** self.lum, self.roots_arr, _cosmo))

    def _slice_band(self, edges, Lavg, percentiles, ndraws, lnprobcut, dev):
        """(nq, S, nbins): per posterior draw the model LF at SLICE_NODES Gauss-Legendre redshifts of every slice, averaged
        with the weights w_g dV/dz(z_g) (veff.slice_model_average); np.percentile over the draws."""
        rows = self._posterior_rows(ndraws, lnprobcut)
        recs = lfbands.pack_draws("zevol", rows, fix_sch_al=self.fix_sch_al, sch_al=self.sch_al, pivots=(self.z1, self.z2, self.z3))
        zg, wg = veff.slice_nodes(edges, self.SLICE_NODES)
        S, G, nb = zg.shape[0], zg.shape[1], Lavg.shape[1]
        Lp = np.ascontiguousarray(np.broadcast_to(Lavg[:, None, :], (S, G, nb))).ravel()
        zp = np.ascontiguousarray(np.broadcast_to(zg[:, :, None], (S, G, nb))).ravel()
        if dev:
            values = lfbands.quantiles_device("zevol", recs, Lp, z=zp, q=percentiles, values=True, device=self.device)[1]
        else:
            values = lfbands.lf_values("zevol", recs, Lp, z=zp)
        avg = veff.slice_model_average(values.reshape(-1, S, G, nb), wg * self.dVdzf(zg))
        return np.percentile(avg, np.atleast_1d(np.asarray(percentiles, dtype=np.float64)), axis=0)

    def triangle_plot(self, outname, lnprobcut=7.5, imgtype='png'):
        """lumfuncmcmc_z.py:546-585.  As for LumFuncMCMC.triangle_plot: the figure is out of scope, the numbers its code
        leaves behind for the driver (run_lumfuncmcmc_z.py:264-281: Lout, zout, medianLF on the mesh of add_subplots
        :524-533, VeffLF) are made, the skipped figure is logged."""
        nsamples = self._select_samples(lnprobcut, keep_lnprob=True)
        zlen = Llen = 100
        self.Lout = np.linspace(min(self.lum) - 0.08, max(self.lum) + 0.01, Llen)
        self.zout = np.linspace(self.zmin, self.zmax, zlen)
        self.medianLF = np.zeros((zlen, Llen))
        # (the reference takes the medians of nsamples WITH its lnprob column here and hands the list to
        # set_parameters_from_list, which reads the leading entries only)
        self.set_parameters_from_list(np.percentile(nsamples, 50.0, axis=0))
        for i in np.arange(zlen):
            self.medianLF[i] = schechter_z(self.Lout, self.zout[i], self.sch_al, self.L1, self.L2, self.L3,
                                           self.phi1, self.phi2, self.phi3, self.z1, self.z2, self.z3)
        self._veff_or_skip()
        self.log.warning("triangle_plot: %s.%s not drawn (plotting is outside the scope of this build); "
                         "Lout, zout, medianLF and the 1/Veff estimate are set as the figure's code would set them" % (outname, imgtype))
