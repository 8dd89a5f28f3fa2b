"""Affine-invariant ensemble sampler (Goodman & Weare stretch move) on the batched boundary.

The reference hands a scalar callable to emcee (lumfuncmcmc.py:489-491) and reads back
`sampler.chain`, `.lnprobability`, `.acor`, `.acceptance_fraction` (:499-513).  emcee is not
installed here, and its per-walker Python call is exactly the overhead the batched C ABI removes,
so this is an own implementation with that read-back surface.  One step = two half-ensemble
updates; each half is ONE call of `log_prob_fn` with a (W/2, ndim) block - the shape
lf_lnprob_batch is built for.

With several ranks (torch.distributed initialised), every rank runs the same sampler with the
same random stream; `log_prob_fn` (lumfuncmcmc_amd.dist.ShardedLnProb) evaluates only its slice
of the block and all-gathers, so the ensembles stay bitwise identical across ranks.
"""
import numpy as np

from .philox import draw, u53


def integrated_time(x, c=5.0):
    """Integrated autocorrelation time of a (nsteps, nwalkers) series, Sokal windowing; finite for
    any input (short chains return a positive estimate instead of raising)."""
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    n = x.shape[0]
    if n < 4:
        return 1.0
    acf = np.zeros(n)
    size = 1 << int(np.ceil(np.log2(2 * n)))
    for k in range(x.shape[1]):
        y = x[:, k] - x[:, k].mean()
        f = np.fft.rfft(y, n=size)
        a = np.fft.irfft(f * np.conjugate(f))[:n]
        if a[0] > 0:
            acf += a / a[0]
    acf /= max(x.shape[1], 1)
    taus = 2.0 * np.cumsum(acf) - 1.0
    m = np.arange(n) < c * taus
    win = int(np.argmin(m)) if not m.all() else n - 1
    tau = float(taus[win])
    return tau if np.isfinite(tau) and tau > 0 else 1.0


# ------------------------------------------------------------------------------------------------------ chain diagnostics
# Autocorrelation time, effective sample size and split-R-hat of a chain by DIRECT sums: on the GPU
# (lf_chain_diag, lf_sampler_diag, lf_ptsampler_diag of include/lfmcmc.h; csrc/lf_diag.h) and as a NumPy twin that states the
# same sums in the same blocks.  The definitions are integrated_time's; the FFT above stays the yardstick.

DIAG_TILE, DIAG_LAGS = 256, 512          # steps per tile and lags per pass of csrc/lf_diag.h


class ChainDiagnostics(object):
    """tau, window, ess, rhat: one entry per series (the ndim parameters, then lnprob when it was given); n steps of
    nwalkers walkers; acf (D, nlags) when it was asked for."""

    def __init__(self, tau, window, ess, rhat, n, nwalkers, acf=None):
        self.tau, self.window, self.ess, self.rhat = tau, window, ess, rhat
        self.n, self.nwalkers, self.acf = int(n), int(nwalkers), acf

    def __repr__(self):
        return "ChainDiagnostics(n=%d, nwalkers=%d, tau=%s, ess=%s, rhat=%s)" % (self.n, self.nwalkers, self.tau, self.ess, self.rhat)


def _chain_args(chain, lnprob, t0):
    chain = np.ascontiguousarray(chain, dtype=np.float64)
    if chain.ndim != 3:
        raise ValueError("chain must be (nwalkers, nsteps, ndim)")
    if lnprob is not None:
        lnprob = np.ascontiguousarray(lnprob, dtype=np.float64)
        if lnprob.shape != chain.shape[:2]:
            raise ValueError("lnprob must be (nwalkers, nsteps)")
    t0 = int(t0)
    if not 0 <= t0 < chain.shape[1]:
        raise ValueError("t0 must lie inside the chain")
    return chain, lnprob, t0


def chain_window(acf, c, n):
    """integrated_time's window rule on acf[0 .. M) of a series of n steps: (tau, window), or None when no window lies
    below M and M < n (more lags are needed).  NumPy; lf_chain_window is the same rule in C."""
    if n < 4:
        return 1.0, 0
    acf = np.asarray(acf, dtype=np.float64)[:n]
    taus = 2.0 * np.cumsum(acf) - 1.0
    m = np.arange(len(acf)) < c * taus
    if m.all():
        if len(acf) < n:
            return None
        win = n - 1
    else:
        win = int(np.argmin(m))
    tau = float(taus[win])
    return (tau if np.isfinite(tau) and tau > 0 else 1.0), win


def _twin_mean(x):
    """Two-pass mean along the last axis, as the device takes it."""
    m0 = x.sum(axis=-1) / x.shape[-1]
    return m0 + (x - m0[..., None]).sum(axis=-1) / x.shape[-1]


def _twin_lag_sums(y, k_lo, k_hi):
    """a[w][k] = sum_{t < n-k} y[w][t] y[w][t+k] for k_lo <= k < k_hi in the device's blocks: per tile of 256 steps four
    runs of 64 steps, each run's totals added tile by tile, then ((q0 + q1) + q2) + q3."""
    W, n = y.shape
    nt = -(-n // DIAG_TILE)
    pad = np.zeros((W, nt * DIAG_TILE + k_hi))
    pad[:, :n] = y
    base = pad[:, :nt * DIAG_TILE]
    out = np.zeros((W, k_hi - k_lo))
    for k in range(k_lo, min(k_hi, n)):
        runs = (base * pad[:, k:k + nt * DIAG_TILE]).reshape(W, nt, 4, 64).sum(axis=3)
        q = np.cumsum(runs, axis=1)[:, -1]
        out[:, k - k_lo] = ((q[:, 0] + q[:, 1]) + q[:, 2]) + q[:, 3]
    return out


def split_rhat(x):
    """Split-R-hat (Gelman et al. 2013) of a (nwalkers, n) series: every walker's range cut into [0, n/2) and [n - n/2, n),
    2 W sequences of length h; Wv = mean of their variances, B / h = variance of their means, sqrt(((h-1)/h Wv + B/h) / Wv).
    The walkers of an ensemble are not independent chains, so this is a sanity check (a stuck or drifting ensemble shows),
    not a convergence proof: the stopping rule of fit_model_converged is built on tau.
    The 2 W halves are added one by one in the order of lfd::split_rhat (csrc/lf_diag.h): walker by walker, first half then
    second, so that exact moments give the device's bits."""
    W, n = x.shape
    h = n // 2
    if h < 2:
        return float("nan")
    halves = np.stack([x[:, :h], x[:, n - h:]], axis=1).reshape(2 * W, h)
    mean = _twin_mean(halves)
    s2 = ((halves - mean[:, None]) ** 2).sum(axis=1) / (h - 1)
    seq = lambda v: np.cumsum(v)[-1]                # np.sum adds eight or more terms in another order
    Wv = seq(s2) / (2 * W)
    Bh = seq((mean - seq(mean) / (2 * W)) ** 2) / (2 * W - 1)
    with np.errstate(all="ignore"):
        return float(np.sqrt(((h - 1.0) / h * Wv + Bh) / Wv))


def chain_diagnostics_twin(chain, lnprob=None, t0=0, c=5.0, nlags=0):
    """The NumPy twin of chain_diagnostics: the same direct sums in the same blocks and passes (512 lags, then twice as many
    until every series has its window).  nlags > 0 also returns the first nlags lags of every ACF."""
    chain, lnprob, t0 = _chain_args(chain, lnprob, t0)
    W, steps, ndim = chain.shape
    n = steps - t0
    series = [chain[:, t0:, d] for d in range(ndim)] + ([lnprob[:, t0:]] if lnprob is not None else [])
    D = len(series)
    tau, window, rhat = np.ones(D), np.zeros(D, dtype=np.int64), np.empty(D)
    curves = []
    for d, x in enumerate(series):
        rhat[d] = split_rhat(x)
        y = x - _twin_mean(x)[:, None]
        Mmax = -(-n // DIAG_LAGS) * DIAG_LAGS
        have, want = 0, DIAG_LAGS
        if nlags > want:
            want = min(-(-nlags // DIAG_LAGS) * DIAG_LAGS, Mmax)
        a = np.zeros((W, 0))
        acf = np.zeros(0)
        while n >= 4:
            a = np.concatenate([a, _twin_lag_sums(y, have, want)], axis=1)
            have = want
            acf = np.zeros(have)
            for w in range(W):
                if a[w, 0] > 0:
                    acf += a[w] / a[w, 0]
            acf /= W
            res = chain_window(acf[:min(have, n)], c, n)
            if res is not None:
                tau[d], window[d] = res
                break
            want = min(2 * have, Mmax)
        curves.append(acf)
    out = None
    if nlags > 0:
        out = np.zeros((D, nlags))
        for d, acf in enumerate(curves):
            k = min(nlags, len(acf))
            out[d, :k] = acf[:k]
    return ChainDiagnostics(tau, window, W * n / tau, rhat, n, W, out)


def _diag_outputs(D):
    return np.empty(D), np.empty(D, dtype=np.int64), np.empty(D), np.empty(D)


def chain_diagnostics(chain, lnprob=None, t0=0, c=5.0, device=None, nlags=0):
    """tau (integrated_time's definition and window rule), its window, ess = W n / tau and split-R-hat (see split_rhat) per
    parameter of `chain` (nwalkers, nsteps, ndim) over steps t0 .. nsteps - and of `lnprob` (nwalkers, nsteps) as one more
    series - computed on the GPU by direct sums (lf_chain_diag).  device: the HIP device ordinal (None = 0); there is no host
    fall-back here, the NumPy statement is chain_diagnostics_twin.  nlags > 0 also returns that many lags of every ACF."""
    import ctypes
    from . import capi
    chain, lnprob, t0 = _chain_args(chain, lnprob, t0)
    lib = capi.load()
    W, steps, ndim = chain.shape
    D = ndim + (lnprob is not None)
    tau, window, ess, rhat = _diag_outputs(D)
    acf = np.empty((D, int(nlags))) if nlags > 0 else None
    rc = lib.lf_chain_diag(0 if device is None else int(device), capi._ptr(chain), capi._ptr(lnprob), W, steps, ndim, t0, steps, float(c),
                           capi._ptr(tau), window.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), capi._ptr(ess), capi._ptr(rhat),
                           capi._ptr(acf), int(nlags))
    if rc != capi.LF_OK:
        raise capi.LFError("lf_chain_diag failed (%d)" % rc)
    return ChainDiagnostics(tau, window, ess, rhat, steps - t0, W, acf)


class EnsembleSampler(object):
    def __init__(self, nwalkers, ndim, log_prob_fn, a=2.0, vectorize=True, seed=None):
        if nwalkers < 2 * ndim or nwalkers % 2:
            raise ValueError("nwalkers must be even and at least 2*ndim (got %d for ndim %d)" % (nwalkers, ndim))
        self.nwalkers, self.ndim, self.a = int(nwalkers), int(ndim), float(a)
        self.log_prob_fn, self.vectorize = log_prob_fn, vectorize
        self.random = np.random.RandomState(seed)
        self.chain = np.empty((self.nwalkers, 0, self.ndim))
        self.lnprobability = np.empty((self.nwalkers, 0))
        self.naccepted = np.zeros(self.nwalkers)
        self.iterations = 0
        self.nevals = 0

    def _lnprob(self, block):
        self.nevals += len(block)
        if self.vectorize:
            lp = np.asarray(self.log_prob_fn(block), dtype=np.float64)
        else:
            lp = np.array([self.log_prob_fn(row) for row in block], dtype=np.float64)
        if np.isnan(lp).any():
            raise ValueError("log_prob_fn returned NaN")
        return lp

    def run_mcmc(self, pos, nsteps, rstate0=None, lnprob0=None):
        if rstate0 is not None:
            self.random.set_state(rstate0)
        p = np.array(pos, dtype=np.float64)
        if p.shape != (self.nwalkers, self.ndim):
            raise ValueError("pos must be (nwalkers, ndim)")
        lp = self._lnprob(p) if lnprob0 is None else np.array(lnprob0, dtype=np.float64)
        W, half = self.nwalkers, self.nwalkers // 2
        chain = np.empty((W, nsteps, self.ndim))
        lnps = np.empty((W, nsteps))
        for it in range(nsteps):
            perm = self.random.permutation(W)
            sets = (perm[:half], perm[half:])
            for s in (0, 1):
                act, oth = sets[s], sets[1 - s]
                zz = ((self.a - 1.0) * self.random.rand(half) + 1.0) ** 2 / self.a
                partner = oth[self.random.randint(len(oth), size=half)]
                prop = p[partner] - (p[partner] - p[act]) * zz[:, None]
                newlp = self._lnprob(prop)
                with np.errstate(invalid="ignore"):          # -inf - -inf = nan: never accepted
                    lnq = (self.ndim - 1.0) * np.log(zz) + newlp - lp[act]
                    acc = np.log(self.random.rand(half)) < lnq
                acc &= np.isfinite(newlp)
                idx = act[acc]
                p[idx] = prop[acc]
                lp[idx] = newlp[acc]
                self.naccepted[idx] += 1
            chain[:, it] = p
            lnps[:, it] = lp
        self.chain = np.concatenate([self.chain, chain], axis=1)
        self.lnprobability = np.concatenate([self.lnprobability, lnps], axis=1)
        self.iterations += nsteps
        return p, lp, self.random.get_state()

    @property
    def acceptance_fraction(self):
        return self.naccepted / max(self.iterations, 1)

    @property
    def flatchain(self):
        return self.chain.reshape(-1, self.ndim)

    def get_autocorr_time(self, c=5.0):
        return np.array([integrated_time(self.chain[:, :, d].T, c=c) for d in range(self.ndim)])

    @property
    def acor(self):
        return self.get_autocorr_time()


def _likelihood_flag(likelihood):
    """("plain", 0) or ("convolved", 1): the device samplers' `likelihood` keyword, checked before any library is touched."""
    if likelihood not in ("plain", "convolved"):
        raise ValueError('likelihood must be "plain" or "convolved", got %r' % (likelihood,))
    return likelihood, int(likelihood == "convolved")


class DeviceEnsembleSampler(object):
    """The same read-back surface, with the whole stretch move on the GPU (lf_sampler_* of
    include/lfmcmc.h): positions, lnprob and the chain stay in HBM, a step is two kernel launches
    - one per half-ensemble (lf_free_step / lf_pers_step: proposal, likelihood and accept step; what
    ctx.last_launch() reports as fused; six with the option "fuse_step" 0 or where lf_main serves)
    - and no host round trip.  Parallel stretch move with two fixed half-ensembles (emcee 2.x form);
    Philox4x32-10 random numbers keyed by `seed`, so (seed, start) determines the chain
    (tests/test_gpu_sampler.py and tests/test_gpu_sampler_shapes.py replay it on the host).
    likelihood="convolved": the target is the flux-error-convolved likelihood (ctx.set_lum_err first; lf_sampler_set_likelihood,
    DESIGN.md section 3.20) - a half-step is then proposal, plain evaluation, the correction's kernels and accept step, still
    without a host round trip, and the chain is the host replay over ctx.lnprob_err_batch."""

    def __init__(self, ctx, nwalkers, a=2.0, seed=0, capacity=1000, likelihood="plain"):
        import ctypes
        self.likelihood = _likelihood_flag(likelihood)[0]
        if nwalkers < 2 * ctx.ndim or nwalkers % 2:
            raise ValueError("nwalkers must be even and at least 2*ndim (got %d for ndim %d)" % (nwalkers, ctx.ndim))
        self._ct = ctypes
        self.ctx, self.nwalkers, self.ndim, self.a, self.seed = ctx, int(nwalkers), ctx.ndim, float(a), int(seed)
        self.capacity = int(capacity)
        h = ctx._lib.lf_sampler_create(ctx._h, self.nwalkers, self.a, ctypes.c_uint64(self.seed), self.capacity)
        if not h:
            raise RuntimeError("lf_sampler_create failed: %s" % ctx._lib.lf_last_error(ctx._h).decode())
        self._h = ctypes.c_void_p(h)
        self._started = False
        if self.likelihood == "convolved":
            try:
                self.set_likelihood("convolved")
            except Exception:
                self.close()
                raise

    def set_likelihood(self, likelihood):
        """"plain" or "convolved" (lf_sampler_set_likelihood): before the start, or between a start and the first step."""
        name, flag = _likelihood_flag(likelihood)
        self.ctx._check(self.ctx._lib.lf_sampler_set_likelihood(self._h, flag))
        self.likelihood = name

    def _p(self, a):
        return a.ctypes.data_as(self._ct.POINTER(self._ct.c_double)) if a is not None else None

    def run_mcmc(self, pos, nsteps, rstate0=None, lnprob0=None):
        """pos=None continues from the current state.  Enqueues and returns after the last step has
        been read back (use `enqueue` + `sync` to overlap with host work)."""
        self.enqueue(pos, nsteps, lnprob0)
        return self.sync()

    def enqueue(self, pos, nsteps, lnprob0=None):
        lib = self.ctx._lib
        if pos is not None or not self._started:
            p = np.ascontiguousarray(pos, dtype=np.float64)
            if p.shape != (self.nwalkers, self.ndim):
                raise ValueError("pos must be (nwalkers, ndim)")
            l0 = None if lnprob0 is None else np.ascontiguousarray(lnprob0, dtype=np.float64)
            self.ctx._check(lib.lf_sampler_start(self._h, self._p(p), self._p(l0)))
            self._started = True
        self.ctx._check(lib.lf_sampler_run(self._h, int(nsteps), None))

    def enqueue_sharded(self, pos, nsteps, group=None, lnprob0=None, force_collective=False, shard="walkers"):
        """The same chain with every half-step sharded over the ranks of a torch.distributed group (one process
        per GPU).

        shard="walkers": every rank holds the whole catalogue; propose everywhere, evaluate the local slice of the
        half, all-gather the slices' lnprob (RCCL, in stream order), accept everywhere.  The chain is bit-identical
        to the one-GPU chain.
        shard="sources": this sampler's context holds 1/world of the catalogue (dist.shard_sources) and its share of
        the grid ("grid_share"); every rank evaluates the WHOLE half on its shard, one all-reduce(SUM) of the half's
        lnprob, accept everywhere.  Only the summation order differs from the one-GPU chain (1e-13)."""
        import torch
        import torch.distributed as dist
        from .dist import slice_bounds
        lib, ct = self.ctx._lib, self._ct
        world = dist.get_world_size(group) if dist.is_initialized() else 1
        rank = dist.get_rank(group) if dist.is_initialized() else 0
        dev = torch.device("cuda", self.ctx.device)
        half = self.nwalkers // 2
        # force_collective: keep the collective with a one-rank group (one-GPU rehearsal of the RCCL path)
        collective = world > 1 or (force_collective and dist.is_initialized())
        nccl = collective and dist.get_backend(group) == "nccl"
        stream = torch.cuda.current_stream(dev).cuda_stream

        def fence_before():           # gloo (rehearsal) does not order with our launches
            if collective and not nccl:
                torch.cuda.current_stream(dev).synchronize()

        def fence_after():            # ... nor its result with the next launch
            if collective and not nccl:
                torch.cuda.synchronize(dev)

        by_source = shard == "sources"
        if shard not in ("walkers", "sources"):
            raise ValueError("shard must be 'walkers' or 'sources'")
        if pos is not None or not self._started:
            p = np.ascontiguousarray(pos, dtype=np.float64)
            l0 = None if lnprob0 is None else np.ascontiguousarray(lnprob0, dtype=np.float64)
            if by_source and l0 is None and collective:
                # the start's lnprob is a sum over the shards too
                t0 = self.ctx.lnprob_torch(torch.from_numpy(p).to(dev))
                fence_before()
                dist.all_reduce(t0, op=dist.ReduceOp.SUM, group=group)
                fence_after()
                l0 = np.ascontiguousarray(t0.cpu().numpy())
            self.ctx._check(lib.lf_sampler_start(self._h, self._p(p), self._p(l0)))
            self._started = True
        if by_source:
            buf = torch.empty((half,), dtype=torch.float64, device=dev)
            for _ in range(int(nsteps)):
                for h in (0, 1):
                    self.ctx._check(lib.lf_sampler_half_eval(self._h, h, 0, half, ct.c_void_p(buf.data_ptr()), ct.c_void_p(stream)))
                    if collective:
                        fence_before()
                        dist.all_reduce(buf, op=dist.ReduceOp.SUM, group=group)
                        fence_after()
                    self.ctx._check(lib.lf_sampler_half_accept(self._h, h, ct.c_void_p(buf.data_ptr()), ct.c_void_p(stream)))
            self._keep = buf
            return
        bounds, per = slice_bounds(half, world)
        lo, hi = bounds[rank]
        # the gather buffer is [world][per]; rank r's rows start at r * per in the half as well, so its first `half`
        # entries are the half's lnprob in walker order (no re-packing for ragged splits)
        buf = torch.full((per * world,), float("-inf"), dtype=torch.float64, device=dev)
        sep = None if (nccl or not collective) else torch.full((per,), float("-inf"), dtype=torch.float64, device=dev)   # RCCL gathers in place
        mine = buf[rank * per:(rank + 1) * per] if sep is None else sep
        for _ in range(int(nsteps)):
            for h in (0, 1):
                self.ctx._check(lib.lf_sampler_half_eval(self._h, h, lo, hi, ct.c_void_p(mine.data_ptr() - lo * 8),
                                                         ct.c_void_p(stream)))
                if collective:
                    fence_before()
                    dist.all_gather_into_tensor(buf, mine, group=group)
                    fence_after()
                self.ctx._check(lib.lf_sampler_half_accept(self._h, h, ct.c_void_p(buf.data_ptr()), ct.c_void_p(stream)))
        self._keep = buf

    def sync(self):
        lib = self.ctx._lib
        t = int(lib.lf_sampler_steps(self._h))
        W, nd = self.nwalkers, self.ndim
        self.chain = np.empty((W, t, nd))
        self.lnprobability = np.empty((W, t))
        self.naccepted = np.empty(W, dtype=np.int64)
        pos, lp = np.empty((W, nd)), np.empty(W)
        self.ctx._check(lib.lf_sampler_read(self._h, self._p(self.chain), self._p(self.lnprobability),
                                            self.naccepted.ctypes.data_as(self._ct.POINTER(self._ct.c_int64)),
                                            self._p(pos), self._p(lp)))
        self.iterations = t
        return pos, lp, None

    @property
    def acceptance_fraction(self):
        return self.naccepted / max(self.iterations, 1)

    @property
    def flatchain(self):
        return self.chain.reshape(-1, self.ndim)

    def get_autocorr_time(self, c=5.0, device=False):
        """device=False: integrated_time on the chain read back by sync(); device=True: diagnostics(c=c).tau, the chain
        stays in HBM."""
        if device:
            return self.diagnostics(c=c).tau
        return np.array([integrated_time(self.chain[:, :, d].T, c=c) for d in range(self.ndim)])

    @property
    def acor(self):
        return self.get_autocorr_time()

    def diagnostics(self, t0=0, c=5.0, with_lnprob=False):
        """ChainDiagnostics of the steps t0 .. now of the chain where it is (lf_sampler_diag): waits for the enqueued steps,
        copies no chain and changes nothing of the sampler's state.  with_lnprob adds the lnprob series as the last entry."""
        D = self.ndim + bool(with_lnprob)
        tau, window, ess, rhat = _diag_outputs(D)
        lib = self.ctx._lib
        self.ctx._check(lib.lf_sampler_diag(self._h, int(t0), float(c), int(bool(with_lnprob)), self._p(tau),
                                            window.ctypes.data_as(self._ct.POINTER(self._ct.c_int64)), self._p(ess), self._p(rhat)))
        return ChainDiagnostics(tau, window, ess, rhat, int(lib.lf_sampler_steps(self._h)) - int(t0), self.nwalkers)

    def close(self):
        if getattr(self, "_h", None) is not None:
            self.ctx._lib.lf_sampler_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---------------------------------------------------------------------------------------------------- parallel tempering
# emcee 2.x's PTSampler read-back surface (betas, chain [T][W][S][ndim], lnlikelihood, lnprobability, acceptance_fraction,
# tswap_acceptance_fraction, acor, thermodynamic_integration_log_evidence) over a flat prior box: the tempered target at
# inverse temperature beta is beta * lnlike.  The stretch move runs on all T x W/2 walkers of a half at once (one block
# for the likelihood), then neighbouring temperatures swap walkers (DESIGN.md section 3.10 states the random streams, the
# swap order and the estimator).  PTSampler is the NumPy statement, DevicePTSampler runs it on the GPU (lf_ptsampler_*);
# with the same seed, ladder and start they make the same chain.

def geometric_betas(ntemps, Tmax):
    """beta_i = Tmax^(-i / (ntemps - 1)): 1 down to 1 / Tmax."""
    ntemps = int(ntemps)
    if ntemps == 1:
        return np.ones(1)
    if not Tmax > 1.0:
        raise ValueError("Tmax must be > 1")
    b = np.power(float(Tmax), -np.arange(ntemps) / (ntemps - 1.0))
    b[0] = 1.0
    return b


def tmax_from_box(loglike_fn, box, n=4096, seed=0):
    """The ladder's top temperature from the data: the finite lnlike of n uniform draws in the prior box spread over
    `spread` nats; Tmax = max(spread, 10) puts beta_min * spread <= 1 nat, so that the hottest chain samples close to the
    prior and the estimator's closing piece over [0, beta_min] is small."""
    box = np.asarray(box, dtype=np.float64)
    u = np.random.default_rng(seed).random((int(n), box.shape[0]))
    lp = np.asarray(loglike_fn(box[:, 0] + u * (box[:, 1] - box[:, 0])), dtype=np.float64)
    lp = lp[np.isfinite(lp)]
    spread = float(lp.max() - lp.min()) if lp.size > 1 else 0.0
    return max(spread, 10.0)


def default_ntemps(Tmax):
    """Adjacent betas a factor of <= sqrt(2) apart: ceil(2 log2 Tmax) + 1 temperatures, 2 to 64 (a factor of 2 leaves the
    estimator's trapezoid ~0.1 nat high at d = 5, and every other temperature - dlnZ - 0.4 off)."""
    return int(min(max(int(np.ceil(2.0 * np.log2(Tmax))) + 1, 2), 64))


def ti_log_evidence(betas, mean_lnlike, fburnin=0.1):
    """(lnZ, dlnZ) by thermodynamic integration.  m_i = post-burn-in mean of mean_lnlike[i] (the walkers' mean lnlike at
    beta_i per step), c = m_0:  lnZ = c + trapezoid in ln(beta) of beta (m - c) over the ladder + beta_min (m_min - c)
    for [0, beta_min].  dlnZ = |lnZ - the same over every other temperature|."""
    betas = np.asarray(betas, dtype=np.float64)
    ml = np.asarray(mean_lnlike, dtype=np.float64)
    istart = int(ml.shape[1] * fburnin + 0.5)
    m = ml[:, istart:].mean(axis=1)

    def est(b, mm):
        c = mm[0]
        y, x = b * (mm - c), np.log(b)
        return c + np.sum(0.5 * (y[:-1] + y[1:]) * (x[:-1] - x[1:])) + b[-1] * (mm[-1] - c)

    lnZ = est(betas, m)
    return float(lnZ), float(abs(lnZ - est(betas[::2], m[::2])))


class _PTSurface(object):
    """What both PT samplers give back once `chain`, `lnlikelihood`, `mean_lnlike`, `naccepted`, `nswap` and
    `iterations` are set."""

    @property
    def lnprobability(self):
        return self.betas[:, None, None] * self.lnlikelihood

    @property
    def acceptance_fraction(self):
        return self.naccepted / max(self.iterations, 1)

    @property
    def tswap_acceptance_fraction(self):
        return self.nswap / float(max(self.iterations, 1) * self.nwalkers)

    def get_autocorr_time(self, c=5.0):
        return np.array([[integrated_time(self.chain[t, :, :, d].T, c=c) for d in range(self.ndim)]
                         for t in range(self.ntemps)])

    @property
    def acor(self):
        return self.get_autocorr_time()

    @property
    def flatchain(self):
        return self.chain.reshape(self.ntemps, -1, self.ndim)

    def thermodynamic_integration_log_evidence(self, fburnin=0.1):
        return ti_log_evidence(self.betas, self.mean_lnlike, fburnin)

    def _ladder(self, ntemps, betas, Tmax, loglike_fn, box):
        if betas is not None:
            b = np.array(betas, dtype=np.float64).ravel()
        else:
            if Tmax is None and ntemps > 1:
                if box is None:
                    raise ValueError("give betas, Tmax or the prior box")
                Tmax = tmax_from_box(loglike_fn, box)
            b = geometric_betas(ntemps, Tmax)
        if len(b) != ntemps or b[0] != 1.0 or np.any(np.diff(b) >= 0) or b[-1] <= 0:
            raise ValueError("betas must be %d values 1 = beta_0 > beta_1 > ... > 0" % ntemps)
        return b


class PTSampler(_PTSurface):
    """The parallel-tempered stretch move in NumPy with the device's Philox streams: any vectorised loglike_fn
    ((B, ndim) -> (B,)); the replay reference of DevicePTSampler.  box: (ndim, 2) prior box, only read to choose Tmax
    when neither betas nor Tmax is given."""

    def __init__(self, ntemps, nwalkers, ndim, loglike_fn, betas=None, Tmax=None, a=2.0, seed=0, box=None):
        if nwalkers < 2 or nwalkers % 2 or not 1 <= ntemps <= 64 or nwalkers > 4096:
            raise ValueError("need even 2 <= nwalkers <= 4096 and 1 <= ntemps <= 64")
        self.ntemps, self.nwalkers, self.ndim, self.a, self.seed = int(ntemps), int(nwalkers), int(ndim), float(a), int(seed)
        self.loglike_fn = loglike_fn
        self.betas = self._ladder(self.ntemps, betas, Tmax, loglike_fn, box)
        self._dbeta = np.concatenate([[0.0], self.betas[:-1] - self.betas[1:]])
        self._p = None
        self.iterations = 0
        self.step = 0

    def _ll(self, block):
        return np.asarray(self.loglike_fn(block), dtype=np.float64)

    def run_mcmc(self, pos, nsteps):
        """pos (T, W, ndim), or None to continue.  Returns (pos, lnprob, lnlike) of the last step."""
        T, W, nd, a = self.ntemps, self.nwalkers, self.ndim, self.a
        half = W // 2
        if pos is not None or self._p is None:
            p = np.array(pos, dtype=np.float64)
            if p.shape != (T, W, nd):
                raise ValueError("pos must be (ntemps, nwalkers, ndim)")
            self._p = p.reshape(T * W, nd).copy()
            self._l = self._ll(self._p)
            if not np.all(np.isfinite(self._l)):
                raise ValueError("every start position needs a finite lnlike")
            self.chain = np.empty((T, W, 0, nd))
            self.lnlikelihood = np.empty((T, W, 0))
            self.mean_lnlike = np.empty((T, 0))
            self.naccepted = np.zeros((T, W), dtype=np.int64)
            self.nswap = np.zeros(max(T - 1, 0), dtype=np.int64)
            self.iterations = self.step = 0
        P, L = self._p, self._l
        nacc = self.naccepted.reshape(-1)
        r = np.arange(T * half)
        t, w = r // half, r % half
        bt = self.betas[t]
        chain = np.empty((T, W, nsteps, nd))
        lnl = np.empty((T, W, nsteps))
        mean = np.empty((T, nsteps))
        for it in range(int(nsteps)):
            s = self.step
            for h in (0, 1):
                r0, r1, r2, _ = draw(s, h, r, 0, self.seed)
                z = ((a - 1.0) * u53(r0, r1) + 1.0) ** 2 / a
                j = t * W + (1 - h) * half + ((r2 * np.uint64(half)) >> np.uint64(32)).astype(np.int64)
                k = t * W + h * half + w
                prop = P[j] - (P[j] - P[k]) * z[:, None]
                newl = self._ll(prop)
                if np.isnan(newl).any():
                    raise ValueError("loglike_fn returned NaN")
                q0, q1, _, _ = draw(s, h, r, 1, self.seed)
                with np.errstate(all="ignore"):
                    lnq = ((nd - 1.0) * np.log(z) + bt * newl) - bt * L[k]
                    acc = (np.log(u53(q0, q1)) < lnq) & (newl > -np.inf)
                P[k[acc]] = prop[acc]
                L[k[acc]] = newl[acc]
                nacc[k[acc]] += 1
            if T > 1:
                r0, r1, r2, r3 = draw(s, 0, np.arange(W, T * W), 2, self.seed)
                keys = ((r0 << np.uint64(32)) | r1).reshape(T - 1, W)
                logu = np.log(u53(r2, r3)).reshape(T - 1, W)
                for i in range(T - 1, 0, -1):
                    sig = np.argsort(keys[i - 1], kind="stable")
                    ia, ib = i * W + np.arange(W), (i - 1) * W + sig
                    acc = logu[i - 1] < self._dbeta[i] * (L[ia] - L[ib])
                    ia, ib = ia[acc], ib[acc]
                    P[ia], P[ib] = P[ib].copy(), P[ia].copy()
                    L[ia], L[ib] = L[ib].copy(), L[ia].copy()
                    self.nswap[i - 1] += int(acc.sum())
            chain[:, :, it] = P.reshape(T, W, nd)
            lnl[:, :, it] = L.reshape(T, W)
            mean[:, it] = L.reshape(T, W).mean(axis=1)
            self.step += 1
        self.chain = np.concatenate([self.chain, chain], axis=2)
        self.lnlikelihood = np.concatenate([self.lnlikelihood, lnl], axis=2)
        self.mean_lnlike = np.concatenate([self.mean_lnlike, mean], axis=1)
        self.iterations += int(nsteps)
        lt = L.reshape(T, W).copy()
        return P.reshape(T, W, nd).copy(), self.betas[:, None] * lt, lt


class DevicePTSampler(_PTSurface):
    """PTSampler on the GPU (lf_ptsampler_* of include/lfmcmc.h): positions, lnlike and the chain stay in HBM, a step is
    three launches and one evaluation of T x W/2 rows per half plus one swap launch.  ntemps x nwalkers walkers; the
    ladder is `betas`, or geometric up to Tmax (Tmax=None: tmax_from_box on the context's prior box, over the likelihood
    being sampled).  likelihood="convolved": the tempered target is beta x the flux-error-convolved likelihood
    (lf_ptsampler_set_likelihood; see DeviceEnsembleSampler)."""

    def __init__(self, ctx, ntemps, nwalkers, betas=None, Tmax=None, a=2.0, seed=0, capacity=1000, likelihood="plain"):
        import ctypes
        self.likelihood, flag = _likelihood_flag(likelihood)
        if nwalkers < 2 or nwalkers % 2:
            raise ValueError("nwalkers must be even and >= 2")
        self._ct = ctypes
        self.ctx, self.ntemps, self.nwalkers, self.ndim = ctx, int(ntemps), int(nwalkers), ctx.ndim
        self.a, self.seed, self.capacity = float(a), int(seed), int(capacity)
        self.betas = self._ladder(self.ntemps, betas, Tmax, ctx.lnprob_err_batch if flag else ctx.lnprob_batch, ctx.prior_box())
        self._betas_c = np.ascontiguousarray(self.betas)
        h = ctx._lib.lf_ptsampler_create(ctx._h, self.ntemps, self.nwalkers, self._p(self._betas_c), self.a,
                                         ctypes.c_uint64(self.seed), self.capacity)
        if not h:
            raise RuntimeError("lf_ptsampler_create failed: %s" % ctx._lib.lf_last_error(ctx._h).decode())
        self._h = ctypes.c_void_p(h)
        self._started = False
        self.iterations = 0
        if flag:
            rc = ctx._lib.lf_ptsampler_set_likelihood(self._h, flag)
            if rc != 0:
                self.close()
                ctx._check(rc)

    def _p(self, a):
        return a.ctypes.data_as(self._ct.POINTER(self._ct.c_double)) if a is not None else None

    def run_mcmc(self, pos, nsteps, lnlike0=None):
        """pos (T, W, ndim), or None to continue.  Returns (pos, lnprob, lnlike) after the last step."""
        self.enqueue(pos, nsteps, lnlike0)
        return self.sync()

    def enqueue(self, pos, nsteps, lnlike0=None):
        lib = self.ctx._lib
        if pos is not None or not self._started:
            p = np.ascontiguousarray(pos, dtype=np.float64)
            if p.shape != (self.ntemps, self.nwalkers, self.ndim):
                raise ValueError("pos must be (ntemps, nwalkers, ndim)")
            l0 = None if lnlike0 is None else np.ascontiguousarray(lnlike0, dtype=np.float64)
            self.ctx._check(lib.lf_ptsampler_start(self._h, self._p(p), self._p(l0)))
            self._started = True
        self.ctx._check(lib.lf_ptsampler_run(self._h, int(nsteps), None))

    def sync(self):
        lib, ct = self.ctx._lib, self._ct
        s = int(lib.lf_ptsampler_steps(self._h))
        T, W, nd = self.ntemps, self.nwalkers, self.ndim
        self.chain = np.empty((T, W, s, nd))
        self.lnlikelihood = np.empty((T, W, s))
        self.mean_lnlike = np.empty((T, s))
        self.naccepted = np.empty((T, W), dtype=np.int64)
        self.nswap = np.zeros(max(T - 1, 0), dtype=np.int64)
        pos, ll = np.empty((T, W, nd)), np.empty((T, W))
        i64 = ct.POINTER(ct.c_int64)
        self.ctx._check(lib.lf_ptsampler_read(self._h, self._p(self.chain), self._p(self.lnlikelihood), self._p(self.mean_lnlike),
                                              self.naccepted.ctypes.data_as(i64),
                                              self.nswap.ctypes.data_as(i64) if T > 1 else None, self._p(pos), self._p(ll)))
        self.iterations = s
        return pos, self.betas[:, None] * ll, ll

    def get_autocorr_time(self, c=5.0, device=False):
        """device=False: integrated_time per temperature on the chain read back; device=True: diagnostics() per temperature."""
        if device:
            return np.array([self.diagnostics(t, c=c).tau for t in range(self.ntemps)])
        return _PTSurface.get_autocorr_time(self, c=c)

    def diagnostics(self, temperature=0, t0=0, c=5.0, with_lnlike=False):
        """ChainDiagnostics of one temperature's chain where it is (lf_ptsampler_diag); see DeviceEnsembleSampler.diagnostics.
        with_lnlike adds the untempered lnlike series as the last entry."""
        D = self.ndim + bool(with_lnlike)
        tau, window, ess, rhat = _diag_outputs(D)
        lib = self.ctx._lib
        self.ctx._check(lib.lf_ptsampler_diag(self._h, int(temperature), int(t0), float(c), int(bool(with_lnlike)), self._p(tau),
                                              window.ctypes.data_as(self._ct.POINTER(self._ct.c_int64)), self._p(ess), self._p(rhat)))
        return ChainDiagnostics(tau, window, ess, rhat, int(lib.lf_ptsampler_steps(self._h)) - int(t0), self.nwalkers)

    def close(self):
        if getattr(self, "_h", None) is not None:
            self.ctx._lib.lf_ptsampler_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
