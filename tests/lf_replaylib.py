"""Host statements the device samplers are replayed against, shared by the sampler tests.

host_replay is DeviceEnsembleSampler's algorithm in NumPy over lumfuncmcmc_amd.philox: the same Philox4x32-10 draws, every
operation of the stretch move rounded on its own, and the likelihood through the context's plain batched call at the batch size
of a half - so a device chain must equal it bit for bit.  grid_moments is the check that shares no algorithm with either: the
posterior's mean and covariance by quadrature.  Test infrastructure only.
"""
import numpy as np

from lumfuncmcmc_amd import synth
from lumfuncmcmc_amd.philox import draw, u53


def host_replay(ctx, pos, nsteps, seed, a=2.0, lnprob0=None, exponent=None, lnprob=None):
    """(chain (W, nsteps, ndim), lnprobability (W, nsteps), naccepted (W,)) of the parallel stretch move with two fixed halves.
    lnprob0: the start's lnprob when the caller has it.  exponent: the power of z in the acceptance ratio (None: ndim - 1, the
    rule; anything else is a deliberately wrong sampler, for sensitivity checks).  lnprob: the batched likelihood (None:
    ctx.lnprob_batch)."""
    f = ctx.lnprob_batch if lnprob is None else lnprob
    W, nd = pos.shape
    half = W // 2
    power = nd - 1.0 if exponent is None else float(exponent)
    p = pos.copy()
    lp = f(p) if lnprob0 is None else np.array(lnprob0, dtype=np.float64)
    chain = np.empty((W, nsteps, nd))
    lnps = np.empty((W, nsteps))
    nacc = np.zeros(W, dtype=np.int64)
    w = np.arange(half)
    for step in range(nsteps):
        for h in (0, 1):
            r0, r1, r2, _ = draw(step, h, w, 0, seed)
            z = ((a - 1.0) * u53(r0, r1) + 1.0) ** 2 / a
            j = (1 - h) * half + ((r2 * np.uint64(half)) >> np.uint64(32)).astype(np.int64)
            k = h * half + w
            prop = p[j] - (p[j] - p[k]) * z[:, None]
            newlp = f(prop)
            q0, q1, _, _ = draw(step, h, w, 1, seed)
            with np.errstate(all="ignore"):
                lnq = power * np.log(z) + newlp - lp[k]
                acc = (np.log(u53(q0, q1)) < lnq) & (newlp > -np.inf)
            p[k[acc]] = prop[acc]
            lp[k[acc]] = newlp[acc]
            nacc[k[acc]] += 1
            chain[k, step] = p[k]
            lnps[k, step] = lp[k]
    return chain, lnps, nacc


def fixcomp_model(n, seed):
    """Fixed completeness, fixed faint-end slope: theta = (log L*, log phi*)."""
    from lumfuncmcmc_amd.model import LumFuncMCMC
    cat = synth.catalogue(n, seed=seed)
    fi = cat["field_ind"]
    return LumFuncMCMC(synth.split_fields(cat["z"], fi), lum=synth.split_fields(cat["lum"], fi),
                       lum_e=synth.split_fields(cat["lum_e"], fi), Flim=list(synth.FLIM), alpha=synth.ALPHA_C,
                       Omega_0=list(synth.OMEGA_0), sch_al=synth.SCH_AL, sch_al_lims=synth.SCH_AL_LIMS, Lstar=synth.LSTAR,
                       Lstar_lims=synth.LSTAR_LIMS, phistar=synth.PHISTAR, phistar_lims=synth.PHISTAR_LIMS, Lc=synth.LC,
                       Lh=synth.LH, nwalkers=32, nsteps=1000, min_comp_frac=0.0, field_ind=fi, fix_comp=True,
                       fix_sch_al=True)


def grid_lnint(ctx, lo, hi, n):
    """ln of the midpoint rule for the integral of exp(lnprob) over [lo, hi] (2-d), n x n cells; then lnprob (n, n), x, y."""
    x = lo[0] + (np.arange(n) + 0.5) * (hi[0] - lo[0]) / n
    y = lo[1] + (np.arange(n) + 0.5) * (hi[1] - lo[1]) / n
    th = np.column_stack([np.repeat(x, n), np.tile(y, n)])
    lp = np.concatenate([ctx.lnprob_batch(th[i:i + 32768]) for i in range(0, len(th), 32768)])
    mx = lp[np.isfinite(lp)].max()
    return mx + np.log(np.sum(np.exp(lp - mx))) + np.log((hi[0] - lo[0]) * (hi[1] - lo[1]) / n / n), lp.reshape(n, n), x, y


def peak_box(ctx, box, drop=40.0, n=400):
    """The part of the 2-d prior box (ndim, 2) within `drop` nats of the posterior's peak, from an n x n grid: (lo, hi)."""
    _, lp, x, y = grid_lnint(ctx, box[:, 0], box[:, 1], n)
    ix, iy = np.nonzero(lp > lp[np.isfinite(lp)].max() - drop)
    dx, dy = x[1] - x[0], y[1] - y[0]
    lo = np.maximum([x[ix.min()] - 3 * dx, y[iy.min()] - 3 * dy], box[:, 0])
    hi = np.minimum([x[ix.max()] + 3 * dx, y[iy.max()] + 3 * dy], box[:, 1])
    return lo, hi


def grid_moments(ctx, lo, hi, n):
    """Mean (2,), covariance (2, 2) and mode (2,) of exp(lnprob) over [lo, hi] by the midpoint rule on n x n cells."""
    _, lp, x, y = grid_lnint(ctx, lo, hi, n)
    with np.errstate(all="ignore"):
        w = np.exp(lp - lp[np.isfinite(lp)].max())
    w /= w.sum()
    wx, wy = w.sum(axis=1), w.sum(axis=0)
    mean = np.array([np.dot(wx, x), np.dot(wy, y)])
    dx, dy = x - mean[0], y - mean[1]
    cxy = float(dx @ w @ dy)
    cov = np.array([[np.dot(wx, dx * dx), cxy], [cxy, np.dot(wy, dy * dy)]])
    i, j = np.unravel_index(np.argmax(w), w.shape)
    return mean, cov, np.array([x[i], y[j]])


def refined_moments(ctx, lo, hi, n0=64, nmax=2048):
    """grid_moments with the spacing halved until the mean and the standard deviations move by less than 1 % of a posterior
    standard deviation: (mean, cov, mode, cells a side)."""
    prev, n = None, n0
    while True:
        mean, cov, mode = grid_moments(ctx, lo, hi, n)
        sd = np.sqrt(np.diag(cov))
        if prev is not None:
            moved = max(np.max(np.abs(mean - prev[0]) / sd), np.max(np.abs(sd - prev[1]) / sd),
                        abs(cov[0, 1] - prev[2]) / (sd[0] * sd[1]))
            if moved < 0.01:
                return mean, cov, mode, n
        assert n < nmax, "the quadrature has not converged at %d cells a side" % n
        prev, n = (mean, sd, cov[0, 1]), 2 * n
