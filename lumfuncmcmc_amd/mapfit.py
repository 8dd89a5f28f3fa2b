"""Maximum a posteriori fit, its Hessian and the Laplace evidence, on the host, over any batched gradient callable

    f(theta[K, ndim]) -> (lnprob[K], grad[K, ndim])

plus the flat prior's box (ndim, 2) - LFContext.lnprob_grad on the GPU, grad.lnprob_grad's twin without one (DESIGN.md
section 3.14).  NumPy only.  Rows whose lnprob is not finite may carry NaN gradients: they are never accepted.
"""
import numpy as np

H_REL = 1.0e-4          # default finite-difference step per coordinate, as a fraction of the box's width
STEPS = (1.0, 0.25, 0.05)      # line-search candidates along the Newton direction (fractions of the full step)


def _box(box):
    box = np.asarray(box, dtype=np.float64)
    if box.ndim != 2 or box.shape[1] != 2 or not np.all(box[:, 1] > box[:, 0]):
        raise ValueError("box must be (ndim, 2) with hi > lo")
    return box


def stencil(theta, box, h=None):
    """The 2 ndim rows of the central-difference stencil of `hessian` around theta (ndim,), and their offsets (plus[ndim],
    minus[ndim]): row 2 j = theta + plus_j e_j, row 2 j + 1 = theta + minus_j e_j."""
    box = _box(box)
    theta = np.asarray(theta, dtype=np.float64)
    nd = theta.size
    h0 = H_REL * (box[:, 1] - box[:, 0]) if h is None else np.broadcast_to(np.asarray(h, dtype=np.float64), (nd,)).copy()
    up, dn = box[:, 1] - theta, theta - box[:, 0]
    hh = np.minimum(h0, 0.5 * np.minimum(up, dn))      # shrunk to stay strictly inside the box (a box may exclude its bounds)
    plus, minus = hh.copy(), -hh
    on = hh <= 0.0                                     # on a bound: one-sided, into the box
    plus[on] = np.where(up[on] > 0.0, h0[on], 0.0)
    minus[on] = np.where(up[on] > 0.0, 0.0, -h0[on])
    rows = np.repeat(theta[None], 2 * nd, axis=0)
    rows[2 * np.arange(nd), np.arange(nd)] += plus
    rows[2 * np.arange(nd) + 1, np.arange(nd)] += minus
    return rows, plus, minus


def _hessian_from(grads, plus, minus):
    """grads (2 ndim, ndim) at the stencil's rows -> the symmetrised Hessian."""
    H = (grads[0::2] - grads[1::2]) / (plus - minus)[:, None]        # row j = d grad / d theta_j
    return 0.5 * (H + H.T)


def hessian(f, theta, box, h=None):
    """Hessian of lnprob at theta (ndim,) by central differences of the gradient: 2 ndim rows in ONE call of f, symmetrised.

    Step per coordinate h_j = 1e-4 (hi_j - lo_j) by default, shrunk to stay inside the box (a coordinate exactly on a bound
    is differenced one-sidedly into the box).  Why 1e-4 of the width: the central difference of g has a truncation error of
    h^2 g''' / 6 - for a posterior whose scale of variation is the box, 1e-8 relative to g' - and a rounding error of
    eps_g |g| / h with eps_g the gradient's relative rounding: the device's and the twin's gradients are good to ~1e-12 of
    their terms' absolute sum, so 1e-12 / 1e-4 = 1e-8 again.  Both errors are near 1e-8 relative; a smaller step lets
    rounding grow, a larger one truncation.  For a gradient that is linear (a Gaussian) only the rounding term remains."""
    rows, plus, minus = stencil(theta, box, h)
    _, g = f(rows)
    return _hessian_from(np.asarray(g, dtype=np.float64), plus, minus)


def _active(theta, grad, box):
    """Coordinates held at a bound: on it, with the gradient pointing out of the box."""
    return ((theta <= box[:, 0]) & (grad < 0.0)) | ((theta >= box[:, 1]) & (grad > 0.0))


def newton_decrement(grad, H, free=None):
    """g^T (-H)^-1 g over the free coordinates; inf when -H is not positive definite there.  Half of it is the expected
    shortfall of lnprob below its maximum."""
    grad, H = np.asarray(grad, dtype=np.float64), np.asarray(H, dtype=np.float64)
    free = np.ones(grad.size, dtype=bool) if free is None else np.asarray(free, dtype=bool)
    if not free.any():
        return 0.0
    M = -H[np.ix_(free, free)]
    if not np.all(np.isfinite(M)) or not np.all(np.isfinite(grad[free])):
        return np.inf
    w = np.linalg.eigvalsh(M)
    if not w[0] > 0.0:
        return np.inf
    return float(grad[free] @ np.linalg.solve(M, grad[free]))


def _direction(grad, H, free):
    """Ascent direction over the free coordinates: Newton's where -H is positive definite, else with the eigenvalues of -H
    replaced by their magnitudes (floored), so that it always points uphill."""
    p = np.zeros(grad.size)
    if not free.any():
        return p
    M = -H[np.ix_(free, free)]
    if not np.all(np.isfinite(M)):
        p[free] = grad[free]
        return p
    w, V = np.linalg.eigh(M)
    w = np.maximum(np.abs(w), 1.0e-8 * max(np.max(np.abs(w)), 1.0e-300))
    p[free] = V @ ((V.T @ grad[free]) / w)
    return p


def maximise(f, box, starts, tol=1.0e-6, max_iter=60, h=None, inset=0.0):
    """Box-constrained Newton iteration for the maximum of lnprob, run for K starts at once.

    Every iteration is ONE batched call of f: for each start that is still running, its line-search candidates along the
    current direction (the full step and fractions of it, projected onto the box), each with the 2 ndim rows of `hessian`'s
    stencil around it - so the candidate that is taken arrives with its gradient and Hessian, and the next direction
    needs no call of its own.  The direction is Newton's over the free coordinates (those not held at a bound with the
    gradient pointing out), with -H made positive definite where it is not.  A start stops when its Newton decrement
    g^T (-H)^-1 g over the free coordinates is <= tol (half of it is the expected shortfall in lnprob).
    inset: the iteration works in the box shrunk by this fraction of its width on every side - for a prior that excludes
    its bounds (lnprob is -inf on them: a maximum there could only be crept up to) pass a small one, 1e-9; the box the
    iteration worked in is returned as "box", and on_bound refers to it.

    Returns a dict: theta, lnprob, grad, hessian of the best start (the largest lnprob among the converged ones, else among
    all), on_bound (mask of coordinates held at a bound), niter, converged, decrement, and all_theta / all_lnprob /
    all_converged over the K starts."""
    box = _box(box)
    if inset:
        box = np.column_stack([box[:, 0] + inset * (box[:, 1] - box[:, 0]), box[:, 1] - inset * (box[:, 1] - box[:, 0])])
    X = np.clip(np.atleast_2d(np.asarray(starts, dtype=np.float64)), box[:, 0], box[:, 1])
    K, nd = X.shape
    if nd != box.shape[0]:
        raise ValueError("starts must be (K, %d)" % box.shape[0])
    per = 1 + 2 * nd

    def evaluate(points):
        """points (M, nd) -> lnprob[M], grad[M, nd], H[M, nd, nd]: one call of f."""
        rows, offs = [], []
        for x in points:
            st, plus, minus = stencil(x, box, h)
            rows.append(x[None])
            rows.append(st)
            offs.append((plus, minus))
        lp, g = f(np.concatenate(rows, axis=0))
        lp, g = np.asarray(lp, dtype=np.float64), np.asarray(g, dtype=np.float64)
        Hs = np.array([_hessian_from(g[i * per + 1:(i + 1) * per], *offs[i]) for i in range(len(points))])
        return lp[::per], g[::per], Hs

    lp, g, H = evaluate(X)
    alive = np.isfinite(lp)                         # a start outside the support never runs
    conv = np.zeros(K, dtype=bool)
    dec = np.full(K, np.inf)
    scale = np.ones(K)
    niter = 0

    def check(k):
        free = ~_active(X[k], g[k], box)
        dec[k] = newton_decrement(g[k], H[k], free)
        conv[k] = dec[k] <= tol

    for k in np.flatnonzero(alive):
        check(k)
    while niter < max_iter and np.any(alive & ~conv):
        run = np.flatnonzero(alive & ~conv)
        cands = []
        for k in run:
            free = ~_active(X[k], g[k], box)
            p = _direction(g[k], H[k], free)
            for s in STEPS:
                cands.append(np.clip(X[k] + scale[k] * s * p, box[:, 0], box[:, 1]))
        clp, cg, cH = evaluate(np.array(cands))
        niter += 1
        for i, k in enumerate(run):
            sl = slice(i * len(STEPS), (i + 1) * len(STEPS))
            vals = np.where(np.isfinite(clp[sl]) & np.all(np.isfinite(cg[sl]), axis=1), clp[sl], -np.inf)
            j = int(np.argmax(vals))
            if vals[j] > lp[k]:
                X[k], lp[k], g[k], H[k] = cands[sl][j], clp[sl][j], cg[sl][j], cH[sl][j]
                scale[k] = min(1.0, scale[k] * (4.0 if j == 0 else 1.0))
                check(k)
            else:
                scale[k] *= 0.1                     # no candidate is higher: shorter steps along the same direction
                if scale[k] < 1.0e-12:
                    alive[k] = False                # (stuck: neither converged nor able to move)
    pool = np.flatnonzero(conv) if conv.any() else np.arange(K)
    best = int(pool[np.argmax(np.where(np.isfinite(lp[pool]), lp[pool], -np.inf))])
    return {"theta": X[best].copy(), "lnprob": float(lp[best]), "grad": g[best].copy(), "hessian": H[best].copy(),
            "on_bound": _active(X[best], g[best], box), "niter": niter, "converged": bool(conv[best]),
            "decrement": float(dec[best]), "box": box, "all_theta": X, "all_lnprob": lp, "all_converged": conv}


def laplace_evidence(lnprob_hat, H, box, on_bound=None):
    """Laplace's approximation of the evidence for a flat prior NORMALISED over the box - the convention of fit_model_pt's
    lnZ (thermodynamic integration from the prior), so the two are directly comparable:

        lnZ = lnprob(theta_hat) + (d / 2) ln 2 pi - 1/2 ln det(-H) - sum_j ln(hi_j - lo_j)

    Returns (lnZ, reason): reason is "" when lnZ is valid, else lnZ is NaN and reason says why (-H not positive definite;
    a coordinate on its bound, where the Gaussian integral is cut)."""
    box = _box(box)
    H = np.asarray(H, dtype=np.float64)
    d = box.shape[0]
    if H.shape != (d, d):
        raise ValueError("H must be (%d, %d)" % (d, d))
    if on_bound is not None and np.any(on_bound):
        return np.nan, "coordinate(s) %s on a bound of the box" % np.flatnonzero(on_bound).tolist()
    if not np.isfinite(lnprob_hat) or not np.all(np.isfinite(H)):
        return np.nan, "lnprob or Hessian not finite"
    w = np.linalg.eigvalsh(-0.5 * (H + H.T))
    if not w[0] > 0.0:
        return np.nan, "-H is not positive definite (smallest eigenvalue %.3g)" % w[0]
    return float(lnprob_hat + 0.5 * d * np.log(2.0 * np.pi) - 0.5 * np.sum(np.log(w)) - np.sum(np.log(box[:, 1] - box[:, 0]))), ""
