"""Mock catalogues drawn from the model, and posterior predictive checks.

The intensity is the likelihood's own interpolant.  For a theta row and field f, piece B of lnprob is the trapezoid sum
trapz(trapz(lambda_f, logL, axis=0), zarr) on the integration grid, and that sum is exactly the integral of

    f_f(z, L) = sum_{j,k} lambda_f[j, k] hat_k(z) hat_{j,k}(L)

(unit hat functions on zarr and on column k's own luminosity nodes).  A mock catalogue is the Poisson process of intensity
f_f in every field: n_f ~ Poisson(M_f) with M_f = sum m_f[j, k], m = (w_z[k] w_L[j, k]) lambda_f[j, k]; every source picks
node (j, k) with probability m / M_f (cumulative sums column k major, then j) and inverts the two hats.  Random numbers are
Philox4x32-10 keyed by the seed, counter (row_id, index, stream word) - csrc/lf_mock.h states the streams.

`MockTwin` is that algorithm in NumPy (the tests' reference; it runs anywhere), `MockGenerator` the same on the GPU through
the C ABI (lf_mock_*).  Both take the dict of `kernel_inputs()` that LFContext takes, and both give a row's catalogue as
a function of (seed, row_id, theta) only.
"""
import ctypes

import numpy as np

from . import hostsetup as hs
from . import philox

TAG = 0x6d6f0000              # the Philox stream word of the mocks (lf_mock.h: MOCK_TAG)
MAX_MEAN = 2.0 ** 31          # expected sources per (row, field) above which a call is refused
MAX_BINS = 1022               # lf_mock_hist's limit on nbins
HIST_CHUNK = 4096             # sources per workgroup of the histogram kernels (lf_mock.h: MOCK_HIST_CHUNK)
MAX_SLOTS2 = 8192             # lf_mock_hist2's limit on (nz + 2)(nl + 2) (lf_mock_hist2.h: MOCK_HIST2_MAX_SLOTS)
SCAN_TILE = 256
_LG2PI = 1.8378770664093453e+00
_LOGGAM_A = (8.333333333333333e-02, -2.777777777777778e-03, 7.936507936507937e-04, -5.952380952380952e-04,
             8.417508417508418e-04, -1.917526917526918e-03, 6.410256410256410e-03, -2.955065359477124e-02,
             1.796443723688307e-01, -1.39243221690590e+00)


class MockError(ValueError):
    pass


def _ndim(variant, fix_sch_al, nf):
    if variant == "zevol":
        return 6 + (0 if fix_sch_al else 1)
    return 2 + (0 if fix_sch_al else 1) + (nf + 1 if variant == "free" else 0)


def _integ_part(inp, nf, S):
    ip = inp.get("integ_part")
    if ip is None:            # a field-summed table: field 0 carries the sum (as LFContext)
        ip = np.zeros((nf, S, S))
        ip[0] = inp["integ_sum"]
    return np.ascontiguousarray(ip, dtype=np.float64)


def _rows(thetas, ndim):
    th = np.ascontiguousarray(np.atleast_2d(np.asarray(thetas, dtype=np.float64)))
    if th.ndim != 2 or th.shape[1] != ndim or th.shape[0] < 1:
        raise ValueError("thetas must be (R, %d) with R >= 1, got %s" % (ndim, th.shape))
    return th


def _row_ids(row_ids, R):
    if row_ids is None:
        return np.arange(R, dtype=np.int64)
    rid = np.ascontiguousarray(np.asarray(row_ids, dtype=np.int64).ravel())
    if rid.size != R:
        raise ValueError("row_ids must have one entry per row")
    return rid


# ----------------------------------------------------------------------------------------------------------- NumPy pieces
def scan(x):
    """The cumulative sums of lf_mock.h (mock_cdf) along the last axis, for masses x >= 0.  First the inclusive prefix sums
    in the device's order: tiles of 256, a Hillis-Steele scan of each tile (x[t] = x[t - d] + x[t], d = 1, 2, .., 128)
    plus the total of the tiles before it.  Every prefix has its own summation tree, so these sums alone may decrease by
    an ulp and may step at a node of zero mass.  Then a running maximum over the nodes with x > 0:
        c[j] = max(0, s[i] for i <= j with x[i] > 0)
    (max is exact: any order gives the same bits).  So c is non-decreasing and c[j] == c[j - 1] (0 for j = 0) wherever
    x[j] == 0: a first-above search never lands on a node of zero mass, and bisection and a linear search agree for every
    threshold.  A positive mass too small to lift its rounded sum above the maximum before it (below about one ulp of
    the running sum) leaves c flat too and cannot be drawn.  Returns (c, total); the total is the running sum of the
    tile totals (the scan's last lane).  It and c[-1] are two roundings of one exact sum and may differ by a few units
    of 2^-53 (each is within (9 + tiles) 2^-53 of the exact sum, relative)."""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[-1]
    out = np.empty_like(x)
    carry = np.zeros(x.shape[:-1])
    for base in range(0, n, SCAN_TILE):
        w = min(SCAN_TILE, n - base)
        t = np.zeros(x.shape[:-1] + (SCAN_TILE,))
        t[..., :w] = x[..., base:base + w]
        d = 1
        while d < SCAN_TILE:
            t[..., d:] = t[..., :-d] + t[..., d:]
            d <<= 1
        out[..., base:base + w] = carry[..., None] + t[..., :w]
        carry = carry + t[..., SCAN_TILE - 1]
    return np.maximum.accumulate(np.where(x > 0.0, out, 0.0), axis=-1), carry


def trapz_weights(x, axis=0):
    """Trapezoid weight of every node along `axis`: half the spacing to each neighbour (0.5 (left + right))."""
    x = np.moveaxis(np.asarray(x, dtype=np.float64), axis, 0)
    d = np.diff(x, axis=0)
    zero = np.zeros((1,) + x.shape[1:])
    left = np.concatenate([zero, d], axis=0)
    right = np.concatenate([d, zero], axis=0)
    return np.moveaxis(0.5 * (left + right), 0, axis)


def hat_inverse(x0, a, b, u):
    """Inverse CDF of the unit hat with left width a, right width b, peak x0 (a width of 0: no mass on that side).  Each
    root is capped at 1 (lf_mock.h: mock_hat): x stays on its side of x0 and never decreases as u grows."""
    x0, a, b, u = (np.asarray(v, dtype=np.float64) for v in (x0, a, b, u))
    with np.errstate(all="ignore"):
        ab = a + b
        left = u < a / ab
        xl = x0 - a * (1.0 - np.minimum(np.sqrt(u * ab / a), 1.0))
        xr = x0 + b * (1.0 - np.minimum(np.sqrt((1.0 - u) * ab / b), 1.0))
    return np.where(left, xl, xr)


def _words(row_ids, index, purpose, f, seed):
    rid = np.asarray(row_ids, dtype=np.int64).astype(np.uint64)
    idx = np.asarray(index, dtype=np.uint64)
    rid, idx, ff = np.broadcast_arrays(rid, idx, np.asarray(f, dtype=np.uint64))
    c3 = np.uint64(TAG | (purpose << 8)) | ff
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return philox.philox4x32(rid & np.uint64(philox.MASK), rid >> np.uint64(32), idx, c3, seed & philox.MASK,
                             (seed >> 32) & philox.MASK)


def loggam(x):
    """NumPy's random_loggam (the Stirling series its legacy Poisson sampler uses), vectorised, same operations."""
    x = np.asarray(x, dtype=np.float64)
    n = np.where(x < 7.0, np.floor(7.0 - x), 0.0).astype(np.int64)
    x0 = x + n
    x2 = (1.0 / x0) * (1.0 / x0)
    gl0 = np.full_like(x, _LOGGAM_A[9])
    for k in range(8, -1, -1):
        gl0 = gl0 * x2
        gl0 = gl0 + _LOGGAM_A[k]
    gl = gl0 / x0 + 0.5 * _LG2PI + (x0 - 0.5) * np.log(x0) - x0
    for k in range(1, 8):
        m = (x < 7.0) & (n >= k)
        gl = np.where(m, gl - np.log(x0 - 1.0), gl)
        x0 = np.where(m, x0 - 1.0, x0)
    return np.where((x == 1.0) | (x == 2.0), 0.0, gl)


def poisson(mean, row_ids, f, seed):
    """The exact Poisson draws of lf_mock.h (mock_poisson), one per entry of `mean`: 0 for mean 0, inversion by sequential
    search below 10, PTRS (Hormann 1993) from 10 on with a fresh Philox block per rejection round.  -1 where the mean is
    not finite, negative or above MAX_MEAN."""
    mu = np.asarray(mean, dtype=np.float64)
    rid, ff = np.broadcast_arrays(np.asarray(row_ids, dtype=np.int64), np.asarray(f, dtype=np.int64))
    mu, rid, ff = np.broadcast_arrays(mu, rid, ff)
    mu, rid, ff = mu.ravel(), rid.ravel(), ff.ravel()
    k = np.zeros(mu.size, dtype=np.int64)
    with np.errstate(all="ignore"):
        bad = ~((mu >= 0.0) & (mu <= MAX_MEAN))
        k[bad] = -1
        small = np.flatnonzero(~bad & (mu > 0.0) & (mu < 10.0))
        if small.size:
            w = _words(rid[small], 0, 0, ff[small], seed)
            u = philox.u53(w[0], w[1])
            m = mu[small]
            p = np.exp(-m)
            F = p.copy()
            ks = np.zeros(small.size, dtype=np.int64)
            act = u > F
            while act.any():
                ks[act] += 1
                p[act] = p[act] * (m[act] / ks[act])
                act &= p != 0.0
                F[act] = F[act] + p[act]
                act &= u > F
            k[small] = ks
        big = np.flatnonzero(~bad & (mu >= 10.0))
        if big.size:
            m = mu[big]
            slam, loglam = np.sqrt(m), np.log(m)
            b = 0.931 + 2.53 * slam
            a = -0.059 + 0.02483 * b
            invalpha = 1.1239 + 1.1328 / (b - 3.4)
            vr = 0.9277 - 3.6224 / (b - 2.0)
            todo = np.arange(big.size)
            rnd = 0
            while todo.size:
                w = _words(rid[big[todo]], rnd, 0, ff[big[todo]], seed)
                U = philox.u53(w[0], w[1]) - 0.5
                V = philox.u53(w[2], w[3])
                us = 0.5 - np.abs(U)
                aa, bb, mm = a[todo], b[todo], m[todo]
                kk = np.floor((2.0 * aa / us + bb) * U + mm + 0.43).astype(np.int64)
                acc = (us >= 0.07) & (V <= vr[todo])
                rej = ~acc & ((kk < 0) | ((us < 0.013) & (V > us)))
                test = ~acc & ~rej
                lhs = np.log(V) + np.log(invalpha[todo]) - np.log(aa / (us * us) + bb)
                rhs = -mm + kk * loglam[todo] - loggam(np.maximum(kk, 0) + 1.0)
                acc |= test & (lhs <= rhs)
                k[big[todo[acc]]] = kk[acc]
                todo = todo[~acc]
                rnd += 1
    return k.reshape(np.shape(mean)) if np.ndim(mean) else int(k[0])


def _first_above(cdf, t):
    """Per row of cdf (n, S): the first index with cdf > t, else the first with cdf >= cdf[-1] (lf_mock.h: mock_search)."""
    above = cdf > t[:, None]
    out = above.argmax(axis=1)
    none = ~above.any(axis=1)
    if none.any():
        out[none] = (cdf[none] >= cdf[none, -1:]).argmax(axis=1)
    return out


class MockTwin(object):
    """NumPy statement of lf_mock_* (same densities, cumulative sums, streams and Poisson draws)."""

    def __init__(self, inputs):
        inp = inputs
        self.variant = inp["variant"]
        self.fix_sch_al = bool(inp.get("fix_sch_al", False))
        self.sch_al0 = float(inp.get("sch_al0", 0.0))
        self.nf = len(inp["field_ind"]) - 1
        self.logL = np.ascontiguousarray(inp["logL"], dtype=np.float64)
        self.S = S = self.logL.shape[0]
        self.zarr = np.asarray(inp["zarr"], dtype=np.float64)
        self.pivots = tuple(inp.get("pivots", (1.20, 1.53, 1.86)))
        self.ndim = _ndim(self.variant, self.fix_sch_al, self.nf)
        if self.variant == "free":
            self.vp = np.asarray(inp["volume_part"], dtype=np.float64)
            self.dl = np.asarray(inp["DL_zarr"], dtype=np.float64)
            self.om0s = np.asarray(inp["Omega_0"], dtype=np.float64) / hs.SQARCSEC
            self.fcmin = float(inp.get("fcmin", 0.1))
        else:
            self.ip = _integ_part(inp, self.nf, S)
        self.wz = trapz_weights(self.zarr)
        self.wL = trapz_weights(self.logL, axis=0)
        self.dl_zarr = inp.get("DL_zarr")     # every variant's kernel_inputs() has it; only the error model needs it
        self.noise = None
        self._band = None                     # piece "below" of the cut process (set_cut_band)

    # ---------------------------------------------------------------- the density
    def lam(self, theta):
        """lambda_f[j, k] for one theta row: (nf, S, S)."""
        th = np.asarray(theta, dtype=np.float64)
        L, S, nf = self.logL, self.S, self.nf
        out = np.empty((nf, S, S))
        with np.errstate(all="ignore"):
            if self.variant == "zevol":
                al = self.sch_al0 if self.fix_sch_al else th[6]
                zrep = np.repeat(self.zarr[None], S, axis=0)
                tlf = hs.schechter_z(L, zrep, al, th[0], th[1], th[2], th[3], th[4], th[5], *self.pivots)
            else:
                al = self.sch_al0 if self.fix_sch_al else th[2]
                tlf = hs.true_lum_func(L, al, th[0], th[1])
            if self.variant == "free":
                k0 = 2 if self.fix_sch_al else 3
                alpha = th[k0 + nf]
                flux = 10 ** L / (4.0 * np.pi * (hs.MPC_CM * self.dl[None]) ** 2)
                for f in range(nf):
                    om = self.om0s[f] * hs.fleming(flux, 1.0e-17 * th[k0 + f], alpha, self.fcmin)
                    out[f] = tlf * (self.vp[None] * om)
            else:
                for f in range(nf):
                    out[f] = tlf * self.ip[f]
        return out

    def masses(self, theta):
        """m_f[j, k] = (w_z[k] w_L[j, k]) lambda_f[j, k]: (nf, S, S)."""
        return (self.wz[None, None, :] * self.wL[None]) * self.lam(theta)

    def _cdfs(self, theta):
        """cdfL (nf, S_k, S_j): column k's masses summed over j; cdfZ (nf, S): column totals summed over k; M (nf).  Both are
        scan()'s cumulative sums: non-decreasing, flat across zero masses.  M is the sum scan's carry (the reported mean)."""
        cdfL, colm = scan(np.swapaxes(self.masses(theta), 1, 2))
        cdfZ, M = scan(colm)
        return cdfL, cdfZ, M

    def means(self, thetas):
        """Expected counts M (R, nf), without the Poisson draws (and without their cap)."""
        return np.array([self._cdfs(t)[2] for t in _rows(thetas, self.ndim)])

    # ---------------------------------------------------------------- the API of MockGenerator
    def counts(self, thetas, seed, row_ids=None):
        """(mean (R, nf), count (R, nf) int64).  Raises MockError where lf_mock_counts returns LF_ERR_ARG."""
        th = _rows(thetas, self.ndim)
        rid = _row_ids(row_ids, th.shape[0])
        if not np.isfinite(th).all():
            raise MockError("row %d: theta is not finite" % int(np.flatnonzero(~np.isfinite(th).all(axis=1))[0]))
        mean = np.array([self._cdfs(t)[2] for t in th])
        cnt = poisson(mean, rid[:, None], np.arange(self.nf)[None, :], seed)
        if (cnt < 0).any():
            r, f = np.argwhere(cnt < 0)[0]
            raise MockError("row %d field %d: expected count %.17g is not finite, negative or above 2^31" % (r, f, mean[r, f]))
        return mean, cnt

    def sources(self, theta, row_id, f, seed, index, cdfs=None):
        """(z, logL) of sources `index` of field f of one row."""
        return self._sources(theta, row_id, f, f, seed, index, cdfs)[:2]

    def _sources(self, theta, row_id, f, fs, seed, index, cdfs=None):
        """(z, logL, k) of sources `index` of field f: k the redshift column of the node each picked; fs the field word of
        the Philox streams (f; the band of the cut process: f | CUT_BAND)."""
        cdfL, cdfZ = (self._cdfs(theta) if cdfs is None else cdfs)[:2]
        idx = np.asarray(index, dtype=np.uint64)
        r = _words(row_id, idx, 1, fs, seed)
        q = _words(row_id, idx, 2, fs, seed)
        cz = cdfZ[f]
        t = philox.u53(r[0], r[1]) * cz[-1]
        k = _first_above(np.broadcast_to(cz, (t.size, self.S)), t)
        tl = t - np.where(k > 0, cz[np.maximum(k - 1, 0)], 0.0)
        j = np.empty_like(k)
        for kk in np.unique(k):
            sel = k == kk
            j[sel] = _first_above(np.broadcast_to(cdfL[f, kk], (int(sel.sum()), self.S)), tl[sel])
        zr, S = self.zarr, self.S
        a = np.where(k > 0, zr[k] - zr[np.maximum(k - 1, 0)], 0.0)
        b = np.where(k < S - 1, zr[np.minimum(k + 1, S - 1)] - zr[k], 0.0)
        z = hat_inverse(zr[k], a, b, philox.u53(r[2], r[3]))
        L = self.logL
        x0 = L[j, k]
        a = np.where(j > 0, x0 - L[np.maximum(j - 1, 0), k], 0.0)
        b = np.where(j < S - 1, L[np.minimum(j + 1, S - 1), k] - x0, 0.0)
        return z, hat_inverse(x0, a, b, philox.u53(q[0], q[1])), k

    def draw(self, thetas, seed, row_ids=None, count=None):
        """(z, logL, field, offsets): the sources of every (row, field) in that order; offsets [R nf + 1]."""
        th = _rows(thetas, self.ndim)
        rid = _row_ids(row_ids, th.shape[0])
        if count is None:
            count = self.counts(th, seed, rid)[1]
        count = np.asarray(count, dtype=np.int64).reshape(th.shape[0], self.nf)
        zs, Ls, fs = [], [], []
        for r in range(th.shape[0]):
            cdfs = self._cdfs(th[r]) if count[r].any() else None
            for f in range(self.nf):
                n = int(count[r, f])
                if n:
                    z, L = self.sources(th[r], rid[r], f, seed, np.arange(n), cdfs)
                    zs.append(z)
                    Ls.append(L)
                    fs.append(np.full(n, f, dtype=np.int32))
        off = np.concatenate([[0], np.cumsum(count.ravel())]).astype(np.int64)
        cat = lambda v, dt: np.concatenate(v).astype(dt) if v else np.zeros(0, dtype=dt)   # noqa: E731
        return cat(zs, np.float64), cat(Ls, np.float64), cat(fs, np.int32), off

    def _binned(self, draw, edges, z_edges=None):
        """Bin what draw() returns (draw, draw_noisy or draw_cut) by its last luminosity column - with z_edges by (z, that column) -
        after the edges are checked; from draw_cut: (hist, kept)."""
        ze, e = (None, _edges(edges)) if z_edges is None else _edges2(z_edges, edges)
        d = draw()
        z, L, off = (d[0], d[1], d[3]) if len(d) == 4 else (d[0], d[2], d[5])
        if ze is None:
            h = bin_sources(L, off, e).reshape(-1, self.nf, e.size + 1)
        else:
            h = bin_sources2(z, L, off, ze, e).reshape(-1, self.nf, ze.size + 1, e.size + 1)
        return (h, d[6]["kept"]) if len(d) == 7 else h

    def hist(self, thetas, edges, seed, row_ids=None):
        """(R, nf, nbins + 2) counts of logL per slot searchsorted(edges, logL, side="right")."""
        return self._binned(lambda: self.draw(thetas, seed, row_ids), edges)

    def hist2(self, thetas, z_edges, edges, seed, row_ids=None, count=None):
        """(R, nf, nz + 2, nl + 2) counts of (z, logL) per slot pair (bin_sources2); count as draw takes it."""
        return self._binned(lambda: self.draw(thetas, seed, row_ids, count), edges, z_edges)

    def hist2_noisy(self, thetas, z_edges, edges, seed, row_ids=None, count=None):
        """hist2() of the true redshifts and the observed luminosities."""
        return self._binned(lambda: self.draw_noisy(thetas, seed, row_ids, count), edges, z_edges)

    def hist2_cut(self, thetas, z_edges, edges, seed, row_ids=None):
        """(hist (R, nf, nz + 2, nl + 2) of the catalogued sources' (z, L_obs), kept (R, nf))."""
        return self._binned(lambda: self.draw_cut(thetas, seed, row_ids), edges, z_edges)

    # ---------------------------------------------------------------- the observation step (lf_mock_noise.h)
    def set_error_model(self, nodes, sigma):
        """sigma(field, log10 flux) of L_obs = L_true + sigma n: `nodes` (M,) log10 flux, `sigma` (nf, M); None clears it."""
        if nodes is None:
            self.noise = self._band = None
            return
        nodes, sigma = check_error_model(nodes, sigma, self.nf)
        if self.dl_zarr is None:
            raise MockError("the inputs hold no DL_zarr: the error model needs it for the sources' fluxes")
        dl = np.asarray(self.dl_zarr, dtype=np.float64)
        if dl.shape != (self.S,) or not np.isfinite(dl).all() or (dl <= 0.0).any():
            raise MockError("DL_zarr must hold S finite values > 0")
        self.noise = (nodes, sigma, ld2_nodes(dl))
        self._band = None                     # (a band belongs to the model it was made under)

    def _observe(self, z, L, fld, off, rid, seed):
        if self.noise is None:
            raise MockError("no error model is set (set_error_model)")
        nodes, sigma, ld2n = self.noise
        sg = np.empty(L.size)
        for f in range(self.nf):
            sel = fld == f
            sg[sel] = sigma_lookup(nodes, sigma[f], log_flux(self.zarr, ld2n, z[sel], L[sel]))
        n = np.diff(off).reshape(-1, self.nf)
        dev = np.concatenate([lum_noise(n[r], rid[r], seed) for r in range(n.shape[0])]) if L.size else np.zeros(0)
        return L + sg * dev, sg

    def draw_noisy(self, thetas, seed, row_ids=None, count=None):
        """(z, L_true, L_obs, sigma, field, offsets): draw()'s sources and what the catalogue records of them."""
        th = _rows(thetas, self.ndim)
        rid = _row_ids(row_ids, th.shape[0])
        z, L, fld, off = self.draw(th, seed, rid, count)
        Lobs, sg = self._observe(z, L, fld, off, rid, seed)
        return z, L, Lobs, sg, fld, off

    def hist_noisy(self, thetas, edges, seed, row_ids=None):
        """hist() of the observed luminosities."""
        return self._binned(lambda: self.draw_noisy(thetas, seed, row_ids), edges)

    # ---------------------------------------------------------------- the cut process (lf_mock_cut.h)
    def set_cut_band(self, logLb, integ_part_b=None):
        """Piece "below" of the cut process: `logLb` (S, S) from band_grid, `integ_part_b` (nf, S, S) from band_integ_part
        (FIXCOMP, ZEVOL; FREE: None).  After set_error_model (a new error model clears the band); None clears it."""
        import copy
        self._band = None
        if logLb is None:
            return
        if self.noise is None:
            raise MockError("no error model is set: set_error_model comes first")
        logLb, ipb = check_cut_band(logLb, integ_part_b, self.logL, self.nf, self.variant != "free")
        b = copy.copy(self)
        b.logL, b.wL, b.noise = logLb, trapz_weights(logLb, axis=0), None
        quiet = ~self.noise[1].any(axis=1)          # a field without errors keeps no band source: no mass
        if self.variant == "free":
            b.om0s = np.where(quiet, 0.0, self.om0s)
        else:
            b.ip = np.where(quiet[:, None, None], 0.0, ipb)
        self._band = b

    def candidates_cut(self, thetas, seed, row_ids=None):
        """Every candidate of the cut process: (z, L_true, L_obs, sigma, field, keep, n_cand (R, nf, 2), mean (R, nf, 2)).
        Per (row, field) piece "above" in index order, then piece "below"; keep: L_obs >= the edge of the column picked."""
        th = _rows(thetas, self.ndim)
        R, nf = th.shape[0], self.nf
        rid = _row_ids(row_ids, R)
        if self.noise is None:
            raise MockError("no error model is set (set_error_model)")
        if self._band is None:
            raise MockError("no cut band is set (set_cut_band, after set_error_model)")
        if not np.isfinite(th).all():
            raise MockError("row %d: theta is not finite" % int(np.flatnonzero(~np.isfinite(th).all(axis=1))[0]))
        nodes, sigma, ld2n = self.noise
        edge = self.logL[0]
        pieces = (self, self._band)
        cache = {}

        def cdfs(r):
            key = th[r].tobytes()
            if key not in cache:
                if len(cache) >= 4:
                    cache.clear()
                cache[key] = [p._cdfs(th[r]) for p in pieces]
            return cache[key]

        n_cand = np.zeros((R, nf, 2), dtype=np.int64)
        mean = np.zeros((R, nf, 2))
        for r in range(R):
            cd = cdfs(r)
            for p in range(2):
                mean[r, :, p] = cd[p][2]
                n_cand[r, :, p] = poisson(cd[p][2], rid[r], np.arange(nf) | (p * CUT_BAND), seed)
        if (n_cand < 0).any():
            r, f, p = np.argwhere(n_cand < 0)[0]
            raise MockError("row %d field %d: expected count %.17g is not finite, negative or above 2^31 (piece \"%s\")"
                            % (r, f, mean[r, f, p], PIECES[p]))
        cols = [[] for _ in range(6)]
        for r in range(R):
            if not n_cand[r].any():
                continue
            cd = cdfs(r)
            for f in range(nf):
                for p in range(2):
                    n = int(n_cand[r, f, p])
                    if not n:
                        continue
                    idx, fs = np.arange(n, dtype=np.uint64), f | (p * CUT_BAND)
                    z, L, k = pieces[p]._sources(th[r], rid[r], f, fs, seed, idx, cd[p])
                    sg = sigma_lookup(nodes, sigma[f], L - ld2n[k])
                    Lo = L + sg * _noise(rid[r], idx, fs, seed)
                    for c, v in zip(cols, (z, L, Lo, sg, np.full(n, f, dtype=np.int32), (Lo >= edge[k]).astype(np.int32))):
                        c.append(v)
        cat = lambda v, dt: np.concatenate(v).astype(dt) if v else np.zeros(0, dtype=dt)   # noqa: E731
        dts = (np.float64,) * 4 + (np.int32,) * 2
        return tuple(cat(c, dt) for c, dt in zip(cols, dts)) + (n_cand, mean)

    def draw_cut(self, thetas, seed, row_ids=None):
        """The catalogued sources of the cut process: (z, L_true, L_obs, sigma, field, offsets, info) - see compact_cut."""
        return compact_cut(*self.candidates_cut(thetas, seed, row_ids))

    def hist_cut(self, thetas, edges, seed, row_ids=None):
        """(hist (R, nf, nbins + 2) of the catalogued sources' L_obs, kept (R, nf))."""
        return self._binned(lambda: self.draw_cut(thetas, seed, row_ids), edges)


CUT_BAND = 0x400              # piece "below": ORed into the field word of the streams, purposes 4 + (0 .. 3) (lf_mock_cut.h)
PIECES = ("above", "below")


def check_cut_band(logLb, integ_part_b, logL, nf, table):
    """(logLb (S, S), integ_part_b (nf, S, S) or None) as float64, or MockError naming what lf_mock_set_cut_band refuses."""
    S = logL.shape[0]
    lb = np.ascontiguousarray(np.asarray(logLb, dtype=np.float64))
    if lb.shape != (S, S):
        raise MockError("logLb must be (S, S) = (%d, %d), got %s" % (S, S, lb.shape))
    bad = ~np.isfinite(lb)
    bad[1:] |= ~(np.diff(lb, axis=0) > 0)
    if bad.any():
        k, j = np.argwhere(bad.T)[0]
        raise MockError("column %d node %d: the band's luminosity nodes must be finite and strictly ascending" % (k, j))
    if (lb[-1] != logL[0]).any():
        raise MockError("column %d: row S - 1 of logLb must equal row 0 of logL (the edge of the cut)"
                        % int(np.flatnonzero(lb[-1] != logL[0])[0]))
    if not table:
        return lb, None
    if integ_part_b is None:
        raise MockError("FIXCOMP/ZEVOL need integ_part_b (the fixed completeness curve at the band's nodes)")
    ipb = np.ascontiguousarray(np.asarray(integ_part_b, dtype=np.float64))
    if ipb.shape != (nf, S, S):
        raise MockError("integ_part_b must be (nf, S, S) = (%d, %d, %d), got %s" % (nf, S, S, ipb.shape))
    bad = ~np.isfinite(ipb) | (ipb < 0.0)
    if bad.any():
        raise MockError("field %d: integ_part_b must be finite and >= 0" % int(np.argwhere(bad)[0][0]))
    return lb, ipb


def cut_depth(sigma, T=7.5):
    """H of the band: T (deconv.CUT_T) times the largest sigma over all fields and nodes."""
    return float(T) * float(np.max(sigma))


def band_grid(inp, H):
    """The band grid of the cut process for the inputs `inp`: (S, S), column k's S nodes equally spaced over
    [Lam_k - H, Lam_k], Lam_k = logL[0, k] (the last row is the edge, bit for bit)."""
    logL = np.asarray(inp["logL"], dtype=np.float64)
    if not (np.isfinite(H) and H > 0.0):
        raise MockError("the band's depth H must be finite and > 0 (an error model that is 0 everywhere needs no band)")
    S = logL.shape[0]
    out = np.empty((S, S))
    for k in range(S):
        out[:, k] = np.linspace(logL[0, k] - H, logL[0, k], S)
    out[-1] = logL[0]
    return out


def band_integ_part(inp, logLb):
    """integ_part of the band for FIXCOMP and ZEVOL inputs: (nf, S, S), volume_part[k] Omega_0[f] / sqarcsec times the modified
    Fleming curve at the fixed Flim0[f], alpha0 at the node's log10 flux logLb[j, k] - ld2n[k], in the form without
    cancellation that Delta B uses (deconv._cut_phi_omega), not the reference's spline."""
    from . import deconv
    from . import grad as G
    lb = np.asarray(logLb, dtype=np.float64)
    nf = len(inp["field_ind"]) - 1
    vp = np.asarray(inp["volume_part"], dtype=np.float64)
    logf = lb - ld2_nodes(inp["DL_zarr"])[None]
    kappa, aC = G._kappa(inp["fcmin"]), float(inp["alpha0"])
    out = np.empty((nf,) + lb.shape)
    with np.errstate(all="ignore"):
        for f in range(nf):
            Flim = float(np.asarray(inp["Flim0"], dtype=np.float64)[f])
            om0 = float(np.asarray(inp["Omega_0"], dtype=np.float64)[f]) / G.SQARCSEC
            y = (logf + 17.0) - np.log10(Flim)
            vv = 10.0 ** (logf + 17.0) * (np.exp(G.LN10 * kappa / aC) / Flim)
            out[f] = vp[None] * (om0 * np.exp(deconv._lcomp(y, vv, aC)))
    return np.where(np.isfinite(out), out, 0.0)


def compact_cut(z, L_true, L_obs, sigma, field, keep, n_cand, mean):
    """The catalogued sources of candidates_cut: (z, L_true, L_obs, sigma, field, offsets [R nf + 1], info), per (row, field)
    piece "above" in index order, then piece "below".  info: n_cand, mean (R, nf, 2), kept (R, nf), n_candidates (R, nf) and
    n_scattered_in (R, nf): the kept sources of piece "below", whose L_true lies below their edge (at it only when a hat's
    root rounds to 1, a chance of about 2^-53 per source)."""
    R, nf = n_cand.shape[:2]
    k = keep != 0
    seg = np.repeat(np.arange(R * nf * 2), n_cand.ravel())
    per = np.bincount(seg[k], minlength=R * nf * 2).reshape(R, nf, 2).astype(np.int64)
    kept = per.sum(axis=2)
    off = np.concatenate([[0], np.cumsum(kept.ravel())]).astype(np.int64)
    info = {"n_cand": n_cand, "mean": mean, "kept": kept, "n_candidates": n_cand.sum(axis=2), "n_scattered_in": per[:, :, 1]}
    return z[k], L_true[k], L_obs[k], sigma[k], field[k], off, info


MAX_NODES = 64                # lf_mock_noise.h: MOCK_MAX_NODES


def check_error_model(nodes, sigma, nf):
    """(nodes (M,), sigma (nf, M)) as float64, or MockError naming what lf_mock_set_error_model refuses."""
    x = np.ascontiguousarray(np.asarray(nodes, dtype=np.float64).ravel())
    M = x.size
    if M < 1 or M > MAX_NODES:
        raise MockError("M must be in 1..%d, got %d nodes" % (MAX_NODES, M))
    s = np.asarray(sigma, dtype=np.float64)
    if s.ndim == 1 and M == 1:
        s = s[:, None]
    if s.shape != (nf, M):
        raise MockError("sigma must be (nf, M) = (%d, %d), got %s" % (nf, M, s.shape))
    bad = ~np.isfinite(x)
    bad[1:] |= ~(np.diff(x) > 0)
    if bad.any():
        raise MockError("node %d: logf_nodes must be finite and strictly ascending" % int(np.flatnonzero(bad)[0]))
    bad = ~np.isfinite(s) | (s < 0.0)
    if bad.any():
        f, i = np.argwhere(bad)[0]
        raise MockError("field %d node %d: sigma must be finite and >= 0" % (f, i))
    return x, np.ascontiguousarray(s)


def ld2_nodes(dl_zarr):
    """log10(4 pi (Mpc DL_zarr)^2) at the redshift nodes (lf_mock_set_error_model's host arithmetic)."""
    dl = hs.MPC_CM * np.asarray(dl_zarr, dtype=np.float64)
    return np.log10(4.0 * 3.141592653589793 * (dl * dl))


def log_flux(zarr, ld2n, z, L):
    """log10 flux (cgs) of sources (z, L): L - ld2(z), ld2 linear between the nodes (lf_mock_noise.h: mock_logflux)."""
    i = np.clip(np.searchsorted(zarr, z, side="right") - 1, 0, zarr.size - 2)
    ld2 = ld2n[i] + (z - zarr[i]) * ((ld2n[i + 1] - ld2n[i]) / (zarr[i + 1] - zarr[i]))
    return L - ld2


def sigma_lookup(nodes, sig, t):
    """One field's sigma at log10 flux t: linear between the nodes, constant outside (lf_mock_noise.h: mock_sigma)."""
    t = np.asarray(t, dtype=np.float64)
    M = nodes.size
    if M == 1:
        return np.full(t.shape, sig[0])
    i = np.clip(np.searchsorted(nodes, t, side="right") - 1, 0, M - 2)
    mid = sig[i] + (t - nodes[i]) * ((sig[i + 1] - sig[i]) / (nodes[i + 1] - nodes[i]))
    return np.where(~(t > nodes[0]), sig[0], np.where(t >= nodes[-1], sig[-1], mid))


def error_model_from_catalogue(logf, sigma, field_ind, nodes=16):
    """The error model a catalogue shows: (nodes (M,), sigma (nf, M)) for set_error_model.  The pooled log10 fluxes are cut
    into `nodes` equal-count bins (in sorted order, ties by position: deterministic); a node is the pooled median log flux
    of its bin, its value for field f the median sigma of f's sources in the bin.  A bin empty for a field takes the value
    of that field's nearest filled bin (the lower one at equal distance), a field without sources the pooled medians;
    nodes that coincide are merged (their sources pooled)."""
    logf = np.asarray(logf, dtype=np.float64).ravel()
    sigma = np.asarray(sigma, dtype=np.float64).ravel()
    fi = np.asarray(field_ind, dtype=np.int64).ravel()
    nf, N = fi.size - 1, logf.size
    if sigma.size != N or fi[-1] != N or fi[0] != 0 or (np.diff(fi) < 0).any():
        raise ValueError("logf, sigma and field_ind do not describe one catalogue")
    if N < 1:
        raise ValueError("the catalogue is empty")
    if not (np.isfinite(logf).all() and np.isfinite(sigma).all() and (sigma >= 0).all()):
        raise ValueError("logf must be finite and sigma finite and >= 0")
    nb = int(min(max(int(nodes), 1), MAX_NODES, N))
    fld = np.repeat(np.arange(nf), np.diff(fi))
    order = np.argsort(logf, kind="stable")
    cut = (np.arange(nb + 1) * N) // nb
    x = np.array([np.median(logf[order[cut[b]:cut[b + 1]]]) for b in range(nb)])
    # merge bins whose nodes coincide
    groups = [[0]]
    for b in range(1, nb):
        if x[b] > x[groups[-1][0]]:
            groups.append([b])
        else:
            groups[-1].append(b)
    M = len(groups)
    xs, pooled, val = np.empty(M), np.empty(M), np.full((nf, M), np.nan)
    for g, bins in enumerate(groups):
        idx = order[cut[bins[0]]:cut[bins[-1] + 1]]
        xs[g] = np.median(logf[idx])
        pooled[g] = np.median(sigma[idx])
        for f in range(nf):
            own = idx[fld[idx] == f]
            if own.size:
                val[f, g] = np.median(sigma[own])
    for f in range(nf):
        have = np.flatnonzero(~np.isnan(val[f]))
        if have.size == 0:
            val[f] = pooled
            continue
        for g in np.flatnonzero(np.isnan(val[f])):
            val[f, g] = val[f, have[np.argmin(np.abs(have - g))]]       # (argmin: the first, i.e. lower, at a tie)
    return xs, val


def _edges(edges):
    e = np.ascontiguousarray(np.asarray(edges, dtype=np.float64).ravel())
    if e.size < 2 or e.size - 1 > MAX_BINS:
        raise ValueError("edges must hold 2 .. %d values" % (MAX_BINS + 1))
    if not np.isfinite(e).all() or (np.diff(e) < 0).any():
        raise ValueError("edges must be finite and non-decreasing")
    return e


def bin_sources(logL, offsets, edges):
    """[len(offsets) - 1, nbins + 2] histogram of each segment of logL by searchsorted(edges, x, side="right")."""
    ns = len(edges) + 1
    slot = np.searchsorted(edges, logL, side="right")
    seg = np.repeat(np.arange(len(offsets) - 1), np.diff(offsets))
    return np.bincount(seg * ns + slot, minlength=(len(offsets) - 1) * ns).reshape(-1, ns).astype(np.int64)


def _edges2(z_edges, edges):
    """(z_edges, edges) as lf_mock_hist2 takes them, or ValueError naming what it refuses"""
    try:
        ze = _edges(z_edges)
    except ValueError as err:
        raise ValueError("z_%s" % err)
    e = _edges(edges)
    if (ze.size + 1) * (e.size + 1) > MAX_SLOTS2:
        raise ValueError("(nz + 2) * (nl + 2) = %d slots: the limit is %d" % ((ze.size + 1) * (e.size + 1), MAX_SLOTS2))
    return ze, e


def bin_sources2(z, logL, offsets, z_edges, edges):
    """[len(offsets) - 1, nz + 2, nl + 2] histogram of each segment of the sources (z, logL): the slot on either axis is
    searchsorted(axis edges, x, side="right") - 0 below the first edge, n + 1 at or above the last.  Summed over the redshift
    slots it is bin_sources(logL, offsets, edges)."""
    nzs, nls = len(z_edges) + 1, len(edges) + 1
    sz = np.searchsorted(z_edges, z, side="right")
    sl = np.searchsorted(edges, logL, side="right")
    nseg = len(offsets) - 1
    seg = np.repeat(np.arange(nseg), np.diff(offsets))
    return np.bincount((seg * nzs + sz) * nls + sl, minlength=nseg * nzs * nls).reshape(nseg, nzs, nls).astype(np.int64)


# --------------------------------------------------------------------------------------------------------------- device
def _i64(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)) if a is not None else None


def _i32(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)) if a is not None else None


class MockGenerator(object):
    """lf_mock_* on the GPU.  `inputs` is the dict LFContext takes (kernel_inputs()); the catalogue arrays are not read."""

    def __init__(self, inputs, device=0):
        from . import capi
        lib = capi.load()
        self._lib, self._h = lib, None
        inp = inputs
        variant = inp["variant"]
        if variant not in capi.VARIANTS:
            raise ValueError("variant must be one of %s" % (sorted(capi.VARIANTS),))
        self.variant = variant
        self.nf = len(inp["field_ind"]) - 1
        logL = capi._f64(inp["logL"])
        S = logL.shape[0]
        if logL.shape != (S, S):
            raise ValueError("logL must be (S, S)")
        self.S = S
        self.fix_sch_al = bool(inp.get("fix_sch_al", False))
        self.ndim = _ndim(variant, self.fix_sch_al, self.nf)
        keep = {"logL": logL, "zarr": capi._f64(inp["zarr"]), "omega0": capi._f64(inp["Omega_0"])}
        if variant == "free":
            keep["volume_part"] = capi._f64(inp["volume_part"])
            keep["dl_zarr"] = capi._f64(inp["DL_zarr"])
        else:
            keep["integ_part"] = _integ_part(inp, self.nf, S)
            if keep["integ_part"].shape != (self.nf, S, S):
                raise ValueError("integ_part must be (nf, S, S)")
        d = capi.LfDesc()
        d.variant = capi.VARIANTS[variant]
        d.fix_sch_al = 1 if self.fix_sch_al else 0
        d.nf, d.S, d.N = self.nf, S, 0
        for k in ("logL", "zarr", "omega0", "volume_part", "dl_zarr", "integ_part"):
            setattr(d, k, capi._ptr(keep.get(k)))
        d.sch_al0 = float(inp.get("sch_al0", 0.0))
        d.fcmin = float(inp.get("fcmin", 0.1))
        piv = inp.get("pivots", (1.20, 1.53, 1.86))
        for i in range(3):
            d.pivots[i] = float(piv[i])
        lims = inp.get("lims")
        if lims:
            for i, name in enumerate(capi.LIM_ORDER):
                d.lims[i][0], d.lims[i][1] = float(lims[name][0]), float(lims[name][1])
        d.device = int(device)
        h = lib.lf_mock_create(ctypes.byref(d))
        if not h:
            raise capi.LFError(lib.lf_mock_last_error(None).decode())
        self._h = ctypes.c_void_p(h)
        self.device = int(device)
        self._dl_zarr = inp.get("DL_zarr")    # every variant's kernel_inputs() has it; only the error model needs it

    def _check(self, rc):
        from . import capi
        if rc == capi.LF_ERR_ARG:
            raise MockError(self._lib.lf_mock_last_error(self._h).decode())
        if rc != capi.LF_OK:
            raise capi.LFError("liblfmcmc error %d: %s" % (rc, self._lib.lf_mock_last_error(self._h).decode()))

    def _head(self, thetas, seed, row_ids):
        """(thetas (R, ndim), R, row ids, the five arguments every lf_mock_* call starts with)"""
        from . import capi
        th = _rows(thetas, self.ndim)
        R = th.shape[0]
        rid = _row_ids(row_ids, R)
        return th, R, rid, (self._h, capi._ptr(th), R, _i64(rid), ctypes.c_uint64(int(seed)))

    def _need_band(self):
        """a generator on which set_cut_band was never called lets the library refuse"""
        if not getattr(self, "_band_set", True):
            raise MockError("no cut band is set (set_cut_band, after set_error_model)")

    def counts(self, thetas, seed, row_ids=None):
        """(mean (R, nf), count (R, nf) int64): expected counts M and their Poisson draws."""
        from . import capi
        th, R, rid, head = self._head(thetas, seed, row_ids)
        mean = np.empty((R, self.nf))
        cnt = np.empty((R, self.nf), dtype=np.int64)
        self._check(self._lib.lf_mock_counts(*head, capi._ptr(mean), _i64(cnt)))
        return mean, cnt

    def _draw(self, entry, thetas, seed, row_ids, count, ncol):
        """lf_mock_draw (ncol = 2 columns of doubles: z, logL) and lf_mock_draw_err (4: z, L_true, L_obs, sigma): the columns,
        field, offsets"""
        from . import capi
        th, R, rid, head = self._head(thetas, seed, row_ids)
        if count is None:
            count = self.counts(th, seed, rid)[1]
        cnt = np.ascontiguousarray(np.asarray(count, dtype=np.int64).reshape(R, self.nf))
        total = int(cnt.sum())
        cols = tuple(np.empty(total) for _ in range(ncol))
        fld = np.empty(total, dtype=np.int32)
        self._check(getattr(self._lib, entry)(*head, _i64(cnt), *[capi._ptr(c) for c in cols], _i32(fld)))
        return cols + (fld, np.concatenate([[0], np.cumsum(cnt.ravel())]).astype(np.int64))

    def draw(self, thetas, seed, row_ids=None, count=None):
        """(z, logL, field, offsets): the sources of every (row, field) in that order (count: from .counts unless given);
        sources of (r, f) are [offsets[r nf + f], offsets[r nf + f + 1])."""
        return self._draw("lf_mock_draw", thetas, seed, row_ids, count, 2)

    def _hist1(self, entry, thetas, edges, seed, row_ids, with_kept):
        from . import capi
        th, R, rid, head = self._head(thetas, seed, row_ids)
        if with_kept:
            self._need_band()
        e = _edges(edges)
        out = np.empty((R, self.nf, e.size + 1), dtype=np.int64)
        kept = np.empty((R, self.nf), dtype=np.int64) if with_kept else None
        self._check(getattr(self._lib, entry)(*head, e.size - 1, capi._ptr(e), _i64(out), *([_i64(kept)] if with_kept else [])))
        return (out, kept) if with_kept else out

    def hist(self, thetas, edges, seed, row_ids=None):
        """(R, nf, nbins + 2) int64: logL of every (row, field) binned by searchsorted(edges, x, side="right")."""
        return self._hist1("lf_mock_hist", thetas, edges, seed, row_ids, False)

    # ---------------------------------------------------------------- the observation step (lf_mock_noise.h)
    def set_error_model(self, nodes, sigma):
        """As MockTwin.set_error_model, uploaded through lf_mock_set_error_model (which validates again)."""
        from . import capi
        if nodes is None:
            self._check(self._lib.lf_mock_set_error_model(self._h, 0, None, None, None))
            return
        x, s = check_error_model(nodes, sigma, self.nf)
        if self._dl_zarr is None:
            raise MockError("the inputs hold no DL_zarr: the error model needs it for the sources' fluxes")
        dl = capi._f64(self._dl_zarr)
        if dl.shape != (self.S,):
            raise MockError("DL_zarr must hold S finite values > 0")
        self._check(self._lib.lf_mock_set_error_model(self._h, x.size, capi._ptr(x), capi._ptr(s), capi._ptr(dl)))

    def draw_noisy(self, thetas, seed, row_ids=None, count=None):
        """(z, L_true, L_obs, sigma, field, offsets): draw()'s sources and what the catalogue records of them, the noise
        added on the device (lf_mock_draw_err)."""
        return self._draw("lf_mock_draw_err", thetas, seed, row_ids, count, 4)

    def hist_noisy(self, thetas, edges, seed, row_ids=None):
        """hist() of the observed luminosities (lf_mock_hist_err)."""
        return self._hist1("lf_mock_hist_err", thetas, edges, seed, row_ids, False)

    # ---------------------------------------------------------------- the cut process (lf_mock_cut.h)
    def set_cut_band(self, logLb, integ_part_b=None):
        """As MockTwin.set_cut_band, uploaded through lf_mock_set_cut_band (which validates again).  None: a band stays on
        the device until the next set_error_model; the calls below then refuse through this flag."""
        from . import capi
        self._band_set = False
        if logLb is None:
            return
        lb = capi._f64(logLb)
        if lb.shape != (self.S, self.S):
            raise MockError("logLb must be (S, S) = (%d, %d), got %s" % (self.S, self.S, lb.shape))
        ipb = None
        if integ_part_b is not None and self.variant != "free":
            ipb = capi._f64(integ_part_b)
            if ipb.shape != (self.nf, self.S, self.S):
                raise MockError("integ_part_b must be (nf, S, S) = (%d, %d, %d), got %s" % (self.nf, self.S, self.S, ipb.shape))
        self._check(self._lib.lf_mock_set_cut_band(self._h, capi._ptr(lb), capi._ptr(ipb)))
        self._band_set = True

    def candidates_cut(self, thetas, seed, row_ids=None):
        """As MockTwin.candidates_cut, drawn, observed and cut on the device (lf_mock_draw_cut)."""
        from . import capi
        th, R, rid, head = self._head(thetas, seed, row_ids)
        self._need_band()
        n_cand = np.zeros((R, self.nf, 2), dtype=np.int64)
        mean = np.zeros((R, self.nf, 2))
        kept = np.zeros((R, self.nf), dtype=np.int64)

        def call(cap, z, L, Lobs, sg, fld, keep):
            self._check(self._lib.lf_mock_draw_cut(*head, cap, capi._ptr(z), capi._ptr(L), capi._ptr(Lobs), capi._ptr(sg), _i32(fld),
                                                   _i32(keep), _i64(n_cand), capi._ptr(mean), _i64(kept)))

        call(0, None, None, None, None, None, None)
        total = int(n_cand.sum())
        z, L, Lobs, sg = np.empty(total), np.empty(total), np.empty(total), np.empty(total)
        fld, keep = np.empty(total, dtype=np.int32), np.empty(total, dtype=np.int32)
        if total:
            call(total, z, L, Lobs, sg, fld, keep)
        return z, L, Lobs, sg, fld, keep, n_cand, mean

    def draw_cut(self, thetas, seed, row_ids=None):
        """The catalogued sources of the cut process: (z, L_true, L_obs, sigma, field, offsets, info) - see compact_cut (the
        compaction runs on the host: the arrays are copied there anyway)."""
        return compact_cut(*self.candidates_cut(thetas, seed, row_ids))

    def hist_cut(self, thetas, edges, seed, row_ids=None):
        """(hist (R, nf, nbins + 2) of the catalogued sources' L_obs, kept (R, nf)) without writing sources (lf_mock_hist_cut)."""
        return self._hist1("lf_mock_hist_cut", thetas, edges, seed, row_ids, True)

    # ---------------------------------------------------------------- binned in (z, L) (lf_mock_hist2.h)
    def _hist2(self, entry, thetas, z_edges, edges, seed, row_ids, count, with_kept):
        from . import capi
        ze, e = _edges2(z_edges, edges)         # (first: a refused grid reaches no library call)
        th, R, rid, head = self._head(thetas, seed, row_ids)
        out = np.empty((R, self.nf, ze.size + 1, e.size + 1), dtype=np.int64)
        grid = (ze.size - 1, capi._ptr(ze), e.size - 1, capi._ptr(e), _i64(out))
        if with_kept:
            kept = np.empty((R, self.nf), dtype=np.int64)
            self._check(getattr(self._lib, entry)(*head, *grid, _i64(kept)))
            return out, kept
        cnt = None
        if count is not None:
            cnt = np.ascontiguousarray(np.asarray(count, dtype=np.int64).reshape(R, self.nf))
        self._check(getattr(self._lib, entry)(*head, _i64(cnt), *grid))
        return out

    def hist2(self, thetas, z_edges, edges, seed, row_ids=None, count=None):
        """(R, nf, nz + 2, nl + 2) int64: (z, logL) of every (row, field) binned as bin_sources2 bins them, without writing
        sources (lf_mock_hist2).  count: None = the Poisson counts, else (R, nf) as draw takes it."""
        return self._hist2("lf_mock_hist2", thetas, z_edges, edges, seed, row_ids, count, False)

    def hist2_noisy(self, thetas, z_edges, edges, seed, row_ids=None, count=None):
        """hist2() of the true redshifts and the observed luminosities (lf_mock_hist2_err)."""
        return self._hist2("lf_mock_hist2_err", thetas, z_edges, edges, seed, row_ids, count, False)

    def hist2_cut(self, thetas, z_edges, edges, seed, row_ids=None):
        """(hist (R, nf, nz + 2, nl + 2) of the catalogued sources' (z, L_obs), kept (R, nf)) (lf_mock_hist2_cut)."""
        _edges2(z_edges, edges)
        self._need_band()
        return self._hist2("lf_mock_hist2_cut", thetas, z_edges, edges, seed, row_ids, None, True)

    def close(self):
        if self._h is not None:
            self._lib.lf_mock_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def generator(inputs, device=True, device_index=0):
    """MockGenerator on the GPU (device=True) or the NumPy MockTwin."""
    return MockGenerator(inputs, device=device_index) if device else MockTwin(inputs)


NOISE_PURPOSE = 3             # the Philox purpose tag of the measurement noise (0: counts, 1 and 2: the sources; lf_mock.h)


def lum_noise(n_per_field, row_id, seed):
    """Standard normal deviates of the sources 0 .. n_f - 1 of every field f of one row (concatenated field by field):
    Box-Muller on the two 53-bit uniforms of the Philox block (row_id, index, NOISE_PURPOSE, f) - a stream of its own, so the
    noiseless draws keep their bits.  Host arithmetic for both generators."""
    out = [_noise(row_id, np.arange(int(n), dtype=np.uint64), f, seed) for f, n in enumerate(n_per_field)]
    return np.concatenate(out) if out else np.zeros(0)


def _noise(row_id, index, fs, seed):
    """lum_noise's deviates of the sources `index` of one field word fs (f; the band of the cut process: f | CUT_BAND)"""
    w = _words(row_id, index, NOISE_PURPOSE, fs, seed)
    u1, u2 = philox.u53(w[0], w[1]), philox.u53(w[2], w[3])
    return np.sqrt(-2.0 * np.log1p(-u1)) * np.cos(2.0 * np.pi * u2)                  # (1 - u1 in (0, 1]: no log of 0)


def catalogue_lists(z, logL, field, nf, lum_err=None, seed=0, row_id=0):
    """Per-field lists in the form the model constructors take: z, lum, lum_e, field_ind.  lum_err=None: lum as drawn and
    lum_e zeros.  lum_err a scalar or one value per field (dex): Gaussian noise of that width is added to every drawn logL
    (after detection: the model of DESIGN.md section 3.18) from lum_noise's stream, lum_e is filled with it, and the
    noiseless luminosities are returned as lum_true."""
    order = np.argsort(field, kind="stable")
    z, logL, field = z[order], logL[order], field[order]
    fi = np.concatenate([[0], np.cumsum(np.bincount(field, minlength=nf))]).astype(np.int64)
    split = lambda a: [a[fi[f]:fi[f + 1]].copy() for f in range(nf)]    # noqa: E731
    if lum_err is None:
        return {"z": split(z), "lum": split(logL), "lum_e": [np.zeros(fi[f + 1] - fi[f]) for f in range(nf)], "field_ind": fi}
    sg = np.asarray(lum_err, dtype=np.float64)
    if sg.ndim == 0:
        sg = np.full(nf, float(sg))
    if sg.shape != (nf,) or not np.all(np.isfinite(sg)) or np.any(sg < 0.0):
        raise ValueError("lum_err must be a finite scalar >= 0 or one such value per field")
    per = np.repeat(sg, np.diff(fi))
    noisy = logL + per * lum_noise(np.diff(fi), row_id, seed)
    return {"z": split(z), "lum": split(noisy), "lum_e": split(per), "field_ind": fi, "lum_true": split(logL)}


def observed_lists(z, logL_true, logL_obs, sigma, field, nf):
    """catalogue_lists for one row of draw_noisy: lum the observed luminosities, lum_e the per-source sigma, lum_true the
    noiseless values."""
    fi = np.concatenate([[0], np.cumsum(np.bincount(field, minlength=nf))]).astype(np.int64)     # (a row is in field order)
    split = lambda a: [a[fi[f]:fi[f + 1]].copy() for f in range(nf)]    # noqa: E731
    return {"z": split(z), "lum": split(logL_obs), "lum_e": split(sigma), "field_ind": fi, "lum_true": split(logL_true)}


def predictive(gen, rows, edges, observed_lum, observed_fi, seed, noisy=False, cut=False):
    """Posterior predictive check of the logL histogram per field: `rows` (R, ndim) posterior draws, `edges` (B + 1),
    the observed catalogue's lum and field_ind.  noisy: the replicates are binned by their observed luminosities under
    the generator's error model (hist_noisy).  cut: the replicates are catalogues of the cut process (hist_cut; the generator
    holds an error model and a band) - `replicated` then bins the catalogued sources only, and the dict also holds
    `replicated_kept` (R, nf), their number.  `expected` stays the count above the edge before the observation, B.  Returns the
    dict of _Base.posterior_predictive."""
    edges = _edges(edges)
    nf = len(observed_fi) - 1
    obs = bin_sources(np.asarray(observed_lum, dtype=np.float64), np.asarray(observed_fi, dtype=np.int64), edges)
    kept = None
    if cut:
        rep, kept = gen.hist_cut(rows, edges, seed)
    else:
        rep = gen.hist_noisy(rows, edges, seed) if noisy else gen.hist(rows, edges, seed)
    expected = gen.counts(rows, seed)[0]
    obs_tot, rep_tot = obs.sum(axis=1), rep.sum(axis=2)
    extra = {"replicated_kept": kept} if cut else {}
    return {**extra, "edges": edges, "observed": obs, "replicated": rep, "expected": expected,
            "percentiles": np.percentile(rep, (16.0, 50.0, 84.0), axis=0),
            "p_upper": np.mean(rep >= obs[None], axis=0), "p_lower": np.mean(rep <= obs[None], axis=0),
            "observed_total": obs_tot, "replicated_total": rep_tot,
            "p_upper_total": np.mean(rep_tot >= obs_tot[None], axis=0), "p_lower_total": np.mean(rep_tot <= obs_tot[None], axis=0),
            "seed": int(seed), "nf": nf}


def deviance(observed, replicated):
    """The omnibus statistic of a 2-D predictive check, per field.  observed [nf, ...cells], replicated [R, nf, ...cells].
    With m the replicates' mean per cell, D(h) = 2 sum_cells [m - h + h ln(h / m)] (h ln h = 0 at h = 0) over the cells with
    m > 0.  Returns (D(observed) [nf], D per replicate [R, nf], p = mean(D_rep >= D_obs) [nf], the number of cells with m = 0
    [nf], the observed sources in those cells [nf])."""
    rep = np.asarray(replicated, dtype=np.float64)
    R, nf = rep.shape[:2]
    rep = rep.reshape(R, nf, -1)
    obs = np.asarray(observed, dtype=np.float64).reshape(nf, -1)
    m = rep.mean(axis=0)
    live = m > 0.0
    msafe = np.where(live, m, 1.0)

    def D(h):
        with np.errstate(divide="ignore", invalid="ignore"):
            t = np.where(h > 0.0, h * np.log(h / msafe), 0.0)
        return 2.0 * np.where(live, msafe - h + t, 0.0).sum(axis=-1)

    d_obs, d_rep = D(obs), D(rep)
    return (d_obs, d_rep, np.mean(d_rep >= d_obs[None], axis=0), (~live).sum(axis=1).astype(np.int64),
            np.where(live, 0.0, obs).sum(axis=1).astype(np.int64))


def predictive2(gen, rows, z_edges, edges, observed_z, observed_lum, observed_fi, seed, noisy=False, cut=False):
    """predictive() with the redshift axis: the replicates are binned in (z, logL) by hist2 (hist2_noisy,
    hist2_cut) and every entry of predictive() is computed from that histogram's marginal over the redshift slots - the same
    integers predictive() returns for the same seed.  On top of them: z_edges; observed_2d [nf, nz + 2, nl + 2],
    replicated_2d [R, nf, nz + 2, nl + 2], percentiles_2d (16, 50, 84), p_upper_2d, p_lower_2d per cell; the N(z) marginal
    observed_z [nf, nz + 2], replicated_z [R, nf, nz + 2], percentiles_z, p_upper_z, p_lower_z; and the omnibus statistic of
    deviance() per field: deviance, replicated_deviance [R, nf], p_deviance, n_empty_cells, observed_in_empty."""
    ze, edges = _edges2(z_edges, edges)
    fi = np.asarray(observed_fi, dtype=np.int64)
    nf = len(fi) - 1
    obs2 = bin_sources2(np.asarray(observed_z, dtype=np.float64), np.asarray(observed_lum, dtype=np.float64), fi, ze, edges)
    kept = None
    if cut:
        rep2, kept = gen.hist2_cut(rows, ze, edges, seed)
    else:
        rep2 = gen.hist2_noisy(rows, ze, edges, seed) if noisy else gen.hist2(rows, ze, edges, seed)
    expected = gen.counts(rows, seed)[0]
    obs, rep = obs2.sum(axis=1), rep2.sum(axis=2)
    obs_z, rep_z = obs2.sum(axis=2), rep2.sum(axis=3)
    obs_tot, rep_tot = obs.sum(axis=1), rep.sum(axis=2)
    d_obs, d_rep, p_dev, n_empty, in_empty = deviance(obs2, rep2)
    extra = {"replicated_kept": kept} if cut else {}
    pct = (16.0, 50.0, 84.0)
    return {**extra, "edges": edges, "observed": obs, "replicated": rep, "expected": expected,
            "percentiles": np.percentile(rep, pct, axis=0),
            "p_upper": np.mean(rep >= obs[None], axis=0), "p_lower": np.mean(rep <= obs[None], axis=0),
            "observed_total": obs_tot, "replicated_total": rep_tot,
            "p_upper_total": np.mean(rep_tot >= obs_tot[None], axis=0), "p_lower_total": np.mean(rep_tot <= obs_tot[None], axis=0),
            "seed": int(seed), "nf": nf,
            "z_edges": ze, "observed_2d": obs2, "replicated_2d": rep2, "percentiles_2d": np.percentile(rep2, pct, axis=0),
            "p_upper_2d": np.mean(rep2 >= obs2[None], axis=0), "p_lower_2d": np.mean(rep2 <= obs2[None], axis=0),
            "observed_z": obs_z, "replicated_z": rep_z, "percentiles_z": np.percentile(rep_z, pct, axis=0),
            "p_upper_z": np.mean(rep_z >= obs_z[None], axis=0), "p_lower_z": np.mean(rep_z <= obs_z[None], axis=0),
            "deviance": d_obs, "replicated_deviance": d_rep, "p_deviance": p_dev, "n_empty_cells": n_empty,
            "observed_in_empty": in_empty}
