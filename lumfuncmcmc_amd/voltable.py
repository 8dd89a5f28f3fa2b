"""The comoving volume out to the redshift of a luminosity distance, as a table the device evaluates per (source, draw)
(lf_veff_draws_zmax of include/lfmcmc.h, csrc/lf_veffdraws.h).

    V(D) = int_{zmin}^{min(zmax, DL^-1(D))} dV/dz dz,   0 for DL^-1(D) <= zmin

with dV/dz the piecewise-linear interpolant dVdzf, exactly as veff.comoving_volume integrates it.  Between two nodes of
dVdzf the integrand is linear in z, so V is an exact quadratic in z there; all that has to be approximated is the smooth
z = DL^-1(D).  The table is V(D) as piecewise polynomials in D, kept in factored form:

  * node pieces: the knots t_0 = zmin < the nodes of dVdzf inside (zmin, zmax) < t_K = zmax and their images D_k = DL(t_k).
    Piece k is chosen by D_k <= D < D_k+1 (that k is unique, so the host's search and the device's find the same one) - the pieces are aligned to the nodes' images, where V'' has its kinks - and is
    V = c0_k + (y_k + hs_k dz) dz, dz = z - t_k, clamped into [c0_k, c0_k+1]; c0_k is the twin's own V at t_k.  So V is
    non-decreasing across every node edge by construction, exactly 0 at D <= D_0 and exactly the twin's full volume at
    D >= D_K.
  * z pieces: NPIECE equal pieces in D over [D_0, D_K], each a polynomial of degree DEG in the piece's own t in [0, 1)
    (Chebyshev interpolation of the inverse, iterated to 1e-15, then the power basis).

`VolumeTable.eval` is the device's evaluation operation by operation (IEEE products and sums, no contraction), so it
returns the device's bits (held per element on the device by tests/test_gpu_volterms.py, and against a 40-digit reference by
tests/test_volterms_cpu.py); `VolumeTable.validate` measures eps_T = max |V_table - V_twin| / V_total.
"""
import numpy as np

from . import veff

NPIECE = 32            # z pieces (VEFFZ_NPIECE of csrc/lf_veffdraws.h)
DEG = 7                # their degree (VEFFZ_DEG)
REC = 8                # doubles per node record: D_k, D_k+1, t_k, c0_k, c0_k+1, y_k, hs_k, 0
HEAD = 8               # D_0, D_K, V_total, NPIECE / (D_K - D_0), first inner node, 1 / node spacing, 0, 0


def _inverse(D, cosmo):
    """DL^-1 to a tighter stop than the twin's 1e-13 (the validation's yardstick)"""
    return veff.redshift_at_distance(D, cosmo, tol=1e-15, maxit=12)


class VolumeTable(object):
    def __init__(self, head, zc, rec, eps=None):
        self.head = np.ascontiguousarray(head, dtype=np.float64)
        self.zc = np.ascontiguousarray(zc, dtype=np.float64)              # (NPIECE, DEG + 1), constant term first
        self.rec = np.ascontiguousarray(rec, dtype=np.float64)            # (K, REC)
        self.eps = eps

    @property
    def d_lo(self):
        return self.head[0]

    @property
    def d_hi(self):
        return self.head[1]

    @property
    def v_total(self):
        return self.head[2]

    def edges(self):
        """Every piece edge in D: the nodes' images and the z pieces' boundaries"""
        inner = self.d_lo + np.arange(1, NPIECE) / self.head[3]
        return np.unique(np.concatenate([self.rec[:, 0], [self.d_hi], inner]))

    def redshift(self, D):
        """The z pieces alone (for D inside the table)"""
        D = np.asarray(D, dtype=np.float64)
        u = (D - self.head[0]) * self.head[3]
        p = np.minimum(u.astype(np.int64), NPIECE - 1)
        t = u - p
        c = self.zc[p]
        z = c[..., DEG]
        for j in range(DEG - 1, -1, -1):
            z = z * t + c[..., j]
        return z

    def eval(self, D):
        """V(D) with the device's operations in the device's order"""
        D = np.atleast_1d(np.asarray(D, dtype=np.float64))
        out = np.zeros(D.shape)
        out[D >= self.d_hi] = self.v_total                       # NaN: neither clamp nor piece -> 0, like the twin
        m = (D > self.d_lo) & (D < self.d_hi)
        if not m.any():
            return out
        d = D[m]
        z = self.redshift(d)
        K = len(self.rec)
        g = np.floor((z - self.head[4]) * self.head[5]) + 1.0
        k = np.minimum(np.maximum(g, 0.0), K - 1.0).astype(np.int64)
        while True:
            dn = (k > 0) & (d < self.rec[k, 0])
            up = (k < K - 1) & (d >= self.rec[k, 1])
            if not (dn.any() or up.any()):
                break
            k = k - dn + up
        r = self.rec[k]
        dz = z - r[:, 2]
        v = r[:, 3] + (r[:, 5] + r[:, 6] * dz) * dz
        out[m] = np.minimum(np.maximum(v, r[:, 3]), r[:, 4])
        return out

    def validate(self, cosmo, dVdzf, zmin, zmax, nsample=100000):
        """eps_T against the twin's V on nsample values uniform in log D, both neighbours of every piece edge, the
        edges and both clamps; raises if V decreases across an edge or a clamp is not exact."""
        e = self.edges()
        lo, hi = np.nextafter(e, -np.inf), np.nextafter(e, np.inf)
        ve, vlo, vhi = self.eval(e), self.eval(lo), self.eval(hi)
        if not (np.all(vlo <= ve) and np.all(ve <= vhi)):
            raise ValueError("the volume table decreases across a piece edge")
        full = veff.comoving_volume(dVdzf, zmin, np.array([zmax]))[0]
        if not (self.eval([self.d_hi, 2.0 * self.d_hi, np.inf]) == full).all() or self.v_total != full:
            raise ValueError("the volume table's upper clamp is not the twin's full volume")
        if not (self.eval([self.d_lo, 0.5 * self.d_lo, 0.0]) == 0.0).all():
            raise ValueError("the volume table's lower clamp is not 0")
        D = np.concatenate([np.exp(np.linspace(np.log(self.d_lo), np.log(self.d_hi), nsample)), e, lo, hi,
                            [0.5 * self.d_lo, 2.0 * self.d_hi]])
        zt = np.minimum(zmax, _inverse(D, cosmo))
        want = veff.comoving_volume(dVdzf, zmin, zt)
        self.eps = float(np.max(np.abs(self.eval(D) - want)) / full)
        return self.eps


EPS_MAX = 1e-13        # what a table must hold, in units of V_total, to be used


def require(tab):
    """tab, or ValueError when it was not validated or misses EPS_MAX: the one place where a table is refused"""
    if tab.eps is None or not tab.eps <= EPS_MAX:
        raise ValueError("the volume table %s: %g of the total volume is required (equal pieces in D suit a survey's redshift "
                         "window, not a wide range)" % ("was not validated" if tab.eps is None else "reaches only %.1e" % tab.eps, EPS_MAX))
    return tab


def build(cosmo, dVdzf, zmin, zmax, validate=True, nsample=100000):
    """The table of V(D) for (cosmo, dVdzf, zmin, zmax); validate: measure .eps (VolumeTable.validate)."""
    zmin, zmax = float(zmin), float(zmax)
    x = dVdzf.x
    if not (zmax > zmin) or zmin < x[0] or zmax > x[-1]:
        raise ValueError("zmin < zmax inside dVdzf's nodes is required")
    inner = x[(x > zmin) & (x < zmax)]
    t = np.concatenate([[zmin], inner, [zmax]])
    K = len(t) - 1
    Dk = np.asarray(cosmo.luminosity_distance(t), dtype=np.float64)
    if not np.all(np.diff(Dk) > 0):
        raise ValueError("the luminosity distance does not resolve dVdzf's nodes")
    c0 = veff.comoving_volume(dVdzf, zmin, t)                        # the twin's own doubles; c0[0] = 0
    c0 = np.maximum.accumulate(c0)
    y = dVdzf(t[:-1])
    mid = 0.5 * (t[:-1] + t[1:])
    hi = np.searchsorted(x, mid).clip(1, len(x) - 1)
    slope = (dVdzf.y[hi] - dVdzf.y[hi - 1]) / (x[hi] - x[hi - 1])
    rec = np.zeros((K, REC))
    rec[:, 0], rec[:, 1], rec[:, 2], rec[:, 3], rec[:, 4], rec[:, 5], rec[:, 6] = Dk[:-1], Dk[1:], t[:-1], c0[:-1], c0[1:], y, 0.5 * slope
    if len(inner) > 1:
        first, inv_h = inner[0], (len(inner) - 1) / (inner[-1] - inner[0])
    else:
        first, inv_h = (inner[0] if len(inner) else zmin), 0.0
    d_lo, d_hi = Dk[0], Dk[-1]
    invw = NPIECE / (d_hi - d_lo)
    # z pieces: Chebyshev interpolation of DL^-1 on each piece, in t = (D - D_0) invw - p
    from numpy.polynomial import chebyshev as C, polynomial as P
    nodes = 0.5 * (C.chebpts1(DEG + 1) + 1.0)                        # in [0, 1]
    Dn = d_lo + (np.arange(NPIECE)[:, None] + nodes[None, :]) / invw
    zn = _inverse(Dn.ravel(), cosmo).reshape(Dn.shape)
    zc = np.zeros((NPIECE, DEG + 1))
    for p in range(NPIECE):
        ch = C.chebfit(2.0 * nodes - 1.0, zn[p], DEG)
        ps = P.Polynomial(C.cheb2poly(ch))(P.Polynomial([-1.0, 2.0]))
        zc[p, :len(ps.coef)] = ps.coef
    tab = VolumeTable([d_lo, d_hi, c0[-1], invw, first, inv_h, 0.0, 0.0], zc, rec)
    # z does not step down across a z piece's boundary
    top = np.nextafter(1.0, 0.0)
    for p in range(1, NPIECE):
        c = tab.zc[p - 1]
        z = c[DEG]
        for j in range(DEG - 1, -1, -1):
            z = z * top + c[j]
        tab.zc[p, 0] = max(tab.zc[p, 0], z)
    if validate:
        tab.validate(cosmo, dVdzf, zmin, zmax, nsample)
    return tab
