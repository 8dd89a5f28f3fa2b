"""Inputs that drive Gamma(a, x), 10^t and the band sort of lf_lumfunc_integral_quantiles over the entry's whole accepted
domain, shared by tests/test_integrals_cpu.py (which checks that the inputs are what they claim)
and tests/test_gpu_integrals.py (which runs them on the device).  NumPy and the package only.

A "free" draw (logL* = 0, logphi* = 0, alpha) has the prefactor 10^0 [* 10^0] = 1 exactly for both kinds and
logLmin - logL* = logLmin exactly, so values[r][p] = Gamma(alpha_r + 1 + kind, exp10(logLmin_p)): the function itself at
the argument lfintegrals.exp10 makes, which is gi_exp10's to the bit.  The "zevol" draws of `lattice_draws` give the same
(logL*, logphi*) = (0, 0) at z = 1 from coefficients that are not zero: 1 * 1 + (-1) * 1 + 0 and 2 * 1 + (-3) * 1 + 1, exact.

With a "zevol" draw (aphi, bphi, cphi) = (0, 1, 0), alpha + 1 + kind = 1 and logLmin = -inf the value is Gamma(1, 0) = 1 times
the prefactor, and logphi* = 0 * (z z) + 1 * z + 0 = z exactly for every finite z (0 * z^2 is +0 or -0, and adding either zero
to z != 0 returns z; z = 0 gives +0, whose 10^t is the same 1): the value is gi_exp10(z_p).  With (0, 0, t_r) it is
gi_exp10(t_r) in every column: a column of values in whatever order the draws come.
"""
import numpy as np

from lumfuncmcmc_amd import lfintegrals as li

SORT_R = (1, 2, 3, 4, 5, 7, 8, 9, 31, 32, 33, 255, 256, 257, 4095, 4096)
SORT_PATTERNS = ("ascending", "descending", "equal", "organ-pipe", "two runs", "inf first")
EXP10_EDGES = (-331.0, -330.0, -323.3, -307.7, 0.0, 308.25, 309.0)


def orders():
    """The 270 orders of the CPU lattice: -5 .. 6 in halves, 0, -1, -2, -3 each +- {0, 1e-12, 1e-9, 1e-6, 1e-3}, 200 seeded
    ones in [-5, 6], and 6.5 and 7 (alpha + 2 at the upper end of alpha's range)."""
    rng = np.random.default_rng(20240)
    a = list(np.arange(-5.0, 6.01, 0.5))
    for c in (0.0, -1.0, -2.0, -3.0):
        for d in (0.0, 1e-12, 1e-9, 1e-6, 1e-3):
            a += [c + d, c - d]
    a += list(rng.uniform(-5.0, 6.0, 200))
    a += [6.5, 7.0]
    return np.unique(np.array(a))


def arguments():
    """The arguments of the CPU lattice: 10^(-6 .. 6 in quarters), 0 and the two doubles around the switch as before; the
    smallest subnormal, 1e-320, the smallest normal double, 10^(-300 .. -10 in decades), 1e-62 and 1e-63 (where x^-5 leaves
    the doubles) and 512, 745, 1400, 1489, 1491 (results below the normal range from 745, exp(-x / 2) = 0 from 1490)."""
    x = list(10.0 ** np.arange(-6.0, 6.01, 0.25)) + [0.0, np.nextafter(li.GI_XSW, 0.0), li.GI_XSW]
    x += [5e-324, 1e-320, np.finfo(np.float64).tiny] + [float("1e-%d" % k) for k in range(10, 301, 10)]
    x += [1e-62, 1e-63, 512.0, 745.0, 1400.0, 1489.0, 1491.0]
    return np.unique(np.array(x))


def exp10_preimage(target):
    """A t with lfintegrals.exp10(t) == target, found next to log10(target)."""
    t0 = float(np.log10(target))
    for s in np.arange(1.0, 2.0, 0.03125):
        for t in (t0 * s, t0 / s):
            if li.exp10(t) == target:
                return t
    raise AssertionError("no t with exp10(t) == %r near %r" % (target, t0))


def lattice_points():
    """logLmin of the device lattice; with logL* = 0 the argument of Gamma is exp10 of each."""
    t = [-np.inf, np.inf, -331.0, -330.0, -323.5, -320.0, -308.0, -307.6]
    t += list(np.arange(-300.0, -9.0, 10.0)) + [-63.0, -62.0] + list(np.arange(-6.0, 3.26, 0.25)) + [0.0]
    t += [exp10_preimage(np.nextafter(1.0, 0.0)), exp10_preimage(np.nextafter(1.0, 2.0))]
    t += [float(np.log10(v)) for v in (512.0, 745.0, 1489.0, 1491.0)] + [6.0, 308.0, 309.0]
    return np.array(t)


def lattice_alpha(kind):
    """One alpha per lattice order with alpha + 1 + kind = a, clipped to the entry's [-6, 5]."""
    return np.clip(orders() - 1.0 - li.KINDS[kind], li.ALPHA_MIN, li.ALPHA_MAX)


def lattice_draws(variant, kind):
    """(draws, z): logL* = 0 and logphi* = 0 in every draw (at z = 1 for "zevol"; z is None for "free")."""
    al = lattice_alpha(kind)
    if variant == "free":
        return np.column_stack([np.zeros(al.size), np.zeros(al.size), al]), None
    rec = np.tile([1.0, -1.0, 0.0, 2.0, -3.0, 1.0, 0.0], (al.size, 1))
    rec[:, 6] = al
    return rec, np.ones(lattice_points().size)


def lattice_regions(x):
    """{label: mask over the arguments} of the regions DESIGN.md section 3.16 reports."""
    return {"x < 1e-6": (x > 0.0) & (x < 1e-6), "[1e-6, 1)": (x >= 1e-6) & (x < 1.0), "[1, 512)": (x >= 1.0) & (x < 512.0),
            "[512, 1490)": (x >= 512.0) & (x < 1490.0)}


def exp10_lattice():
    """t of the 10^t check: 2000 seeded values in [-7, 7], 500 in [-330, 309) and the edges."""
    return np.concatenate([np.random.default_rng(4).uniform(-7.0, 7.0, 2000), np.random.default_rng(5).uniform(-330.0, 309.0, 500),
                           EXP10_EDGES])


def exp10_case(kind, t):
    """(draw, logLmin, z, want) of a one-draw "zevol" call whose values are 10^t_p ("number") or 10^t_p 10^(t_p / 2)
    ("lumdens": logL* = 0 * (z z) + 0.5 z + 0, exact), made with lfintegrals.exp10."""
    t = np.asarray(t, dtype=np.float64)
    if kind == "number":
        draw, want = [0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0], li.exp10(t)
    else:
        with np.errstate(all="ignore"):
            draw, want = [0.0, 0.5, 0.0, 0.0, 1.0, 0.0, -1.0], li.exp10(t) * li.exp10(0.5 * t)
    return np.array([draw]), np.full(t.size, -np.inf), t, want


def sort_pattern(name, R):
    """t_r, r < R, in the named order; "ascending" is R distinct values over [-3, 3], whose powers of ten are distinct too."""
    asc = np.linspace(-3.0, 3.0, R)
    if name == "ascending":
        return asc
    if name == "descending":
        return asc[::-1].copy()
    if name == "equal":
        return np.full(R, 0.5)
    if name == "organ-pipe":
        return np.concatenate([asc[0::2], asc[1::2][::-1]])
    if name == "two runs":
        t = np.empty(R)
        h = (R + 1) // 2
        t[0::2], t[1::2] = asc[:h], asc[h:]
        return t
    if name == "inf first":
        return np.concatenate([[309.0], asc[:R - 1]])
    raise ValueError(name)


def sort_draws(t, alpha=0.0):
    """"zevol" draws with logL* = 0 and logphi* = t_r at every z."""
    rec = np.zeros((len(t), 7))
    rec[:, 5] = t
    rec[:, 6] = alpha
    return rec
