"""Shared inputs and yardsticks of the chain-diagnostics tests (test_diag_cpu.py, test_gpu_diag.py): seeded AR(1) chains, the
FFT form of the ACF exactly as sampler.integrated_time computes it, and literal NumPy statements of split-R-hat and ESS;
integer series on which the device's sums are exact, with exact_acf, the curve it must then give bit for bit; and truth_acf,
the direct sums of a real series in extended precision, with the bound a correct kernel stays inside.
Test infrastructure only."""
import numpy as np

# (n, W, rho, offset); the seed of a case is its position in this list
CASES = [(2000, 32, 0.9, 43.0), (5000, 64, 0.97, -3.0), (300, 16, 0.5, 0.0), (20000, 32, 0.99, 2.5)]


def ar1(seed):
    """(W, n) series x_t = rho x_{t-1} + sqrt(1 - rho^2) e_t, scaled by 0.01 and offset to parameter-like values."""
    from scipy.signal import lfilter
    n, W, rho, offset = CASES[seed]
    rs = np.random.RandomState(seed)
    e = rs.standard_normal((W, n))
    e[:, 1:] *= np.sqrt(1.0 - rho * rho)
    x = lfilter([1.0], [1.0, -rho], e, axis=1)
    return 0.01 * x + offset


def shifted(x):
    """The same series with 3 standard deviations added to the second half: not stationary."""
    y = x.copy()
    y[:, x.shape[1] // 2:] += 3.0 * x.std()
    return y


def fft_acf(x):
    """integrated_time's own lines on a (W, n) series: the normalised ACF averaged over the walkers (n lags)."""
    x = np.asarray(x, dtype=np.float64).T
    n = x.shape[0]
    acf = np.zeros(n)
    size = 1 << int(np.ceil(np.log2(2 * n)))
    for k in range(x.shape[1]):
        y = x[:, k] - x[:, k].mean()
        f = np.fft.rfft(y, n=size)
        a = np.fft.irfft(f * np.conjugate(f))[:n]
        if a[0] > 0:
            acf += a / a[0]
    acf /= max(x.shape[1], 1)
    return acf


def fft_window(acf, c=5.0):
    """integrated_time's window lines on that curve: (tau before the finite / positive convention, window, margin), margin =
    min over m <= window of |m - c taus[m]|: how far the window is from hanging on a rounding error."""
    n = len(acf)
    taus = 2.0 * np.cumsum(acf) - 1.0
    m = np.arange(n) < c * taus
    win = int(np.argmin(m)) if not m.all() else n - 1
    margin = float(np.min(np.abs(np.arange(win + 1) - c * taus[:win + 1])))
    return float(taus[win]), win, margin


def rhat_numpy(x):
    """Split-R-hat of a (W, n) series, literally (Gelman et al. 2013)."""
    W, n = x.shape
    h = n // 2
    halves = np.concatenate([x[:, :h], x[:, n - h:]], axis=0)
    means, variances = halves.mean(axis=1), halves.var(axis=1, ddof=1)
    Wv, Bh = variances.mean(), means.var(ddof=1)
    return float(np.sqrt(((h - 1.0) / h * Wv + Bh) / Wv))


# ---------------------------------------------------------------------------------------------------- exact inputs
# Integer series for which every step of the device's diagnostics is exact in double, in any order and with or without
# FMA: the sums of the range and of both halves are divisible by their lengths, so every two-pass mean is an integer, the
# centred values are integers and every lag sum and sum of squared deviations stays far below 2^53.  What is left to round
# is a_w[k] / a_w[0], the walker sum in walker order and the division by W (and R-hat's host arithmetic on exact moments).

EXACT_N = [4, 5, 7, 8, 9, 63, 64, 65, 255, 256, 257, 300, 511, 512, 513, 767, 768, 769, 1023, 1024, 1025, 1100]
# The later-pass cases, W = 4, c = 50: n -> lags computed when the window is decided.  The windows are 550, 642, 1009 and
# 1101 (asserted in test_diag_cpu.py): the first three are decided by the second pass (512 new lags, 1024 in all - 1009 lies
# below 1024, so n = 1100 needs no third pass), the last by a third pass that Mmax = 1536 cuts short of 2048.
DRIFT_LAGS = {600: 1024, 700: 1024, 1100: 1024, 1200: 1536}
DRIFT_N = sorted(DRIFT_LAGS)
SLICE_SHAPE = (1025, 8, 520, 1024)             # W, D, n, nlags: two slices of one pass
SLICE_BYTES = 64 << 20                         # the per-slice budget of diag_run


def _fix_sums(x):
    """Adjust a few elements of every (W, n) integer walker so that sum(x[:h]) and sum(x[n-h:]) are divisible by h = n // 2
    and sum(x) by n: the last element of each half, then the middle one (n odd) or the last one by h (n even)."""
    x = np.array(x, dtype=np.int64)
    W, n = x.shape
    h = n // 2
    if h >= 1:
        x[:, h - 1] -= x[:, :h].sum(axis=1) % h
        x[:, n - 1] -= x[:, n - h:].sum(axis=1) % h
    if n % 2:
        x[:, h] -= x.sum(axis=1) % n
    elif h >= 1:
        x[:, n - 1] += np.where(x.sum(axis=1) % n != 0, h, 0)
    assert np.all(x.sum(axis=1) % n == 0)
    if h >= 1:
        assert np.all(x[:, :h].sum(axis=1) % h == 0) and np.all(x[:, n - h:].sum(axis=1) % h == 0)
    return x


def lattice(seed, W, n, offset=40000):
    """(W, n) int64, seeded and correlated: x[t] = (7 x[t-1]) // 8 + e[t], |e| <= 1000 (so |x| <= 8000), sums fixed as in
    _fix_sums, an integer offset added."""
    rs = np.random.RandomState(1000 + seed)
    e = rs.randint(-1000, 1001, size=(W, n)).astype(np.int64)
    x = np.empty((W, n), dtype=np.int64)
    x[:, 0] = e[:, 0]
    for t in range(1, n):
        x[:, t] = (7 * x[:, t - 1]) // 8 + e[:, t]
    return _fix_sums(x) + offset


def drift(seed, W, n):
    """(W, n) int64: 8 t + noise in [-3, 3], sums fixed as in _fix_sums.  Its window under c = 50 lies deep in the chain."""
    rs = np.random.RandomState(2000 + seed)
    return _fix_sums(8 * np.arange(n, dtype=np.int64)[None, :] + rs.randint(-3, 4, size=(W, n)))


def exact_lag_sums(x_int, nlags):
    """a_w[k] = sum_{t < n-k} y[t] y[t+k], y = x - mean(x), in int64 for k < nlags (0 for k >= n).  (W, nlags) int64."""
    x = np.asarray(x_int)
    assert x.dtype == np.int64 and x.ndim == 2
    W, n = x.shape
    s = x.sum(axis=1)
    assert np.all(s % n == 0), "the walker sums must be divisible by n"
    y = x - (s // n)[:, None]
    assert n * int(np.max(np.abs(y))) ** 2 < 2 ** 53
    a = np.zeros((W, nlags), dtype=np.int64)
    for k in range(min(n, nlags)):
        a[:, k] = (y[:, :n - k] * y[:, k:]).sum(axis=1)
    return a


def exact_ratios(x_int, nlags):
    """(live, ratio): live[w] = a_w[0] > 0, ratio[w][k] = a_w[k] / a_w[0] correctly rounded (exact integers divided in
    float64); rows of walkers that are not live hold 0.0."""
    a = exact_lag_sums(x_int, nlags)
    live = a[:, 0] > 0
    ratio = np.zeros(a.shape)
    ratio[live] = a[live].astype(np.float64) / a[live, :1].astype(np.float64)
    return live, ratio


def walker_average(rows, W):
    """The kernel's stated order on ratio curves: added one by one in walker order from 0.0, then divided by W."""
    acf = None
    for r in rows:
        acf = np.zeros(len(r)) if acf is None else acf
        acf = acf + r
    return acf / float(W)


def exact_acf(x_int, nlags):
    """The ACF of an integer (W, n) series whose walker sums are divisible by n, as the device must give it bit for bit:
    a_w[k] in int64, then a_w[k] / a_w[0], the walker sum in walker order and the division by W in float64.  Walkers with
    a_w[0] <= 0 are left out (and still counted in W).  Lags at and past n are 0.0."""
    live, ratio = exact_ratios(x_int, nlags)
    if not live.any():
        return np.zeros(nlags)
    return walker_average((ratio[w] for w in range(len(live)) if live[w]), len(live))


def lags_past(n):
    """The next multiple of 512 above n, plus 512: whole lag tiles past the end of the series."""
    return (n // 512 + 1) * 512 + 512


def passes(window, n):
    """Lags diag_run has computed when a window is first decided, nlags = 0: 512, then doubled, capped at Mmax."""
    mmax = -(-n // 512) * 512
    have = 512
    while window >= have and have < mmax:
        have = min(2 * have, mmax)
    return have


def slices(W, D, want):
    """(slice length in lags, number of slices) of a pass of `want` lags in diag_run."""
    sl = max(SLICE_BYTES // (W * D * 8) // 512, 1) * 512
    return sl, -(-want // sl)


GROUP_D = [1, 2, 3, 4, 5, 7, 8, 9]             # series counts around the groups of 4 of lf_diag_acf
GROUP_N, GROUP_W = 257, 2
CONSTANTS = [0.1, 43.7, -3.3, 1e-3]            # not representable: a constant series must still centre to exactly 0
CONSTANT_N = [4, 7, 300, 1025]


def group_series(D):
    """(D, W, n) int64: D different lattice series of GROUP_W walkers and GROUP_N steps, with different offsets."""
    return np.stack([lattice(100 + d, GROUP_W, GROUP_N, offset=40000 + 1000 * d) for d in range(D)])


def slice_patterns():
    """(5, n) int64 for SLICE_SHAPE: four lattice walkers and a constant one."""
    n = SLICE_SHAPE[2]
    return np.concatenate([lattice(200, 4, n), np.full((1, n), 40000, dtype=np.int64)])


def slice_pattern_of(w, d):
    return (w + 2 * d) % 5


def slice_expected(patterns, d, W, nlags):
    """The exact ACF of series d of the chain whose walker w is patterns[slice_pattern_of(w, d)]: five ratio curves, added
    in walker order."""
    live, ratio = exact_ratios(patterns, nlags)
    idx = [slice_pattern_of(w, d) for w in range(W)]
    return walker_average((ratio[i] for i in idx if live[i]), W)


# ------------------------------------------------------------------------------------------- a high-precision truth
def _extended():
    """np.longdouble when it is the 80-bit format or better (eps <= 1.1e-19), else None."""
    return np.longdouble if np.finfo(np.longdouble).eps <= 1.1e-19 else None


def _truth_ratios(x, nlags, shift_ulps=0):
    """ratio[w][k] = a_w[k] / a_w[0] by direct sums in extended precision, every walker's mean moved by shift_ulps ulp (of
    the mean as a double).  (W, nlags) in the extended type (np.longdouble, or mpmath at 40 digits as an object array)."""
    x = np.asarray(x, dtype=np.float64)
    W, n = x.shape
    L = min(n, nlags)
    ld = _extended()
    if ld is not None:
        xl = x.astype(ld)
        mean = xl.sum(axis=1) / ld(n)
        mean = mean + ld(shift_ulps) * np.spacing(np.abs(mean.astype(np.float64))).astype(ld)
        y = xl - mean[:, None]
        a = np.zeros((W, nlags), dtype=ld)
        for k in range(L):
            a[:, k] = (y[:, :n - k] * y[:, k:]).sum(axis=1)
        return a / a[:, :1]
    import mpmath
    mp = mpmath.mp.clone()
    mp.dps = 40
    out = np.empty((W, nlags), dtype=object)
    for w in range(W):
        xs = [mp.mpf(float(v)) for v in x[w]]
        mean = mp.fsum(xs) / n
        mean = mean + shift_ulps * mp.mpf(float(np.spacing(abs(float(mean)))))
        y = [v - mean for v in xs]
        a0 = mp.fdot(y, y)
        for k in range(nlags):
            out[w, k] = mp.fdot(y[:n - k], y[k:]) / a0 if k < L else mp.mpf(0)
    return out


def truth_acf(x, nlags):
    """The ACF of a real (W, n) series by direct sums in extended precision (np.longdouble with eps <= 1.1e-19, else mpmath
    at 40 digits), and S: the largest change of that curve over the lags when every walker's mean is moved by +1 or -1 ulp
    of that mean (each walker taken at the sign that moves its term more: no choice of signs moves the curve further).
    Returns (acf as float64, S).  All walkers must have a_w[0] > 0."""
    W = np.shape(x)[0]
    r0, rp, rm = (_truth_ratios(x, nlags, s) for s in (0, 1, -1))
    acf = r0.sum(axis=0) / W
    moved = np.maximum(np.abs(rp - r0), np.abs(rm - r0)).sum(axis=0) / W
    return np.array([float(v) for v in acf]), float(np.max(moved))


def truth_bound(n, S):
    """2 ((n + 16) 2^-53 + S): an n-term sum relative to a[0] at its worst, 16 more roundings for the means and centring,
    the conditioning S a correctly rounded mean cannot avoid, doubled for the division and the walker average."""
    return 2.0 * ((n + 16) * 2.0 ** -53 + S)


def real_cases():
    """name -> (W, n) real series of the comparisons with truth_acf."""
    base = ar1(0)[:8, :1100]
    wide = (base - 43.0) / 0.01 * 100.0 + 1e6
    return {"ar1(2)": ar1(2), "ar1(0)[:8,:1100]": base, "offset 1e6 spread 100": wide, "n 1025": ar1(1)[:8, 200:1225]}
