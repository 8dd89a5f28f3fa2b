"""Shared inputs and yardsticks of the chain-diagnostics tests (test_diag_cpu.py, test_gpu_diag.py): seeded AR(1) chains, the
FFT form of the ACF exactly as sampler.integrated_time computes it, and literal NumPy statements of split-R-hat and ESS.
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
