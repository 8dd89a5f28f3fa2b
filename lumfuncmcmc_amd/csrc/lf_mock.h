// lf_mock.h - mock catalogues drawn from the model on the device (lf_mock_*, include/lfmcmc.h).
//
// The density.  For a theta row and a field f, piece B of lnprob is trapz(trapz(lambda_f, logL, axis=0), zarr) on the one
// aliased grid logL[j][k] (j = luminosity, k = redshift; every column k has its own luminosity nodes), with
//     lambda_f[j][k] = phi(logL[j][k], zarr[k]; theta) * C_f[j][k]
//     FREE:             C_f = volume_part[k] * Omega_0[f] / sqarcsec * fleming(10^logL / (4 pi (Mpc DL_zarr[k])^2), 1e-17 Flim_f, alpha_C)
//     FIXCOMP, ZEVOL:   C_f = integ_part[f][j][k]
// and phi = TrueLumFunc (schechter_z for ZEVOL).  That trapezoid sum is exactly the integral of
//     f_f(z, L) = sum_{j,k} lambda_f[j][k] hat_k(z) hat_{j,k}(L)
// with hat_k the unit hat on zarr at node k and hat_{j,k} the unit hat on column k's own luminosity nodes at node j (area =
// the trapezoid weight: half the spacing to each neighbour, one-sided at the ends).  A mock is the Poisson process of
// intensity f_f: n_f ~ Poisson(M_f), M_f = sum_{j,k} m[j][k], m[j][k] = (w_z[k] w_L[j][k]) lambda_f[j][k]; each source
// picks node (j, k) with probability m / M_f and inverts the two hats with one uniform each.
//
// Node order (the cumulative sums): column k major, then j.  cdfZ[k] = column masses summed over k' <= k; cdfL[k][j] =
// masses of column k summed over j' <= j.  Both are made by mock_cdf in two steps.  The prefix sums s run in tiles of 256: a
// Hillis-Steele scan of the tile in LDS (step d = 1, 2, .. 128: x[t] = x[t - d] + x[t]) plus the running total of the
// tiles before it - one fixed order, whatever the batch.  That gives every prefix its own summation tree, so s alone may
// go down by an ulp from one node to the next and may step at a node of mass 0.  What is stored is therefore the running
// maximum over the nodes with mass,
//     c[j] = max(0, s[i] for i <= j with m[i] > 0)
// (the same tiles with max for +; max is exact and associative, so c is a function of s alone).  Guaranteed of cdfZ and of
// every column of cdfL, on the device and in the host twin (mock.scan) alike:
//     c is non-decreasing;   c[j] == c[j - 1] (0 for j = 0) wherever m[j] == 0;   c[j] is s at some node i <= j with mass,
//     so it keeps s's error bound against the exact sum, (9 + tiles before j) 2^-53 relative.
// A source with uniform u takes t = u cdfZ[S - 1], the first column with cdfZ[k] > t, then the first j with
// cdfL[k][j] > t - cdfZ[k - 1] (0 for k = 0).  On such sums bisection (mock_search) and a linear search find the same index
// for every t, and a node of zero mass is never chosen.  Not guaranteed: a node whose mass is positive but too small to
// lift its rounded sum above the maximum before it (below about one ulp of the running sum) owns no part of the range
// and cannot be drawn.  If rounding leaves no entry above t (t at the very top, or the remainder above a column's last
// sum), the first entry that reaches the last one is taken instead (>=): the last node that raised the sum.  The
// reported mean M_f is the sum scan's running total.  It and cdfZ[S - 1] are two roundings of one exact sum and may differ
// by a few units of 2^-53 (each is within (9 + tiles) 2^-53 of the exact sum, relative).
//
// Hat inversion, left width a, right width b, peak x0 (a width of zero: no mass on that side):
//     u < a / (a + b):  x = x0 - a (1 - sqrt(u (a + b) / a))       else:  x = x0 + b (1 - sqrt((1 - u) (a + b) / b))
// with each root capped at 1: next to the branch point the rounded quotient can exceed 1 by an ulp, which would put x on
// the wrong side of x0.  With the cap x stays in [x0 - a, x0 + b] (as rounded) and never decreases as u grows.
//
// Random numbers: Philox4x32-10 (lf_kernels.h), key = seed, counter = (row_id lo, row_id hi, index, MOCK_TAG | purpose << 8 |
// field).  purpose 0: the count, index = rejection round; purpose 1: source `index` of the (row, field) - words 0-1 the
// node's uniform, 2-3 the redshift hat's; purpose 2: the same source's luminosity hat (words 0-1).  The samplers use
// streams 0-2 and lf_veff 0x5eed in that word: a mock seeded like a chain is unrelated to it.  A row's catalogue depends
// on (seed, row_id, theta) only.
//
// Poisson count: mean 0 -> 0; mean < 10: inversion by sequential search (one uniform, round 0); mean >= 10: PTRS (Hormann
// 1993; NumPy's legacy random_poisson_ptrs, its random_loggam included), a fresh Philox block per rejection round.  A mean
// that is not finite, negative or above MOCK_MAX_MEAN gives count -1 (the host reports LF_ERR_ARG naming the row).
//
// Kernels (256 threads, no scratch):
//   lf_mock_mass   grid (S columns, rows x nf): one column of one (row, field): lambda, m, the column's cumulative sums
//                  (cdfL) and its total (colm).  LDS: 2 KiB (one tile, shared by the sum scan and the max scan).
//   lf_mock_total  grid (rows x nf): cumulative sums of the column totals (cdfZ), M_f, the Poisson count.  LDS: 2 KiB.
//   lf_mock_draw   one thread per source: (row, field) from the offsets by binary search, node search, two hat
//                  inversions, plain vector stores of z, logL, field.  No LDS.
//   lf_mock_hist   the same draw binned by logL: a workgroup takes up to MOCK_HIST_CHUNK sources of one (row, field),
//                  bins them into an LDS histogram and adds it to HBM with 64-bit integer atomics (order-free, so the
//                  result is deterministic).  LDS: 12 KiB (edges 8 KiB, 32-bit counters 4 KiB).
#pragma once
#include "lf_kernels.h"

namespace lf {

constexpr int MOCK_THREADS = 256;
constexpr unsigned int MOCK_TAG = 0x6d6f0000u;          // "mo": the Philox stream word of the mocks
constexpr double MOCK_MAX_MEAN = 2147483648.0;          // 2^31 expected sources per (row, field)
constexpr int MOCK_MAX_BINS = 1022;                     // nbins + 1 edges <= 1024 doubles, nbins + 2 slots <= 1024 counters
constexpr int MOCK_HIST_ITEMS = 16;                     // sources per thread of lf_mock_hist
constexpr int MOCK_HIST_CHUNK = MOCK_THREADS * MOCK_HIST_ITEMS;

struct MockConst {
    int variant, fix_sch_al, nf, S, ndim;
    double sch_al0;
    double om0s[MAXF];        // FREE: Omega_0[f] / sqarcsec (float areas, lumfuncmcmc.py:375)
    double fc_ratio;          // FREE: |a / (1 - a)|, a = (2 fcmin - 1)^2
    double pivots[3];         // ZEVOL
    const double* logL;       // [S][S]
    const double* zarr;       // [S]
    const double* volume_part;// [S]   FREE
    const double* dl_zarr;    // [S]   FREE
    const double* integ_part; // [nf][S][S]  FIXCOMP, ZEVOL
};

// hat inversion, see the file comment (no contraction: the host twin makes the same roundings)
__device__ __forceinline__ double mock_hat(double x0, double a, double b, double u) {
#pragma clang fp contract(off)
    const double ab = a + b;
    if (u < a / ab) {
        const double s = fmin(sqrt(u * ab / a), 1.0);
        return x0 - a * (1.0 - s);
    }
    const double s = fmin(sqrt((1.0 - u) * ab / b), 1.0);
    return x0 + b * (1.0 - s);
}

// first index i in [0, n) with v[i] > t; if there is none, the first with v[i] >= v[n - 1]
__device__ __forceinline__ int mock_search(const double* __restrict__ v, int n, double t) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (v[mid] > t) hi = mid; else lo = mid + 1;
    }
    if (lo < n) return lo;
    const double top = v[n - 1];
    lo = 0; hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (v[mid] >= top) hi = mid; else lo = mid + 1;
    }
    return lo;
}

__device__ __forceinline__ void mock_philox(unsigned long long row_id, unsigned int index, unsigned int purpose, int f,
                                            unsigned long long seed, unsigned int (&r)[4]) {
    philox4x32((unsigned int)row_id, (unsigned int)(row_id >> 32), index, MOCK_TAG | (purpose << 8) | (unsigned int)f,
               (unsigned int)seed, (unsigned int)(seed >> 32), r);
}

// NumPy's random_loggam (Stirling series), operation for operation
__device__ __forceinline__ double mock_loggam(double x) {
#pragma clang fp contract(off)
    const double a[10] = {8.333333333333333e-02, -2.777777777777778e-03, 7.936507936507937e-04, -5.952380952380952e-04,
                          8.417508417508418e-04, -1.917526917526918e-03, 6.410256410256410e-03, -2.955065359477124e-02,
                          1.796443723688307e-01, -1.39243221690590e+00};
    if (x == 1.0 || x == 2.0) return 0.0;
    long long n = 0;
    if (x < 7.0) n = (long long)(7 - x);
    double x0 = x + (double)n;
    const double x2 = (1.0 / x0) * (1.0 / x0);
    const double lg2pi = 1.8378770664093453e+00;
    double gl0 = a[9];
    for (int k = 8; k >= 0; --k) {
        gl0 *= x2;
        gl0 += a[k];
    }
    double gl = gl0 / x0 + 0.5 * lg2pi + (x0 - 0.5) * log(x0) - x0;
    if (x < 7.0)
        for (long long k = 1; k <= n; ++k) {
            gl -= log(x0 - 1.0);
            x0 -= 1.0;
        }
    return gl;
}

// the exact Poisson draw of the file comment; -1 for a mean the caller must refuse.  Forced inline, as mock_loggam: it has two
// callers (lf_mock_total; lf_mock_count_cut of lf_mock_cut.h), and each keeps the instructions it had as the only one
__device__ __forceinline__ long long mock_poisson(double mu, unsigned long long row_id, int f, unsigned long long seed) {
#pragma clang fp contract(off)
    if (!(mu >= 0.0) || !(mu <= MOCK_MAX_MEAN)) return -1;      // (NaN fails both)
    if (mu == 0.0) return 0;
    unsigned int r[4];
    if (mu < 10.0) {
        mock_philox(row_id, 0u, 0u, f, seed, r);
        const double u = u53(r[0], r[1]);
        double p = exp(-mu), F = p;
        long long k = 0;
        while (u > F) {
            ++k;
            p *= mu / (double)k;
            if (p == 0.0) break;               // the tail is exhausted: F stays below u only by rounding
            F += p;
        }
        return k;
    }
    const double slam = sqrt(mu), loglam = log(mu);
    const double b = 0.931 + 2.53 * slam;
    const double a = -0.059 + 0.02483 * b;
    const double invalpha = 1.1239 + 1.1328 / (b - 3.4);
    const double vr = 0.9277 - 3.6224 / (b - 2.0);
    for (unsigned int round = 0;; ++round) {
        mock_philox(row_id, round, 0u, f, seed, r);
        const double U = u53(r[0], r[1]) - 0.5;
        const double V = u53(r[2], r[3]);
        const double us = 0.5 - fabs(U);
        const long long k = (long long)floor((2.0 * a / us + b) * U + mu + 0.43);
        if (us >= 0.07 && V <= vr) return k;
        if (k < 0 || (us < 0.013 && V > us)) continue;
        if ((log(V) + log(invalpha) - log(a / (us * us) + b)) <= (-mu + (double)k * loglam - mock_loggam((double)(k + 1))))
            return k;
    }
}

// what lambda_f needs of one (row, field, column k): the same for every node of the column
struct MockColumn {
    double lstar, phi0, ap1;      // L*, LN10 10^phi*, alpha + 1 (at zarr[k] for ZEVOL)
    double flim, alpha, ftau;     // FREE: 1e-17 Flim_f, alpha_C, f_tau
    double d2, vp, om0s;          // FREE: 4 pi (Mpc DL_zarr[k])^2, volume_part[k], Omega_0[f] / sqarcsec
};

__device__ inline MockColumn mock_column(const MockConst& mc, const double* __restrict__ th, int f, int k) {
#pragma clang fp contract(off)
    MockColumn c{};
    double lphi, al;
    if (mc.variant == LF_ZEVOL) {
        al = mc.fix_sch_al ? mc.sch_al0 : th[6];
        double aL, bL, cL, aP, bP, cP;
        quad_coef(th[3], th[4], th[5], mc.pivots[0], mc.pivots[1], mc.pivots[2], aP, bP, cP);
        quad_coef(th[0], th[1], th[2], mc.pivots[0], mc.pivots[1], mc.pivots[2], aL, bL, cL);
        const double z = mc.zarr[k];
        lphi = quad_nofma(aP, bP, cP, z, z * z);
        c.lstar = quad_nofma(aL, bL, cL, z, z * z);
    } else {
        c.lstar = th[0];
        lphi = th[1];
        al = mc.fix_sch_al ? mc.sch_al0 : th[2];
    }
    c.phi0 = 2.302585092994045684 * exp10(lphi);
    c.ap1 = al + 1.0;
    if (mc.variant == LF_FREE) {
        const int k0 = mc.fix_sch_al ? 2 : 3;
        c.flim = 1.0e-17 * th[k0 + f];
        c.alpha = th[k0 + mc.nf];
        c.ftau = c.flim * exp10(-sqrt(mc.fc_ratio * (1.0 / (c.alpha * c.alpha))));      // VmaxLumFunc.py:164-167
        const double dl = 3.086e24 * mc.dl_zarr[k];
        c.d2 = 4.0 * 3.141592653589793 * (dl * dl);
        c.vp = mc.volume_part[k];
        c.om0s = mc.om0s[f];
    }
    return c;
}

// lambda_f at node (j, k): TrueLumFunc (lumfuncmcmc.py:44) times C_f
__device__ inline double mock_lambda(const MockConst& mc, const MockColumn& c, int f, int j, int k) {
#pragma clang fp contract(off)
    const int S = mc.S;
    const double L = mc.logL[(size_t)j * S + k];
    const double t = L - c.lstar;
    const double tlf = c.phi0 * exp10(t * c.ap1) * exp(-exp10(t));
    double w;
    if (mc.variant == LF_FREE) {
        const double flux = exp10(L) / c.d2;
        const double num = c.alpha * log10(flux / c.flim);                              // VmaxLumFunc.py:118-127, :141
        const double fc = 0.5 * (1.0 + num / sqrt(1.0 + num * num));
        const double om = c.om0s * pow(fc, 1.0 / (1.0 - exp(-flux / c.ftau)));
        w = c.vp * om;
    } else {
        w = mc.integ_part[((size_t)f * S + j) * S + k];
    }
    return tlf * w;
}

// inclusive scan of one tile of 256 values in LDS (Hillis-Steele), then + carry; returns this thread's prefix and leaves
// the tile's total (carry included) in `carry` for every thread
__device__ __forceinline__ double mock_scan_tile(double* __restrict__ buf, double v, double& carry) {
    const int t = threadIdx.x;
    buf[t] = v;
    __syncthreads();
#pragma unroll
    for (int d = 1; d < MOCK_THREADS; d <<= 1) {
        const double o = t >= d ? buf[t - d] : 0.0;
        __syncthreads();
        if (t >= d) buf[t] = o + buf[t];
        __syncthreads();
    }
    const double out = carry + buf[t];
    const double tot = carry + buf[MOCK_THREADS - 1];
    __syncthreads();
    carry = tot;
    return out;
}

// running maximum of one tile of 256 values >= 0 in LDS (the same tree with max for +), continued from `top`; returns this
// thread's maximum and leaves the tile's (top included) in `top` for every thread.  Max is exact: the order is immaterial.
__device__ __forceinline__ double mock_max_tile(double* __restrict__ buf, double v, double& top) {
    const int t = threadIdx.x;
    buf[t] = v;
    __syncthreads();
#pragma unroll
    for (int d = 1; d < MOCK_THREADS; d <<= 1) {
        const double o = t >= d ? buf[t - d] : 0.0;
        __syncthreads();
        if (t >= d) buf[t] = fmax(o, buf[t]);
        __syncthreads();
    }
    const double out = fmax(top, buf[t]);
    const double tot = fmax(top, buf[MOCK_THREADS - 1]);
    __syncthreads();
    top = tot;
    return out;
}

// The cumulative sums of the file comment for n masses mass(0) .. mass(n - 1) >= 0, one workgroup of 256, tile by tile:
// out[j] = the largest prefix sum at a node i <= j with mass(i) > 0 (0 if there is none); returns the sum scan's running
// total (all threads).  buf: the 2 KiB tile, used by both scans in turn.  lf_mock_mass, lf_mock_total and the tests' probe
// (tests/mock_probe.hip) all run this one loop.
template <class Mass>
__device__ __forceinline__ double mock_cdf(double* __restrict__ buf, int n, Mass mass, double* __restrict__ out) {
    double carry = 0.0, top = 0.0;
    for (int base = 0; base < n; base += MOCK_THREADS) {
        const int j = base + (int)threadIdx.x;
        const double m = j < n ? mass(j) : 0.0;
        const double s = mock_scan_tile(buf, m, carry);
        const double c = mock_max_tile(buf, m > 0.0 ? s : 0.0, top);
        if (j < n) out[j] = c;
    }
    return carry;
}

// trapezoid weight of node i of n nodes x[i * stride]: half the spacing to each neighbour
__device__ __forceinline__ double mock_weight(const double* __restrict__ x, int stride, int i, int n) {
#pragma clang fp contract(off)
    const double dl = i > 0 ? x[(size_t)i * stride] - x[(size_t)(i - 1) * stride] : 0.0;
    const double dr = i < n - 1 ? x[(size_t)(i + 1) * stride] - x[(size_t)i * stride] : 0.0;
    return 0.5 * (dl + dr);
}

// blockIdx.x = column k, blockIdx.y = rf = row * nf + f.  cdfL: [rows * nf][S][S] (column-major per rf), colm: [rows * nf][S]
__global__ __launch_bounds__(MOCK_THREADS) void lf_mock_mass(MockConst mc, const double* __restrict__ theta,
                                                             double* __restrict__ cdfL, double* __restrict__ colm) {
#pragma clang fp contract(off)
    __shared__ double buf[MOCK_THREADS];
    const int k = blockIdx.x, rf = blockIdx.y, S = mc.S;
    const int row = rf / mc.nf, f = rf - row * mc.nf;
    const double* th = theta + (size_t)row * mc.ndim;
    const double wz = mock_weight(mc.zarr, 1, k, S);
    const MockColumn col = mock_column(mc, th, f, k);
    double* out = cdfL + ((size_t)rf * S + k) * S;
    const double total = mock_cdf(buf, S, [&](int j) {
#pragma clang fp contract(off)
        const double wl = mock_weight(mc.logL + k, S, j, S);
        return (wz * wl) * mock_lambda(mc, col, f, j, k);
    }, out);
    if (threadIdx.x == 0) colm[(size_t)rf * S + k] = total;
}

// blockIdx.x = rf.  cdfZ: [rows * nf][S]; mean, count: [rows * nf]
__global__ __launch_bounds__(MOCK_THREADS) void lf_mock_total(int S, int nf, const double* __restrict__ colm,
                                                              const long long* __restrict__ row_ids, unsigned long long seed,
                                                              double* __restrict__ cdfZ, double* __restrict__ mean,
                                                              long long* __restrict__ count) {
    __shared__ double buf[MOCK_THREADS];
    const int rf = blockIdx.x;
    const double* cm = colm + (size_t)rf * S;
    const double total = mock_cdf(buf, S, [&](int k) { return cm[k]; }, cdfZ + (size_t)rf * S);
    if (threadIdx.x == 0) {
        const int row = rf / nf, f = rf - row * nf;
        mean[rf] = total;
        count[rf] = mock_poisson(total, (unsigned long long)row_ids[row], f, seed);
    }
}

// source i of (row, field) rf: its redshift and log luminosity
__device__ __forceinline__ void mock_source(const MockConst& mc, int rf, int f, unsigned long long row_id, unsigned int i,
                                            unsigned long long seed, const double* __restrict__ cdfL,
                                            const double* __restrict__ cdfZ, double& z, double& L) {
#pragma clang fp contract(off)
    const int S = mc.S;
    unsigned int r[4], q[4];
    mock_philox(row_id, i, 1u, f, seed, r);
    mock_philox(row_id, i, 2u, f, seed, q);
    const double* cz = cdfZ + (size_t)rf * S;
    const double t = u53(r[0], r[1]) * cz[S - 1];
    const int k = mock_search(cz, S, t);
    const double tl = t - (k > 0 ? cz[k - 1] : 0.0);
    const int j = mock_search(cdfL + ((size_t)rf * S + k) * S, S, tl);
    const double* zr = mc.zarr;
    z = mock_hat(zr[k], k > 0 ? zr[k] - zr[k - 1] : 0.0, k < S - 1 ? zr[k + 1] - zr[k] : 0.0, u53(r[2], r[3]));
    const double* lc = mc.logL + k;
    const double x0 = lc[(size_t)j * S];
    L = mock_hat(x0, j > 0 ? x0 - lc[(size_t)(j - 1) * S] : 0.0, j < S - 1 ? lc[(size_t)(j + 1) * S] - x0 : 0.0, u53(q[0], q[1]));
}

// the same source (the same statements and streams), and the column k of the node it picked (lf_mock_cut.h)
__device__ __forceinline__ void mock_source(const MockConst& mc, int rf, int f, unsigned long long row_id, unsigned int i,
                                            unsigned long long seed, const double* __restrict__ cdfL,
                                            const double* __restrict__ cdfZ, double& z, double& L, int& k) {
#pragma clang fp contract(off)
    const int S = mc.S;
    unsigned int r[4], q[4];
    mock_philox(row_id, i, 1u, f, seed, r);
    mock_philox(row_id, i, 2u, f, seed, q);
    const double* cz = cdfZ + (size_t)rf * S;
    const double t = u53(r[0], r[1]) * cz[S - 1];
    k = mock_search(cz, S, t);
    const double tl = t - (k > 0 ? cz[k - 1] : 0.0);
    const int j = mock_search(cdfL + ((size_t)rf * S + k) * S, S, tl);
    const double* zr = mc.zarr;
    z = mock_hat(zr[k], k > 0 ? zr[k] - zr[k - 1] : 0.0, k < S - 1 ? zr[k + 1] - zr[k] : 0.0, u53(r[2], r[3]));
    const double* lc = mc.logL + k;
    const double x0 = lc[(size_t)j * S];
    L = mock_hat(x0, j > 0 ? x0 - lc[(size_t)(j - 1) * S] : 0.0, j < S - 1 ? lc[(size_t)(j + 1) * S] - x0 : 0.0, u53(q[0], q[1]));
}

// offsets [nrf + 1]: sources of rf are [off[rf], off[rf + 1]); rf = first index with off[rf + 1] > g
__device__ __forceinline__ int mock_owner(const long long* __restrict__ off, int nrf, long long g) {
    int lo = 0, hi = nrf - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (off[mid + 1] > g) hi = mid; else lo = mid + 1;
    }
    return lo;
}

__global__ __launch_bounds__(MOCK_THREADS) void lf_mock_draw(MockConst mc, int nrf, const long long* __restrict__ off,
                                                             const long long* __restrict__ row_ids, unsigned long long seed,
                                                             const double* __restrict__ cdfL, const double* __restrict__ cdfZ,
                                                             double* __restrict__ z, double* __restrict__ logL,
                                                             int* __restrict__ field) {
    const long long g = (long long)blockIdx.x * MOCK_THREADS + threadIdx.x;
    if (g >= off[nrf]) return;
    const int rf = mock_owner(off, nrf, g);
    const int row = rf / mc.nf, f = rf - row * mc.nf;
    double zz, LL;
    mock_source(mc, rf, f, (unsigned long long)row_ids[row], (unsigned int)(g - off[rf]), seed, cdfL, cdfZ, zz, LL);
    z[g] = zz;
    logL[g] = LL;
    field[g] = f;
}

// blk: [nrf + 1] workgroup offsets (rf owns workgroups blk[rf] .. blk[rf + 1] - 1, MOCK_HIST_CHUNK sources each);
// hist: [nrf][nbins + 2], slot = searchsorted(edges, logL, side="right")
__global__ __launch_bounds__(MOCK_THREADS) void lf_mock_hist(MockConst mc, int nrf, const long long* __restrict__ blk,
                                                             const long long* __restrict__ count,
                                                             const long long* __restrict__ row_ids, unsigned long long seed,
                                                             const double* __restrict__ cdfL, const double* __restrict__ cdfZ,
                                                             int nbins, const double* __restrict__ edges,
                                                             unsigned long long* __restrict__ hist) {
    __shared__ double le[MOCK_MAX_BINS + 2];
    __shared__ unsigned int lh[MOCK_MAX_BINS + 2];
    const int ne = nbins + 1, ns = nbins + 2;
    for (int i = threadIdx.x; i < ne; i += MOCK_THREADS) le[i] = edges[i];
    for (int i = threadIdx.x; i < ns; i += MOCK_THREADS) lh[i] = 0u;
    __syncthreads();
    const long long b = blockIdx.x;
    const int rf = mock_owner(blk, nrf, b);
    const int row = rf / mc.nf, f = rf - row * mc.nf;
    const unsigned long long rid = (unsigned long long)row_ids[row];
    const long long first = (b - blk[rf]) * MOCK_HIST_CHUNK, n = count[rf];
    for (int s = 0; s < MOCK_HIST_ITEMS; ++s) {
        const long long i = first + (long long)s * MOCK_THREADS + threadIdx.x;
        if (i >= n) break;
        double zz, LL;
        mock_source(mc, rf, f, rid, (unsigned int)i, seed, cdfL, cdfZ, zz, LL);
        int lo = 0, hi = ne;                        // number of edges <= LL
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (le[mid] <= LL) lo = mid + 1; else hi = mid;
        }
        atomicAdd(&lh[lo], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < ns; i += MOCK_THREADS)
        if (lh[i]) atomicAdd(&hist[(size_t)rf * ns + i], (unsigned long long)lh[i]);
}

}  // namespace lf
