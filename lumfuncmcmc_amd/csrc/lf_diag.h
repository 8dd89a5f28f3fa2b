// lf_diag.h - chain diagnostics where the chain is: the autocorrelation function of every
// parameter's series by DIRECT sums, and the per-walker moments split-R-hat needs.  Replaces the read-back behind
//     tau = np.max(sampler.acor); burnin = min(int(3 tau), nsteps // 2)          lumfuncmcmc.py:499-501
// (W x steps x ndim doubles to the host, one FFT pair per (walker, parameter)).
//
// A series is x[t] = chain[w][t0 + t][d], t < n (the samplers' layout [W][cap][ndim]; series d == ndim is the lnprob
// chain [W][cap] when given).  Defined as sampler.integrated_time defines them:
//     y = x - mean(x),  a[k] = sum_{t < n-k} y[t] y[t+k],  acf[d][k] = (1 / W) sum_w a_w[k] / a_w[0]   (walkers with a_w[0] <= 0 left out).
//
// lf_diag_moments  one workgroup per (walker, series): the mean over [0, n) and, for the halves [0, h) and [n-h, n), h = n / 2,
//                  mean and sum of squared deviations.  Every mean is m0 = sum(x) / len, then m0 + sum(x - m0) / len.
// lf_diag_acf      one workgroup of 256 threads per (tile of 512 lags, walker, group of up to 4 series).  It walks the range in
//                  tiles of 256 steps; a tile's centred values go to LDS for the group's series at once (the steps of one
//                  walker are ndim doubles apart): the tile itself (read by broadcast) and the 768 values the 512 lags reach
//                  from it.  Lane l of every wave owns the 8 lags K0 + 8 l .. + 7, wave q the 64 steps q 64 .. + 63 of the tile:
//                  per 8 steps a thread reads 8 + 8 doubles of LDS, 16 bytes at a time, for 64 FMAs.  A thread's lagged reads
//                  start 8 doubles apart, so the lagged row stores position p at p + 2 (p / 8): lanes 10 doubles apart, which
//                  keeps 16-byte alignment and puts the 16 lanes of every group of a 16-byte read on different banks (20 l mod 64
//                  = 4 (5 l mod 16)).  Positions at or past n hold 0.0, which is the t < n - k of the definition.
//                  Order of the sums, fixed and independent of how many lags or series a call asks for: a (wave, tile) sum
//                  over its 64 steps in step order by FMA, added to the wave's running total tile by tile, the four waves'
//                  totals added as ((q0 + q1) + q2) + q3.  No atomics.  Hence acf[d][k] has the same bits for any M and any
//                  batch.
// lf_diag_norm     acf[d][k] = (sum over w in order of a_w[k] / a_w[0]) / W.
//
// Host part (namespace lfd, plain C++): integrated_time's window rule on an ACF curve, and split-R-hat from the moments.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

namespace lf {

constexpr int DIAG_THREADS = 256;
constexpr int DIAG_TB = 256;                  // steps per tile
constexpr int DIAG_RL = 8;                    // lags per thread
constexpr int DIAG_LT = 64 * DIAG_RL;         // lags per workgroup
constexpr int DIAG_DG = 4;                    // series per workgroup
constexpr int DIAG_BASEROW = DIAG_TB + 8;     // rows 8 doubles off a multiple of 32: the group's rows start on different banks
constexpr int DIAG_LAGROW = 968;              // >= idx(TB + LT - 1) + 1 = 958, and 8 off a multiple of 32
constexpr int DIAG_LDS_BYTES = (DIAG_DG * (DIAG_BASEROW + DIAG_LAGROW) + DIAG_DG) * 8;       // 39 456

struct DiagSeries {
    const double* chain;      // [W][cap][ndim]
    const double* lnp;        // [W][cap] or NULL
    long long cap;
    int ndim, D;              // D = ndim + (lnp != NULL)
    long long t0;
    int n;
};

__device__ __forceinline__ double diag_x(const DiagSeries& s, int w, int d, long long t) {
    const long long row = (long long)w * s.cap + s.t0 + t;
    return d < s.ndim ? s.chain[row * s.ndim + d] : s.lnp[row];
}

// sum over the workgroup in a fixed tree; every thread gets it
__device__ __forceinline__ double diag_block_sum(double v, double* sh) {
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int s = DIAG_THREADS / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
        __syncthreads();
    }
    const double r = sh[0];
    __syncthreads();
    return r;
}

// the two-pass mean of x[lo .. hi) and, with ssd, the sum of squared deviations from it
__device__ __forceinline__ double diag_mean(const DiagSeries& s, int w, int d, int lo, int hi, double* sh, double* ssd) {
    const double len = (double)(hi - lo);
    double v = 0.0;
    for (int t = lo + threadIdx.x; t < hi; t += DIAG_THREADS) v += diag_x(s, w, d, t);
    const double m0 = diag_block_sum(v, sh) / len;
    v = 0.0;
    for (int t = lo + threadIdx.x; t < hi; t += DIAG_THREADS) v += diag_x(s, w, d, t) - m0;
    const double m = m0 + diag_block_sum(v, sh) / len;
    if (ssd) {
        v = 0.0;
        for (int t = lo + threadIdx.x; t < hi; t += DIAG_THREADS) {
            const double y = diag_x(s, w, d, t) - m;
            v = fma(y, y, v);
        }
        *ssd = diag_block_sum(v, sh);
    }
    return m;
}

// grid (W, D).  mean[w][d]; mom[w][d][4] = {mean, ssd} of the first half, {mean, ssd} of the second
__global__ __launch_bounds__(DIAG_THREADS) void lf_diag_moments(DiagSeries s, double* __restrict__ mean, double* __restrict__ mom) {
    __shared__ double sh[DIAG_THREADS];
    const int w = blockIdx.x, d = blockIdx.y;
    const int h = s.n / 2;
    double qa = 0.0, qb = 0.0;
    const double m = diag_mean(s, w, d, 0, s.n, sh, nullptr);
    const double ma = diag_mean(s, w, d, 0, h, sh, &qa);
    const double mb = diag_mean(s, w, d, s.n - h, s.n, sh, &qb);
    if (threadIdx.x == 0) {
        const size_t i = (size_t)w * s.D + d;
        mean[i] = m;
        mom[4 * i] = ma;
        mom[4 * i + 1] = qa;
        mom[4 * i + 2] = mb;
        mom[4 * i + 3] = qb;
    }
}

// where position p of the lagged segment is stored in its row
__device__ __forceinline__ int diag_idx(int p) { return p + 2 * (p >> 3); }

// grid (lag tiles of the pass, W, groups of DIAG_DG series).  a[w][d][tile 512 + l] = a_w[k_lo + tile 512 + l] of series d
// (row length Mp = gridDim.x 512); a0[w][d] = a_w[0], written by the pass that holds lag 0.
__global__ __launch_bounds__(DIAG_THREADS) void lf_diag_acf(DiagSeries s, const double* __restrict__ mean, int k_lo, double* __restrict__ a,
                                                            double* __restrict__ a0) {
    __shared__ __attribute__((aligned(16))) double ybase[DIAG_DG][DIAG_BASEROW];
    __shared__ __attribute__((aligned(16))) double ylag[DIAG_DG][DIAG_LAGROW];
    __shared__ double mu[DIAG_DG];
    const int w = blockIdx.y, g0 = blockIdx.z * DIAG_DG;
    const int nd = min(DIAG_DG, s.D - g0);
    const int K0 = k_lo + blockIdx.x * DIAG_LT;
    const int lane = threadIdx.x & 63, q = threadIdx.x >> 6;
    if ((int)threadIdx.x < nd) mu[threadIdx.x] = mean[(size_t)w * s.D + g0 + threadIdx.x];
    __syncthreads();
    double tot[DIAG_DG][DIAG_RL];
#pragma unroll
    for (int g = 0; g < DIAG_DG; ++g)
#pragma unroll
        for (int j = 0; j < DIAG_RL; ++j) tot[g][j] = 0.0;

    for (int tb = 0; tb + K0 < s.n; tb += DIAG_TB) {
        // the tile and the 768 values its lags reach, centred, series-major; 0.0 at and past n
        for (int e = threadIdx.x; e < DIAG_DG * (DIAG_TB + DIAG_TB + DIAG_LT); e += DIAG_THREADS) {
            const int g = e & (DIAG_DG - 1), i = e >> 2;
            if (g >= nd) continue;
            const bool lagged = i >= DIAG_TB;
            const int p = lagged ? i - DIAG_TB : i;
            const long long t = (long long)tb + p + (lagged ? K0 : 0);
            const double v = t < s.n ? diag_x(s, w, g0 + g, t) - mu[g] : 0.0;
            if (lagged) ylag[g][diag_idx(p)] = v;
            else ybase[g][p] = v;
        }
        __syncthreads();
#pragma unroll
        for (int g = 0; g < DIAG_DG; ++g) {
            if (g < nd) {
                const double* yb = ybase[g] + q * 64;
                // idx(u + 8 lane + j) = 10 lane + idx(u) + j for u % 8 == 0: 16-byte aligned, read two doubles at a time
                const double* yl = ylag[g] + 10 * lane + diag_idx(q * 64);
                double acc[DIAG_RL], win[2 * DIAG_RL];
#pragma unroll
                for (int j = 0; j < DIAG_RL; ++j) {
                    acc[j] = 0.0;
                    win[j] = yl[j];
                }
#pragma unroll
                for (int it = 0; it < 64 / DIAG_RL; ++it) {
#pragma unroll
                    for (int j = 0; j < DIAG_RL; ++j) win[DIAG_RL + j] = yl[10 * (it + 1) + j];
#pragma unroll
                    for (int i = 0; i < DIAG_RL; ++i) {
                        const double x = yb[it * DIAG_RL + i];
#pragma unroll
                        for (int j = 0; j < DIAG_RL; ++j) acc[j] = fma(x, win[i + j], acc[j]);
                    }
#pragma unroll
                    for (int j = 0; j < DIAG_RL; ++j) win[j] = win[DIAG_RL + j];
                }
#pragma unroll
                for (int j = 0; j < DIAG_RL; ++j) tot[g][j] += acc[j];
            }
        }
        __syncthreads();
    }

    // ((q0 + q1) + q2) + q3 per lag, through the lagged rows' LDS
    double* red = &ylag[0][0];
    static_assert(4 * DIAG_LT <= DIAG_DG * DIAG_LAGROW, "the waves' totals fit the lagged rows");
    const size_t Mp = (size_t)gridDim.x * DIAG_LT;
#pragma unroll
    for (int g = 0; g < DIAG_DG; ++g) {
        if (g < nd) {
#pragma unroll
            for (int j = 0; j < DIAG_RL; ++j) red[q * DIAG_LT + lane * DIAG_RL + j] = tot[g][j];
            __syncthreads();
            for (int l = threadIdx.x; l < DIAG_LT; l += DIAG_THREADS) {
                const double v = ((red[l] + red[DIAG_LT + l]) + red[2 * DIAG_LT + l]) + red[3 * DIAG_LT + l];
                const size_t sd = (size_t)w * s.D + g0 + g;
                a[sd * Mp + (size_t)blockIdx.x * DIAG_LT + l] = v;
                if (K0 + l == 0) a0[sd] = v;
            }
            __syncthreads();
        }
    }
}

// grid over D x Mp entries.  acf[d][l] of the pass's lags
__global__ __launch_bounds__(DIAG_THREADS) void lf_diag_norm(const double* __restrict__ a, const double* __restrict__ a0, int W, int D,
                                                             long long Mp, double* __restrict__ acf) {
    const long long i = (long long)blockIdx.x * DIAG_THREADS + threadIdx.x;
    if (i >= (long long)D * Mp) return;
    const int d = (int)(i / Mp);
    const long long l = i - (long long)d * Mp;
    double sum = 0.0;
    for (int w = 0; w < W; ++w) {
        const double z = a0[(size_t)w * D + d];
        if (z > 0.0) sum += a[((size_t)w * D + d) * (size_t)Mp + (size_t)l] / z;
    }
    acf[i] = sum / (double)W;
}

}  // namespace lf

namespace lfd {

// integrated_time's window on acf[0 .. M): taus[m] = 2 sum_{k <= m} acf[k] - 1, the window the first m with not (m < c taus[m]).
// Returns 0 when decided (then *window, *tau; no window below n means n - 1; a tau that is not finite or not positive gives 1.0;
// n < 4 gives 1.0 and window 0), 1 when no window lies below M and M < n: more lags are needed.
inline int chain_window(const double* acf, int64_t M, double c, int64_t n, double* tau, int64_t* window) {
#pragma clang fp contract(off)
    if (n < 4) {
        *tau = 1.0;
        *window = 0;
        return 0;
    }
    const int64_t L = M < n ? M : n;
    double cs = 0.0, taus = 0.0;
    int64_t win = -1;
    for (int64_t m = 0; m < L; ++m) {
        cs += acf[m];
        taus = 2.0 * cs - 1.0;
        if (!((double)m < c * taus)) {
            win = m;
            break;
        }
    }
    if (win < 0) {
        if (L < n) return 1;
        win = n - 1;                 // taus is taus[n - 1] here
    }
    *window = win;
    *tau = (std::isfinite(taus) && taus > 0.0) ? taus : 1.0;
    return 0;
}

// Split-R-hat (Gelman et al. 2013) of one parameter from mom[w][stride 4 D] = {mean, ssd} of each half of every walker: the
// 2 W half-sequences of length h have means th_j and variances s2_j = ssd_j / (h - 1);
//     Wv = mean(s2_j),  B / h = var(th_j, ddof = 1),  R-hat = sqrt(((h - 1) / h Wv + B / h) / Wv).   NaN for h < 2.
inline double split_rhat(const double* mom, int W, size_t stride, int64_t h) {
#pragma clang fp contract(off)
    if (h < 2) return std::nan("");
    const int m = 2 * W;
    double sm = 0.0, sv = 0.0;
    for (int w = 0; w < W; ++w)
        for (int p = 0; p < 2; ++p) {
            sm += mom[w * stride + 2 * p];
            sv += mom[w * stride + 2 * p + 1] / (double)(h - 1);
        }
    const double gm = sm / m, Wv = sv / m;
    double bs = 0.0;
    for (int w = 0; w < W; ++w)
        for (int p = 0; p < 2; ++p) {
            const double e = mom[w * stride + 2 * p] - gm;
            bs += e * e;
        }
    const double Bh = bs / (m - 1);
    const double vp = (double)(h - 1) / (double)h * Wv + Bh;
    return std::sqrt(vp / Wv);
}

}  // namespace lfd
