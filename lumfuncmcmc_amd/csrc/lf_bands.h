// lf_bands.h - percentiles of the model luminosity function over R posterior draws at P points (post-fit; DESIGN.md
// section 3.9).  Replaces the draw loop of LumFuncMCMC.set_median_fit (lumfuncmcmc.py:527-567: R TrueLumFunc
// evaluations over the catalogue, then np.median over the draws) and gives the credible bands around it.
//
// One workgroup of 256 threads owns BANDS_SLOTS = 4096 keys of LDS (32 KiB): G = 4096 / Rp points at a time, Rp = the
// power of two >= R.  Per pass it
//   1. evaluates v[r][p] for its G points and R draws (device-library exp10 / exp, the host's order of operations, no
//      contraction) and stores the order-preserving 64-bit key of each value; the Rp - R slots of a point left over and
//      the slots of points past P hold BANDS_PAD, a key above every finite value's and +inf's;
//   2. sorts each point's Rp keys ascending with one bitonic network run over all 4096 slots (a compare-exchange never
//      crosses a point: the partner of slot i at distance j < Rp lies in the same aligned run of Rp slots, and the
//      direction is taken from the slot's index within its run, so that every run ends ascending);
//   3. reads the order statistics the quantiles need and applies NumPy's rule (below), G x nq results.
// The R x P matrix never exists in HBM (unless the caller asks for it: `values`), every point is read once and every
// quantile written once.  Grid-stride over passes: P may be 10^6 and more.
//
// The quantile rule is NumPy 2.x's, bit for bit, given the same values:
//   np.percentile (LINEAR): the host turns each q into (prev, next, gamma) exactly as numpy's _quantile /
//   _get_indexes / _get_gamma do (vi = (R - 1) q / 100; lf_lumfunc_quantiles in lfmcmc.hip); here  d = b - a,
//   result = a + d * gamma  if gamma < 0.5  else  b - d * (1 - gamma)   (numpy's _lerp, applied literally:
//   a == b == inf gives NaN as np.percentile does);
//   np.median (MEDIAN): the middle order statistic, or (a + b) / 2 for even R (np.mean of the two middle ones).
// A NaN among a point's values makes every result of the point NaN (numpy's slices_having_nans / _median_nancheck).  NaN
// keys sort below -inf (negative sign) or between +inf and the pad (positive sign), so the point has a NaN exactly when
// its smallest or its largest order statistic decodes to one.
#pragma once

#include <hip/hip_runtime.h>

#include "lf_gammainc.h"

namespace lf {

constexpr int BANDS_SLOTS = 4096;             // keys per workgroup: R <= 4096
constexpr int BANDS_THREADS = 256;
constexpr int BANDS_MAXQ = 32;
constexpr unsigned long long BANDS_PAD = ~0ull;

// Order-preserving map of binary64 to unsigned 64-bit: negative values flip all bits, the others set the sign bit.
__device__ __forceinline__ unsigned long long bands_key(double v) {
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

__device__ __forceinline__ double bands_value(unsigned long long k) {
    return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
}

// The model LF of one draw at one point, operations as hostsetup.true_lum_func / schechter_z group them:
//   LN10 * 10^logphistar * 10^(t (alpha + 1)) * exp(-10^t),  t = logL - logLstar, multiplied left to right.
// NP = 3 (single Schechter): rec = {logLstar, LN10 * 10^logphistar, alpha + 1} - the first factor and alpha + 1 do not
// depend on the point, the host makes them (they are numpy scalar operations in the reference's order too).
// NP = 7 (z-evolving): rec = {aL, bL, cL, aphi, bphi, cphi, alpha + 1}: logLstar = aL (z z) + bL z + cL, logphistar the
// same, so 10^logphistar is per point here.
template <int NP>
__device__ __forceinline__ double bands_eval(const double* __restrict__ rec, double logL, double z) {
#pragma clang fp contract(off)
    double lstar, pref;
    if constexpr (NP == 3) {
        lstar = rec[0];
        pref = rec[1];
    } else {
        const double zz = z * z;
        lstar = rec[0] * zz + rec[1] * z + rec[2];
        const double lphi = rec[3] * zz + rec[4] * z + rec[5];
        pref = 2.302585092994045684 * exp10(lphi);
    }
    const double t = logL - lstar;
    return pref * exp10(t * rec[NP - 1]) * exp(-exp10(t));
}

// The integrated LF of one draw above one limit: prefactor * Gamma(a, 10^(logLmin - logLstar)),
// a = alpha + 1 + KIND; KIND 0 = number density (prefactor 10^logphistar), 1 = luminosity density (10^logphistar
// 10^logLstar).  NP = 3: rec = {logLstar, prefactor, a}, the host makes the last two; NP = 7: rec = {aL, bL, cL, aphi,
// bphi, cphi, a}, prefactor per point.  The powers of ten are gi_exp10's, which lfintegrals.exp10 repeats to the bit.
template <int NP, int KIND>
__device__ __forceinline__ double bands_integ_eval(const double* __restrict__ rec, double logLmin, double z) {
#pragma clang fp contract(off)
    double lstar, pref;
    if constexpr (NP == 3) {
        lstar = rec[0];
        pref = rec[1];
    } else {
        const double zz = z * z;
        lstar = rec[0] * zz + rec[1] * z + rec[2];
        const double lphi = rec[3] * zz + rec[4] * z + rec[5];
        pref = KIND ? gi_exp10(lphi) * gi_exp10(lstar) : gi_exp10(lphi);
    }
    return pref * gammainc_upper(rec[NP - 1], gi_exp10(logLmin - lstar));
}

// 2. bitonic sort of every aligned run of Rp slots of key[BANDS_SLOTS]; ends with the workgroup synchronised
__device__ __forceinline__ void bands_sort(unsigned long long* key, int Rp) {
    for (int k = 2; k <= Rp; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = threadIdx.x; t < BANDS_SLOTS / 2; t += BANDS_THREADS) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));      // bit j of i is clear; partner i + j
                const bool up = (i & k & (Rp - 1)) == 0;
                const unsigned long long a = key[i], b = key[i + j];
                if ((a > b) == up) {
                    key[i] = b;
                    key[i + j] = a;
                }
            }
            __syncthreads();
        }
    }
}

// 3. quantiles of the G sorted runs: consecutive threads take consecutive points of one quantile (coalesced rows of out)
// qtab[3 q + {0, 1, 2}] = {prev, next, gamma} per quantile (LINEAR; indices stored as doubles, exact).
__device__ __forceinline__ void bands_quantiles(const unsigned long long* key, long long base, int G, int Rp, int R, long long P,
                                                const double* __restrict__ qtab, int nq, int median, double* __restrict__ out) {
#pragma clang fp contract(off)
    for (int t = threadIdx.x; t < G * nq; t += BANDS_THREADS) {
        const int qi = t / G, s = t - qi * G;
        const long long p = base + s;
        if (p >= P) continue;
        const unsigned long long* run = key + s * Rp;
        double res;
        if (__builtin_isnan(bands_value(run[0])) || __builtin_isnan(bands_value(run[R - 1]))) {
            res = __builtin_nan("");
        } else if (median) {
            const int h = R >> 1;
            res = (R & 1) ? bands_value(run[h]) : (bands_value(run[h - 1]) + bands_value(run[h])) / 2.0;
        } else {
            const double a = bands_value(run[(int)qtab[3 * qi]]), b = bands_value(run[(int)qtab[3 * qi + 1]]);
            const double g = qtab[3 * qi + 2];
            const double d = b - a;
            res = g < 0.5 ? a + d * g : b - d * (1.0 - g);
        }
        out[(size_t)qi * (size_t)P + (size_t)p] = res;
    }
}

template <int NP>
__global__ __launch_bounds__(BANDS_THREADS) void lf_bands(const double* __restrict__ recs, int R, int lg, const double* __restrict__ logL,
                                                          const double* __restrict__ zp, long long P, const double* __restrict__ qtab, int nq,
                                                          int median, double* __restrict__ out, double* __restrict__ values) {
#pragma clang fp contract(off)
    __shared__ unsigned long long key[BANDS_SLOTS];
    const int Rp = 1 << lg;
    const int G = BANDS_SLOTS >> lg;
    for (long long base = (long long)blockIdx.x * G; base < P; base += (long long)gridDim.x * G) {
        // 1. values -> keys
        for (int i = threadIdx.x; i < BANDS_SLOTS; i += BANDS_THREADS) {
            const int r = i & (Rp - 1);
            const long long p = base + (i >> lg);
            unsigned long long k = BANDS_PAD;
            if (r < R && p < P) {
                const double v = bands_eval<NP>(recs + (size_t)r * NP, logL[p], NP == 7 ? zp[p] : 0.0);
                if (values) values[(size_t)r * (size_t)P + (size_t)p] = v;
                k = bands_key(v);
            }
            key[i] = k;
        }
        __syncthreads();
        bands_sort(key, Rp);
        bands_quantiles(key, base, G, Rp, R, P, qtab, nq, median, out);
        __syncthreads();                                   // the next pass overwrites the keys
    }
}

// lf_bands with the integrated LF in stage 1 (logL holds the lower limits logLmin); stages 2 and 3 are lf_bands's.
template <int NP, int KIND>
__global__ __launch_bounds__(BANDS_THREADS) void lf_bands_integ(const double* __restrict__ recs, int R, int lg,
                                                                const double* __restrict__ logL, const double* __restrict__ zp, long long P,
                                                                const double* __restrict__ qtab, int nq, int median,
                                                                double* __restrict__ out, double* __restrict__ values) {
#pragma clang fp contract(off)
    __shared__ unsigned long long key[BANDS_SLOTS];
    const int Rp = 1 << lg;
    const int G = BANDS_SLOTS >> lg;
    for (long long base = (long long)blockIdx.x * G; base < P; base += (long long)gridDim.x * G) {
        for (int i = threadIdx.x; i < BANDS_SLOTS; i += BANDS_THREADS) {
            const int r = i & (Rp - 1);
            const long long p = base + (i >> lg);
            unsigned long long k = BANDS_PAD;
            if (r < R && p < P) {
                const double v = bands_integ_eval<NP, KIND>(recs + (size_t)r * NP, logL[p], NP == 7 ? zp[p] : 0.0);
                if (values) values[(size_t)r * (size_t)P + (size_t)p] = v;
                k = bands_key(v);
            }
            key[i] = k;
        }
        __syncthreads();
        bands_sort(key, Rp);
        bands_quantiles(key, base, G, Rp, R, P, qtab, nq, median, out);
        __syncthreads();
    }
}

}  // namespace lf
