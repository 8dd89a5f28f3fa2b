// lf_veffdraws.h - the binned 1/Veff luminosity function of the catalogue under R posterior draws of the completeness
// parameters, and its percentiles over the draws (post-fit; lf_veff_draws of include/lfmcmc.h).
//
//   values[r][b] = sum_{i : bin_of[i] == b} w_i(d_r),   d_r = (Flim_0 .. Flim_{nf-1}, alpha)
//   w_i(d)       = vol_i > 0 ? 1 / (pref0 fleming(flux_i, Flim_{field_i}, alpha, fcmin) vol_i) : 0
//
// fleming with veff_weights' order of operations (lf_kernels.h; VmaxLumFunc.py:116-127, :164-167), no contraction.
//
// No atomics, one fixed order of summation: the host sorts the sources by bin (a stable counting sort; sources outside
// [0, nbin) are dropped), so that every bin is a contiguous segment, and cuts each segment into chunks of at most
// VEFFD_CHUNK sources - a chunk never spans two bins.
//   1. veffd_partial: one workgroup of 256 threads per (chunk, tile of 256 draws), one draw per thread.  The workgroup
//      stages the chunk's flux, 1 / (pref0 vol) (0 where vol <= 0) and field in LDS once; every thread walks the chunk in
//      source order with its sum in a register.  All lanes read the same source: broadcasts.  A thread's Flim are in LDS
//      as [field][lane] (consecutive lanes, consecutive banks).  The flux ftau where the modified curve has its knee is
//      Flim * 10^-sqrt(ratio / alpha^2), whose second factor depends on the draw alone and stays in a register: the product
//      is veff_weights' own, so a table of ftau would hold the same bits and double the LDS.
//      partial[chunk][r] gets the sum.
//   2. veffd_reduce: values[r][b] = the partials of bin b's chunks, added in chunk order; 0.0 for a bin without sources.
//   3. veffd_quant: lf_bands's stages over the nbin points with the values read from memory - bands_key, bands_sort,
//      bands_quantiles of lf_bands.h as they are (NumPy's quantile rule bit for bit; R <= 4096).
// So two calls with the same inputs give the same bits, and row r of values depends on draw r and the catalogue only: the
// chunks do not depend on R, and a thread's sum does not depend on its lane, its tile or the other draws.
//
// LDS: veffd_partial 32 KiB (Flim, 16 fields x 256 lanes) + 2 x 2 KiB (flux, 1 / (pref0 vol)) + 1 KiB (field) = 37 KiB, four
// workgroups per CU (160 KiB), four waves per SIMD - which 128 VGPRs allow; veffd_reduce none; veffd_quant the 32 KiB of
// keys.  nf is a runtime value <= VEFFD_MAXF; the Flim table is sized for the maximum so that the size is the compiler's
// to report (tests/test_veffdraws_resources.py).
#pragma once

#include <hip/hip_runtime.h>

#include "lf_bands.h"

namespace lf {

constexpr int VEFFD_CHUNK = 256;              // sources per chunk
constexpr int VEFFD_THREADS = 256;            // draws per tile
constexpr int VEFFD_MAXF = 16;

template <bool FCMIN>
__global__ __launch_bounds__(VEFFD_THREADS) void veffd_partial(const double* __restrict__ flux, const double* __restrict__ ipv,
                                                               const int* __restrict__ field, const long long* __restrict__ cstart,
                                                               const int* __restrict__ clen, const double* __restrict__ draws, int nf,
                                                               int R, double fc_ratio, double* __restrict__ partial) {
#pragma clang fp contract(off)
    static_assert(VEFFD_CHUNK <= VEFFD_THREADS, "one source per thread when the chunk is staged");
    __shared__ double s_flim[VEFFD_MAXF][VEFFD_THREADS];
    __shared__ double s_flux[VEFFD_CHUNK], s_ipv[VEFFD_CHUNK];
    __shared__ int s_field[VEFFD_CHUNK];
    const int c = blockIdx.x, lane = threadIdx.x;
    const int r = blockIdx.y * VEFFD_THREADS + lane;
    const long long s0 = cstart[c];
    const int len = clen[c];
    if (lane < len) {
        s_flux[lane] = flux[s0 + lane];
        s_ipv[lane] = ipv[s0 + lane];
        s_field[lane] = field[s0 + lane];
    }
    // (the lanes past R of the last tile work on the last draw and store nothing)
    const double* __restrict__ d = draws + (size_t)(r < R ? r : R - 1) * (size_t)(nf + 1);
    for (int f = 0; f < nf; ++f) s_flim[f][lane] = d[f];
    const double alpha = d[nf];
    double knee = 0.0;
    if constexpr (FCMIN) knee = exp10(-sqrt(fc_ratio / (alpha * alpha)));           // VmaxLumFunc.py:164-167
    __syncthreads();
    double acc = 0.0;
    for (int i = 0; i < len; ++i) {
        const double f = s_flux[i], fl = s_flim[s_field[i]][lane];
        const double num = alpha * log10(f / fl);                                   // :118-120
        double fc = 0.5 * (1.0 + num / sqrt(1.0 + num * num));
        if constexpr (FCMIN) {
            const double ftau = fl * knee;
            fc = pow(fc, 1.0 / (1.0 - exp(-f / ftau)));                             // :141, :125
        }
        const double a = s_ipv[i];
        acc += a > 0.0 ? a / fc : 0.0;
    }
    if (r < R) partial[(size_t)c * (size_t)R + (size_t)r] = acc;
}

// bin_c0[b] .. bin_c0[b + 1]: the chunks of bin b.  Consecutive threads take consecutive draws (coalesced rows of partial).
__global__ __launch_bounds__(VEFFD_THREADS) void veffd_reduce(const double* __restrict__ partial, const int* __restrict__ bin_c0, int nbin,
                                                              int R, double* __restrict__ values) {
#pragma clang fp contract(off)
    const int b = blockIdx.y;
    const int r = blockIdx.x * VEFFD_THREADS + threadIdx.x;
    if (r >= R) return;
    double s = 0.0;
    for (int c = bin_c0[b]; c < bin_c0[b + 1]; ++c) s += partial[(size_t)c * (size_t)R + (size_t)r];
    values[(size_t)r * (size_t)nbin + (size_t)b] = s;
}

// lf_bands with stage 1 replaced by a read of values[R][P]
__global__ __launch_bounds__(BANDS_THREADS) void veffd_quant(const double* __restrict__ values, int R, int lg, int P,
                                                             const double* __restrict__ qtab, int nq, int median,
                                                             double* __restrict__ out) {
    __shared__ unsigned long long key[BANDS_SLOTS];
    const int Rp = 1 << lg;
    const int G = BANDS_SLOTS >> lg;
    for (int base = blockIdx.x * G; base < P; base += gridDim.x * G) {
        for (int i = threadIdx.x; i < BANDS_SLOTS; i += BANDS_THREADS) {
            const int r = i & (Rp - 1);
            const int p = base + (i >> lg);
            key[i] = (r < R && p < P) ? bands_key(values[(size_t)r * (size_t)P + (size_t)p]) : BANDS_PAD;
        }
        __syncthreads();
        bands_sort(key, Rp);
        bands_quantiles(key, base, G, Rp, R, P, qtab, nq, median, out);
        __syncthreads();                                   // the next pass overwrites the keys
    }
}

}  // namespace lf
