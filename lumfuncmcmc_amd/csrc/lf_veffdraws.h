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
//
// veffd_partial_zmax (lf_veff_draws_zmax) is stage 1 with every source's volume ending at the z_max of
// the DRAW's flux cut: per source the LDS holds s_i = sqrt(L_i / 4 pi) / Mpc_cm in the place of 1 / (pref0 vol), per (field,
// lane) c = fmin^(-1/2) next to Flim, and per (source, lane) the volume is V(D), D = s_i c (one rounded product), from the
// table of lumfuncmcmc_amd/voltable.py:
//   D >= D_K: V_total (the weight's first factor is then the host's 1 / (pref0 V_total): lf_veff_draws' bits); D <= D_0, NaN: 0;
//   otherwise z = the z piece's polynomial (VEFFZ_NPIECE equal pieces in D, degree VEFFZ_DEG, Horner in the piece's own
//   t in [0, 1)), the node piece k with D_k <= D < D_k+1 - guessed from z (the nodes are evenly spaced), then its
//   neighbour, then a bisection of the records' edges (at most 31 steps, whatever the table's guess is worth) - and
//   V = c0_k + (y_k + hs_k dz) dz, dz = z - t_k, clamped into [c0_k, c0_k+1].
// The grid, the chunks, the order of summation, stages 2 and 3 are veffd_partial's.  Chosen layout: the 256-lane tile stays,
// and the kernel is instantiated for nf <= VEFFZ_FEW = 8 and for nf <= 16 fields.  LDS = 2 x MAXF x 2 KiB (Flim and c,
// [MAXF fields][256 lanes]) + 2 x 2 KiB (flux, s) + 1 KiB (field) + 2.25 KiB (the z pieces, rows padded to 9 doubles so that
// the 32 pieces start on 32 different bank pairs): 40192 bytes for 8 fields - four workgroups per CU (160 KiB), four waves
// per SIMD, veffd_partial's occupancy - and 72960 bytes for 16 - two workgroups, two waves per SIMD.  The compiler reports 48
// VGPRs for all four instantiations, so the LDS alone sets the occupancy.  The z pieces are read at lane-divergent addresses
// (ds_read_b64: a conflict only between different pieces within 32 lanes, and the lanes of a chunk - one luminosity bin -
// fall into a few neighbouring pieces); the node records (64 bytes each, one per node of dV/dz: up to 64 MB) cannot be in
// LDS and are read through L1 / L2, one aligned half line per (source, lane) between the clamps, beside the loop's pow, exp
// and log10 in fp64.  Rejected: one 16-field layout for every nf (half the occupancy for the common catalogues of a few
// fields); 128-lane tiles (two waves per SIMD again, at twice the staging and launches); c in registers indexed by a runtime
// field (scratch, or a select chain per field); one polynomial of V per node with its own coefficients (more bytes per pair
// and a builder that inverts DL several times per node); the z pieces through L1 (a second divergent global read per pair).
#pragma once

#include <hip/hip_runtime.h>

#include "lf_bands.h"

namespace lf {

constexpr int VEFFD_CHUNK = 256;              // sources per chunk
constexpr int VEFFD_THREADS = 256;            // draws per tile
constexpr int VEFFD_MAXF = 16;
constexpr int VEFFZ_NPIECE = 32;              // z pieces of the volume table (voltable.NPIECE)
constexpr int VEFFZ_DEG = 7;                  // their degree (voltable.DEG)
constexpr int VEFFZ_FEW = 8;                  // the narrow instantiation's fields
constexpr int VEFFZ_REC = 8;                  // doubles per node record: D_k, D_k+1, t_k, c0_k, c0_k+1, y_k, hs_k, 0

// the table's scalars: D_0, D_K, NPIECE / (D_K - D_0), the first inner node and 1 / spacing (the guess of k), K, and the
// weight's first factor at the upper clamp, 1 / (pref0 V_total) as the host divides it
struct VeffzHead {
    double d_lo, d_hi, invw, z_first, inv_h, a_full;
    int K;
};

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

template <bool FCMIN, int MAXF>
__global__ __launch_bounds__(VEFFD_THREADS) void veffd_partial_zmax(const double* __restrict__ flux, const double* __restrict__ dist,
                                                                    const int* __restrict__ field, const long long* __restrict__ cstart,
                                                                    const int* __restrict__ clen, const double* __restrict__ draws,
                                                                    const double* __restrict__ cfac, int nf, int R, double fc_ratio,
                                                                    double pref0, VeffzHead h, const double* __restrict__ zc,
                                                                    const double* __restrict__ rec, double* __restrict__ partial) {
#pragma clang fp contract(off)
    static_assert(VEFFD_CHUNK <= VEFFD_THREADS, "one source per thread when the chunk is staged");
    constexpr int ZROW = VEFFZ_DEG + 2;                                             // padded row of the z pieces
    __shared__ double s_flim[MAXF][VEFFD_THREADS], s_c[MAXF][VEFFD_THREADS];
    __shared__ double s_flux[VEFFD_CHUNK], s_dist[VEFFD_CHUNK];
    __shared__ double s_zc[VEFFZ_NPIECE * ZROW];
    __shared__ int s_field[VEFFD_CHUNK];
    const int c = blockIdx.x, lane = threadIdx.x;
    const int r = blockIdx.y * VEFFD_THREADS + lane;
    const long long s0 = cstart[c];
    const int len = clen[c];
    if (lane < len) {
        s_flux[lane] = flux[s0 + lane];
        s_dist[lane] = dist[s0 + lane];
        s_field[lane] = field[s0 + lane];
    }
    for (int j = lane; j < VEFFZ_NPIECE * (VEFFZ_DEG + 1); j += VEFFD_THREADS)
        s_zc[(j / (VEFFZ_DEG + 1)) * ZROW + j % (VEFFZ_DEG + 1)] = zc[j];
    const size_t rr = (size_t)(r < R ? r : R - 1);
    const double* __restrict__ d = draws + rr * (size_t)(nf + 1);
    for (int f = 0; f < nf; ++f) {
        s_flim[f][lane] = d[f];
        s_c[f][lane] = cfac[rr * (size_t)nf + (size_t)f];
    }
    const double alpha = d[nf];
    double knee = 0.0;
    if constexpr (FCMIN) knee = exp10(-sqrt(fc_ratio / (alpha * alpha)));
    __syncthreads();
    double acc = 0.0;
    for (int i = 0; i < len; ++i) {
        const int fi = s_field[i];
        const double D = s_dist[i] * s_c[fi][lane];
        double a = 0.0;                                                             // 1 / (pref0 V), 0 without a volume
        if (D >= h.d_hi) {
            a = h.a_full;
        } else if (D > h.d_lo) {
            const double u = (D - h.d_lo) * h.invw;
            const int p = min((int)u, VEFFZ_NPIECE - 1);
            const double t = u - (double)p;
            const double* __restrict__ q = s_zc + p * ZROW;
            double z = q[VEFFZ_DEG];
#pragma unroll
            for (int j = VEFFZ_DEG - 1; j >= 0; --j) z = z * t + q[j];
            const double g = floor((z - h.z_first) * h.inv_h) + 1.0;
            int k = (int)fmin(fmax(g, 0.0), (double)(h.K - 1));
            const double* __restrict__ rk = rec + (size_t)k * VEFFZ_REC;
            if (D < rk[0] || D >= rk[1]) {                                          // the guess is off: its neighbour, or bisect
                k = D < rk[0] ? max(k - 1, 0) : min(k + 1, h.K - 1);
                rk = rec + (size_t)k * VEFFZ_REC;
                if (D < rk[0] || D >= rk[1]) {
                    int lo = 0, hi = h.K - 1;                                       // the last k with D_k <= D: at most 31 steps
                    while (lo < hi) {
                        const int mid = lo + (hi - lo + 1) / 2;
                        if (rec[(size_t)mid * VEFFZ_REC] <= D) lo = mid; else hi = mid - 1;
                    }
                    k = lo;
                    rk = rec + (size_t)k * VEFFZ_REC;
                }
            }
            const double dz = z - rk[2];
            double V = rk[3] + (rk[5] + rk[6] * dz) * dz;
            V = fmin(fmax(V, rk[3]), rk[4]);
            a = V > 0.0 ? 1.0 / (pref0 * V) : 0.0;
        }
        const double f = s_flux[i], fl = s_flim[fi][lane];
        const double num = alpha * log10(f / fl);
        double fc = 0.5 * (1.0 + num / sqrt(1.0 + num * num));
        if constexpr (FCMIN) {
            const double ftau = fl * knee;
            fc = pow(fc, 1.0 / (1.0 - exp(-f / ftau)));
        }
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
