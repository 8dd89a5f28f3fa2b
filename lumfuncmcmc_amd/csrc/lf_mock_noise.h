// lf_mock_noise.h - the observation step of the mock catalogues on the device (lf_mock_draw_err, lf_mock_hist_err,
// include/lfmcmc.h).  lf_mock.h draws a source's true (z, L); this header adds what the catalogue
// records of it under the generative model of section 3.18:
//     L_obs = L_true + sigma * n,   n ~ N(0, 1),   sigma = sigma(field, log10 flux of the true source)   (after detection)
//
// The error model.  M nodes x[0] < .. < x[M - 1] of log10 flux (cgs), shared by the fields, and sig[f][M] >= 0: sigma is
// linear between the nodes and constant outside them (M = 1: one value per field).  mock_sigma: t <= x[0] -> sig[0];
// t >= x[M - 1] -> sig[M - 1]; else i = (number of nodes <= t) - 1 and
//     sigma = sig[i] + (t - x[i]) * ((sig[i + 1] - sig[i]) / (x[i + 1] - x[i])).
//
// The flux of a mock source at (z, L):  log10 f = L - ld2(z), ld2 the linear interpolant over zarr of
// ld2n[k] = log10(4 pi (3.086e24 DL_zarr[k])^2) (the host makes ld2n): i = (number of zarr <= z) - 1 clamped to 0 .. S - 2,
//     ld2 = ld2n[i] + (z - zarr[i]) * ((ld2n[i + 1] - ld2n[i]) / (zarr[i + 1] - zarr[i])).
// Both interpolants run with contraction off: the host twin (mock.py) states the same expressions in the same order.
//
// The noise.  Philox block (row_id, index, purpose 3, field) of lf_mock.h's stream word - a block of its own, so the true
// draws keep their bits - and Box-Muller on its two 53-bit uniforms: n = sqrt(-2 log1p(-u1)) * cos(2 pi u2) (1 - u1 is in
// (0, 1]: no log of 0; n is finite, so sigma = 0 gives L_obs = L_true + (+-0) = L_true bit for bit).  This is mock.lum_noise.
//
// Kernels (256 threads, no scratch):
//   lf_mock_draw_err  one thread per source, as lf_mock_draw: mock_source, then flux, sigma (table through global loads)
//                     and noise; plain vector stores of z, L_true, L_obs, sigma, field.  No LDS.
//   lf_mock_hist_err  lf_mock_hist's shape (MOCK_HIST_CHUNK sources of one (row, field) per workgroup, LDS histogram, 64-bit
//                     integer atomics to HBM), binned by L_obs.  LDS: lf_mock_hist's 12 KiB plus the nodes and the
//                     workgroup's field's sigma row, 2 x 64 doubles = 1 KiB.
#pragma once
#include "lf_mock.h"

namespace lf {

constexpr int MOCK_MAX_NODES = 64;
constexpr unsigned int MOCK_NOISE_PURPOSE = 3u;

struct MockNoise {
    int M;                    // nodes, 1 .. MOCK_MAX_NODES
    const double* nodes;      // [M] log10 flux
    const double* sigma;      // [nf][M] dex
    const double* ld2n;       // [S] log10(4 pi (Mpc DL_zarr)^2)
};

// sigma(t) on one field's row of the table, see the file comment
__device__ __forceinline__ double mock_sigma(const double* __restrict__ x, const double* __restrict__ sig, int M, double t) {
#pragma clang fp contract(off)
    if (!(t > x[0])) return sig[0];
    if (t >= x[M - 1]) return sig[M - 1];
    int lo = 1, hi = M - 1;                     // first node > t (x[0] < t < x[M - 1])
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (x[mid] > t) hi = mid; else lo = mid + 1;
    }
    const int i = lo - 1;
    return sig[i] + (t - x[i]) * ((sig[i + 1] - sig[i]) / (x[i + 1] - x[i]));
}

// log10 flux of a source of log luminosity L at redshift z
__device__ __forceinline__ double mock_logflux(const double* __restrict__ zarr, const double* __restrict__ ld2n, int S, double z,
                                               double L) {
#pragma clang fp contract(off)
    int lo = 0, hi = S;                         // number of zarr <= z
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (zarr[mid] <= z) lo = mid + 1; else hi = mid;
    }
    int i = lo - 1;
    i = i < 0 ? 0 : (i > S - 2 ? S - 2 : i);
    const double ld2 = ld2n[i] + (z - zarr[i]) * ((ld2n[i + 1] - ld2n[i]) / (zarr[i + 1] - zarr[i]));
    return L - ld2;
}

// standard normal deviate of source `index` of (row, field)
__device__ __forceinline__ double mock_noise(unsigned long long row_id, unsigned int index, int f, unsigned long long seed) {
#pragma clang fp contract(off)
    unsigned int r[4];
    mock_philox(row_id, index, MOCK_NOISE_PURPOSE, f, seed, r);
    const double u1 = u53(r[0], r[1]), u2 = u53(r[2], r[3]);
    return sqrt(-2.0 * log1p(-u1)) * cos((2.0 * 3.141592653589793) * u2);
}

__device__ __forceinline__ double mock_observe(double L, double sg, double n) {
#pragma clang fp contract(off)
    return L + sg * n;
}

__global__ __launch_bounds__(MOCK_THREADS) void lf_mock_draw_err(MockConst mc, MockNoise mn, int nrf, const long long* __restrict__ off,
                                                                 const long long* __restrict__ row_ids, unsigned long long seed,
                                                                 const double* __restrict__ cdfL, const double* __restrict__ cdfZ,
                                                                 double* __restrict__ z, double* __restrict__ logL,
                                                                 double* __restrict__ logLobs, double* __restrict__ sigma,
                                                                 int* __restrict__ field) {
    const long long g = (long long)blockIdx.x * MOCK_THREADS + threadIdx.x;
    if (g >= off[nrf]) return;
    const int rf = mock_owner(off, nrf, g);
    const int row = rf / mc.nf, f = rf - row * mc.nf;
    const unsigned long long rid = (unsigned long long)row_ids[row];
    const unsigned int i = (unsigned int)(g - off[rf]);
    double zz, LL;
    mock_source(mc, rf, f, rid, i, seed, cdfL, cdfZ, zz, LL);
    const double t = mock_logflux(mc.zarr, mn.ld2n, mc.S, zz, LL);
    const double sg = mock_sigma(mn.nodes, mn.sigma + (size_t)f * mn.M, mn.M, t);
    z[g] = zz;
    logL[g] = LL;
    logLobs[g] = mock_observe(LL, sg, mock_noise(rid, i, f, seed));
    sigma[g] = sg;
    field[g] = f;
}

// blk, count, hist: as lf_mock_hist; slot = searchsorted(edges, L_obs, side="right")
__global__ __launch_bounds__(MOCK_THREADS) void lf_mock_hist_err(MockConst mc, MockNoise mn, int nrf, const long long* __restrict__ blk,
                                                                 const long long* __restrict__ count,
                                                                 const long long* __restrict__ row_ids, unsigned long long seed,
                                                                 const double* __restrict__ cdfL, const double* __restrict__ cdfZ,
                                                                 int nbins, const double* __restrict__ edges,
                                                                 unsigned long long* __restrict__ hist) {
    __shared__ double le[MOCK_MAX_BINS + 2];
    __shared__ unsigned int lh[MOCK_MAX_BINS + 2];
    __shared__ double lx[MOCK_MAX_NODES], ls[MOCK_MAX_NODES];
    const long long b = blockIdx.x;
    const int rf = mock_owner(blk, nrf, b);
    const int row = rf / mc.nf, f = rf - row * mc.nf;
    const int ne = nbins + 1, ns = nbins + 2, M = mn.M;
    for (int i = threadIdx.x; i < ne; i += MOCK_THREADS) le[i] = edges[i];
    for (int i = threadIdx.x; i < ns; i += MOCK_THREADS) lh[i] = 0u;
    if ((int)threadIdx.x < M) {
        lx[threadIdx.x] = mn.nodes[threadIdx.x];
        ls[threadIdx.x] = mn.sigma[(size_t)f * M + threadIdx.x];
    }
    __syncthreads();
    const unsigned long long rid = (unsigned long long)row_ids[row];
    const long long first = (b - blk[rf]) * MOCK_HIST_CHUNK, n = count[rf];
    for (int s = 0; s < MOCK_HIST_ITEMS; ++s) {
        const long long i = first + (long long)s * MOCK_THREADS + threadIdx.x;
        if (i >= n) break;
        double zz, LL;
        mock_source(mc, rf, f, rid, (unsigned int)i, seed, cdfL, cdfZ, zz, LL);
        const double t = mock_logflux(mc.zarr, mn.ld2n, mc.S, zz, LL);
        const double sg = mock_sigma(lx, ls, M, t);
        const double Lo = mock_observe(LL, sg, mock_noise(rid, (unsigned int)i, f, seed));
        int lo = 0, hi = ne;                        // number of edges <= Lo
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (le[mid] <= Lo) lo = mid + 1; else hi = mid;
        }
        atomicAdd(&lh[lo], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < ns; i += MOCK_THREADS)
        if (lh[i]) atomicAdd(&hist[(size_t)rf * ns + i], (unsigned long long)lh[i]);
}

}  // namespace lf
