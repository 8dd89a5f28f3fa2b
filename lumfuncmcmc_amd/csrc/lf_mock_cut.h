// lf_mock_cut.h - mock catalogues of the cut process on the device (lf_mock_draw_cut, lf_mock_hist_cut, include/lfmcmc.h;
// DESIGN.md section 3.32): what the convolved likelihood under a cut on the observed flux models (section 3.31).  Sources
// are detected at their true flux and catalogued only when L_obs = L_true + sigma n >= Lam_k = logL[0][k], the lower edge
// of the integration grid at the redshift column k of the node the source picked.
//
// A cut mock is the union of two independent Poisson processes of candidates, each observed and cut in the same way:
//   piece "above"  lf_mock.h's process on the integration grid (L_true >= Lam_k), Philox purposes 0-3 as ever: the same
//                  counts, true draws and noise deviates as lf_mock_draw_err gives;
//   piece "below"  the same kind of process on the band grid logLb[j][k], S nodes over [Lam_k - H, Lam_k] per column
//                  (lf_mock_set_cut_band; lf_mock_mass and lf_mock_total run on it with logL and integ_part exchanged), on
//                  purposes 4-7 (count, node and z hat, L hat, noise): MOCK_CUT_BAND is ORed into the field argument of
//                  mock_poisson, mock_source and mock_noise, which lands on bit 2 of the purpose byte of the stream word
//                  (MOCK_TAG | purpose << 8 | field; fields are below 256).  Piece "above" keeps its bits.
// Observation of a candidate (z, L_t) of column k, contraction off, the host twin (mock.py) stating the same expressions:
//     sigma = mock_sigma(field, L_t - ld2n[k])      (the column's own ld2n[k], as u in Delta B; not the interpolant in z)
//     L_o   = L_t + sigma * n                       (mock_observe, mock_noise)
//     keep  = L_o >= logL[0][k]
// Rejection is exact: no truncated-normal draw, no inverse error function.
//
// Kernels (256 threads, no scratch; launched once per piece):
//   lf_mock_count_cut  one thread per (row, field): the band's Poisson count on purpose 4 from the mean lf_mock_total left.
//   lf_mock_draw_cut   one thread per candidate of one piece, lf_mock_draw_err's shape: candidate i of (row, field) rf goes
//                      to slot dst[rf] + i; plain vector stores of z, L_true, L_obs, sigma, field and a 32-bit keep flag.
//                      The kept sources are compacted on the host.  No LDS.
//   lf_mock_hist_cut   lf_mock_hist_err's shape (MOCK_HIST_CHUNK candidates of one (row, field) per workgroup, LDS
//                      histogram, 64-bit integer atomics to HBM): bins the kept candidates by L_o and counts them per
//                      (row, field) in kept[rf].  Both pieces add into one histogram; integer adds are order-free.  LDS:
//                      lf_mock_hist_err's 13 KiB plus one counter.  The edge and ld2n[k] are plain global loads.
#pragma once
#include "lf_mock_noise.h"

namespace lf {

constexpr unsigned int MOCK_CUT_BAND = 4u << 8;         // piece "below": purposes 4 + (0 .. 3)

struct MockCut {
    const double* edge;       // [S] Lam_k: row 0 of the integration grid's logL (= row S - 1 of the band's)
    unsigned int stream;      // 0: piece "above"; MOCK_CUT_BAND: piece "below"
};

// candidate i of (row, field) rf of one piece: true draw, observation, cut
__device__ __forceinline__ bool mock_cut_candidate(const MockConst& mc, const MockCut& ct, const double* __restrict__ ld2n,
                                                   const double* __restrict__ nodes, const double* __restrict__ sig, int M, int rf,
                                                   int f, unsigned long long rid, unsigned int i, unsigned long long seed,
                                                   const double* __restrict__ cdfL, const double* __restrict__ cdfZ, double& z,
                                                   double& L, double& Lo, double& sg) {
#pragma clang fp contract(off)
    const int fs = f | (int)ct.stream;
    int k;
    mock_source(mc, rf, fs, rid, i, seed, cdfL, cdfZ, z, L, k);
    sg = mock_sigma(nodes, sig, M, L - ld2n[k]);
    Lo = mock_observe(L, sg, mock_noise(rid, i, fs, seed));
    return Lo >= ct.edge[k];
}

// mean: [nrf] the band's expected counts (lf_mock_total); count: [nrf], -1 for a mean the caller must refuse
__global__ __launch_bounds__(MOCK_THREADS) void lf_mock_count_cut(int nrf, int nf, const double* __restrict__ mean,
                                                                  const long long* __restrict__ row_ids, unsigned long long seed,
                                                                  long long* __restrict__ count) {
    const int rf = blockIdx.x * MOCK_THREADS + threadIdx.x;
    if (rf >= nrf) return;
    const int row = rf / nf, f = rf - row * nf;
    count[rf] = mock_poisson(mean[rf], (unsigned long long)row_ids[row], f | (int)MOCK_CUT_BAND, seed);
}

// off: [nrf + 1] this piece's candidates of rf are [off[rf], off[rf + 1]); dst: [nrf] their first slot in the outputs
__global__ __launch_bounds__(MOCK_THREADS) void lf_mock_draw_cut(MockConst mc, MockNoise mn, MockCut ct, int nrf,
                                                                 const long long* __restrict__ off, const long long* __restrict__ dst,
                                                                 const long long* __restrict__ row_ids, unsigned long long seed,
                                                                 const double* __restrict__ cdfL, const double* __restrict__ cdfZ,
                                                                 double* __restrict__ z, double* __restrict__ logL,
                                                                 double* __restrict__ logLobs, double* __restrict__ sigma,
                                                                 int* __restrict__ field, int* __restrict__ keep) {
    const long long g = (long long)blockIdx.x * MOCK_THREADS + threadIdx.x;
    if (g >= off[nrf]) return;
    const int rf = mock_owner(off, nrf, g);
    const int row = rf / mc.nf, f = rf - row * mc.nf;
    const unsigned int i = (unsigned int)(g - off[rf]);
    double zz, LL, Lo, sg;
    const bool kept = mock_cut_candidate(mc, ct, mn.ld2n, mn.nodes, mn.sigma + (size_t)f * mn.M, mn.M, rf, f,
                                         (unsigned long long)row_ids[row], i, seed, cdfL, cdfZ, zz, LL, Lo, sg);
    const long long o = dst[rf] + (long long)i;
    z[o] = zz;
    logL[o] = LL;
    logLobs[o] = Lo;
    sigma[o] = sg;
    field[o] = f;
    keep[o] = kept ? 1 : 0;
}

// blk, count, hist: as lf_mock_hist_err, of one piece; kept: [nrf] the candidates that pass the cut
__global__ __launch_bounds__(MOCK_THREADS) void lf_mock_hist_cut(MockConst mc, MockNoise mn, MockCut ct, int nrf,
                                                                 const long long* __restrict__ blk, const long long* __restrict__ count,
                                                                 const long long* __restrict__ row_ids, unsigned long long seed,
                                                                 const double* __restrict__ cdfL, const double* __restrict__ cdfZ,
                                                                 int nbins, const double* __restrict__ edges,
                                                                 unsigned long long* __restrict__ hist,
                                                                 unsigned long long* __restrict__ kept) {
    __shared__ double le[MOCK_MAX_BINS + 2];
    __shared__ unsigned int lh[MOCK_MAX_BINS + 2];
    __shared__ double lx[MOCK_MAX_NODES], ls[MOCK_MAX_NODES];
    __shared__ unsigned int lk;
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
    if (threadIdx.x == 0) lk = 0u;
    __syncthreads();
    const unsigned long long rid = (unsigned long long)row_ids[row];
    const long long first = (b - blk[rf]) * MOCK_HIST_CHUNK, n = count[rf];
    unsigned int mine = 0u;
    for (int s = 0; s < MOCK_HIST_ITEMS; ++s) {
        const long long i = first + (long long)s * MOCK_THREADS + threadIdx.x;
        if (i >= n) break;
        double zz, LL, Lo, sg;
        if (!mock_cut_candidate(mc, ct, mn.ld2n, lx, ls, M, rf, f, rid, (unsigned int)i, seed, cdfL, cdfZ, zz, LL, Lo, sg)) continue;
        int lo = 0, hi = ne;                        // number of edges <= Lo
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (le[mid] <= Lo) lo = mid + 1; else hi = mid;
        }
        atomicAdd(&lh[lo], 1u);
        ++mine;
    }
    if (mine) atomicAdd(&lk, mine);
    __syncthreads();
    for (int i = threadIdx.x; i < ns; i += MOCK_THREADS)
        if (lh[i]) atomicAdd(&hist[(size_t)rf * ns + i], (unsigned long long)lh[i]);
    if (threadIdx.x == 0 && lk) atomicAdd(&kept[rf], (unsigned long long)lk);
}

}  // namespace lf
