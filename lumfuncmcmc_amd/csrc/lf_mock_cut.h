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

// lf_mock.h's mock_loggam and mock_poisson, statement for statement, for the band's count.  Copies, not calls: with a second
// caller the compiler no longer inlines mock_poisson into lf_mock_total, whose code would change; f carries MOCK_CUT_BAND.
__device__ inline double mock_cut_loggam(double x) {
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

__device__ inline long long mock_cut_poisson(double mu, unsigned long long row_id, int f, unsigned long long seed) {
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
        if ((log(V) + log(invalpha) - log(a / (us * us) + b)) <= (-mu + (double)k * loglam - mock_cut_loggam((double)(k + 1))))
            return k;
    }
}

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
    count[rf] = mock_cut_poisson(mean[rf], (unsigned long long)row_ids[row], f | (int)MOCK_CUT_BAND, seed);
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
