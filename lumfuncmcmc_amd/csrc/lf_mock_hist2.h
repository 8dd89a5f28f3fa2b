// lf_mock_hist2.h - the mock catalogues binned in redshift and luminosity on the device (lf_mock_hist2, lf_mock_hist2_err,
// lf_mock_hist2_cut, include/lfmcmc.h).  lf_mock_hist, lf_mock_hist_err and lf_mock_hist_cut draw every
// source's redshift and drop it; this header bins the pair (z, L) of the same sources, L being logL of the plain process,
// logL_obs of the noisy one and logL_obs of the kept candidates of the cut process.  Redshift carries no noise.
//
// The sources.  Nothing is drawn here: the kernel calls lf_mock.h's mock_owner and mock_source, lf_mock_noise.h's
// mock_logflux, mock_sigma, mock_noise and mock_observe and lf_mock_cut.h's mock_cut_candidate with the arguments
// lf_mock_hist, lf_mock_hist_err and lf_mock_hist_cut give them (the sigma row and the nodes in LDS, ld2n and the cut's edge
// through global loads), so the Philox purposes, the statements and their `fp contract(off)` are those headers' own and a
// source binned here is the source lf_mock_draw, lf_mock_draw_err or lf_mock_draw_cut writes, bit for bit.
//
// Slots.  sz = number of z_edges <= z (searchsorted(z_edges, z, side="right"), 0 .. nz + 1), sl = number of edges <= L
// (0 .. nl + 1); hist[rf][sz][sl], [nrf][nz + 2][nl + 2] 64-bit counts.  Summed over sz it is lf_mock_hist's histogram.
//
// Work.  lf_mock_hist's: a workgroup of 256 takes up to MOCK_HIST_CHUNK sources of one (row, field), thread t the sources
// first + s 256 + t, bins them into a tile of 32-bit counters in LDS with LDS atomics, and then adds the tile's non-zero
// counters to HBM with 64-bit integer atomics.  A counter holds at most MOCK_HIST_CHUNK < 2^32.  Integer addition is
// associative and commutative, so neither the order of the LDS atomics within a workgroup nor the order in which the
// workgroups (and, in the cut process, the two pieces' launches) reach HBM can change a count: two calls give the same bits.
//
// The tile.  Row sz of the tile starts at word sz * ls, ls = (nl + 2) | 1: the rows keep the output's order (L fastest), so the
// flush walks the output linearly and neighbouring lanes add to neighbouring HBM words, and the row stride is odd.
//   - LDS atomics go to bank (word mod 32) and lanes of one half-wave that meet on a bank take turns.  A luminosity function
//     is steep: most sources of a wave fall into the few lowest luminosity slots and spread over redshift.  With a stride that
//     is a multiple of 32 (nl + 2 = 32, 64, 128: natural choices) every redshift row would put those slots on the same few
//     banks; an odd stride walks the rows through all 32.  Lanes that share a slot share an address and are serialised by
//     the hardware whatever the layout: at worst 64 turns per wave-instruction, one LDS cycle per source, against the
//     source's own two Philox blocks, two bisections through global memory and two square roots.  Private copies of the tile
//     per wave would remove that cycle and multiply the zeroing and the flush by the number of copies; they are not worth it.
//   - Flush.  Only the (nz + 2)(nl + 2) words in use are zeroed and read back, 256 consecutive words per step (conflict
//     free), and only non-zero counters reach HBM: a workgroup issues at most min(slots, MOCK_HIST_CHUNK) global atomics.  A
//     sparse tile costs its LDS sweep (at most 32 reads per thread) and nothing in HBM.
// Limits, set by static LDS: nz and nl in 1 .. MOCK_MAX_BINS each (the edge arrays of lf_mock_hist, one per axis) and
// (nz + 2)(nl + 2) <= MOCK_HIST2_MAX_SLOTS = 8192.  The padded tile then needs at most 8192 + (nz + 2) <= 9216 words (the
// padding is largest for the longest redshift axis, 1024 rows of 8 slots): MOCK_HIST2_TILE_WORDS.  Static LDS:
//     counters 9216 x 4 = 36864 B, the two edge arrays 2 x 1024 x 8 = 16384 B                       plain   53248 B
//     + lf_mock_hist_err's nodes and sigma row, 2 x 64 x 8 = 1024 B                                   noisy   54272 B
//     + one counter of kept candidates (8 B with its alignment)                                       cut     54280 B
// under the 64 KiB a kernel may declare statically, and three workgroups fit a CU's 160 KiB (two are what DESIGN.md section
// 3.35 relies on; registers allow more).
//
// Kernel (256 threads, no scratch): lf_mock_hist2<P>, P = MOCK_HIST2_PLAIN, _NOISY, _CUT; the cut process launches it once per
// piece, as lf_mock_hist_cut is launched.
#pragma once
#include "lf_mock.h"
#include "lf_mock_noise.h"
#include "lf_mock_cut.h"

namespace lf {

constexpr int MOCK_HIST2_MAX_SLOTS = 8192;              // (nz + 2)(nl + 2)
constexpr int MOCK_HIST2_TILE_WORDS = 9216;             // the tile with its odd row stride, see the file comment
constexpr int MOCK_HIST2_PLAIN = 0, MOCK_HIST2_NOISY = 1, MOCK_HIST2_CUT = 2;

// number of entries of v[0 .. n) that are <= x (v non-decreasing)
__device__ __forceinline__ int mock_slot(const double* __restrict__ v, int n, double x) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (v[mid] <= x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// blk, count, row_ids, cdfL, cdfZ: as lf_mock_hist (of one piece in the cut process); mn: read for P != PLAIN; ct, kept: read
// for P == CUT (kept: [nrf] the candidates that pass the cut); hist: [nrf][nz + 2][nl + 2]
template <int P>
__global__ __launch_bounds__(MOCK_THREADS) void lf_mock_hist2(MockConst mc, MockNoise mn, MockCut ct, int nrf,
                                                              const long long* __restrict__ blk, const long long* __restrict__ count,
                                                              const long long* __restrict__ row_ids, unsigned long long seed,
                                                              const double* __restrict__ cdfL, const double* __restrict__ cdfZ, int nz,
                                                              const double* __restrict__ z_edges, int nl,
                                                              const double* __restrict__ edges, unsigned long long* __restrict__ hist,
                                                              unsigned long long* __restrict__ kept) {
    __shared__ unsigned int lh[MOCK_HIST2_TILE_WORDS];
    __shared__ double lze[MOCK_MAX_BINS + 2];
    __shared__ double le[MOCK_MAX_BINS + 2];
    __shared__ double lx[MOCK_MAX_NODES], ls[MOCK_MAX_NODES];      // (P == PLAIN touches neither these nor lk: they take no LDS)
    __shared__ unsigned int lk[1];
    const long long b = blockIdx.x;
    const int rf = mock_owner(blk, nrf, b);
    const int row = rf / mc.nf, f = rf - row * mc.nf;
    const int nze = nz + 1, nle = nl + 1, nzs = nz + 2, nls = nl + 2, stride = nls | 1;
    for (int i = threadIdx.x; i < nze; i += MOCK_THREADS) lze[i] = z_edges[i];
    for (int i = threadIdx.x; i < nle; i += MOCK_THREADS) le[i] = edges[i];
    for (int i = threadIdx.x; i < nzs * stride; i += MOCK_THREADS) lh[i] = 0u;
    if constexpr (P != MOCK_HIST2_PLAIN) {
        if ((int)threadIdx.x < mn.M) {
            lx[threadIdx.x] = mn.nodes[threadIdx.x];
            ls[threadIdx.x] = mn.sigma[(size_t)f * mn.M + threadIdx.x];
        }
    }
    if constexpr (P == MOCK_HIST2_CUT) {
        if (threadIdx.x == 0) lk[0] = 0u;
    }
    __syncthreads();
    const unsigned long long rid = (unsigned long long)row_ids[row];
    const long long first = (b - blk[rf]) * MOCK_HIST_CHUNK, n = count[rf];
    unsigned int mine = 0u;
    for (int s = 0; s < MOCK_HIST_ITEMS; ++s) {
        const long long i = first + (long long)s * MOCK_THREADS + threadIdx.x;
        if (i >= n) break;
        double zz, LL, Lb;
        if constexpr (P == MOCK_HIST2_PLAIN) {
            mock_source(mc, rf, f, rid, (unsigned int)i, seed, cdfL, cdfZ, zz, LL);
            Lb = LL;
        } else if constexpr (P == MOCK_HIST2_NOISY) {
            mock_source(mc, rf, f, rid, (unsigned int)i, seed, cdfL, cdfZ, zz, LL);
            const double t = mock_logflux(mc.zarr, mn.ld2n, mc.S, zz, LL);
            const double sg = mock_sigma(lx, ls, mn.M, t);
            Lb = mock_observe(LL, sg, mock_noise(rid, (unsigned int)i, f, seed));
        } else {
            double sg;
            if (!mock_cut_candidate(mc, ct, mn.ld2n, lx, ls, mn.M, rf, f, rid, (unsigned int)i, seed, cdfL, cdfZ, zz, LL, Lb, sg)) continue;
            ++mine;
        }
        const int sz = mock_slot(lze, nze, zz), sl = mock_slot(le, nle, Lb);
        atomicAdd(&lh[sz * stride + sl], 1u);
    }
    if constexpr (P == MOCK_HIST2_CUT) {
        if (mine) atomicAdd(&lk[0], mine);
    }
    __syncthreads();
    unsigned long long* out = hist + (size_t)rf * nzs * nls;
    for (int i = threadIdx.x; i < nzs * nls; i += MOCK_THREADS) {
        const int sz = i / nls, sl = i - sz * nls;
        const unsigned int c = lh[sz * stride + sl];
        if (c) atomicAdd(&out[i], (unsigned long long)c);
    }
    if constexpr (P == MOCK_HIST2_CUT) {
        if (threadIdx.x == 0 && lk[0]) atomicAdd(&kept[rf], (unsigned long long)lk[0]);
    }
}

}  // namespace lf
