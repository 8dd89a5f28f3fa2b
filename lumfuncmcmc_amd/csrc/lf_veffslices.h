// lf_veffslices.h - the 1/Veff points in redshift slices with their bootstrap (lf_veff_slices of include/lfmcmc.h; DESIGN.md
// section 3.36).  The host sorts the sources that have a slice by slice (a stable counting sort): slice s is the contiguous
// segment off_s .. off_s + n_s of the sorted records, one 16-byte record (phi, bin, slice) per source.
//
//   sums[k][s][b] = sum over the draws j = 0 .. n_s - 1 of resample k of slice s of phi[idx_ksj] [bin(idx_ksj) == b]
//   idx_0sj = off_s + j                                            (k = 0: the catalogue itself)
//   idx_ksj = off_s + min(floor(u53(r0, r1) n_s), n_s - 1),        r = Philox4x32-10(counter (j, s, k, VEFFS_PURPOSE), key seed)
//           = off_s + boot_idx[k - 1][off_s + j]                   when the caller gives the indices (checked by the host)
//
// No floating-point atomics, one fixed order of summation, so the same inputs give the same bits on every call and device:
//   veffs_pack     one thread per sorted position: the record from the weights (veff_weights' phi, in the caller's order).
//   veffs_partial  grid (chunks, nboot + 1).  The host cuts every slice's draws into chunks of at most VEFFS_CHUNK draws - a
//                  compile-time constant: nothing depends on the device's CU count.  A workgroup of T lanes takes one chunk of
//                  one resample.  Lane l adds the chunk's draws l, l + T, l + 2 T, .. in that order into its own bins in LDS,
//                  acc[bin][lane] (bin-major: the lanes of a wave write consecutive doubles, 32 lanes on 64 different banks,
//                  whatever bins they hold).  VEFFS_UNROLL gathers are issued before the first of them is added.  Then the
//                  lanes are folded in a fixed tree: for st = T / 2, T / 4, .., 1: acc[b][l] += acc[b][l + st] for l < st.
//                  acc[b][0] goes to partial[k][chunk][b] by plain vector stores.
//   veffs_reduce   rows 0 .. nboot of the grid: one thread per (k, s, b) adds the partials of slice s's chunks in chunk order
//                  into sums.  The last row counts the catalogue's records per (s, b) with integer adds (LDS, then global).
//
// LDS: veffs_partial VEFFS_LDS_DOUBLES = 4096 doubles = 32768 bytes for each of its three instantiations <NB> (the most bins it
// serves: 16, 32 or 64, with T = 4096 / NB = 256, 128 or 64 lanes; the host takes the smallest NB >= nbin); veffs_reduce 4096
// counters of 4 bytes = 16384 bytes.  Five workgroups of veffs_partial share a CU's 160 KiB: VEFFS_WG_PER_CU = 5, that is 20,
// 10 or 5 waves per CU; the registers (at most 64 VGPRs) would allow eight waves per SIMD, so LDS alone sets the occupancy.
#pragma once

#include <hip/hip_runtime.h>

#include "lf_kernels.h"

namespace lf {

constexpr int VEFFS_CHUNK = 4096;             // draws per chunk
constexpr int VEFFS_MAXBIN = 64;
constexpr int VEFFS_MAXSLICE = 64;
constexpr int VEFFS_MAXBOOT = 10000;
constexpr int VEFFS_LDS_DOUBLES = 4096;       // bins x lanes of one workgroup of veffs_partial
constexpr int VEFFS_LDS_BYTES = VEFFS_LDS_DOUBLES * 8;
constexpr int VEFFS_WG_PER_CU = 5;            // 160 KiB / VEFFS_LDS_BYTES
constexpr int VEFFS_UNROLL = 4;               // gathers in flight per lane
constexpr int VEFFS_REDUCE_THREADS = 256;
constexpr int VEFFS_REDUCE_LDS_BYTES = VEFFS_MAXSLICE * VEFFS_MAXBIN * 4;
// the Philox stream word of the slices' bootstrap ("slic"): lf_veff has 0x5eed there, the mocks 0x6d6f...., the samplers 0 - 2
constexpr unsigned int VEFFS_PURPOSE = 0x736c6963u;
static_assert(VEFFS_LDS_BYTES * VEFFS_WG_PER_CU <= 160 * 1024 && VEFFS_LDS_BYTES < 64 * 1024, "LDS of veffs_partial");

struct alignas(16) VeffsRec {
    double phi;
    int bin;                     // -1: no bin
    int slice;
};
// chunk c: the draws first .. first + count of slice `slice`, whose n sources start at sorted position off
struct alignas(8) VeffsChunk {
    int slice, first, count, off, n, pad;
};

// slice_of, bin_of: the caller's, [n]; order[p]: the source at sorted position p
__global__ __launch_bounds__(256) void veffs_pack(const double* __restrict__ phi, const int* __restrict__ slice_of,
                                                  const int* __restrict__ bin_of, const int* __restrict__ order, int m, int nbin,
                                                  VeffsRec* __restrict__ rec) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= m) return;
    const int i = order[p], b = bin_of[i];
    VeffsRec r;
    r.phi = phi[i];
    r.bin = b >= 0 && b < nbin ? b : -1;
    r.slice = slice_of[i];
    rec[p] = r;
}

// boot_idx: [nboot][m] local indices or NULL; partial: [nboot + 1][nch][nbin]
template <int NB>
__global__ __launch_bounds__(VEFFS_LDS_DOUBLES / NB) void veffs_partial(const VeffsRec* __restrict__ rec, const VeffsChunk* __restrict__ chunk,
                                                                        int nch, int nbin, const long long* __restrict__ boot_idx, long long m,
                                                                        unsigned long long seed, double* __restrict__ partial) {
#pragma clang fp contract(off)
    constexpr int T = VEFFS_LDS_DOUBLES / NB;
    static_assert(T >= 64 && (T & (T - 1)) == 0 && T >= NB && VEFFS_CHUNK % (T * VEFFS_UNROLL) == 0, "lanes of veffs_partial");
    __shared__ double acc[NB * T];
    const int lane = threadIdx.x, c = blockIdx.x, k = blockIdx.y;
    const VeffsChunk ch = chunk[c];
    for (int b = 0; b < nbin; ++b) acc[b * T + lane] = 0.0;          // (the lane's own slots: no barrier before it adds to them)
    const long long* __restrict__ given = k > 0 && boot_idx ? boot_idx + (size_t)(k - 1) * (size_t)m + (size_t)ch.off : nullptr;
    const VeffsRec* __restrict__ seg = rec + ch.off;
    for (int i0 = lane; i0 < ch.count; i0 += T * VEFFS_UNROLL) {
        VeffsRec r[VEFFS_UNROLL];
#pragma unroll
        for (int u = 0; u < VEFFS_UNROLL; ++u) {
            const int i = i0 + u * T;
            r[u].phi = 0.0;
            r[u].bin = -1;
            if (i < ch.count) {
                const int j = ch.first + i;
                int idx = j;
                if (given) {
                    idx = (int)given[j];
                } else if (k > 0) {
                    unsigned int w[4];
                    philox4x32((unsigned int)j, (unsigned int)ch.slice, (unsigned int)k, VEFFS_PURPOSE, (unsigned int)seed,
                               (unsigned int)(seed >> 32), w);
                    idx = (int)(u53(w[0], w[1]) * (double)ch.n);
                    if (idx >= ch.n) idx = ch.n - 1;
                }
                r[u] = seg[idx];
            }
        }
#pragma unroll
        for (int u = 0; u < VEFFS_UNROLL; ++u)
            if (r[u].bin >= 0) acc[r[u].bin * T + lane] += r[u].phi;
    }
    __syncthreads();
    for (int st = T / 2; st >= 1; st >>= 1) {
        const int sh = __builtin_ctz(st);
        for (int e = lane; e < (nbin << sh); e += T) {
            const int at = (e >> sh) * T + (e & (st - 1));
            acc[at] += acc[at + st];
        }
        __syncthreads();
    }
    if (lane < nbin) partial[((size_t)k * (size_t)nch + (size_t)c) * (size_t)nbin + (size_t)lane] = acc[lane * T];
}

// grid (x, nres + 1), nres = nboot + 1.  c0[s] .. c0[s + 1]: the chunks of slice s.  counts: [nslice][nbin], zero on entry.
__global__ __launch_bounds__(VEFFS_REDUCE_THREADS) void veffs_reduce(const double* __restrict__ partial, const int* __restrict__ c0, int nch,
                                                                     int nslice, int nbin, int nres, const VeffsRec* __restrict__ rec, int m,
                                                                     double* __restrict__ sums, unsigned long long* __restrict__ counts) {
#pragma clang fp contract(off)
    __shared__ unsigned int h[VEFFS_MAXSLICE * VEFFS_MAXBIN];
    const int k = blockIdx.y, cells = nslice * nbin;
    if (k < nres) {
        const int e = blockIdx.x * VEFFS_REDUCE_THREADS + threadIdx.x;
        if (e >= cells) return;
        const int s = e / nbin, b = e - s * nbin;
        double t = 0.0;
        for (int c = c0[s]; c < c0[s + 1]; ++c) t += partial[((size_t)k * (size_t)nch + (size_t)c) * (size_t)nbin + (size_t)b];
        sums[(size_t)k * (size_t)cells + (size_t)e] = t;
        return;
    }
    for (int e = threadIdx.x; e < cells; e += VEFFS_REDUCE_THREADS) h[e] = 0u;
    __syncthreads();
    for (long long p = (long long)blockIdx.x * VEFFS_REDUCE_THREADS + threadIdx.x; p < m; p += (long long)gridDim.x * VEFFS_REDUCE_THREADS) {
        const VeffsRec r = rec[p];
        if (r.bin >= 0) atomicAdd(&h[r.slice * nbin + r.bin], 1u);
    }
    __syncthreads();
    for (int e = threadIdx.x; e < cells; e += VEFFS_REDUCE_THREADS)
        if (h[e]) atomicAdd(&counts[e], (unsigned long long)h[e]);
}

}  // namespace lf
