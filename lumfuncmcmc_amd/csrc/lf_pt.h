// lf_pt.h - parallel tempering around the plain evaluation (lf_ptsampler_*).
//
// T temperatures, inverse temperatures beta_0 = 1 > beta_1 > ... > beta_{T-1} > 0, W walkers each, in the two fixed halves of
// the stretch move.  The prior is a flat box (lnprob = lnlike inside, -inf outside), so the tempered target is beta * lnprob
// and no likelihood kernel changes: a half-step is
//   lf_pt_propose (T x halfW proposals, one launch) -> the plain evaluation of the T x halfW rows -> lf_pt_accept,
// and after both halves lf_pt_swap (one workgroup) exchanges walkers between neighbouring temperatures and records the
// step.  Random numbers: sampler_draw of lf_kernels.h, counter (step, half, index, stream), key = seed:
//   stream 0 / 1, index t * halfW + w: stretch factor and partner / accept uniform of walker w of the half at temperature t
//     (temperature 0 draws exactly the numbers of lf_sampler_*: with T = 1 the chain is the ensemble sampler's, bit for bit);
//   stream 2, half 0, index i * W + k: the swap between temperatures i and i - 1 - key (r0 << 32) | r1 of walker k of
//     temperature i for the pairing permutation, uniform u53(r2, r3) for the decision.
#pragma once

#include <hip/hip_runtime.h>

namespace lf {

constexpr int PT_MAXW = 4096;                 // walkers per temperature: the swap sort's LDS (32 KiB of 64-bit keys)
constexpr int PT_MAXT = 64;
constexpr int PT_SWAP_THREADS = 1024;

struct PtArgs {
    int T, W, halfW, ndim, half;
    unsigned long long step, seed;
    double a;                    // stretch scale
    const double* betas;         // [T]
    double* pos;                 // [T][W][ndim]
    double* lnl;                 // [T][W] untempered lnlike (= lnprob: the prior is flat)
    double* prop;                // [T][halfW][ndim] proposals of the active half
    double* zz;                  // [T][halfW] their stretch factors
    const double* newl;          // [T][halfW] lnlike of the proposals
    long long* nacc;             // [T][W]
};

struct PtSwapArgs {
    int T, W, ndim;
    unsigned long long step, seed;
    long long t, cap;            // chain slot of this step, chain capacity (steps)
    const double* dbeta;         // [T] beta_{i-1} - beta_i (host, in double); entry 0 unused
    double* pos;                 // [T][W][ndim]
    double* lnl;                 // [T][W]
    int* sig;                    // [T-1][W] pairing permutations (scratch of this launch)
    long long* nswap;            // [T-1] accepted swaps of the pair (i, i - 1) at i - 1
    double* chain;               // [T][W][cap][ndim]
    double* chain_lnl;           // [T][W][cap]
    double* mean_lnl;            // [T][cap]
};

// 8 lanes per walker (lf_propose's arithmetic): row r = t * halfW + w.
__global__ __launch_bounds__(64) void lf_pt_propose(PtArgs p) {
    const int gt = blockIdx.x * blockDim.x + threadIdx.x;
    const int r = gt >> 3, f = gt & 7;
    if (r >= p.T * p.halfW) return;
    const int t = r / p.halfW, w = r - t * p.halfW;
    unsigned int rr[4];
    sampler_draw(p.step, p.half, r, 0, p.seed, rr);
    const double z = stretch_z(p.a, u53(rr[0], rr[1]));
    const size_t base = (size_t)t * p.W;
    const size_t j = base + (1 - p.half) * p.halfW + (int)(((unsigned long long)rr[2] * (unsigned long long)p.halfW) >> 32);
    const size_t k = base + p.half * p.halfW + w;
    for (int i = f; i < p.ndim; i += 8)
        p.prop[(size_t)r * p.ndim + i] = stretch_point(p.pos[j * p.ndim + i], p.pos[k * p.ndim + i], z);
    if (f == 0) p.zz[r] = z;
}

// lnq = (lnz_term + beta newl) - beta oldl, in this association: at beta = 1 it is accept_walker's lnz_term + newlp - oldlp.
__global__ __launch_bounds__(64) void lf_pt_accept(PtArgs p) {
#pragma clang fp contract(off)
    const int gt = blockIdx.x * blockDim.x + threadIdx.x;
    const int r = gt >> 3, f = gt & 7;
    if (r >= p.T * p.halfW) return;
    const int t = r / p.halfW, w = r - t * p.halfW;
    const size_t k = (size_t)t * p.W + p.half * p.halfW + w;
    unsigned int rr[4];
    sampler_draw(p.step, p.half, r, 1, p.seed, rr);
    const double lnz_term = (p.ndim - 1.0) * log(p.zz[r]);
    const double logu = log(u53(rr[0], rr[1]));
    const double b = p.betas[t], newl = p.newl[r], oldl = p.lnl[k];
    const double lnq = (lnz_term + b * newl) - b * oldl;
    if (!((logu < lnq) && (newl > -__builtin_huge_val()))) return;
    for (int i = f; i < p.ndim; i += 8) p.pos[k * p.ndim + i] = p.prop[(size_t)r * p.ndim + i];
    if (f == 0) {
        p.lnl[k] = newl;
        p.nacc[k] += 1;
    }
}

// One workgroup.  1. The pairing permutations of every pair, which depend on the random numbers only: the W keys of a pair
// fill an aligned run of Wp slots (Wp = the power of two >= W, pad keys ~0 behind), as many runs as fit the 4096 slots are
// sorted at once by one bitonic network (lf_bands.h's segmented form), and every walker finds its rank by binary search in
// its run - ties broken by index, so sig is numpy's stable argsort - and writes sig[i - 1][rank] = k.  2. The swaps, pair by
// pair from the hottest down, a barrier between pairs (pair (i, i - 1) reads what pair (i + 1, i) wrote).  3. The chain's
// row of every temperature and the per-temperature mean of lnlike (one wave per temperature, fixed order).
__device__ __forceinline__ unsigned long long pt_swap_key(const PtSwapArgs& s, int i, int k) {
    unsigned int rr[4];
    sampler_draw(s.step, 0, i * s.W + k, 2, s.seed, rr);
    return ((unsigned long long)rr[0] << 32) | rr[1];
}

__global__ __launch_bounds__(PT_SWAP_THREADS) void lf_pt_swap(PtSwapArgs s) {
#pragma clang fp contract(off)
    __shared__ unsigned long long key[PT_MAXW];
    __shared__ int nacc[PT_MAXT];
    const int tid = threadIdx.x, W = s.W, T = s.T;
    int lg = 0;
    while ((1 << lg) < W) ++lg;
    const int Wp = 1 << lg, G = PT_MAXW >> lg;            // runs per pass
    if (tid < PT_MAXT) nacc[tid] = 0;
    // 1. permutations, G pairs per pass (pair i = 1 + run index)
    for (int i0 = 1; i0 < T; i0 += G) {
        const int np = min(G, T - i0);
        const int slots = np * Wp;
        for (int x = tid; x < slots; x += PT_SWAP_THREADS) {
            const int g = x >> lg, k = x & (Wp - 1);
            key[x] = k < W ? pt_swap_key(s, i0 + g, k) : ~0ull;
        }
        __syncthreads();
        for (int kk = 2; kk <= Wp; kk <<= 1) {
            for (int j = kk >> 1; j > 0; j >>= 1) {
                for (int t = tid; t < slots / 2; t += PT_SWAP_THREADS) {
                    const int x = ((t & ~(j - 1)) << 1) | (t & (j - 1));      // bit j of x is clear; partner x + j
                    const bool up = (x & kk & (Wp - 1)) == 0;
                    const unsigned long long a = key[x], b = key[x + j];
                    if ((a > b) == up) {
                        key[x] = b;
                        key[x + j] = a;
                    }
                }
                __syncthreads();
            }
        }
        for (int x = tid; x < np * W; x += PT_SWAP_THREADS) {
            const int g = x / W, k = x - g * W, i = i0 + g;
            const unsigned long long* run = key + g * Wp;
            const unsigned long long v = pt_swap_key(s, i, k);
            int lo = 0, hi = Wp;                                // first slot whose key is >= v
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (run[mid] < v) lo = mid + 1;
                else hi = mid;
            }
            int rank = lo;
            if (lo + 1 < Wp && run[lo + 1] == v)                 // an equal key (2^-64 per pair of walkers): count those before k
                for (int m = 0; m < k; ++m) rank += pt_swap_key(s, i, m) == v;
            s.sig[(size_t)(i - 1) * W + rank] = k;
        }
        __syncthreads();                                         // the keys are overwritten by the next pass
    }
    // 2. swaps, hottest pair first
    for (int i = T - 1; i >= 1; --i) {
        const double db = s.dbeta[i];
        for (int k = tid; k < W; k += PT_SWAP_THREADS) {
            const int m = s.sig[(size_t)(i - 1) * W + k];
            const size_t a = (size_t)i * W + k, b = (size_t)(i - 1) * W + m;
            unsigned int rr[4];
            sampler_draw(s.step, 0, i * W + k, 2, s.seed, rr);
            const double la = s.lnl[a], lb = s.lnl[b];
            const double d = la - lb;
            if (log(u53(rr[2], rr[3])) < db * d) {
                s.lnl[a] = lb;
                s.lnl[b] = la;
                for (int q = 0; q < s.ndim; ++q) {
                    const double xa = s.pos[a * s.ndim + q];
                    s.pos[a * s.ndim + q] = s.pos[b * s.ndim + q];
                    s.pos[b * s.ndim + q] = xa;
                }
                atomicAdd(&nacc[i - 1], 1);
            }
        }
        __syncthreads();
    }
    if (tid < T - 1) s.nswap[tid] += nacc[tid];
    // 3. the step's record
    const size_t TW = (size_t)T * W;
    for (size_t x = tid; x < TW; x += PT_SWAP_THREADS) {
        s.chain_lnl[x * s.cap + s.t] = s.lnl[x];
        for (int q = 0; q < s.ndim; ++q) s.chain[(x * s.cap + s.t) * s.ndim + q] = s.pos[x * s.ndim + q];
    }
    const int wave = tid >> 6, lane = tid & 63;
    for (int t = wave; t < T; t += PT_SWAP_THREADS / 64) {
        double acc = 0.0;
        for (int k = lane; k < W; k += 64) acc += s.lnl[(size_t)t * W + k];
        for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
        if (lane == 0) s.mean_lnl[(size_t)t * s.cap + s.t] = acc / W;
    }
}

}  // namespace lf
