// lf_lumpost.h - per-source posterior of the TRUE luminosity under the flux-error-convolved model (lf_deconv.h), marginalised
// over a batch of posterior rows.
//
// For source i (sigma_i > 0) and row r the posterior of delta = true - catalogued log-luminosity is the reweighting of the
// nodes delta_k = sqrt(2) sigma_i x_k that deconv_source walks, p_k = exp(av_k) / sum_j exp(av_j) with av_k that routine's
// exponent.  Its moments
//     e1_ir = sum_k p_k delta_k,   e2_ir = sum_k p_k delta_k^2       (dex, dex^2)
// ride the same online softmax as two more numerators (lumpost_source), and over the R' rows whose plain lnprob is finite
//     m1_i = (1 / R') sum_r e1_ir,   m2_i = (1 / R') sum_r e2_ir.
//
// lf_lumpost_part  grid (narrow chunks + wide chunks, tiles of the group), 256 threads.  Block (c, j): chunk c - of the table
//                  lf_deconv_part takes (c < n0: up to DECONV_CH sources, the Gauss-Hermite table) or behind them of the wide
//                  list's (up to DECONV_WIDE_CH sources of one class, that class's table) - and the LUMPOST_RT rows of tile j
//                  of the launch's group.  The node table and the tile's row constants (deconv_row, once per block and row)
//                  go to LDS.  Thread t owns sources t, t + 256, ... of the chunk: per source it walks the tile's live rows in
//                  row order, the two running sums in registers, and stores them to slab j at the source's slot (a narrow
//                  source: its place in the context's order; a wide one: N + its place in the wide list).  A tile without a
//                  live row stores 0, 0; a source whose sigma is not > 0 is skipped and its slots are never read.
// lf_lumpost_fold  one thread per slot, after each group: sum += slab 0, slab 1, ... in tile order, by load / add / store
//                  into the slot's running pair; after the last group instead  m = sum / R'  (NaN when R' = 0) to m1, m2 at
//                  the source's place in the CALLER's order (caller[slot]: the permutation the context keeps).
// The order is fixed - rows in row order inside a tile, tiles in tile order, then one division - and free of atomics: two calls
// on the same inputs give the same bits, and an R = 1 call gives exactly that row's e1 and e2 (0 + x and x / 1 are exact).
// Nothing is shared between the rows of a tile but the node table: every (source, row) pair takes deconv_source's steps.
#pragma once

#include <hip/hip_runtime.h>

#include "lf_deconv.h"
#include "lf_deconv_wide.h"
#include "lf_layout.h"

namespace lf {

// the node table of the largest wide class and the tile's row constants
constexpr int LUMPOST_LDS_BYTES = DECONV_WIDE_TABLE_BYTES + LUMPOST_RT * (int)sizeof(DeconvRow);

struct LumPostArgs {
    DeconvArgs d;                // lf_deconv_part's: the narrow chunks (part, out: not used)
    DeconvWideArgs w;            // lf_deconv_wide_part's: the wide chunks (w.d.part, w.d.out: not used)
    int n0, nw;                  // narrow chunks, wide chunks
    int N, nslots;               // sources of the context; slots: N + sources of the wide list
    double* slab;                // [LUMPOST_SLABS][2][nslots]: a tile's sums of e1, then of e2
    double* run;                 // [2][nslots]: the running sums over the groups so far
    const int* caller;           // [nslots]: the slot's source in the caller's order
    double *m1, *m2;             // [N], caller's order; zeroed before the first launch (a source with sigma = 0 keeps 0)
};

// deconv_source's loop (lf_deconv.h: the same exponent in the same association, the same steps for m and s) with the numerators
// of delta and delta^2 beside s: e1 = E_p[delta], e2 = E_p[delta^2] of source g against row constants w
template <int V>
__device__ __forceinline__ void lumpost_source(const DeconvArgs& a, const DeconvRow& w, int g, double sg, int K, const double* nd,
                                               double& e1, double& e2) {
    double lb[3] = {0.0, 0.0, 0.0};
    const double t = deconv_t<V>(a, w, g, lb);
    const double y0 = (a.logf[g] - LF_FREF) - w.lF;
    const double v0 = a.U[g] * w.vs;
    const GradComp c0 = comp_form<false>(w.aC, w.aC_ln, w.kc2, y0, v0);
    const double s2 = 1.41421356237309504880 * sg;
    double m = -HUGE_VAL, s = 0.0, nD = 0.0, nQ = 0.0;
    for (int k = 0; k < K; ++k) {
        const double dl = s2 * nd[k];
        const double em = expm1(LF_LN10 * dl);
        const GradComp ck = comp_form<false>(w.aC, w.aC_ln, w.kc2, y0 + dl, v0 * (em + 1.0));
        const double av = nd[K + k] + ((w.c1l * dl - t * em) + (ck.l - c0.l));
        if (av == -HUGE_VAL) continue;
        const double d = av - m;
        const double e = exp(-fabs(d));
        const double dq = dl * dl;
        if (d > 0.0) {
            s = fma(s, e, 1.0);
            nD = fma(nD, e, dl), nQ = fma(nQ, e, dq);
            m = av;
        } else {
            s += e;
            nD = fma(e, dl, nD), nQ = fma(e, dq, nQ);
        }
    }
    e1 = nD / s, e2 = nQ / s;
}

// row0: the first row of the launch's group; nrows: the rows of the call
template <int V>
__global__ __launch_bounds__(BLOCK) void lf_lumpost_part(LumPostArgs x, int row0, int nrows) {
    __shared__ double nd[2 * DECONV_WIDE_KMAX];
    __shared__ DeconvRow rw[LUMPOST_RT];
    const int blk = blockIdx.x, tile = blockIdx.y, tid = threadIdx.x;
    const bool wide = blk >= x.n0;
    const DeconvArgs& a = wide ? x.w.d : x.d;
    const int cb = wide ? blk - x.n0 : blk;
    const int r0 = row0 + tile * LUMPOST_RT;
    unsigned live = 0;
#pragma unroll
    for (int r = 0; r < LUMPOST_RT; ++r)
        if (r0 + r < nrows && isfinite(a.lnprob[r0 + r])) live |= 1u << r;
    const int first = a.chunk_start[cb], len = a.chunk_len[cb];
    double* s1 = x.slab + (size_t)tile * 2 * x.nslots + (wide ? x.N : 0) + first;
    double* s2 = s1 + x.nslots;
    if (!live) {
        for (int i = tid; i < len; i += BLOCK)
            if (a.sigma[first + i] > 0.0) s1[i] = 0.0, s2[i] = 0.0;
        return;
    }
    int K = a.dc.K;
    const double* tab = a.nodes;
    if (wide) {
        const int cls = x.w.chunk_class[cb];
        K = x.w.K[cls];
        tab = x.w.tables + x.w.off[cls];
    }
    for (int i = tid; i < 2 * K; i += BLOCK) nd[i] = tab[i];
    if (tid < LUMPOST_RT && (live >> tid & 1u)) rw[tid] = deconv_row<V>(a, r0 + tid, a.chunk_field[cb]);
    __syncthreads();
    for (int i = tid; i < len; i += BLOCK) {
        const int g = first + i;
        const double sg = a.sigma[g];
        if (!(sg > 0.0)) continue;
        double a1 = 0.0, a2 = 0.0;
        for (int r = 0; r < LUMPOST_RT; ++r) {
            if (!(live >> r & 1u)) continue;
            double e1, e2;
            lumpost_source<V>(a, rw[r], g, sg, K, nd, e1, e2);
            a1 += e1, a2 += e2;
        }
        s1[i] = a1, s2[i] = a2;
    }
}

// grid (ceil(nslots / 256)), 256 threads.  ntiles: the slabs the group's launch filled; first / last: the call's first / last
// group; n_used: R'
__global__ __launch_bounds__(BLOCK) void lf_lumpost_fold(LumPostArgs x, int ntiles, int first, int last, int n_used) {
    const int slot = blockIdx.x * BLOCK + threadIdx.x;
    if (slot >= x.nslots) return;
    const double sg = slot < x.N ? x.d.sigma[slot] : x.w.d.sigma[slot - x.N];
    if (!(sg > 0.0)) return;
    double a1 = first ? 0.0 : x.run[slot], a2 = first ? 0.0 : x.run[x.nslots + slot];
    for (int j = 0; j < ntiles; ++j) {
        const double* s = x.slab + (size_t)j * 2 * x.nslots + slot;
        a1 += s[0], a2 += s[x.nslots];
    }
    if (!last) {
        x.run[slot] = a1, x.run[x.nslots + slot] = a2;
        return;
    }
    const int i = x.caller[slot];
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    x.m1[i] = n_used > 0 ? a1 / (double)n_used : nan;
    x.m2[i] = n_used > 0 ? a2 / (double)n_used : nan;
}

}  // namespace lf
