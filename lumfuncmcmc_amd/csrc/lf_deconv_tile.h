// lf_deconv_tile.h - the correction of the flux-error-convolved likelihood (lf_deconv.h) for a TILE of rows per block, for the
// variants whose completeness is not the row's own (FIXCOMP, ZEVOL).
//
// Of a node term  ln w_k + ((c1l delta - t_i em) + (l(f_i 10^delta) - l(f_i)))  only c1l = ln10 (alpha + 1) and t_i =
// 10^(L_i - L*) belong to the row: delta = sqrt(2) sigma_i x_k, em = expm1(ln10 delta) and the whole completeness ratio
// belong to the source and the node.  lf_deconv_part makes them again for every row; here a block takes DECONV_RT
// consecutive rows and makes them once.
//
// lf_deconv_tile   grid (chunks, tiles), 256 threads.  Block (c, tile): chunk c of the chunk table lf_deconv_part takes and
//                  rows tile * DECONV_RT ... of the launch's nrows.  A row is live when it lies below nrows and its plain
//                  lnprob is finite - the same in every thread of the block, read before any barrier; a tile without a live
//                  row returns there.  The node table and the live rows' constants (deconv_row) go to LDS.  Thread t takes
//                  sources t, t + 256, ... of the chunk in that order (lf_deconv_part's order): per source sigma_i (skipped
//                  unless > 0), y_i, v_i, l(f_i) once and t_i per live row (deconv_t); per node delta, em and the
//                  completeness ratio once, then per live row the exponent and one step of lf_deconv_part's log-sum-exp with
//                  its running maximum.  The tail is block_sum over the DECONV_RT sums; the live rows' go to
//                  part[row][chunk], a row that is not live has its slot left alone (lf_deconv_final does not read it).
// A row's operations and their order are lf_deconv_part's and take nothing from the other rows of its tile, from nrows or
// from its place in the batch: the same bits at any B and any position.  lf_deconv_final is the second stage as it is.
// No FREE instantiation: there the completeness is the row's own and only 10^delta could be shared.
// The rows' steps are unrolled (their state is in registers); a scheduling barrier after each keeps the compiler from
// interleaving eight exp or log bodies, which cost 142 to 284 registers instead of 107.
#pragma once

#include <hip/hip_runtime.h>

#include "lf_deconv.h"

namespace lf {

constexpr int DECONV_RT = 8;                                      // rows of a tile
// the node table, the rows' constants, the four waves' totals and the tile's sums
constexpr int DECONV_TILE_LDS_BYTES = 2 * DECONV_KMAX * 8 + DECONV_RT * (int)sizeof(DeconvRow) + 4 * DECONV_RT * 8 + DECONV_RT * 8;

template <int V>
__global__ __launch_bounds__(BLOCK) void lf_deconv_tile(DeconvArgs a, int nrows) {
    static_assert(V == LF_FIXCOMP || V == LF_ZEVOL, "the FREE completeness is the row's own: lf_deconv_part");
    __shared__ double nd[2 * DECONV_KMAX];
    __shared__ DeconvRow rw[DECONV_RT];
    __shared__ double red[4][DECONV_RT];
    __shared__ double tot[DECONV_RT];
    const int blk = blockIdx.x, row0 = blockIdx.y * DECONV_RT, tid = threadIdx.x;
    unsigned live = 0;
#pragma unroll
    for (int r = 0; r < DECONV_RT; ++r)
        if (row0 + r < nrows && isfinite(a.lnprob[row0 + r])) live |= 1u << r;
    if (!live) return;
    const int K = a.dc.K;
    if (tid < 2 * K) nd[tid] = a.nodes[tid];
    if (tid < DECONV_RT && (live >> tid & 1u)) rw[tid] = deconv_row<V>(a, row0 + tid, a.chunk_field[blk]);
    __syncthreads();
    // the completeness in force is the context's, the same in every row: the first live row's copy
    const DeconvRow& w0 = rw[__builtin_ctz(live)];
    const double aC = w0.aC, lF = w0.lF, vs = w0.vs;
    const int first = a.chunk_start[blk], len = a.chunk_len[blk];
    double acc[DECONV_RT];
#pragma unroll
    for (int r = 0; r < DECONV_RT; ++r) acc[r] = 0.0;
    for (int i = tid; i < len; i += BLOCK) {
        const int g = first + i;
        const double sg = a.sigma[g];
        if (!(sg > 0.0)) continue;
        const double y0 = (a.logf[g] - LF_FREF) - lF;
        const double v0 = a.U[g] * vs;
        const double l0 = comp_form<false>(aC, 0.0, 0.0, y0, v0).l;
        const double s2 = 1.41421356237309504880 * sg;
        double t[DECONV_RT], m[DECONV_RT], s[DECONV_RT];
#pragma unroll
        for (int r = 0; r < DECONV_RT; ++r) {
            double lb[3] = {0.0, 0.0, 0.0};
            t[r] = (live >> r & 1u) ? deconv_t<V>(a, rw[r], g, lb) : 0.0;
            m[r] = -HUGE_VAL, s[r] = 0.0;
            __builtin_amdgcn_sched_barrier(0);
        }
        for (int k = 0; k < K; ++k) {
            const double dl = s2 * nd[k];
            const double em = expm1(LF_LN10 * dl);
            const double dcomp = comp_form<false>(aC, 0.0, 0.0, y0 + dl, v0 * (em + 1.0)).l - l0;
            const double lw = nd[K + k];
#pragma unroll
            for (int r = 0; r < DECONV_RT; ++r) {
                if (!(live >> r & 1u)) continue;
                const double av = lw + ((rw[r].c1l * dl - t[r] * em) + dcomp);
                if (av == -HUGE_VAL) continue;
                const double d = av - m[r];
                const double e = exp(-fabs(d));
                if (d > 0.0) {
                    s[r] = fma(s[r], e, 1.0);
                    m[r] = av;
                } else {
                    s[r] += e;
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
#pragma unroll
        for (int r = 0; r < DECONV_RT; ++r)
        {
            if (live >> r & 1u) acc[r] += m[r] + log(s[r]);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    block_sum(acc, red, tot);
    if (tid < DECONV_RT && (live >> tid & 1u)) a.part[(size_t)(row0 + tid) * a.nch + blk] = tot[tid];
}

}  // namespace lf
