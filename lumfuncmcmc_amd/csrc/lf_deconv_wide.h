// lf_deconv_wide.h - the flux-error-convolved likelihood (lf_deconv.h) for the sources whose sigma lies above the validated
// range of the context's Gauss-Hermite order: the "wide" rule (option "deconv_wide"), value and gradient.
//
// Gauss-Hermite nodes spread with sigma while the completeness has a branch point 1 / alpha_C dex off the real axis, so no
// order up to 32 reaches 1e-7 above 0.09 dex.  A wide source is integrated by a composite rule instead: [-T, T] sigma cut into
// panels at most DECONV_WIDE_H dex wide at the upper edge of the source's sigma class, DECONV_WIDE_NPAN Gauss-Legendre nodes
// on each.  A class's table is stored in lf_deconv.h's form - x_k with delta = sqrt(2) sigma_i x_k, and the log of the whole
// weight, the Gaussian density included - so a source's nodes are taken by deconv_source, the routine of lf_deconv_part and
// lf_deconv_grad_part, with K = the class's node count.
//
// lf_set_lum_err gathers the wide sources into arrays of their own (sorted by field, then class, then the context's order),
// leaves 0 in the context's sigma array for them (the narrow kernels skip them: exactly 0) and cuts the list into chunks of up
// to DECONV_WIDE_CH sources of one field and one class: a block's node count is uniform.
//
// lf_deconv_wide_part       grid (wide chunks, rows), 256 threads.  The class's table goes to LDS; the row's constants are
//                           deconv_row's; thread t takes sources t, t + 256, ... of its chunk in that order; block_sum ->
//                           part[row][narrow chunks + chunk]: the slots behind the narrow blocks', read by lf_deconv_final in
//                           its one fixed order.
// lf_deconv_wide_grad_part  the same with the dgrad_slots<V>() sums of lf_deconv_grad.h -> gpart[row][narrow chunks + chunk][],
//                           read by lf_deconv_grad_final (the chunk's field: the combined field table).
// A row whose plain lnprob is not finite: the block returns before any barrier, as lf_deconv_part's does.
// No atomics; nothing in either order depends on the batch: a row's value has the same bits at any B and any position.
#pragma once

#include <hip/hip_runtime.h>

#include "lf_deconv.h"
#include "lf_deconv_grad.h"
#include "lf_layout.h"
#include "lf_math.h"

namespace lf {

constexpr int DECONV_WIDE_TABLE_BYTES = 2 * DECONV_WIDE_KMAX * 8;
constexpr int DECONV_WIDE_LDS_BYTES = DECONV_WIDE_TABLE_BYTES + 4 * 8;                  // the table, the four waves' totals
template <int V>
constexpr int dwide_grad_lds_bytes() { return DECONV_WIDE_TABLE_BYTES + 4 * dgrad_slots<V>() * 8; }

struct DeconvWideArgs {
    // lf_deconv_part's, with the per-source arrays and the chunk table of the WIDE list, part advanced past the narrow blocks'
    // slots (nch: all blocks of a row, narrow and wide - the stride); nodes, dc.K: not used here
    DeconvArgs d;
    const int* chunk_class;      // [wide chunks]
    const double* tables;        // per class at off[c]: x_k [K_c], then the log weights [K_c]
    int K[DECONV_WIDE_NCLASS], off[DECONV_WIDE_NCLASS];
};

struct DeconvWideGradArgs {
    DeconvWideArgs w;
    double* gpart;               // [rows][nch][DGRAD_SLOTS], advanced past the narrow blocks' slots
};

// lf_deconv.h's deconv_items for a wide chunk: the class's table to nd, then the chunk's sources
template <int V, bool GRAD, int NS>
__device__ __forceinline__ bool deconv_wide_items(const DeconvWideArgs& wa, double* nd, double (&acc)[NS]) {
    const DeconvArgs& a = wa.d;
    const int b = blockIdx.y, blk = blockIdx.x, tid = threadIdx.x;
    if (!isfinite(a.lnprob[b])) return false;
    const int cls = wa.chunk_class[blk];
    const int K = wa.K[cls];
    const double* tab = wa.tables + wa.off[cls];
    for (int i = tid; i < 2 * K; i += BLOCK) nd[i] = tab[i];
    __syncthreads();
    const DeconvRow w = deconv_row<V>(a, b, a.chunk_field[blk]);
    const int first = a.chunk_start[blk], len = a.chunk_len[blk];
#pragma unroll
    for (int j = 0; j < NS; ++j) acc[j] = 0.0;
    for (int i = tid; i < len; i += BLOCK) {
        const int g = first + i;
        deconv_source<V, GRAD>(a, w, g, a.sigma[g], K, nd, acc);
    }
    return true;
}

template <int V>
__global__ __launch_bounds__(BLOCK) void lf_deconv_wide_part(DeconvWideArgs wa) {
    __shared__ double nd[2 * DECONV_WIDE_KMAX];
    __shared__ double red[4][1];
    double acc[1];
    if (!deconv_wide_items<V, false>(wa, nd, acc)) return;
    const int b = blockIdx.y, blk = blockIdx.x;
    block_sum(acc, red, wa.d.part + (size_t)b * wa.d.nch + blk);
}

template <int V>
__global__ __launch_bounds__(BLOCK) void lf_deconv_wide_grad_part(DeconvWideGradArgs ga) {
    constexpr int NS = dgrad_slots<V>();
    __shared__ double nd[2 * DECONV_WIDE_KMAX];
    __shared__ double red[4][NS];
    double acc[NS];
    if (!deconv_wide_items<V, true>(ga.w, nd, acc)) return;
    const int b = blockIdx.y, blk = blockIdx.x;
    block_sum(acc, red, ga.gpart + ((size_t)b * ga.w.d.nch + blk) * DGRAD_SLOTS);
}

}  // namespace lf
