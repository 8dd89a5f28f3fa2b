// lf_vefftrue.h - the deconvolved 1/Veff points: the sources' posteriors of the TRUE luminosity (lf_lumpost.h) binned in
// luminosity, per posterior row, and their percentiles over the rows (lf_veff_true of include/lfmcmc.h).
//
// For source i, row r and node k of the source's rule (the Gauss-Hermite order of lf_set_lum_err, or its wide class):
//     dl_ik = (sqrt(2) sigma_i) x_k,   L_ik = lum_i + dl_ik              (one rounded product, one rounded add: vefft_node)
//     p_irk = exp(av_k - m) / sum_j exp(av_j - m),   av_k deconv_source's exponent, m = max_j av_j
//     values[r][b] = sum_i sum_k [edges[b] <= L_ik < edges[b + 1]] p_irk exp(-l_irk) / (pref0 vol)
// l_irk = ln fc^(1/d) at the node's TRUE flux, the value comp_form<false> gives inside the node loop: exp(-l) is 1 / fc of the
// modified Fleming curve.  A source with sigma_i = 0 is one node at dl = 0 with p = 1.  A node whose exponent is -inf has p = 0.
// The product p exp(-l) is formed in ONE exponent, exp(bv_k - m) / sum with bv_k = av_k without its + l_k: for a node far below
// Flim (l of -1e3 .. -1e5) exp(av_k - m) is 0 or subnormal and exp(-l) is +inf while their product is an ordinary number
// (DESIGN.md section 3.27).
//
// lf_vefftrue_part    grid (narrow chunks + wide chunks, rows of the launch's group), 256 threads: block (c, j) takes chunk c
//                     of lf_lumpost_part's tables and row row0 + j.  The node table, the edges and one histogram per wave go
//                     to LDS.  Wave w takes the chunk's sources 64 w .. 64 w + 63, then 64 (w + 4) .., in that order.  Of a
//                     batch of 64, lane j first forms what source j's nodes share (t, y0, v0, l(f_i), lum: vefft_source);
//                     then the wave walks the batch in source order with LANES ON NODES, the source's constants handed round
//                     by __shfl: one source on 64 lanes in passes of 64 nodes (K > 32), or two sources on the two half-waves
//                     (K <= 32).  The normaliser: max and sum over the source's lanes by an xor butterfly (every lane gets the
//                     same bits).  A source's nodes ascend in L, so its lanes hold non-decreasing bin indices: a segmented
//                     inclusive scan (offsets 1, 2, .., 32; a lane adds its neighbour's sum when that neighbour has its bin)
//                     leaves a (source, bin) pair's sum in the segment's last lane, which adds it to the wave's histogram by
//                     load / add / store - one lane per bin at a time: pass after pass, the lower half-wave's source before
//                     the upper's, sources in order.  The block then stores ((w0 + w1) + w2) + w3 to partial[c][j][bin].
// lf_vefftrue_reduce  one thread per (row, bin): the chunks' partial sums in chunk order -> values[r][b], and to the row's
//                     place among the USED rows (a row is used when its plain lnprob is finite), which lf_veffdraws.h's
//                     veffd_quant reads; an unused row gets NaN.
// No atomics, one fixed order: two calls give the same bits, and a row's values do not depend on R, on its place or on the
// other rows.  partial has VEFFT_ROWS rows whatever R: the host runs groups of VEFFT_ROWS rows one after the other.
//
// LDS: static, the node table (2304 bytes) and the row's constants (176 bytes): 2480 bytes; dynamic, sized by the call's nbin
// (vefft_dyn_lds_bytes): the edges and one histogram per wave, 2016 bytes at 50 bins, 40 976 at 1024.  The registers allow
// five waves per SIMD (five workgroups per CU); LDS caps that only above 757 bins (four workgroups), and at 1024 bins three fit.
#pragma once

#include <hip/hip_runtime.h>

#include "lf_deconv.h"
#include "lf_deconv_wide.h"
#include "lf_layout.h"

namespace lf {

constexpr int VEFFT_MAXBIN = 1024;
constexpr int VEFFT_ROWS = 16;                // rows of one launch group
constexpr int VEFFT_MAX_ROWS = 4096;          // rows of a call (the quantile stage's limit)
constexpr int VEFFT_PASSES = (DECONV_WIDE_KMAX + 63) / 64;
constexpr int VEFFT_LDS_BYTES = DECONV_WIDE_TABLE_BYTES + (int)sizeof(DeconvRow);      // static
// dynamic: nbin + 1 edges, rounded up to an even count, then four histograms of nbin
constexpr int vefft_edge_slots(int nbin) { return (nbin + 2) & ~1; }
constexpr int vefft_dyn_lds_bytes(int nbin) { return (vefft_edge_slots(nbin) + 4 * nbin) * 8; }

struct VeffTrueArgs {
    DeconvArgs d;                // lf_deconv_part's: the narrow chunks (part, out: not used)
    DeconvWideArgs w;            // lf_deconv_wide_part's: the wide chunks (w.d.part, w.d.out: not used)
    int n0, nw;                  // narrow chunks, wide chunks
    const int* in_wide;          // [N]: 1 = the source stands in the wide list (its entry of d.sigma is 0, and it is no one-node source)
    const double* edges;         // [nbin + 1]
    int nbin;
    double pv;                   // pref0 vol
    double* partial;             // [n0 + nw][VEFFT_ROWS][nbin]
    double* values;              // [R][nbin]
    double* used;                // [R'][nbin]: the used rows' values, in row order
    const int* slot;             // [R]: the row's place among the used rows
};

// what lane j holds of source j of the wave's batch.  kind 0: no source, or one the chunk's rule does not take; 1: sigma = 0, one
// node; 2: the rule's K nodes
struct VeffTrueSrc {
    int kind;
    double s2, t, y0, v0, l0, lum;
};
template <int V>
__device__ __forceinline__ VeffTrueSrc vefft_source(const VeffTrueArgs& x, const DeconvArgs& a, const DeconvRow& w, bool wide, int g) {
    VeffTrueSrc s{};
    const double sg = a.sigma[g];
    s.kind = sg > 0.0 ? 2 : (wide || x.in_wide[g] ? 0 : 1);
    if (s.kind == 0) return s;
    double lb[3] = {0.0, 0.0, 0.0};
    s.t = deconv_t<V>(a, w, g, lb);
    s.y0 = (a.logf[g] - LF_FREF) - w.lF;
    s.v0 = a.U[g] * w.vs;
    s.l0 = comp_form<false>(w.aC, w.aC_ln, w.kc2, s.y0, s.v0).l;
    s.s2 = 1.41421356237309504880 * sg;
    s.lum = a.lum[g];
    return s;
}
__device__ __forceinline__ VeffTrueSrc vefft_bcast(const VeffTrueSrc& s, int j) {
    VeffTrueSrc o;
    o.kind = __shfl(s.kind, j, 64);
    o.s2 = __shfl(s.s2, j, 64), o.t = __shfl(s.t, j, 64), o.y0 = __shfl(s.y0, j, 64);
    o.v0 = __shfl(s.v0, j, 64), o.l0 = __shfl(s.l0, j, 64), o.lum = __shfl(s.lum, j, 64);
    return o;
}

// the node's offset and true luminosity: the product and the sum are rounded once each, never contracted - the bin of a node
// that falls on an edge is decided by these bits
__device__ __forceinline__ double vefft_node(double lum, double s2, double xk, double& dl) {
#pragma clang fp contract(off)
    dl = s2 * xk;
    return lum + dl;
}

// searchsorted(edges, L, side = "right") - 1: the last edge at or below L; -1 below edges[0], nbin at or above edges[nbin]
__device__ __forceinline__ int vefft_bin(const double* ed, int nbin, double L) {
    int lo = 0, hi = nbin + 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (ed[mid] <= L) lo = mid + 1;
        else hi = mid;
    }
    return lo - 1;
}

// row0: the first row of the launch's group; dynamic LDS: vefft_dyn_lds_bytes(x.nbin).  The statements: lf_vefftrue_part_body.h,
// shared with lf_vefftrue_part_cut (lf_vefftrue_cut.h)
template <int V>
__global__ __launch_bounds__(BLOCK) void lf_vefftrue_part(VeffTrueArgs x, int row0) {
    constexpr bool CUT = false;
    const double* const invg = nullptr;
    const long long wide_off = 0;
#include "lf_vefftrue_part_body.h"
}

// grid (ceil(nbin / 256), rows of the group), 256 threads
__global__ __launch_bounds__(BLOCK) void lf_vefftrue_reduce(VeffTrueArgs x, int row0) {
    const int b = blockIdx.x * BLOCK + threadIdx.x;
    const int row = row0 + blockIdx.y;
    if (b >= x.nbin) return;
    double* out = x.values + (size_t)row * (size_t)x.nbin + b;
    if (!isfinite(x.d.lnprob[row])) {
        *out = __longlong_as_double(0x7ff8000000000000ll);
        return;
    }
    const int nch = x.n0 + x.nw;
    double s = 0.0;
    for (int c = 0; c < nch; ++c) s += x.partial[((size_t)c * VEFFT_ROWS + blockIdx.y) * (size_t)x.nbin + b];
    *out = s;
    x.used[(size_t)x.slot[row] * (size_t)x.nbin + b] = s;
}

}  // namespace lf
