// lf_deconv.h - the flux-error-convolved likelihood (Eddington-bias correction) for a batch of rows.
//
// The catalogued log-luminosity of source i is its true one plus Gaussian noise of sigma_i dex, and the completeness acts on
// the TRUE flux, so the noise integrates out of the expected counts: piece B stays, and each per-source term of piece A,
// t_i = ln[phi(L_i) Omega(L_i, z_i)], becomes ln of its convolution with N(0, sigma_i^2).  By K-point Gauss-Hermite
// quadrature (nodes x_k, weights w_k), written as a correction to the plain value:
//     lnprob_err = lnprob + Delta,   Delta = sum_i Delta_i,   Delta_i = ln sum_k (w_k / sqrt(pi)) exp(t_ik - t_i),
//     delta = sqrt(2) sigma_i x_k,   E = 10^delta = 1 + expm1(ln10 delta),
//     t_ik - t_i = ln10 (alpha + 1) delta - 10^(L_i - L*) (E - 1) + l(f_i E) - l(f_i),
// L* = L*(z_i) for the z-evolving model (phi* cancels), l = ln fc^(1/d) by lf_grad.h's comp_form<false> - FREE: the
// row's Flim_f and alpha_C; FIXCOMP, ZEVOL: the fixed ones the model was built with (the ratio does not depend on the row
// then, but it is evaluated here all the same: no table of N x K values).  The inner sum is a log-sum-exp with a running
// maximum (ratios of e^(+-hundreds) occur for faint sources at large sigma): one exponential per node.  A node whose term is
// -inf adds exactly 0; a source with sigma_i = 0 is skipped and adds exactly 0.
//
// lf_deconv_part   grid (blocks, rows), 256 threads.  Block c: chunk c of up to DECONV_CH sources of one field (the
//                  context's per-source arrays plus sigma; FIXCOMP, ZEVOL: plus the sources' log flux and 10^(log flux + 17)).
//                  The node table {x_k}, {ln(w_k / sqrt(pi))} is copied to LDS; the row's constants are scalars.  Thread t
//                  takes sources t, t + 256, ... of its chunk in that order (deconv_items, the loop of lf_deconv_grad_part
//                  too; a source's nodes: deconv_source, lf_deconv_wide.h's too); then the block's tail (block_sum, lf_math.h) -> part[row][block].
// lf_deconv_final  one wave per row: lane l adds blocks l, l + 64, ... in that order, then the shuffle tree; out = lnprob +
//                  Delta.  A row whose lnprob is -inf stays -inf; NaN becomes -inf.
// No atomics; nothing in either order depends on the batch: a row's value has the same bits at any B and any position.
#pragma once

#include <hip/hip_runtime.h>

#include "lf_grad.h"
#include "lf_layout.h"
#include "lf_math.h"

namespace lf {

constexpr int DECONV_LDS_BYTES = (2 * DECONV_KMAX + 4) * 8;      // the node table and the four waves' totals

struct DeconvArgs {
    GradConst gc;
    DeconvConst dc;
    const double* theta;         // [rows][ndim]
    const double* lnprob;        // [rows]: what the lnprob path gave for these rows
    double* part;                // [rows][nch]
    double* out;                 // [rows]
    // per-source arrays (FREE, FIXCOMP: lum, -, 10^(lum - 42); ZEVOL: lum, z, -), log flux, 10^(log flux + 17), sigma
    const double *lum, *a1, *P, *logf, *U, *sigma;
    const double* nodes;         // [2 K]: x_k, then ln(w_k / sqrt(pi))
    const int *chunk_start, *chunk_len, *chunk_field;
    int nch;
};

// l alone at (y, v): comp_form's DERIV = false instantiation under the name the probe and its tests know
__device__ __forceinline__ double deconv_lcomp(double aC, double y, double v) { return comp_form<false>(aC, 0.0, 0.0, y, v).l; }

// what a block's items share: the row's theta and what the node exponents take from it and from the block's field
struct DeconvRow {
    GradRow r;
    double c1l, Q;               // ln10 (alpha + 1); 10^(42 - L*) (FREE, FIXCOMP)
    double aC, lF, vs;           // the completeness in force: alpha_C, log10 Flim, 10^(kappa / alpha_C) / Flim
    double aC_ln, kc2;           // grad_comp_row's (the gradient only)
    GradPiv pv;                  // ZEVOL
};
template <int V>
__device__ __forceinline__ DeconvRow deconv_row(const DeconvArgs& a, int b, int f) {
    const GradConst& gc = a.gc;
    DeconvRow w{};
    w.r = grad_row<V>(gc, a.theta + (size_t)b * gc.ndim, V == LF_FREE ? f : 0);
    w.c1l = LF_LN10 * (w.r.al + 1.0);
    const double flim = V == LF_FREE ? w.r.flim : a.dc.flim0[f];
    w.aC = V == LF_FREE ? w.r.aC : a.dc.alpha0;
    w.lF = log10(flim);
    w.vs = exp(LF_LN10 * gc.kappa / w.aC) / flim;
    w.aC_ln = w.aC / LF_LN10, w.kc2 = LF_LN10 * gc.kappa / (w.aC * w.aC);
    w.Q = V == LF_ZEVOL ? 0.0 : exp(LF_LN10 * (LF_LREF - w.r.L[0]));
    if (V == LF_ZEVOL) w.pv = grad_piv(gc);
    return w;
}
// t = 10^(L - L*) of source g; ZEVOL: L* at its z, and lb the Lagrange basis there (else lb stays as it is)
template <int V>
__device__ __forceinline__ double deconv_t(const DeconvArgs& a, const DeconvRow& w, int g, double (&lb)[3]) {
    if (V == LF_ZEVOL) return exp(LF_LN10 * (a.lum[g] - zevol_Lstar(w.r, w.pv, a.a1[g], lb)));
    return a.P[g] * w.Q;
}

// One source of both part kernels and of lf_deconv_wide.h's: source g of the arrays in `a` (sigma sg > 0) against the K nodes
// {x_k}, {ln of the whole weight} at nd[0 .. 2K), added to the thread's NS running sums.  GRAD false: acc[0] += Delta_i.
// GRAD true: the numerators of lf_deconv_grad.h ride the same online softmax, acc = that header's slots; m and s, and so
// Delta_i, take the same steps either way.
template <int V, bool GRAD, int NS>
__device__ __forceinline__ void deconv_source(const DeconvArgs& a, const DeconvRow& w, int g, double sg, int K, const double* nd,
                                              double (&acc)[NS]) {
    constexpr bool DERIV = GRAD && V == LF_FREE;  // dF, dC: of a completeness that is the row's own
    double lb[3] = {0.0, 0.0, 0.0};
    const double t = deconv_t<V>(a, w, g, lb);
    const double y0 = (a.logf[g] - LF_FREF) - w.lF;
    const double v0 = a.U[g] * w.vs;
    const GradComp c0 = comp_form<DERIV>(w.aC, w.aC_ln, w.kc2, y0, v0);
    const double s2 = 1.41421356237309504880 * sg;
    double m = -HUGE_VAL, s = 0.0, nD = 0.0, nE = 0.0, nF = 0.0, nC = 0.0;
    for (int k = 0; k < K; ++k) {
        const double dl = s2 * nd[k];
        const double em = expm1(LF_LN10 * dl);
        const GradComp ck = comp_form<DERIV>(w.aC, w.aC_ln, w.kc2, y0 + dl, v0 * (em + 1.0));
        const double av = nd[K + k] + ((w.c1l * dl - t * em) + (ck.l - c0.l));
        if (av == -HUGE_VAL) continue;
        const double d = av - m;
        const double e = exp(-fabs(d));
        if (d > 0.0) {
            s = fma(s, e, 1.0);
            if (GRAD) nD = fma(nD, e, dl), nE = fma(nE, e, em);
            if (DERIV) nF = fma(nF, e, ck.dF), nC = fma(nC, e, ck.dC);
            m = av;
        } else {
            s += e;
            if (GRAD) nD = fma(e, dl, nD), nE = fma(e, em, nE);
            if (DERIV) nF = fma(e, ck.dF, nF), nC = fma(e, ck.dC, nC);
        }
    }
    if constexpr (!GRAD) {
        acc[0] += m + log(s);
    } else if constexpr (V == LF_ZEVOL) {
        const double gL = t * (nE / s);
#pragma unroll
        for (int q = 0; q < 3; ++q) acc[q] += lb[q] * gL;
        acc[3] += nD / s;
    } else {
        acc[0] += t * (nE / s);
        acc[1] += nD / s;
        if constexpr (DERIV) {
            acc[2] += nF / s - c0.dF;
            acc[3] += nC / s - c0.dC;
        }
    }
}

// The item loop of both part kernels: block (blockIdx.x, row blockIdx.y) takes its chunk's sources as the header says and
// leaves each thread's NS running sums in acc (deconv_source).  nd: LDS for the node table.  False when the row's lnprob is
// not finite: the whole block returns then, before any barrier (the rows' second stages do not read the partial sums of such a
// row).
template <int V, bool GRAD, int NS>
__device__ __forceinline__ bool deconv_items(const DeconvArgs& a, double* nd, double (&acc)[NS]) {
    const int b = blockIdx.y, blk = blockIdx.x, tid = threadIdx.x;
    if (!isfinite(a.lnprob[b])) return false;
    const int K = a.dc.K;
    if (tid < 2 * K) nd[tid] = a.nodes[tid];
    __syncthreads();
    const DeconvRow w = deconv_row<V>(a, b, a.chunk_field[blk]);
    const int first = a.chunk_start[blk], len = a.chunk_len[blk];
#pragma unroll
    for (int j = 0; j < NS; ++j) acc[j] = 0.0;
    for (int i = tid; i < len; i += BLOCK) {
        const int g = first + i;
        const double sg = a.sigma[g];
        if (!(sg > 0.0)) continue;
        deconv_source<V, GRAD>(a, w, g, sg, K, nd, acc);
    }
    return true;
}

template <int V>
__global__ __launch_bounds__(BLOCK) void lf_deconv_part(DeconvArgs a) {
    __shared__ double nd[2 * DECONV_KMAX];
    __shared__ double red[4][1];
    double acc[1];
    if (!deconv_items<V, false>(a, nd, acc)) return;
    const int b = blockIdx.y, blk = blockIdx.x;
    block_sum(acc, red, a.part + (size_t)b * a.nch + blk);
}

// grid (rows), 64 threads
__global__ __launch_bounds__(64) void lf_deconv_final(DeconvArgs a) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const double lp = a.lnprob[b];
    if (!isfinite(lp)) {
        if (lane == 0) a.out[b] = lp != lp ? -HUGE_VAL : lp;
        return;
    }
    const double* part = a.part + (size_t)b * a.nch;
    double s = 0.0;
    for (int c = lane; c < a.nch; c += 64) s += part[c];
    s = wave_sum(s);
    if (lane == 0) {
        const double v = lp + s;
        a.out[b] = v != v ? -HUGE_VAL : v;
    }
}

}  // namespace lf
