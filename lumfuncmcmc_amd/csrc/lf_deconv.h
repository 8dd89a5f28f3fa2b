// lf_deconv.h - the flux-error-convolved likelihood (Eddington-bias correction) for a batch of rows.
//
// The catalogued log-luminosity of source i is its true one plus Gaussian noise of sigma_i dex, and the completeness acts on
// the TRUE flux, so the noise integrates out of the expected counts: piece B stays, and each per-source term of piece A,
// t_i = ln[phi(L_i) Omega(L_i, z_i)], becomes ln of its convolution with N(0, sigma_i^2).  By K-point Gauss-Hermite
// quadrature (nodes x_k, weights w_k), written as a correction to the plain value:
//     lnprob_err = lnprob + Delta,   Delta = sum_i Delta_i,   Delta_i = ln sum_k (w_k / sqrt(pi)) exp(t_ik - t_i),
//     delta = sqrt(2) sigma_i x_k,   E = 10^delta = 1 + expm1(ln10 delta),
//     t_ik - t_i = ln10 (alpha + 1) delta - 10^(L_i - L*) (E - 1) + l(f_i E) - l(f_i),
// L* = L*(z_i) for the z-evolving model (phi* cancels), l = ln fc^(1/d) in lf_grad.h's form without cancellation - FREE: the
// row's Flim_f and alpha_C; FIXCOMP, ZEVOL: the fixed ones the model was built with (the ratio does not depend on the row
// then, but it is evaluated here all the same: no table of N x K values).  The inner sum is a log-sum-exp with a running
// maximum (ratios of e^(+-hundreds) occur for faint sources at large sigma): one exponential per node.  A node whose term is
// -inf adds exactly 0; a source with sigma_i = 0 is skipped and adds exactly 0.
//
// lf_deconv_part   grid (blocks, rows), 256 threads.  Block c: chunk c of up to DECONV_CH sources of one field (the
//                  context's per-source arrays plus sigma; FIXCOMP, ZEVOL: plus the sources' log flux and 10^(log flux + 17)).
//                  The node table {x_k}, {ln(w_k / sqrt(pi))} is copied to LDS; the row's constants are scalars.  Thread t
//                  takes sources t, t + 256, ... of its chunk in that order; then the wave's 64 lanes by the shuffle tree of
//                  wave_sum, the four waves' totals through LDS as ((w0 + w1) + w2) + w3 -> part[row][block].
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

// l = ln fc^(1/d) at y = log10(f / Flim), v = f / f_tau (grad_comp's value, without its derivatives)
__device__ __forceinline__ double deconv_lcomp(double aC, double y, double v) {
    const double num = aC * y;
    const double den = sqrt(fma(num, num, 1.0));
    const double d = -expm1(-v);
    double lnfc;
    if (num < 0.0) lnfc = -log(2.0 * den * (den - num));
    else lnfc = log1p(-0.5 / (den * (den + num)));
    return lnfc / d;
}

template <int V>
__global__ __launch_bounds__(BLOCK) void lf_deconv_part(DeconvArgs a) {
    __shared__ double nd[2 * DECONV_KMAX];
    __shared__ double red[4];
    const int b = blockIdx.y, blk = blockIdx.x, tid = threadIdx.x;
    if (!isfinite(a.lnprob[b])) return;           // (the whole block: lf_deconv_final does not read `part` then)
    const int K = a.dc.K;
    if (tid < 2 * K) nd[tid] = a.nodes[tid];
    __syncthreads();
    const GradConst& gc = a.gc;
    const int f = a.chunk_field[blk];
    const GradRow r = grad_row<V>(gc, a.theta + (size_t)b * gc.ndim, V == LF_FREE ? f : 0);
    const double c1l = LF_LN10 * (r.al + 1.0);
    const double flim = V == LF_FREE ? r.flim : a.dc.flim0[f];
    const double aC = V == LF_FREE ? r.aC : a.dc.alpha0;
    const double lF = log10(flim);
    const double vs = exp(LF_LN10 * gc.kappa / aC) / flim;
    const double Q = V == LF_ZEVOL ? 0.0 : exp(LF_LN10 * (LF_LREF - r.L[0]));
    GradPiv pv{};
    if (V == LF_ZEVOL) pv = grad_piv(gc);
    const int first = a.chunk_start[blk], len = a.chunk_len[blk];
    double acc = 0.0;
    for (int i = tid; i < len; i += BLOCK) {
        const int g = first + i;
        const double sg = a.sigma[g];
        if (!(sg > 0.0)) continue;
        double t;
        if (V == LF_ZEVOL) {
            double l[3];
            grad_basis(pv, a.a1[g], l);
            const double Lz = fma(l[2], r.L[2], fma(l[1], r.L[1], l[0] * r.L[0]));
            t = exp(LF_LN10 * (a.lum[g] - Lz));
        } else {
            t = a.P[g] * Q;
        }
        const double y0 = (a.logf[g] - LF_FREF) - lF;
        const double v0 = a.U[g] * vs;
        const double l0 = deconv_lcomp(aC, y0, v0);
        const double s2 = 1.41421356237309504880 * sg;
        double m = -HUGE_VAL, s = 0.0;
        for (int k = 0; k < K; ++k) {
            const double dl = s2 * nd[k];
            const double em = expm1(LF_LN10 * dl);
            const double av = nd[K + k] + ((c1l * dl - t * em) + (deconv_lcomp(aC, y0 + dl, v0 * (em + 1.0)) - l0));
            if (av == -HUGE_VAL) continue;
            const double d = av - m;
            const double e = exp(-fabs(d));
            if (d > 0.0) {
                s = fma(s, e, 1.0);
                m = av;
            } else {
                s += e;
            }
        }
        acc += m + log(s);
    }
    const int lane = tid & 63, wv = tid >> 6;
    const double ws = wave_sum(acc);
    if (lane == 0) red[wv] = ws;
    __syncthreads();
    if (tid == 0) a.part[(size_t)b * a.nch + blk] = ((red[0] + red[1]) + red[2]) + red[3];
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
