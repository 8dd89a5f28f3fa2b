// lf_deconv_grad.h - the gradient of the flux-error-convolved likelihood's correction Delta (lf_deconv.h)
// with respect to a row's own theta elements, for a batch of rows; added to the plain gradient (lf_grad.h) it is the gradient
// of lnprob_err.
//
// For source i with sigma_i > 0 the node exponents are lf_deconv.h's,
//     a_ik = ln(w_k / sqrt(pi)) + ln10 (alpha + 1) delta_ik - t_i em_ik + l(f_i E_ik) - l(f_i),
//     delta_ik = sqrt(2) sigma_i x_k,  em = expm1(ln10 delta),  E = em + 1,  t_i = 10^(L_i - L*),   Delta_i = ln sum_k e^(a_ik),
// and with p_ik = e^(a_ik) / sum_k e^(a_ik)
//     d Delta_i / d L*      = ln10 t_i sum_k p_ik em_ik            (z-evolving: times the Lagrange basis l_m(z_i) for L_m)
//     d Delta_i / d alpha   = ln10 sum_k p_ik delta_ik             (absent when the slope is fixed)
//     d Delta_i / d phi*    = 0 exactly                            (phi* cancels in a_ik)
//     d Delta_i / d Flim_f  = [sum_k p_ik dF(f_i E_ik) - dF(f_i)] / Flim_f         (FREE only; f the field of i)
//     d Delta_i / d alpha_C =  sum_k p_ik dC(f_i E_ik) - dC(f_i)                   (FREE only)
// dF, dC: grad_comp's (lf_grad.h), taken at (y, v) as the nodes have them.  The sums over k are one online softmax: the running
// maximum m, the sum s and one weighted numerator per quantity (delta, em; FREE: dF, dC); a node that raises the maximum
// rescales s and every numerator by the same e^(-|d|); a node whose exponent is -inf is skipped (p = 0).  A source with
// sigma_i = 0 adds exactly 0 to every element.
//
// lf_deconv_grad_part   grid (blocks, rows), 256 threads; the chunk table is lf_deconv_part's (chunks of up to DECONV_CH sources
//                       of one field).  The node table goes to LDS; the row's constants are scalars.  Thread t takes sources
//                       t, t + 256, ... of its chunk in that order, DGRAD_SLOTS running sums; then the wave's 64 lanes by the
//                       shuffle tree of wave_sum, the four waves' totals through LDS as ((w0 + w1) + w2) + w3 ->
//                       part[row][block][DGRAD_SLOTS].  A block returns at once when the row's lnprob is not finite.
// lf_deconv_grad_final  one wave per row: per element, lane l adds blocks l, l + 64, ... in that order (the Flim_f element:
//                       its field's blocks only), then the shuffle tree; grad[e] += scale x sum (ln10 for L and alpha,
//                       1 / Flim_f, 1 for alpha_C) on top of the plain gradient already there.  NaN in every element when
//                       lnprob is not finite.
// No atomics; nothing in either order depends on the batch: a row's gradient has the same bits at any B and any position.
// Slots: FREE {L*, alpha, Flim_f, alpha_C};  FIXCOMP {L*, alpha};  ZEVOL {L1, L2, L3, alpha}.
#pragma once

#include <hip/hip_runtime.h>

#include "lf_deconv.h"
#include "lf_grad.h"
#include "lf_layout.h"
#include "lf_math.h"

namespace lf {

constexpr int DGRAD_SLOTS = 4;                                   // the stride of `part`
template <int V>
constexpr int dgrad_slots() { return V == LF_FIXCOMP ? 2 : 4; }  // the slots a variant fills
template <int V>
constexpr int dgrad_lds_bytes() { return (2 * DECONV_KMAX + 4 * dgrad_slots<V>()) * 8; }   // the node table, the four waves' totals

struct DeconvGradArgs {
    DeconvArgs d;                // lf_deconv_part's (part, out: not used here)
    double* gpart;               // [rows][nch][DGRAD_SLOTS]
    double* grad;                // [rows][ndim]: the plain gradient on entry, the convolved one on return
};

// grad_comp (lf_grad.h) at y = log10(f / Flim), v = f / f_tau: l has deconv_lcomp's bits
__device__ __forceinline__ GradComp dgrad_comp(double aC, double aC_ln, double kc2, double y, double v) {
    const double num = aC * y;
    const double den = sqrt(fma(num, num, 1.0));
    const double e = exp(-v);
    const double d = -expm1(-v);
    double lnfc, gp;
    if (num < 0.0) {
        const double s = den - num;
        lnfc = -log(2.0 * den * s);
        gp = s / (den * den);
    } else {
        const double s = den + num;
        lnfc = log1p(-0.5 / (den * s));
        gp = 1.0 / (den * den * s);
    }
    GradComp c;
    c.l = lnfc / d;
    const double lw = e > 0.0 ? c.l * (v * e / d) : 0.0;
    c.dF = lw - gp * aC_ln / d;
    c.dC = fma(lw, kc2, gp * y / d);
    return c;
}

template <int V>
__global__ __launch_bounds__(BLOCK) void lf_deconv_grad_part(DeconvGradArgs ga) {
    constexpr int NS = dgrad_slots<V>();
    __shared__ double nd[2 * DECONV_KMAX];
    __shared__ double red[4][NS];
    const DeconvArgs& a = ga.d;
    const int b = blockIdx.y, blk = blockIdx.x, tid = threadIdx.x;
    if (!isfinite(a.lnprob[b])) return;           // (the whole block: lf_deconv_grad_final does not read `gpart` then)
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
    const double aC_ln = aC / LF_LN10, kc2 = LF_LN10 * gc.kappa / (aC * aC);
    const double Q = V == LF_ZEVOL ? 0.0 : exp(LF_LN10 * (LF_LREF - r.L[0]));
    GradPiv pv{};
    if (V == LF_ZEVOL) pv = grad_piv(gc);
    const int first = a.chunk_start[blk], len = a.chunk_len[blk];
    double acc[NS];
#pragma unroll
    for (int j = 0; j < NS; ++j) acc[j] = 0.0;
    for (int i = tid; i < len; i += BLOCK) {
        const int g = first + i;
        const double sg = a.sigma[g];
        if (!(sg > 0.0)) continue;
        double t;
        double lb[3] = {0.0, 0.0, 0.0};
        if (V == LF_ZEVOL) {
            grad_basis(pv, a.a1[g], lb);
            const double Lz = fma(lb[2], r.L[2], fma(lb[1], r.L[1], lb[0] * r.L[0]));
            t = exp(LF_LN10 * (a.lum[g] - Lz));
        } else {
            t = a.P[g] * Q;
        }
        const double y0 = (a.logf[g] - LF_FREF) - lF;
        const double v0 = a.U[g] * vs;
        GradComp c0{0.0, 0.0, 0.0};
        if (V == LF_FREE) c0 = dgrad_comp(aC, aC_ln, kc2, y0, v0);
        else c0.l = deconv_lcomp(aC, y0, v0);
        const double s2 = 1.41421356237309504880 * sg;
        double m = -HUGE_VAL, s = 0.0, nD = 0.0, nE = 0.0, nF = 0.0, nC = 0.0;
        for (int k = 0; k < K; ++k) {
            const double dl = s2 * nd[k];
            const double em = expm1(LF_LN10 * dl);
            GradComp ck{0.0, 0.0, 0.0};
            if (V == LF_FREE) ck = dgrad_comp(aC, aC_ln, kc2, y0 + dl, v0 * (em + 1.0));
            else ck.l = deconv_lcomp(aC, y0 + dl, v0 * (em + 1.0));
            const double av = nd[K + k] + ((c1l * dl - t * em) + (ck.l - c0.l));
            if (av == -HUGE_VAL) continue;
            const double d = av - m;
            const double e = exp(-fabs(d));
            if (d > 0.0) {
                s = fma(s, e, 1.0);
                nD = fma(nD, e, dl);
                nE = fma(nE, e, em);
                if (V == LF_FREE) nF = fma(nF, e, ck.dF), nC = fma(nC, e, ck.dC);
                m = av;
            } else {
                s += e;
                nD = fma(e, dl, nD);
                nE = fma(e, em, nE);
                if (V == LF_FREE) nF = fma(e, ck.dF, nF), nC = fma(e, ck.dC, nC);
            }
        }
        const double gL = t * (nE / s);
        if (V == LF_ZEVOL) {
#pragma unroll
            for (int q = 0; q < 3; ++q) acc[q] += lb[q] * gL;
            acc[3] += nD / s;
        } else {
            acc[0] += gL;
            acc[1] += nD / s;
            if (V == LF_FREE) {
                acc[2] += nF / s - c0.dF;
                acc[3] += nC / s - c0.dC;
            }
        }
    }
    const int lane = tid & 63, wv = tid >> 6;
#pragma unroll
    for (int j = 0; j < NS; ++j) {
        const double ws = wave_sum(acc[j]);
        if (lane == 0) red[wv][j] = ws;
    }
    __syncthreads();
    if (tid < NS) ga.gpart[((size_t)b * a.nch + blk) * DGRAD_SLOTS + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
}

// grid (rows), 64 threads
template <int V>
__global__ __launch_bounds__(64) void lf_deconv_grad_final(DeconvGradArgs ga) {
    const DeconvArgs& a = ga.d;
    const int b = blockIdx.x, lane = threadIdx.x;
    const GradConst& gc = a.gc;
    double* out = ga.grad + (size_t)b * gc.ndim;
    if (!isfinite(a.lnprob[b])) {
        if (lane < gc.ndim) out[lane] = __builtin_nan("");
        return;
    }
    const double* th = a.theta + (size_t)b * gc.ndim;
    const double* part = ga.gpart + (size_t)b * a.nch * DGRAD_SLOTS;
    const int kF = gc.fix_sch_al ? 2 : 3;         // FREE: theta index of Flim_0
    for (int e = 0; e < gc.ndim; ++e) {
        int slot = -1, fld = -1;
        double scale = LF_LN10;
        if (V == LF_ZEVOL) {
            if (e < 3) slot = e;
            else if (e == 6) slot = 3;
        } else {
            if (e == 0) slot = 0;
            else if (e == 1) slot = -1;
            else if (!gc.fix_sch_al && e == 2) slot = 1;
            else if (V == LF_FREE && e < kF + gc.nf) slot = 2, fld = e - kF, scale = 1.0 / th[e];
            else if (V == LF_FREE) slot = 3, scale = 1.0;
        }
        if (slot < 0) continue;                   // (phi*: the correction does not depend on it - the plain element stays)
        double sm = 0.0;
        for (int c = lane; c < a.nch; c += 64)
            if (fld < 0 || a.chunk_field[c] == fld) sm += part[(size_t)c * DGRAD_SLOTS + slot];
        sm = wave_sum(sm);
        if (lane == 0) out[e] += scale * sm;
    }
}

}  // namespace lf
