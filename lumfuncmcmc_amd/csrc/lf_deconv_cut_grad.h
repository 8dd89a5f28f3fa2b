// lf_deconv_cut_grad.h - the gradient of Delta B, the change of the expected counts under a cut on the OBSERVED flux
// (lf_deconv_cut.h; DESIGN.md sections 3.31, 3.33), with respect to a row's own theta elements, for a batch of rows.
//
// u does not depend on theta, so with the host tables of lf_deconv_cut.h (c_n: the weights of MINUS Delta B)
//     -Delta B = sum_n I_n,   I_n = c_n phi_theta(L_n[, z_j]) [fc^(1/d)_theta(L_n - ld2_j): FREE],
// and the derivatives are piece B's lattice derivatives (lf_grad.h: lf_grad_part's lattice branch) with c_n in the place of
// W om0: with x = L_n - L*, t = 10^x, c1 = alpha + 1
//     d(-Delta B) / d L*      = ln10 sum_n I_n (t - c1)
//     d(-Delta B) / d phi*    = ln10 sum_n I_n                  (phi* does not cancel here, unlike in Delta)
//     d(-Delta B) / d alpha   = ln10 sum_n I_n x
//     d(-Delta B) / d Flim_f  = sum_{n of field f} I_n dF_n / Flim_f,   d / d alpha_C = sum_n I_n dC_n      (FREE only)
// z-evolving: the L_m and phi_m elements are the L* and phi* terms times the Lagrange basis l_m(z_j).  The running sums are
// those of lf_grad_part's lattice blocks.  lf_grad_final subtracts them (lnprob = A - B); here lnprob_cut = lnprob + Delta -
// Delta B and c holds the weights of MINUS Delta B, so the second stage adds them.
//
// lf_deconv_cut_grad_part   lf_deconv_cut_part's grid (cut chunks, rows), chunk table, node order and block tail: 256 threads,
//                           thread t takes nodes t, t + 256, ... of its chunk in that order, cgrad_slots<V>() running sums;
//                           block_sum -> cgpart[row][chunk][GRAD_SLOTS].  A node whose I is 0 or NaN adds exactly 0 to every
//                           slot.  A row whose lnprob is not finite: the block returns.
// lf_deconv_cut_grad_final  one wave per row, lf_grad_final's arrangement (final_nan_row, grad_elem, final_lane_sum: lane l
//                           adds chunks l, l + 64, ... in that order, the Flim_f element its field's chunks only, then the
//                           shuffle tree; scale: ln10, 1 / Flim_f, 1 for alpha_C).  alone = 0: grad[e] += scale x sum, on top
//                           of the plain and the Delta gradient already there.  alone = 1 (lf_cut_term_grad_batch): out =
//                           Delta B by lf_deconv_cut_final's statements over the value's slots, grad[e] = 0 - scale x sum,
//                           the gradient of Delta B itself; NaN for a row whose lnprob is not finite.
// No atomics; nothing in either order depends on the batch: a row's bits are the same at any B and any position.
// Slots: FREE, FIXCOMP {L*, phi*, alpha, Flim_f, alpha_C} (FIXCOMP: the first three);  ZEVOL {L1, L2, L3, phi1, phi2, phi3, alpha}.
#pragma once

#include <hip/hip_runtime.h>

#include "lf_deconv_cut.h"
#include "lf_grad.h"
#include "lf_layout.h"
#include "lf_math.h"

namespace lf {

template <int V>
constexpr int cgrad_slots() { return V == LF_FREE ? 5 : (V == LF_FIXCOMP ? 3 : 7); }      // the slots a variant sums
template <int V>
constexpr int cgrad_lds_bytes() { return 4 * cgrad_slots<V>() * 8; }                      // the four waves' totals

struct DeconvCutGradArgs {
    DeconvCutArgs d;             // lf_deconv_cut_part's (part, out: read and written by the second stage with alone = 1)
    double* cgpart;              // [rows][nch][GRAD_SLOTS]
    double* grad;                // [rows][ndim]
    int alone;                   // 0: add the gradient of -Delta B to grad; 1: out = Delta B, grad = its gradient
};

template <int V>
__global__ __launch_bounds__(BLOCK) void lf_deconv_cut_grad_part(DeconvCutGradArgs ga) {
    constexpr int NS = cgrad_slots<V>();
    __shared__ double red[4][NS];
    const DeconvCutArgs& a = ga.d;
    const int b = blockIdx.y, blk = blockIdx.x, tid = threadIdx.x;
    if (!isfinite(a.lnprob[b])) return;
    const GradConst& gc = a.gc;
    const int f = a.chunk_field[blk];
    const GradRow r = grad_row<V>(gc, a.theta + (size_t)b * gc.ndim, V == LF_FREE ? f : 0);
    const double c1 = r.al + 1.0;
    GradPiv pv{};
    GradCompRow cr{};
    double Q = 0.0;
    if (V == LF_ZEVOL) pv = grad_piv(gc);
    else Q = exp(LF_LN10 * (LF_LREF - r.L[0]));
    if (V == LF_FREE) cr = grad_comp_row(r, gc.kappa);
    const int first = a.chunk_start[blk], len = a.chunk_len[blk];
    double acc[NS];
#pragma unroll
    for (int j = 0; j < NS; ++j) acc[j] = 0.0;
    for (int i = tid; i < len; i += BLOCK) {
        const int g = first + i;
        // (I: deconv_cut_term's statements, with x, t and the completeness' derivatives kept)
        if (V == LF_ZEVOL) {
            double l[3];
            const double x = a.L[g] - zevol_Lstar(r, pv, a.a3[g], l);
            const double t = exp(LF_LN10 * x);
            const double phz = fma(l[2], r.ph[2], fma(l[1], r.ph[1], l[0] * r.ph[0]));
            const double I = a.c[g] * (LF_LN10 * exp(fma(LF_LN10, fma(x, c1, phz), -t)));
            if (!(fabs(I) > 0.0)) continue;       // (0 or NaN: exactly nothing, as piece B's nodes)
            const double wl = I * (t - c1);
#pragma unroll
            for (int m = 0; m < 3; ++m) {
                acc[m] = fma(l[m], wl, acc[m]);
                acc[3 + m] = fma(l[m], I, acc[3 + m]);
            }
            acc[6] = fma(I, x, acc[6]);
        } else {
            const double x = a.L[g] - r.L[0];
            const double t = a.P[g] * Q;
            GradComp cp{0.0, 0.0, 0.0};
            if (V == LF_FREE) cp = comp_form<true>(cr.aC, cr.aC_ln, cr.kc2, (a.a3[g] - LF_FREF) - cr.lF, a.a4[g] * cr.vs);
            const double I = a.c[g] * (LF_LN10 * exp(fma(LF_LN10, fma(x, c1, r.ph[0]), -t) + cp.l));
            if (!(fabs(I) > 0.0)) continue;
            acc[1] += I;
            acc[0] = fma(I, t - c1, acc[0]);
            acc[2] = fma(I, x, acc[2]);
            if (V == LF_FREE) {
                acc[3] = fma(I, cp.dF, acc[3]);
                acc[4] = fma(I, cp.dC, acc[4]);
            }
        }
    }
    block_sum(acc, red, ga.cgpart + ((size_t)b * a.nch + blk) * GRAD_SLOTS);
}

// grid (rows), 64 threads
template <int V>
__global__ __launch_bounds__(64) void lf_deconv_cut_grad_final(DeconvCutGradArgs ga) {
    const DeconvCutArgs& a = ga.d;
    const int b = blockIdx.x, lane = threadIdx.x;
    const GradConst& gc = a.gc;
    double* out = ga.grad + (size_t)b * gc.ndim;
    if (final_nan_row(a.lnprob[b], out, gc.ndim)) {
        if (ga.alone && lane == 0) a.out[b] = __builtin_nan("");
        return;
    }
    if (ga.alone) {                               // (lf_deconv_cut_final's statements)
        const double* part = a.part + (size_t)b * a.stride;
        double s = 0.0;
        for (int c = lane; c < a.nch; c += 64) s += part[c];
        s = wave_sum(s);
        if (lane == 0) a.out[b] = 0.0 - s;
    }
    const double* th = a.theta + (size_t)b * gc.ndim;
    const double* part = ga.cgpart + (size_t)b * a.nch * GRAD_SLOTS;
    for (int e = 0; e < gc.ndim; ++e) {
        const GradElem el = grad_elem<V>(gc, th, e);
        const int slot = el.kind;                 // (the slots are in the elements' order)
        const double sm = wave_sum(final_lane_sum<GRAD_SLOTS>(part + slot, a.nch, el.fld, [&](int c) { return a.chunk_field[c]; }));
        if (lane != 0) continue;
        if (ga.alone) out[e] = 0.0 - el.scale * sm;           // (no nodes: +0)
        else out[e] += el.scale * sm;
    }
}

}  // namespace lf
