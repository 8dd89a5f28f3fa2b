// lf_deconv_grad.h - the gradient of the flux-error-convolved likelihood's correction Delta (lf_deconv.h)
// with respect to a row's own theta elements, for a batch of rows; added to the plain gradient (lf_grad.h) it is the gradient
// of lnprob_err.
//
// For source i with sigma_i > 0 the node exponents a_ik are lf_deconv.h's (delta_ik, em_ik, E_ik, t_i as there), Delta_i =
// ln sum_k e^(a_ik), and with p_ik = e^(a_ik) / sum_k e^(a_ik)
//     d Delta_i / d L*      = ln10 t_i sum_k p_ik em_ik            (z-evolving: times the Lagrange basis l_m(z_i) for L_m)
//     d Delta_i / d alpha   = ln10 sum_k p_ik delta_ik             (absent when the slope is fixed)
//     d Delta_i / d phi*    = 0 exactly                            (phi* cancels in a_ik)
//     d Delta_i / d Flim_f  = [sum_k p_ik dF(f_i E_ik) - dF(f_i)] / Flim_f         (FREE only; f the field of i)
//     d Delta_i / d alpha_C =  sum_k p_ik dC(f_i E_ik) - dC(f_i)                   (FREE only)
// dF, dC: comp_form<true>'s (lf_grad.h), taken at (y, v) as the nodes have them.  The sums over k ride the online softmax of
// deconv_items (lf_deconv.h): next to its running maximum m and sum s, one weighted numerator per quantity (delta, em; FREE:
// dF, dC); a node that raises the maximum rescales s and every numerator by the same e^(-|d|); a node whose exponent is -inf
// is skipped (p = 0).  A source with sigma_i = 0 adds exactly 0 to every element.
//
// lf_deconv_grad_part   lf_deconv_part's grid, chunk table, item order and block tail (lf_deconv.h), with dgrad_slots<V>()
//                       running sums -> gpart[row][block][DGRAD_SLOTS].
// lf_deconv_grad_final  one wave per row, lf_grad_final's arrangement (lf_grad.h: the NaN row, the elements' fields and
//                       factors, the lanes' order over the blocks): grad[e] += factor x sum, on top of the plain gradient
//                       already there.
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

// l, dF, dC at (y, v): comp_form's DERIV = true instantiation under the name the probe and its tests know
__device__ __forceinline__ GradComp dgrad_comp(double aC, double aC_ln, double kc2, double y, double v) {
    return comp_form<true>(aC, aC_ln, kc2, y, v);
}

template <int V>
__global__ __launch_bounds__(BLOCK) void lf_deconv_grad_part(DeconvGradArgs ga) {
    constexpr int NS = dgrad_slots<V>();
    __shared__ double nd[2 * DECONV_KMAX];
    __shared__ double red[4][NS];
    double acc[NS];
    if (!deconv_items<V, true>(ga.d, nd, acc)) return;
    const int b = blockIdx.y, blk = blockIdx.x;
    block_sum(acc, red, ga.gpart + ((size_t)b * ga.d.nch + blk) * DGRAD_SLOTS);
}

// grid (rows), 64 threads
template <int V>
__global__ __launch_bounds__(64) void lf_deconv_grad_final(DeconvGradArgs ga) {
    const DeconvArgs& a = ga.d;
    const int b = blockIdx.x, lane = threadIdx.x;
    const GradConst& gc = a.gc;
    double* out = ga.grad + (size_t)b * gc.ndim;
    if (final_nan_row(a.lnprob[b], out, gc.ndim)) return;
    const double* th = a.theta + (size_t)b * gc.ndim;
    const double* part = ga.gpart + (size_t)b * a.nch * DGRAD_SLOTS;
    for (int e = 0; e < gc.ndim; ++e) {
        const GradElem el = grad_elem<V>(gc, th, e);
        int slot;                                 // (phi: the correction does not depend on it - the plain element stays)
        if (V == LF_ZEVOL) slot = e < 3 ? e : (e == 6 ? 3 : -1);
        else slot = el.kind == 1 ? -1 : (el.kind > 1 ? el.kind - 1 : 0);
        if (slot < 0) continue;
        const double sm = wave_sum(final_lane_sum<DGRAD_SLOTS>(part + slot, a.nch, el.fld, [&](int c) { return a.chunk_field[c]; }));
        if (lane == 0) out[e] += el.scale * sm;
    }
}

}  // namespace lf
