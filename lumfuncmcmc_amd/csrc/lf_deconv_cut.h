// lf_deconv_cut.h - the convolved likelihood under a cut on the OBSERVED flux: the change of the
// expected counts, piece B, when the catalogue keeps a source whose catalogued luminosity L_o = L_t + eps lies at or above the
// integration grid's lower edge Lam_f(z).  More sources scatter up across the edge than down:
//     Delta B = sum_f sum_j wz_j V_j [ int_{Lam - H}^{Lam} phi Omega Q(-u) dL - int_{Lam}^{min(Lam + H, Lh)} phi Omega Q(u) dL ],
//     u = (L - Lam_fj) / s_f(L - ld2_j),   Q(x) = erfc(x / sqrt 2) / 2,   lnprob_cut = lnprob + Delta - Delta B.
// u does not depend on theta (the edge is fixed at the constructor's completeness, the error model is fixed), so the nodes
// L_n of a composite Gauss-Legendre rule on both sides of the edge and the whole weight
//     c_n = -/+ wz_j V_j (GL weight) Q(|u_n|) Omega_0f [fc^(1/d) at the node: FIXCOMP, ZEVOL]
// are host tables (lf_hostprep.h: cut_tables, in extended precision; the weights of MINUS Delta B), and the device evaluates
//     -Delta B = sum_n c_n phi_theta(L_n[, z_j]) [fc^(1/d)_theta(L_n - ld2_j): FREE]
// with piece B's node forms (lf_grad.h: lf_grad_part's lattice branch, comp_form) - no erfc here.
//
// lf_deconv_cut_part  grid (chunks, rows), 256 threads.  Block c: chunk c of up to DECONV_CUT_CH nodes of one field.  Thread t
//                     takes nodes t, t + 256, ... of its chunk in that order; then the block's tail (block_sum, lf_math.h):
//                     the wave's 64 lanes by the shuffle tree, the four waves' totals through LDS as ((w0 + w1) + w2) + w3
//                     -> part[row][block], slots behind the narrow and wide blocks' of lf_deconv.h, which lf_deconv_final
//                     adds with them, unchanged.  A row whose lnprob is not finite: the block returns (its slots are not read).
// lf_deconv_cut_final lf_cut_term_batch's second stage, one wave per row: lane l adds the row's cut slots l, l + 64, ... in that
//                     order, the shuffle tree; out = Delta B = -(sum); NaN for a row whose lnprob is not finite.
// No atomics; nothing in either order depends on the batch: a row's value has the same bits at any B and any position.
#pragma once

#include <hip/hip_runtime.h>

#include "lf_grad.h"
#include "lf_layout.h"
#include "lf_math.h"

namespace lf {

struct DeconvCutArgs {
    GradConst gc;
    const double* theta;         // [rows][ndim]
    const double* lnprob;        // [rows]: what the lnprob path gave for these rows
    double* part;                // [rows][stride], advanced to the cut blocks' first slot
    double* out;                 // [rows] (lf_deconv_cut_final)
    const double *L, *P, *c, *a3, *a4;      // the nodes (lf_hostprep.h: CutTables)
    const int *chunk_start, *chunk_len, *chunk_field;
    int stride;                  // slots of a row
    int nch;                     // cut chunks
};

// c_n phi Omega of node g: piece B's node form with the weight c in the place of W om0
template <int V>
__device__ __forceinline__ double deconv_cut_term(const DeconvCutArgs& a, const GradRow& r, const GradPiv& pv, const GradCompRow& cr,
                                                  double c1, double Q, int g) {
    if (V == LF_ZEVOL) {
        double l[3];
        const double x = a.L[g] - zevol_Lstar(r, pv, a.a3[g], l);
        const double t = exp(LF_LN10 * x);
        const double phz = fma(l[2], r.ph[2], fma(l[1], r.ph[1], l[0] * r.ph[0]));
        return a.c[g] * (LF_LN10 * exp(fma(LF_LN10, fma(x, c1, phz), -t)));
    }
    const double x = a.L[g] - r.L[0];
    const double t = a.P[g] * Q;
    double lc = 0.0;
    if (V == LF_FREE) lc = comp_form<false>(cr.aC, 0.0, 0.0, (a.a3[g] - LF_FREF) - cr.lF, a.a4[g] * cr.vs).l;
    return a.c[g] * (LF_LN10 * exp(fma(LF_LN10, fma(x, c1, r.ph[0]), -t) + lc));
}

template <int V>
__global__ __launch_bounds__(BLOCK) void lf_deconv_cut_part(DeconvCutArgs a) {
    __shared__ double red[4][1];
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
    double acc[1] = {0.0};
    for (int i = tid; i < len; i += BLOCK) {
        const double I = deconv_cut_term<V>(a, r, pv, cr, c1, Q, first + i);
        if (!(fabs(I) > 0.0)) continue;           // (0 or NaN: exactly nothing, as piece B's nodes)
        acc[0] += I;
    }
    block_sum(acc, red, a.part + (size_t)b * a.stride + blk);
}

// grid (rows), 64 threads
__global__ __launch_bounds__(64) void lf_deconv_cut_final(DeconvCutArgs a) {
    const int b = blockIdx.x, lane = threadIdx.x;
    if (!isfinite(a.lnprob[b])) {
        if (lane == 0) a.out[b] = __builtin_nan("");
        return;
    }
    const double* part = a.part + (size_t)b * a.stride;
    double s = 0.0;
    for (int c = lane; c < a.nch; c += 64) s += part[c];
    s = wave_sum(s);
    if (lane == 0) a.out[b] = 0.0 - s;            // (no nodes: +0)
}

}  // namespace lf
