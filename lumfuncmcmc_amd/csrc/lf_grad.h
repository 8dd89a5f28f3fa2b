// lf_grad.h - the gradient of lnprob = A - B (the two pieces of lf_lnprob_pieces) with respect to a row's own theta elements,
// for a batch of rows.  The function differentiated is the oracle's: piece_a, piece_b, fleming with the
// decay (fcmin truthy), schechter_z.  Units are theta's own (Flim in 1e-17).
//
// With x = lum - L*, t = 10^x, c1 = alpha + 1 a Schechter term has
//     d ln tlf / d L* = ln10 (t - c1),   d / d phi* = ln10,   d / d alpha = ln10 x;
// z-evolving: L*(z) = sum_m l_m(z) L_m, phi*(z) = sum_m l_m(z) phi_m with the Lagrange basis l_m on the pivots, so the
// derivatives with respect to L_m and phi_m are the above times l_m(z).
// The completeness fc^(1/d) (modified Fleming) has ln = l = ln(fc) / d with
//     y = log10(f / F),  num = alpha_C y,  den = sqrt(1 + num^2),  fc = (1 + num / den) / 2,
//     v = f / f_tau = (f / F) 10^(kappa / alpha_C)  (kappa = sqrt|a / (1 - a)|),  d = 1 - e^(-v) = -expm1(-v),
// all in forms without cancellation:
//     num >= 0: ln fc = log1p(-1 / (2 den (den + num))),  g' = d ln fc / d num = 1 / (den^2 (den + num));
//     num <  0: ln fc = -ln(2 den (den - num)),           g' = (den - num) / den^2           (den + num = 1 / (den - num));
//     w = v e^(-v) / d  (-> 1 as v -> 0; 0 when e^(-v) is 0);
//     d l / d Flim    = (l w - g' alpha_C / (ln10 d)) / Flim,
//     d l / d alpha_C = g' y / d + l w ln10 kappa / alpha_C^2.
// Piece A sums these over the sources, piece B sums them times the integrand W om0_f tlf fc^(1/d) over the lattice's nodes
// (W: piece_b's trapezoid weights).  A node whose integrand is exactly 0 (or NaN) contributes exactly 0.  What does not depend
// on a source beyond a sum made once is closed-form: d A / d phi* = N ln10, d A / d phi_m = ln10 sum_i l_m(z_i) (GradConst::sl).
//
// lf_grad_part   grid (blocks, rows), 256 threads.  Block c < nchA: chunk c of up to GRAD_CH sources of one field (the context's
//                per-source arrays, lf_hostprep.h: catalogue); block nchA + q: field q % nfB of the lattice's nodes [q / nfB
//                GRAD_CH, + GRAD_CH) (FREE: nfB = nf; else the fields are summed in W: nfB = 1).  Thread t takes items t, t + 256,
//                ... of its chunk in that order, GRAD_SLOTS running sums; then the block's tail (block_sum, lf_math.h): the
//                wave's 64 lanes by the shuffle tree of wave_sum, the four waves' totals through LDS as ((w0 + w1) + w2) + w3
//                -> part[row][block][GRAD_SLOTS].
// lf_grad_final  one wave per row: element e = scale x ((closed form + sum of the source blocks' slot) - sum of the lattice
//                blocks' slot); lane l adds blocks l, l + 64, ... in that order (final_lane_sum; the Flim_f element: its
//                field's blocks only), then the shuffle tree; scale (grad_elem): ln10, 1 / Flim_f, 1 for alpha_C.  A row
//                whose lnprob is not finite gets NaN in every element (final_nan_row).
// The completeness form above is written once, comp_form<DERIV>; lf_deconv.h and lf_deconv_grad.h call it at their nodes, and
// lf_deconv_grad_final is made of lf_grad_final's helpers.
// No atomics; nothing in either order depends on the batch: a row's gradient has the same bits at any B and any position.
// Slots: FREE, FIXCOMP {L*, phi*, alpha, Flim_f, alpha_C};  ZEVOL {L1, L2, L3, phi1, phi2, phi3, alpha}.
#pragma once

#include <hip/hip_runtime.h>

#include "lf_layout.h"
#include "lf_math.h"

namespace lf {

constexpr int GRAD_LDS_BYTES = 4 * GRAD_SLOTS * 8;       // the four waves' totals

struct GradArgs {
    GradConst gc;
    const double* theta;         // [rows][ndim]
    const double* lnprob;        // [rows]: what the lnprob path gave for these rows
    double* part;                // [rows][nblk][GRAD_SLOTS]
    double* grad;                // [rows][ndim]
    // per-source arrays (FREE: lum, logf, 10^(lum - 42), 10^(logf + 17); FIXCOMP: lum, -, 10^(lum - 42), -; ZEVOL: lum, z, -, -)
    const double *lum, *a1, *P, *U;
    const int *chunk_start, *chunk_len, *chunk_field;
    // lattice (FREE: a3 = log flux, a4 = 10^(a3 + 17); ZEVOL: a3 = z)
    const double *G, *PG, *W, *a3, *a4;
    int nnodes, nchA, nchB, nfB;
};

// theta row, by variant
struct GradRow {
    double L[3], ph[3];          // FREE / FIXCOMP: [0] only
    double al, flim, aC;         // flim: of the block's field
};

template <int V>
__device__ __forceinline__ GradRow grad_row(const GradConst& gc, const double* __restrict__ th, int f) {
    GradRow r{};
    if (V == LF_ZEVOL) {
#pragma unroll
        for (int m = 0; m < 3; ++m) r.L[m] = th[m], r.ph[m] = th[3 + m];
        r.al = gc.fix_sch_al ? gc.sch_al0 : th[6];
    } else {
        r.L[0] = th[0], r.ph[0] = th[1];
        r.al = gc.fix_sch_al ? gc.sch_al0 : th[2];
        if (V == LF_FREE) {
            const int k = gc.fix_sch_al ? 2 : 3;
            r.flim = th[k + f];
            r.aC = th[k + gc.nf];
        }
    }
    return r;
}

// the completeness of one flux: l = ln(fc) / d and its two derivatives without their factors 1 / Flim and 1
struct GradComp {
    double l, dF, dC;
};
// y = log10(f / F), u = f / F; cst: what depends on the row only
struct GradCompRow {
    double lF, aC, vs, aC_ln, kc2;      // log10 Flim, alpha_C, 10^(kappa / alpha_C) / Flim, alpha_C / ln10, ln10 kappa / alpha_C^2
};
__device__ __forceinline__ GradCompRow grad_comp_row(const GradRow& r, double kappa) {
    GradCompRow q;
    q.lF = log10(r.flim);
    q.aC = r.aC;
    q.vs = exp(LF_LN10 * kappa / r.aC) / r.flim;
    q.aC_ln = r.aC / LF_LN10;
    q.kc2 = LF_LN10 * kappa / (r.aC * r.aC);
    return q;
}
// The one body of the form above at y = log10(f / Flim), v = f / f_tau.  DERIV false: l only (dF = dC = 0), by the same
// statements - l has the same bits either way.
template <bool DERIV>
__device__ __forceinline__ GradComp comp_form(double aC, double aC_ln, double kc2, double y, double v) {
    const double num = aC * y;
    const double den = sqrt(fma(num, num, 1.0));
    const double e = DERIV ? exp(-v) : 0.0;
    const double d = -expm1(-v);
    double lnfc, gp = 0.0;
    if (num < 0.0) {
        const double s = den - num;
        lnfc = -log(2.0 * den * s);
        if (DERIV) gp = s / (den * den);
    } else {
        const double s = den + num;
        lnfc = log1p(-0.5 / (den * s));
        if (DERIV) gp = 1.0 / (den * den * s);
    }
    GradComp c{lnfc / d, 0.0, 0.0};
    if (DERIV) {
        const double lw = e > 0.0 ? c.l * (v * e / d) : 0.0;
        c.dF = lw - gp * aC_ln / d;
        c.dC = fma(lw, kc2, gp * y / d);
    }
    return c;
}
// logf: log10 of the flux, U = 10^(logf + 17)
__device__ __forceinline__ GradComp grad_comp(const GradCompRow& q, double logf, double U) {
    return comp_form<true>(q.aC, q.aC_ln, q.kc2, (logf - LF_FREF) - q.lF, U * q.vs);
}

// the Lagrange basis on the pivots at z
struct GradPiv {
    double z1, z2, z3, i1, i2, i3;
};
__device__ __forceinline__ GradPiv grad_piv(const GradConst& gc) {
    GradPiv p;
    p.z1 = gc.pivots[0], p.z2 = gc.pivots[1], p.z3 = gc.pivots[2];
    p.i1 = 1.0 / ((p.z1 - p.z2) * (p.z1 - p.z3));
    p.i2 = 1.0 / ((p.z2 - p.z1) * (p.z2 - p.z3));
    p.i3 = 1.0 / ((p.z3 - p.z1) * (p.z3 - p.z2));
    return p;
}
__device__ __forceinline__ void grad_basis(const GradPiv& p, double z, double (&l)[3]) {
    const double a = z - p.z1, b = z - p.z2, c = z - p.z3;
    l[0] = b * c * p.i1;
    l[1] = a * c * p.i2;
    l[2] = a * b * p.i3;
}
// L*(z) of a z-evolving row, and the basis l at z it is made with
__device__ __forceinline__ double zevol_Lstar(const GradRow& r, const GradPiv& p, double z, double (&l)[3]) {
    grad_basis(p, z, l);
    return fma(l[2], r.L[2], fma(l[1], r.L[1], l[0] * r.L[0]));
}

template <int V>
__global__ __launch_bounds__(BLOCK) void lf_grad_part(GradArgs a) {
    __shared__ double red[4][GRAD_SLOTS];
    const int b = blockIdx.y, blk = blockIdx.x, tid = threadIdx.x;
    if (!isfinite(a.lnprob[b])) return;           // (the whole block: lf_grad_final writes NaN without reading `part`)
    const GradConst& gc = a.gc;
    const bool src = blk < a.nchA;
    const int q = blk - a.nchA;
    const int f = src ? a.chunk_field[blk] : q % a.nfB;
    const GradRow r = grad_row<V>(gc, a.theta + (size_t)b * gc.ndim, V == LF_FREE ? f : 0);
    const double c1 = r.al + 1.0;
    double acc[GRAD_SLOTS - 1];
#pragma unroll
    for (int j = 0; j < GRAD_SLOTS - 1; ++j) acc[j] = 0.0;

    if (V == LF_ZEVOL) {
        const GradPiv pv = grad_piv(gc);
        const int first = src ? a.chunk_start[blk] : (q / a.nfB) * GRAD_CH;
        const int len = src ? a.chunk_len[blk] : min(GRAD_CH, a.nnodes - first);
        for (int i = tid; i < len; i += BLOCK) {
            const int g = first + i;
            double l[3];
            const double x = (src ? a.lum[g] : a.G[g]) - zevol_Lstar(r, pv, src ? a.a1[g] : a.a3[g], l);
            const double t = exp(LF_LN10 * x);
            double I = 1.0;
            if (!src) {
                const double phz = fma(l[2], r.ph[2], fma(l[1], r.ph[1], l[0] * r.ph[0]));
                I = a.W[g] * (LF_LN10 * exp(fma(LF_LN10, fma(x, c1, phz), -t)));
                if (!(fabs(I) > 0.0)) continue;
            }
            const double wl = I * (t - c1);
#pragma unroll
            for (int m = 0; m < 3; ++m) {
                acc[m] = fma(l[m], wl, acc[m]);
                if (!src) acc[3 + m] = fma(l[m], I, acc[3 + m]);
            }
            acc[6] = fma(I, x, acc[6]);
        }
    } else {
        const double Q = exp(LF_LN10 * (LF_LREF - r.L[0]));
        GradCompRow cr{};
        if (V == LF_FREE) cr = grad_comp_row(r, gc.kappa);
        const int first = src ? a.chunk_start[blk] : (q / a.nfB) * GRAD_CH;
        const int len = src ? a.chunk_len[blk] : min(GRAD_CH, a.nnodes - first);
        const double om0 = V == LF_FREE ? gc.om0_grid[f] : 1.0;
        for (int i = tid; i < len; i += BLOCK) {
            const int g = first + i;
            const double x = (src ? a.lum[g] : a.G[g]) - r.L[0];
            const double t = (src ? a.P[g] : a.PG[g]) * Q;
            GradComp cp{0.0, 0.0, 0.0};
            if (V == LF_FREE) cp = grad_comp(cr, src ? a.a1[g] : a.a3[g], src ? a.U[g] : a.a4[g]);
            double I = 1.0;
            if (!src) {
                I = a.W[g] * om0 * (LF_LN10 * exp(fma(LF_LN10, fma(x, c1, r.ph[0]), -t) + cp.l));
                if (!(fabs(I) > 0.0)) continue;
                acc[1] += I;
            }
            acc[0] = fma(I, t - c1, acc[0]);
            acc[2] = fma(I, x, acc[2]);
            if (V == LF_FREE) {
                acc[3] = fma(I, cp.dF, acc[3]);
                acc[4] = fma(I, cp.dC, acc[4]);
            }
        }
    }

    block_sum(acc, red, a.part + ((size_t)b * (a.nchA + a.nchB * a.nfB) + blk) * GRAD_SLOTS);
}

// ---- what the rows' second stages share (lf_grad_final, lf_deconv_grad_final: one wave per row) ----
// A row whose lnprob is not finite: NaN in every element, and the caller returns
__device__ __forceinline__ bool final_nan_row(double lnprob, double* __restrict__ out, int ndim) {
    if (isfinite(lnprob)) return false;
    if ((int)threadIdx.x < ndim) out[threadIdx.x] = __builtin_nan("");
    return true;
}
// theta element e: what it is (FREE / FIXCOMP: 0 L*, 1 phi*, 2 alpha, 3 Flim_f, 4 alpha_C; ZEVOL: e itself - L1, L2, L3, phi1,
// phi2, phi3, alpha), the field whose blocks alone count (-1: all) and the factor of the blocks' sum (ln10; 1 / Flim_f; 1)
struct GradElem {
    int kind, fld;
    double scale;
};
template <int V>
__device__ __forceinline__ GradElem grad_elem(const GradConst& gc, const double* __restrict__ th, int e) {
    GradElem g{e, -1, LF_LN10};
    const int kF = gc.fix_sch_al ? 2 : 3;         // FREE: theta index of Flim_0
    if (V == LF_ZEVOL || e < 2) return g;
    if (!gc.fix_sch_al && e == 2) return g;
    if (V != LF_FREE) return g;                   // (FIXCOMP has no further element)
    if (e < kF + gc.nf) g.kind = 3, g.fld = e - kF, g.scale = 1.0 / th[e];
    else g.kind = 4, g.scale = 1.0;
    return g;
}
// this lane's share of the sum over n blocks of part[block LD]: blocks lane, lane + 64, ... in that order, those of field fld
// only (fld < 0: all; field_of(block): its field); wave_sum of it is the row's sum
template <int LD, class F>
__device__ __forceinline__ double final_lane_sum(const double* __restrict__ part, int n, int fld, F field_of) {
    double s = 0.0;
    for (int c = threadIdx.x; c < n; c += 64)
        if (fld < 0 || field_of(c) == fld) s += part[(size_t)c * LD];
    return s;
}

// grid (rows), 64 threads
template <int V>
__global__ __launch_bounds__(64) void lf_grad_final(GradArgs a) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const GradConst& gc = a.gc;
    double* out = a.grad + (size_t)b * gc.ndim;
    if (final_nan_row(a.lnprob[b], out, gc.ndim)) return;
    const double* th = a.theta + (size_t)b * gc.ndim;
    const int nblkB = a.nchB * a.nfB, nblk = a.nchA + nblkB;
    const double* part = a.part + (size_t)b * nblk * GRAD_SLOTS;
    for (int e = 0; e < gc.ndim; ++e) {
        const GradElem el = grad_elem<V>(gc, th, e);
        const int slot = el.kind;                 // (the slots are in the elements' order)
        double closed = 0.0;
        if (V == LF_ZEVOL) {
            if (e >= 3 && e < 6) closed = gc.sl[e - 3];
        } else if (e == 1) {
            closed = gc.nsrc;
        }
        double sA = final_lane_sum<GRAD_SLOTS>(part + slot, a.nchA, el.fld, [&](int c) { return a.chunk_field[c]; });
        double sB = final_lane_sum<GRAD_SLOTS>(part + (size_t)a.nchA * GRAD_SLOTS + slot, nblkB, el.fld, [&](int q) { return q % a.nfB; });
        sA = wave_sum(sA);
        sB = wave_sum(sB);
        if (lane == 0) out[e] = el.scale * ((closed + sA) - sB);
    }
}

}  // namespace lf
