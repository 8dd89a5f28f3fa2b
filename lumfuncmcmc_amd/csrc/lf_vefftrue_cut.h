// lf_vefftrue_cut.h - the deconvolved 1/Veff points (lf_vefftrue.h) under the cut on the OBSERVED flux (lf_deconv_cut.h): the
// catalogued volume per node (option "deconv_cut_veff"; lf_veff_true_cut, lf_cut_volume of include/lfmcmc.h; DESIGN.md section
// 3.34).
//
// Under the cut a true luminosity L of field f is catalogued at redshift column j with probability Q(-u_fj), so the volume that
// belongs to node k of source i is not the survey's but the part of it in which L_ik is catalogued:
//     g_f(L) = (sum_j wv_j Q(-u_fj(L))) / (sum_j wv_j),   wv_j = wz_j V_j,   u_fj = (L - lam_j) / s_f(L - ld2_j),
//     Q(x) = erfc(x / sqrt 2) / 2,   weight_irk = p_irk exp(-l_irk) / (pref0 vol g_f(i)(L_ik)),
// lam the grid's lower edge, s_f the field's error model (lf_hostprep.h: cut_sigma's statements), all S columns.  g does not
// depend on theta: it is computed once per (source, node), not once per row.
//
// The sum (vefft_cut_g; deconv.py: cut_volume_fraction has the same statements): columns left to right into one accumulator, no
// fma contraction; u > DECONV_CUT_UMAX: a term of exactly wv_j; u < -DECONV_CUT_UMAX: exactly 0; else wv_j (0.5 erfc(-u / sqrt
// 2)); a field whose model sigma is 0 at every node: the step, wv_j when L >= lam_j.  The denominator is the host's, summed the
// same way.  L - ld2_j falls as j rises, so the error model's segment moves one way: it is walked, not searched per column (both
// directions are written, so that a grid whose ld2 does not ascend gets the same segment as the search).
//
// lf_vefftrue_cutvol    grid (narrow chunks + wide chunks), 256 threads: block c takes chunk c of lf_lumpost_part's tables, one
//                       thread per (source, node) pair of the chunk, pairs t, t + 256, ... - a source's nodes on consecutive
//                       threads.  The image {lam, ld2, wv [S each], the model's nodes [M], sigma [nf][M]} goes to dynamic LDS
//                       (vefft_cut_lds_bytes); the columns' reads are broadcasts.  invg[slot] = 1 / g, or 0 where the node is
//                       dropped (g = 0 or g < min_vol_frac) or is no node (the other K - 1 slots of a source with sigma = 0, the
//                       narrow slots of a wide source).  L_ik is vefft_node's: the bits that choose the bin.  dropped[c]: the
//                       chunk's dropped nodes, by the block's fixed tree (ints: exact in any order).
// lf_cut_volume_points  one thread per caller point (field, L) -> g: the same device function (the element test's entry).
// lf_vefftrue_part_cut  lf_vefftrue_part's statements with CUT = true (lf_vefftrue_part_body.h): the same kernel but for the
//                       factor invg[slot] on every node's weight.  A kernel of its own name: lf_vefftrue_part keeps its
//                       arguments and its instructions.
// No atomics.  Slots: narrow source g (the device's order), node k: g K + k; wide source g (the wide list's order): N K + g
// DECONV_WIDE_KMAX + k.  8 bytes per slot: 256 MB at 1e6 sources and K = 32.
#pragma once

#include <hip/hip_runtime.h>

#include "lf_layout.h"
#include "lf_vefftrue.h"

namespace lf {

// the cut model's image in device memory, as the kernels stage it in LDS: lam [S], ld2 [S], wv [S], nodes [M], sigma [nf][M]
struct VeffCutTab {
    const double* img;
    int S, M, nf;
    unsigned step;               // bit f: field f's sigma is 0 at every node (the step)
    double den;                  // sum_j wv_j, left to right
    double min_vol_frac;
};
constexpr int vefft_cut_slots(int S, int M, int nf) { return 3 * S + M + nf * M; }
constexpr int vefft_cut_lds_bytes(int S, int M, int nf) { return vefft_cut_slots(S, M, nf) * 8; }

// g_f(L) from the staged image im; sg: field f's row of sigma (in im); step: the field's sigma is 0 throughout
__device__ __forceinline__ double vefft_cut_g(const double* im, int S, int M, const double* sg, bool step, double den, double L) {
#pragma clang fp contract(off)
    const double *lam = im, *ld2 = im + S, *wv = im + 2 * S, *nd = im + 3 * S;
    double acc = 0.0;
    int i = M > 1 ? M - 2 : 0;
    for (int j = 0; j < S; ++j) {
        double term;
        if (step) {
            term = L >= lam[j] ? wv[j] : 0.0;
        } else {
            const double t = L - ld2[j];
            double s;
            if (M == 1 || !(t > nd[0])) {
                s = sg[0];
            } else if (t >= nd[M - 1]) {
                s = sg[M - 1];
            } else {
                while (i > 0 && nd[i] > t) --i;                    // (the last node at or below t, within 0 .. M - 2)
                while (i < M - 2 && nd[i + 1] <= t) ++i;
                s = sg[i] + (t - nd[i]) * ((sg[i + 1] - sg[i]) / (nd[i + 1] - nd[i]));
            }
            const double u = (L - lam[j]) / s;
            if (u > DECONV_CUT_UMAX) term = wv[j];
            else if (u < -DECONV_CUT_UMAX) term = 0.0;
            else term = wv[j] * (0.5 * erfc(-u / 1.41421356237309504880));
        }
        acc += term;
    }
    return acc / den;
}

// the image to LDS (every thread of the block; the caller's barrier follows)
__device__ __forceinline__ void vefft_cut_stage(const VeffCutTab& t, double* im) {
    const int n = vefft_cut_slots(t.S, t.M, t.nf);
    for (int i = threadIdx.x; i < n; i += BLOCK) im[i] = t.img[i];
}

// x: lf_veff_true's arguments (the chunk tables, lum, sigma, the node tables; the row's and the bins' members are not read)
__global__ __launch_bounds__(BLOCK) void lf_vefftrue_cutvol(VeffTrueArgs x, VeffCutTab t, double* invg, long long wide_off, int* dropped) {
    extern __shared__ double vefft_cut_im[];
    __shared__ double nd[DECONV_WIDE_KMAX];
    __shared__ int red[4];
    const int blk = blockIdx.x, tid = threadIdx.x;
    const bool wide = blk >= x.n0;
    const DeconvArgs& a = wide ? x.w.d : x.d;
    const int cb = wide ? blk - x.n0 : blk;
    int K = x.d.dc.K;
    const double* tab = x.d.nodes;
    if (wide) {
        const int cls = x.w.chunk_class[cb];
        K = x.w.K[cls];
        tab = x.w.tables + x.w.off[cls];
    }
    const int stride = wide ? DECONV_WIDE_KMAX : K;
    vefft_cut_stage(t, vefft_cut_im);
    for (int i = tid; i < K; i += BLOCK) nd[i] = tab[i];
    __syncthreads();
    const int f = a.chunk_field[cb];
    const double* sg = vefft_cut_im + 3 * t.S + t.M + f * t.M;
    const bool step = (t.step >> f) & 1u;
    const int first = a.chunk_start[cb], len = a.chunk_len[cb];
    double* out = invg + (wide ? wide_off : 0ll);
    int nd_drop = 0;
    for (int i = tid; i < len * K; i += BLOCK) {
        const int src = first + i / K, k = i - (i / K) * K;
        const double sgi = a.sigma[src];
        double r = 0.0;
        bool node = false;
        double L = 0.0;
        if (sgi > 0.0) {
            double dl;
            L = vefft_node(a.lum[src], 1.41421356237309504880 * sgi, nd[k], dl);
            node = true;
        } else if (!wide && !x.in_wide[src] && k == 0) {
            L = a.lum[src];
            node = true;
        }
        if (node) {
            const double g = vefft_cut_g(vefft_cut_im, t.S, t.M, sg, step, t.den, L);
            if (g > 0.0 && g >= t.min_vol_frac) r = 1.0 / g;
            else ++nd_drop;
        }
        out[(long long)src * stride + k] = r;
    }
    // the chunk's count: the wave's lanes by the shuffle tree, the four waves through LDS
    for (int off = 32; off > 0; off >>= 1) nd_drop += __shfl_xor(nd_drop, off, 64);
    if ((tid & 63) == 0) red[tid >> 6] = nd_drop;
    __syncthreads();
    if (tid == 0) dropped[blk] = (red[0] + red[1]) + (red[2] + red[3]);
}

// grid (ceil(n / 256)), 256 threads; dynamic LDS: vefft_cut_lds_bytes
__global__ __launch_bounds__(BLOCK) void lf_cut_volume_points(VeffCutTab t, const int* field, const double* L, int n, double* g) {
    extern __shared__ double vefft_cut_im[];
    vefft_cut_stage(t, vefft_cut_im);
    __syncthreads();
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const int f = field[i];
    g[i] = vefft_cut_g(vefft_cut_im, t.S, t.M, vefft_cut_im + 3 * t.S + t.M + f * t.M, (t.step >> f) & 1u, t.den, L[i]);
}

// lf_vefftrue_part with the nodes' factors: dynamic LDS vefft_dyn_lds_bytes(x.nbin), as there
template <int V>
__global__ __launch_bounds__(BLOCK) void lf_vefftrue_part_cut(VeffTrueArgs x, int row0, const double* invg, long long wide_off) {
    constexpr bool CUT = true;
#include "lf_vefftrue_part_body.h"
}

}  // namespace lf
