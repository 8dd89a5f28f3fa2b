// lf_vefftrue_part_body.h - the statements of lf_vefftrue_part (lf_vefftrue.h) and of lf_vefftrue_part_cut (lf_vefftrue_cut.h),
// included in both kernels' bodies: NOT a header of its own.  In scope where it is included: x (VeffTrueArgs), row0, V, and
//     constexpr bool CUT; const double* invg; long long wide_off;
// CUT: every node's weight is multiplied by invg[slot], 1 / g of the node's catalogued volume fraction
// or 0 for a dropped node, before the segmented scan - one 8-byte load per lane and node, the lanes of a source on consecutive
// slots: a narrow source g's at g K + k, a wide source's at wide_off + g DECONV_WIDE_KMAX + k.  CUT = false: the statements of
// lf_vefftrue_part as they were, nothing more - the text is shared so that the plain kernel's instructions cannot drift.
    __shared__ double nd[2 * DECONV_WIDE_KMAX];
    extern __shared__ double vefft_dyn[];
    __shared__ DeconvRow rw;
    const int blk = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int row = row0 + blockIdx.y;
    const bool wide = blk >= x.n0;
    const DeconvArgs& a = wide ? x.w.d : x.d;
    const int cb = wide ? blk - x.n0 : blk;
    if (!isfinite(a.lnprob[row])) return;                 // (the whole block, before any barrier; the reduce does not read its slots)
    int K = a.dc.K;
    const double* tab = a.nodes;
    if (wide) {
        const int cls = x.w.chunk_class[cb];
        K = x.w.K[cls];
        tab = x.w.tables + x.w.off[cls];
    }
    const int nbin = x.nbin;
    double* ed = vefft_dyn;                                // [nbin + 1]
    double* hist = vefft_dyn + vefft_edge_slots(nbin);     // [4][nbin]
    for (int i = tid; i < 2 * K; i += BLOCK) nd[i] = tab[i];
    for (int i = tid; i <= nbin; i += BLOCK) ed[i] = x.edges[i];
    double* hw = hist + wv * nbin;
    for (int i = lane; i < nbin; i += 64) hw[i] = 0.0;
    if (tid == 0) rw = deconv_row<V>(a, row, a.chunk_field[cb]);
    __syncthreads();
    const DeconvRow& w = rw;                               // (read where it is used: the row's constants need no registers of their own)
    const int first = a.chunk_start[cb], len = a.chunk_len[cb];
    const bool halves = K <= 32;                           // two sources at once, one per half-wave
    const int per = halves ? 2 : 1;
    const int sub = halves ? lane >> 5 : 0, k0 = halves ? lane & 31 : lane;
    const int npass = halves ? 1 : (K + 63) >> 6;
    for (int base = wv * 64; base < len; base += 4 * 64) {
        const int nsrc = min(64, len - base);
        VeffTrueSrc mine{};
        if (lane < nsrc) mine = vefft_source<V>(x, a, w, wide, first + base + lane);
        for (int j0 = 0; j0 < nsrc; j0 += per) {
            const int j = j0 + sub;
            VeffTrueSrc s = vefft_bcast(mine, j < nsrc ? j : j0);
            if (j >= nsrc) s.kind = 0;
            const double* ig = nullptr;
            if (CUT) {
                const long long src = first + base + j;
                ig = invg + (wide ? wide_off + src * DECONV_WIDE_KMAX : src * (long long)x.d.dc.K);
            }
            double av[VEFFT_PASSES], val[VEFFT_PASSES];
            int bin[VEFFT_PASSES];
            double m = -HUGE_VAL;
#pragma unroll
            for (int p = 0; p < VEFFT_PASSES; ++p) {
                av[p] = -HUGE_VAL, val[p] = 0.0, bin[p] = -2;
                if (p >= npass) continue;
                const int k = p * 64 + k0;
                if (s.kind == 2 && k < K) {
                    double dl;
                    const double L = vefft_node(s.lum, s.s2, nd[k], dl);
                    const double em = expm1(LF_LN10 * dl);
                    const double l = comp_form<false>(w.aC, w.aC_ln, w.kc2, s.y0 + dl, s.v0 * (em + 1.0)).l;
                    const double sch = w.c1l * dl - s.t * em;
                    av[p] = nd[K + k] + (sch + (l - s.l0));
                    val[p] = nd[K + k] + (sch - s.l0);                 // av - l, formed without l
                    bin[p] = vefft_bin(ed, nbin, L);
                } else if (s.kind == 1 && k == 0) {
                    av[p] = 0.0;
                    val[p] = -s.l0;
                    bin[p] = vefft_bin(ed, nbin, s.lum);
                }
                m = fmax(m, av[p]);
            }
            // the source's normaliser: over its 32 or 64 lanes
            for (int off = halves ? 16 : 32; off > 0; off >>= 1) m = fmax(m, __shfl_xor(m, off, 64));
            double e[VEFFT_PASSES], tot = 0.0;
#pragma unroll
            for (int p = 0; p < VEFFT_PASSES; ++p) {
                e[p] = av[p] == -HUGE_VAL ? 0.0 : exp(av[p] - m);
                tot += e[p];
            }
            for (int off = halves ? 16 : 32; off > 0; off >>= 1) tot += __shfl_xor(tot, off, 64);
#pragma unroll
            for (int p = 0; p < VEFFT_PASSES; ++p) {
                if (p >= npass) continue;
                // p exp(-l) / pv in one exponent; a node whose exponent is -inf adds exactly 0
                double v = av[p] == -HUGE_VAL ? 0.0 : (exp(val[p] - m) / tot) / x.pv;
                if (CUT && av[p] != -HUGE_VAL) v *= ig[p * 64 + k0];        // (0: the node adds exactly 0)
                const int b = bin[p];
                // the segment's sum to its last lane (a source's lanes: k0 >= off keeps a half-wave to itself)
#pragma unroll
                for (int off = 1; off < 64; off <<= 1) {
                    const double vu = __shfl_up(v, off, 64);
                    const int bu = __shfl_up(b, off, 64);
                    if (k0 >= off && bu == b) v += vu;
                }
                const int bn = __shfl_down(b, 1, 64);
                const bool tail = (k0 == (halves ? 31 : 63) || bn != b) && b >= 0 && b < nbin;
                for (int ph = 0; ph < per; ++ph) {
                    if (tail && sub == ph) hw[b] += v;
                    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                }
            }
        }
    }
    __syncthreads();
    double* dst = x.partial + ((size_t)blk * VEFFT_ROWS + blockIdx.y) * (size_t)nbin;
    for (int i = tid; i < nbin; i += BLOCK) dst[i] = ((hist[i] + hist[nbin + i]) + hist[2 * nbin + i]) + hist[3 * nbin + i];
