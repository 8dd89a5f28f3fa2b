// lf_hostprep.h - the host's derivation of every table the kernels read, apart from its upload (lfmcmc.hip: build,
// get_chunks, build_compressed, ensure_deal call these and copy what they return to the device).
//
// Pure host C++ (no HIP, no context, no environment): vectors in, vectors out, so tests/test_hostprep_cpu.py checks
// on any machine what used to show only in a parity run on the GPU.  The constants block KConst is filled in place, member by
// member, by the functions that derive its members (the context's copy starts zeroed and is compared by bytes).
#pragma once
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/lfmcmc.h"
#include "lf_compress.h"
#include "lf_gridbound.h"
#include "lf_layout.h"

namespace lfh {

using namespace lf;

// v[(first + i) w + .] = v[order[i] w + .]: an index order applied to a run of records of w elements
template <typename T>
void reorder(std::vector<T>& v, const std::vector<size_t>& order, size_t w = 1, size_t first = 0) {
    std::vector<T> t(order.size() * w);
    for (size_t i = 0; i < order.size(); ++i)
        for (size_t j = 0; j < w; ++j) t[w * i + j] = v[w * order[i] + j];
    std::copy(t.begin(), t.end(), v.begin() + (std::ptrdiff_t)(first * w));
}

// every redshift column of the [S][S] lattice has the same luminosity nodes
inline bool same_columns(const double* logL, int S) {
    for (int j = 0; j < S; ++j)
        for (int k = 1; k < S; ++k)
            if (logL[(size_t)j * S + k] != logL[(size_t)j * S]) return false;
    return true;
}

// the smallest a4 of chunk ch of `size` nodes (NaN-safe: a NaN node keeps the general form)
inline double chunk_min(const std::vector<double>& a4, size_t ch, size_t size) {
    double m = HUGE_VAL;
    for (size_t g = ch * size; g < std::min(a4.size(), (ch + 1) * size); ++g) m = std::isnan(a4[g]) ? 0.0 : std::fmin(m, a4[g]);
    return m;
}

// the completeness ratio |a / (1 - a)|, a = (2 fcmin - 1)^2 (VmaxLumFunc.py:164)
inline double fc_ratio(double fcmin) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const double a = (2.0 * fcmin - 1.0) * (2.0 * fcmin - 1.0);
    return std::fabs(a / (1.0 - a));
}

// ---- per-source tables, in the order the kernels read them, and the members of kc that come from the descriptor and the
// catalogue (everything but the cells' and the grid's)
struct Catalogue {
    std::vector<int64_t> perm;            // row i of the tables is source perm[i] of the descriptor
    std::vector<double> lum, a1, P, U;    // (FREE, ZEVOL: a1 is the sorted key - log-flux, redshift - the chunk keys come from)
};

inline Catalogue catalogue(const lf_desc* d, KConst& kc) {
    const int nf = d->nf, S = d->S;
    const int64_t N = d->N;
    kc.variant = d->variant;
    kc.fix_sch_al = d->fix_sch_al ? 1 : 0;
    kc.specialise = 1;
    kc.grid_part = 0;
    kc.grid_parts = 1;
    kc.tables = 1;
    kc.key_x0 = 0.0;
    kc.nf = nf;
    kc.S = S;
    if (d->variant == LF_FREE) kc.ndim = 2 + (kc.fix_sch_al ? 0 : 1) + nf + 1;
    else if (d->variant == LF_FIXCOMP) kc.ndim = 2 + (kc.fix_sch_al ? 0 : 1);
    else kc.ndim = 6 + (kc.fix_sch_al ? 0 : 1);
    for (int f = 0; f < MAXF; ++f) {
        kc.lnom0_src[f] = 0.0;
        kc.om0_grid[f] = 0.0;
        kc.flim0[f] = 0.0;
    }
    for (int f = 0; f < nf; ++f) {
        // per-source term: Omega_0_arr is dtype=int (lumfuncmcmc.py:285) -> truncation toward zero
        kc.lnom0_src[f] = std::log(std::trunc(d->omega0[f]) / LF_SQARCSEC);
        kc.om0_grid[f] = d->omega0[f] / LF_SQARCSEC;           // integral: float (lumfuncmcmc.py:375)
        if (d->flim0) kc.flim0[f] = d->flim0[f];
    }
    kc.fc_ratio = fc_ratio(d->fcmin);
    std::memcpy(kc.lims, d->lims, sizeof(kc.lims));
    std::memcpy(kc.pivots, d->pivots, sizeof(kc.pivots));
    kc.sch_al0 = d->sch_al0;
    kc.alpha0 = d->alpha0;

    // FREE: the sources of a field are put in order of flux (the layout is ours to choose; a
    // sum over sources does not care), so that a chunk's first source is its faintest and the kernels can pick
    // a cheaper form of the term per (walker, chunk) - see term_free_noexp.  NaN fluxes go last.
    Catalogue t;
    std::vector<int64_t>& perm = t.perm;
    perm.resize((size_t)N);
    for (int64_t i = 0; i < N; ++i) perm[(size_t)i] = i;
    // ZEVOL: in order of redshift, so that a lane's ST sources are neighbours in z and 10^(-L*(z)) of all of them follows
    // from ONE exponential at the lane's middle source (lf_kernels.h: the local form of the z-evolving term).
    if (d->variant == LF_FREE || d->variant == LF_ZEVOL) {
        const double* key = d->variant == LF_FREE ? d->logf : d->z;
        for (int f = 0; f < nf; ++f)
            std::stable_sort(perm.begin() + d->field_ind[f], perm.begin() + d->field_ind[f + 1], [&](int64_t a, int64_t b) {
                const double x = key[a], y = key[b];
                return std::isnan(y) ? !std::isnan(x) : x < y;
            });
    }
    std::vector<double>&lumv = t.lum, &a1 = t.a1, &P = t.P, &U = t.U;
    lumv.resize((size_t)N), a1.resize((size_t)N), P.resize((size_t)N), U.resize((size_t)N);
    for (int64_t i = 0; i < N; ++i) lumv[(size_t)i] = d->lum[perm[(size_t)i]];
    for (int64_t i = 0; i < N; ++i) {
        const double lum = lumv[(size_t)i];
        if (d->variant == LF_FREE) {
            a1[i] = d->logf[perm[(size_t)i]];
            P[i] = std::pow(10.0, lum - LF_LREF);
            U[i] = std::pow(10.0, d->logf[perm[(size_t)i]] - LF_FREF);
        } else if (d->variant == LF_FIXCOMP) {
            a1[i] = std::log(d->om_arr[perm[(size_t)i]]);
            P[i] = std::pow(10.0, lum - LF_LREF);
            U[i] = 0.0;
        } else {
            a1[i] = d->z[perm[(size_t)i]];
            P[i] = std::log(d->om_arr[perm[(size_t)i]]);
            U[i] = d->z[perm[(size_t)i]] * d->z[perm[(size_t)i]];
        }
    }
    // per-field extremes for the mode classification in lf_prepare
    for (int f = 0; f < MAXF; ++f) {
        kc.nsrc[f] = 0;
        kc.pmax[f] = kc.lum_min[f] = kc.lum_max[f] = kc.a_min[f] = kc.u_min[f] = kc.u_max[f] = kc.z_lo[f] = kc.z_hi[f] = kc.slc[f] = kc.sp[f] = kc.som[f] = kc.sz[f] = kc.sz2[f] = 0.0;
    }
    for (int f = 0; f < nf; ++f) {
        const int64_t lo = d->field_ind[f], hi = d->field_ind[f + 1];
        kc.nsrc[f] = (int)(hi - lo);
        if (hi <= lo) continue;
        double pmax = -HUGE_VAL, lmin = HUGE_VAL, lmax = -HUGE_VAL, amin = HUGE_VAL, amax = -HUGE_VAL, zlo = HUGE_VAL, zhi = -HUGE_VAL;
        bool nan = false;
        long double slc = 0.0L, sp = 0.0L, som = 0.0L, sz = 0.0L, sz2 = 0.0L;
        for (int64_t i = lo; i < hi; ++i) {
            const double lum = lumv[(size_t)i];
            slc += (long double)(lum - LF_LREF);
            if (d->variant != LF_ZEVOL) sp += (long double)P[i];
            if (d->variant == LF_FIXCOMP) som += (long double)a1[i];
            if (d->variant == LF_ZEVOL) {
                som += (long double)P[i];
                sz += (long double)d->z[perm[(size_t)i]];
                sz2 += (long double)U[i];             // the rounded z_i^2 the kernels use
            }
            lmin = std::fmin(lmin, lum);
            lmax = std::fmax(lmax, lum);
            nan = nan || std::isnan(lum);
            if (d->variant != LF_ZEVOL) pmax = std::fmax(pmax, P[i]);
            const double a = d->variant == LF_FREE ? a1[i] : (d->variant == LF_FIXCOMP ? a1[i] : P[i]);
            amin = std::fmin(amin, a);
            amax = std::fmax(amax, a);
            nan = nan || std::isnan(a);
            if (d->variant == LF_ZEVOL) {
                zlo = std::fmin(zlo, d->z[perm[(size_t)i]]);
                zhi = std::fmax(zhi, d->z[perm[(size_t)i]]);
                nan = nan || std::isnan(d->z[perm[(size_t)i]]);
            }
        }
        if (nan) amin = -HUGE_VAL;                 // NaN input: force the careful path
        kc.pmax[f] = pmax;
        kc.lum_min[f] = lmin;
        kc.lum_max[f] = lmax;
        kc.a_min[f] = amin;
        kc.u_min[f] = d->variant == LF_FREE ? std::pow(10.0, amin - LF_FREF) : 0.0;
        kc.u_max[f] = d->variant == LF_FREE ? (nan ? HUGE_VAL : std::pow(10.0, amax - LF_FREF)) : 0.0;
        kc.z_lo[f] = zlo;
        kc.z_hi[f] = zhi;
        kc.slc[f] = (double)slc;
        kc.sp[f] = (double)sp;
        kc.som[f] = (double)som;
        kc.sz[f] = (double)sz;
        kc.sz2[f] = (double)sz2;
    }
    if (d->variant == LF_FREE || d->variant == LF_ZEVOL) {
        // origin of the integer keys of log-flux (ZEVOL: of redshift)
        double x0 = HUGE_VAL;
        for (int64_t i = 0; i < N; ++i)
            if (std::isfinite(a1[(size_t)i])) x0 = std::fmin(x0, a1[(size_t)i]);
        kc.key_x0 = std::isfinite(x0) ? x0 : 0.0;
    }
    return t;
}

// ---- the catalogue's cells.
// The cells of a FREE catalogue (lf_kernels.h: CELL_M): runs of flux-neighbouring sources of one field no wider than
// 2 rho, rho = min(CELL_RHO_H, CELL_RHO_G / alpha_hi) with alpha_hi the prior box's largest alpha_C (walkers outside the
// box are -inf before any sum is looked at).  x = the flux-sorted logf.  Walker-independent: built once.  A field with a
// non-finite flux, or a prior box so wide in alpha_C that cells would hold fewer than four sources on average, gets
// none (kc.cells = 0: every walker is summed over the sources, as before).
// ZEVOL: half the width of a cell in redshift such that every walker inside the prior box of (L1, L2, L3) may be summed
// over the cells (lf_kernels.h: ZCELL_X1, ZCELL_X2).  L*(z) is the parabola through (pivot_i, L_i): its slope at a given
// z and its curvature are linear in (L1, L2, L3), so their largest magnitudes over the box are taken at its corners, and
// the slope's over the catalogue's redshifts at their ends.  0: no cells (an unbounded box, coinciding pivots).
// rho_max, x1, x2: ZCELL_RHO, ZCELL_X1, ZCELL_X2 of lf_kernels.h
inline double zcell_rho_for_box(const KConst& kc, int nf, double rho_max, double x1, double x2) {
    const double lo = kc.lims[LF_LIM_LSTAR][0], hi = kc.lims[LF_LIM_LSTAR][1];
    double zmin = HUGE_VAL, zmax = -HUGE_VAL;
    for (int f = 0; f < nf; ++f)
        if (kc.nsrc[f] > 0) {
            zmin = std::fmin(zmin, kc.z_lo[f]);
            zmax = std::fmax(zmax, kc.z_hi[f]);
        }
    if (!(std::isfinite(lo) && std::isfinite(hi) && std::isfinite(zmin) && std::isfinite(zmax))) return 0.0;
    const double z1 = kc.pivots[0], z2 = kc.pivots[1], z3 = kc.pivots[2];
    if (!(z1 != z2 && z2 != z3 && z1 != z3)) return 0.0;
    double smax = 0.0, amax = 0.0;
    for (int corner = 0; corner < 8; ++corner) {
        const double L1 = corner & 1 ? hi : lo, L2 = corner & 2 ? hi : lo, L3 = corner & 4 ? hi : lo;
        const double d12 = (L2 - L1) / (z2 - z1), d23 = (L3 - L2) / (z3 - z2);
        const double a = (d23 - d12) / (z3 - z1);                     // divided differences: L* = L1 + d12 (z - z1) + a (z - z1)(z - z2)
        for (double z : {zmin, zmax}) smax = std::fmax(smax, std::fabs(d12 + a * (2.0 * z - z1 - z2)));
        amax = std::fmax(amax, std::fabs(a));
    }
    double rho = rho_max;
    // (a little inside the limits: lf_prepare evaluates the same quantities from its own rounded coefficients)
    if (smax > 0.0) rho = std::fmin(rho, 0.98 * x1 / (LF_LN10 * smax));
    if (amax > 0.0) rho = std::fmin(rho, std::sqrt(0.98 * x2 / (LF_LN10 * amax)));
    return std::isfinite(rho) ? rho : 0.0;
}

// ZEVOL: the weights of the sources in their cells and in the compressed catalogue, 10^(lum_i - 42)
inline std::vector<double> lum_weights(const std::vector<double>& lum) {
    std::vector<double> wts(lum.size());
    for (size_t i = 0; i < lum.size(); ++i) wts[i] = std::pow(10.0, lum[i] - LF_LREF);
    return wts;
}

struct Cells {
    bool built = false;                   // false: no cells (everything below is empty; kc keeps what was written on the way)
    std::vector<double> rec;              // [cells][M + 2] {midpoint, S_0 .. S_M}
    std::vector<int> start, len, field;   // per chunk of cells: first cell, cells, field
};

// wts: NULL (FREE: cells in log-flux, plain power sums, chunks of 64 cells) or the sources' weights (ZEVOL: cells in
// redshift, S_j = sum_i wts_i d_i^j, chunks of BLOCK cells; lf_kernels.h: ZCELL_RHO).  FREE: writes kc.kf_first, kf_last, cc_fstart.
// M: the orders kept, CELL_M / ZCELL_M of lf_kernels.h; rho_g, rho_h: its CELL_RHO_G, CELL_RHO_H (FREE)
inline Cells build_cells(KConst& kc, const std::vector<int64_t>& field_ind, const std::vector<double>& x, int nf, int M, double rho_g,
                         double rho_h, const double* wts = nullptr) {
    const int64_t N = field_ind[(size_t)nf];
    const double ahi = kc.lims[LF_LIM_ALPHA][1];
    if (!wts && (!(ahi > 0.0) || !std::isfinite(ahi))) return {};
    const double rho = wts ? kc.zcell_rho : std::fmin(rho_h, rho_g / ahi);
    if (!(rho > 0.0)) return {};
    const size_t per_chunk = wts ? (size_t)BLOCK : 64;
    const size_t rec = (size_t)M + 2;                     // doubles per cell: midpoint, S_0 .. S_M
    Cells t;
    std::vector<double>& cd = t.rec;
    std::vector<int>&cst = t.start, &cln = t.len, &cfl = t.field;
    size_t nreal = 0;                    // cells with sources
    std::vector<long double> S((size_t)M + 1);
    for (int f = 0; f < nf; ++f) {
        const int64_t lo = field_ind[f], hi = field_ind[f + 1];
        if (hi <= lo) continue;
        for (int64_t i = lo; i < hi; ++i)
            if (!std::isfinite(x[(size_t)i]) || (wts && !(std::isfinite(wts[(size_t)i]) && wts[(size_t)i] > 0.0))) return {};
        if (!wts) {
            const double k0 = std::floor((x[(size_t)lo] - kc.key_x0) * KEY_SCALE), k1 = std::ceil((x[(size_t)hi - 1] - kc.key_x0) * KEY_SCALE);
            if (!(k0 >= 0.0 && k1 < (double)KEY_MAX)) return {};
            kc.kf_first[f] = (int)k0;
            kc.kf_last[f] = (int)k1;
        }
        const size_t first_cell = cd.size() / rec;
        for (int64_t i = lo; i < hi;) {
            int64_t j = i + 1;
            while (j < hi && x[(size_t)j] - x[(size_t)i] <= 2.0 * rho) ++j;
            const double xc = 0.5 * (x[(size_t)i] + x[(size_t)j - 1]);
            std::fill(S.begin(), S.end(), 0.0L);
            for (int64_t k = i; k < j; ++k) {
                const long double dlt = (long double)x[(size_t)k] - (long double)xc;
                long double pw = wts ? (long double)wts[(size_t)k] : 1.0L;
                for (int m = 0; m <= M; ++m) {
                    S[m] += pw;
                    pw *= dlt;
                }
            }
            cd.push_back(xc);
            for (int m = 0; m <= M; ++m) cd.push_back((double)S[m]);
            i = j;
        }
        size_t ncf = cd.size() / rec - first_cell;
        nreal += ncf;
        if (!wts) {
            // lf_free addresses chunk cc at cell 64 cc and masks nothing: pad the field to whole chunks with cells of no
            // sources (all sums 0) at the last real midpoint (inside the tables wherever the real cell is)
            kc.cc_fstart[f] = (int)cst.size();
            const double xlast = cd[cd.size() - rec];
            while (ncf % 64) {
                cd.push_back(xlast);
                for (int m = 0; m <= M; ++m) cd.push_back(0.0);
                ++ncf;
            }
        }
        for (size_t s0 = 0; s0 < ncf; s0 += per_chunk) {                // a cell chunk = one wave's lanes (lf_free.h) / one workgroup's threads
            cst.push_back((int)(first_cell + s0));
            cln.push_back((int)std::min<size_t>(per_chunk, ncf - s0));        // (FREE: pads included; they add 0)
            cfl.push_back(f);
        }
    }
    if (!wts) {                                                       // (a field without cells starts where the next one does)
        for (int f = nf; f <= MAXF; ++f) kc.cc_fstart[f] = (int)cst.size();
        for (int f = nf - 1; f >= 0; --f)
            if (field_ind[f + 1] <= field_ind[f]) kc.cc_fstart[f] = kc.cc_fstart[f + 1];
    }
    // (too few sources per cell to pay - for a big catalogue: for a small one even cells of one source apiece beat the
    // per-source path, whose cost is its per-item overhead: 10^3 sources, 16 rows: 23.5 us per evaluation over the sources,
    // 17.5 in lf_main's three launches, 12 over cells)
    if (nreal == 0 || ((size_t)N < 4 * nreal && N > 65536)) return {};
    t.built = true;
    return t;
}

// ---- a catalogue's chunks of `ch` sources of one field.
// hx: the flux-sorted logf of the REAL catalogue (FREE), or NULL (no keys: the chunks never take the table form)
struct Chunks {
    std::vector<int> start, len, field, keys;     // keys: KEY_STRIDE ints per chunk
};

inline Chunks chunk_table(const std::vector<int64_t>& field_ind, int nf, int ch, double key_x0, double g_margin, double h_margin,
                          const double* hx = nullptr, int lane_w = 0) {
    Chunks t;
    std::vector<int>&st = t.start, &ln = t.len, &fl = t.field, &keys = t.keys;
    for (int f = 0; f < nf; ++f) {
        for (int64_t s = field_ind[f]; s < field_ind[f + 1]; s += ch) {
            st.push_back((int)s);
            ln.push_back((int)std::min<int64_t>(ch, field_ind[f + 1] - s));
            fl.push_back(f);
        }
    }
    // Keys for the table-driven form of the FREE term (lf_free.h), rounded so that a key test that
    // passes implies the real-valued condition: kfirst = floor, klast = ceil of (x - x0) 2^20 for the chunk's
    // faintest / brightest source; kamax = the largest alpha_C (x 2^16, floor) for which alpha_C times the widest
    // lane of the chunk (a lane = lane_w neighbours in flux) stays within the g table's margin - 0 when that
    // width already exceeds the h table's margin.  A chunk with a non-finite flux gets keys that fail every test.
    // KS ints per chunk: {kfirst, klast, kamax of the whole chunk, -, kamax of each of its 8 waves}: with lanes of
    // flux-neighbours a wave is 64 lane_w consecutive sources, and a chunk's widest lanes cluster in one or two waves (the
    // sparse end of a field): decided per wave, 0.4 % of the (walker, wave) pairs of the bench workload miss the table
    // form instead of 3.4 %.
    constexpr int KS = KEY_STRIDE;
    keys.assign((size_t)KS * st.size(), 0);
    for (size_t i = 0; i < st.size(); ++i) {
        keys[KS * i] = -1;
        keys[KS * i + 1] = KEY_MAX;
        if (!hx) continue;
        const int64_t s = st[i], n = ln[i];
        if (lane_w <= 0) continue;                // (a kernel that holds no lanes of flux-neighbours: no keys)
        bool finite = true;
        for (int64_t j = 0; j < n; ++j) finite = finite && std::isfinite(hx[s + j]);
        if (!finite) continue;
        const double k0 = std::floor((hx[s] - key_x0) * KEY_SCALE), k1 = std::ceil((hx[s + n - 1] - key_x0) * KEY_SCALE);
        if (!(k0 >= 0.0 && k1 < (double)KEY_MAX)) continue;
        auto amax_key = [&](double spread) {
            double amax = spread > 0.0 ? g_margin / spread : 3.0e4;
            if (spread > h_margin) amax = 0.0;
            return (int)std::floor(std::fmin(amax, 3.0e4) * KEY_ASCALE);
        };
        double spread = 0.0, wspread[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        const int64_t per_wave = 64 * (int64_t)lane_w;
        for (int64_t j = 0; j < n; j += lane_w) {
            const double sp = hx[s + std::min<int64_t>(j + lane_w, n) - 1] - hx[s + j];
            spread = std::fmax(spread, sp);
            const int64_t wv = std::min<int64_t>(j / per_wave, 7);
            wspread[wv] = std::fmax(wspread[wv], sp);
        }
        keys[KS * i] = (int)k0;
        keys[KS * i + 1] = (int)k1;
        keys[KS * i + 2] = amax_key(spread);
        for (int wv = 0; wv < 8; ++wv) keys[KS * i + 4 + wv] = amax_key(wspread[wv]);
    }
    // Chunk order.  The kernels deal contiguous runs of chunk indices to the 8 XCDs (lf_main: in dispatch order inside
    // each run; lf_free: one queue per run), and with the catalogue sorted by flux a chunk's cost depends on its rank
    // in its field (bright chunks run the forms without the exponential for most walkers).  So: deal the chunks
    // round-robin into 8 groups (every group gets the same mix of ranks and fields: natural order would hand one XCD
    // only full-cost chunks), and inside a group put the expensive chunks first - longest first keeps the drain of
    // the launch short: the faint ones before the bright ones, and, with lanes of flux-neighbours (lf_free), before
    // both the chunks whose lanes are too wide for the tables at ordinary alpha_C (the sparse ends of a field: the
    // general form, twice the cost per term).
    const size_t n = st.size();
    if (n > 8) {
        std::vector<size_t> rank(n);                  // rank of the chunk inside its field (natural order is field-major)
        for (size_t i = 0, r = 0; i < n; ++i) {
            r = (i > 0 && fl[i] == fl[i - 1]) ? r + 1 : 0;
            rank[i] = r;
        }
        const int wide = (int)(32.0 * KEY_ASCALE);
        auto cls = [&](size_t i) { return (lane_w > 0 && hx) ? std::min(keys[KS * i + 2], wide) : wide; };
        std::vector<size_t> order;
        order.reserve(n);
        for (size_t g = 0; g < 8; ++g) {
            std::vector<size_t> grp;
            for (size_t i = g; i < n; i += 8) grp.push_back(i);
            std::stable_sort(grp.begin(), grp.end(), [&](size_t a, size_t b) {
                const int ca = cls(a), cb = cls(b);
                return ca != cb ? ca < cb : rank[a] < rank[b];
            });
            order.insert(order.end(), grp.begin(), grp.end());
        }
        reorder(st, order);
        reorder(ln, order);
        reorder(fl, order);
        reorder(keys, order, KS);
    }
    return t;
}

// ---- grid-node tables
struct GridSwitches {                     // (the environment's A/B switches, read by the caller)
    bool gridq = true, zgrid_cols = true, collapse = true;
};

struct Grid {
    std::vector<double> G, PG, W, a3, a4;           // [nodes]
    std::vector<double> L, wL, ck, Dk;              // FREE: the factors of a separable grid (empty otherwise)
    bool binned = false;                            // FREE, separable: piece B over flux bins with a proven bound (lf_gridbound.h)
    lfq::GridQ gridq;
    bool zgrid_cols = false;                        // ZEVOL: the lattice is stored column by column
    std::vector<double> nodes4, zcol;               // FIXCOMP, ZEVOL: {G, PG, W, column} in chunks of 64, {z, z^2} per column
    std::vector<double> a4min, nodes8;              // per chunk of BLOCK nodes; FREE: {G, PG, W, a3, a4, chunk's smallest a4, -, -}
};

// kc: the prior box and fc_ratio (catalogue() first)
inline Grid grid_tables(const lf_desc* d, const KConst& kc, const GridSwitches& sw) {
    const int nf = d->nf, S = d->S;
    // trapz weights from the actual spacings (scipy trapz = sum d*(y1+y0)/2)
    size_t nn = (size_t)S * S;
    const size_t nn2 = nn;               // (the lattice; nn becomes S below when the fixed-completeness grid collapses to its rows)
    Grid t;
    std::vector<double>&G = t.G, &PG = t.PG, &W = t.W, &a3 = t.a3, &a4 = t.a4;
    G.resize(nn), PG.resize(nn), W.resize(nn), a3.assign(nn, 0.0), a4.assign(nn, 0.0);
    std::vector<double> wz(S);
    t.L.resize(S), t.wL.resize(S), t.ck.resize(S), t.Dk.resize(S);      // (of column 0: the grid's own when it is separable)
    for (int k = 0; k < S; ++k) {
        const double dl = k > 0 ? d->zarr[k] - d->zarr[k - 1] : 0.0;
        const double dr = k < S - 1 ? d->zarr[k + 1] - d->zarr[k] : 0.0;
        wz[k] = 0.5 * (dl + dr);
        if (d->variant == LF_FREE) {
            const double dlcm = LF_MPC_CM * d->dl_zarr[k];
            t.Dk[k] = std::log10(4.0 * M_PI * dlcm * dlcm);
            t.ck[k] = wz[k] * d->volume_part[k];
        }
    }
    for (int j = 0; j < S; ++j) {
        for (int k = 0; k < S; ++k) {
            const size_t g = (size_t)j * S + k;
            const double x = d->logL[g];
            const double dl = j > 0 ? x - d->logL[g - S] : 0.0;
            const double dr = j < S - 1 ? d->logL[g + S] - x : 0.0;
            const double wl = 0.5 * (dl + dr);
            const double w = wl * wz[k];
            if (k == 0) t.L[j] = x, t.wL[j] = wl;
            G[g] = x;
            PG[g] = std::pow(10.0, x - LF_LREF);
            if (d->variant == LF_FREE) {
                const double lf = x - t.Dk[k];
                a3[g] = lf;
                a4[g] = std::pow(10.0, lf - LF_FREF);
                W[g] = w * d->volume_part[k];
            } else {
                double s = 0.0;
                for (int f = 0; f < nf; ++f) s += d->integ_part[(size_t)f * nn2 + g];
                W[g] = w * s;
                if (d->variant == LF_ZEVOL) {
                    a3[g] = d->zarr[k];
                    a4[g] = d->zarr[k] * d->zarr[k];
                }
            }
        }
    }
    const bool sep = same_columns(d->logL, S);
    if (d->variant == LF_FREE && S <= GRIDC_MAX_S && sep) {
        // piece B over flux bins (lf_gridbound.h): the bins are proven for the context's whole prior box of (alpha_C, Flim),
        // or the lattice stays.  Every rank of a sharded run derives the same bins from the same grid and box.
        const double alo = kc.lims[LF_LIM_ALPHA][0], ahi = kc.lims[LF_LIM_ALPHA][1];
        const double flo = kc.lims[LF_LIM_FLIM][0], fhi = kc.lims[LF_LIM_FLIM][1];
        if (alo > 0.0 && ahi >= alo && flo > 0.0 && fhi >= flo && std::isfinite(ahi) && std::isfinite(fhi) && sw.gridq) {
            const lfq::Box bx{std::sqrt(kc.fc_ratio), alo, ahi, std::log10(flo) + LF_FREF, std::log10(fhi) + LF_FREF};
            t.binned = lfq::build_gridq(bx, S, t.L.data(), t.wL.data(), t.ck.data(), t.Dk.data(), LF_FREF, LF_LREF, t.gridq);
        }
    } else {
        t.L.clear(), t.wL.clear(), t.ck.clear(), t.Dk.clear();
    }
    if (d->variant == LF_ZEVOL && S >= BLOCK / (ZCOLS - 1) && sw.zgrid_cols) {
        // z-evolving: store the lattice column by column (a sum does not care; lf_kernels.h: gridsum_body takes what depends
        // on the walker per COLUMN).  S >= 128: a chunk of 256 nodes then touches at most 3 columns.
        std::vector<double> tr(nn);
        for (std::vector<double>* arr : {&G, &PG, &W, &a3, &a4}) {
            for (int j = 0; j < S; ++j)
                for (int k = 0; k < S; ++k) tr[(size_t)k * S + j] = (*arr)[(size_t)j * S + k];
            arr->swap(tr);
        }
        t.zgrid_cols = true;
    }
    if (d->variant == LF_FIXCOMP && sw.collapse && sep) {
        // Fixed completeness: the integrand at node (j, k) is T_w(L_jk) W_jk with everything but the Schechter function
        // T folded into W.  When every redshift column has the same luminosity nodes (the constructor clips the columns'
        // lower ends to the catalogue's faintest luminosity: with min_comp_frac = 0 all of them) T depends on the row only
        // and the double sum is sum_j T_w(L_j) (sum_k W_jk): S nodes instead of S^2, exactly - the trapezoid rule's sums
        // in another order.  Row sums in extended precision.
        for (int j = 0; j < S; ++j) {
            long double rs = 0.0L;
            for (int k = 0; k < S; ++k) rs += (long double)W[(size_t)j * S + k];
            G[(size_t)j] = G[(size_t)j * S];
            PG[(size_t)j] = PG[(size_t)j * S];
            W[(size_t)j] = (double)rs;
            a3[(size_t)j] = a4[(size_t)j] = 0.0;
        }
        nn = (size_t)S;
        for (std::vector<double>* arr : {&G, &PG, &W, &a3, &a4}) arr->resize(nn);
    }
    if (d->variant != LF_FREE) {
        // lf_pers reads the nodes as 32-byte records {G, PG, W, redshift column}, padded to whole chunks of 64 (pads: W = 0)
        const size_t nch = (nn + 63) / 64;
        t.nodes4.assign(nch * 64 * 4, 0.0);
        for (size_t g = 0; g < nch * 64; ++g) {
            const size_t gg = std::min(g, nn - 1);
            double* r = &t.nodes4[g * 4];
            r[0] = G[gg];
            r[1] = PG[gg];
            r[2] = g < nn ? W[gg] : 0.0;
            r[3] = t.zgrid_cols ? (double)(gg / (size_t)S) : 0.0;      // (column-major lattice: node = k S + j)
        }
        t.zcol.resize((size_t)S * 2);
        for (int k = 0; k < S; ++k) {
            t.zcol[(size_t)2 * k] = d->zarr[k];
            t.zcol[(size_t)2 * k + 1] = d->zarr[k] * d->zarr[k];
        }
    }
    // per chunk of 256 nodes the smallest a4 (FREE)
    t.a4min.assign((nn + BLOCK - 1) / BLOCK, 0.0);
    for (size_t ch = 0; ch < t.a4min.size(); ++ch) t.a4min[ch] = d->variant == LF_FREE ? chunk_min(a4, ch, BLOCK) : 0.0;
    // lf_free reads the nodes as 64-byte records {G, PG, W, a3, a4, smallest a4 of the node's chunk of 64, -, -}, padded
    // to whole chunks (pads: the last node again with W = 0): one contiguous load per lane, nothing to mask
    if (d->variant == LF_FREE) {
        const size_t nch64 = (nn + 63) / 64;
        t.nodes8.assign(nch64 * 64 * 8, 0.0);
        for (size_t ch = 0; ch < nch64; ++ch) {
            const double m = chunk_min(a4, ch, 64);
            for (size_t l = 0; l < 64; ++l) {
                const size_t g = std::min(ch * 64 + l, nn - 1);
                double* r = &t.nodes8[(ch * 64 + l) * 8];
                r[0] = G[g];
                r[1] = PG[g];
                r[2] = ch * 64 + l < nn ? W[g] : 0.0;
                r[3] = a3[g];
                r[4] = a4[g];
                r[5] = m;
            }
        }
    }
    return t;
}

// ---- the compressed catalogue (lf_compress.h) from the per-source tables.  FREE: key = logf_i, weight 1; ZEVOL: key = z_i,
// weight 10^(lum_i - 42) (lum: the sources' lum, ZEVOL only).  L .. Dk: the separable grid's factors (empty: no compressed grid).
struct Compressed {
    int bad_field = -1;                   // >= 0: this field cannot be compressed to the error bound (nothing below is valid)
    std::vector<int64_t> field_ind;
    std::vector<double> lum, node, U, weight;      // the pseudo-sources, sources of a field contiguous
    int nbins = 0;
    double bound = 0.0;
    bool grid = false;                    // FREE, separable grid: the compressed grid was found too
    lfc::GridOut go;
    std::vector<double> A4, PGL;
};

inline Compressed compress(const KConst& kc, const std::vector<int64_t>& field_ind, const std::vector<double>& key, const std::vector<double>& lum,
                           const std::vector<double>& L, const std::vector<double>& wL, const std::vector<double>& ck,
                           const std::vector<double>& Dk) {
    const int64_t N = (int64_t)key.size();
    std::vector<double> wt;
    lfc::Model m{};
    if (kc.variant == LF_FREE) {
        m.kind = 0;
        m.fc_ratio = kc.fc_ratio;
        m.alpha_lo = kc.lims[LF_LIM_ALPHA][0];
        m.alpha_hi = kc.lims[LF_LIM_ALPHA][1];
        m.flim_lo = kc.lims[LF_LIM_FLIM][0];
        m.flim_hi = kc.lims[LF_LIM_FLIM][1];
    } else {
        m.kind = 1;
        m.L_lo = kc.lims[LF_LIM_LSTAR][0];
        m.L_hi = kc.lims[LF_LIM_LSTAR][1];
        for (int i = 0; i < 3; ++i) m.piv[i] = kc.pivots[i];
        wt = lum_weights(lum);
    }
    lfc::Out out;
    Compressed cc;
    cc.field_ind.assign(1, 0);
    // one validated set of bins for the whole catalogue's coordinate range, shared by the fields
    double klo = HUGE_VAL, khi = -HUGE_VAL;
    for (int64_t i = 0; i < N; ++i) {
        klo = std::fmin(klo, key[(size_t)i]);
        khi = std::fmax(khi, key[(size_t)i]);
    }
    const lfc::Bins bins = lfc::shared_bins(m, klo, khi);
    for (int f = 0; f < kc.nf; ++f) {
        const int64_t lo = field_ind[f], hi = field_ind[f + 1];
        if (!lfc::compress_field(m, key.data() + lo, wt.empty() ? nullptr : wt.data() + lo, hi - lo, out, &bins)) {
            cc.bad_field = f;
            return cc;
        }
        // in order of the coordinate inside the field, like the real catalogue (bins that kept their sources hold
        // them in catalogue order): a chunk's first pseudo-source is its faintest
        const size_t a = (size_t)cc.field_ind.back(), b = out.node.size();
        std::vector<size_t> idx(b - a);
        for (size_t i = 0; i < idx.size(); ++i) idx[i] = a + i;
        std::stable_sort(idx.begin(), idx.end(), [&](size_t x, size_t y) { return out.node[x] < out.node[y]; });
        reorder(out.weight, idx, 1, a);
        reorder(out.node, idx, 1, a);
        cc.field_ind.push_back((int64_t)out.node.size());
    }
    const size_t n = out.node.size();
    cc.nbins = out.nbins;
    cc.bound = out.bound;
    cc.lum.assign(n, kc.variant == LF_ZEVOL ? LF_LREF : 0.0);
    cc.U.resize(n);
    for (size_t i = 0; i < n; ++i) cc.U[i] = kc.variant == LF_FREE ? std::pow(10.0, out.node[i] - LF_FREF) : out.node[i] * out.node[i];
    cc.node.swap(out.node);
    cc.weight.swap(out.weight);
    // the integration grid, when it is separable (no bins found: the full grid stays in use)
    if (kc.variant == LF_FREE && !L.empty()) {
        lfc::Model mg = m;
        mg.kind = 2;
        const int S = kc.S;
        if (lfc::compress_grid(mg, S, L.data(), wL.data(), ck.data(), Dk.data(), cc.go)) {
            cc.A4.resize(cc.go.u.size()), cc.PGL.resize((size_t)S);
            for (size_t i = 0; i < cc.go.u.size(); ++i) cc.A4[i] = std::pow(10.0, cc.go.u[i] - LF_FREF);
            for (int j = 0; j < S; ++j) cc.PGL[(size_t)j] = std::pow(10.0, L[(size_t)j] - LF_LREF);
            cc.grid = true;
        }
    }
    return cc;
}

// ---- the gradient kernels' constants (lf_grad.h).  z: the sources' redshifts (ZEVOL; any order), else NULL.
// sl[m] = sum_i l_m(z_i) with l_m the Lagrange basis on the pivots: d A / d phi_m = ln10 sl[m] does not depend on theta.
inline GradConst grad_const(const KConst& kc, int64_t N, const double* z) {
    GradConst g{};
    g.variant = kc.variant, g.fix_sch_al = kc.fix_sch_al, g.nf = kc.nf, g.ndim = kc.ndim;
    g.sch_al0 = kc.sch_al0;
    g.kappa = std::sqrt(kc.fc_ratio);
    for (int f = 0; f < MAXF; ++f) g.om0_grid[f] = kc.om0_grid[f];
    for (int m = 0; m < 3; ++m) g.pivots[m] = kc.pivots[m];
    g.nsrc = (double)N;
    if (kc.variant == LF_ZEVOL && z) {
        const long double z1 = kc.pivots[0], z2 = kc.pivots[1], z3 = kc.pivots[2];
        long double s[3] = {0.0L, 0.0L, 0.0L};
        for (int64_t i = 0; i < N; ++i) {
            const long double a = z[i] - z1, b = z[i] - z2, c = z[i] - z3;
            s[0] += b * c / ((z1 - z2) * (z1 - z3));
            s[1] += a * c / ((z2 - z1) * (z2 - z3));
            s[2] += a * b / ((z3 - z1) * (z3 - z2));
        }
        for (int m = 0; m < 3; ++m) g.sl[m] = (double)s[m];
    }
    return g;
}

// ---- the Gauss-Hermite rule of the flux-error-convolved likelihood (lf_deconv.h): x[K] ascending and lnw[K] = ln(w_k / sqrt(pi))
// for the weight e^(-x^2).  Newton iterations on the orthonormal Hermite recurrence in extended precision, the positive roots
// from the largest down (the classic starting guesses), mirrored.  False for K outside 2..64.  (deconv.py: gauss_hermite is
// the same routine.)
inline bool gauss_hermite(int K, double* x, double* lnw) {
    if (K < 2 || K > 64) return false;
    const long double PI = 3.14159265358979323846264338327950288L;
    const long double pim4 = 1.0L / std::sqrt(std::sqrt(PI));
    const long double n = (long double)K;
    std::vector<long double> xs((size_t)K, 0.0L), ws((size_t)K, 0.0L);
    auto eval = [&](long double z, long double& pp) {
        long double p1 = pim4, p2 = 0.0L;
        for (int j = 1; j <= K; ++j) {
            const long double p3 = p2;
            p2 = p1;
            p1 = z * std::sqrt(2.0L / j) * p2 - std::sqrt((long double)(j - 1) / j) * p3;
        }
        pp = std::sqrt(2.0L * n) * p2;
        return p1;
    };
    long double z = 0.0L;
    for (int i = 0; i < (K + 1) / 2; ++i) {
        if (i == 0) z = std::sqrt(2.0L * n + 1.0L) - 1.85575L * std::pow(2.0L * n + 1.0L, -1.0L / 6.0L);
        else if (i == 1) z -= 1.14L * std::pow(n, 0.426L) / z;
        else if (i == 2) z = 1.86L * z - 0.86L * xs[(size_t)K - 1];
        else if (i == 3) z = 1.91L * z - 0.91L * xs[(size_t)K - 2];
        else z = 2.0L * z - xs[(size_t)(K - i + 1)];
        long double pp = 1.0L;
        for (int it = 0; it < 100; ++it) {
            const long double p1 = eval(z, pp);
            const long double dz = p1 / pp;
            z -= dz;
            if (std::fabs(dz) <= 1.0e-18L * std::fmax(std::fabs(z), 1.0L)) break;
        }
        if (K % 2 == 1 && i == K / 2) z = 0.0L;
        eval(z, pp);
        xs[(size_t)(K - 1 - i)] = z;
        xs[(size_t)i] = -z;
        ws[(size_t)(K - 1 - i)] = ws[(size_t)i] = 2.0L / (pp * pp);
    }
    for (int k = 0; k < K; ++k) {
        x[k] = (double)xs[(size_t)k];
        lnw[k] = (double)(std::log(ws[(size_t)k]) - 0.5L * std::log(PI));
    }
    return true;
}

// the largest sigma (dex) order K is validated for, < 0 for an order that is not supported
inline double deconv_sigma_max(int K) {
    for (int i = 0; i < DECONV_NORDERS; ++i)
        if (DECONV_ORDERS[i] == K) return DECONV_SIGMA_MAX[i];
    return -1.0;
}

// ---- the wide rule of the flux-error-convolved likelihood (lf_deconv_wide.h) ----
// The n-point Gauss-Legendre rule on [-1, 1], x ascending: Newton iterations on the Legendre recurrence in extended precision,
// the positive roots mirrored.  False for n outside 1..64.  (deconv.py: gauss_legendre is the same routine.)
inline bool gauss_legendre(int n, long double* x, long double* w) {
    if (n < 1 || n > 64) return false;
    const long double PI = 3.14159265358979323846264338327950288L;
    auto eval = [&](long double z, long double& pp) {
        long double p1 = 1.0L, p2 = 0.0L;
        for (int j = 1; j <= n; ++j) {
            const long double p3 = p2;
            p2 = p1;
            p1 = ((2 * j - 1) * z * p2 - (j - 1) * p3) / j;
        }
        pp = n * (z * p1 - p2) / (z * z - 1.0L);
        return p1;
    };
    for (int i = 0; i < (n + 1) / 2; ++i) {
        long double z = std::cos(PI * (i + 0.75L) / (n + 0.5L)), pp = 1.0L;
        for (int it = 0; it < 100; ++it) {
            const long double dz = eval(z, pp) / pp;
            z -= dz;
            if (std::fabs(dz) <= 1.0e-19L) break;
        }
        if (n % 2 == 1 && i == n / 2) z = 0.0L;
        eval(z, pp);
        x[i] = -z, x[n - 1 - i] = z;
        w[i] = w[n - 1 - i] = 2.0L / ((1.0L - z * z) * pp * pp);
    }
    return true;
}

// The table of sigma class cls in the kernel's form: K = DECONV_WIDE_PANELS[cls] * DECONV_WIDE_NPAN nodes, x[K] ascending with
// delta = sqrt(2) sigma x, and lnw[K] = ln[w_j (T / panels) exp(-u^2 / 2) / sqrt(2 pi)] at u = sqrt(2) x - equal panels on
// [-T, T] sigma.  Returns K.  (deconv.py: composite_table.)
inline int wide_table(int cls, double* x, double* lnw) {
    const int panels = DECONV_WIDE_PANELS[cls], np_ = DECONV_WIDE_NPAN;
    long double gx[64], gw[64];
    gauss_legendre(np_, gx, gw);
    const long double PI = 3.14159265358979323846264338327950288L;
    const long double T = (long double)DECONV_WIDE_T, half = T / panels;
    for (int p = 0; p < panels; ++p)
        for (int j = 0; j < np_; ++j) {
            const long double u = -T + (2 * p + 1) * half + half * gx[j];
            x[p * np_ + j] = (double)(u / std::sqrt(2.0L));
            lnw[p * np_ + j] = (double)(std::log(gw[j] * half) - 0.5L * u * u - 0.5L * std::log(2.0L * PI));
        }
    return panels * np_;
}
inline int wide_nodes(int cls) { return DECONV_WIDE_PANELS[cls] * DECONV_WIDE_NPAN; }

// the class of a sigma above the narrow limit: the first whose upper edge is not below it; -1 above the top edge
inline int wide_class(double sigma) {
    for (int c = 0; c < DECONV_WIDE_NCLASS; ++c)
        if (sigma <= DECONV_WIDE_EDGE[c]) return c;
    return -1;
}

// The wide list of a catalogue in the context's order (sigma[i], the fields' ranges field_ind): the indices of the sources with
// sigma above smax sorted by field, then class, then index, and its chunks of up to DECONV_WIDE_CH sources of one field and
// one class.
struct WideList {
    std::vector<int64_t> src;                     // indices into the context's order
    std::vector<int> start, len, field, cls;      // the chunks, into src
};
inline WideList wide_list(const std::vector<double>& sigma, const std::vector<int64_t>& field_ind, int nf, double smax) {
    WideList wl;
    for (int f = 0; f < nf; ++f)
        for (int c = 0; c < DECONV_WIDE_NCLASS; ++c) {
            const size_t first = wl.src.size();
            for (int64_t i = field_ind[f]; i < field_ind[f + 1]; ++i)
                if (sigma[(size_t)i] > smax && wide_class(sigma[(size_t)i]) == c) wl.src.push_back(i);
            for (size_t s = first; s < wl.src.size(); s += DECONV_WIDE_CH) {
                wl.start.push_back((int)s);
                wl.len.push_back((int)std::min<size_t>(DECONV_WIDE_CH, wl.src.size() - s));
                wl.field.push_back(f);
                wl.cls.push_back(c);
            }
        }
    return wl;
}

// ---- the change of the expected counts under a cut on the observed flux (lf_deconv_cut.h) ----
// One field's sigma at log10 flux t: linear between the nodes, constant outside (mock.py: sigma_lookup; lf_mock_noise.h:
// mock_sigma).  T = double: the statements the panels are placed with (deconv.py: _cut_sigma has the same ones); long double:
// the weights'.
template <typename T>
inline T cut_sigma(const double* nodes, const double* sig, int M, T t) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    if (M == 1 || !(t > (T)nodes[0])) return (T)sig[0];
    if (t >= (T)nodes[M - 1]) return (T)sig[M - 1];
    int i = (int)(std::upper_bound(nodes, nodes + M, (double)t) - nodes) - 1;
    i = std::min(std::max(i, 0), M - 2);
    return (T)sig[i] + (t - (T)nodes[i]) * (((T)sig[i + 1] - (T)sig[i]) / ((T)nodes[i + 1] - (T)nodes[i]));
}

// What is wrong with an error model (nodes[M] ascending, sigma[nf][M]), or "" - lf_set_cut_error_model's refusals
inline std::string cut_model_check(const double* nodes, int M, const double* sigma, int nf) {
    if (!nodes || !sigma) return "NULL nodes or sigma";
    if (M < 1 || M > DECONV_CUT_MAX_NODES) return "M must be in 1.." + std::to_string(DECONV_CUT_MAX_NODES);
    for (int m = 0; m < M; ++m) {
        if (!std::isfinite(nodes[m])) return "nodes must be finite";
        if (m > 0 && !(nodes[m] > nodes[m - 1])) return "nodes must increase";
    }
    for (int f = 0; f < nf; ++f) {
        int zeros = 0;
        for (int m = 0; m < M; ++m) {
            const double s = sigma[(size_t)f * M + m];
            if (!std::isfinite(s) || s < 0.0) return "sigma must be finite and >= 0";
            if (s > DECONV_CUT_SIGMA_MAX) {
                char msg[200];
                std::snprintf(msg, sizeof(msg), "sigma = %.4g dex of field %d is above %.2f dex, the largest value the cut model is "
                              "validated for (per-column error below 1e-7)", s, f, DECONV_CUT_SIGMA_MAX);
                return msg;
            }
            zeros += s == 0.0 ? 1 : 0;
        }
        if (zeros != 0 && zeros != M)
            return "the sigma of field " + std::to_string(f) + " is 0 at some nodes and not at others: all 0 (no errors) or all > 0";
    }
    return "";
}

// The node tables: per field f with errors and redshift column j the composite Gauss-Legendre rule on [Lam - H, Lam] and
// [Lam, min(Lam + H, top)], Lam = lam[j] the grid's lower edge, H = DECONV_CUT_T x the field's largest sigma.  Panels of
// DECONV_CUT_NPAN nodes are laid from Lam outwards, each no wider than DECONV_CUT_PANEL_SIGMA x the smallest sigma on it,
// than DECONV_CUT_H dex, and than the distance to the next node of the error model (where s has a kink); a panel wholly
// beyond |u| = DECONV_CUT_UMAX is not made.  Placement in double with the statements of deconv.py: _cut_panels (the same
// panels on both sides); the weights in long double:
//     c = -/+ wz_j vol_j (GL weight) Q(|u|) om0_f [fc^(1/d) at the node: fixed completeness],  u = (L - Lam) / s_f(L - ld2_j),
// the weights of MINUS Delta B (- below the cut, + above).  Nodes whose weight is exactly 0 are dropped.  limit > 0 (tests):
// only the first `limit` nodes of every field are kept.  A field's nodes are contiguous, columns ascending; chunks of
// DECONV_CUT_CH nodes of one field.  err: "" or what is refused.
struct CutTables {
    std::string err;
    std::vector<double> L, P, c, a3, a4;          // a3: FREE log flux, ZEVOL redshift; a4: FREE 10^(a3 + 17)
    std::vector<int> start, len, field;
    int nnodes[MAXF] = {};
    double H[MAXF] = {};
};
inline CutTables cut_tables(int variant, int nf, int S, const double* lam, const double* top, const double* zarr, const double* vol,
                            const double* ld2, const double* om0, const double* flim0, double alpha0, double kappa, const double* nodes,
                            int M, const double* sigma, int64_t limit) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    CutTables t;
    long double gxl[64], gwl[64];
    gauss_legendre(DECONV_CUT_NPAN, gxl, gwl);
    double gx[DECONV_CUT_NPAN];
    for (int k = 0; k < DECONV_CUT_NPAN; ++k) gx[k] = (double)gxl[k];
    const long double SQRT2 = std::sqrt(2.0L), LN10 = std::log(10.0L);
    for (int f = 0; f < nf; ++f) {
        const double* sg = sigma + (size_t)f * M;
        const double smax = *std::max_element(sg, sg + M);
        const double H = DECONV_CUT_T * smax;
        t.H[f] = H;
        const size_t first = t.L.size();
        for (int j = 0; j < S && H > 0.0; ++j) {
            const double dl = j > 0 ? zarr[j] - zarr[j - 1] : 0.0, dr = j < S - 1 ? zarr[j + 1] - zarr[j] : 0.0;
            const long double wv = (long double)(0.5 * (dl + dr)) * (long double)vol[j] * (long double)om0[f];
            for (int side = 0; side < 2; ++side) {
                const double dir = side == 0 ? -1.0 : 1.0;
                const double total = side == 0 ? H : std::fmin(lam[j] + H, top[j]) - lam[j];
                std::vector<double> brk;
                for (int m = 0; m < M; ++m) {
                    const double x = nodes[m] + ld2[j];
                    const double dk = side == 0 ? lam[j] - x : x - lam[j];
                    if (dk > 0.0 && dk < total) brk.push_back(dk);
                }
                std::sort(brk.begin(), brk.end());
                double d = 0.0;
                size_t kb = 0;
                int made = 0;
                while (d < total) {
                    while (kb < brk.size() && brk[kb] <= d) ++kb;
                    const double seg_end = kb < brk.size() ? brk[kb] : total;
                    const double s0 = cut_sigma<double>(nodes, sg, M, lam[j] + dir * d - ld2[j]);
                    double h = std::fmin(std::fmin(DECONV_CUT_PANEL_SIGMA * s0, DECONV_CUT_H), seg_end - d);
                    double s1 = cut_sigma<double>(nodes, sg, M, lam[j] + dir * (d + h) - ld2[j]);
                    if (s1 < s0) {
                        h = std::fmin(h, DECONV_CUT_PANEL_SIGMA * s1);
                        s1 = cut_sigma<double>(nodes, sg, M, lam[j] + dir * (d + h) - ld2[j]);
                    }
                    double dn = d + h;
                    if (seg_end - dn < 1.0e-9) dn = seg_end, h = dn - d;
                    if (!(h > 0.0)) break;
                    if (!(d > DECONV_CUT_UMAX * std::fmax(s0, s1))) {
                        if (++made > DECONV_CUT_MAX_PANELS) {
                            t.err = "the error model of field " + std::to_string(f) + " needs more than " +
                                    std::to_string(DECONV_CUT_MAX_PANELS) + " panels on one side of the cut in redshift column " +
                                    std::to_string(j) + ": its sigma varies too strongly across the band of 7.5 sigma_max";
                            return t;
                        }
                        const double half = 0.5 * h, mid = (lam[j] + dir * d) + dir * half;
                        for (int k = 0; k < DECONV_CUT_NPAN; ++k) {
                            const double Ln = mid + half * gx[k];
                            const long double Lq = (long double)Ln, tf = Lq - (long double)ld2[j];
                            const long double s = cut_sigma<long double>(nodes, sg, M, tf);
                            const long double u = (Lq - (long double)lam[j]) / s;
                            long double w = wv * ((long double)half * gwl[k]) * (0.5L * erfcl(std::fabs(u) / SQRT2));
                            if (variant != LF_FREE) {
                                // fc^(1/d) at the node's flux, the fixed curve (lf_grad.h: comp_form's statements)
                                const long double y = (tf + 17.0L) - std::log10((long double)flim0[f]);
                                const long double num = (long double)alpha0 * y, den = std::sqrt(num * num + 1.0L);
                                const long double v = std::exp(LN10 * (y + (long double)kappa / (long double)alpha0));
                                const long double dd = -std::expm1(-v);
                                const long double lnfc = num < 0.0L ? -std::log(2.0L * den * (den - num)) : std::log1p(-0.5L / (den * (den + num)));
                                w *= std::exp(lnfc / dd);
                            }
                            const double c = (double)(side == 0 ? -w : w);
                            if (c == 0.0 || c != c) continue;
                            const double a3 = variant == LF_FREE ? Ln - ld2[j] : (variant == LF_ZEVOL ? zarr[j] : 0.0);
                            t.L.push_back(Ln);
                            t.P.push_back(std::pow(10.0, Ln - LF_LREF));
                            t.c.push_back(c);
                            t.a3.push_back(a3);
                            t.a4.push_back(variant == LF_FREE ? std::pow(10.0, a3 - LF_FREF) : 0.0);
                        }
                    }
                    d = dn;
                }
            }
        }
        if (limit > 0 && t.L.size() - first > (size_t)limit)
            for (std::vector<double>* a : {&t.L, &t.P, &t.c, &t.a3, &t.a4}) a->resize(first + (size_t)limit);
        t.nnodes[f] = (int)(t.L.size() - first);
        for (size_t s = first; s < t.L.size(); s += DECONV_CUT_CH) {
            t.start.push_back((int)s);
            t.len.push_back((int)std::min<size_t>(DECONV_CUT_CH, t.L.size() - s));
            t.field.push_back(f);
        }
    }
    return t;
}

// ---- lf_free's static deal (lf_layout.h: DEAL_*): flux bins, then cell chunks, each to the virtual workgroup that would be done
// first - a bin costs a wave cost_b = 8 units, a cell chunk 3 (tools/stamps_fused.py), and the ranks of the younger half are
// counted cost_h = 8 units behind (swept on one box, tools/deal_sweep.sh: 13.4 us per 128-row evaluation at 8-10, 13.75 at 0-6,
// 14.0 at 16; the arithmetic deal 15.25; at 256 rows, where a workgroup serves an elder and a younger rank, all within 2 %).  Bins that a source-sharded rank does not integrate (grid_share) cost nothing.  The table depends
// on the context (numbers of cell chunks and bins, grid share) only - never on the batch.
// (also behind lf_deal_table for the CPU tests)
inline std::vector<int> make_deal(int nchC, int nbq, int grid_part, int grid_parts, int cost_h = 8, int cost_b = 8) {
    std::vector<int> load(VF), cnt_c(VF, 0), cnt_b(VF, 0), own_c(nchC), own_b(nbq);
    for (int v = 0; v < VF; ++v) load[v] = v >= VF / 2 ? cost_h : 0;
    auto next = [&]() { return (int)(std::min_element(load.begin(), load.end()) - load.begin()); };      // (ties: the lowest rank)
    for (int b = 0; b < nbq; ++b) {
        const int v = next();
        own_b[b] = v;
        ++cnt_b[v];
        load[v] += grid_parts > 1 && b % grid_parts != grid_part ? 0 : cost_b;
    }
    for (int i = 0; i < nchC; ++i) {
        const int v = next();
        own_c[i] = v;
        ++cnt_c[v];
        load[v] += 3;
    }
    std::vector<int> t(DEAL_LIST + nchC + nbq);
    t[0] = 0;
    t[DEAL_BINS] = 0;
    for (int v = 0; v < VF; ++v) {
        t[v + 1] = t[v] + cnt_c[v];
        t[DEAL_BINS + v + 1] = t[DEAL_BINS + v] + cnt_b[v];
    }
    std::vector<int> at_c(t.begin(), t.begin() + VF), at_b(t.begin() + DEAL_BINS, t.begin() + DEAL_BINS + VF);
    for (int i = 0; i < nchC; ++i) t[DEAL_LIST + at_c[own_c[i]]++] = i;
    for (int b = 0; b < nbq; ++b) t[DEAL_LIST + nchC + at_b[own_b[b]]++] = b;
    return t;
}

// ---- who finishes a tile of lf_free's polling hand-over (lf_tile.h): the workgroup expected to END LAST, so that the others'
// partial sums are in memory when it gets there.  Per group size fgroup = 8, 16, 24, 32 (entry fgroup / 8 - 1; lf_tile.h:
// tile_ranks) the PHYSICAL rank with the largest dealt cost: rank r of fgroup serves the virtual ranks r, r + fgroup, ... of the
// deal table t, a bin this context integrates costs cost_b, a cell chunk 3, and the ranks of the group's younger half
// (r >= fgroup / 2: the second workgroups of their CUs) start cost_h behind - make_deal's units and make_deal's handicap.  Ties
// go to the highest rank, the youngest.  Like the table, the ranks depend on the context only.
inline std::array<int, 4> deal_finishers(const std::vector<int>& t, int nchC, int nbq, int grid_part, int grid_parts, int cost_h = 8,
                                         int cost_b = 8) {
    int vcost[VF];
    for (int v = 0; v < VF; ++v) {
        vcost[v] = 3 * (t[v + 1] - t[v]);
        for (int i = t[DEAL_BINS + v]; i < t[DEAL_BINS + v + 1]; ++i) {
            const int b = t[DEAL_LIST + nchC + i];
            vcost[v] += grid_parts > 1 && b % grid_parts != grid_part ? 0 : cost_b;
        }
    }
    (void)nbq;
    std::array<int, 4> fin{};
    for (int g = 0; g < 4; ++g) {
        const int fgroup = 8 * (g + 1);
        int best = 0, bestc = -1;
        for (int r = 0; r < fgroup; ++r) {
            int c = r >= fgroup / 2 ? cost_h : 0;
            for (int v = r; v < VF; v += fgroup) c += vcost[v];
            if (c >= bestc) best = r, bestc = c;
        }
        fin[(size_t)g] = best;
    }
    return fin;
}

// ---- the quantile arguments of the band entries (lf_bands.h: bands_quantiles; lf_veffdraws.h), checked and prepared: q[nq] in
// [0, 100] with nq <= maxq (LF_Q_LINEAR), or nq == 1 and q ignored (LF_Q_MEDIAN); R draws in 2^lg slots.
// tab holds {prev, next, gamma} per quantile:
// numpy 2.x's np.percentile(v, q, axis=0) index arithmetic (percentile: qf = q / 100; _QuantileMethods["linear"]:
// vi = (R - 1) qf; _get_indexes: prev = floor(vi), next = prev + 1, vi >= R - 1 -> both -1 (the last), vi < 0 -> both 0;
// _get_gamma: gamma = vi - prev with the CLAMPED prev, so vi + 1 past the end)
struct Quantiles {
    bool ok = false;
    std::vector<double> tab;
    int lg = 0;
};

inline Quantiles quantiles(int32_t R, int32_t nq, const double* q, int32_t method, int maxq) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    Quantiles t;
    if (method == LF_Q_MEDIAN ? nq != 1 : (method != LF_Q_LINEAR || nq < 1 || nq > maxq || !q)) return t;
    t.tab.assign(3 * (size_t)nq, 0.0);
    for (int i = 0; method == LF_Q_LINEAR && i < nq; ++i) {
        if (!(q[i] >= 0.0 && q[i] <= 100.0)) return t;                       // (NaN fails both)
        const double qf = q[i] / 100.0;
        const double vi = (double)(R - 1) * qf;
        double prev = std::floor(vi), next = prev + 1.0;
        if (vi >= (double)(R - 1)) prev = next = -1.0;
        if (vi < 0.0) prev = next = 0.0;
        t.tab[3 * i + 2] = vi - prev;
        t.tab[3 * i] = prev < 0.0 ? (double)(R - 1) : prev;
        t.tab[3 * i + 1] = next < 0.0 ? (double)(R - 1) : next;
    }
    while ((1 << t.lg) < R) ++t.lg;
    t.ok = true;
    return t;
}

}  // namespace lfh
