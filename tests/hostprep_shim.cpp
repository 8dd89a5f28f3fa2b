// hostprep_shim.cpp - csrc/lf_hostprep.h behind a C interface, for tests/test_hostprep_cpu.py.  Compiled by the host compiler
// with no ROCm include path: that it compiles is the check that the header is host-only.  A call derives one set of tables
// and parks its vectors in numbered slots; hp_get_d / hp_get_i copy a slot out (out = NULL: its size only).
#include "../lumfuncmcmc_amd/csrc/lf_hostprep.h"

namespace {
std::vector<double> D[16];
std::vector<int> I[8];
template <typename T>
int64_t get(const std::vector<T>& v, T* out) {
    if (out) std::copy(v.begin(), v.end(), out);
    return (int64_t)v.size();
}
}  // namespace

extern "C" {

int64_t hp_get_d(int slot, double* out) { return get(D[slot], out); }
int64_t hp_get_i(int slot, int* out) { return get(I[slot], out); }

// layout constants the test's bounds are stated in
double hp_const(int id) {
    const double v[] = {0.0, 0.0, 0.0, 0.0, 0.0, (double)lf::BLOCK,
                        (double)lf::KEY_STRIDE, lf::KEY_SCALE, (double)lf::KEY_MAX, (double)lf::MAXF, (double)sizeof(lf::KConst)};
    return v[id];
}

// perm, lum, a1, P, U: [N]; fields: [17][MAXF] = nsrc, pmax, lum_min, lum_max, a_min, u_min, u_max, z_lo, z_hi, slc, sp, som, sz,
// sz2, lnom0_src, om0_grid, flim0; scalars: key_x0, fc_ratio, ndim
void hp_catalogue(const lf_desc* d, int64_t* perm, double* lum, double* a1, double* P, double* U, double* fields, double* scalars) {
    lf::KConst kc{};
    const lfh::Catalogue c = lfh::catalogue(d, kc);
    std::copy(c.perm.begin(), c.perm.end(), perm);
    std::copy(c.lum.begin(), c.lum.end(), lum);
    std::copy(c.a1.begin(), c.a1.end(), a1);
    std::copy(c.P.begin(), c.P.end(), P);
    std::copy(c.U.begin(), c.U.end(), U);
    const double* rows[] = {nullptr, kc.pmax, kc.lum_min, kc.lum_max, kc.a_min, kc.u_min, kc.u_max, kc.z_lo, kc.z_hi, kc.slc, kc.sp,
                            kc.som, kc.sz, kc.sz2, kc.lnom0_src, kc.om0_grid, kc.flim0};
    for (int f = 0; f < lf::MAXF; ++f) {
        fields[f] = kc.nsrc[f];
        for (int r = 1; r < 17; ++r) fields[r * lf::MAXF + f] = rows[r][f];
    }
    scalars[0] = kc.key_x0, scalars[1] = kc.fc_ratio, scalars[2] = kc.ndim;
}

// slots D0.. = G, PG, W, a3, a4, L, wL, ck, Dk, nodes4, zcol, a4min, nodes8, the flux bins' rec.  Returns zgrid_cols + 2 binned.
int hp_grid(const lf_desc* d, int gridq, int zgrid_cols, int collapse) {
    lf::KConst kc{};
    lfh::catalogue(d, kc);
    lfh::GridSwitches sw;
    sw.gridq = gridq, sw.zgrid_cols = zgrid_cols, sw.collapse = collapse;
    lfh::Grid g = lfh::grid_tables(d, kc, sw);
    std::vector<double>* v[] = {&g.G, &g.PG, &g.W, &g.a3, &g.a4, &g.L, &g.wL, &g.ck, &g.Dk, &g.nodes4, &g.zcol, &g.a4min, &g.nodes8, &g.gridq.rec};
    for (int i = 0; i < 14; ++i) D[i].swap(*v[i]);
    return (g.zgrid_cols ? 1 : 0) + (g.binned ? 2 : 0);
}

// The cells of the descriptor's catalogue (FREE, ZEVOL).  D0 = the records, D1 = the sorted key, D2 = {rho (ZEVOL)}; I0.. = the
// chunks' start, len, field; I3 = kf_first[MAXF], kf_last[MAXF], cc_fstart[MAXF + 1].  Returns built.
// par: CELL_RHO_G, CELL_RHO_H, ZCELL_RHO, ZCELL_X1, ZCELL_X2, CELL_M, ZCELL_M of lf_kernels.h
int hp_cells(const lf_desc* d, const double* par) {
    lf::KConst kc{};
    lfh::Catalogue c = lfh::catalogue(d, kc);
    for (int f = 0; f < lf::MAXF; ++f) kc.kf_last[f] = lf::KEY_MAX;
    const std::vector<int64_t> fi(d->field_ind, d->field_ind + d->nf + 1);
    lfh::Cells cl;
    if (d->variant == LF_ZEVOL) {
        kc.zcell_rho = lfh::zcell_rho_for_box(kc, d->nf, par[2], par[3], par[4]);
        cl = lfh::build_cells(kc, fi, c.a1, d->nf, (int)par[6], par[0], par[1], lfh::lum_weights(c.lum).data());
    } else {
        cl = lfh::build_cells(kc, fi, c.a1, d->nf, (int)par[5], par[0], par[1]);
    }
    D[0].swap(cl.rec), D[1].swap(c.a1), D[2].assign(1, kc.zcell_rho);
    I[0].swap(cl.start), I[1].swap(cl.len), I[2].swap(cl.field);
    I[3].assign(kc.kf_first, kc.kf_first + lf::MAXF);
    I[3].insert(I[3].end(), kc.kf_last, kc.kf_last + lf::MAXF);
    I[3].insert(I[3].end(), kc.cc_fstart, kc.cc_fstart + lf::MAXF + 1);
    return cl.built;
}

// The table of chunks of ch sources; lane_w > 0: with keys from the sorted key.  I0.. = start, len, field, keys; D0 = the sorted
// key, D1 = {key_x0}
void hp_chunks(const lf_desc* d, int ch, int lane_w, double g_margin, double h_margin) {
    lf::KConst kc{};
    lfh::Catalogue c = lfh::catalogue(d, kc);
    const std::vector<int64_t> fi(d->field_ind, d->field_ind + d->nf + 1);
    lfh::Chunks t = lfh::chunk_table(fi, d->nf, ch, kc.key_x0, g_margin, h_margin, lane_w > 0 ? c.a1.data() : nullptr, lane_w);
    I[0].swap(t.start), I[1].swap(t.len), I[2].swap(t.field), I[3].swap(t.keys);
    D[0].swap(c.a1), D[1].assign(1, kc.key_x0);
}

}  // extern "C"
