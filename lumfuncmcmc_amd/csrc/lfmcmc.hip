// lfmcmc.hip - C ABI (include/lfmcmc.h) over the gfx950 kernels in lf_kernels.h.
//
// Host side of the boundary: copies the catalogue and grids to HBM once, derives the
// parameter-independent tables (P_i, U_i, trapezoid weights, field-summed integrand), and per
// call enqueues prepare -> per-source sum -> grid integral -> finalize on one HIP stream.
#include "../../include/lfmcmc.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <map>
#include <string>
#include <type_traits>
#include <vector>

#include "lf_bands.h"
#include "lf_compress.h"
#include "lf_devmem.h"
#include "lf_diag.h"
#include "lf_deconv.h"
#include "lf_deconv_cut.h"
#include "lf_deconv_cut_grad.h"
#include "lf_deconv_grad.h"
#include "lf_deconv_tile.h"
#include "lf_deconv_wide.h"
#include "lf_lumpost.h"
#include "lf_grad.h"
#include "lf_gridbound.h"
#include "lf_hostcall.h"
#include "lf_hostprep.h"
#include "lf_kernels.h"
#include "lf_free.h"
#include "lf_mock.h"
#include "lf_mock_noise.h"
#include "lf_mock_cut.h"
#include "lf_mock_hist2.h"
#include "lf_pers.h"
#include "lf_pt.h"
#include "lf_veffdraws.h"
#include "lf_vefftrue.h"
#include "lf_vefftrue_cut.h"
#include "lf_veffslices.h"

namespace {

thread_local std::string g_create_error = "";

struct ChunkTable {
    int n = 0;
    Buf<int> d_start, d_len, d_field;
    Buf<int> d_keys;           // FREE, real catalogue: lf::KEY_STRIDE ints per chunk (get_chunks)
};

struct EventPair {
    hipEvent_t a, b;
    int kind;
    int count = 1;        // launches between the two events (option "profile_span")
};

// compressed catalogue (lf_compress.h): weighted pseudo-sources, sources of a field contiguous
struct CompressedCat {
    bool built = false;
    int64_t n = 0;
    std::vector<int64_t> field_ind;
    Buf<double> d_lum, d_a1, d_U, d_W;
    std::map<int, ChunkTable> chunks;
    int nbins = 0;
    double bound = 0.0;
};

// FREE: the compressed integration grid (lf_compress.h), built with the compressed catalogue when the grid is separable
struct CompressedGrid {
    bool built = false;
    int nb = 0;
    double bound = 0.0;
    Buf<double> d_U, d_A4, d_omega, d_L, d_PGL;
    Buf<int> d_row0, d_nrows, d_off;
};

}  // namespace

struct lf_ctx {
    lf::KConst kc{};
    int device = 0;
    int64_t N = 0;
    int nnodes = 0;
    std::vector<int64_t> field_ind;
    std::vector<double> h_x;            // FREE: host copy of the flux-sorted logf (chunk keys are derived from it)
    Buf<unsigned long long> d_forms;         // census of the term forms (option "count_forms"), FORM_COUNT slots
    int last_launch[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // lf_last_launch
    Buf<unsigned long long> d_stamps;        // kc.stamps (LF_STAMPS builds, lf_debug_stamps)
    Buf<int> d_queue;                    // FREE: item counters of the persistent workgroups, [tiles][lf::QSTRIDE]
    // the catalogue's cells (lf_kernels.h: CELL_M, ZCELL_M) - {x_c, S_0 .. S_M} per cell, chunks of 64 (FREE) / 256 (ZEVOL) cells of one field
    Buf<double> d_cells;                 // [ncell][8]
    Buf<int> d_cc_start;                 // [ncchunk] first cell of the chunk
    Buf<int> d_deal;                     // lf_free's deal of cell chunks and flux bins to its virtual workgroups (lf_free.h: DEAL_*)
    int64_t deal_key = -1;               // ... made for this (cell chunks, bins, grid share)
    int deal_fin = lf::FIN_LAST;         // ... and who finishes a polling tile under it, per group size (lf_tile.h: tile_finisher)
    Buf<int> d_cc_len;                   // [ncchunk] cells in the chunk (<= 64)
    Buf<int> d_cc_field;                 // [ncchunk]
    int ncell = 0, ncchunk = 0;
    int64_t opt_cells = 1;               // 0: sum every walker over the sources (A/B runs)
    int slots_free[3] = {0, 0, 0};       // workgroups of lf_free<2 / 4 / 8> the chip holds at once (0 = not asked yet)
    int num_cu = 0;
    // device tables
    Buf<double> d_lum, d_a1, d_P, d_U;
    Buf<double> d_G, d_PG, d_W, d_a3, d_a4, d_a4min, d_nodes8;
    std::map<int, ChunkTable> chunks;   // keyed by sources-per-chunk
    std::map<int, ChunkTable> chunks_free;   // the persistent FREE kernel's (lf_free.h): 512 ST sources per chunk, lanes of ST
    int64_t opt_persistent = 1;         // FREE: 1 = lf_free (persistent 512-thread workgroups) for catalogues that fill it
    int64_t opt_fuse = 1;               // lf_free: prepare and finalize inside the one launch (plain evaluations)
    int64_t opt_fuse_step = 1;          // ... and the sampler's half-step too (0: three launches per half-step, A/B runs)
    bool queue_zero = false;            // d_queue is all zeros (what a fused launch needs and leaves behind)
    bool parts_empty = false;           // every slot of d_partB / d_partR is lf::PART_EMPTY (what the polling hand-over needs and leaves behind, lf_tile.h)
    Buf<int> d_err;                     // device error word (a finisher gave up polling)
    // lf_free's one-launch form reads its launch-invariant arguments from a block in device memory (lf_free.h: FreeBlock), one
    // per sources-per-lane slot (the chunk tables depend on it); the pinned shadow holds what was last uploaded: an upload
    // only when the bytes change (free_block)
    Buf<unsigned char> d_fblk[3];       // (bytes: a FreeBlock rounded up to whole 256-byte lines)
    Buf<unsigned char, true> h_fblk[3];
    bool fblk_valid[3] = {false, false, false};
    int64_t fblk_uploads = 0;           // uploads so far (lf_free_block_uploads: the tests' debug counter)
    int64_t opt_poll = 1;               // 0: the one-launch form hands over through the tile's counter only (A/B runs)
    int64_t opt_free_st = 0;            // lf_free: sources per lane, 0 = chosen from N and B, else 2 / 4 / 8 (tuning runs)
    int64_t opt_geometry = -1;          // index into GEOS, -1 = auto
    int64_t opt_walker_tile = 0;        // walkers per workgroup (<= the geometry's maximum), 0 = auto
    int64_t opt_taper = 0;              // 1: quarter-size walker tiles for the last ~1/8 of the walkers (second pass over the catalogue)
    int64_t opt_skip_grid = 0;          // 1: leave piece B out (source-sharded ranks other than the first)
    int64_t opt_compress = 0;           // 1: piece A from the compressed catalogue (FREE, ZEVOL)
    int64_t opt_compress_grid = 1;      // with compress: also the FREE integration grid, when it is separable
    CompressedCat cmp;
    // FREE: the factors of a separable integration grid (every redshift column has the same luminosity nodes),
    // kept on the host for the compressed grid; empty when the grid is not separable
    std::vector<double> h_L, h_wL, h_ck, h_Dk;
    CompressedGrid gridc;
    // FREE, separable grid: piece B over flux bins with a proven bound (lf_gridbound.h); lf_free's default when built
    struct {
        bool built = false;
        int nb = 0;
        double margin = 0.0;
        Buf<double> d_rec, d_omega;
        Buf<int> d_rows;
    } gridq;
    int64_t opt_grid_shortcut = 1;      // 0: lf_free integrates the lattice (A/B runs)
    // FIXCOMP, ZEVOL: the grid's nodes as 32-byte records {G, PG, W, column} padded to chunks of 64, and the columns' redshifts
    // (lf_pers.h: the persistent kernel of these variants)
    Buf<double> d_nodes4, d_zcol;
    int nch4 = 0;
    int slots_pers = 0;                 // workgroups of lf_pers the chip holds at once (0 = not asked yet)
    Buf<double> d_partR;                // rescue partials [B][chunks of the real catalogue]
    Buf<int> d_slow;                    // {count, walker indices...} of the walkers lf_prepare flagged SLOW (compressed mode)
    // workspace
    int cap_B = 0;                      // padded walker capacity
    Buf<double> d_theta, d_out, d_outA, d_outB;
    Buf<double> d_wrec, d_partA, d_partB;
    Buf<int> d_wstat, d_wmode;
    Buf<double> d_wbase;
    Buf<double, true> h_theta, h_out;   // pinned staging
    // the gradient (lf_grad.h): its constants, the chunks of the catalogue its source blocks and those of lf_deconv.h and
    // lf_deconv_grad.h take (made at first use), the blocks' partial sums [rows][blocks][GRAD_SLOTS], and the host forms'
    // results {value [B], grad [B][ndim]} with their pinned staging
    lf::GradConst gradc{};
    ChunkTable src_chunks;
    bool src_chunks_built = false;
    Buf<double> d_gpart, d_gout;
    Buf<double, true> h_gout;
    // the flux-error-convolved likelihood (lf_deconv.h; lf_set_lum_err): the sources' order in the device tables, whether every
    // redshift column of the grid has the same luminosity nodes, sigma (and, FIXCOMP / ZEVOL, the log flux and 10^(that + 17))
    // in that order, the node table and the blocks' partial sums [rows][chunks]
    std::vector<int64_t> perm;
    bool grid_separable = false;
    lf::DeconvConst deconvc{};
    bool deconv_set = false;
    int64_t opt_deconv_unchecked = 0;   // 1: lf_set_lum_err takes sigma above the validated range of the order (tests, A/B runs)
    int64_t opt_deconv_tile = 0;        // 1: FIXCOMP, ZEVOL: the value's first stage by tiles of rows (lf_deconv_tile.h); FREE: no effect
    Buf<double> d_sigma, d_elogf, d_eU, d_ghnodes, d_dpart;
    Buf<double> d_dgpart;               // its gradient's partial sums [rows][chunks][DGRAD_SLOTS] (lf_deconv_grad.h)
    // the wide rule (lf_deconv_wide.h): the sources above the order's limit in arrays of their own (lf_set_lum_err; their
    // entries of d_sigma are 0), their chunks, the classes' tables, and the field of every block of a row - the narrow chunks',
    // then the wide ones' (what the second stages read when n > 0)
    int64_t opt_deconv_wide = 0;        // 1: lf_set_lum_err takes sigma up to the wide rule's top edge
    struct {
        int n = 0;                      // wide chunks
        Buf<double> d_lum, d_a1, d_P, d_logf, d_U, d_sigma, d_tables;
        Buf<int> d_start, d_len, d_class, d_field_all;
        int K[lf::DECONV_WIDE_NCLASS] = {}, off[lf::DECONV_WIDE_NCLASS] = {};
    } wide;
    // the cut on the observed flux (lf_deconv_cut.h; lf_set_cut_error_model): what the tables are made from - the grid's lower
    // and upper edges per redshift column, the redshifts, and where the descriptor gave them dVc/dz/dOmega and log10(4 pi DL^2)
    // (empty: not given) - the error model, and the node tables with their chunks (n: chunks; 0 without the model, or with
    // sigma = 0 throughout)
    std::vector<double> h_edge_lo, h_edge_hi, h_zarr, h_vol, h_ld2, h_om0;
    int64_t opt_cut_limit = 0;          // > 0: only the first so many nodes of every field (tests)
    int64_t opt_cut_grad = 0;           // 1: the gradient entries of the convolved likelihood serve the cut model (lf_deconv_cut_grad.h)
    Buf<double> d_cgpart;               // the cut gradient's partial sums [rows][cut chunks][GRAD_SLOTS]
    struct {
        bool model = false, built = false;       // an error model is set; the tables are made (fixed completeness: by lf_set_lum_err)
        int M = 0;
        std::vector<double> nodes, sigma;
        int n = 0;
        int nnodes[lf::MAXF] = {};
        double H[lf::MAXF] = {};
        Buf<double> d_L, d_P, d_c, d_a3, d_a4;
        Buf<int> d_start, d_len, d_field;
    } cut;
    // the per-source posterior of the true luminosity (lf_lumpost.h): every slot's source in the caller's order - the context's
    // sources, then those of the wide list (lf_set_lum_err) - and the workspace: the slabs, the running sums, m1 and m2
    Buf<int> d_lp_caller;
    int lp_nslots = 0;
    Buf<double> d_lumpost;
    Buf<int> d_vt_inwide;               // lf_vefftrue.h: 1 for the sources of the wide list, in the device's order
    Buf<double> d_vt_work;              // lf_veff_true's workspace: edges, quantile table, partial sums, values, used rows, out
    Buf<int> d_vt_slot;                 // ... and the rows' places among the used rows
    // the catalogued volume per node under the cut (lf_vefftrue_cut.h; option "deconv_cut_veff"): the model's image, the table
    // of 1 / g per (source, node) slot - made at the first lf_veff_true call after lf_set_lum_err, for one min_vol_frac, and
    // kept until the luminosity errors, the error model or min_vol_frac change - and the chunks' dropped counts
    int64_t opt_cut_veff = 0;           // 1: lf_veff_true serves a context with the cut model
    struct {
        bool img = false, built = false;      // the image is made (per error model); the table is made
        double min_vol_frac = 0.0;
        size_t slots = 0;
        long long wide_off = 0, dropped = 0;
        double ms = -1.0;               // the table kernel's device time when it was last made under lf_set_profiling
        lf::VeffCutTab tab{};
        Buf<double> d_img, d_invg;
        Buf<int> d_drop;
    } cutv;
    hipStream_t stream = nullptr;
    hipStream_t last_stream = nullptr;   // stream of the previous enqueue (workspace is shared)
    bool any_enqueued = false;
    // profiling
    int profiling = 0;   // 0 off, 1 lf_main only, 2 every launch
    lf::ZCells zcells{};                // ZEVOL, real catalogue: the cell workgroups' arguments for the launch being enqueued (nchC = 0: none)
    int64_t opt_profile_every = 1;      // ... of every n-th evaluation only (an event pair costs the stream ~4 us: it drains the queue)
    int64_t prof_tick = 0;
    int64_t opt_profile_span = 1;       // one event pair around this many CONSECUTIVE one-launch evaluations (their average: a pair of
                                        // barrier packets around every single launch adds the dispatch to it)
    int64_t prof_pos = 0;               // this evaluation's place in its period of opt_profile_every
    bool prof_span_ok = false;          // this evaluation is one launch (spans make sense)
    bool span_open = false;
    EventPair span_ep{};
    bool prof_this = true;              // (this evaluation is one of them)
    std::vector<EventPair> events;
    double acc_ms[4] = {0, 0, 0, 0};
    int64_t acc_n[4] = {0, 0, 0, 0};
    std::string err;
};

namespace {

// upload(c, buffer, vector, buffer, vector, ...): each vector to a new allocation of its size; stops at the first error
inline int upload(lf_ctx*) { return LF_OK; }
template <typename T, typename... Rest>
int upload(lf_ctx* c, Buf<T>& dst, const std::vector<T>& src, Rest&... rest) {
    LF_HIP(c, dst.upload(src.data(), src.size()));
    return upload(c, rest...);
}

// The catalogue's cells (lf_hostprep.h: build_cells), to the device.  No cells: nothing happens (kc.cells stays 0).
int upload_cells(lf_ctx* c, const lfh::Cells& cl) {
    if (!cl.built) return LF_OK;
    const int rc = upload(c, c->d_cells, cl.rec, c->d_cc_start, cl.start, c->d_cc_len, cl.len, c->d_cc_field, cl.field);
    if (rc != LF_OK) return rc;
    c->ncell = (int)(cl.rec.size() / (c->kc.variant == LF_ZEVOL ? lf::ZCELL_REC : lf::CELL_REC));
    c->ncchunk = (int)cl.start.size();
    c->kc.cells = c->opt_cells ? 1 : 0;
    return LF_OK;
}

// The table of chunks of `ch` sources (lf_hostprep.h: chunk_table), made and uploaded when it is first asked for.
// hx: the flux-sorted logf of the REAL catalogue (FREE), or NULL (no keys: the chunks never take the table form)
int get_chunks(lf_ctx* c, std::map<int, ChunkTable>& tables, const std::vector<int64_t>& field_ind, int ch,
               ChunkTable** out, const double* hx = nullptr, int lane_w = 0) {
    auto it = tables.find(ch);
    if (it != tables.end()) {
        *out = &it->second;
        return LF_OK;
    }
    const lfh::Chunks h = lfh::chunk_table(field_ind, c->kc.nf, ch, c->kc.key_x0, lf::G_MARGIN, lf::H_MARGIN, hx, lane_w);
    ChunkTable t;
    t.n = (int)h.start.size();
    const int rc = upload(c, t.d_start, h.start, t.d_len, h.len, t.d_field, h.field, t.d_keys, h.keys);
    if (rc != LF_OK) return rc;
    *out = &tables.emplace(ch, std::move(t)).first->second;       // (only a complete table enters the map)
    return LF_OK;
}

// launch geometries of the per-source kernel: sources per lane (ST) x walkers per workgroup (TW)
struct Geo {
    int st, tw, twb;     // sources per lane, walkers per source workgroup, walkers per grid workgroup
};
// instantiated geometries; [0] and [1] are the defaults for large and small problems
constexpr Geo GEOS[] = {{8, 16, 16}, {2, 8, 2}, {8, 8, 8}, {8, 4, 4}, {4, 8, 4}, {4, 4, 4}, {6, 16, 16}, {4, 16, 16}, {2, 8, 16}};
constexpr int NGEO = sizeof(GEOS) / sizeof(GEOS[0]);

int pick_geometry(const lf_ctx* c, int B) {
    if (c->opt_geometry >= 0 && c->opt_geometry < NGEO) return (int)c->opt_geometry;
    // The big tile (2048 sources x 16 walkers) amortises loads and reductions best, but the launch wants >= ~1024
    // workgroups (4 per CU).  Below that keep the 2048-source chunks and shrink the walker tile (16 -> 8 -> 4);
    // tiny catalogues take the 512-source chunks.  (Measured at B = 128, lf_main in us, geometries 0 / 2 / 3 / 1:
    // N = 4e5: 98 / 95 / 100 / 122;  2e5: 67 / 60 / 62 / 72;  1e5: 49 / 43 / 42 / 49;  3e4: 39 / 30 / 30 / 30.)
    // Fixed completeness on a grid summed over its rows (build(): S nodes, one or two chunks): the per-source part is idle
    // and the grid part is a serial loop over a workgroup's walkers - two per workgroup instead of 16 (lf_main 14.2 -> 6.5 us
    // at 128 rows).
    if (c->kc.variant == LF_FIXCOMP && c->nnodes <= 2 * lf::BLOCK) return 1;
    const int64_t chunks = (c->N + GEOS[0].st * lf::BLOCK - 1) / (GEOS[0].st * lf::BLOCK);
    if (chunks * ((B + 15) / 16) >= 1024) return 0;
    if (chunks * ((B + 7) / 8) >= 1024) return 2;
    if (chunks * ((B + 3) / 4) >= 384) return 3;
    return 1;
}

int ensure_workspace(lf_ctx* c, int Bpad, size_t partA, size_t partB, size_t partR = 0) {
    int rc;
    if (Bpad > c->cap_B) {
        const size_t nb = (size_t)std::max(Bpad, c->cap_B * 2);
        LF_HIP(c, hipDeviceSynchronize());
        c->cap_B = 0;                    // (a failed allocation below: everything is made anew by the next call)
        LF_HIP(c, c->d_theta.alloc(nb * 16));
        LF_HIP(c, c->d_out.alloc(nb));
        LF_HIP(c, c->d_outA.alloc(nb));
        LF_HIP(c, c->d_outB.alloc(nb));
        LF_HIP(c, c->d_wrec.alloc(nb * lf::REC));
        LF_HIP(c, c->d_wstat.alloc(nb));
        LF_HIP(c, c->d_wmode.alloc(nb * lf::MAXF * lf::WM));
        LF_HIP(c, c->d_wbase.alloc(nb));
        LF_HIP(c, c->d_slow.alloc(nb + 1));
        LF_HIP(c, hipMemset(c->d_slow, 0, (nb + 1) * sizeof(int)));
        LF_HIP(c, c->h_theta.alloc(nb * 16));
        LF_HIP(c, c->h_out.alloc(nb * 3));
        c->cap_B = (int)nb;
    }
    if (partA > c->d_partA.size() && (rc = grow(c, c->d_partA, partA)) != LF_OK) return rc;
    if (partR > c->d_partR.size()) {
        if ((rc = grow(c, c->d_partR, partR)) != LF_OK) return rc;
        c->parts_empty = false;
    }
    if (partB > c->d_partB.size()) {
        if ((rc = grow(c, c->d_partB, partB)) != LF_OK) return rc;
        c->parts_empty = false;
    }
    return LF_OK;
}

struct Prof {
    lf_ctx* c;
    hipStream_t s;
    int kind;
    EventPair ep{};
    bool on, span;
    Prof(lf_ctx* c_, hipStream_t s_, int k) : c(c_), s(s_), kind(k) {
        // (option "profile_span" = n > 1, profiling level 1, one-launch evaluations: ONE pair around n consecutive launches)
        span = k == 1 && c->profiling == 1 && c->opt_profile_span > 1 && c->prof_span_ok;
        on = !span && c->prof_this && (c->profiling >= 2 || (c->profiling == 1 && k == 1));
        if (on) {
            hipEventCreate(&ep.a);
            hipEventCreate(&ep.b);
            ep.kind = kind;
            hipEventRecord(ep.a, s);
        }
        if (span && c->prof_pos == 0 && !c->span_open) {
            hipEventCreate(&c->span_ep.a);
            hipEventCreate(&c->span_ep.b);
            c->span_ep.kind = kind;
            c->span_ep.count = 0;
            hipEventRecord(c->span_ep.a, s);
            c->span_open = true;
        }
    }
    ~Prof() {
        if (on) {
            hipEventRecord(ep.b, s);
            c->events.push_back(ep);
        }
        if (span && c->span_open) {
            ++c->span_ep.count;
            if (c->span_ep.count >= std::min(c->opt_profile_span, c->opt_profile_every)) {
                hipEventRecord(c->span_ep.b, s);
                c->events.push_back(c->span_ep);
                c->span_open = false;
            }
        }
    }
};

// enqueue the three launches of one batched evaluation on `s`: prepare -> main (A and B) -> finalize
template <int VARIANT, int GI, bool CMP = false>
void launch_geo(lf_ctx* c, dim3 grid, lf::Tiling tl, int ntilesB, int twb, int nblkB, hipStream_t s,
                const lf::SrcArrays& sa, const lf::NodeArrays& na, int B, int nchA, int nchB,
                const lf::Rescue& rs = lf::Rescue{}, const lf::GridC& gc = lf::GridC{}) {
    using namespace lf;
    if (std::getenv("LF_DEBUG_OCC")) {
        int nb = -1;
        hipFuncAttributes fa{};
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, lf_main<VARIANT, GEOS[GI].st, GEOS[GI].tw, GEOS[GI].twb, CMP>, BLOCK, 0);
        hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(&lf_main<VARIANT, GEOS[GI].st, GEOS[GI].tw, GEOS[GI].twb, CMP>));
        std::fprintf(stderr, "lf_main<%d,%d,%d,%d,%d>: %d workgroups per CU (occupancy API), %d VGPRs, %zu B LDS, grid %u\n", VARIANT,
                     GEOS[GI].st, GEOS[GI].tw, GEOS[GI].twb, (int)CMP, nb, fa.numRegs, fa.sharedSizeBytes, grid.x);
    }
    ZCells zc{};
    if (!CMP && ((VARIANT == LF_ZEVOL && c->zcells.nchC > 0) || VARIANT == LF_FIXCOMP)) {
        zc = c->zcells;
        // the per-source items are shared by a bounded number of workers (lf_kernels.h: lf_main), the cell workgroups come
        // after them: (chunk, tile of TW walkers)
        const int nsrc_wg = nchA * (tl.ntiles + tl.ntiles_s);
        // (one per CU: idle workers still cost ~0.6 us per 256 of them - 20.7 / 19.8 / 18.9 us with 4 / 2 / 1 per CU at 128
        // rows - and the rare walker that needs the sources has 490 items for 256 workers)
        zc.nwork = std::min(nsrc_wg, std::max(c->num_cu, 1));
        if (zc.nwork > 0) {
            grid.x = (unsigned)(nblkB + zc.nwork + zc.nchC * ((B + GEOS[GI].tw - 1) / GEOS[GI].tw));
            c->last_launch[4] = (int)grid.x;
        }
    }
    hipLaunchKernelGGL((lf_main<VARIANT, GEOS[GI].st, GEOS[GI].tw, GEOS[GI].twb, CMP>), grid, dim3(BLOCK), 0, s, c->kc, sa,
                       na, c->d_wrec, c->d_wmode, B, tl, nchA, ntilesB, twb, nblkB, c->d_partA, nchA, c->d_partB, nchB, rs, gc, zc);
}

// compressed-catalogue launches: the pseudo-sources are few, so only the small-tile geometries are instantiated
constexpr int CMP_GEOS[] = {8, 1, 4, 2};     // [0] is the default: few sources per lane, 16 walkers per grid workgroup
template <int VARIANT>
void launch_main_cmp(lf_ctx* c, int gi, dim3 grid, lf::Tiling tl, int ntilesB, int twb, int nblkB, hipStream_t s,
                     const lf::SrcArrays& sa, const lf::NodeArrays& na, int B, int nchA, int nchB, const lf::Rescue& rs,
                     const lf::GridC& gc) {
    switch (gi) {
        case 1: launch_geo<VARIANT, 1, true>(c, grid, tl, ntilesB, twb, nblkB, s, sa, na, B, nchA, nchB, rs, gc); break;
        case 4: launch_geo<VARIANT, 4, true>(c, grid, tl, ntilesB, twb, nblkB, s, sa, na, B, nchA, nchB, rs, gc); break;
        case 2: launch_geo<VARIANT, 2, true>(c, grid, tl, ntilesB, twb, nblkB, s, sa, na, B, nchA, nchB, rs, gc); break;
        default: launch_geo<VARIANT, 8, true>(c, grid, tl, ntilesB, twb, nblkB, s, sa, na, B, nchA, nchB, rs, gc);
    }
}

template <int VARIANT>
void launch_main(lf_ctx* c, int gi, dim3 grid, lf::Tiling tl, int ntilesB, int twb, int nblkB, hipStream_t s,
                 const lf::SrcArrays& sa, const lf::NodeArrays& na, int B, int nchA, int nchB, const lf::Rescue& rs) {
    switch (gi) {
        case 0: launch_geo<VARIANT, 0>(c, grid, tl, ntilesB, twb, nblkB, s, sa, na, B, nchA, nchB, rs); break;
        case 1: launch_geo<VARIANT, 1>(c, grid, tl, ntilesB, twb, nblkB, s, sa, na, B, nchA, nchB, rs); break;
        case 2: launch_geo<VARIANT, 2>(c, grid, tl, ntilesB, twb, nblkB, s, sa, na, B, nchA, nchB, rs); break;
        case 3: launch_geo<VARIANT, 3>(c, grid, tl, ntilesB, twb, nblkB, s, sa, na, B, nchA, nchB, rs); break;
        case 4: launch_geo<VARIANT, 4>(c, grid, tl, ntilesB, twb, nblkB, s, sa, na, B, nchA, nchB, rs); break;
        case 5: launch_geo<VARIANT, 5>(c, grid, tl, ntilesB, twb, nblkB, s, sa, na, B, nchA, nchB, rs); break;
        case 6: launch_geo<VARIANT, 6>(c, grid, tl, ntilesB, twb, nblkB, s, sa, na, B, nchA, nchB, rs); break;
        case 7: launch_geo<VARIANT, 7>(c, grid, tl, ntilesB, twb, nblkB, s, sa, na, B, nchA, nchB, rs); break;
        default: launch_geo<VARIANT, 8>(c, grid, tl, ntilesB, twb, nblkB, s, sa, na, B, nchA, nchB, rs);
    }
}

// FREE variant, real catalogue, catalogues large enough to fill it: prepare -> lf_free (persistent 512-thread workgroups,
// pieces A and B, lf_free.h) -> finalize
// Source-chunk size of the persistent FREE kernel (lf_free.h), for walkers that are summed over the sources: sources per
// lane 8 (the table lookup is shared by 8 terms) once the catalogue gives 4096-source chunks enough to go round, else 4
// (measured on a warmed-up device, cells off, 128 rows, us: N = 2.5e5 58.1 -> 55.7, 1e5 45.7 -> 40.2 going from ST = 8
// to 4).  free_st overrides (tuning runs).
struct FreeShape {
    int st;
    int64_t items_per_tile;      // source chunks + grid chunks of 512 nodes' worth (the old item count: the crossover rule
                                 // for contexts without cells was measured in these units)
};
FreeShape free_shape(const lf_ctx* c) {
    using namespace lf;
    FreeShape fs;
    const int64_t chunks8 = (c->N + 8 * (int64_t)PB - 1) / (8 * (int64_t)PB);
    fs.st = c->opt_free_st ? (int)c->opt_free_st : (chunks8 >= 74 ? 8 : 4);
    const int64_t nchB = c->opt_skip_grid ? 0 : (c->nnodes + PB - 1) / PB;
    fs.items_per_tile = (c->N + (int64_t)PB * fs.st - 1) / ((int64_t)PB * fs.st) + nchB * 2;
    return fs;
}

// The number of groups of 8 workgroups (one per XCD under round-robin placement) lf_free<ST> is launched with: no more
// than the chip holds at once, no more than there are items.
template <int ST>
int free_groups(lf_ctx* c, int slot, int ntiles, int nchA, int nchB, int nchC) {
    using namespace lf;
    if (c->slots_free[slot] == 0) {
        int nb = 0;
        auto* k = static_cast<void (*)(KConst, SrcArrays, NodeArrays, const double*, const int*, FreeArgs)>(lf_free<ST, false>);
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k, PB, 0) != hipSuccess || nb < 1) nb = 1;
        c->slots_free[slot] = nb * std::max(c->num_cu, 1);
        if (std::getenv("LF_DEBUG_OCC")) {
            hipFuncAttributes at{};
            hipFuncGetAttributes(&at, reinterpret_cast<const void*>(k));
            std::fprintf(stderr, "lf_free<%d>: %d workgroups per CU (occupancy API), %d VGPRs, %zu B LDS\n", ST, nb, at.numRegs, at.sharedSizeBytes);
        }
    }
    // (at most VF workgroups per tile: the cells' and the grid's chunks are dealt to VF virtual workgroups, lf_free.h)
    const int64_t per_tile = std::min<int64_t>(VF / 8, ((int64_t)nchA + nchB + nchC + 7) / 8);
    return (int)std::max<int64_t>(1, std::min<int64_t>(c->slots_free[slot] / 8, (int64_t)ntiles * std::max<int64_t>(per_tile, 1)));
}

// lf_free's static deal (lf_hostprep.h: make_deal) with the costs of the tuning runs (tools/deal_sweep.sh), if any.  No table (the
// arithmetic deal): no bins, or more entries than the kernel keeps in LDS.
std::vector<int> make_deal(int nchC, int nbq, int grid_part, int grid_parts) {
    const char *h = std::getenv("LF_DEAL_H"), *b = std::getenv("LF_DEAL_B");
    return lfh::make_deal(nchC, nbq, grid_part, grid_parts, h ? std::atoi(h) : 8, b ? std::atoi(b) : 8);
}

// ... and the finisher ranks that go with it (lf_hostprep.h: deal_finishers), packed a byte per group size as the kernel reads them.
// A/B runs (is the computed rank the one that ends last?): LF_FIN_SHIFT moves every rank up or down, LF_FIN_RANK names it.
int deal_finishers(const std::vector<int>& t, int nchC, int nbq, int grid_part, int grid_parts) {
    const char *h = std::getenv("LF_DEAL_H"), *b = std::getenv("LF_DEAL_B"), *sh = std::getenv("LF_FIN_SHIFT"), *fr = std::getenv("LF_FIN_RANK");
    const std::array<int, 4> f = lfh::deal_finishers(t, nchC, nbq, grid_part, grid_parts, h ? std::atoi(h) : 8, b ? std::atoi(b) : 8);
    int word = 0;
    for (int g = 0; g < 4; ++g)
        word |= std::min(std::max((fr ? std::atoi(fr) : f[(size_t)g]) + (sh ? std::atoi(sh) : 0), 0), 8 * g + 7) << (8 * g);
    return word;
}

int ensure_deal(lf_ctx* c, int nchC, int nbq, hipStream_t s) {
    using namespace lf;
    const int64_t key = nbq <= 0 || DEAL_LIST + nchC + nbq > DEAL_MAX || std::getenv("LF_NO_DEAL")      // (the variable: A/B runs)
                            ? 0 : 1 + nchC + 4096ll * nbq + (4096ll * 4096) * (c->kc.grid_part + 4096ll * c->kc.grid_parts);
    if (key == c->deal_key) return LF_OK;
    if (key > 0) {
        const std::vector<int> t = make_deal(nchC, nbq, c->kc.grid_part, c->kc.grid_parts);
        if (!c->d_deal) LF_HIP(c, c->d_deal.alloc(DEAL_MAX));
        if (c->any_enqueued) LF_HIP(c, hipStreamSynchronize(c->last_stream));        // (a launch may still be reading the old table)
        LF_HIP(c, hipMemcpy(c->d_deal, t.data(), t.size() * sizeof(int), hipMemcpyHostToDevice));
        c->deal_fin = deal_finishers(t, nchC, nbq, c->kc.grid_part, c->kc.grid_parts);
    }
    c->deal_key = key;
    return LF_OK;
}

// The tiles' counters of the persistent kernels (d_queue: QSTRIDE per tile, lf_tile.h), grown to ntiles; a new buffer is not zero.
int ensure_queue(lf_ctx* c, int ntiles) {
    using namespace lf;
    if ((size_t)(ntiles * QSTRIDE) > c->d_queue.size()) {
        const int rc = grow(c, c->d_queue, (size_t)std::max(2 * ntiles * QSTRIDE, 1024));
        if (rc != LF_OK) return rc;
        c->queue_zero = false;
    }
    return LF_OK;
}

// Every evaluation, before its first launch.  The workspace is shared by consecutive calls: order a stream switch behind the
// previous work.  Then the evaluation's place in the profile (one_launch: spans make sense).
int begin_enqueue(lf_ctx* c, hipStream_t s, bool one_launch) {
    if (c->any_enqueued && c->last_stream != s) LF_HIP(c, hipStreamSynchronize(c->last_stream));
    c->last_stream = s;
    c->any_enqueued = true;
    c->prof_pos = c->prof_tick++ % c->opt_profile_every;
    c->prof_this = c->profiling > 0 && c->prof_pos == 0;
    c->prof_span_ok = one_launch;
    return LF_OK;
}

// What the one-launch form's hand-over (lf_tile.h) finds before the launch.  The tiles' counters start at zero: a fused launch
// leaves them so, lf_prepare zeroes them for the three-launch form.  The polling hand-over (PART_EMPTY) wants every slot of
// the two partial-sum buffers empty: a fused launch leaves them so, every other form leaves sums behind.
int ready_tiles(lf_ctx* c, hipStream_t s, bool fused, bool poll) {
    using namespace lf;
    if (fused && !c->queue_zero) {
        LF_HIP(c, hipMemsetAsync(c->d_queue, 0, c->d_queue.size() * sizeof(int), s));
        c->queue_zero = true;
    }
    if (poll && !c->parts_empty) {
        static_assert((PART_EMPTY >> 32) == (PART_EMPTY & 0xffffffffull), "filled by 32-bit words");
        LF_HIP(c, hipMemsetD32Async((hipDeviceptr_t)c->d_partB, (int)(PART_EMPTY & 0xffffffffull), c->d_partB.size() * 2, s));
        LF_HIP(c, hipMemsetD32Async((hipDeviceptr_t)c->d_partR, (int)(PART_EMPTY & 0xffffffffull), c->d_partR.size() * 2, s));
        if (!c->d_err) {
            LF_HIP(c, c->d_err.alloc(1));
            LF_HIP(c, hipMemsetAsync(c->d_err, 0, sizeof(int), s));
        }
        c->parts_empty = true;
    }
    if (!poll) c->parts_empty = false;
    return LF_OK;
}

// The one-launch lf_free's block (lf_free.h: FreeBlock) of this slot, made anew at every enqueue and uploaded only when its bytes
// differ from the shadow's: the first use, a reallocated buffer (ensure_workspace / ensure_queue / ensure_deal), an option
// that changes KConst or FreeArgs (cells, tables, specialise, grid_shortcut, skip_grid, poll, the stamps pointer).  The copy
// is ordered on the launch's stream, like the launch (legal under stream capture); the shadow it reads from is not rewritten
// before that copy is done.  The block's per-launch fields are zero: the kernel takes them from its FreeLaunch.
int free_block(lf_ctx* c, int slot, const lf::SrcArrays& sa, const lf::NodeArrays& na, const lf::FreeArgs& fa, hipStream_t s) {
    using namespace lf;
    // The bytes are compared, padding included: the block is zeroed and filled member by member (a copy of a whole struct made
    // on the stack would bring its padding's garbage along - and an upload with every call).  c->kc is zero-initialised with
    // the context and only ever written member by member.
    FreeBlock b;
    std::memset(&b, 0, sizeof(b));
    std::memcpy(&b.kc, &c->kc, sizeof(KConst));
    b.sa = sa;                          // (pointers only: no padding)
    static_assert(sizeof(SrcArrays) == 10 * sizeof(void*), "SrcArrays has no padding");
    b.na.G = na.G, b.na.PG = na.PG, b.na.W = na.W, b.na.a3 = na.a3, b.na.a4 = na.a4, b.na.a4min = na.a4min, b.na.nnodes = na.nnodes;
    FreeArgs& d = b.fa;                 // (theta, out, B, ntiles, tile_stride stay zero: the kernel takes them from its FreeLaunch)
    d.nchA = fa.nchA, d.nchB = fa.nchB, d.nslot = fa.nslot, d.skip_grid = fa.skip_grid;
    d.queues = fa.queues, d.partA = fa.partA, d.partB = fa.partB, d.cells = fa.cells, d.nodes8 = fa.nodes8, d.deal = fa.deal;
    d.cc_len = fa.cc_len, d.cc_field = fa.cc_field, d.nchC = fa.nchC, d.fin_ranks = fa.fin_ranks, d.partC = fa.partC, d.wstat = fa.wstat;
    d.wrec_w = fa.wrec_w, d.wmode_w = fa.wmode_w, d.wstat_w = fa.wstat_w, d.wbase_w = fa.wbase_w;
    d.gq_rec = fa.gq_rec, d.gq_omega = fa.gq_omega, d.gq_rows = fa.gq_rows, d.nbq = fa.nbq, d.poll = fa.poll, d.err = fa.err;
    static_assert(sizeof(FreeArgs) == 208 && sizeof(NodeArrays) == 56, "a field was added: copy it above");
    if (c->fblk_valid[slot] && std::memcmp(c->h_fblk[slot], &b, sizeof(b)) == 0) return LF_OK;
    constexpr size_t bytes = (sizeof(FreeBlock) + 255) / 256 * 256;
    if (!c->d_fblk[slot]) {
        LF_HIP(c, c->d_fblk[slot].alloc(bytes));
        LF_HIP(c, c->h_fblk[slot].alloc(bytes));
    } else {
        // the previous upload may still be reading the shadow (nothing to wait for inside a capture: it began on an idle device)
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        LF_HIP(c, hipStreamIsCapturing(s, &cs));
        if (cs == hipStreamCaptureStatusNone) LF_HIP(c, hipStreamSynchronize(s));
    }
    std::memcpy(c->h_fblk[slot], &b, sizeof(b));
    LF_HIP(c, hipMemcpyAsync(c->d_fblk[slot], c->h_fblk[slot], sizeof(b), hipMemcpyHostToDevice, s));
    c->fblk_valid[slot] = true;
    ++c->fblk_uploads;
    return LF_OK;
}

template <int ST>
void launch_free(lf_ctx* c, int slot, int B, int ntiles, const lf::SrcArrays& sa, const lf::NodeArrays& na, lf::FreeArgs fa, hipStream_t s,
                 bool fused, const lf::StepArgs* sp = nullptr, const lf::AcceptArgs* ap = nullptr) {
    // (fa.nslot is set by the caller from free_groups(), which is also what the grid is made of here; fused without sp: the
    // caller has brought the slot's block up to date, free_block)
    using namespace lf;
    const dim3 grid((unsigned)(8 * fa.tile_stride));
    const int info[8] = {ST, PTW, PTW, fused ? 3 : 2, (int)grid.x, fa.nchA, fa.nchB, B};
    std::memcpy(c->last_launch, info, sizeof(info));
    if (fused && sp) hipLaunchKernelGGL((lf_free_step<ST>), grid, dim3(PB), 0, s, c->kc, sa, na, fa, *sp, *ap);      // the sampler's half-step
    else if (fused)
        hipLaunchKernelGGL((lf_free<ST, false, true>), grid, dim3(PB), 0, s, (FreeBlockPtr)(const FreeBlock*)c->d_fblk[slot].get(),
                           FreeLaunch{fa.theta, fa.out, fa.B, fa.ntiles, fa.tile_stride});
    else if (c->kc.forms) hipLaunchKernelGGL((lf_free<ST, true>), grid, dim3(PB), 0, s, c->kc, sa, na, c->d_wrec, c->d_wmode, fa);
    else hipLaunchKernelGGL((lf_free<ST, false>), grid, dim3(PB), 0, s, c->kc, sa, na, c->d_wrec, c->d_wmode, fa);
}

int enqueue_free(lf_ctx* c, const double* d_theta, int B, double* d_out, double* d_outA, double* d_outB, hipStream_t s,
                 const lf::StepArgs& sp, const lf::AcceptArgs& ap) {
    using namespace lf;
    const int ntiles = (B + PTW - 1) / PTW;
    const FreeShape fs = free_shape(c);
    const int st = fs.st, slot = fs.st == 8 ? 2 : (fs.st == 4 ? 1 : 0);
    ChunkTable* ct = nullptr;
    int rc = get_chunks(c, c->chunks_free, c->field_ind, PB * st, &ct, c->h_x.data(), st);
    if (rc != LF_OK) return rc;
    const int nchA = ct->n;
    const bool gq = c->gridq.built && c->opt_grid_shortcut && !c->opt_skip_grid;      // piece B over flux bins (one bin per chunk)
    const int nchB = c->opt_skip_grid ? 0 : (gq ? c->gridq.nb : (c->nnodes + 63) / 64);        // chunks of 64 nodes: a wave's lanes
    const int nchC = c->kc.cells ? c->ncchunk : 0;
    const int g8 = st == 8 ? free_groups<8>(c, slot, ntiles, nchA, nchB, nchC)
                 : st == 4 ? free_groups<4>(c, slot, ntiles, nchA, nchB, nchC) : free_groups<2>(c, slot, ntiles, nchA, nchB, nchC);
    // the grid's and the cells' partial sums: one per (walker, workgroup serving the walker's tile)
    const int nslot = VF;                  // one per (walker, VIRTUAL workgroup of its tile): independent of the batch
    rc = ensure_workspace(c, B, (size_t)B * std::max(nchA, 1), (size_t)B * nslot, (size_t)B * nslot);
    if (rc != LF_OK) return rc;
    if ((rc = ensure_deal(c, nchC, gq ? c->gridq.nb : 0, s)) != LF_OK) return rc;
    if ((rc = ensure_queue(c, ntiles)) != LF_OK) return rc;
    // One launch instead of three (lf_free.h: FUSED) for the plain evaluation; the sampler's propose / accept steps, the
    // two-piece diagnostics, the census and the profile of every launch keep lf_prepare and lf_finalize.
    // ... and so is the sampler's half-step (proposal in the prologue, accept / reject by the tile's finishing workgroup)
    const bool stepf = sp.enabled && ap.enabled && c->opt_fuse_step;
    const bool fused = c->opt_fuse && (stepf || (!sp.enabled && !ap.enabled)) && !d_outA && !d_outB && d_out && !c->kc.forms && c->profiling < 2 &&
                       nchA + nchB > 0;
    const bool poll = fused && c->opt_poll && nslot <= 64;
    if ((rc = begin_enqueue(c, s, fused)) != LF_OK || (rc = ready_tiles(c, s, fused, poll)) != LF_OK) return rc;
    if (!fused) {
        c->queue_zero = false;
        Prof p(c, s, 0);
        hipLaunchKernelGGL(lf_prepare, dim3((B + 7) / 8), dim3(64), 0, s, c->kc, sp, d_theta, B, c->d_wrec,
                           c->d_wstat, c->d_wmode, c->d_wbase, (int*)nullptr, c->d_queue, ntiles * QSTRIDE);
    }
    const SrcArrays sa{c->d_lum, c->d_a1, c->d_P, c->d_U, nullptr, ct->d_start, ct->d_len, ct->d_field, ct->d_keys, nullptr};
    const NodeArrays na{c->d_G, c->d_PG, c->d_W, c->d_a3, c->d_a4, c->d_a4min, c->nnodes};
    FreeArgs fa{B, ntiles, nchA, nchB, nslot, g8, (int)c->opt_skip_grid, c->d_queue, c->d_partA, c->d_partB,
                c->d_cells, c->d_nodes8, c->deal_key > 0 ? c->d_deal : nullptr, c->d_cc_len, c->d_cc_field, nchC,
                poll && c->deal_key > 0 ? c->deal_fin : FIN_LAST, c->d_partR, c->d_wstat,
                d_theta, d_out, c->d_wrec, c->d_wmode, c->d_wstat, c->d_wbase,
                gq ? c->gridq.d_rec : nullptr, gq ? c->gridq.d_omega : nullptr, gq ? c->gridq.d_rows : nullptr, gq ? c->gridq.nb : 0,
                poll ? 1 : 0, c->d_err};
    if (fused && !stepf && (rc = free_block(c, slot, sa, na, fa, s)) != LF_OK) return rc;      // (outside the launch's event pair)
    {
        Prof p(c, s, 1);
        if (nchA + nchB > 0) {
            const StepArgs* psp = fused && stepf ? &sp : nullptr;
            if (st == 8) launch_free<8>(c, slot, B, ntiles, sa, na, fa, s, fused, psp, &ap);
            else if (st == 4) launch_free<4>(c, slot, B, ntiles, sa, na, fa, s, fused, psp, &ap);
            else launch_free<2>(c, slot, B, ntiles, sa, na, fa, s, fused, psp, &ap);
        }
    }
    if (!fused) {
        Prof p(c, s, 3);
        const int nB = nchB > 0 ? nslot : 0, nC = nchC > 0 ? nslot : 0;
        hipLaunchKernelGGL(lf_finalize, dim3(B), dim3(64), 0, s, c->d_partA, nchA, nchA, c->d_partB, nB, nB,
                           nC > 0 ? (const double*)c->d_partR : (const double*)nullptr, nC, (int)STAT_CELLS, c->d_wstat, c->d_wbase, B, ap,
                           d_out, d_outA, d_outB, (int*)nullptr, 0);
    }
    LF_HIP(c, hipGetLastError());
    return LF_OK;
}

// The z-evolving and fixed-completeness variants in persistent workgroups (lf_pers.h): one launch for a plain evaluation,
// lf_prepare / lf_pers / lf_finalize for the sampler's steps and the two-piece diagnostics.
template <int VARIANT>
int enqueue_pers_v(lf_ctx* c, const double* d_theta, int B, double* d_out, double* d_outA, double* d_outB, hipStream_t s,
                   const lf::StepArgs& sp, const lf::AcceptArgs& ap) {
    using namespace lf;
    const int ntiles = (B + PTW - 1) / PTW;
    if (c->slots_pers == 0) {
        int nb = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, lf_pers<VARIANT, true>, PB, 0) != hipSuccess || nb < 1) nb = 1;
        c->slots_pers = std::min(nb, 2) * std::max(c->num_cu, 1);      // (two per CU: what the kernel is sized for)
    }
    const int nchB = c->opt_skip_grid ? 0 : c->nch4;
    const int nchC = VARIANT == LF_ZEVOL && c->kc.cells ? (c->ncell + 63) / 64 : 0;
    // groups of 8 workgroups: no more than the chip holds at once, no more than there is work for
    const int64_t per_tile = std::max<int64_t>(1, std::min<int64_t>(VF / 8, ((int64_t)nchB + nchC + 7) / 8));
    const int g8 = (int)std::max<int64_t>(1, std::min<int64_t>(c->slots_pers / 8, (int64_t)ntiles * per_tile));
    const int nslot = VF;                  // one per (walker, VIRTUAL workgroup of its tile), lf_free.h
    int rc = ensure_workspace(c, B, (size_t)B * nslot, (size_t)B * nslot, (size_t)B * nslot);
    if (rc != LF_OK) return rc;
    if ((rc = ensure_queue(c, ntiles)) != LF_OK) return rc;
    const bool stepf = sp.enabled && ap.enabled && c->opt_fuse_step;       // the sampler's half-step: one launch too
    const bool fused = c->opt_fuse && (stepf || (!sp.enabled && !ap.enabled)) && !d_outA && !d_outB && d_out && c->profiling < 2;
    const bool poll = fused && c->opt_poll;       // (lf_tile.h: PART_EMPTY)
    if ((rc = begin_enqueue(c, s, fused)) != LF_OK || (rc = ready_tiles(c, s, fused, poll)) != LF_OK) return rc;
    if (!fused) {
        Prof p(c, s, 0);
        hipLaunchKernelGGL(lf_prepare, dim3((B + 7) / 8), dim3(64), 0, s, c->kc, sp, d_theta, B, c->d_wrec,
                           c->d_wstat, c->d_wmode, c->d_wbase, (int*)nullptr, c->d_queue, 0);
    }
    const PersArgs pa{B, ntiles, nchB, nchC, c->ncell, nslot, g8, c->d_queue, c->d_partA, c->d_partB, c->d_partR, c->d_nodes4, c->d_zcol,
                      c->d_cells, c->d_lum, c->d_a1, c->d_P, c->d_U, d_theta, d_out, c->d_wrec, c->d_wmode, c->d_wstat, poll ? 1 : 0, c->d_err};
    {
        Prof p(c, s, 1);
        const dim3 grid((unsigned)(8 * g8));
        const int info[8] = {0, PTW, PTW, fused ? 5 : 4, (int)grid.x, nchC, nchB, B};
        std::memcpy(c->last_launch, info, sizeof(info));
        if (fused && stepf) hipLaunchKernelGGL((lf_pers_step<VARIANT>), grid, dim3(PB), 0, s, c->kc, pa, sp, ap);
        else if (fused) hipLaunchKernelGGL((lf_pers<VARIANT, true>), grid, dim3(PB), 0, s, c->kc, pa);
        else hipLaunchKernelGGL((lf_pers<VARIANT, false>), grid, dim3(PB), 0, s, c->kc, pa);
    }
    if (!fused) {
        Prof p(c, s, 3);
        hipLaunchKernelGGL(lf_finalize, dim3(B), dim3(64), 0, s, c->d_partA, nslot, nslot, c->d_partB, nchB > 0 ? nslot : 0, nslot,
                           nchC > 0 ? (const double*)c->d_partR : (const double*)nullptr, nchC > 0 ? nslot : 0, (int)STAT_CELLS, c->d_wstat,
                           c->d_wbase, B, ap, d_out, d_outA, d_outB, (int*)nullptr, VARIANT == LF_FIXCOMP ? (int)STAT_SLOW : 0);
    }
    LF_HIP(c, hipGetLastError());
    return LF_OK;
}

int enqueue(lf_ctx* c, const double* d_theta, int B, double* d_out, double* d_outA, double* d_outB,
            hipStream_t s, const lf::StepArgs* step = nullptr, const lf::AcceptArgs* accept = nullptr) {
    using namespace lf;
    StepArgs sp{};
    AcceptArgs ap{};
    if (step) sp = *step;
    if (accept) ap = *accept;
    // the persistent kernel takes the free variant's direct path whenever the catalogue can fill it and no launch
    // geometry of lf_main was asked for explicitly
    // (source-sharded ranks whose piece B goes over flux bins split the BINS: every rank must then be in lf_free, whatever
    // the size of its shard - lf_main has no bins)
    const bool shared_bins = c->kc.variant == LF_FREE && c->kc.grid_parts > 1 && c->gridq.built && c->opt_grid_shortcut && !c->opt_skip_grid;
    if (c->kc.variant == LF_FREE && c->opt_persistent && c->opt_geometry < 0 && c->opt_walker_tile == 0 && !c->opt_taper &&
        !(c->opt_compress && c->cmp.built) && (c->N >= 8192 || c->kc.cells || c->opt_persistent == 2 || shared_bins)) {
        // Measured crossover (tools/time_parts.py on a warmed-up device, lf_main / lf_free in us; 128 rows: N = 5e4 33 / 37,
        // 7e4 36 / 38, 1e5 40 / 40, 1.8e5 49 / 49, 2.5e5 60 / 56, 5e5 95 / 72, 1e6 168 / 112; N = 1e6 with 16 / 32 / 64 /
        // 256 rows: 29 / 79, 50 / 56, 91 / 72, 327 / 205; N = 1e5 with 512 rows: 127 / 120): the persistent kernel wins
        // once every one of its ~512 workgroups gets about four items or more; below that its coarse items cost more
        // than its tables save.  opt_persistent = 2 or an explicit free_st force it (tests, tuning runs).
        // With the catalogue's cells (the normal case) piece A costs next to nothing and the kernel takes 22-34 us up to
        // 128 rows whatever N is (the grid integral): it wins from N x rows ~ 1e7 (lf_main / lf_free, 128 rows: N = 5e4
        // 32 / 34, 1e5 40 / 33, 2.5e5 60 / 33; N = 1e6 with 16 / 32 / 64 rows: 30 / 24, 50 / 25, 94 / 30; N = 1e5 with
        // 32 / 512 rows: 16 / 25, 126 / 88).  A plain evaluation is ONE launch in lf_free against three: the period of
        // back-to-back evaluations (tools/sweep_small.sh, lf_main / lf_free in us, 128 rows: N = 1e4 29.3 / 26.1, 3e4 37.0 /
        // 26.4, 7.8e4 44.4 / 26.9; 16 rows, where the Python caller binds both: 17-18 / 18.5-18.9) moves the crossover
        // down to N x rows ~ 1.2e6 from 32 rows.
        const int64_t ntiles = (B + PTW - 1) / PTW;
        const int64_t items = free_shape(c).items_per_tile * ntiles;
        // (an evaluation over cells costs 12-18 us whatever N and B are: always - the sampler's steps and the diagnostics
        // included, so that a row has the same bits whichever entry point evaluates it)
        const bool wins = c->kc.cells ? true : items >= 4 * 2 * (int64_t)std::max(c->num_cu, 1);
        if (wins || shared_bins || c->opt_persistent == 2 || c->opt_free_st)
            return enqueue_free(c, d_theta, B, d_out, d_outA, d_outB, s, sp, ap);
    }
    // z-evolving (with its cells, grid by columns) and fixed completeness: the persistent kernel of lf_pers.h, unless a launch
    // geometry of lf_main was asked for, the census is on (its counters live in lf_main), or the catalogue is compressed
    if (c->kc.variant != LF_FREE && c->opt_persistent && c->opt_geometry < 0 && c->opt_walker_tile == 0 && !c->opt_taper &&
        !(c->opt_compress && c->cmp.built) && !c->kc.forms && c->d_nodes4 &&
        (c->kc.variant == LF_FIXCOMP || (c->kc.cells && c->kc.zgrid_cols && c->kc.S <= PERS_MAXS))) {
        return c->kc.variant == LF_FIXCOMP ? enqueue_pers_v<LF_FIXCOMP>(c, d_theta, B, d_out, d_outA, d_outB, s, sp, ap)
                                           : enqueue_pers_v<LF_ZEVOL>(c, d_theta, B, d_out, d_outA, d_outB, s, sp, ap);
    }
    c->parts_empty = false;           // (lf_main leaves sums in the partial-sum buffers: the polling hand-over refills them)
    // compressed catalogue: piece A over the weighted pseudo-sources, plus rescue workgroups over the real one
    const bool cmp = c->opt_compress && c->cmp.built && c->kc.variant != LF_FIXCOMP;
    int gi = pick_geometry(c, B);
    if (cmp) {
        bool ok = false;
        for (int g : CMP_GEOS) ok = ok || g == gi;
        if (!ok || c->opt_geometry < 0) gi = CMP_GEOS[0];
    }
    const Geo geo = GEOS[gi];
    ChunkTable *ct = nullptr, *ctd = nullptr;
    // (ZEVOL, real catalogue: the chunk keys carry the widest lane of z-neighbours, lane = geo.st consecutive sources -
    // what the local form of the term needs to know, lf_kernels.h: srcsum_body)
    const double* hz = c->kc.variant == LF_ZEVOL && !c->h_x.empty() ? c->h_x.data() : nullptr;
    int rc = cmp ? get_chunks(c, c->cmp.chunks, c->cmp.field_ind, geo.st * BLOCK, &ct)
                 : get_chunks(c, c->chunks, c->field_ind, geo.st * BLOCK, &ct, hz, hz ? geo.st : 0);
    if (rc != LF_OK) return rc;
    if (cmp && (rc = get_chunks(c, c->chunks, c->field_ind, geo.st * BLOCK, &ctd, hz, hz ? geo.st : 0)) != LF_OK) return rc;
    const int nchA = ct->n;
    const int nchD = cmp ? ctd->n : 0;
    // rescue workgroups leave at once unless a walker was flagged; still, each costs a dispatch slot: scale with B
    const int nresc = cmp ? std::min(nchD, std::min(1024, std::max(128, 2 * B))) : 0;
    // (the compressed grid's chunks are bins of its own: ranks that split piece B keep to the lattice's granules)
    const bool cgrid = cmp && c->gridc.built && c->opt_compress_grid && !c->opt_skip_grid && c->kc.grid_parts <= 1;
    const int nchB = c->opt_skip_grid ? 0 : (cgrid ? (c->gridc.nb + 15) / 16 : (c->nnodes + BLOCK - 1) / BLOCK);
    // ZEVOL on the real catalogue: walkers lf_prepare flags STAT_CELLS are summed over the cells in redshift (partR)
    const int nchC = !cmp && c->kc.variant == LF_ZEVOL && c->kc.cells ? c->ncchunk : 0;
    rc = ensure_workspace(c, B, (size_t)B * std::max(nchA, 1), (size_t)B * std::max(nchB, 1), (size_t)B * std::max(nchD, nchC));
    if (rc != LF_OK) return rc;
    c->zcells = ZCells{c->d_cells, c->d_cc_start, c->d_cc_len, c->d_cc_field, nchC, c->d_partR, c->d_wstat, 0};
    if ((rc = begin_enqueue(c, s, false)) != LF_OK) return rc;

    {
        Prof p(c, s, 0);
        hipLaunchKernelGGL(lf_prepare, dim3((B + 7) / 8), dim3(64), 0, s, c->kc, sp, d_theta, B, c->d_wrec,
                           c->d_wstat, c->d_wmode, c->d_wbase, cmp ? c->d_slow : nullptr, c->d_queue, 0);
    }
    const SrcArrays sd{c->d_lum, c->d_a1, c->d_P, c->d_U, nullptr, ct->d_start, ct->d_len, ct->d_field, ct->d_keys, c->d_queue};
    SrcArrays sa = sd;
    Rescue rs{};
    GridC gc{};
    if (cgrid) {
        const auto& g = c->gridc;
        gc = GridC{g.d_U, g.d_A4, g.d_row0, g.d_nrows, g.d_off, g.d_omega, g.d_L, g.d_PGL, g.nb, c->kc.S};
    }
    if (cmp) {
        sa = SrcArrays{c->cmp.d_lum, c->cmp.d_a1, c->cmp.d_lum, c->cmp.d_U, c->cmp.d_W, ct->d_start, ct->d_len, ct->d_field, ct->d_keys, nullptr};
        rs.sd = sd;
        rs.sd.chunk_start = ctd->d_start;
        rs.sd.chunk_len = ctd->d_len;
        rs.sd.chunk_field = ctd->d_field;
        rs.sd.chunk_keys = ctd->d_keys;
        rs.slow_count = c->d_slow;
        rs.slow_list = c->d_slow + 1;
        rs.partR = c->d_partR;
        rs.nchD = nchD;
        rs.nresc = nresc;
    }
    NodeArrays na{c->d_G, c->d_PG, c->d_W, c->d_a3, c->d_a4, c->d_a4min, c->nnodes};
    {
        Prof p(c, s, 1);
        int tw = geo.tw, twb = geo.twb;
        if (cmp && nchB > 0) {
            // the grid integral is all the work there is: walkers per grid workgroup such that the launch
            // still has ~2000 workgroups (8 per CU), as many as the instantiation allows otherwise
            // (the compressed grid has only a few bin groups, each workgroup little work per walker: fewer, fatter ones)
            const int64_t want = cgrid ? 768 : 2048;
            int t = 1;
            while (t < geo.twb && (int64_t)nchB * ((B + 2 * t - 1) / (2 * t)) >= want) t *= 2;
            twb = t;
        }
        if (cmp && nchA > 0) {
            // the pseudo-sources are a handful of chunks: per workgroup the walker loop is a chain of dependent
            // terms (latency, not issue), so small batches get few walkers per workgroup and many workgroups
            int t = 1;
            while (t < geo.tw && (int64_t)nchA * ((B + 2 * t - 1) / (2 * t)) >= 1024) t *= 2;
            tw = t;
        }
        if (c->opt_walker_tile > 0) {
            tw = (int)std::min<int64_t>(c->opt_walker_tile, geo.tw);
            twb = (int)std::min<int64_t>(c->opt_walker_tile, geo.twb);
        }
        // tapered tiling: the last ~1/8 of the walkers go in quarter-size tiles that are dispatched last
        Tiling tl{tw, 0, B, std::max(1, tw / 4), 0};
        if (c->opt_taper && !cmp && B >= 2 * tw && tw >= 4) {
            const int tail = std::max(tw, ((B / 8 + tw - 1) / tw) * tw);       // whole big tiles' worth of walkers
            tl.B1 = ((B - tail) / tw) * tw;
        }
        tl.ntiles = (tl.B1 + tw - 1) / tw;
        tl.ntiles_s = (B - tl.B1 + tl.tws - 1) / tl.tws;
        const int ntilesB = (B + twb - 1) / twb;
        const int nblkB = nchB * ntilesB;
        // 1-D grid: B items, big A items, small A items, rescue workgroups
        dim3 grid((unsigned)(nblkB + nchA * (tl.ntiles + tl.ntiles_s) + nresc));
        const int info[8] = {geo.st, geo.tw, geo.twb, cmp ? 1 : 0, (int)grid.x, nchA, nchB, B};
        std::memcpy(c->last_launch, info, sizeof(info));
        if (grid.x > 0) {
            if (cmp) {
                if (c->kc.variant == LF_FREE) launch_main_cmp<LF_FREE>(c, gi, grid, tl, ntilesB, twb, nblkB, s, sa, na, B, nchA, nchB, rs, gc);
                else launch_main_cmp<LF_ZEVOL>(c, gi, grid, tl, ntilesB, twb, nblkB, s, sa, na, B, nchA, nchB, rs, gc);
            } else switch (c->kc.variant) {
                case LF_FREE: launch_main<LF_FREE>(c, gi, grid, tl, ntilesB, twb, nblkB, s, sa, na, B, nchA, nchB, rs); break;
                case LF_FIXCOMP: launch_main<LF_FIXCOMP>(c, gi, grid, tl, ntilesB, twb, nblkB, s, sa, na, B, nchA, nchB, rs); break;
                default: launch_main<LF_ZEVOL>(c, gi, grid, tl, ntilesB, twb, nblkB, s, sa, na, B, nchA, nchB, rs);
            }
        }
    }
    {
        Prof p(c, s, 3);
        hipLaunchKernelGGL(lf_finalize, dim3(B), dim3(64), 0, s, c->d_partA, nchA, nchA, c->d_partB, nchB, nchB,
                           cmp || nchC > 0 ? c->d_partR : nullptr, cmp ? nchD : nchC, (int)(cmp ? STAT_SLOW : STAT_CELLS), c->d_wstat,
                           c->d_wbase, B, ap, d_out, d_outA, d_outB, cmp ? c->d_slow : nullptr,
                           !cmp && c->kc.variant == LF_FIXCOMP && nchA > 0 ? (int)STAT_SLOW : 0);
    }
    LF_HIP(c, hipGetLastError());
    return LF_OK;
}

// The three families below (lf_grad.h, lf_deconv.h, lf_deconv_grad.h) launch a part kernel on a grid (blocks, rows) and a
// second stage on (rows), the context's variant as the template argument.  A grid's second dimension holds 65 535 rows:
// launch(V, b0, nb) for rows [b0, b0 + nb) in chunks of 32 768, V the variant as a std::integral_constant.
template <class F>
void launch_rows(int variant, int B, F launch) {
    const auto rows = [&](auto v) {
        for (int b0 = 0; b0 < B; b0 += 32768) launch(v, b0, std::min(32768, B - b0));
    };
    switch (variant) {
        case LF_FREE: rows(std::integral_constant<int, LF_FREE>{}); break;
        case LF_FIXCOMP: rows(std::integral_constant<int, LF_FIXCOMP>{}); break;
        default: rows(std::integral_constant<int, LF_ZEVOL>{});
    }
}

// the chunks of the catalogue that the three families' source blocks take, made and uploaded at first use
static_assert(lf::GRAD_CH == lf::DECONV_CH, "lf_grad_part and the lf_deconv*_part kernels share one chunk table");
int src_chunk_table(lf_ctx* c) {
    if (c->src_chunks_built) return LF_OK;
    const lfh::Chunks h = lfh::chunk_table(c->field_ind, c->kc.nf, lf::GRAD_CH, 0.0, 0.0, 0.0);
    ChunkTable& t = c->src_chunks;
    t.n = (int)h.start.size();
    const int rc = upload(c, t.d_start, h.start, t.d_len, h.len, t.d_field, h.field);
    if (rc != LF_OK) return rc;
    c->src_chunks_built = true;
    return LF_OK;
}

// The gradient of lnprob for B rows (lf_grad.h): the lnprob path itself first (d_lnp: what lf_lnprob_batch_device gives, and what
// decides which rows get NaN), then the blocks' partial sums and the rows' second stage, all on `s`.
int enqueue_grad(lf_ctx* c, const double* d_theta, int B, double* d_lnp, double* d_grad, hipStream_t s) {
    using namespace lf;
    int rc;
    if ((rc = src_chunk_table(c)) != LF_OK) return rc;
    const ChunkTable& t = c->src_chunks;
    const int nchA = t.n;
    const int nchB = (c->nnodes + GRAD_CH - 1) / GRAD_CH;
    const int nfB = c->kc.variant == LF_FREE ? c->kc.nf : 1;
    const int nblk = nchA + nchB * nfB;
    const size_t need = (size_t)B * std::max(nblk, 1) * GRAD_SLOTS;
    if (need > c->d_gpart.size() && (rc = grow(c, c->d_gpart, need)) != LF_OK) return rc;
    if ((rc = enqueue(c, d_theta, B, d_lnp, nullptr, nullptr, s)) != LF_OK) return rc;
    const GradArgs ga{c->gradc, d_theta, d_lnp, c->d_gpart, d_grad, c->d_lum, c->d_a1, c->d_P, c->d_U, t.d_start, t.d_len, t.d_field,
                      c->d_G, c->d_PG, c->d_W, c->d_a3, c->d_a4, c->nnodes, nchA, nchB, nfB};
    launch_rows(c->kc.variant, B, [&](auto v, int b0, int nb) {
        GradArgs g = ga;
        g.theta += (size_t)b0 * g.gc.ndim;
        g.lnprob += b0;
        g.part += (size_t)b0 * nblk * GRAD_SLOTS;
        g.grad += (size_t)b0 * g.gc.ndim;
        if (nblk > 0) hipLaunchKernelGGL(lf_grad_part<v()>, dim3((unsigned)nblk, (unsigned)nb), dim3(BLOCK), 0, s, g);
        hipLaunchKernelGGL(lf_grad_final<v()>, dim3((unsigned)nb), dim3(64), 0, s, g);
    });
    LF_HIP(c, hipGetLastError());
    return LF_OK;
}

// what the entry points of the three families refuse before the device is touched; err: those of the convolved likelihood
int family_check(lf_ctx* c, const char* fn, bool err, const void* theta, int B, const void* out) {
    if (!c) return LF_ERR_ARG;
    if (!theta || !out || B <= 0) {
        c->err = std::string(fn) + ": NULL pointer or B <= 0";
        return LF_ERR_ARG;
    }
    if (err && !c->deconv_set) {
        c->err = std::string(fn) + ": no luminosity errors set (call lf_set_lum_err first)";
        return LF_ERR_ARG;
    }
    if (c->opt_skip_grid || c->kc.grid_parts > 1) {
        c->err = std::string(fn) + ": no " + (err ? "convolved likelihood" : "gradient") +
                 " of a source-sharded context (options skip_grid, grid_share)";
        return LF_ERR_ARG;
    }
    return LF_OK;
}

// what stays refused on a context with the cut model (lf_set_cut_error_model), with what is missing
int cut_refuse(lf_ctx* c, const char* fn, const char* missing) {
    if (!c->cut.model) return LF_OK;
    c->err = std::string(fn) + ": not under a cut on the observed flux (lf_set_cut_error_model): " + missing;
    return LF_ERR_ARG;
}

// the cut gradient's partial sums for B rows (lf_deconv_cut_grad.h)
int cut_grad_workspace(lf_ctx* c, int B) {
    const size_t need = (size_t)B * std::max(c->cut.n, 1) * lf::GRAD_SLOTS;
    return need > c->d_cgpart.size() ? grow(c, c->d_cgpart, need) : LF_OK;
}

// What the correction's kernels need before anything is enqueued: the chunk table and the blocks' partial sums [rows][chunks]
// (grad: and [rows][chunks][DGRAD_SLOTS]); chunks: the narrow ones and behind them those of the wide list.
int deconv_prepare(lf_ctx* c, int B, bool grad) {
    int rc;
    if ((rc = src_chunk_table(c)) != LF_OK) return rc;
    const size_t need = (size_t)B * std::max(c->src_chunks.n + c->wide.n + c->cut.n, 1);
    if (need > c->d_dpart.size() && (rc = grow(c, c->d_dpart, need)) != LF_OK) return rc;
    if (grad && need * lf::DGRAD_SLOTS > c->d_dgpart.size() && (rc = grow(c, c->d_dgpart, need * lf::DGRAD_SLOTS)) != LF_OK) return rc;
    if (grad && c->opt_cut_grad && c->cut.n > 0) return cut_grad_workspace(c, B);
    return LF_OK;
}

lf::DeconvArgs deconv_args(lf_ctx* c, const double* d_theta, double* d_lnp, double* d_out) {
    const bool fr = c->kc.variant == LF_FREE;
    const ChunkTable& t = c->src_chunks;
    return lf::DeconvArgs{c->gradc, c->deconvc, d_theta, d_lnp, c->d_dpart, d_out, c->d_lum, c->d_a1, c->d_P,
                          fr ? c->d_a1.get() : c->d_elogf.get(), fr ? c->d_U.get() : c->d_eU.get(), c->d_sigma, c->d_ghnodes,
                          t.d_start, t.d_len, c->wide.n ? c->wide.d_field_all.get() : t.d_field.get(), t.n + c->wide.n + c->cut.n};
}

// The cut model's node tables (lf_hostprep.h: cut_tables) from the context's error model, to the device.  flim0, alpha0: the
// fixed completeness (FIXCOMP, ZEVOL; FREE: not read).
int cut_build(lf_ctx* c, const double* flim0, double alpha0) {
    auto& t = c->cut;
    t.built = false, t.n = 0;
    const lfh::CutTables h = lfh::cut_tables(c->kc.variant, c->kc.nf, c->kc.S, c->h_edge_lo.data(), c->h_edge_hi.data(), c->h_zarr.data(),
                                             c->h_vol.data(), c->h_ld2.data(), c->h_om0.data(), flim0, alpha0, c->gradc.kappa,
                                             t.nodes.data(), t.M, t.sigma.data(), c->opt_cut_limit);
    if (!h.err.empty()) {
        c->err = "lf_set_cut_error_model: " + h.err;
        return LF_ERR_ARG;
    }
    for (int f = 0; f < c->kc.nf; ++f) t.nnodes[f] = h.nnodes[f], t.H[f] = h.H[f];
    if (!h.start.empty()) {
        int rc = upload(c, t.d_L, h.L, t.d_P, h.P, t.d_c, h.c, t.d_a3, h.a3, t.d_a4, h.a4);
        if (rc != LF_OK) return rc;
        if ((rc = upload(c, t.d_start, h.start, t.d_len, h.len, t.d_field, h.field)) != LF_OK) return rc;
    }
    t.n = (int)h.start.size();
    t.built = true;
    return LF_OK;
}

// lf_deconv_cut.h's arguments for rows whose slots start at `part` ([rows][stride]; the cut blocks' behind the first `before`)
lf::DeconvCutArgs deconv_cut_args(lf_ctx* c, const double* d_theta, const double* d_lnp, double* part, int stride, int before, double* d_out) {
    const auto& t = c->cut;
    return lf::DeconvCutArgs{c->gradc, d_theta, d_lnp, part + before, d_out, t.d_L, t.d_P, t.d_c, t.d_a3, t.d_a4,
                             t.d_start, t.d_len, t.d_field, stride, t.n};
}

// lf_deconv_cut_grad.h's arguments for rows [b0, ...) of a call whose arguments are ca (cgpart: [rows][cut chunks][GRAD_SLOTS])
lf::DeconvCutGradArgs deconv_cut_grad_args(const lf::DeconvCutArgs& ca, int b0, double* cgpart, double* grad, bool alone) {
    lf::DeconvCutGradArgs g{ca, cgpart + (size_t)b0 * ca.nch * lf::GRAD_SLOTS, grad + (size_t)b0 * ca.gc.ndim, alone ? 1 : 0};
    g.d.theta += (size_t)b0 * ca.gc.ndim;
    g.d.lnprob += b0;
    if (g.d.part) g.d.part += (size_t)b0 * ca.stride;
    if (g.d.out) g.d.out += b0;
    return g;
}

// lf_deconv_wide.h's arguments from the narrow kernels' (da: the rows of one launch): the wide list's arrays and chunks, the
// partial sums advanced past the narrow blocks' slots
lf::DeconvWideArgs deconv_wide_args(lf_ctx* c, const lf::DeconvArgs& da) {
    const auto& w = c->wide;
    const int n0 = c->src_chunks.n;
    lf::DeconvWideArgs wa{};
    wa.d = da;
    wa.d.part = da.part + n0;
    wa.d.lum = w.d_lum, wa.d.a1 = w.d_a1, wa.d.P = w.d_P, wa.d.logf = w.d_logf, wa.d.U = w.d_U, wa.d.sigma = w.d_sigma;
    wa.d.chunk_start = w.d_start, wa.d.chunk_len = w.d_len, wa.d.chunk_field = w.d_field_all + n0;
    wa.chunk_class = w.d_class;
    wa.tables = w.d_tables;
    for (int k = 0; k < lf::DECONV_WIDE_NCLASS; ++k) wa.K[k] = w.K[k], wa.off[k] = w.off[k];
    return wa;
}

// the value's two kernels on the plain lnprob of B rows (da.lnprob).  tile: the first stage by tiles of DECONV_RT rows where the
// variant has that kernel (a chunk of launch_rows is a whole number of tiles, except the last)
void launch_deconv(lf_ctx* c, const lf::DeconvArgs& da, int B, hipStream_t s, bool tile) {
    using namespace lf;
    static_assert(32768 % DECONV_RT == 0, "launch_rows' chunks are whole tiles");
    launch_rows(c->kc.variant, B, [&](auto v, int b0, int nb) {
        DeconvArgs g = da;
        g.theta += (size_t)b0 * g.gc.ndim;
        g.lnprob += b0;
        g.part += (size_t)b0 * g.nch;
        g.out += b0;
        const int n0 = c->src_chunks.n, nw = c->wide.n;     // the narrow blocks of a row and the wide ones (g.nch = n0 + nw + the cut's)
        bool tiled = false;
        if constexpr (v() != LF_FREE) {
            tiled = tile && n0 > 0;
            if (tiled)
                hipLaunchKernelGGL(lf_deconv_tile<v()>, dim3((unsigned)n0, (unsigned)((nb + DECONV_RT - 1) / DECONV_RT)), dim3(BLOCK),
                                   0, s, g, nb);
        }
        if (n0 > 0 && !tiled) hipLaunchKernelGGL(lf_deconv_part<v()>, dim3((unsigned)n0, (unsigned)nb), dim3(BLOCK), 0, s, g);
        if (nw > 0) hipLaunchKernelGGL(lf_deconv_wide_part<v()>, dim3((unsigned)nw, (unsigned)nb), dim3(BLOCK), 0, s, deconv_wide_args(c, g));
        if (c->cut.n > 0)
            hipLaunchKernelGGL(lf_deconv_cut_part<v()>, dim3((unsigned)c->cut.n, (unsigned)nb), dim3(BLOCK), 0, s,
                               deconv_cut_args(c, g.theta, g.lnprob, g.part, g.nch, n0 + nw, nullptr));
        hipLaunchKernelGGL(lf_deconv_final, dim3((unsigned)nb), dim3(64), 0, s, g);
    });
}

// The flux-error-convolved lnprob of B rows (lf_deconv.h): the lnprob path itself first (d_lnp: what lf_lnprob_batch_device
// gives, bit for bit), then the blocks' partial sums of the correction and the rows' second stage, all on `s`.
int enqueue_deconv(lf_ctx* c, const double* d_theta, int B, double* d_lnp, double* d_out, hipStream_t s) {
    int rc;
    if ((rc = deconv_prepare(c, B, false)) != LF_OK) return rc;
    if ((rc = enqueue(c, d_theta, B, d_lnp, nullptr, nullptr, s)) != LF_OK) return rc;
    launch_deconv(c, deconv_args(c, d_theta, d_lnp, d_out), B, s, c->opt_deconv_tile != 0);
    LF_HIP(c, hipGetLastError());
    return LF_OK;
}

// The flux-error-convolved lnprob of B rows and its gradient (lf_deconv_grad.h), all on `s`: the plain lnprob and the plain
// gradient (enqueue_grad: d_lnp, d_grad), the value's kernels as enqueue_deconv launches them on that lnprob (d_out: what
// lf_lnprob_err_batch_device gives, bit for bit), then the correction's gradient, added to d_grad in place,
// and with the option "deconv_cut_grad" under a cut model the gradient of -Delta B (lf_deconv_cut_grad.h), added behind it.
int enqueue_deconv_grad(lf_ctx* c, const double* d_theta, int B, double* d_lnp, double* d_out, double* d_grad, hipStream_t s) {
    using namespace lf;
    int rc;
    if ((rc = deconv_prepare(c, B, true)) != LF_OK) return rc;
    if ((rc = enqueue_grad(c, d_theta, B, d_lnp, d_grad, s)) != LF_OK) return rc;
    const DeconvGradArgs da{deconv_args(c, d_theta, d_lnp, d_out), c->d_dgpart, d_grad};
    launch_deconv(c, da.d, B, s, false);          // (the gradient's value: the per-row kernels whatever "deconv_tile" says)
    // the cut's gradient (option "deconv_cut_grad"; no nodes - an error model of sigma = 0 -: nothing is launched)
    const bool cut_grad = c->opt_cut_grad && c->cut.n > 0;
    const DeconvCutArgs ca = deconv_cut_args(c, d_theta, d_lnp, nullptr, 0, 0, nullptr);
    launch_rows(c->kc.variant, B, [&](auto v, int b0, int nb) {
        DeconvGradArgs g = da;
        const int n0 = c->src_chunks.n, nw = c->wide.n;
        g.d.theta += (size_t)b0 * g.d.gc.ndim;
        g.d.lnprob += b0;
        g.d.nch = n0 + nw;                        // (Delta's blocks: the cut's have no slots in gpart, and no field in chunk_field)
        g.gpart += (size_t)b0 * g.d.nch * DGRAD_SLOTS;
        g.grad += (size_t)b0 * g.d.gc.ndim;
        if (n0 > 0) hipLaunchKernelGGL(lf_deconv_grad_part<v()>, dim3((unsigned)n0, (unsigned)nb), dim3(BLOCK), 0, s, g);
        if (nw > 0)
            hipLaunchKernelGGL(lf_deconv_wide_grad_part<v()>, dim3((unsigned)nw, (unsigned)nb), dim3(BLOCK), 0, s,
                               DeconvWideGradArgs{deconv_wide_args(c, g.d), g.gpart + (size_t)n0 * DGRAD_SLOTS});
        hipLaunchKernelGGL(lf_deconv_grad_final<v()>, dim3((unsigned)nb), dim3(64), 0, s, g);
        if (cut_grad) {                           // (per element: plain, then Delta, then the cut)
            const DeconvCutGradArgs cg = deconv_cut_grad_args(ca, b0, c->d_cgpart, d_grad, false);
            hipLaunchKernelGGL(lf_deconv_cut_grad_part<v()>, dim3((unsigned)c->cut.n, (unsigned)nb), dim3(BLOCK), 0, s, cg);
            hipLaunchKernelGGL(lf_deconv_cut_grad_final<v()>, dim3((unsigned)nb), dim3(64), 0, s, cg);
        }
    });
    LF_HIP(c, hipGetLastError());
    return LF_OK;
}

// The host forms' way in and out.  stage_theta: the workspace for B rows, theta through the pinned staging to d_theta on the
// context's stream.  fetch: n doubles of d through the pinned h, on that stream, and the wait for them.
int stage_theta(lf_ctx* c, const double* theta, int B) {
    int rc;
    LF_HIP(c, hipSetDevice(c->device));
    if ((rc = ensure_workspace(c, B, 0, 0)) != LF_OK) return rc;
    const size_t tb = (size_t)B * c->kc.ndim * sizeof(double);
    std::memcpy(c->h_theta, theta, tb);
    LF_HIP(c, hipMemcpyAsync(c->d_theta, c->h_theta, tb, hipMemcpyHostToDevice, c->stream));
    return LF_OK;
}
int fetch(lf_ctx* c, double* h, const double* d, size_t n) {
    LF_HIP(c, hipMemcpyAsync(h, d, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    LF_HIP(c, hipStreamSynchronize(c->stream));
    return LF_OK;
}
// a "(value, gradient)" call on host arrays: enq(d_value [B], d_grad [B][ndim]) enqueues it on the context's stream
template <class F>
int host_value_grad(lf_ctx* c, const double* theta, int B, double* value, double* grad, F enq) {
    int rc;
    if ((rc = stage_theta(c, theta, B)) != LF_OK) return rc;
    const size_t no = (size_t)B * (c->kc.ndim + 1);
    if (no > c->d_gout.size()) {
        if ((rc = grow(c, c->d_gout, no)) != LF_OK) return rc;
        LF_HIP(c, c->h_gout.alloc(no));
    }
    if ((rc = enq(c->d_gout.get(), c->d_gout + B)) != LF_OK) return rc;
    if ((rc = fetch(c, c->h_gout, c->d_gout, no)) != LF_OK) return rc;
    if (value) std::memcpy(value, c->h_gout, (size_t)B * sizeof(double));
    std::memcpy(grad, c->h_gout + B, (no - B) * sizeof(double));
    return LF_OK;
}

// Build the compressed catalogue and grid (lf_hostprep.h: compress) from the host's copy of the keys and the device's of lum.
int build_compressed(lf_ctx* c) {
    if (c->cmp.built) return LF_OK;
    if (c->kc.variant == LF_FIXCOMP) return LF_OK;          // piece A is closed-form already
    std::vector<double> lum;
    if (c->kc.variant == LF_ZEVOL) {
        lum.resize((size_t)c->N);
        if (c->N) LF_HIP(c, hipMemcpy(lum.data(), c->d_lum, lum.size() * sizeof(double), hipMemcpyDeviceToHost));
    }
    lfh::Compressed h = lfh::compress(c->kc, c->field_ind, c->h_x, lum, c->h_L, c->h_wL, c->h_ck, c->h_Dk);
    if (h.bad_field >= 0) {
        c->err = "compress: the catalogue of field " + std::to_string(h.bad_field) + " cannot be compressed to the error bound "
                 "(non-finite coordinate, or a prior box the bins cannot resolve)";
        return LF_ERR_ARG;
    }
    // Both are built here and enter the context together, complete: a failed upload leaves nothing behind
    CompressedCat cc;
    CompressedGrid g;
    int rc = upload(c, cc.d_lum, h.lum, cc.d_a1, h.node, cc.d_U, h.U, cc.d_W, h.weight);
    if (rc == LF_OK && h.grid)
        rc = upload(c, g.d_U, h.go.u, g.d_A4, h.A4, g.d_omega, h.go.omega, g.d_L, c->h_L, g.d_PGL, h.PGL, g.d_row0, h.go.row0,
                    g.d_nrows, h.go.nrows, g.d_off, h.go.off);
    if (rc != LF_OK) return rc;
    cc.n = (int64_t)h.node.size();
    cc.field_ind.swap(h.field_ind);
    cc.nbins = h.nbins;
    cc.bound = h.bound;
    cc.built = true;
    g.nb = h.go.nb;
    g.bound = h.go.bound;
    g.built = h.grid;
    c->cmp = std::move(cc);
    c->gridc = std::move(g);
    return LF_OK;
}

// see lf_set_option("compress"): direct vs compressed lnprob on 64 in-prior theta rows of this context
int compress_selfcheck(lf_ctx* c) {
    using namespace lf;
    const int B = 64, nd = c->kc.ndim, nf = c->kc.nf;
    std::vector<double> th((size_t)B * nd), direct(B), comp(B);
    uint64_t st = 0x9e3779b97f4a7c15ull;
    auto uni = [&]() {                                  // splitmix64 -> [0, 1)
        uint64_t z = (st += 0x9e3779b97f4a7c15ull);
        z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
        z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
        return (double)((z ^ (z >> 31)) >> 11) * 1.1102230246251565e-16;
    };
    auto in = [&](int lim, double lo_frac) {            // a point of the prior interval `lim` (upper part for L*)
        const double lo = c->kc.lims[lim][0], hi = c->kc.lims[lim][1];
        return lo + (hi - lo) * (lo_frac + (1.0 - lo_frac) * uni());
    };
    for (int b = 0; b < B; ++b) {
        double* t = th.data() + (size_t)b * nd;
        int k = 0;
        if (c->kc.variant == LF_ZEVOL) {
            for (int i = 0; i < 3; ++i) t[k++] = in(LF_LIM_LSTAR, 0.3);     // (the faint end of the L* box is the underflow zone)
            for (int i = 0; i < 3; ++i) t[k++] = in(LF_LIM_PHISTAR, 0.0);
            if (!c->kc.fix_sch_al) t[k++] = in(LF_LIM_SCH_AL, 0.0);
        } else {
            t[k++] = in(LF_LIM_LSTAR, 0.3);
            t[k++] = in(LF_LIM_PHISTAR, 0.0);
            if (!c->kc.fix_sch_al) t[k++] = in(LF_LIM_SCH_AL, 0.0);
            if (c->kc.variant == LF_FREE) {
                for (int f = 0; f < nf; ++f) t[k++] = in(LF_LIM_FLIM, 0.0);
                t[k++] = in(LF_LIM_ALPHA, 0.0);
            }
        }
    }
    const int64_t was = c->opt_compress;
    int rc = ensure_workspace(c, B, 0, 0);
    for (int pass = 0; pass < 2 && rc == LF_OK; ++pass) {
        c->opt_compress = pass;
        LF_HIP(c, hipMemcpy(c->d_theta, th.data(), th.size() * sizeof(double), hipMemcpyHostToDevice));
        rc = enqueue(c, c->d_theta, B, c->d_out, nullptr, nullptr, c->stream);
        if (rc != LF_OK) break;
        LF_HIP(c, hipStreamSynchronize(c->stream));
        LF_HIP(c, hipMemcpy(pass ? comp.data() : direct.data(), c->d_out, B * sizeof(double), hipMemcpyDeviceToHost));
    }
    c->opt_compress = was;
    if (rc != LF_OK) return rc;
    double worst = 0.0;
    int nfin = 0;
    for (int b = 0; b < B; ++b) {
        if (std::isinf(direct[b]) || std::isinf(comp[b])) {
            if (direct[b] != comp[b]) worst = HUGE_VAL;
            continue;
        }
        ++nfin;
        worst = std::fmax(worst, std::fabs(comp[b] - direct[b]) / std::fmax(std::fabs(direct[b]), 1e-300));
    }
    if (!(worst <= 1.0e-12)) {
        char msg[200];
        std::snprintf(msg, sizeof(msg), "compress: the compressed catalogue differs from the direct path by %.3g (relative) on "
                      "%d of 64 self-check walkers of this prior box: option refused", worst, nfin);
        c->err = msg;
        return LF_ERR_ARG;
    }
    return LF_OK;
}

void free_ctx(lf_ctx* c) {
    if (!c) return;
    hipSetDevice(c->device);
    if (c->stream) hipStreamSynchronize(c->stream);
    for (auto& e : c->events) {
        hipEventDestroy(e.a);
        hipEventDestroy(e.b);
    }
    if (c->stream) hipStreamDestroy(c->stream);
    delete c;                            // (its buffers go with it: lf_devmem.h)
}

// Derive every table (lf_hostprep.h), upload it, set the context's fields.  The three environment variables: A/B runs and tests.
int build(lf_ctx* c, const lf_desc* d) {
    using namespace lf;
    const int nf = d->nf;
    KConst& kc = c->kc;
    kc.forms = nullptr;
#ifdef LF_STAMPS
    kc.stamps = nullptr;
#endif
    c->N = d->N;
    c->field_ind.assign(d->field_ind, d->field_ind + nf + 1);
    lfh::Catalogue cat = lfh::catalogue(d, kc);
    c->gradc = lfh::grad_const(kc, d->N, d->variant == LF_ZEVOL ? cat.a1.data() : nullptr);
    c->perm = cat.perm;
    c->grid_separable = lfh::same_columns(d->logL, d->S);
    {
        const size_t S = (size_t)d->S;
        c->h_edge_lo.assign(d->logL, d->logL + S);
        c->h_edge_hi.assign(d->logL + (S - 1) * S, d->logL + S * S);
        c->h_zarr.assign(d->zarr, d->zarr + S);
        if (d->volume_part) c->h_vol.assign(d->volume_part, d->volume_part + S);
        if (d->dl_zarr) {
            c->h_ld2.resize(S);
            for (size_t k = 0; k < S; ++k) {
                const double dlcm = LF_MPC_CM * d->dl_zarr[k];
                c->h_ld2[k] = std::log10(4.0 * M_PI * dlcm * dlcm);
            }
        }
        c->h_om0.resize((size_t)nf);
        for (int f = 0; f < nf; ++f) c->h_om0[(size_t)f] = d->omega0[f] / LF_SQARCSEC;
    }
    int rc;
    kc.cells = 0;
    kc.zcell_rho = 0.0;
    for (int f = 0; f < MAXF; ++f) {
        kc.kf_first[f] = 0;
        kc.kf_last[f] = lf::KEY_MAX;
    }
    for (int f = 0; f <= MAXF; ++f) kc.cc_fstart[f] = 0;
    if (d->variant == LF_FREE && (rc = upload_cells(c, lfh::build_cells(kc, c->field_ind, cat.a1, nf, CELL_M, CELL_RHO_G, CELL_RHO_H))) != LF_OK) return rc;
    if (d->variant == LF_ZEVOL) {
        kc.zcell_rho = lfh::zcell_rho_for_box(kc, nf, ZCELL_RHO, ZCELL_X1, ZCELL_X2);
        if ((rc = upload_cells(c, lfh::build_cells(kc, c->field_ind, cat.a1, nf, ZCELL_M, CELL_RHO_G, CELL_RHO_H, lfh::lum_weights(cat.lum).data()))) != LF_OK) return rc;
    }
    if ((rc = upload(c, c->d_lum, cat.lum, c->d_a1, cat.a1, c->d_P, cat.P, c->d_U, cat.U)) != LF_OK) return rc;
    if (d->variant != LF_FIXCOMP) c->h_x.swap(cat.a1);      // (the sorted values the chunk keys come from)

    lfh::GridSwitches sw;
    sw.gridq = !std::getenv("LF_NO_GRIDQ");
    sw.zgrid_cols = !std::getenv("LF_NO_ZGRID_COLS");
    sw.collapse = !std::getenv("LF_NO_COLLAPSE_GRID");
    lfh::Grid gr = lfh::grid_tables(d, kc, sw);
    c->nnodes = (int)gr.G.size();
    kc.zgrid_cols = gr.zgrid_cols ? 1 : 0;
    if (gr.binned) {
        auto& g = c->gridq;
        if ((rc = upload(c, g.d_rec, gr.gridq.rec, g.d_omega, gr.gridq.omega, g.d_rows, gr.gridq.rows)) != LF_OK) return rc;
        g.nb = gr.gridq.nb;
        g.margin = gr.gridq.margin;
        g.built = true;
    }
    if ((rc = upload(c, c->d_G, gr.G, c->d_PG, gr.PG, c->d_W, gr.W, c->d_a3, gr.a3, c->d_a4, gr.a4)) != LF_OK) return rc;
    if (d->variant != LF_FREE) {
        if ((rc = upload(c, c->d_nodes4, gr.nodes4, c->d_zcol, gr.zcol)) != LF_OK) return rc;
        c->nch4 = (int)(gr.nodes4.size() / (64 * 4));
    }
    if ((rc = upload(c, c->d_a4min, gr.a4min)) != LF_OK) return rc;
    if (d->variant == LF_FREE && (rc = upload(c, c->d_nodes8, gr.nodes8)) != LF_OK) return rc;
    c->h_L.swap(gr.L), c->h_wL.swap(gr.wL), c->h_ck.swap(gr.ck), c->h_Dk.swap(gr.Dk);
    {
        hipDeviceProp_t prop;
        LF_HIP(c, hipGetDeviceProperties(&prop, c->device));
        c->num_cu = prop.multiProcessorCount;
        LF_HIP(c, c->d_queue.alloc(1024));
        LF_HIP(c, hipMemset(c->d_queue, 0, 1024 * sizeof(int)));
    }
    LF_HIP(c, hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    const int mb = d->max_batch > 0 ? d->max_batch : 1024;
    return ensure_workspace(c, mb, 0, 0);
}

}  // namespace

extern "C" {

int lf_deal_table(int n_cell_chunks, int n_bins, int grid_part, int grid_parts, int32_t* table, int64_t cap) {
    using namespace lf;
    if (n_cell_chunks < 0 || n_bins < 0 || grid_parts < 0 || grid_part < 0 || (grid_parts > 0 && grid_part >= grid_parts)) return LF_ERR_ARG;
    const int64_t n = (int64_t)DEAL_LIST + n_cell_chunks + n_bins;
    if (!table) return (int)n;
    if (cap < n) return LF_ERR_ARG;
    const std::vector<int> t = make_deal(n_cell_chunks, n_bins, grid_part, grid_parts);
    for (int64_t i = 0; i < n; ++i) table[i] = t[(size_t)i];
    return (int)n;
}

int lf_deal_finishers(int n_cell_chunks, int n_bins, int grid_part, int grid_parts, int32_t ranks[4]) {
    using namespace lf;
    if (n_cell_chunks < 0 || n_bins < 0 || grid_parts < 0 || grid_part < 0 || (grid_parts > 0 && grid_part >= grid_parts) || !ranks) return LF_ERR_ARG;
    const int word = deal_finishers(make_deal(n_cell_chunks, n_bins, grid_part, grid_parts), n_cell_chunks, n_bins, grid_part, grid_parts);
    for (int g = 0; g < 4; ++g) ranks[g] = (word >> (8 * g)) & 0xff;
    return LF_OK;
}

int lf_abi_version(void) { return LF_ABI_VERSION; }

const char* lf_last_error(const lf_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

lf_ctx* lf_create(const lf_desc* d) {
    g_create_error.clear();
    if (!d) {
        g_create_error = "lf_create: NULL descriptor";
        return nullptr;
    }
    auto bad = [&](const char* m) {
        g_create_error = std::string("lf_create: ") + m;
        return (lf_ctx*)nullptr;
    };
    if (d->variant < LF_FREE || d->variant > LF_ZEVOL) return bad("unknown variant");
    if (d->nf < 1 || d->nf > LF_MAX_FIELDS) return bad("nf out of range (1..LF_MAX_FIELDS)");
    if (d->S < 2 || d->S > 4096) return bad("S out of range");
    if (d->N < 0 || d->N > 2000000000LL) return bad("N out of range");
    if (!d->field_ind || !d->omega0 || !d->logL || !d->zarr) return bad("NULL field_ind/omega0/logL/zarr");
    if (d->N > 0 && !d->lum) return bad("NULL lum");
    if (d->field_ind[0] != 0 || d->field_ind[d->nf] != d->N) return bad("field_ind must span [0, N]");
    for (int f = 0; f < d->nf; ++f)
        if (d->field_ind[f + 1] < d->field_ind[f]) return bad("field_ind must be non-decreasing");
    if (!(d->fcmin > 0.0 && d->fcmin < 1.0) || d->fcmin == 0.5) return bad("fcmin must be in (0,1), != 0.5");
    if (d->variant == LF_FREE) {
        if ((d->N > 0 && !d->logf) || !d->volume_part || !d->dl_zarr) return bad("FREE needs logf, volume_part, dl_zarr");
    } else {
        if ((d->N > 0 && !d->om_arr) || !d->integ_part) return bad("FIXCOMP/ZEVOL need om_arr, integ_part");
        if (d->variant == LF_FIXCOMP && !d->flim0) return bad("FIXCOMP needs flim0");
        if (d->variant == LF_ZEVOL && d->N > 0 && !d->z) return bad("ZEVOL needs z");
        if (d->variant == LF_ZEVOL && (d->pivots[0] == d->pivots[1] || d->pivots[0] == d->pivots[2] ||
                                       d->pivots[1] == d->pivots[2]))
            return bad("ZEVOL pivots must be distinct");
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return bad("no HIP device visible");
    if (d->device < 0 || d->device >= ndev) return bad("device ordinal out of range");
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, d->device) != hipSuccess) return bad("hipGetDeviceProperties failed");
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        g_create_error = std::string("lf_create: device is ") + prop.gcnArchName + ", this library is built for gfx950 only";
        return nullptr;
    }
    if (hipSetDevice(d->device) != hipSuccess) return bad("hipSetDevice failed");
    lf_ctx* c = new (std::nothrow) lf_ctx();
    if (!c) return bad("out of host memory");
    c->device = d->device;
    int rc = LF_OK;
    try {
        rc = build(c, d);
    } catch (const std::bad_alloc&) {
        c->err = "out of host memory";
        rc = LF_ERR_NOMEM;
    }
    if (rc != LF_OK) {
        g_create_error = "lf_create: " + c->err;
        free_ctx(c);
        return nullptr;
    }
    return c;
}

void lf_destroy(lf_ctx* ctx) { free_ctx(ctx); }

int lf_ndim(const lf_ctx* ctx) { return ctx ? ctx->kc.ndim : LF_ERR_ARG; }

int lf_lnprob_batch_device(lf_ctx* c, const double* d_theta, int B, double* d_out, void* hip_stream) {
    if (!c) return LF_ERR_ARG;
    if (!d_theta || !d_out || B <= 0) {
        c->err = "lf_lnprob_batch_device: NULL pointer or B <= 0";
        return LF_ERR_ARG;
    }
    LF_HIP(c, hipSetDevice(c->device));
    return enqueue(c, d_theta, B, d_out, nullptr, nullptr, (hipStream_t)hip_stream);
}

int lf_lnprob_batch_device_n(lf_ctx* c, const double* d_theta, int B, int K, double* d_out, void* hip_stream) {
    if (!c) return LF_ERR_ARG;
    if (!d_theta || !d_out || B <= 0 || K <= 0) {
        c->err = "lf_lnprob_batch_device_n: NULL pointer, B <= 0 or K <= 0";
        return LF_ERR_ARG;
    }
    LF_HIP(c, hipSetDevice(c->device));
    const size_t nd = (size_t)c->kc.ndim;
    for (int k = 0; k < K; ++k) {
        const int rc = enqueue(c, d_theta + (size_t)k * B * nd, B, d_out + (size_t)k * B, nullptr, nullptr, (hipStream_t)hip_stream);
        if (rc != LF_OK) return rc;
    }
    return LF_OK;
}

static int host_eval(lf_ctx* c, const double* theta, int B, double* out, double* outA, double* outB) {
    using namespace lf;
    if (!c) return LF_ERR_ARG;
    if (!theta || B <= 0 || (!out && !(outA && outB))) {
        c->err = "lf_lnprob_batch: NULL pointer or B <= 0";
        return LF_ERR_ARG;
    }
    LF_HIP(c, hipSetDevice(c->device));
    int rc = ensure_workspace(c, B, 0, 0);
    if (rc != LF_OK) return rc;
    const size_t tb = (size_t)B * c->kc.ndim * sizeof(double);
    std::memcpy(c->h_theta, theta, tb);
    LF_HIP(c, hipMemcpyAsync(c->d_theta, c->h_theta, tb, hipMemcpyHostToDevice, c->stream));
    // (the two pieces only when they are asked for: a plain evaluation then takes lf_free's one-launch form)
    rc = enqueue(c, c->d_theta, B, c->d_out, outA ? c->d_outA : nullptr, outB ? c->d_outB : nullptr, c->stream);
    if (rc != LF_OK) return rc;
    const size_t ob = (size_t)B * sizeof(double);
    LF_HIP(c, hipMemcpyAsync(c->h_out, c->d_out, ob, hipMemcpyDeviceToHost, c->stream));
    if (outA) {
        LF_HIP(c, hipMemcpyAsync(c->h_out + B, c->d_outA, ob, hipMemcpyDeviceToHost, c->stream));
        LF_HIP(c, hipMemcpyAsync(c->h_out + 2 * (size_t)B, c->d_outB, ob, hipMemcpyDeviceToHost, c->stream));
    }
    LF_HIP(c, hipStreamSynchronize(c->stream));
    if (out && c->d_err) {
        // lnprob is never NaN - unless a polling finisher gave up (lf_tile.h: PART_POLLS): then say so instead of handing NaN on
        bool nan = false;
        for (int i = 0; i < B; ++i) nan = nan || c->h_out[i] != c->h_out[i];
        if (nan) {
            int e = 0;
            LF_HIP(c, hipMemcpy(&e, c->d_err, sizeof(int), hipMemcpyDeviceToHost));
            if (e) {
                c->err = "lf_lnprob_batch: a tile's finishing workgroup waited in vain for the tile's partial sums (device stalled?)";
                return LF_ERR_HIP;
            }
        }
    }
    if (out) std::memcpy(out, c->h_out, ob);
    if (outA) {
        std::memcpy(outA, c->h_out + B, ob);
        std::memcpy(outB, c->h_out + 2 * (size_t)B, ob);
    }
    return LF_OK;
}

int lf_lnprob_batch(lf_ctx* c, const double* theta, int B, double* out) {
    if (c && !out) {
        c->err = "lf_lnprob_batch: NULL out";
        return LF_ERR_ARG;
    }
    return host_eval(c, theta, B, out, nullptr, nullptr);
}

int lf_lnprob_pieces(lf_ctx* c, const double* theta, int B, double* outA, double* outB) {
    if (c && (!outA || !outB)) {
        c->err = "lf_lnprob_pieces: NULL output";
        return LF_ERR_ARG;
    }
    return host_eval(c, theta, B, nullptr, outA, outB);
}

int lf_lnprob_grad_batch_device(lf_ctx* c, const double* d_theta, int B, double* d_lnprob, double* d_grad, void* hip_stream) {
    int rc = family_check(c, "lf_lnprob_grad_batch_device", false, d_theta, B, d_grad);
    if (rc != LF_OK) return rc;
    LF_HIP(c, hipSetDevice(c->device));
    if (!d_lnprob) {
        // (the rows' lnprob decides their NaN: into the context's own buffer, sized before the lnprob path may replace it)
        if ((rc = ensure_workspace(c, B, 0, 0)) != LF_OK) return rc;
        d_lnprob = c->d_out;
    }
    return enqueue_grad(c, d_theta, B, d_lnprob, d_grad, (hipStream_t)hip_stream);
}

int lf_lnprob_grad_batch(lf_ctx* c, const double* theta, int B, double* lnprob, double* grad) {
    const int rc = family_check(c, "lf_lnprob_grad_batch", false, theta, B, grad);
    if (rc != LF_OK) return rc;
    return host_value_grad(c, theta, B, lnprob, grad, [&](double* d_lnp, double* d_grad) {
        return enqueue_grad(c, c->d_theta, B, d_lnp, d_grad, c->stream);
    });
}

int lf_gauss_hermite(int K, double* x, double* lnw) {
    if (!x || !lnw || !lfh::gauss_hermite(K, x, lnw)) return LF_ERR_ARG;
    return LF_OK;
}

int lf_deconv_info(int32_t* orders, double* sigma_max, int cap, int* default_order, int* chunk) {
    if (default_order) *default_order = lf::DECONV_DEFAULT_ORDER;
    if (chunk) *chunk = lf::DECONV_CH;
    for (int i = 0; i < lf::DECONV_NORDERS && i < cap; ++i) {
        if (orders) orders[i] = lf::DECONV_ORDERS[i];
        if (sigma_max) sigma_max[i] = lf::DECONV_SIGMA_MAX[i];
    }
    return lf::DECONV_NORDERS;
}

int lf_deconv_wide_info(double* edges, int32_t* nodes, int cap, int* chunk, double* T, int* npanel, double* h, int cls, double* x,
                        double* lnw) {
    if (chunk) *chunk = lf::DECONV_WIDE_CH;
    if (T) *T = lf::DECONV_WIDE_T;
    if (npanel) *npanel = lf::DECONV_WIDE_NPAN;
    if (h) *h = lf::DECONV_WIDE_H;
    for (int i = 0; i < lf::DECONV_WIDE_NCLASS && i < cap; ++i) {
        if (edges) edges[i] = lf::DECONV_WIDE_EDGE[i];
        if (nodes) nodes[i] = lfh::wide_nodes(i);
    }
    if (x || lnw) {
        if (!x || !lnw || cls < 0 || cls >= lf::DECONV_WIDE_NCLASS) return LF_ERR_ARG;
        lfh::wide_table(cls, x, lnw);
    }
    return lf::DECONV_WIDE_NCLASS;
}

int lf_set_lum_err(lf_ctx* c, const double* sigma, int K, const double* logf, const double* flim0, double alpha0) {
    using namespace lf;
    if (!c) return LF_ERR_ARG;
    auto bad = [&](const std::string& m) {
        c->err = "lf_set_lum_err: " + m;
        return (int)LF_ERR_ARG;
    };
    const int64_t N = c->N;
    const int nf = c->kc.nf;
    if (N > 0 && !sigma) return bad("NULL sigma");
    const double smax = lfh::deconv_sigma_max(K);
    if (smax < 0.0) return bad("order K = " + std::to_string(K) + " is not supported (4, 6, 8, 10, 12, 16, 20, 24, 32)");
    if (!c->grid_separable && !c->cut.model)
        return bad("the grid's redshift columns have their own luminosity nodes (min_comp_frac > 0.001): a cut on the observed "
                   "flux would change the expected counts, which this model leaves as they are (lf_set_cut_error_model, called "
                   "first, adds that change)");
    const bool fr = c->kc.variant == LF_FREE;
    if (!fr) {
        if (!flim0 || (N > 0 && !logf)) return bad("fixed completeness (FIXCOMP, ZEVOL) needs logf and flim0");
        if (!std::isfinite(alpha0) || alpha0 == 0.0) return bad("alpha0 must be finite and not 0");
        for (int f = 0; f < nf; ++f)
            if (!(flim0[f] > 0.0) || !std::isfinite(flim0[f])) return bad("flim0 must be finite and > 0");
    }
    const double top = DECONV_WIDE_EDGE[DECONV_WIDE_NCLASS - 1];
    for (int64_t i = 0; i < N; ++i) {
        if (!std::isfinite(sigma[i]) || sigma[i] < 0.0) return bad("sigma must be finite and >= 0 (source " + std::to_string(i) + ")");
        if (c->opt_deconv_wide) {
            if (sigma[i] > top) {
                char msg[200];
                std::snprintf(msg, sizeof(msg), "sigma = %.4g dex of source %lld is above %.2f dex, the largest value the wide rule "
                              "(option deconv_wide) is validated for", sigma[i], (long long)i, top);
                return bad(msg);
            }
        } else if (sigma[i] > smax && !c->opt_deconv_unchecked) {
            char msg[200];
            std::snprintf(msg, sizeof(msg), "sigma = %.4g dex of source %lld is above %.2f dex, the largest value the order K = %d is "
                          "validated for (per-source error below 1e-7; K = 32 reaches 0.09)", sigma[i], (long long)i, smax, K);
            return bad(msg);
        }
        if (!fr && sigma[i] > 0.0 && !std::isfinite(logf[i])) return bad("logf must be finite (source " + std::to_string(i) + ")");
    }
    LF_HIP(c, hipSetDevice(c->device));
    LF_HIP(c, hipDeviceSynchronize());               // (a call in flight may read the buffers replaced below)
    c->deconv_set = false;
    c->cutv.built = false;
    std::vector<double> sg((size_t)N), lf_, u_, nodes((size_t)2 * K);
    for (int64_t i = 0; i < N; ++i) sg[(size_t)i] = sigma[c->perm[(size_t)i]];
    lfh::gauss_hermite(K, nodes.data(), nodes.data() + K);
    // the wide list (option "deconv_wide"): the sources above the order's limit; the narrow kernels find sigma = 0 for them
    c->wide.n = 0;
    lfh::WideList wl;
    if (c->opt_deconv_wide) wl = lfh::wide_list(sg, c->field_ind, nf, smax);
    const std::vector<double> sg_all = sg;
    for (int64_t i : wl.src) sg[(size_t)i] = 0.0;
    int rc = upload(c, c->d_sigma, sg, c->d_ghnodes, nodes);
    if (rc != LF_OK) return rc;
    DeconvConst dc{};
    dc.K = K;
    if (!fr) {
        lf_.resize((size_t)N), u_.resize((size_t)N);
        for (int64_t i = 0; i < N; ++i) {
            lf_[(size_t)i] = logf[c->perm[(size_t)i]];
            u_[(size_t)i] = std::pow(10.0, lf_[(size_t)i] - LF_FREF);
        }
        if ((rc = upload(c, c->d_elogf, lf_, c->d_eU, u_)) != LF_OK) return rc;
        dc.alpha0 = alpha0;
        for (int f = 0; f < nf; ++f) dc.flim0[f] = flim0[f];
    }
    if (!wl.src.empty()) {
        // what the terms read per source, as the context's own arrays hold it (FREE: the log flux is a1, 10^(that + 17) is U)
        std::vector<double> h[4];
        const double* dev[4] = {c->d_lum, c->d_a1, c->d_P, c->d_U};
        for (int k = 0; k < 4; ++k) {
            h[k].resize((size_t)N);
            LF_HIP(c, hipMemcpy(h[k].data(), dev[k], (size_t)N * sizeof(double), hipMemcpyDeviceToHost));
        }
        const std::vector<double>&hl = fr ? h[1] : lf_, &hu = fr ? h[3] : u_;
        const size_t nw = wl.src.size();
        std::vector<double> wlum(nw), wa1(nw), wP(nw), wlogf(nw), wU(nw), wsg(nw);
        for (size_t j = 0; j < nw; ++j) {
            const size_t i = (size_t)wl.src[j];
            wlum[j] = h[0][i], wa1[j] = h[1][i], wP[j] = h[2][i], wlogf[j] = hl[i], wU[j] = hu[i], wsg[j] = sg_all[i];
        }
        auto& w = c->wide;
        std::vector<double> tables;
        for (int k = 0; k < DECONV_WIDE_NCLASS; ++k) {
            w.K[k] = lfh::wide_nodes(k);
            w.off[k] = (int)tables.size();
            tables.resize(tables.size() + 2 * (size_t)w.K[k]);
            lfh::wide_table(k, tables.data() + w.off[k], tables.data() + w.off[k] + w.K[k]);
        }
        // the field of every block of a row: the chunks the narrow kernels take (src_chunk_table's), then the wide ones
        std::vector<int> field_all = lfh::chunk_table(c->field_ind, nf, GRAD_CH, 0.0, 0.0, 0.0).field;
        field_all.insert(field_all.end(), wl.field.begin(), wl.field.end());
        if ((rc = src_chunk_table(c)) != LF_OK) return rc;
        if ((rc = upload(c, w.d_lum, wlum, w.d_a1, wa1, w.d_P, wP, w.d_logf, wlogf, w.d_U, wU, w.d_sigma, wsg, w.d_tables, tables)) != LF_OK)
            return rc;
        if ((rc = upload(c, w.d_start, wl.start, w.d_len, wl.len, w.d_class, wl.cls, w.d_field_all, field_all)) != LF_OK) return rc;
        w.n = (int)wl.start.size();
    }
    // lf_lumpost.h's slots: where each source of the device's arrays stands in the caller's catalogue
    std::vector<int> caller((size_t)N + wl.src.size());
    for (int64_t i = 0; i < N; ++i) caller[(size_t)i] = (int)c->perm[(size_t)i];
    for (size_t j = 0; j < wl.src.size(); ++j) caller[(size_t)N + j] = (int)c->perm[(size_t)wl.src[j]];
    if ((rc = upload(c, c->d_lp_caller, caller)) != LF_OK) return rc;
    std::vector<int> in_wide((size_t)N, 0);
    for (int64_t i : wl.src) in_wide[(size_t)i] = 1;
    if ((rc = upload(c, c->d_vt_inwide, in_wide)) != LF_OK) return rc;
    c->lp_nslots = (int)caller.size();
    c->deconvc = dc;
    // the cut model's tables at a fixed completeness: the curve arrived with this call
    if (c->cut.model && !fr && (rc = cut_build(c, flim0, alpha0)) != LF_OK) {
        if (rc == LF_ERR_ARG) c->err = "lf_set_lum_err: the cut model's tables: " + c->err;
        return rc;
    }
    c->deconv_set = true;
    return LF_OK;
}

int lf_set_cut_error_model(lf_ctx* c, const double* nodes, int M, const double* sigma) {
    if (!c) return LF_ERR_ARG;
    auto bad = [&](const std::string& m) {
        c->err = "lf_set_cut_error_model: " + m;
        return (int)LF_ERR_ARG;
    };
    if (c->opt_skip_grid || c->kc.grid_parts > 1) return bad("no convolved likelihood of a source-sharded context (options skip_grid, grid_share)");
    if (c->grid_separable)
        return bad("every redshift column of the grid has the same luminosity nodes (min_comp_frac <= 0.001): there is no cut on "
                   "the observed flux, and the expected counts stay as they are");
    if (c->deconv_set) return bad("luminosity errors are set already: call this before lf_set_lum_err");
    if (c->h_vol.empty() || c->h_ld2.empty()) return bad("the descriptor must hold volume_part and dl_zarr (FIXCOMP, ZEVOL too) for the cut model");
    const std::string why = lfh::cut_model_check(nodes, M, sigma, c->kc.nf);
    if (!why.empty()) return bad(why);
    LF_HIP(c, hipSetDevice(c->device));
    LF_HIP(c, hipDeviceSynchronize());               // (a call in flight may read the buffers replaced below)
    auto& t = c->cut;
    t.model = false, t.built = false, t.n = 0;
    c->cutv.built = false, c->cutv.img = false;
    t.M = M;
    t.nodes.assign(nodes, nodes + M);
    t.sigma.assign(sigma, sigma + (size_t)c->kc.nf * M);
    if (c->kc.variant == LF_FREE) {
        t.model = true;
        const int rc = cut_build(c, nullptr, 0.0);
        if (rc != LF_OK) t.model = false;
        return rc;
    }
    // fixed completeness: the tables hold the curve, which lf_set_lum_err brings; a dry run refuses now what would be refused then
    const lfh::CutTables dry = lfh::cut_tables(LF_FREE, c->kc.nf, c->kc.S, c->h_edge_lo.data(), c->h_edge_hi.data(), c->h_zarr.data(),
                                               c->h_vol.data(), c->h_ld2.data(), c->h_om0.data(), nullptr, 0.0, 0.0, t.nodes.data(), M,
                                               t.sigma.data(), c->opt_cut_limit);
    if (!dry.err.empty()) return bad(dry.err);
    for (int f = 0; f < c->kc.nf; ++f) t.nnodes[f] = dry.nnodes[f], t.H[f] = dry.H[f];
    t.model = true;
    return LF_OK;
}

int lf_cut_info(lf_ctx* c, int32_t* nnodes, double* H, int cap, int* chunk, int* chunks) {
    if (!c) return LF_ERR_ARG;
    if (chunk) *chunk = lf::DECONV_CUT_CH;
    if (!c->cut.model) {
        c->err = "lf_cut_info: no cut model set (call lf_set_cut_error_model first)";
        return LF_ERR_ARG;
    }
    if (chunks) *chunks = c->cut.built ? c->cut.n : -1;
    for (int f = 0; f < c->kc.nf && f < cap; ++f) {
        if (nnodes) nnodes[f] = c->cut.nnodes[f];
        if (H) H[f] = c->cut.H[f];
    }
    return c->kc.nf;
}

int lf_cut_term_batch(lf_ctx* c, const double* theta, int B, double* out) {
    using namespace lf;
    int rc = family_check(c, "lf_cut_term_batch", true, theta, B, out);
    if (rc != LF_OK) return rc;
    if (!c->cut.model || !c->cut.built) {
        c->err = "lf_cut_term_batch: no cut model set (call lf_set_cut_error_model, then lf_set_lum_err)";
        return LF_ERR_ARG;
    }
    if ((rc = stage_theta(c, theta, B)) != LF_OK) return rc;
    const int n = c->cut.n;
    const size_t need = (size_t)B * std::max(n, 1);
    if (need > c->d_dpart.size() && (rc = grow(c, c->d_dpart, need)) != LF_OK) return rc;
    if ((rc = enqueue(c, c->d_theta, B, c->d_outB, nullptr, nullptr, c->stream)) != LF_OK) return rc;
    const DeconvCutArgs ca = deconv_cut_args(c, c->d_theta, c->d_outB, c->d_dpart, n, 0, c->d_outA);
    launch_rows(c->kc.variant, B, [&](auto v, int b0, int nb) {
        DeconvCutArgs g = ca;
        g.theta += (size_t)b0 * g.gc.ndim;
        g.lnprob += b0;
        g.part += (size_t)b0 * g.stride;
        g.out += b0;
        if (n > 0) hipLaunchKernelGGL(lf_deconv_cut_part<v()>, dim3((unsigned)n, (unsigned)nb), dim3(BLOCK), 0, c->stream, g);
        hipLaunchKernelGGL(lf_deconv_cut_final, dim3((unsigned)nb), dim3(64), 0, c->stream, g);
    });
    LF_HIP(c, hipGetLastError());
    if ((rc = fetch(c, c->h_out, c->d_outA, (size_t)B)) != LF_OK) return rc;
    std::memcpy(out, c->h_out, (size_t)B * sizeof(double));
    return LF_OK;
}

int lf_cut_term_grad_batch(lf_ctx* c, const double* theta, int B, double* out, double* grad) {
    using namespace lf;
    int rc = family_check(c, "lf_cut_term_grad_batch", true, theta, B, out && grad ? out : nullptr);
    if (rc != LF_OK) return rc;
    if (!c->cut.model || !c->cut.built) {
        c->err = "lf_cut_term_grad_batch: no cut model set (call lf_set_cut_error_model, then lf_set_lum_err)";
        return LF_ERR_ARG;
    }
    return host_value_grad(c, theta, B, out, grad, [&](double* d_val, double* d_grad) -> int {
        int rc;
        const int n = c->cut.n;
        const size_t need = (size_t)B * std::max(n, 1);
        if (need > c->d_dpart.size() && (rc = grow(c, c->d_dpart, need)) != LF_OK) return rc;
        if ((rc = cut_grad_workspace(c, B)) != LF_OK) return rc;
        if ((rc = enqueue(c, c->d_theta, B, c->d_outB, nullptr, nullptr, c->stream)) != LF_OK) return rc;
        const DeconvCutArgs ca = deconv_cut_args(c, c->d_theta, c->d_outB, c->d_dpart, n, 0, d_val);
        launch_rows(c->kc.variant, B, [&](auto v, int b0, int nb) {
            const DeconvCutGradArgs cg = deconv_cut_grad_args(ca, b0, c->d_cgpart, d_grad, true);
            if (n > 0) {
                hipLaunchKernelGGL(lf_deconv_cut_part<v()>, dim3((unsigned)n, (unsigned)nb), dim3(BLOCK), 0, c->stream, cg.d);
                hipLaunchKernelGGL(lf_deconv_cut_grad_part<v()>, dim3((unsigned)n, (unsigned)nb), dim3(BLOCK), 0, c->stream, cg);
            }
            hipLaunchKernelGGL(lf_deconv_cut_grad_final<v()>, dim3((unsigned)nb), dim3(64), 0, c->stream, cg);
        });
        LF_HIP(c, hipGetLastError());
        return LF_OK;
    });
}

int lf_lnprob_err_batch_device(lf_ctx* c, const double* d_theta, int B, double* d_out, void* hip_stream) {
    int rc = family_check(c, "lf_lnprob_err_batch_device", true, d_theta, B, d_out);
    if (rc != LF_OK) return rc;
    LF_HIP(c, hipSetDevice(c->device));
    // (the rows' plain lnprob: into the context's own buffer, sized before the lnprob path may replace it)
    if ((rc = ensure_workspace(c, B, 0, 0)) != LF_OK) return rc;
    return enqueue_deconv(c, d_theta, B, c->d_outB, d_out, (hipStream_t)hip_stream);
}

int lf_lnprob_err_batch(lf_ctx* c, const double* theta, int B, double* out) {
    int rc = family_check(c, "lf_lnprob_err_batch", true, theta, B, out);
    if (rc != LF_OK) return rc;
    if ((rc = stage_theta(c, theta, B)) != LF_OK) return rc;
    if ((rc = enqueue_deconv(c, c->d_theta, B, c->d_outB, c->d_outA, c->stream)) != LF_OK) return rc;
    if ((rc = fetch(c, c->h_out, c->d_outA, (size_t)B)) != LF_OK) return rc;
    std::memcpy(out, c->h_out, (size_t)B * sizeof(double));
    return LF_OK;
}

int lf_lnprob_err_grad_batch_device(lf_ctx* c, const double* d_theta, int B, double* d_lnprob_err, double* d_grad, void* hip_stream) {
    int rc = family_check(c, "lf_lnprob_err_grad_batch_device", true, d_theta, B, d_grad);
    if (rc != LF_OK) return rc;
    if (!c->opt_cut_grad && (rc = cut_refuse(c, "lf_lnprob_err_grad_batch_device", "the gradient of Delta B, the cut's change of the expected counts, is not provided")) != LF_OK) return rc;
    LF_HIP(c, hipSetDevice(c->device));
    // (the rows' plain lnprob, and the value when it is not asked for: into the context's own buffers, sized before the
    // lnprob path may replace them)
    if ((rc = ensure_workspace(c, B, 0, 0)) != LF_OK) return rc;
    return enqueue_deconv_grad(c, d_theta, B, c->d_outB, d_lnprob_err ? d_lnprob_err : c->d_outA.get(), d_grad, (hipStream_t)hip_stream);
}

int lf_lnprob_err_grad_batch(lf_ctx* c, const double* theta, int B, double* lnprob_err, double* grad) {
    int rc = family_check(c, "lf_lnprob_err_grad_batch", true, theta, B, grad);
    if (rc != LF_OK) return rc;
    if (!c->opt_cut_grad && (rc = cut_refuse(c, "lf_lnprob_err_grad_batch", "the gradient of Delta B, the cut's change of the expected counts, is not provided")) != LF_OK) return rc;
    return host_value_grad(c, theta, B, lnprob_err, grad, [&](double* d_val, double* d_grad) {
        return enqueue_deconv_grad(c, c->d_theta, B, c->d_outB, d_val, d_grad, c->stream);
    });
}

int lf_lum_posterior_info(int* row_tile, int* max_rows) {
    if (row_tile) *row_tile = lf::LUMPOST_RT;
    if (max_rows) *max_rows = lf::LUMPOST_MAX_ROWS;
    return LF_OK;
}

int lf_lum_posterior(lf_ctx* c, const double* theta, int R, double* m1, double* m2, int* n_used) {
    using namespace lf;
    int rc = family_check(c, "lf_lum_posterior", true, theta, R, m1);
    if (rc != LF_OK) return rc;
    if (!m2 || !n_used || R > LUMPOST_MAX_ROWS) {
        c->err = "lf_lum_posterior: NULL pointer or R outside 1.." + std::to_string(LUMPOST_MAX_ROWS);
        return LF_ERR_ARG;
    }
    if ((rc = stage_theta(c, theta, R)) != LF_OK) return rc;
    if ((rc = src_chunk_table(c)) != LF_OK) return rc;
    const size_t N = (size_t)c->N, ns = (size_t)c->lp_nslots;
    const size_t need = std::max<size_t>((2 * LUMPOST_SLABS + 2) * ns + 2 * N, 1);
    if (need > c->d_lumpost.size() && (rc = grow(c, c->d_lumpost, need)) != LF_OK) return rc;
    // the rows' plain lnprob decides which are used: R' is counted here, the kernels read the same array
    double* d_lnp = c->d_outB;
    if ((rc = enqueue(c, c->d_theta, R, d_lnp, nullptr, nullptr, c->stream)) != LF_OK) return rc;
    if ((rc = fetch(c, c->h_out, d_lnp, (size_t)R)) != LF_OK) return rc;
    int used = 0;
    for (int r = 0; r < R; ++r) used += std::isfinite(c->h_out[r]) ? 1 : 0;
    *n_used = used;
    if (N == 0) return LF_OK;
    LumPostArgs x{};
    x.d = deconv_args(c, c->d_theta, d_lnp, nullptr);
    if (c->wide.n) x.w = deconv_wide_args(c, x.d);
    x.n0 = c->src_chunks.n, x.nw = c->wide.n, x.N = (int)N, x.nslots = (int)ns;
    x.slab = c->d_lumpost;
    x.run = x.slab + 2 * LUMPOST_SLABS * ns;
    x.m1 = x.run + 2 * ns, x.m2 = x.m1 + N;
    x.caller = c->d_lp_caller;
    LF_HIP(c, hipMemsetAsync(x.m1, 0, 2 * N * sizeof(double), c->stream));
    // groups of LUMPOST_SLABS tiles: the tiles' sums, then their fold into the running sums; no used row: the fold alone (NaN)
    constexpr int GROUP = LUMPOST_RT * LUMPOST_SLABS;
    const int ngroups = used > 0 ? (R + GROUP - 1) / GROUP : 1;
    const unsigned fblocks = (unsigned)((ns + BLOCK - 1) / BLOCK);
    launch_rows(c->kc.variant, 1, [&](auto v, int, int) {
        for (int g = 0; g < ngroups; ++g) {
            const int row0 = g * GROUP;
            const int ntiles = used > 0 ? std::min(LUMPOST_SLABS, (R - row0 + LUMPOST_RT - 1) / LUMPOST_RT) : 0;
            if (ntiles > 0)
                hipLaunchKernelGGL(lf_lumpost_part<v()>, dim3((unsigned)(x.n0 + x.nw), (unsigned)ntiles), dim3(BLOCK), 0, c->stream, x, row0, R);
            hipLaunchKernelGGL(lf_lumpost_fold, dim3(fblocks), dim3(BLOCK), 0, c->stream, x, ntiles, g == 0 ? 1 : 0,
                               g == ngroups - 1 ? 1 : 0, used);
        }
    });
    LF_HIP(c, hipGetLastError());
    LF_HIP(c, hipMemcpyAsync(m1, x.m1, N * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    LF_HIP(c, hipMemcpyAsync(m2, x.m2, N * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    LF_HIP(c, hipStreamSynchronize(c->stream));
    return LF_OK;
}

static double g_vefft_ms[3] = {-1.0, -1.0, -1.0};      // device times of the last lf_veff_true call's three stages under lf_set_profiling (any context's)

int lf_veff_true_info(int* max_rows, int* max_bins) {
    if (max_rows) *max_rows = lf::VEFFT_MAX_ROWS;
    if (max_bins) *max_bins = lf::VEFFT_MAXBIN;
    return lf::VEFFT_ROWS;
}

int lf_veff_true_ms(double ms[3]) {
    if (!ms) return LF_ERR_ARG;
    for (int s = 0; s < 3; ++s) ms[s] = g_vefft_ms[s];
    return g_vefft_ms[0] < 0.0 ? LF_ERR_ARG : LF_OK;
}

namespace {
// the events around every launch of lf_veff_true: made as they are recorded, destroyed with the call
struct Stamps {
    std::vector<hipEvent_t> ev;
    ~Stamps() {
        for (hipEvent_t e : ev) hipEventDestroy(e);
    }
    hipError_t mark(hipStream_t s) {
        hipEvent_t e;
        hipError_t rc = hipEventCreate(&e);
        if (rc != hipSuccess) return rc;
        ev.push_back(e);
        return hipEventRecord(e, s);
    }
};
}  // namespace

namespace {
// The cut model's image for lf_vefftrue_cut.h - lam, ld2, wv = wz V, the error model - to the device, once per error model.
// wv and its sum are formed here with the statements of deconv.py: cut_volume_fraction (no contraction, left to right).
int cut_volume_image(lf_ctx* c, const char* fn) {
#pragma clang fp contract(off)
    auto& v = c->cutv;
    if (v.img) return LF_OK;
    const int S = c->kc.S, M = c->cut.M, nf = c->kc.nf;
    if (lf::vefft_cut_lds_bytes(S, M, nf) > 60 * 1024) {
        c->err = std::string(fn) + ": the grid's " + std::to_string(S) + " redshift columns and the error model's " + std::to_string(M) +
                 " nodes need " + std::to_string(lf::vefft_cut_lds_bytes(S, M, nf)) + " bytes of LDS, above the 61440 the kernel stages";
        return LF_ERR_ARG;
    }
    std::vector<double> img((size_t)lf::vefft_cut_slots(S, M, nf));
    double den = 0.0;
    for (int j = 0; j < S; ++j) {
        const double dl = j > 0 ? c->h_zarr[j] - c->h_zarr[j - 1] : 0.0, dr = j < S - 1 ? c->h_zarr[j + 1] - c->h_zarr[j] : 0.0;
        const double wz = 0.5 * (dl + dr);
        const double wv = wz * c->h_vol[j];
        img[(size_t)j] = c->h_edge_lo[j], img[(size_t)S + j] = c->h_ld2[j], img[(size_t)2 * S + j] = wv;
        den += wv;
    }
    unsigned step = 0;
    for (int m = 0; m < M; ++m) img[(size_t)3 * S + m] = c->cut.nodes[m];
    for (int f = 0; f < nf; ++f) {
        bool zero = true;
        for (int m = 0; m < M; ++m) {
            const double sg = c->cut.sigma[(size_t)f * M + m];
            img[(size_t)3 * S + M + (size_t)f * M + m] = sg;
            zero = zero && sg == 0.0;
        }
        step |= zero ? 1u << f : 0u;
    }
    if (!(den > 0.0) || !std::isfinite(den)) {
        c->err = std::string(fn) + ": the grid's volume, the sum of wz V over the redshift columns, is not finite and > 0";
        return LF_ERR_ARG;
    }
    const int rc = upload(c, v.d_img, img);
    if (rc != LF_OK) return rc;
    v.tab = lf::VeffCutTab{v.d_img, S, M, nf, step, den, 0.0};
    v.img = true;
    return LF_OK;
}

// The table of 1 / g per (source, node) slot (lf_vefftrue_cutvol), made when it is missing or was made for another
// min_vol_frac.  x: the call's arguments (the chunk tables and the sources' arrays).
int cut_volume_table(lf_ctx* c, const char* fn, const lf::VeffTrueArgs& x, double min_vol_frac) {
    using namespace lf;
    auto& v = c->cutv;
    if (v.built && v.min_vol_frac == min_vol_frac) return LF_OK;
    int rc = cut_volume_image(c, fn);
    if (rc != LF_OK) return rc;
    v.built = false;
    const size_t N = (size_t)c->N, nwide = (size_t)c->lp_nslots - N;
    const size_t slots = N * (size_t)x.d.dc.K + nwide * (size_t)DECONV_WIDE_KMAX;
    const size_t nch = (size_t)(x.n0 + x.nw);
    if (slots > v.d_invg.size()) {
        LF_HIP(c, hipDeviceSynchronize());
        if (v.d_invg.alloc(slots) != hipSuccess) {
            (void)hipGetLastError();
            c->err = std::string(fn) + ": no device memory for the table of catalogued volumes: " + std::to_string(slots) +
                     " (source, node) slots of 8 bytes, " + std::to_string(slots * 8) + " bytes (option deconv_cut_veff)";
            return LF_ERR_NOMEM;
        }
    }
    if (nch > v.d_drop.size() && (rc = grow(c, v.d_drop, nch)) != LF_OK) return rc;
    v.slots = slots, v.wide_off = (long long)(N * (size_t)x.d.dc.K);
    VeffCutTab t = v.tab;
    t.min_vol_frac = min_vol_frac;
    Stamps st;
    LF_HIP(c, hipMemsetAsync(v.d_invg, 0, slots * sizeof(double), c->stream));
    LF_HIP(c, st.mark(c->stream));
    if (nch > 0)
        hipLaunchKernelGGL(lf_vefftrue_cutvol, dim3((unsigned)nch), dim3(BLOCK), (unsigned)vefft_cut_lds_bytes(t.S, t.M, t.nf), c->stream, x, t,
                           v.d_invg.get(), v.wide_off, v.d_drop.get());
    LF_HIP(c, hipGetLastError());
    LF_HIP(c, st.mark(c->stream));
    std::vector<int> drop(nch, 0);
    if (nch > 0) LF_HIP(c, hipMemcpyAsync(drop.data(), v.d_drop, nch * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    LF_HIP(c, hipStreamSynchronize(c->stream));
    float ms = 0.0f;
    LF_HIP(c, hipEventElapsedTime(&ms, st.ev[0], st.ev[1]));
    v.ms = ms;
    v.dropped = 0;
    for (int d : drop) v.dropped += d;
    v.min_vol_frac = min_vol_frac;
    v.built = true;
    return LF_OK;
}

int veff_true_host(lf_ctx* c, const char* fn, const double* theta, int R, const double* edges, int nbin, double pref0, double vol,
                   double min_vol_frac, int nq, const double* q, int method, double* out, double* values, int* n_used);
}  // namespace

int lf_veff_true(lf_ctx* c, const double* theta, int R, const double* edges, int nbin, double pref0, double vol, int nq, const double* q,
                 int method, double* out, double* values, int* n_used) {
    return veff_true_host(c, "lf_veff_true", theta, R, edges, nbin, pref0, vol, 0.0, nq, q, method, out, values, n_used);
}

int lf_veff_true_cut(lf_ctx* c, const double* theta, int R, const double* edges, int nbin, double pref0, double vol, double min_vol_frac,
                     int nq, const double* q, int method, double* out, double* values, int* n_used) {
    return veff_true_host(c, "lf_veff_true_cut", theta, R, edges, nbin, pref0, vol, min_vol_frac, nq, q, method, out, values, n_used);
}

int lf_veff_true_cut_info(lf_ctx* c, int64_t* slots, int64_t* bytes, int64_t* dropped) {
    if (!c) return LF_ERR_ARG;
    if (!c->cutv.built) {
        c->err = "lf_veff_true_cut_info: no table of catalogued volumes yet (option deconv_cut_veff, a cut model, then lf_veff_true)";
        return LF_ERR_ARG;
    }
    if (slots) *slots = (int64_t)c->cutv.slots;
    if (bytes) *bytes = (int64_t)(c->cutv.slots * sizeof(double));
    if (dropped) *dropped = (int64_t)c->cutv.dropped;
    return LF_OK;
}

int lf_veff_true_cut_ms(lf_ctx* c, double* ms) {
    if (!c || !ms) return LF_ERR_ARG;
    *ms = c->cutv.ms;
    return c->cutv.ms < 0.0 ? LF_ERR_ARG : LF_OK;
}

int lf_cut_volume(lf_ctx* c, const int32_t* field, const double* L, int64_t n, double* g_out) {
    using namespace lf;
    if (!c) return LF_ERR_ARG;
    auto bad = [&](const std::string& m) {
        c->err = "lf_cut_volume: " + m;
        return (int)LF_ERR_ARG;
    };
    if (!c->cut.model) return bad("no cut model set (call lf_set_cut_error_model first)");
    if (n < 1 || n > (int64_t)1 << 24) return bad("n outside 1..16777216");
    if (!field || !L || !g_out) return bad("NULL pointer");
    for (int64_t i = 0; i < n; ++i) {
        if (field[i] < 0 || field[i] >= c->kc.nf) return bad("field outside 0.." + std::to_string(c->kc.nf - 1) + " (point " + std::to_string(i) + ")");
        if (!std::isfinite(L[i])) return bad("L must be finite (point " + std::to_string(i) + ")");
    }
    LF_HIP(c, hipSetDevice(c->device));
    int rc = cut_volume_image(c, "lf_cut_volume");
    if (rc != LF_OK) return rc;
    Buf<double> d_L, d_g;
    Buf<int> d_f;
    LF_HIP(c, d_L.upload(L, (size_t)n));
    LF_HIP(c, d_f.upload(field, (size_t)n));
    LF_HIP(c, d_g.alloc((size_t)n));
    const VeffCutTab t = c->cutv.tab;
    hipLaunchKernelGGL(lf_cut_volume_points, dim3((unsigned)((n + BLOCK - 1) / BLOCK)), dim3(BLOCK), (unsigned)vefft_cut_lds_bytes(t.S, t.M, t.nf),
                       c->stream, t, d_f.get(), d_L.get(), (int)n, d_g.get());
    LF_HIP(c, hipGetLastError());
    LF_HIP(c, hipMemcpyAsync(g_out, d_g, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    LF_HIP(c, hipStreamSynchronize(c->stream));
    return LF_OK;
}

namespace {
int veff_true_host(lf_ctx* c, const char* fn, const double* theta, int R, const double* edges, int nbin, double pref0, double vol,
                   double min_vol_frac, int nq, const double* q, int method, double* out, double* values, int* n_used) {
    using namespace lf;
    // every argument is checked before the device is touched
    int rc = family_check(c, fn, true, theta, R, out);
    if (rc != LF_OK) return rc;
    if (!c->opt_cut_veff &&
        (rc = cut_refuse(c, fn, "per-source volumes (a z_max per source under the cut) are not provided: the points take one volume")) != LF_OK)
        return rc;
    const bool cut = c->cut.model;
    auto bad = [&](const std::string& m) {
        c->err = std::string(fn) + ": " + m;
        return (int)LF_ERR_ARG;
    };
    if (!(min_vol_frac >= 0.0) || !(min_vol_frac <= 1.0)) return bad("min_vol_frac outside 0..1");
    if (min_vol_frac > 0.0 && !cut) return bad("min_vol_frac > 0 needs a cut model (lf_set_cut_error_model): without one every node has the whole volume");
    if (!edges || !n_used) return bad("NULL pointer");
    if (R > VEFFT_MAX_ROWS) return bad("R outside 1.." + std::to_string(VEFFT_MAX_ROWS));
    if (nbin < 1 || nbin > VEFFT_MAXBIN) return bad("nbin outside 1.." + std::to_string(VEFFT_MAXBIN));
    for (int b = 0; b <= nbin; ++b)
        if (!std::isfinite(edges[b]) || (b > 0 && !(edges[b] > edges[b - 1]))) return bad("edges must be finite and strictly ascending");
    if (!(pref0 > 0.0) || !(vol > 0.0) || !std::isfinite(pref0) || !std::isfinite(vol)) return bad("pref0 and vol must be finite and > 0");
    if (!lfh::quantiles(R, nq, q, method, BANDS_MAXQ).ok) return bad("bad nq, q or method");
    if ((rc = stage_theta(c, theta, R)) != LF_OK) return rc;
    if ((rc = src_chunk_table(c)) != LF_OK) return rc;
    // the rows' plain lnprob decides which are used: R' is counted here, the kernels read the same array
    double* d_lnp = c->d_outB;
    if ((rc = enqueue(c, c->d_theta, R, d_lnp, nullptr, nullptr, c->stream)) != LF_OK) return rc;
    if ((rc = fetch(c, c->h_out, d_lnp, (size_t)R)) != LF_OK) return rc;
    std::vector<int> slot((size_t)R, 0);
    int used = 0;
    for (int r = 0; r < R; ++r) {
        slot[(size_t)r] = used;
        used += std::isfinite(c->h_out[r]) ? 1 : 0;
    }
    *n_used = used;
    for (double& t : g_vefft_ms) t = -1.0;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    const size_t nb = (size_t)nbin;
    if (used == 0) {
        std::fill(out, out + (size_t)nq * nb, nan);
        if (values) std::fill(values, values + (size_t)R * nb, nan);
        return LF_OK;
    }
    const lfh::Quantiles qt = lfh::quantiles(used, nq, q, method, BANDS_MAXQ);
    VeffTrueArgs x{};
    x.d = deconv_args(c, c->d_theta, d_lnp, nullptr);
    if (c->wide.n) x.w = deconv_wide_args(c, x.d);
    x.n0 = c->N > 0 ? c->src_chunks.n : 0, x.nw = c->wide.n;
    x.in_wide = c->d_vt_inwide;
    x.nbin = nbin;
    x.pv = pref0 * vol;
    const size_t nch = (size_t)(x.n0 + x.nw);
    // one workspace on the context, grown when a call needs more: edges | quantile table | partial | values | used | out
    const size_t o_q = nb + 1, o_part = o_q + qt.tab.size(), o_val = o_part + nch * VEFFT_ROWS * nb, o_used = o_val + (size_t)R * nb,
                 o_out = o_used + (size_t)used * nb, need = o_out + (size_t)nq * nb;
    if (need > c->d_vt_work.size() && (rc = grow(c, c->d_vt_work, need)) != LF_OK) return rc;
    if ((size_t)R > c->d_vt_slot.size() && (rc = grow(c, c->d_vt_slot, (size_t)R)) != LF_OK) return rc;
    double* wk = c->d_vt_work;
    LF_HIP(c, hipMemcpyAsync(wk, edges, (nb + 1) * sizeof(double), hipMemcpyHostToDevice, c->stream));
    LF_HIP(c, hipMemcpyAsync(wk + o_q, qt.tab.data(), qt.tab.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
    LF_HIP(c, hipMemcpyAsync(c->d_vt_slot, slot.data(), (size_t)R * sizeof(int), hipMemcpyHostToDevice, c->stream));
    LF_HIP(c, hipStreamSynchronize(c->stream));            // (the sources of the copies are this call's own)
    x.edges = wk, x.partial = wk + o_part, x.values = wk + o_val, x.used = wk + o_used, x.slot = c->d_vt_slot;
    if (cut && (rc = cut_volume_table(c, fn, x, min_vol_frac)) != LF_OK) return rc;
    const double* d_invg = c->cutv.d_invg;
    const long long wide_off = c->cutv.wide_off;
    double *d_q = wk + o_q, *d_used = wk + o_used, *d_out = wk + o_out, *d_val = wk + o_val;
    // the stages' times are taken only under lf_set_profiling: an event pair around every launch keeps it from overlapping the
    // one before
    const bool timed = c->profiling > 0;
    Stamps st;
    const unsigned bblocks = (unsigned)((nbin + BLOCK - 1) / BLOCK);
    const unsigned lds = (unsigned)vefft_dyn_lds_bytes(nbin);
    hipError_t he = hipSuccess;
    launch_rows(c->kc.variant, 1, [&](auto v, int, int) {
        for (int row0 = 0; row0 < R && he == hipSuccess; row0 += VEFFT_ROWS) {
            const unsigned nr = (unsigned)std::min(VEFFT_ROWS, R - row0);
            if (timed && (he = st.mark(c->stream)) != hipSuccess) break;
            if (nch > 0 && cut)
                hipLaunchKernelGGL(lf_vefftrue_part_cut<v()>, dim3((unsigned)nch, nr), dim3(BLOCK), lds, c->stream, x, row0, d_invg, wide_off);
            else if (nch > 0)
                hipLaunchKernelGGL(lf_vefftrue_part<v()>, dim3((unsigned)nch, nr), dim3(BLOCK), lds, c->stream, x, row0);
            if (timed && (he = st.mark(c->stream)) != hipSuccess) break;
            hipLaunchKernelGGL(lf_vefftrue_reduce, dim3(bblocks, nr), dim3(BLOCK), 0, c->stream, x, row0);
        }
    });
    LF_HIP(c, he);
    LF_HIP(c, hipGetLastError());
    if (timed) LF_HIP(c, st.mark(c->stream));
    const int G = BANDS_SLOTS >> qt.lg;
    hipLaunchKernelGGL(veffd_quant, dim3((unsigned)((nbin + G - 1) / G)), dim3(BANDS_THREADS), 0, c->stream, d_used, used, qt.lg, nbin, d_q,
                       nq, method == LF_Q_MEDIAN ? 1 : 0, d_out);
    LF_HIP(c, hipGetLastError());
    if (timed) LF_HIP(c, st.mark(c->stream));
    LF_HIP(c, hipMemcpyAsync(out, d_out, (size_t)nq * nb * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (values) LF_HIP(c, hipMemcpyAsync(values, d_val, (size_t)R * nb * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    LF_HIP(c, hipStreamSynchronize(c->stream));
    // part: the even intervals, reduce: the odd ones (the last ends at the quantile stage's first stamp), then the quantiles
    double ms[3] = {0.0, 0.0, 0.0};
    const size_t ne = st.ev.size();
    for (size_t i = 0; i + 1 < ne; ++i) {
        float t = 0.0f;
        LF_HIP(c, hipEventElapsedTime(&t, st.ev[i], st.ev[i + 1]));
        ms[i + 2 == ne ? 2 : (i & 1)] += t;
    }
    for (int s = 0; s < 3 && timed; ++s) g_vefft_ms[s] = ms[s];
    return LF_OK;
}
}  // namespace

int lf_set_profiling(lf_ctx* c, int enabled) {
    if (!c) return LF_ERR_ARG;
    c->profiling = enabled < 0 ? 0 : (enabled > 2 ? 2 : enabled);
    return LF_OK;
}

int lf_kernel_times(lf_ctx* c, double ms[4], int64_t launches[4]) {
    if (!c || !ms || !launches) return LF_ERR_ARG;
    LF_HIP(c, hipSetDevice(c->device));
    if (c->span_open) {                  // (a span cut short: what it holds so far)
        if (c->span_ep.count > 0) {
            hipEventRecord(c->span_ep.b, c->last_stream);
            c->events.push_back(c->span_ep);
        } else {
            hipEventDestroy(c->span_ep.a);
            hipEventDestroy(c->span_ep.b);
        }
        c->span_open = false;
    }
    for (auto& e : c->events) {
        LF_HIP(c, hipEventSynchronize(e.b));
        float t = 0.f;
        LF_HIP(c, hipEventElapsedTime(&t, e.a, e.b));
        c->acc_ms[e.kind] += t;
        c->acc_n[e.kind] += e.count;
        hipEventDestroy(e.a);
        hipEventDestroy(e.b);
    }
    c->events.clear();
    for (int i = 0; i < 4; ++i) {
        ms[i] = c->acc_ms[i];
        launches[i] = c->acc_n[i];
        c->acc_ms[i] = 0;
        c->acc_n[i] = 0;
    }
    return LF_OK;
}

#ifdef LF_STAMPS
// diagnostic build only (tools/stamps.py): arm / read the per-workgroup time stamps of lf_main's source workgroups
int lf_debug_stamps(lf_ctx* c, uint64_t* out, int64_t nblocks) {
    if (!c) return LF_ERR_ARG;
    LF_HIP(c, hipSetDevice(c->device));
    LF_HIP(c, hipDeviceSynchronize());
    if (!out) {                                   // arm for nblocks workgroups
        c->d_stamps.reset();
        c->kc.stamps = nullptr;
        if (nblocks > 0) {
            const int rc = grow(c, c->d_stamps, (size_t)nblocks * 8, false);       // (the device is idle already)
            if (rc != LF_OK) return rc;
            LF_HIP(c, hipMemset(c->d_stamps, 0, (size_t)nblocks * 8 * sizeof(uint64_t)));
            c->kc.stamps = c->d_stamps;
        }
        return LF_OK;
    }
    if (!c->kc.stamps) return LF_ERR_ARG;
    LF_HIP(c, hipMemcpy(out, c->kc.stamps, (size_t)nblocks * 8 * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return LF_OK;
}
#endif

int lf_veff(int device, int64_t n, const double* flux, const double* flim, const double* vol, double vol_all, double pref0,
            double alpha, double fcmin, const int32_t* bin_of, int32_t nbin, int32_t nboot, const int64_t* boot_idx, uint64_t seed,
            double* phi, double* sums) {
    if (n <= 0 || !flux || !flim || !phi || pref0 <= 0.0 || nbin < 0 || nbin > lf::VEFF_MAXBIN || nboot < 0 || (nbin > 0 && (!bin_of || !sums)))
        return LF_ERR_ARG;
    // the caller's resampling indices address phi and bin_of on the device: outside [0, n) they are refused here
    if (boot_idx && nbin > 0)
        for (int64_t i = 0; i < n * (int64_t)nboot; ++i)
            if (boot_idx[i] < 0 || boot_idx[i] >= n) return LF_ERR_ARG;
    if (hipSetDevice(device) != hipSuccess) return LF_ERR_NODEV;
    Buf<double> d_flux, d_flim, d_vol, d_phi, d_sums;
    Buf<int> d_bin;
    Buf<long long> d_idx;
    const size_t nb = (size_t)n * sizeof(double);
    HostCall hc;
    if (hc.ok(alloc_all(d_flux, (size_t)n, d_flim, (size_t)n, d_phi, (size_t)n)) && (!vol || hc.ok(d_vol.alloc((size_t)n)))) {
        hc.ok(hipMemcpy(d_flux, flux, nb, hipMemcpyHostToDevice));
        hc.ok(hipMemcpy(d_flim, flim, nb, hipMemcpyHostToDevice));
        if (vol) hc.ok(hipMemcpy(d_vol, vol, nb, hipMemcpyHostToDevice));
        if (hc.rc == LF_OK) {
            hipLaunchKernelGGL(lf::veff_weights, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, d_flux, d_flim, d_vol, vol_all, pref0,
                               alpha, fcmin > 0.0 ? lfh::fc_ratio(fcmin) : 0.0, fcmin > 0.0 ? 1 : 0, (long long)n, d_phi);
            hc.ok(hipGetLastError());
        }
        if (hc.rc == LF_OK && nbin > 0) {
            const size_t sb = (size_t)(nboot + 1) * nbin * sizeof(double);
            if (hc.ok(alloc_all(d_bin, (size_t)n, d_sums, (size_t)(nboot + 1) * nbin)) && (!boot_idx || hc.ok(d_idx.alloc((size_t)n * nboot)))) {
                hc.ok(hipMemcpy(d_bin, bin_of, (size_t)n * sizeof(int), hipMemcpyHostToDevice));
                hc.ok(hipMemset(d_sums, 0, sb));
                if (boot_idx) hc.ok(hipMemcpy(d_idx, boot_idx, (size_t)n * nboot * sizeof(long long), hipMemcpyHostToDevice));
                if (hc.rc == LF_OK) {
                    const unsigned gx = (unsigned)std::min<int64_t>((n + 255) / 256, 1024);
                    hipLaunchKernelGGL(lf::veff_bins, dim3(gx, (unsigned)(nboot + 1)), dim3(256), 0, 0, d_phi, d_bin, (long long)n, nbin,
                                       d_idx, (unsigned long long)seed, d_sums);
                    hc.ok(hipGetLastError());
                    hc.ok(hipMemcpy(sums, d_sums, sb, hipMemcpyDeviceToHost));
                }
            }
        }
        if (hc.rc == LF_OK) hc.ok(hipMemcpy(phi, d_phi, nb, hipMemcpyDeviceToHost));
    }
    return hc.rc;
}

static double g_veffs_ms = -1.0;      // device time of the last lf_veff_slices call's two kernels (veffs_partial, veffs_reduce)

int lf_veff_slices(int device, int64_t n, const double* flux, const double* flim, const double* vol, double pref0, double alpha, double fcmin,
                   const int32_t* slice_of, int32_t nslice, const int32_t* bin_of, int32_t nbin, int32_t nboot, const int64_t* boot_idx,
                   uint64_t seed, double* phi, double* sums, int64_t* counts) {
    // every argument is checked before the device is touched
    if (!flux || !flim || !vol || !slice_of || !bin_of || !phi || !sums || !counts || n <= 0 || n > (int64_t)INT32_MAX || nslice < 1 ||
        nslice > lf::VEFFS_MAXSLICE || nbin < 1 || nbin > lf::VEFFS_MAXBIN || nboot < 0 || nboot > lf::VEFFS_MAXBOOT || !(pref0 > 0.0))
        return LF_ERR_ARG;
    // stable counting sort of the sources by slice; a source outside [0, nslice) has no slice and enters no sum
    std::vector<int> off((size_t)nslice + 1, 0);
    for (int64_t i = 0; i < n; ++i)
        if (slice_of[i] >= 0 && slice_of[i] < nslice) ++off[(size_t)slice_of[i] + 1];
    for (int s = 0; s < nslice; ++s) off[s + 1] += off[s];
    const int m = off[nslice];
    std::vector<int> order((size_t)m);
    {
        std::vector<int> at(off.begin(), off.end() - 1);
        for (int64_t i = 0; i < n; ++i)
            if (slice_of[i] >= 0 && slice_of[i] < nslice) order[(size_t)at[slice_of[i]]++] = (int)i;
    }
    // the caller's resampling indices address the slice's records on the device: outside [0, n_s) they are refused here
    if (boot_idx)
        for (int k = 0; k < nboot; ++k)
            for (int s = 0; s < nslice; ++s) {
                const int64_t ns = off[s + 1] - off[s];
                const int64_t* row = boot_idx + (size_t)k * (size_t)m;
                for (int p = off[s]; p < off[s + 1]; ++p)
                    if (row[p] < 0 || row[p] >= ns) return LF_ERR_ARG;
            }
    // chunks of at most VEFFS_CHUNK draws within a slice; c0[s] = the first chunk of slice s
    std::vector<lf::VeffsChunk> chunks;
    std::vector<int> c0((size_t)nslice + 1, 0);
    for (int s = 0; s < nslice; ++s) {
        c0[s] = (int)chunks.size();
        const int ns = off[s + 1] - off[s];
        for (int f = 0; f < ns; f += lf::VEFFS_CHUNK) chunks.push_back({s, f, std::min(lf::VEFFS_CHUNK, ns - f), off[s], ns, 0});
    }
    const size_t nch = chunks.size();
    c0[nslice] = (int)nch;
    const int nres = nboot + 1;
    const size_t cells = (size_t)nslice * nbin;
    if (hipSetDevice(device) != hipSuccess) return LF_ERR_NODEV;
    Buf<double> d_flux, d_flim, d_vol, d_phi, d_part, d_sums;
    Buf<int> d_slice, d_bin, d_order, d_c0;
    Buf<long long> d_idx;
    Buf<unsigned long long> d_counts;
    Buf<lf::VeffsRec> d_rec;
    Buf<lf::VeffsChunk> d_chunk;
    HostCall hc;
    g_veffs_ms = -1.0;
    static_assert(sizeof(int) == sizeof(int32_t) && sizeof(long long) == sizeof(int64_t), "the caller's arrays are uploaded as they are");
    if (hc.ok(d_flux.upload(flux, (size_t)n)) && hc.ok(d_flim.upload(flim, (size_t)n)) && hc.ok(d_vol.upload(vol, (size_t)n)) &&
        hc.ok(d_slice.upload(slice_of, (size_t)n)) && hc.ok(d_bin.upload(bin_of, (size_t)n)) && hc.ok(d_order.upload(order.data(), (size_t)m)) &&
        hc.ok(d_chunk.upload(chunks.data(), nch)) && hc.ok(d_c0.upload(c0.data(), c0.size())) &&
        (!boot_idx || hc.ok(d_idx.upload((const long long*)boot_idx, (size_t)nboot * (size_t)m))) &&
        hc.ok(alloc_all(d_phi, (size_t)n, d_rec, (size_t)m, d_part, (size_t)nres * nch * nbin, d_sums, (size_t)nres * cells, d_counts, cells)) &&
        hc.ok(hipMemset(d_counts, 0, cells * sizeof(unsigned long long)))) {
        hipLaunchKernelGGL(lf::veff_weights, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, d_flux, d_flim, d_vol, 0.0, pref0, alpha,
                           fcmin > 0.0 ? lfh::fc_ratio(fcmin) : 0.0, fcmin > 0.0 ? 1 : 0, (long long)n, d_phi);
        hc.ok(hipGetLastError());
        if (m > 0) {
            hipLaunchKernelGGL(lf::veffs_pack, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, 0, d_phi, d_slice, d_bin, d_order, m, (int)nbin, d_rec);
            hc.ok(hipGetLastError());
        }
        hc.stamp(0, 0);
        if (nch > 0) {
            // the smallest instantiation that holds the call's bins: the most lanes
            auto kernel = nbin <= 16 ? lf::veffs_partial<16> : (nbin <= 32 ? lf::veffs_partial<32> : lf::veffs_partial<64>);
            const unsigned lanes = (unsigned)(lf::VEFFS_LDS_DOUBLES / (nbin <= 16 ? 16 : (nbin <= 32 ? 32 : 64)));
            hipLaunchKernelGGL(kernel, dim3((unsigned)nch, (unsigned)nres), dim3(lanes), 0, 0, d_rec, d_chunk, (int)nch, (int)nbin, d_idx,
                               (long long)m, (unsigned long long)seed, d_part);
            hc.ok(hipGetLastError());
        }
        // enough workgroups for the (k, s, b) sums, and for the last row's pass over the records
        const unsigned gx = (unsigned)std::max<size_t>((cells + lf::VEFFS_REDUCE_THREADS - 1) / lf::VEFFS_REDUCE_THREADS,
                                                       std::min<size_t>(((size_t)m + 4095) / 4096, 256));
        hipLaunchKernelGGL(lf::veffs_reduce, dim3(gx, (unsigned)nres + 1), dim3(lf::VEFFS_REDUCE_THREADS), 0, 0, d_part, d_c0, (int)nch, (int)nslice,
                           (int)nbin, nres, d_rec, m, d_sums, d_counts);
        hc.ok(hipGetLastError());
        hc.stamp(1, 0);
        hc.ok(hipMemcpy(sums, d_sums, (size_t)nres * cells * sizeof(double), hipMemcpyDeviceToHost));
        hc.ok(hipMemcpy(counts, d_counts, cells * sizeof(int64_t), hipMemcpyDeviceToHost));
        hc.ok(hipMemcpy(phi, d_phi, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
        hc.elapsed(0, 1, &g_veffs_ms);
        if (hc.rc != LF_OK) g_veffs_ms = -1.0;
    }
    return hc.rc;
}

double lf_veff_slices_ms(void) { return g_veffs_ms; }

static double g_bands_ms = -1.0;      // device time of the last lf_lumfunc_quantiles kernel (lf_lumfunc_quantiles_ms)
static double g_integ_ms = -1.0;      // the same of lf_lumfunc_integral_quantiles

// lf_lumfunc_quantiles (kind < 0: the differential LF, lf_bands) and lf_lumfunc_integral_quantiles (kind LF_INT_NUMBER /
// LF_INT_LUMDENS: lf_bands_integ, logL holds the lower limits) share everything but the per-draw factors and the kernel.
static int bands_run(int device, int variant, int kind, int32_t R, const double* draws, int64_t P, const double* logL, const double* z,
                     int32_t nq, const double* q, int32_t method, double* out, double* values, double* ms_out) {
#pragma clang fp contract(off)
    // every argument is checked before the device is touched
    if (variant < LF_FREE || variant > LF_ZEVOL || R < 1 || R > lf::BANDS_SLOTS || P < 1 || P > ((int64_t)1 << 40) || !draws ||
        !logL || !out || (variant == LF_ZEVOL && !z))
        return LF_ERR_ARG;
    const lfh::Quantiles qt = lfh::quantiles(R, nq, q, method, lf::BANDS_MAXQ);
    if (!qt.ok) return LF_ERR_ARG;
    const std::vector<double>& qtab = qt.tab;
    const int lg = qt.lg, np_in = variant == LF_ZEVOL ? 7 : 3;
    if (kind >= 0) {
        for (int r = 0; r < R; ++r) {
            const double al = draws[(size_t)r * np_in + np_in - 1];
            if (!(al >= -6.0 && al <= 5.0)) return LF_ERR_ARG;              // (NaN fails both)
        }
        for (int64_t p = 0; p < P; ++p)
            if (logL[p] != logL[p]) return LF_ERR_ARG;                      // -inf is allowed: x = 0
    }
    // the per-draw factors the kernel takes as they are (lf_bands.h): alpha + 1, and for the single Schechter
    // LN10 * 10^logphistar - numpy scalar operations in the reference, made here with the host's pow (a volatile base keeps
    // the compiler from turning pow(10, x) into exp10, which the C library does not round the same way)
    std::vector<double> rec((size_t)R * np_in);
    volatile double ten = 10.0;
    for (int r = 0; r < R; ++r) {
        const double* d = draws + (size_t)r * np_in;
        double* o = rec.data() + (size_t)r * np_in;
        if (np_in == 3) {
            o[0] = d[0];
            if (kind < 0)
                o[1] = 2.302585092994045684 * std::pow((double)ten, d[1]);
            else if (kind == LF_INT_LUMDENS)
                o[1] = std::pow((double)ten, d[1]) * std::pow((double)ten, d[0]);
            else
                o[1] = std::pow((double)ten, d[1]);
        } else {
            for (int c = 0; c < 6; ++c) o[c] = d[c];
        }
        o[np_in - 1] = d[np_in - 1] + 1.0;
        if (kind > 0) o[np_in - 1] = o[np_in - 1] + 1.0;          // (alpha + 1) + 1, as lfintegrals adds them
    }
    if (hipSetDevice(device) != hipSuccess) return LF_ERR_NODEV;
    Buf<double> d_rec, d_logL, d_z, d_q, d_out, d_val;
    const size_t pb = (size_t)P * sizeof(double);
    HostCall hc;
    *ms_out = -1.0;
    if (hc.ok(alloc_all(d_rec, rec.size(), d_logL, (size_t)P)) && (variant != LF_ZEVOL || hc.ok(d_z.alloc((size_t)P))) &&
        hc.ok(alloc_all(d_q, qtab.size(), d_out, (size_t)nq * P)) && (!values || hc.ok(d_val.alloc((size_t)R * P)))) {
        hc.ok(hipMemcpy(d_rec, rec.data(), rec.size() * sizeof(double), hipMemcpyHostToDevice));
        hc.ok(hipMemcpy(d_logL, logL, pb, hipMemcpyHostToDevice));
        if (d_z) hc.ok(hipMemcpy(d_z, z, pb, hipMemcpyHostToDevice));
        hc.ok(hipMemcpy(d_q, qtab.data(), qtab.size() * sizeof(double), hipMemcpyHostToDevice));
        if (hc.rc == LF_OK) {
            int ncu = 0;
            if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || ncu < 1) ncu = 256;
            const int64_t G = lf::BANDS_SLOTS >> lg;
            const unsigned grid = (unsigned)std::min<int64_t>((P + G - 1) / G, (int64_t)ncu * 5);       // five 32-KiB workgroups per CU (LDS)
            hc.stamp(0, 0);
            using kernel_t = void (*)(const double*, int, int, const double*, const double*, long long, const double*, int, int, double*,
                                      double*);
            const kernel_t kernels[3][2] = {{lf::lf_bands<3>, lf::lf_bands<7>},
                                            {lf::lf_bands_integ<3, 0>, lf::lf_bands_integ<7, 0>},
                                            {lf::lf_bands_integ<3, 1>, lf::lf_bands_integ<7, 1>}};
            hipLaunchKernelGGL(kernels[kind + 1][variant == LF_ZEVOL ? 1 : 0], dim3(grid), dim3(lf::BANDS_THREADS), 0, 0, d_rec, (int)R, lg,
                               d_logL, d_z, (long long)P, d_q, (int)nq, method == LF_Q_MEDIAN ? 1 : 0, d_out, d_val);
            hc.ok(hipGetLastError());
            hc.stamp(1, 0);
            hc.ok(hipMemcpy(out, d_out, (size_t)nq * pb, hipMemcpyDeviceToHost));
            if (values) hc.ok(hipMemcpy(values, d_val, (size_t)R * pb, hipMemcpyDeviceToHost));
            hc.elapsed(0, 1, ms_out);
        }
    }
    return hc.rc;
}

int lf_lumfunc_quantiles(int device, int variant, int32_t R, const double* draws, int64_t P, const double* logL, const double* z,
                         int32_t nq, const double* q, int32_t method, double* out, double* values) {
    return bands_run(device, variant, -1, R, draws, P, logL, z, nq, q, method, out, values, &g_bands_ms);
}

int lf_lumfunc_integral_quantiles(int device, int variant, int kind, int32_t R, const double* draws, int64_t P, const double* logLmin,
                                  const double* z, int32_t nq, const double* q, int32_t method, double* out, double* values) {
    if (kind != LF_INT_NUMBER && kind != LF_INT_LUMDENS) return LF_ERR_ARG;
    return bands_run(device, variant, kind, R, draws, P, logLmin, z, nq, q, method, out, values, &g_integ_ms);
}

int lf_lumfunc_integral_quantiles_ms(double* ms) {
    if (!ms) return LF_ERR_ARG;
    *ms = g_integ_ms;
    return g_integ_ms < 0.0 ? LF_ERR_ARG : LF_OK;
}

int lf_lumfunc_quantiles_ms(double* ms) {
    if (!ms) return LF_ERR_ARG;
    *ms = g_bands_ms;
    return g_bands_ms < 0.0 ? LF_ERR_ARG : LF_OK;
}

static double g_veffd_ms[3] = {-1.0, -1.0, -1.0};      // device times of the last lf_veff_draws / lf_veff_draws_zmax call's three stages

// The volume table of lf_veff_draws_zmax as the caller passes it (lumfuncmcmc_amd/voltable.py)
struct VeffzTable {
    const double *fmin, *head, *zc, *rec;
    int64_t nrec;
};

// every field of the table the kernel's search and clamps rely on: finite, edges strictly increasing and chained from D_0 to
// D_K, volumes non-decreasing from 0 to V_total > 0
static bool veffz_table_ok(const VeffzTable& t) {
    if (!t.head || !t.zc || !t.rec || t.nrec < 1 || t.nrec > (int64_t)INT32_MAX) return false;
    for (int j = 0; j < 6; ++j)
        if (!std::isfinite(t.head[j])) return false;
    const double d_lo = t.head[0], d_hi = t.head[1], v_total = t.head[2], invw = t.head[3];
    if (!(d_lo > 0.0) || !(d_hi > d_lo) || !(v_total > 0.0) || !(invw > 0.0) || !(t.head[5] >= 0.0)) return false;
    if (!((d_hi - d_lo) * invw <= lf::VEFFZ_NPIECE + 0.5)) return false;
    for (int j = 0; j < lf::VEFFZ_NPIECE * (lf::VEFFZ_DEG + 1); ++j)
        if (!std::isfinite(t.zc[j])) return false;
    for (int64_t k = 0; k < t.nrec; ++k) {
        const double* r = t.rec + (size_t)k * lf::VEFFZ_REC;
        for (int j = 0; j < 7; ++j)
            if (!std::isfinite(r[j])) return false;
        if (!(r[1] > r[0]) || !(r[4] >= r[3])) return false;
        if (k + 1 < t.nrec && (r[1] != r[lf::VEFFZ_REC] || r[4] != r[lf::VEFFZ_REC + 3])) return false;
    }
    const double* last = t.rec + (size_t)(t.nrec - 1) * lf::VEFFZ_REC;
    return t.rec[0] == d_lo && t.rec[3] == 0.0 && last[1] == d_hi && last[4] == v_total;
}

// lf_veff_draws (zt == NULL: second = vol or NULL for vol_all) and lf_veff_draws_zmax (second = dist): the argument checks,
// the sort by bin, the chunks and stages 2 and 3 are shared; stage 1 is veffd_partial or veffd_partial_zmax
static int veffd_run(int device, int64_t n, const double* flux, const int32_t* field, const double* second, double vol_all, double pref0,
                     double fcmin, const int32_t* bin_of, int32_t nbin, int32_t nf, int32_t R, const double* draws, const VeffzTable* zt,
                     int32_t nq, const double* q, int32_t method, double* out, double* values) {
#pragma clang fp contract(off)
    // every argument is checked before the device is touched
    if (!flux || !field || !bin_of || !draws || !out || n <= 0 || n > (int64_t)INT32_MAX || nbin < 1 || nbin > lf::VEFF_MAXBIN || nf < 1 ||
        nf > lf::VEFFD_MAXF || R < 1 || R > lf::BANDS_SLOTS || !(pref0 > 0.0))
        return LF_ERR_ARG;
    const lfh::Quantiles qt = lfh::quantiles(R, nq, q, method, lf::BANDS_MAXQ);
    if (!qt.ok) return LF_ERR_ARG;
    const std::vector<double>& qtab = qt.tab;
    const int lg = qt.lg;
    for (int64_t i = 0; i < n; ++i)
        if (field[i] < 0 || field[i] >= nf) return LF_ERR_ARG;
    for (int r = 0; r < R; ++r) {
        const double* d = draws + (size_t)r * (nf + 1);
        for (int f = 0; f < nf; ++f)
            if (!std::isfinite(d[f]) || d[f] <= 0.0) return LF_ERR_ARG;
        if (!std::isfinite(d[nf]) || d[nf] == 0.0) return LF_ERR_ARG;
    }
    std::vector<double> cfac;                                // fmin^(-1/2) per draw and field; +inf for no cut
    if (zt) {
        if (!second || !zt->fmin || !veffz_table_ok(*zt)) return LF_ERR_ARG;
        for (int64_t i = 0; i < n; ++i)
            if (!std::isfinite(second[i]) || second[i] < 0.0) return LF_ERR_ARG;
        cfac.resize((size_t)R * nf);
        for (size_t j = 0; j < cfac.size(); ++j) {
            if (!std::isfinite(zt->fmin[j]) || zt->fmin[j] < 0.0) return LF_ERR_ARG;
            cfac[j] = 1.0 / std::sqrt(zt->fmin[j]);
        }
    }
    // stable counting sort of the sources by bin; the sources outside [0, nbin) are dropped
    std::vector<int64_t> first((size_t)nbin + 1, 0);
    for (int64_t i = 0; i < n; ++i)
        if (bin_of[i] >= 0 && bin_of[i] < nbin) ++first[(size_t)bin_of[i] + 1];
    for (int b = 0; b < nbin; ++b) first[b + 1] += first[b];
    const int64_t m = first[nbin];
    std::vector<double> sflux((size_t)m), sipv((size_t)m);   // sipv: 1 / (pref0 vol), or the source's s_i under zt
    std::vector<int> sfield((size_t)m);
    {
        std::vector<int64_t> at(first.begin(), first.end() - 1);
        for (int64_t i = 0; i < n; ++i) {
            if (bin_of[i] < 0 || bin_of[i] >= nbin) continue;
            const int64_t k = at[bin_of[i]]++;
            sflux[k] = flux[i];
            if (zt) {
                sipv[k] = second[i];
            } else {
                const double v = second ? second[i] : vol_all;
                sipv[k] = v > 0.0 ? 1.0 / (pref0 * v) : 0.0;
            }
            sfield[k] = field[i];
        }
    }
    // chunks of at most VEFFD_CHUNK sources within a bin's segment; bin_c0[b] = the first chunk of bin b
    std::vector<long long> cstart;
    std::vector<int> clen, bin_c0((size_t)nbin + 1, 0);
    for (int b = 0; b < nbin; ++b) {
        bin_c0[b] = (int)cstart.size();
        for (int64_t s = first[b]; s < first[b + 1]; s += lf::VEFFD_CHUNK) {
            cstart.push_back((long long)s);
            clen.push_back((int)std::min<int64_t>(lf::VEFFD_CHUNK, first[b + 1] - s));
        }
    }
    const size_t nch = cstart.size();
    bin_c0[nbin] = (int)nch;
    const double ratio = fcmin > 0.0 ? lfh::fc_ratio(fcmin) : 0.0;
    if (hipSetDevice(device) != hipSuccess) return LF_ERR_NODEV;
    Buf<double> d_flux, d_ipv, d_draws, d_part, d_val, d_q, d_out, d_cfac, d_zc, d_rec;
    Buf<int> d_field, d_clen, d_c0;
    Buf<long long> d_cstart;
    HostCall hc;
    for (double& t : g_veffd_ms) t = -1.0;
    if (zt && !(hc.ok(d_cfac.upload(cfac.data(), cfac.size())) && hc.ok(d_zc.upload(zt->zc, (size_t)lf::VEFFZ_NPIECE * (lf::VEFFZ_DEG + 1))) &&
                hc.ok(d_rec.upload(zt->rec, (size_t)zt->nrec * lf::VEFFZ_REC))))
        return hc.rc;
    if (hc.ok(d_flux.upload(sflux.data(), (size_t)m)) && hc.ok(d_ipv.upload(sipv.data(), (size_t)m)) && hc.ok(d_field.upload(sfield.data(), (size_t)m)) &&
        hc.ok(d_cstart.upload(cstart.data(), nch)) && hc.ok(d_clen.upload(clen.data(), nch)) && hc.ok(d_c0.upload(bin_c0.data(), bin_c0.size())) &&
        hc.ok(d_draws.upload(draws, (size_t)R * (nf + 1))) && hc.ok(d_q.upload(qtab.data(), qtab.size())) &&
        hc.ok(alloc_all(d_part, nch * (size_t)R, d_val, (size_t)R * nbin, d_out, (size_t)nq * nbin))) {
        const unsigned tiles = (unsigned)((R + lf::VEFFD_THREADS - 1) / lf::VEFFD_THREADS);
        hc.stamp(0, 0);
        if (nch > 0 && zt) {
            const lf::VeffzHead head = {zt->head[0], zt->head[1], zt->head[3], zt->head[4], zt->head[5], 1.0 / (pref0 * zt->head[2]),
                                        (int)zt->nrec};
            auto kernel = nf <= lf::VEFFZ_FEW ? (fcmin > 0.0 ? lf::veffd_partial_zmax<true, lf::VEFFZ_FEW> : lf::veffd_partial_zmax<false, lf::VEFFZ_FEW>)
                                              : (fcmin > 0.0 ? lf::veffd_partial_zmax<true, lf::VEFFD_MAXF> : lf::veffd_partial_zmax<false, lf::VEFFD_MAXF>);
            hipLaunchKernelGGL(kernel, dim3((unsigned)nch, tiles), dim3(lf::VEFFD_THREADS), 0, 0, d_flux, d_ipv, d_field, d_cstart, d_clen,
                               d_draws, d_cfac, (int)nf, (int)R, ratio, pref0, head, d_zc, d_rec, d_part);
            hc.ok(hipGetLastError());
        } else if (nch > 0) {
            auto kernel = fcmin > 0.0 ? lf::veffd_partial<true> : lf::veffd_partial<false>;
            hipLaunchKernelGGL(kernel, dim3((unsigned)nch, tiles), dim3(lf::VEFFD_THREADS), 0, 0, d_flux, d_ipv, d_field, d_cstart, d_clen,
                               d_draws, (int)nf, (int)R, ratio, d_part);
            hc.ok(hipGetLastError());
        }
        hc.stamp(1, 0);
        hipLaunchKernelGGL(lf::veffd_reduce, dim3(tiles, (unsigned)nbin), dim3(lf::VEFFD_THREADS), 0, 0, d_part, d_c0, (int)nbin, (int)R, d_val);
        hc.ok(hipGetLastError());
        hc.stamp(2, 0);
        const int G = lf::BANDS_SLOTS >> lg;
        hipLaunchKernelGGL(lf::veffd_quant, dim3((unsigned)((nbin + G - 1) / G)), dim3(lf::BANDS_THREADS), 0, 0, d_val, (int)R, lg, (int)nbin,
                           d_q, (int)nq, method == LF_Q_MEDIAN ? 1 : 0, d_out);
        hc.ok(hipGetLastError());
        hc.stamp(3, 0);
        hc.ok(hipMemcpy(out, d_out, (size_t)nq * nbin * sizeof(double), hipMemcpyDeviceToHost));
        if (values) hc.ok(hipMemcpy(values, d_val, (size_t)R * nbin * sizeof(double), hipMemcpyDeviceToHost));
        for (int s = 0; s < 3; ++s) hc.elapsed(s, s + 1, &g_veffd_ms[s]);
        if (hc.rc != LF_OK)
            for (double& t : g_veffd_ms) t = -1.0;
    }
    return hc.rc;
}

int lf_veff_draws(int device, int64_t n, const double* flux, const int32_t* field, const double* vol, double vol_all, double pref0,
                  double fcmin, const int32_t* bin_of, int32_t nbin, int32_t nf, int32_t R, const double* draws, int32_t nq,
                  const double* q, int32_t method, double* out, double* values) {
    return veffd_run(device, n, flux, field, vol, vol_all, pref0, fcmin, bin_of, nbin, nf, R, draws, nullptr, nq, q, method, out, values);
}

int lf_veff_draws_zmax(int device, int64_t n, const double* flux, const int32_t* field, const double* dist, double pref0, double fcmin,
                       const int32_t* bin_of, int32_t nbin, int32_t nf, int32_t R, const double* draws, const double* fmin,
                       const double* vt_head, const double* vt_zc, const double* vt_rec, int64_t vt_nrec, int32_t nq, const double* q,
                       int32_t method, double* out, double* values) {
    if (!dist || !fmin) return LF_ERR_ARG;
    const VeffzTable zt = {fmin, vt_head, vt_zc, vt_rec, vt_nrec};
    return veffd_run(device, n, flux, field, dist, 0.0, pref0, fcmin, bin_of, nbin, nf, R, draws, &zt, nq, q, method, out, values);
}

int lf_veff_draws_ms(double* ms) {
    if (!ms) return LF_ERR_ARG;
    for (int s = 0; s < 3; ++s) ms[s] = g_veffd_ms[s];
    return g_veffd_ms[0] < 0.0 ? LF_ERR_ARG : LF_OK;
}

int lf_veff_draws_chunk(void) { return lf::VEFFD_CHUNK; }

int lf_last_launch(const lf_ctx* c, int32_t info[8]) {
    if (!c || !info) return LF_ERR_ARG;
    for (int i = 0; i < 8; ++i) info[i] = c->last_launch[i];
    return LF_OK;
}

int lf_free_block_uploads(const lf_ctx* c, int64_t* n) {
    if (!c || !n) return LF_ERR_ARG;
    *n = c->fblk_uploads;
    return LF_OK;
}

int lf_form_counts(lf_ctx* c, int64_t counts[9]) {
    if (!c || !counts) return LF_ERR_ARG;
    for (int i = 0; i < lf::FORM_COUNT; ++i) counts[i] = 0;
    if (!c->d_forms) return LF_OK;
    LF_HIP(c, hipSetDevice(c->device));
    LF_HIP(c, hipDeviceSynchronize());
    unsigned long long h[lf::FORM_COUNT];
    LF_HIP(c, hipMemcpy(h, c->d_forms, sizeof(h), hipMemcpyDeviceToHost));
    for (int i = 0; i < lf::FORM_COUNT; ++i) counts[i] = (int64_t)h[i];
    return LF_OK;
}

int lf_set_option(lf_ctx* c, const char* key, int64_t value) {
    if (!c || !key) return LF_ERR_ARG;
    // the options that are one number of the context: a flag (value != 0), or a clamped value
    using Set = void (*)(lf_ctx*, int64_t);
    static const struct {
        const char* key;
        Set set;
    } plain[] = {
        {"taper", [](lf_ctx* c, int64_t v) { c->opt_taper = v != 0; }},
        {"fuse", [](lf_ctx* c, int64_t v) { c->opt_fuse = v != 0; }},
        {"fuse_step", [](lf_ctx* c, int64_t v) { c->opt_fuse_step = v != 0; }},
        {"poll", [](lf_ctx* c, int64_t v) { c->opt_poll = v != 0; }},
        {"cells", [](lf_ctx* c, int64_t v) { c->opt_cells = v != 0; c->kc.cells = c->opt_cells && c->ncell > 0; }},
        {"tables", [](lf_ctx* c, int64_t v) { c->kc.tables = v != 0; }},
        {"specialise", [](lf_ctx* c, int64_t v) { c->kc.specialise = v != 0; }},
        {"grid_shortcut", [](lf_ctx* c, int64_t v) { c->opt_grid_shortcut = v != 0; }},
        {"compress_grid", [](lf_ctx* c, int64_t v) { c->opt_compress_grid = v != 0; }},
        {"skip_grid", [](lf_ctx* c, int64_t v) { c->opt_skip_grid = v != 0; }},
        {"deconv_unchecked", [](lf_ctx* c, int64_t v) { c->opt_deconv_unchecked = v != 0; }},
        {"deconv_tile", [](lf_ctx* c, int64_t v) { c->opt_deconv_tile = v != 0; }},
        {"deconv_wide", [](lf_ctx* c, int64_t v) { c->opt_deconv_wide = v != 0; }},
        {"deconv_cut_limit", [](lf_ctx* c, int64_t v) { c->opt_cut_limit = v < 0 ? 0 : v; }},
        {"deconv_cut_grad", [](lf_ctx* c, int64_t v) { c->opt_cut_grad = v != 0; }},
        {"deconv_cut_veff", [](lf_ctx* c, int64_t v) { c->opt_cut_veff = v != 0; }},
        {"persistent", [](lf_ctx* c, int64_t v) { c->opt_persistent = v < 0 ? 0 : (v > 2 ? 2 : v); }},
        {"profile_every", [](lf_ctx* c, int64_t v) { c->opt_profile_every = v < 1 ? 1 : v; c->prof_tick = 0; }},
        {"profile_span", [](lf_ctx* c, int64_t v) { c->opt_profile_span = v < 1 ? 1 : v; c->prof_tick = 0; }},
    };
    for (const auto& o : plain)
        if (std::strcmp(key, o.key) == 0) {
            o.set(c, value);
            return LF_OK;
        }
    if (std::strcmp(key, "geometry") == 0) {
        if (value < -1 || value >= NGEO) {
            c->err = "geometry must be -1 (auto) or an index below " + std::to_string(NGEO);
            return LF_ERR_ARG;
        }
        c->opt_geometry = value;
        return LF_OK;
    }
    if (std::strcmp(key, "compress") == 0) {
        if (value != 0) {
            hipSetDevice(c->device);
            const bool fresh = !c->cmp.built;
            int rc = build_compressed(c);
            if (rc != LF_OK) return rc;
            // The bins were accepted on a SAMPLED estimate of the interpolation error (lf_compress.h).  Before a freshly
            // built compressed catalogue may serve, it must also reproduce the direct path on walkers drawn from THIS
            // context's prior box: 64 theta rows (deterministic stream), both paths, lnprob to 1e-12 and the same -inf
            // pattern - otherwise the option is refused and the compressed tables are dropped.
            if (fresh && c->cmp.built && (rc = compress_selfcheck(c)) != LF_OK) {
                c->cmp = CompressedCat{};
                c->gridc = CompressedGrid{};
                return rc;
            }
        }
        c->opt_compress = value != 0;
        return LF_OK;
    }
    if (std::strcmp(key, "count_forms") == 0) {
        hipSetDevice(c->device);
        if (value != 0 && !c->d_forms) LF_HIP(c, c->d_forms.alloc(lf::FORM_COUNT));
        if (c->d_forms) {
            LF_HIP(c, hipDeviceSynchronize());
            LF_HIP(c, hipMemset(c->d_forms, 0, lf::FORM_COUNT * sizeof(unsigned long long)));
        }
        c->kc.forms = value != 0 ? c->d_forms : nullptr;
        return LF_OK;
    }
    if (std::strcmp(key, "free_st") == 0) {
        if (value != 0 && value != 2 && value != 4 && value != 8) {
            c->err = "free_st must be 0 (auto), 2, 4 or 8";
            return LF_ERR_ARG;
        }
        c->opt_free_st = value;
        return LF_OK;
    }
    if (std::strcmp(key, "grid_share") == 0) {
        // value = part + parts * 65536: integrate only the node chunks c with c % parts == part (source-sharded ranks,
        // whose lnprob values are summed); one part, or a value below 65536 (no parts at all), = the whole grid.  Where there are
        // parts, a part that they do not have is refused, part 1 of one part included (it used to pass as the whole grid: a rank
        // set up so would add the whole of piece B to the sum a second time)
        const int64_t parts = value >> 16, part = value & 0xffff;
        if (value < 0 || (parts >= 1 && part >= parts)) {
            c->err = "grid_share must be part + 65536 * parts with part < parts";
            return LF_ERR_ARG;
        }
        c->kc.grid_parts = parts > 1 ? (int)parts : 1;
        c->kc.grid_part = parts > 1 ? (int)part : 0;
        return LF_OK;
    }
    if (std::strcmp(key, "walker_tile") == 0) {
        if (value < 0 || value > 64) {
            c->err = "walker_tile must be 0 (auto) .. 64";
            return LF_ERR_ARG;
        }
        c->opt_walker_tile = value;
        return LF_OK;
    }
    c->err = std::string("unknown option ") + key;
    return LF_ERR_ARG;
}

int64_t lf_compress_keys(int kind, const double* params, const double* key, const double* wt, int64_t n,
                         double* node, double* weight, int64_t cap, double* bound) {
    if (!params || (!key && n > 0) || n < 0 || (kind != 0 && kind != 1)) return LF_ERR_ARG;
    lfc::Model m{};
    m.kind = kind;
    if (kind == 0) {
        m.fc_ratio = params[0];
        m.alpha_lo = params[1];
        m.alpha_hi = params[2];
        m.flim_lo = params[3];
        m.flim_hi = params[4];
    } else {
        m.L_lo = params[0];
        m.L_hi = params[1];
        for (int i = 0; i < 3; ++i) m.piv[i] = params[2 + i];
    }
    lfc::Out out;
    if (!lfc::compress_field(m, key, wt, n, out)) return LF_ERR_ARG;
    if (bound) *bound = out.bound;
    const int64_t cnt = (int64_t)out.node.size();
    if (cnt > cap || !node || !weight) return cnt;
    std::copy(out.node.begin(), out.node.end(), node);
    std::copy(out.weight.begin(), out.weight.end(), weight);
    return cnt;
}

int64_t lf_compress_grid(const double* params, int S, const double* L, const double* wL, const double* ck, const double* Dk,
                         double* u, int32_t* row0, int32_t* nrows, int32_t* off, double* omega, int64_t cap_bins,
                         int64_t cap_omega, double* bound) {
    if (!params || !L || !wL || !ck || !Dk || S < 2) return LF_ERR_ARG;
    lfc::Model m{};
    m.kind = 2;
    m.fc_ratio = params[0];
    m.alpha_lo = params[1];
    m.alpha_hi = params[2];
    m.flim_lo = params[3];
    m.flim_hi = params[4];
    lfc::GridOut g;
    if (!lfc::compress_grid(m, S, L, wL, ck, Dk, g)) return LF_ERR_ARG;
    if (bound) *bound = g.bound;
    if (g.nb > cap_bins || (int64_t)g.omega.size() > cap_omega || !u || !row0 || !nrows || !off || !omega) return g.nb;
    std::copy(g.u.begin(), g.u.end(), u);
    std::copy(g.row0.begin(), g.row0.end(), row0);
    std::copy(g.nrows.begin(), g.nrows.end(), nrows);
    std::copy(g.off.begin(), g.off.end(), off);
    std::copy(g.omega.begin(), g.omega.end(), omega);
    return g.nb;
}

int64_t lf_grid_bins(const double* params, int S, const double* L, const double* wL, const double* ck, const double* Dk,
                     double* edges, double* rec, int32_t* rows, double* omega, int64_t cap_bins, int64_t cap_omega, double* margin) {
    if (!params || !L || !wL || !ck || !Dk || S < 2) return LF_ERR_ARG;
    if (!(params[1] > 0.0) || !(params[3] > 0.0)) return LF_ERR_ARG;
    const lfq::Box bx{std::sqrt(params[0]), params[1], params[2], std::log10(params[3]) + LF_FREF, std::log10(params[4]) + LF_FREF};
    lfq::GridQ g;
    if (!lfq::build_gridq(bx, S, L, wL, ck, Dk, LF_FREF, LF_LREF, g)) return LF_ERR_ARG;
    if (margin) *margin = g.margin;
    if (g.nb > cap_bins || (int64_t)g.omega.size() > cap_omega || !edges || !rec || !rows || !omega) return g.nb;
    std::copy(g.edges.begin(), g.edges.end(), edges);
    std::copy(g.rec.begin(), g.rec.end(), rec);
    std::copy(g.rows.begin(), g.rows.end(), rows);
    std::copy(g.omega.begin(), g.omega.end(), omega);
    return g.nb;
}

/* ---------------------------------------------------------------------------------------------
 * device-resident ensemble sampler
 * ------------------------------------------------------------------------------------------- */
struct lf_sampler {
    lf_ctx* ctx = nullptr;
    int W = 0, ndim = 0;
    double a = 2.0;
    uint64_t seed = 0, step = 0;
    int64_t cap = 0, t = 0;
    Buf<double> d_pos, d_lnp, d_prop, d_zz, d_newlp;
    Buf<double> d_chain, d_chain_lnp;
    Buf<long long> d_nacc;
    bool started = false;
    // lf_sampler_set_likelihood: the flux-error-convolved likelihood, the plain lnprob of the rows it evaluates [W], whether
    // the start's lnprob was the sampler's own evaluation, whether a step has been taken since the start
    bool convolved = false, own_start = false, moved = false;
    Buf<double> d_plain;
};

namespace {

// A sampler's evaluation of B rows on `s`: the plain lnprob (the three-piece form), or with convolved the plain lnprob into
// d_plain and the correction's kernels on it, per the context's "deconv_tile" (enqueue_deconv) - d_out either way.
int sampler_eval(lf_ctx* c, bool convolved, const double* d_theta, int B, double* d_plain, double* d_out, hipStream_t s) {
    if (!convolved) return enqueue(c, d_theta, B, d_out, nullptr, nullptr, s);
    return enqueue_deconv(c, d_theta, B, d_plain, d_out, s);
}

// What both samplers' set_likelihood entries check and prepare: family_check's refusals, the call's place (before a step),
// and with convolved everything the correction needs for `rows` rows (d_plain, the evaluation's workspace, deconv_prepare),
// now rather than by a resize inside a running chain.
int sampler_likelihood(lf_ctx* c, const char* fn, int convolved, bool moved, int rows, Buf<double>& d_plain) {
    if (moved) {
        c->err = std::string(fn) + ": the chain has taken a step (valid before the start, or between a start and the first step)";
        return LF_ERR_ARG;
    }
    if (!convolved) return LF_OK;
    int rc = family_check(c, fn, true, c, 1, c);
    if (rc != LF_OK) return rc;
    LF_HIP(c, hipSetDevice(c->device));
    if (d_plain.size() < (size_t)rows) LF_HIP(c, d_plain.alloc((size_t)rows));
    if ((rc = ensure_workspace(c, rows, 0, 0)) != LF_OK) return rc;
    return deconv_prepare(c, rows, false);
}

// A sampler's chains on the device are [rows][cap][width], the caller's [rows][t][width] (t steps taken): packed on the device
// first, then ONE copy to the host (a strided copy into pageable host memory goes row by row).  parts[0] is the widest.
struct ChainPart {
    double* dst;            // host (NULL: not asked for)
    const double* src;
    size_t rows, width;
};
int read_chains(lf_ctx* c, const char* fn, const ChainPart* parts, int nparts, size_t cap, size_t t) {
    bool any = false;
    for (int i = 0; i < nparts; ++i) any = any || parts[i].dst;
    if (t == 0 || !any) return LF_OK;
    Buf<double> tmp;
    LF_HIP(c, tmp.alloc(parts[0].rows * t * parts[0].width));
    for (int i = 0; i < nparts; ++i) {
        const ChainPart& p = parts[i];
        if (!p.dst) continue;
        if (hipMemcpy2D(tmp, t * p.width * 8, p.src, cap * p.width * 8, t * p.width * 8, p.rows, hipMemcpyDeviceToDevice) != hipSuccess ||
            hipMemcpy(p.dst, tmp, p.rows * t * p.width * 8, hipMemcpyDeviceToHost) != hipSuccess) {
            c->err = std::string(fn) + ": copy failed";
            return LF_ERR_HIP;
        }
    }
    return LF_OK;
}

}  // namespace

lf_sampler* lf_sampler_create(lf_ctx* c, int nwalkers, double a, uint64_t seed, int64_t capacity_steps) {
    if (!c) return nullptr;
    if (nwalkers < 2 || (nwalkers & 1) || capacity_steps < 1 || !(a > 1.0)) {
        c->err = "lf_sampler_create: nwalkers must be even and >= 2, a > 1, capacity_steps >= 1";
        return nullptr;
    }
    if (hipSetDevice(c->device) != hipSuccess) return nullptr;
    lf_sampler* sm = new (std::nothrow) lf_sampler();
    if (!sm) return nullptr;
    sm->ctx = c;
    sm->W = nwalkers;
    sm->ndim = c->kc.ndim;
    sm->a = a;
    sm->seed = seed;
    sm->cap = capacity_steps;
    const size_t W = (size_t)nwalkers, nd = (size_t)sm->ndim, cap = (size_t)capacity_steps;
    if (alloc_all(sm->d_pos, W * nd, sm->d_lnp, W, sm->d_prop, W * nd, sm->d_zz, W, sm->d_newlp, W, sm->d_chain, W * cap * nd,
                  sm->d_chain_lnp, W * cap, sm->d_nacc, W) != hipSuccess) {
        c->err = "lf_sampler_create: device allocation failed";
        lf_sampler_destroy(sm);
        return nullptr;
    }
    return sm;
}

void lf_sampler_destroy(lf_sampler* sm) {
    if (!sm) return;
    if (sm->ctx) {
        hipSetDevice(sm->ctx->device);
        hipDeviceSynchronize();
    }
    delete sm;
}

int lf_sampler_start(lf_sampler* sm, const double* pos, const double* lnprob0) {
    if (!sm || !pos) return LF_ERR_ARG;
    lf_ctx* c = sm->ctx;
    LF_HIP(c, hipSetDevice(c->device));
    const size_t W = (size_t)sm->W, nd = (size_t)sm->ndim;
    LF_HIP(c, hipMemcpy(sm->d_pos, pos, W * nd * 8, hipMemcpyHostToDevice));
    LF_HIP(c, hipMemset(sm->d_nacc, 0, W * sizeof(long long)));
    if (lnprob0) {
        LF_HIP(c, hipMemcpy(sm->d_lnp, lnprob0, W * 8, hipMemcpyHostToDevice));
    } else {
        int rc = sampler_eval(c, sm->convolved, sm->d_pos, sm->W, sm->d_plain, sm->d_lnp, c->stream);
        if (rc != LF_OK) return rc;
        LF_HIP(c, hipStreamSynchronize(c->stream));
    }
    sm->own_start = !lnprob0;
    sm->moved = false;
    sm->step = 0;
    sm->t = 0;
    sm->started = true;
    return LF_OK;
}

int lf_sampler_set_likelihood(lf_sampler* sm, int convolved) {
    if (!sm) return LF_ERR_ARG;
    lf_ctx* c = sm->ctx;
    int rc = sampler_likelihood(c, "lf_sampler_set_likelihood", convolved, sm->moved, sm->W, sm->d_plain);
    if (rc != LF_OK) return rc;
    const bool changed = sm->convolved != (convolved != 0);
    sm->convolved = convolved != 0;
    if (changed && sm->started && sm->own_start) {
        // the start's lnprob was this sampler's evaluation, of the other likelihood: once more
        if ((rc = sampler_eval(c, sm->convolved, sm->d_pos, sm->W, sm->d_plain, sm->d_lnp, c->stream)) != LF_OK) return rc;
        LF_HIP(c, hipStreamSynchronize(c->stream));
    }
    return LF_OK;
}

int lf_sampler_run(lf_sampler* sm, int64_t nsteps, void* hip_stream) {
    if (!sm || nsteps < 0) return LF_ERR_ARG;
    lf_ctx* c = sm->ctx;
    if (!sm->started) {
        c->err = "lf_sampler_run: call lf_sampler_start first";
        return LF_ERR_ARG;
    }
    if (sm->t + nsteps > sm->cap) {
        c->err = "lf_sampler_run: chain capacity exceeded";
        return LF_ERR_ARG;
    }
    LF_HIP(c, hipSetDevice(c->device));
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : c->stream;
    const int halfW = sm->W / 2;
    if (nsteps > 0) sm->moved = true;
    for (int64_t it = 0; it < nsteps; ++it) {
        for (int half = 0; half < 2; ++half) {
            lf::StepArgs sp{1, half, halfW, sm->ndim, sm->step, sm->seed, sm->a, sm->d_pos, sm->d_prop, sm->d_zz};
            lf::AcceptArgs ap{1, half, halfW, sm->ndim, sm->step, sm->seed, (long long)sm->t, (long long)sm->cap,
                              sm->d_pos, sm->d_lnp, sm->d_prop, sm->d_zz, sm->d_nacc, sm->d_chain, sm->d_chain_lnp};
            int rc;
            if (sm->convolved) {
                // propose, the plain evaluation, the correction's kernels, accept: the option "fuse_step" does not apply
                hipLaunchKernelGGL(lf::lf_propose, dim3((halfW + 7) / 8), dim3(64), 0, s, sp);
                LF_HIP(c, hipGetLastError());
                if ((rc = sampler_eval(c, true, sm->d_prop, halfW, sm->d_plain, sm->d_newlp, s)) != LF_OK) return rc;
                hipLaunchKernelGGL(lf::lf_accept, dim3(halfW), dim3(64), 0, s, ap, (const double*)sm->d_newlp);
                LF_HIP(c, hipGetLastError());
                continue;
            }
            rc = enqueue(c, nullptr, halfW, sm->d_newlp, nullptr, nullptr, s, &sp, &ap);
            if (rc != LF_OK) return rc;
        }
        sm->step += 1;
        sm->t += 1;
    }
    return LF_OK;
}

int lf_sampler_read(lf_sampler* sm, double* chain, double* chain_lnprob, int64_t* naccepted, double* pos, double* lnprob) {
    if (!sm) return LF_ERR_ARG;
    lf_ctx* c = sm->ctx;
    LF_HIP(c, hipSetDevice(c->device));
    LF_HIP(c, hipDeviceSynchronize());
    const size_t W = (size_t)sm->W, nd = (size_t)sm->ndim;
    const ChainPart parts[2] = {{chain, sm->d_chain, W, nd}, {chain_lnprob, sm->d_chain_lnp, W, 1}};
    const int rc = read_chains(c, "lf_sampler_read", parts, 2, (size_t)sm->cap, (size_t)sm->t);
    if (rc != LF_OK) return rc;
    if (naccepted) LF_HIP(c, hipMemcpy(naccepted, sm->d_nacc, W * sizeof(long long), hipMemcpyDeviceToHost));
    if (pos) LF_HIP(c, hipMemcpy(pos, sm->d_pos, W * nd * 8, hipMemcpyDeviceToHost));
    if (lnprob) LF_HIP(c, hipMemcpy(lnprob, sm->d_lnp, W * 8, hipMemcpyDeviceToHost));
    return LF_OK;
}

int64_t lf_sampler_steps(const lf_sampler* sm) { return sm ? sm->t : LF_ERR_ARG; }

int lf_sampler_half_eval(lf_sampler* sm, int half, int lo, int hi, double* d_newlp, void* hip_stream) {
    if (!sm || !d_newlp || half < 0 || half > 1 || lo < 0 || hi < lo || hi > sm->W / 2) return LF_ERR_ARG;
    lf_ctx* c = sm->ctx;
    if (!sm->started || sm->t >= sm->cap) {
        c->err = "lf_sampler_half_eval: not started, or chain capacity exceeded";
        return LF_ERR_ARG;
    }
    LF_HIP(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)hip_stream;          // as given: NULL is the default stream (cf. lf_lnprob_batch_device)
    const int halfW = sm->W / 2;
    lf::StepArgs sp{1, half, halfW, sm->ndim, sm->step, sm->seed, sm->a, sm->d_pos, sm->d_prop, sm->d_zz};
    hipLaunchKernelGGL(lf::lf_propose, dim3((halfW + 7) / 8), dim3(64), 0, s, sp);
    LF_HIP(c, hipGetLastError());
    if (hi > lo)
        return sampler_eval(c, sm->convolved, sm->d_prop + (size_t)lo * sm->ndim, hi - lo, sm->d_plain + lo, d_newlp + lo, s);
    return LF_OK;
}

int lf_sampler_half_accept(lf_sampler* sm, int half, const double* d_newlp, void* hip_stream) {
    if (!sm || !d_newlp || half < 0 || half > 1) return LF_ERR_ARG;
    lf_ctx* c = sm->ctx;
    if (!sm->started || sm->t >= sm->cap) {
        c->err = "lf_sampler_half_accept: not started, or chain capacity exceeded";
        return LF_ERR_ARG;
    }
    LF_HIP(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)hip_stream;          // as given: NULL is the default stream (cf. lf_lnprob_batch_device)
    const int halfW = sm->W / 2;
    lf::AcceptArgs ap{1, half, halfW, sm->ndim, sm->step, sm->seed, (long long)sm->t, (long long)sm->cap,
                      sm->d_pos, sm->d_lnp, sm->d_prop, sm->d_zz, sm->d_nacc, sm->d_chain, sm->d_chain_lnp};
    hipLaunchKernelGGL(lf::lf_accept, dim3(halfW), dim3(64), 0, s, ap, d_newlp);
    LF_HIP(c, hipGetLastError());
    sm->moved = true;
    if (half == 1) {
        sm->step += 1;
        sm->t += 1;
    }
    return LF_OK;
}

/* ---------------------------------------------------------------------------------------------
 * parallel-tempered sampler (lf_pt.h)
 * ------------------------------------------------------------------------------------------- */
struct lf_ptsampler {
    lf_ctx* ctx = nullptr;
    int T = 0, W = 0, ndim = 0;
    double a = 2.0;
    uint64_t seed = 0, step = 0;
    int64_t cap = 0, t = 0;
    Buf<double> d_betas, d_dbeta;
    Buf<double> d_pos, d_lnl, d_prop, d_zz, d_newl;
    Buf<double> d_chain, d_chain_lnl, d_mean;
    Buf<long long> d_nacc, d_nswap;
    Buf<int> d_sig;
    bool started = false;
    // lf_ptsampler_set_likelihood: as lf_sampler's (d_plain: [T x W])
    bool convolved = false, own_start = false, moved = false;
    Buf<double> d_plain;
};

lf_ptsampler* lf_ptsampler_create(lf_ctx* c, int ntemps, int nwalkers, const double* betas, double a, uint64_t seed,
                                  int64_t capacity_steps) {
    if (!c) return nullptr;
    bool ok = ntemps >= 1 && ntemps <= lf::PT_MAXT && nwalkers >= 2 && !(nwalkers & 1) && nwalkers <= lf::PT_MAXW &&
              capacity_steps >= 1 && a > 1.0 && betas && betas[0] == 1.0;
    for (int i = 1; ok && i < ntemps; ++i) ok = betas[i] > 0.0 && betas[i] < betas[i - 1];
    if (!ok) {
        c->err = "lf_ptsampler_create: need 1 <= ntemps <= 64, even 2 <= nwalkers <= 4096, a > 1, capacity_steps >= 1, "
                 "betas[0] == 1 > betas[1] > ... > 0";
        return nullptr;
    }
    if (hipSetDevice(c->device) != hipSuccess) return nullptr;
    lf_ptsampler* sm = new (std::nothrow) lf_ptsampler();
    if (!sm) return nullptr;
    sm->ctx = c;
    sm->T = ntemps;
    sm->W = nwalkers;
    sm->ndim = c->kc.ndim;
    sm->a = a;
    sm->seed = seed;
    sm->cap = capacity_steps;
    const size_t T = (size_t)ntemps, TW = T * nwalkers, nd = (size_t)sm->ndim, cap = (size_t)capacity_steps, TH = TW / 2;
    std::vector<double> dbeta(T, 0.0);
    for (size_t i = 1; i < T; ++i) dbeta[i] = betas[i - 1] - betas[i];
    ok = sm->d_betas.upload(betas, T) == hipSuccess && sm->d_dbeta.upload(dbeta.data(), T) == hipSuccess &&
         alloc_all(sm->d_pos, TW * nd, sm->d_lnl, TW, sm->d_prop, TH * nd, sm->d_zz, TH, sm->d_newl, TH, sm->d_chain, TW * cap * nd,
                   sm->d_chain_lnl, TW * cap, sm->d_mean, T * cap, sm->d_nacc, TW, sm->d_nswap, T, sm->d_sig,
                   std::max<size_t>(T - 1, 1) * nwalkers) == hipSuccess;
    // the evaluation's workspace for the T x W / 2 rows of a half-step, now rather than by a resize inside a running chain
    ok = ok && ensure_workspace(c, (int)TH, 0, 0) == LF_OK;
    if (!ok) {
        c->err = "lf_ptsampler_create: device allocation failed";
        lf_ptsampler_destroy(sm);
        return nullptr;
    }
    return sm;
}

void lf_ptsampler_destroy(lf_ptsampler* sm) {
    if (!sm) return;
    if (sm->ctx) {
        hipSetDevice(sm->ctx->device);
        hipDeviceSynchronize();
    }
    delete sm;
}

int lf_ptsampler_start(lf_ptsampler* sm, const double* pos, const double* lnlike0) {
    if (!sm || !pos) return LF_ERR_ARG;
    lf_ctx* c = sm->ctx;
    LF_HIP(c, hipSetDevice(c->device));
    const size_t TW = (size_t)sm->T * sm->W, nd = (size_t)sm->ndim;
    std::vector<double> l(TW);
    if (lnlike0) {
        std::copy(lnlike0, lnlike0 + TW, l.begin());
    } else {
        LF_HIP(c, hipMemcpy(sm->d_pos, pos, TW * nd * 8, hipMemcpyHostToDevice));
        int rc = sampler_eval(c, sm->convolved, sm->d_pos, (int)TW, sm->d_plain, sm->d_lnl, c->stream);
        if (rc != LF_OK) return rc;
        LF_HIP(c, hipStreamSynchronize(c->stream));
        LF_HIP(c, hipMemcpy(l.data(), sm->d_lnl, TW * 8, hipMemcpyDeviceToHost));
    }
    for (size_t i = 0; i < TW; ++i) {
        if (!std::isfinite(l[i])) {
            c->err = "lf_ptsampler_start: every start position needs a finite lnprob";
            return LF_ERR_ARG;
        }
    }
    LF_HIP(c, hipMemcpy(sm->d_pos, pos, TW * nd * 8, hipMemcpyHostToDevice));
    LF_HIP(c, hipMemcpy(sm->d_lnl, l.data(), TW * 8, hipMemcpyHostToDevice));
    LF_HIP(c, hipMemset(sm->d_nacc, 0, TW * sizeof(long long)));
    LF_HIP(c, hipMemset(sm->d_nswap, 0, (size_t)sm->T * sizeof(long long)));
    sm->own_start = !lnlike0;
    sm->moved = false;
    sm->step = 0;
    sm->t = 0;
    sm->started = true;
    return LF_OK;
}

int lf_ptsampler_set_likelihood(lf_ptsampler* sm, int convolved) {
    if (!sm) return LF_ERR_ARG;
    lf_ctx* c = sm->ctx;
    const int TW = sm->T * sm->W;
    int rc = sampler_likelihood(c, "lf_ptsampler_set_likelihood", convolved, sm->moved, TW, sm->d_plain);
    if (rc != LF_OK) return rc;
    const bool changed = sm->convolved != (convolved != 0);
    sm->convolved = convolved != 0;
    if (changed && sm->started && sm->own_start) {
        // the start's lnlike was this sampler's evaluation, of the other likelihood: once more (it has to stay finite)
        std::vector<double> l((size_t)TW);
        if ((rc = sampler_eval(c, sm->convolved, sm->d_pos, TW, sm->d_plain, sm->d_lnl, c->stream)) != LF_OK) return rc;
        LF_HIP(c, hipStreamSynchronize(c->stream));
        LF_HIP(c, hipMemcpy(l.data(), sm->d_lnl, l.size() * 8, hipMemcpyDeviceToHost));
        for (double v : l) {
            if (!std::isfinite(v)) {
                sm->started = false;
                c->err = "lf_ptsampler_set_likelihood: every start position needs a finite lnprob (start again)";
                return LF_ERR_ARG;
            }
        }
    }
    return LF_OK;
}

int lf_ptsampler_run(lf_ptsampler* sm, int64_t nsteps, void* hip_stream) {
    if (!sm || nsteps < 0) return LF_ERR_ARG;
    lf_ctx* c = sm->ctx;
    if (!sm->started) {
        c->err = "lf_ptsampler_run: call lf_ptsampler_start first";
        return LF_ERR_ARG;
    }
    if (sm->t + nsteps > sm->cap) {
        c->err = "lf_ptsampler_run: chain capacity exceeded";
        return LF_ERR_ARG;
    }
    LF_HIP(c, hipSetDevice(c->device));
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : c->stream;
    const int halfW = sm->W / 2, rows = sm->T * halfW;
    const dim3 grid((rows * 8 + 63) / 64);
    if (nsteps > 0) sm->moved = true;
    for (int64_t it = 0; it < nsteps; ++it) {
        for (int half = 0; half < 2; ++half) {
            lf::PtArgs p{sm->T, sm->W, halfW, sm->ndim, half, sm->step, sm->seed, sm->a, sm->d_betas, sm->d_pos, sm->d_lnl,
                         sm->d_prop, sm->d_zz, sm->d_newl, sm->d_nacc};
            hipLaunchKernelGGL(lf::lf_pt_propose, grid, dim3(64), 0, s, p);
            LF_HIP(c, hipGetLastError());
            int rc = sampler_eval(c, sm->convolved, sm->d_prop, rows, sm->d_plain, sm->d_newl, s);
            if (rc != LF_OK) return rc;
            hipLaunchKernelGGL(lf::lf_pt_accept, grid, dim3(64), 0, s, p);
            LF_HIP(c, hipGetLastError());
        }
        lf::PtSwapArgs q{sm->T, sm->W, sm->ndim, sm->step, sm->seed, (long long)sm->t, (long long)sm->cap, sm->d_dbeta, sm->d_pos,
                         sm->d_lnl, sm->d_sig, sm->d_nswap, sm->d_chain, sm->d_chain_lnl, sm->d_mean};
        hipLaunchKernelGGL(lf::lf_pt_swap, dim3(1), dim3(lf::PT_SWAP_THREADS), 0, s, q);
        LF_HIP(c, hipGetLastError());
        sm->step += 1;
        sm->t += 1;
    }
    return LF_OK;
}

int lf_ptsampler_read(lf_ptsampler* sm, double* chain, double* chain_lnlike, double* mean_lnlike, int64_t* naccepted,
                      int64_t* nswap, double* pos, double* lnlike) {
    if (!sm) return LF_ERR_ARG;
    lf_ctx* c = sm->ctx;
    LF_HIP(c, hipSetDevice(c->device));
    LF_HIP(c, hipDeviceSynchronize());
    const size_t T = (size_t)sm->T, TW = T * sm->W, nd = (size_t)sm->ndim;
    const ChainPart parts[3] = {{chain, sm->d_chain, TW, nd}, {chain_lnlike, sm->d_chain_lnl, TW, 1}, {mean_lnlike, sm->d_mean, T, 1}};
    const int rc = read_chains(c, "lf_ptsampler_read", parts, 3, (size_t)sm->cap, (size_t)sm->t);
    if (rc != LF_OK) return rc;
    if (naccepted) LF_HIP(c, hipMemcpy(naccepted, sm->d_nacc, TW * sizeof(long long), hipMemcpyDeviceToHost));
    if (nswap && T > 1) LF_HIP(c, hipMemcpy(nswap, sm->d_nswap, (T - 1) * sizeof(long long), hipMemcpyDeviceToHost));
    if (pos) LF_HIP(c, hipMemcpy(pos, sm->d_pos, TW * nd * 8, hipMemcpyDeviceToHost));
    if (lnlike) LF_HIP(c, hipMemcpy(lnlike, sm->d_lnl, TW * 8, hipMemcpyDeviceToHost));
    return LF_OK;
}

int64_t lf_ptsampler_steps(const lf_ptsampler* sm) { return sm ? sm->t : LF_ERR_ARG; }

}  // extern "C"

/* ---------------------------------------------------------------------------------------------
 * chain diagnostics on the device (lf_diag.h)
 * ------------------------------------------------------------------------------------------- */
namespace {

double g_diag_ms = -1.0;        // device time of the kernels of the last diagnostics call (lf_diag_last)
int64_t g_diag_lags = 0;        // lags it computed per series

// The diagnostics of a chain in device memory, [W][cap][ndim] (+ lnprob [W][cap]) over steps [t0, t1): tau, window, ess, rhat of
// the D = ndim + (d_lnp != NULL) series; acf (host, [D][acf_cap]) when asked for.  Lags are computed in passes of whole tiles
// of 512 - 512 first, then up to twice as many as there are, until every series has its window (or n lags exist) - and a
// pass in slices whose partial sums stay below 64 MiB.  Launches go to `st`; synchronises it.  `err` takes the message.
int diag_run(std::string& err, hipStream_t st, const double* d_chain, const double* d_lnp, int W, int64_t cap, int ndim, int64_t t0,
             int64_t t1, double c, double* tau, int64_t* window, double* ess, double* rhat, double* acf, int64_t acf_cap) {
#pragma clang fp contract(off)
    const int D = ndim + (d_lnp ? 1 : 0);
    const int64_t n = t1 - t0;
    g_diag_ms = -1.0;
    g_diag_lags = 0;
    if (W > 65535 || D > 65535 || n > ((int64_t)1 << 30)) {
        err = "diagnostics: at most 65535 walkers and 2^30 steps";
        return LF_ERR_ARG;
    }
    HostCall hc(&err, "diagnostics: ");
    const size_t WD = (size_t)W * D;
    Buf<double> d_mean, d_mom, d_a0, d_a, d_acf;
    double ms_total = 0.0;
    auto timed = [&]() {            // closes a bracket of launches: waits for it and adds its device time
        double ms = 0.0;
        if (hc.stamp(1, st) && hc.wait(1) && hc.elapsed(0, 1, &ms)) ms_total += ms;
    };
    const lf::DiagSeries ser{d_chain, d_lnp, (long long)cap, ndim, D, (long long)t0, (int)n};
    std::vector<double> mom(4 * WD);
    if (hc.ok(alloc_all(d_mean, WD, d_mom, 4 * WD, d_a0, WD))) {
        hc.stamp(0, st);
        hipLaunchKernelGGL(lf::lf_diag_moments, dim3((unsigned)W, (unsigned)D), dim3(lf::DIAG_THREADS), 0, st, ser, d_mean.get(), d_mom.get());
        hc.ok(hipGetLastError());
        timed();
        hc.ok(hipMemcpy(mom.data(), d_mom, 4 * WD * sizeof(double), hipMemcpyDeviceToHost));
    }
    std::vector<std::vector<double>> curve(D);
    std::vector<char> decided(D, 0);
    if (hc.rc == LF_OK) {
        for (int d = 0; d < D; ++d) {
            rhat[d] = lfd::split_rhat(mom.data() + 4 * d, W, 4 * (size_t)D, n / 2);
            if (n < 4) decided[d] = (char)(lfd::chain_window(nullptr, 0, c, n, &tau[d], &window[d]) == 0);
        }
    }
    const int64_t Mmax = (n + lf::DIAG_LT - 1) / lf::DIAG_LT * lf::DIAG_LT;
    int64_t have = 0, want = lf::DIAG_LT;
    if (acf && acf_cap > want) want = std::min<int64_t>((acf_cap + lf::DIAG_LT - 1) / lf::DIAG_LT * lf::DIAG_LT, Mmax);
    const int64_t slice = std::max<int64_t>(((int64_t)64 << 20) / (int64_t)(WD * sizeof(double)) / lf::DIAG_LT, 1) * lf::DIAG_LT;
    const unsigned groups = (unsigned)((D + lf::DIAG_DG - 1) / lf::DIAG_DG);
    while (hc.rc == LF_OK && n >= 4) {
        for (int64_t lo = have; hc.rc == LF_OK && lo < want; lo += slice) {
            const int64_t Mp = std::min(slice, want - lo);
            std::vector<double> part((size_t)D * Mp);
            if (!hc.ok(alloc_all(d_a, WD * Mp, d_acf, (size_t)D * Mp))) break;
            hc.stamp(0, st);
            hipLaunchKernelGGL(lf::lf_diag_acf, dim3((unsigned)(Mp / lf::DIAG_LT), (unsigned)W, groups), dim3(lf::DIAG_THREADS), 0, st, ser,
                               d_mean.get(), (int)lo, d_a.get(), d_a0.get());
            hc.ok(hipGetLastError());
            hipLaunchKernelGGL(lf::lf_diag_norm, dim3((unsigned)(((int64_t)D * Mp + lf::DIAG_THREADS - 1) / lf::DIAG_THREADS)),
                               dim3(lf::DIAG_THREADS), 0, st, d_a.get(), d_a0.get(), W, D, (long long)Mp, d_acf.get());
            hc.ok(hipGetLastError());
            timed();
            hc.ok(hipMemcpy(part.data(), d_acf, part.size() * sizeof(double), hipMemcpyDeviceToHost));
            for (int d = 0; d < D && hc.rc == LF_OK; ++d) curve[d].insert(curve[d].end(), part.begin() + (size_t)d * Mp, part.begin() + (size_t)(d + 1) * Mp);
        }
        if (hc.rc != LF_OK) break;
        have = want;
        bool all = true;
        for (int d = 0; d < D; ++d) {
            if (!decided[d]) decided[d] = (char)(lfd::chain_window(curve[d].data(), have, c, n, &tau[d], &window[d]) == 0);
            all = all && decided[d];
        }
        if (all || have >= Mmax) break;
        want = std::min(2 * have, Mmax);
    }
    if (hc.rc != LF_OK) return hc.rc;
    for (int d = 0; d < D; ++d) {
        ess[d] = (double)W * (double)n / tau[d];
        if (acf)
            for (int64_t k = 0; k < acf_cap; ++k) acf[(size_t)d * acf_cap + k] = k < (int64_t)curve[d].size() ? curve[d][k] : 0.0;
    }
    g_diag_ms = ms_total;
    g_diag_lags = have;
    return LF_OK;
}

}  // namespace

extern "C" {

int lf_chain_window(const double* acf, int64_t M, double c, int64_t n, double* tau, int64_t* window) {
    if (!tau || !window || n < 1 || M < 0 || !(c > 0.0) || (n >= 4 && (!acf || M < 1))) return LF_ERR_ARG;
    return lfd::chain_window(acf, M, c, n, tau, window);
}

int lf_chain_diag(int device, const double* chain, const double* lnprob, int W, int64_t steps, int ndim, int64_t t0, int64_t t1, double c,
                  double* tau, int64_t* window, double* ess, double* rhat, double* acf, int64_t acf_cap) {
    if (!chain || !tau || !window || !ess || !rhat || W < 1 || ndim < 1 || t0 < 0 || t1 > steps || t1 <= t0 || !(c > 0.0) || acf_cap < 0 ||
        (acf && acf_cap < 1))
        return LF_ERR_ARG;
    if (hipSetDevice(device) != hipSuccess) return LF_ERR_NODEV;
    Buf<double> d_chain, d_lnp;
    const size_t rows = (size_t)W * (size_t)steps;
    if (d_chain.upload(chain, rows * ndim) != hipSuccess || (lnprob && d_lnp.upload(lnprob, rows) != hipSuccess)) return LF_ERR_HIP;
    std::string err;
    return diag_run(err, nullptr, d_chain, lnprob ? d_lnp.get() : nullptr, W, steps, ndim, t0, t1, c, tau, window, ess, rhat, acf, acf_cap);
}

int lf_sampler_diag(lf_sampler* sm, int64_t t0, double c, int with_lnprob, double* tau, int64_t* window, double* ess, double* rhat) {
    if (!sm || !tau || !window || !ess || !rhat || !sm->started || t0 < 0 || sm->t <= t0 || !(c > 0.0)) return LF_ERR_ARG;
    lf_ctx* cx = sm->ctx;
    LF_HIP(cx, hipSetDevice(cx->device));
    LF_HIP(cx, hipDeviceSynchronize());
    return diag_run(cx->err, cx->stream, sm->d_chain, with_lnprob ? sm->d_chain_lnp.get() : nullptr, sm->W, sm->cap, sm->ndim, t0, sm->t, c, tau,
                    window, ess, rhat, nullptr, 0);
}

int lf_ptsampler_diag(lf_ptsampler* sm, int temperature, int64_t t0, double c, int with_lnlike, double* tau, int64_t* window, double* ess,
                      double* rhat) {
    if (!sm || !tau || !window || !ess || !rhat || !sm->started || temperature < 0 || temperature >= sm->T || t0 < 0 || sm->t <= t0 ||
        !(c > 0.0))
        return LF_ERR_ARG;
    lf_ctx* cx = sm->ctx;
    LF_HIP(cx, hipSetDevice(cx->device));
    LF_HIP(cx, hipDeviceSynchronize());
    const size_t off = (size_t)temperature * sm->W * (size_t)sm->cap;
    return diag_run(cx->err, cx->stream, sm->d_chain + off * sm->ndim, with_lnlike ? sm->d_chain_lnl + off : nullptr, sm->W, sm->cap, sm->ndim,
                    t0, sm->t, c, tau, window, ess, rhat, nullptr, 0);
}

int lf_diag_last(double* kernel_ms, int64_t* lags) {
    if (!kernel_ms || !lags) return LF_ERR_ARG;
    *kernel_ms = g_diag_ms;
    *lags = g_diag_lags;
    return g_diag_ms < 0.0 ? LF_ERR_ARG : LF_OK;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------------------------------
// Mock catalogues (csrc/lf_mock.h).  Rows go through the kernels in chunks of `rch` (the cumulative
// sums of a chunk fit a fixed workspace budget); each row's work is independent of the chunk it is in.
// ------------------------------------------------------------------------------------------------------------------------
struct lf_mock {
    int device = 0;
    lf::MockConst mc{};
    int rch = 1;                          // rows per chunk
    Buf<double> d_grid[5];                // logL, zarr, volume_part, dl_zarr, integ_part
    Buf<double> d_theta, d_cdfL, d_colm, d_cdfZ, d_mean;
    Buf<long long> d_rid, d_count, d_off;
    Buf<double> d_z, d_L, d_edges;        // d_z, d_L, d_fld: the sources of the largest chunk drawn so far
    Buf<int> d_fld;
    Buf<unsigned long long> d_hist;
    lf::MockNoise mn{};                   // the error model (section 3.23); mn.M == 0: none set
    Buf<double> d_nodes, d_sigma, d_ld2n; // its tables
    Buf<double> d_Lobs, d_sg;             // as d_z: the observed luminosities and sigmas of the largest chunk drawn so far
    bool band = false;                    // the cut process (section 3.32): lf_mock_set_cut_band has made piece "below"
    lf::MockConst mcb{};                  // mc with the band's logL and integ_part; a field without errors has no mass in it
    Buf<double> d_logLb, d_ipb;
    Buf<double> d_cdfLb, d_colmb, d_cdfZb, d_meanb;       // the band's cumulative sums of a chunk, as d_cdfL ..
    Buf<long long> d_countb, d_offb, d_dst;               // d_dst: [2][rch nf] the pieces' first slots in the outputs
    Buf<int> d_keep;
    Buf<unsigned long long> d_kept;
    Buf<double> d_zedges;                 // the redshift edges of lf_mock_hist2* (section 3.35), made at the first such call
    std::string err;
};

namespace {

thread_local std::string g_mock_create_error = "";
constexpr size_t MOCK_WORKSPACE = (size_t)512 << 20;      // bytes of cumulative sums per chunk of rows

int mock_fail(lf_mock* m, const char* fn, const std::string& msg) {
    m->err = std::string(fn) + ": " + msg;
    return LF_ERR_ARG;
}

enum MockNeeds { MOCK_NEEDS_NOTHING, MOCK_NEEDS_MODEL, MOCK_NEEDS_BAND };      // what a process needs set: sections 3.23, 3.32

// the arguments every call shares, in the order every call refuses them; row r's theta must be finite
int mock_check(lf_mock* m, const char* fn, const double* theta, int32_t R, MockNeeds needs = MOCK_NEEDS_NOTHING) {
    if (R <= 0) return mock_fail(m, fn, "R must be >= 1");
    if (!theta) return mock_fail(m, fn, "theta is NULL");
    const int nd = m->mc.ndim;
    for (int32_t r = 0; r < R; ++r)
        for (int d = 0; d < nd; ++d)
            if (!std::isfinite(theta[(size_t)r * nd + d]))
                return mock_fail(m, fn, "row " + std::to_string(r) + ": theta is not finite");
    m->err.clear();
    if (needs >= MOCK_NEEDS_MODEL && m->mn.M == 0) return mock_fail(m, fn, "no error model is set (lf_mock_set_error_model)");
    if (needs >= MOCK_NEEDS_BAND && !m->band)
        return mock_fail(m, fn, "no cut band is set (lf_mock_set_cut_band, after lf_mock_set_error_model)");
    return LF_OK;
}

int mock_edges_ok(lf_mock* m, const char* fn, const char* name, int32_t n, const double* e) {
    for (int i = 0; i <= n; ++i)
        if (!std::isfinite(e[i]) || (i > 0 && !(e[i] >= e[i - 1])))
            return mock_fail(m, fn, std::string(name) + " must be finite and non-decreasing");
    return LF_OK;
}

// the caller's counts [R nf], each in 0 .. 2^32 - 1; *total: their sum
int mock_counts_ok(lf_mock* m, const char* fn, const int64_t* count, int32_t R, int64_t* total) {
    const int nf = m->mc.nf;
    *total = 0;
    for (int64_t i = 0; i < (int64_t)R * nf; ++i) {
        if (count[i] < 0 || count[i] > (int64_t)UINT32_MAX)
            return mock_fail(m, fn, "row " + std::to_string(i / nf) + " field " + std::to_string(i % nf) + ": count out of range");
        *total += count[i];
    }
    return LF_OK;
}

// One piece of a mock process: what its kernels read, and where a chunk's cumulative sums, means, counts and offsets are.
// Piece 0 is the process on the integration grid (piece "above" of the cut process), piece 1 the band's (piece "below").
struct MockPiece {
    const lf::MockConst& mc;
    double *cdfL, *colm, *cdfZ, *mean;
    long long *count, *off;
    lf::MockCut ct;
};

MockPiece mock_piece(lf_mock* m, int piece) {
    if (piece) return {m->mcb, m->d_cdfLb, m->d_colmb, m->d_cdfZb, m->d_meanb, m->d_countb, m->d_offb, {m->d_grid[0], lf::MOCK_CUT_BAND}};
    return {m->mc, m->d_cdfL, m->d_colm, m->d_cdfZ, m->d_mean, m->d_count, m->d_off, {m->d_grid[0], 0u}};
}

// masses, cumulative sums, means and counts of one piece for the n rows from r0 that are on the device, means and counts
// copied to the host; the band draws its counts from its own Poisson stream; a refused mean ends with `suffix`
int mock_masses(lf_mock* m, const char* fn, const MockPiece& p, const char* suffix, int32_t r0, int n, uint64_t seed,
                std::vector<double>& mean, std::vector<long long>& count) {
    const int nf = m->mc.nf, S = m->mc.S, nrf = n * nf;
    hipLaunchKernelGGL(lf::lf_mock_mass, dim3((unsigned)S, (unsigned)nrf), dim3(lf::MOCK_THREADS), 0, 0, p.mc, m->d_theta, p.cdfL, p.colm);
    LF_HIP(m, hipGetLastError());
    hipLaunchKernelGGL(lf::lf_mock_total, dim3((unsigned)nrf), dim3(lf::MOCK_THREADS), 0, 0, S, nf, p.colm, m->d_rid,
                       (unsigned long long)seed, p.cdfZ, p.mean, p.count);
    LF_HIP(m, hipGetLastError());
    if (p.ct.stream) {
        hipLaunchKernelGGL(lf::lf_mock_count_cut, dim3((unsigned)((nrf + lf::MOCK_THREADS - 1) / lf::MOCK_THREADS)), dim3(lf::MOCK_THREADS),
                           0, 0, nrf, nf, p.mean, m->d_rid, (unsigned long long)seed, p.count);
        LF_HIP(m, hipGetLastError());
    }
    mean.resize((size_t)nrf);
    count.resize((size_t)nrf);
    LF_HIP(m, hipMemcpy(mean.data(), p.mean, (size_t)nrf * sizeof(double), hipMemcpyDeviceToHost));
    LF_HIP(m, hipMemcpy(count.data(), p.count, (size_t)nrf * sizeof(long long), hipMemcpyDeviceToHost));
    for (int i = 0; i < nrf; ++i)
        if (count[(size_t)i] < 0) {
            char b[200];
            std::snprintf(b, sizeof b, "row %d field %d: expected count %.17g is not finite, negative or above 2^31%s", r0 + i / nf, i % nf,
                          mean[(size_t)i], suffix);
            return mock_fail(m, fn, b);
        }
    return LF_OK;
}

// rows r0 .. r0 + n - 1 to the device, then mock_masses of the process's pieces: one, or the cut process's two - "above" is
// refused before "below" is launched, and a refused mean names its piece
int mock_chunk(lf_mock* m, const char* fn, int npiece, const double* theta, int32_t r0, int n, const int64_t* row_ids, uint64_t seed,
               std::vector<double> (&mean)[2], std::vector<long long> (&count)[2]) {
    const int nd = m->mc.ndim;
    std::vector<long long> rid((size_t)n);
    for (int i = 0; i < n; ++i) rid[(size_t)i] = row_ids ? (long long)row_ids[r0 + i] : (long long)(r0 + i);
    LF_HIP(m, hipMemcpy(m->d_theta, theta + (size_t)r0 * nd, (size_t)n * nd * sizeof(double), hipMemcpyHostToDevice));
    LF_HIP(m, hipMemcpy(m->d_rid, rid.data(), (size_t)n * sizeof(long long), hipMemcpyHostToDevice));
    static const char* const suffix[2] = {" (piece \"above\")", " (piece \"below\")"};
    for (int piece = 0; piece < npiece; ++piece) {
        const int rc = mock_masses(m, fn, mock_piece(m, piece), npiece == 2 ? suffix[piece] : "", r0, n, seed, mean[piece], count[piece]);
        if (rc != LF_OK) return rc;
    }
    return LF_OK;
}

// every buffer that holds fewer than n elements is replaced by one of n (each by its own size: after a failed allocation the
// empty one is made again)
int mock_grow(lf_mock*, size_t) { return LF_OK; }
template <typename T, typename... Rest>
int mock_grow(lf_mock* m, size_t n, Buf<T>& b, Rest&... rest) {
    const int rc = n > b.size() ? grow(m, b, n, false) : LF_OK;
    return rc != LF_OK ? rc : mock_grow(m, n, rest...);
}

// mock_fetch(m, n, host, buffer, host, buffer, ...): the first n elements of every buffer to its host array
int mock_fetch(lf_mock*, size_t) { return LF_OK; }
template <typename H, typename T, typename... Rest>
int mock_fetch(lf_mock* m, size_t n, H* host, const Buf<T>& b, Rest&&... rest) {
    static_assert(sizeof(H) == sizeof(T), "host and device element sizes differ");
    LF_HIP(m, hipMemcpy(host, b, n * sizeof(T), hipMemcpyDeviceToHost));
    return mock_fetch(m, n, rest...);
}

// lf_mock_draw (noisy = false: logL_obs and sigma are not used) and lf_mock_draw_err
int mock_draw(lf_mock* m, const char* fn, bool noisy, const double* theta, int32_t R, const int64_t* row_ids, uint64_t seed,
              const int64_t* count, double* z, double* logL, double* logL_obs, double* sigma, int32_t* field) {
    if (!m) return LF_ERR_ARG;
    int rc = mock_check(m, fn, theta, R, noisy ? MOCK_NEEDS_MODEL : MOCK_NEEDS_NOTHING);
    if (rc != LF_OK) return rc;
    if (!count) return mock_fail(m, fn, "count is NULL");
    int64_t total;
    if ((rc = mock_counts_ok(m, fn, count, R, &total)) != LF_OK) return rc;
    if (total > 0 && (!z || !logL || !field || (noisy && (!logL_obs || !sigma))))
        return mock_fail(m, fn, noisy ? "z, logL_true, logL_obs, sigma or field is NULL" : "z, logL or field is NULL");
    LF_HIP(m, hipSetDevice(m->device));
    const int nf = m->mc.nf;
    std::vector<double> mu[2];
    std::vector<long long> n[2], off;
    int64_t done = 0;
    for (int32_t r0 = 0; r0 < R; r0 += m->rch) {
        const int rows = std::min<int32_t>(m->rch, R - r0);
        const int nrf = rows * nf;
        off.assign((size_t)nrf + 1, 0);
        for (int i = 0; i < nrf; ++i) off[(size_t)i + 1] = off[(size_t)i] + count[(size_t)r0 * nf + i];
        const int64_t tot = off[(size_t)nrf];
        if (tot == 0) continue;
        if ((rc = mock_chunk(m, fn, 1, theta, r0, rows, row_ids, seed, mu, n)) != LF_OK) return rc;
        rc = noisy ? mock_grow(m, (size_t)tot, m->d_z, m->d_L, m->d_Lobs, m->d_sg, m->d_fld)
                   : mock_grow(m, (size_t)tot, m->d_z, m->d_L, m->d_fld);
        if (rc != LF_OK) return rc;
        LF_HIP(m, hipMemcpy(m->d_off, off.data(), off.size() * sizeof(long long), hipMemcpyHostToDevice));
        const dim3 grid((unsigned)((tot + lf::MOCK_THREADS - 1) / lf::MOCK_THREADS)), block(lf::MOCK_THREADS);
        if (noisy)
            hipLaunchKernelGGL(lf::lf_mock_draw_err, grid, block, 0, 0, m->mc, m->mn, nrf, m->d_off, m->d_rid, (unsigned long long)seed,
                               m->d_cdfL, m->d_cdfZ, m->d_z, m->d_L, m->d_Lobs, m->d_sg, m->d_fld);
        else
            hipLaunchKernelGGL(lf::lf_mock_draw, grid, block, 0, 0, m->mc, nrf, m->d_off, m->d_rid, (unsigned long long)seed, m->d_cdfL,
                               m->d_cdfZ, m->d_z, m->d_L, m->d_fld);
        LF_HIP(m, hipGetLastError());
        rc = noisy ? mock_fetch(m, (size_t)tot, z + done, m->d_z, logL + done, m->d_L, logL_obs + done, m->d_Lobs, sigma + done, m->d_sg,
                                field + done, m->d_fld)
                   : mock_fetch(m, (size_t)tot, z + done, m->d_z, logL + done, m->d_L, field + done, m->d_fld);
        if (rc != LF_OK) return rc;
        done += tot;
    }
    return LF_OK;
}

// The loop of the six histogram entries, after their checks and the upload of their edges: per chunk of rows the masses of
// the process's npiece pieces, the caller's counts in the place of the Poisson draws (count: NULL = keep those), d_hist (ns
// slots per (row, field)) and, with `kept`, d_kept zeroed, per piece the prefix sums of its workgroups and one launch, then
// hist and kept copied out.  launch(piece view, nrf, grid) starts the entry's kernel: the piece's `off` holds the prefix sums.
template <typename Launch>
int mock_binned(lf_mock* m, const char* fn, int npiece, const double* theta, int32_t R, const int64_t* row_ids, uint64_t seed,
                const int64_t* count, int64_t ns, int64_t* hist, int64_t* kept, Launch launch) {
    int rc;
    const int nf = m->mc.nf;
    std::vector<double> mu[2];
    std::vector<long long> n[2], blk;
    for (int32_t r0 = 0; r0 < R; r0 += m->rch) {
        const int rows = std::min<int32_t>(m->rch, R - r0);
        const int nrf = rows * nf;
        if ((rc = mock_chunk(m, fn, npiece, theta, r0, rows, row_ids, seed, mu, n)) != LF_OK) return rc;
        if (count) {          // the caller's counts take the place of the Poisson draws lf_mock_total left on the device
            for (int i = 0; i < nrf; ++i) n[0][(size_t)i] = (long long)count[(size_t)r0 * nf + i];
            LF_HIP(m, hipMemcpy(m->d_count, n[0].data(), (size_t)nrf * sizeof(long long), hipMemcpyHostToDevice));
        }
        if ((rc = mock_grow(m, (size_t)nrf * ns, m->d_hist)) != LF_OK) return rc;
        LF_HIP(m, hipMemset(m->d_hist, 0, (size_t)nrf * ns * sizeof(unsigned long long)));
        if (kept) LF_HIP(m, hipMemset(m->d_kept, 0, (size_t)nrf * sizeof(unsigned long long)));
        for (int piece = 0; piece < npiece; ++piece) {
            blk.assign((size_t)nrf + 1, 0);
            for (int i = 0; i < nrf; ++i)
                blk[(size_t)i + 1] = blk[(size_t)i] + (n[piece][(size_t)i] + lf::MOCK_HIST_CHUNK - 1) / lf::MOCK_HIST_CHUNK;
            const long long nblk = blk[(size_t)nrf];
            if (nblk == 0) continue;
            if (nblk > (long long)INT32_MAX) return mock_fail(m, fn, "too many sources for one launch: pass fewer rows per call");
            const MockPiece p = mock_piece(m, piece);
            LF_HIP(m, hipMemcpy(p.off, blk.data(), blk.size() * sizeof(long long), hipMemcpyHostToDevice));
            launch(p, nrf, dim3((unsigned)nblk));
            LF_HIP(m, hipGetLastError());
        }
        if ((rc = mock_fetch(m, (size_t)nrf * ns, hist + (size_t)r0 * nf * ns, m->d_hist)) != LF_OK) return rc;
        if (kept && (rc = mock_fetch(m, (size_t)nrf, kept + (size_t)r0 * nf, m->d_kept)) != LF_OK) return rc;
    }
    return LF_OK;
}

// The three histograms in luminosity alone: their checks, the edges to the device, then mock_binned.  needs == MOCK_NEEDS_BAND
// is the cut process: two pieces, and `kept` is an output
template <typename Launch>
int mock_hist1(lf_mock* m, const char* fn, MockNeeds needs, const double* theta, int32_t R, const int64_t* row_ids, uint64_t seed,
               int32_t nbins, const double* edges, int64_t* hist, int64_t* kept, Launch launch) {
    if (!m) return LF_ERR_ARG;
    const bool cut = needs == MOCK_NEEDS_BAND;
    int rc = mock_check(m, fn, theta, R, needs);
    if (rc != LF_OK) return rc;
    if (nbins < 1 || nbins > lf::MOCK_MAX_BINS) return mock_fail(m, fn, "nbins must be in 1.." + std::to_string(lf::MOCK_MAX_BINS));
    if (!edges || !hist || (cut && !kept)) return mock_fail(m, fn, cut ? "edges, hist or kept is NULL" : "edges or hist is NULL");
    if ((rc = mock_edges_ok(m, fn, "edges", nbins, edges)) != LF_OK) return rc;
    LF_HIP(m, hipSetDevice(m->device));
    LF_HIP(m, hipMemcpy(m->d_edges, edges, (size_t)(nbins + 1) * sizeof(double), hipMemcpyHostToDevice));
    return mock_binned(m, fn, cut ? 2 : 1, theta, R, row_ids, seed, nullptr, nbins + 2, hist, kept, launch);
}

}  // namespace

extern "C" {

lf_mock* lf_mock_create(const lf_desc* d) {
    g_mock_create_error.clear();
    auto bad = [&](const std::string& msg) {
        g_mock_create_error = "lf_mock_create: " + msg;
        return (lf_mock*)nullptr;
    };
    if (!d) return bad("NULL descriptor");
    if (d->variant < LF_FREE || d->variant > LF_ZEVOL) return bad("unknown variant");
    if (d->nf < 1 || d->nf > LF_MAX_FIELDS) return bad("nf out of range (1..LF_MAX_FIELDS)");
    if (d->S < 2 || d->S > 4096) return bad("S out of range");
    if (!d->logL || !d->zarr) return bad("NULL logL/zarr");
    if (d->variant == LF_FREE) {
        if (!d->volume_part || !d->dl_zarr || !d->omega0) return bad("FREE needs volume_part, dl_zarr, omega0");
        if (!(d->fcmin > 0.0 && d->fcmin < 1.0) || d->fcmin == 0.5) return bad("fcmin must be in (0,1), != 0.5");
    } else {
        if (!d->integ_part) return bad("FIXCOMP/ZEVOL need integ_part");
        if (d->variant == LF_ZEVOL && (d->pivots[0] == d->pivots[1] || d->pivots[0] == d->pivots[2] || d->pivots[1] == d->pivots[2]))
            return bad("ZEVOL pivots must be distinct");
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return bad("no HIP device visible");
    if (d->device < 0 || d->device >= ndev) return bad("device ordinal out of range");
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, d->device) != hipSuccess) return bad("hipGetDeviceProperties failed");
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return bad(std::string("device is ") + prop.gcnArchName + ", this library is built for gfx950 only");
    if (hipSetDevice(d->device) != hipSuccess) return bad("hipSetDevice failed");
    lf_mock* m = new (std::nothrow) lf_mock();
    if (!m) return bad("out of host memory");
    m->device = d->device;
    lf::MockConst& mc = m->mc;
    const int S = d->S, nf = d->nf;
    mc.variant = d->variant;
    mc.fix_sch_al = d->fix_sch_al ? 1 : 0;
    mc.nf = nf;
    mc.S = S;
    mc.ndim = d->variant == LF_ZEVOL ? 6 + (mc.fix_sch_al ? 0 : 1) : 2 + (mc.fix_sch_al ? 0 : 1) + (d->variant == LF_FREE ? nf + 1 : 0);
    mc.sch_al0 = d->sch_al0;
    const double sq = 180.0 / M_PI * 3600.0, sqarcsec = sq * sq;       // VmaxLumFunc.py:43
    for (int f = 0; f < nf; ++f) mc.om0s[f] = d->variant == LF_FREE ? d->omega0[f] / sqarcsec : 0.0;
    if (d->variant == LF_FREE) mc.fc_ratio = lfh::fc_ratio(d->fcmin);
    for (int i = 0; i < 3; ++i) mc.pivots[i] = d->pivots[i];
    const size_t SS = (size_t)S * S;
    const double* src[5] = {d->logL, d->zarr, d->variant == LF_FREE ? d->volume_part : nullptr,
                            d->variant == LF_FREE ? d->dl_zarr : nullptr, d->variant == LF_FREE ? nullptr : d->integ_part};
    const size_t len[5] = {SS, (size_t)S, (size_t)S, (size_t)S, (size_t)nf * SS};
    const size_t per_rf = SS + 2 * (size_t)S;           // doubles of cumulative sums per (row, field)
    m->rch = (int)std::max<size_t>(1, std::min<size_t>(1024, MOCK_WORKSPACE / (per_rf * nf * sizeof(double))));
    const size_t nrf = (size_t)m->rch * nf;
    bool ok = true;
    for (int i = 0; i < 5 && ok; ++i)
        if (src[i]) ok = m->d_grid[i].upload(src[i], len[i]) == hipSuccess;
    ok = ok && alloc_all(m->d_theta, (size_t)m->rch * mc.ndim, m->d_rid, (size_t)m->rch, m->d_cdfL, nrf * SS, m->d_colm, nrf * S,
                         m->d_cdfZ, nrf * S, m->d_mean, nrf, m->d_count, nrf, m->d_off, nrf + 1, m->d_edges,
                         (size_t)lf::MOCK_MAX_BINS + 1) == hipSuccess;
    if (!ok) {
        delete m;
        return bad("device allocation or copy failed");
    }
    mc.logL = m->d_grid[0];
    mc.zarr = m->d_grid[1];
    mc.volume_part = m->d_grid[2];
    mc.dl_zarr = m->d_grid[3];
    mc.integ_part = m->d_grid[4];
    return m;
}

void lf_mock_destroy(lf_mock* m) {
    if (!m) return;
    hipSetDevice(m->device);
    delete m;
}

const char* lf_mock_last_error(const lf_mock* m) { return m ? m->err.c_str() : g_mock_create_error.c_str(); }

int lf_mock_counts(lf_mock* m, const double* theta, int32_t R, const int64_t* row_ids, uint64_t seed, double* mean, int64_t* count) {
    static const char* fn = "lf_mock_counts";
    if (!m) return LF_ERR_ARG;
    int rc = mock_check(m, fn, theta, R);
    if (rc != LF_OK) return rc;
    if (!mean || !count) return mock_fail(m, fn, "mean or count is NULL");
    LF_HIP(m, hipSetDevice(m->device));
    const int nf = m->mc.nf;
    std::vector<double> mu[2];
    std::vector<long long> n[2];
    for (int32_t r0 = 0; r0 < R; r0 += m->rch) {
        const int rows = std::min<int32_t>(m->rch, R - r0);
        if ((rc = mock_chunk(m, fn, 1, theta, r0, rows, row_ids, seed, mu, n)) != LF_OK) return rc;
        for (size_t i = 0; i < mu[0].size(); ++i) {
            mean[(size_t)r0 * nf + i] = mu[0][i];
            count[(size_t)r0 * nf + i] = n[0][i];
        }
    }
    return LF_OK;
}

int lf_mock_draw(lf_mock* m, const double* theta, int32_t R, const int64_t* row_ids, uint64_t seed, const int64_t* count, double* z,
                 double* logL, int32_t* field) {
    return mock_draw(m, "lf_mock_draw", false, theta, R, row_ids, seed, count, z, logL, nullptr, nullptr, field);
}

int lf_mock_hist(lf_mock* m, const double* theta, int32_t R, const int64_t* row_ids, uint64_t seed, int32_t nbins, const double* edges,
                 int64_t* hist) {
    auto launch = [&](const MockPiece& p, int nrf, dim3 grid) {
        hipLaunchKernelGGL(lf::lf_mock_hist, grid, dim3(lf::MOCK_THREADS), 0, 0, p.mc, nrf, p.off, p.count, m->d_rid,
                           (unsigned long long)seed, p.cdfL, p.cdfZ, nbins, m->d_edges, m->d_hist);
    };
    return mock_hist1(m, "lf_mock_hist", MOCK_NEEDS_NOTHING, theta, R, row_ids, seed, nbins, edges, hist, nullptr, launch);
}

// The error model of the observation step (csrc/lf_mock_noise.h).
int lf_mock_set_error_model(lf_mock* m, int32_t M, const double* logf_nodes, const double* sigma, const double* dl_zarr) {
    static const char* fn = "lf_mock_set_error_model";
    if (!m) return LF_ERR_ARG;
    m->err.clear();
    if (M == 0) {
        m->mn.M = 0;
        m->band = false;
        return LF_OK;
    }
    if (M < 0 || M > lf::MOCK_MAX_NODES) return mock_fail(m, fn, "M must be in 0.." + std::to_string(lf::MOCK_MAX_NODES));
    if (!logf_nodes || !sigma || !dl_zarr) return mock_fail(m, fn, "logf_nodes, sigma or dl_zarr is NULL");
    const int nf = m->mc.nf, S = m->mc.S;
    for (int i = 0; i < M; ++i)
        if (!std::isfinite(logf_nodes[i]) || (i > 0 && !(logf_nodes[i] > logf_nodes[i - 1])))
            return mock_fail(m, fn, "node " + std::to_string(i) + ": logf_nodes must be finite and strictly ascending");
    for (int f = 0; f < nf; ++f)
        for (int i = 0; i < M; ++i)
            if (!std::isfinite(sigma[(size_t)f * M + i]) || sigma[(size_t)f * M + i] < 0.0)
                return mock_fail(m, fn, "field " + std::to_string(f) + " node " + std::to_string(i) + ": sigma must be finite and >= 0");
    std::vector<double> ld2n((size_t)S);
    for (int k = 0; k < S; ++k) {
        if (!std::isfinite(dl_zarr[k]) || !(dl_zarr[k] > 0.0))
            return mock_fail(m, fn, "dl_zarr[" + std::to_string(k) + "] must be finite and > 0");
        const double dl = 3.086e24 * dl_zarr[k];
        ld2n[(size_t)k] = std::log10(4.0 * 3.141592653589793 * (dl * dl));
    }
    LF_HIP(m, hipSetDevice(m->device));
    m->mn.M = 0;                          // (a failed upload leaves no model)
    m->band = false;                      // (a band belongs to the model it was made under: lf_mock_set_cut_band comes after)
    LF_HIP(m, m->d_nodes.upload(logf_nodes, (size_t)M));
    LF_HIP(m, m->d_sigma.upload(sigma, (size_t)nf * M));
    LF_HIP(m, m->d_ld2n.upload(ld2n.data(), (size_t)S));
    m->mn.nodes = m->d_nodes;
    m->mn.sigma = m->d_sigma;
    m->mn.ld2n = m->d_ld2n;
    m->mn.M = M;
    return LF_OK;
}

int lf_mock_draw_err(lf_mock* m, const double* theta, int32_t R, const int64_t* row_ids, uint64_t seed, const int64_t* count, double* z,
                     double* logL_true, double* logL_obs, double* sigma, int32_t* field) {
    return mock_draw(m, "lf_mock_draw_err", true, theta, R, row_ids, seed, count, z, logL_true, logL_obs, sigma, field);
}

int lf_mock_hist_err(lf_mock* m, const double* theta, int32_t R, const int64_t* row_ids, uint64_t seed, int32_t nbins,
                     const double* edges, int64_t* hist) {
    auto launch = [&](const MockPiece& p, int nrf, dim3 grid) {
        hipLaunchKernelGGL(lf::lf_mock_hist_err, grid, dim3(lf::MOCK_THREADS), 0, 0, p.mc, m->mn, nrf, p.off, p.count, m->d_rid,
                           (unsigned long long)seed, p.cdfL, p.cdfZ, nbins, m->d_edges, m->d_hist);
    };
    return mock_hist1(m, "lf_mock_hist_err", MOCK_NEEDS_MODEL, theta, R, row_ids, seed, nbins, edges, hist, nullptr, launch);
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------------------------------
// Mock catalogues of the cut process (csrc/lf_mock_cut.h)
// ------------------------------------------------------------------------------------------------------------------------
extern "C" {

int lf_mock_set_cut_band(lf_mock* m, const double* logLb, const double* integ_part_b) {
    static const char* fn = "lf_mock_set_cut_band";
    if (!m) return LF_ERR_ARG;
    m->err.clear();
    if (m->mn.M == 0) return mock_fail(m, fn, "no error model is set: lf_mock_set_error_model comes first");
    if (!logLb) return mock_fail(m, fn, "logLb is NULL");
    const int nf = m->mc.nf, S = m->mc.S, M = m->mn.M;
    const size_t SS = (size_t)S * S;
    const bool table = m->mc.variant != LF_FREE;
    if (table && !integ_part_b) return mock_fail(m, fn, "FIXCOMP/ZEVOL need integ_part_b (the fixed completeness curve at the band's nodes)");
    LF_HIP(m, hipSetDevice(m->device));
    std::vector<double> edge((size_t)S), sig((size_t)nf * M);
    LF_HIP(m, hipMemcpy(edge.data(), m->d_grid[0], (size_t)S * sizeof(double), hipMemcpyDeviceToHost));
    LF_HIP(m, hipMemcpy(sig.data(), m->d_sigma, sig.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (int k = 0; k < S; ++k) {
        for (int j = 0; j < S; ++j)
            if (!std::isfinite(logLb[(size_t)j * S + k]) || (j > 0 && !(logLb[(size_t)j * S + k] > logLb[(size_t)(j - 1) * S + k])))
                return mock_fail(m, fn, "column " + std::to_string(k) + " node " + std::to_string(j) +
                                            ": the band's luminosity nodes must be finite and strictly ascending");
        if (logLb[(size_t)(S - 1) * S + k] != edge[(size_t)k])
            return mock_fail(m, fn, "column " + std::to_string(k) + ": row S - 1 of logLb must equal row 0 of logL (the edge of the cut)");
    }
    std::vector<double> ipb;
    if (table) {
        ipb.assign(integ_part_b, integ_part_b + (size_t)nf * SS);
        for (size_t i = 0; i < ipb.size(); ++i)
            if (!std::isfinite(ipb[i]) || ipb[i] < 0.0)
                return mock_fail(m, fn, "field " + std::to_string(i / SS) + ": integ_part_b must be finite and >= 0");
    }
    m->band = false;
    m->mcb = m->mc;
    // a field whose sigma is 0 everywhere keeps no band source: it gets no mass (and so no candidates)
    for (int f = 0; f < nf; ++f) {
        bool none = true;
        for (int i = 0; i < M; ++i) none = none && sig[(size_t)f * M + i] == 0.0;
        if (!none) continue;
        if (table) std::fill(ipb.begin() + (size_t)f * SS, ipb.begin() + (size_t)(f + 1) * SS, 0.0);
        else m->mcb.om0s[f] = 0.0;
    }
    LF_HIP(m, m->d_logLb.upload(logLb, SS));
    if (table) LF_HIP(m, m->d_ipb.upload(ipb.data(), ipb.size()));
    const size_t nrf = (size_t)m->rch * nf;
    if (m->d_cdfLb.size() < nrf * SS)
        LF_HIP(m, alloc_all(m->d_cdfLb, nrf * SS, m->d_colmb, nrf * S, m->d_cdfZb, nrf * S, m->d_meanb, nrf, m->d_countb, nrf, m->d_offb,
                            nrf + 1, m->d_dst, 2 * nrf, m->d_kept, nrf));
    m->mcb.logL = m->d_logLb;
    m->mcb.integ_part = table ? m->d_ipb.get() : nullptr;
    m->band = true;
    return LF_OK;
}

int lf_mock_draw_cut(lf_mock* m, const double* theta, int32_t R, const int64_t* row_ids, uint64_t seed, int64_t cap, double* z,
                     double* logL_true, double* logL_obs, double* sigma, int32_t* field, int32_t* keep, int64_t* n_cand, double* mean,
                     int64_t* kept) {
    static const char* fn = "lf_mock_draw_cut";
    if (!m) return LF_ERR_ARG;
    int rc = mock_check(m, fn, theta, R, MOCK_NEEDS_BAND);
    if (rc != LF_OK) return rc;
    if (!n_cand || !mean) return mock_fail(m, fn, "n_cand or mean is NULL");
    if (cap < 0) return mock_fail(m, fn, "cap must be >= 0");
    if (cap > 0 && (!z || !logL_true || !logL_obs || !sigma || !field || !keep || !kept))
        return mock_fail(m, fn, "z, logL_true, logL_obs, sigma, field, keep or kept is NULL");
    LF_HIP(m, hipSetDevice(m->device));
    const int nf = m->mc.nf;
    std::vector<double> mu[2];
    std::vector<long long> n[2], off, dst;
    int64_t total = 0;
    for (int32_t r0 = 0; r0 < R; r0 += m->rch) {
        const int rows = std::min<int32_t>(m->rch, R - r0);
        if ((rc = mock_chunk(m, fn, 2, theta, r0, rows, row_ids, seed, mu, n)) != LF_OK) return rc;
        for (int i = 0; i < rows * nf; ++i) {
            const size_t o = 2 * ((size_t)r0 * nf + i);
            n_cand[o] = n[0][(size_t)i], n_cand[o + 1] = n[1][(size_t)i];
            mean[o] = mu[0][(size_t)i], mean[o + 1] = mu[1][(size_t)i];
            total += n[0][(size_t)i] + n[1][(size_t)i];
        }
    }
    if (total > cap || cap == 0) return LF_OK;          // the counts alone: the caller sizes the arrays and calls again
    for (int64_t i = 0; i < (int64_t)R * nf; ++i) kept[i] = 0;
    int64_t done = 0;
    for (int32_t r0 = 0; r0 < R; r0 += m->rch) {
        const int rows = std::min<int32_t>(m->rch, R - r0);
        const int nrf = rows * nf;
        // (one chunk: its cumulative sums are still on the device)
        if (R > m->rch && (rc = mock_chunk(m, fn, 2, theta, r0, rows, row_ids, seed, mu, n)) != LF_OK) return rc;
        const int64_t* nc = n_cand + 2 * (size_t)r0 * nf;
        dst.assign(2 * (size_t)nrf, 0);
        long long tot = 0;
        for (int i = 0; i < nrf; ++i) {
            dst[(size_t)i] = tot;
            dst[(size_t)nrf + i] = tot + nc[2 * i];
            tot += nc[2 * i] + nc[2 * i + 1];
        }
        if (tot == 0) continue;
        if ((rc = mock_grow(m, (size_t)tot, m->d_z, m->d_L, m->d_Lobs, m->d_sg, m->d_fld, m->d_keep)) != LF_OK) return rc;
        LF_HIP(m, hipMemcpy(m->d_dst, dst.data(), dst.size() * sizeof(long long), hipMemcpyHostToDevice));
        for (int piece = 0; piece < 2; ++piece) {
            off.assign((size_t)nrf + 1, 0);
            for (int i = 0; i < nrf; ++i) off[(size_t)i + 1] = off[(size_t)i] + nc[2 * i + piece];
            const long long np = off[(size_t)nrf];
            if (np == 0) continue;
            const MockPiece p = mock_piece(m, piece);
            LF_HIP(m, hipMemcpy(p.off, off.data(), off.size() * sizeof(long long), hipMemcpyHostToDevice));
            hipLaunchKernelGGL(lf::lf_mock_draw_cut, dim3((unsigned)((np + lf::MOCK_THREADS - 1) / lf::MOCK_THREADS)), dim3(lf::MOCK_THREADS),
                               0, 0, p.mc, m->mn, p.ct, nrf, p.off, m->d_dst + (size_t)piece * nrf, m->d_rid, (unsigned long long)seed,
                               p.cdfL, p.cdfZ, m->d_z, m->d_L, m->d_Lobs, m->d_sg, m->d_fld, m->d_keep);
            LF_HIP(m, hipGetLastError());
        }
        if ((rc = mock_fetch(m, (size_t)tot, z + done, m->d_z, logL_true + done, m->d_L, logL_obs + done, m->d_Lobs, sigma + done, m->d_sg,
                             field + done, m->d_fld, keep + done, m->d_keep)) != LF_OK)
            return rc;
        for (int i = 0; i < nrf; ++i) {
            const int64_t a = done + dst[(size_t)i], b = a + nc[2 * i] + nc[2 * i + 1];
            int64_t k = 0;
            for (int64_t s = a; s < b; ++s) k += keep[s] != 0;
            kept[(size_t)r0 * nf + i] = k;
        }
        done += tot;
    }
    return LF_OK;
}

int lf_mock_hist_cut(lf_mock* m, const double* theta, int32_t R, const int64_t* row_ids, uint64_t seed, int32_t nbins,
                     const double* edges, int64_t* hist, int64_t* kept) {
    auto launch = [&](const MockPiece& p, int nrf, dim3 grid) {
        hipLaunchKernelGGL(lf::lf_mock_hist_cut, grid, dim3(lf::MOCK_THREADS), 0, 0, p.mc, m->mn, p.ct, nrf, p.off, p.count, m->d_rid,
                           (unsigned long long)seed, p.cdfL, p.cdfZ, nbins, m->d_edges, m->d_hist, m->d_kept);
    };
    return mock_hist1(m, "lf_mock_hist_cut", MOCK_NEEDS_BAND, theta, R, row_ids, seed, nbins, edges, hist, kept, launch);
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------------------------------
// The mocks binned in redshift and luminosity (csrc/lf_mock_hist2.h)
// ------------------------------------------------------------------------------------------------------------------------
namespace {

// the three entries: P = lf::MOCK_HIST2_PLAIN (count: NULL = the Poisson counts), _NOISY (the same), _CUT (count NULL; kept)
int mock_hist2(lf_mock* m, const char* fn, int P, const double* theta, int32_t R, const int64_t* row_ids, uint64_t seed,
               const int64_t* count, int32_t nz, const double* z_edges, int32_t nl, const double* edges, int64_t* hist, int64_t* kept) {
    if (!m) return LF_ERR_ARG;
    const MockNeeds needs = P == lf::MOCK_HIST2_CUT ? MOCK_NEEDS_BAND : P == lf::MOCK_HIST2_NOISY ? MOCK_NEEDS_MODEL : MOCK_NEEDS_NOTHING;
    int rc = mock_check(m, fn, theta, R, needs);
    if (rc != LF_OK) return rc;
    // (the slot count before the axes' upper limits: a grid that is too large hears of the limit it broke first)
    if (nz < 1) return mock_fail(m, fn, "nz must be in 1.." + std::to_string(lf::MOCK_MAX_BINS));
    if (nl < 1) return mock_fail(m, fn, "nl must be in 1.." + std::to_string(lf::MOCK_MAX_BINS));
    const int64_t ns = ((int64_t)nz + 2) * ((int64_t)nl + 2);
    if (ns > lf::MOCK_HIST2_MAX_SLOTS)
        return mock_fail(m, fn, "(nz + 2) * (nl + 2) = " + std::to_string(ns) + " slots: the limit is " +
                                    std::to_string(lf::MOCK_HIST2_MAX_SLOTS));
    if (nz > lf::MOCK_MAX_BINS) return mock_fail(m, fn, "nz must be in 1.." + std::to_string(lf::MOCK_MAX_BINS));
    if (nl > lf::MOCK_MAX_BINS) return mock_fail(m, fn, "nl must be in 1.." + std::to_string(lf::MOCK_MAX_BINS));
    if (!z_edges || !edges || !hist || (P == lf::MOCK_HIST2_CUT && !kept))
        return mock_fail(m, fn, P == lf::MOCK_HIST2_CUT ? "z_edges, edges, hist or kept is NULL" : "z_edges, edges or hist is NULL");
    if ((rc = mock_edges_ok(m, fn, "z_edges", nz, z_edges)) != LF_OK) return rc;
    if ((rc = mock_edges_ok(m, fn, "edges", nl, edges)) != LF_OK) return rc;
    int64_t total;
    if (count && (rc = mock_counts_ok(m, fn, count, R, &total)) != LF_OK) return rc;
    LF_HIP(m, hipSetDevice(m->device));
    if (m->d_zedges.size() == 0 && (rc = grow(m, m->d_zedges, (size_t)lf::MOCK_MAX_BINS + 1, false)) != LF_OK) return rc;
    LF_HIP(m, hipMemcpy(m->d_zedges, z_edges, (size_t)(nz + 1) * sizeof(double), hipMemcpyHostToDevice));
    LF_HIP(m, hipMemcpy(m->d_edges, edges, (size_t)(nl + 1) * sizeof(double), hipMemcpyHostToDevice));
    auto launch = [&](const MockPiece& p, int nrf, dim3 grid) {
        const dim3 block(lf::MOCK_THREADS);
        if (P == lf::MOCK_HIST2_PLAIN)
            hipLaunchKernelGGL(lf::lf_mock_hist2<lf::MOCK_HIST2_PLAIN>, grid, block, 0, 0, p.mc, m->mn, p.ct, nrf, p.off, p.count, m->d_rid,
                               (unsigned long long)seed, p.cdfL, p.cdfZ, nz, m->d_zedges, nl, m->d_edges, m->d_hist, nullptr);
        else if (P == lf::MOCK_HIST2_NOISY)
            hipLaunchKernelGGL(lf::lf_mock_hist2<lf::MOCK_HIST2_NOISY>, grid, block, 0, 0, p.mc, m->mn, p.ct, nrf, p.off, p.count, m->d_rid,
                               (unsigned long long)seed, p.cdfL, p.cdfZ, nz, m->d_zedges, nl, m->d_edges, m->d_hist, nullptr);
        else
            hipLaunchKernelGGL(lf::lf_mock_hist2<lf::MOCK_HIST2_CUT>, grid, block, 0, 0, p.mc, m->mn, p.ct, nrf, p.off, p.count, m->d_rid,
                               (unsigned long long)seed, p.cdfL, p.cdfZ, nz, m->d_zedges, nl, m->d_edges, m->d_hist, m->d_kept);
    };
    return mock_binned(m, fn, P == lf::MOCK_HIST2_CUT ? 2 : 1, theta, R, row_ids, seed, count, ns, hist, kept, launch);
}

}  // namespace

extern "C" {

int lf_mock_hist2(lf_mock* m, const double* theta, int32_t R, const int64_t* row_ids, uint64_t seed, const int64_t* count, int32_t nz,
                  const double* z_edges, int32_t nl, const double* edges, int64_t* hist) {
    return mock_hist2(m, "lf_mock_hist2", lf::MOCK_HIST2_PLAIN, theta, R, row_ids, seed, count, nz, z_edges, nl, edges, hist, nullptr);
}

int lf_mock_hist2_err(lf_mock* m, const double* theta, int32_t R, const int64_t* row_ids, uint64_t seed, const int64_t* count,
                      int32_t nz, const double* z_edges, int32_t nl, const double* edges, int64_t* hist) {
    return mock_hist2(m, "lf_mock_hist2_err", lf::MOCK_HIST2_NOISY, theta, R, row_ids, seed, count, nz, z_edges, nl, edges, hist, nullptr);
}

int lf_mock_hist2_cut(lf_mock* m, const double* theta, int32_t R, const int64_t* row_ids, uint64_t seed, int32_t nz,
                      const double* z_edges, int32_t nl, const double* edges, int64_t* hist, int64_t* kept) {
    return mock_hist2(m, "lf_mock_hist2_cut", lf::MOCK_HIST2_CUT, theta, R, row_ids, seed, nullptr, nz, z_edges, nl, edges, hist, kept);
}

}  // extern "C"
