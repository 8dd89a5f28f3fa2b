// lf_layout.h - what the host's table preparation (lf_hostprep.h) and the kernels (lf_kernels.h, lf_tile.h, lf_free.h) must
// agree on: the constants block KConst and the sizes, strides and scales of the tables.  No device code and nothing included: any
// C++17 compiler reads it.
#pragma once

#define LF_LN10 2.302585092994045684
#define LF_LREF 42.0        // P_i = 10^(lum_i - LF_LREF),  Q_w = 10^(LF_LREF - L*_w)
#define LF_FREF (-17.0)     // U_i = 10^(logf_i - LF_FREF)
#define LF_SQARCSEC 42545170296.152206       // (180/pi*3600)^2, VmaxLumFunc.py:43
#define LF_MPC_CM 3.086e24                   // lumfuncmcmc.py:70

namespace lf {

constexpr int BLOCK = 256;   // 4 waves
constexpr int MAXF = 8;
constexpr int KEY_STRIDE = 12;   // ints per chunk in SrcArrays::chunk_keys
constexpr int ZCOLS = 3;                  // redshift columns a chunk of the column-major z-evolving grid may touch
constexpr double KEY_SCALE = 1048576.0;     // keys of log-flux: (x - x0) * 2^20, 1e-6 dex
constexpr double KEY_ASCALE = 65536.0;      // keys of alpha_C
constexpr int KEY_MAX = 2147483000;

struct KConst {
    int variant, fix_sch_al, nf, S, ndim;
    int specialise;           // 1: chunk-level term specialisation (term_free_noexp); 0 for A/B runs
    int cells;                // FREE, ZEVOL: 1 = the catalogue's cells exist and lf_prepare may flag walkers STAT_CELLS
    int cc_fstart[MAXF + 1];  // FREE: cell chunks (64 cells) of field f are [cc_fstart[f], cc_fstart[f + 1])
    int zgrid_cols;           // ZEVOL: 1 = the grid's nodes are stored column by column (node = k S + j) and S >= BLOCK / (ZCOLS - 1),
                              // so that a chunk of BLOCK nodes touches at most ZCOLS redshift columns (gridsum_body)
    double zcell_rho;         // ZEVOL: half the largest width of a cell in redshift (lf_kernels.h: ZCELL_RHO)
    int kf_first[MAXF], kf_last[MAXF];   // FREE: keys (floor / ceil) of each field's faintest / brightest source
    int grid_part, grid_parts; // source-sharded ranks split piece B too: this context integrates the node chunks c with
                              // c % grid_parts == grid_part (the others contribute 0); 0 / 1 = the whole grid
    double lnom0_src[MAXF];   // ln(trunc(Omega_0[f]) / sqarcsec)   (int-truncated, lumfuncmcmc.py:285)
    double om0_grid[MAXF];    // Omega_0[f] / sqarcsec              (float, lumfuncmcmc.py:375)
    double fc_ratio;          // |a / (1 - a)|, a = (2 fcmin - 1)^2 (VmaxLumFunc.py:164-165)
    double lims[5][2];
    double pivots[3];
    double sch_al0, alpha0;
    double flim0[MAXF];
    // per-field extremes of the catalogue, for the mode classification
    int nsrc[MAXF];
    double pmax[MAXF];        // max 10^(lum-42)            (FREE, FIXCOMP)
    double lum_min[MAXF], lum_max[MAXF];
    double a_min[MAXF];       // FREE: min logf             FIXCOMP/ZEVOL: min ln(Om_arr)
    double u_min[MAXF];       // FREE: 10^(min logf + 17)
    double u_max[MAXF];       // FREE: 10^(max logf + 17)
    double z_lo[MAXF], z_hi[MAXF];   // ZEVOL
    double key_x0;            // FREE: origin of the integer keys of log-flux (the catalogue's smallest logf)
    int tables;               // FREE: 1 = table-driven form of the term where it applies (default), 0 = general form only
    // optional census of which form of the term / node ran (bench.py's flop accounting, tests): terms or node-fields
    // added per (walker, chunk) by one lane; NULL = off (the default: no atomics on the path)
    unsigned long long* forms;
#ifdef LF_STAMPS
    // diagnostic build (tools/stamps.py): s_memtime at four points of every source workgroup; never in the product
    unsigned long long* stamps;
#endif
    // per-field sums for the closed-form part of piece A:
    //   sum_i ln TrueLumFunc_i = n (ln ln10 + ln10 phi*) + c1 (sum(lum_i - 42) - n (L* - 42)) - Q sum P_i
    double slc[MAXF];         // sum (lum_i - 42)
    double sp[MAXF];          // sum 10^(lum_i - 42)
    double som[MAXF];         // FIXCOMP/ZEVOL: sum ln(Om_arr_i)
    double sz[MAXF], sz2[MAXF];   // ZEVOL: sum z_i, sum z_i^2  (L*(z), phi*(z) enter the log-terms linearly)
};

constexpr int GRIDC_MAX_S = 512;   // FREE: the largest grid side the compressed grid and the flux bins are built for

constexpr int PB = 512;      // threads per persistent workgroup: 8 waves
// The cells' and the grid's chunks of a tile are dealt to VF VIRTUAL workgroups, and partB / partC hold one partial sum per
// (walker, virtual workgroup): the workgroups that actually serve the tile (at most VF: 32 at 128 rows, 16 at 256, 8 when a
// group serves several tiles in turn) take the virtual ranks r, r + fgroup, ... and keep their sums apart.  So a walker's
// partial sums - and with them the bits of its lnprob - do not depend on how many rows share its call, on its place in
// the batch, or on how a batch is sharded over GPUs.
constexpr int VF = 32;
// The deal table: [0 .. VF] where rank vr's cell chunks start in the list, [VF + 1 .. 2 VF + 1] the same for its bins, then the
// list (cell chunks rank by rank, then bins rank by rank).  Who gets what is decided by COST: a flux bin costs a wave about
// 2.7 cell chunks, and the workgroups of ranks >= VF / 2 are the younger ones of their CUs, behind their elders when the sums
// begin (tools/stamps_fused.py) - the host deals bins, then cells, each to the rank that would be done first (lf_hostprep.h:
// make_deal has the costs and the sweep they come from).  With the arithmetic deal (bin c to rank c mod VF, cell chunk cc to rank (cc + VF / 2) mod VF) the busiest rank of the
// benchmark's context had a bin and two cell chunks (10.4k cycles), the average being 6.6k, and the 17th bin sat on a younger
// rank with two cell chunks of its own.  A context's table depends on its numbers of bins and cell chunks only: a row's
// partial sums (one per virtual rank) are the same whatever the batch.
constexpr int DEAL_BINS = VF + 1, DEAL_LIST = 2 * (VF + 1), DEAL_MAX = 512;

// The gradient kernels (lf_grad.h): sources / nodes per block, doubles per block in its partial sums (7 used at most), and the
// constants of a context they read (lf_hostprep.h: grad_const).
constexpr int GRAD_CH = 1024;
constexpr int GRAD_SLOTS = 8;
struct GradConst {
    int variant, fix_sch_al, nf, ndim;
    double sch_al0;
    double kappa;                // sqrt(KConst::fc_ratio): f_tau = F 10^(-kappa / alpha_C)
    double om0_grid[MAXF];
    double pivots[3];
    double sl[3];                // ZEVOL: sum_i l_m(z_i), l_m the Lagrange basis on the pivots (else 0)
    double nsrc;                 // N
};

// The flux-error-convolved likelihood (lf_deconv.h): sources per block, the supported Gauss-Hermite
// orders with the largest sigma (dex) each is validated for (worst per-source error below 1e-7 over the probe set of
// tests/test_deconv_cpu.py; lf_set_lum_err refuses larger values), and the default order.
constexpr int DECONV_CH = 1024;
constexpr int DECONV_KMAX = 32;
constexpr int DECONV_NORDERS = 9;
constexpr int DECONV_ORDERS[DECONV_NORDERS] = {4, 6, 8, 10, 12, 16, 20, 24, 32};
constexpr double DECONV_SIGMA_MAX[DECONV_NORDERS] = {0.01, 0.03, 0.04, 0.05, 0.06, 0.06, 0.07, 0.08, 0.09};
constexpr int DECONV_DEFAULT_ORDER = 32;
// Its wide rule (lf_deconv_wide.h), for sigma above the order's limit: the classes' upper edges (dex;
// the last is the largest sigma accepted), per class the panels of the composite Gauss-Legendre rule on [-T, T] sigma - the
// fewest that are at most DECONV_WIDE_H dex wide at the class's upper edge - the nodes per panel, and the sources per block.
constexpr int DECONV_WIDE_CH = 256;
constexpr int DECONV_WIDE_NCLASS = 5;
constexpr double DECONV_WIDE_EDGE[DECONV_WIDE_NCLASS] = {0.10, 0.15, 0.20, 0.25, 0.30};
constexpr int DECONV_WIDE_PANELS[DECONV_WIDE_NCLASS] = {6, 9, 12, 15, 18};
constexpr int DECONV_WIDE_NPAN = 8;
constexpr double DECONV_WIDE_T = 7.5;
constexpr double DECONV_WIDE_H = 0.25;
constexpr int DECONV_WIDE_KMAX = DECONV_WIDE_PANELS[DECONV_WIDE_NCLASS - 1] * DECONV_WIDE_NPAN;    // 144 nodes
struct DeconvConst {
    int K;                       // nodes
    double alpha0;               // FIXCOMP, ZEVOL: the fixed completeness the model was built with
    double flim0[MAXF];          // ... in theta's units (1e-17)
};
// The change of the expected counts under a cut on the OBSERVED flux (lf_deconv_cut.h): nodes per block;
// the half-width of the band around the cut in units of a field's largest sigma; the nodes of a panel of the composite
// Gauss-Legendre rule, a panel's largest width in units of the smallest sigma on it and in dex; |u| beyond which a panel is
// not made (Q(9) = 1.1e-19); the most panels on one side of one (field, column); the largest sigma the rule is validated for.
constexpr int DECONV_CUT_CH = 1024;
constexpr double DECONV_CUT_T = 7.5;
constexpr int DECONV_CUT_NPAN = 8;
constexpr double DECONV_CUT_PANEL_SIGMA = 2.5;
constexpr double DECONV_CUT_H = 0.25;
constexpr double DECONV_CUT_UMAX = 9.0;
constexpr int DECONV_CUT_MAX_PANELS = 64;
constexpr double DECONV_CUT_SIGMA_MAX = 0.30;
constexpr int DECONV_CUT_MAX_NODES = 64;     // nodes of an error model (lf_mock_noise.h: MOCK_MAX_NODES)
// The per-source posterior of the true luminosity (lf_lumpost.h).  LUMPOST_RT: rows of a tile, summed in
// row order; the tiles' sums are added in tile order.  A tile's rows share nothing but the node table and one 16-byte store
// per source, against K exponents each, so the height buys no arithmetic; 2 keeps the sum of LUMPOST_RT + 1 equal addends to
// one rounding (x + x is exact), which is what bounds the mean of equal rows to 2 ulp of the row's own value.  LUMPOST_SLABS:
// tiles of one launch, each with a slab of 2 doubles per source - the workspace is (LUMPOST_SLABS + 1) * 16 bytes per source
// whatever the number of rows; LUMPOST_MAX_ROWS: the rows of a call (the posterior bands' limit).
constexpr int LUMPOST_RT = 2;
constexpr int LUMPOST_SLABS = 16;
constexpr int LUMPOST_MAX_ROWS = 4096;

}  // namespace lf
