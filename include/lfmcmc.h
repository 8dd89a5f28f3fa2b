/*
 * lfmcmc.h - C ABI of liblfmcmc.so: the per-step log-posterior of LumFuncMCMC on MI355X (gfx950).
 *
 * The reference has no FFI: its hot path is a bound Python method handed to emcee,
 *     emcee.EnsembleSampler(nwalkers, ndim, self.lnprob)          lumfuncmcmc.py:487-489
 *     emcee.EnsembleSampler(nwalkers, ndim, self.lnprob)          lumfuncmcmc_z.py:444
 * with signature  f(theta: float64[ndim]) -> float  (-inf outside the prior or on underflow,
 * never NaN).  This header is the boundary a maintainer would bind instead (ctypes stub in
 * INTEGRATION.md): plain pointers and sizes, no torch / numpy types.
 *
 * Each entry point names the reference interface it replaces (file:line in the reference).
 *
 * Threading: one in-flight call per context; lf_create / lf_destroy are not thread-safe.
 * Ownership: the caller owns every host buffer it passes (they are copied during lf_create);
 * the library owns all device memory.  No entry point throws; errors are negative return codes
 * plus a message from lf_last_error().
 */
#ifndef LFMCMC_H
#define LFMCMC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LF_ABI_VERSION 3
#define LF_MAX_FIELDS 8

/* model variants = the three log-posterior callables of the reference */
enum {
    LF_FREE = 0,    /* LumFuncMCMC.lnprob          lumfuncmcmc.py:395-409  (completeness free)  */
    LF_FIXCOMP = 1, /* LumFuncMCMC.lnprob_fix_comp lumfuncmcmc.py:411-424  (completeness fixed) */
    LF_ZEVOL = 2    /* LumFuncMCMCz.lnprob         lumfuncmcmc_z.py:378-392 (z-evolving L*, phi*) */
};

/* return codes */
enum {
    LF_OK = 0,
    LF_ERR_ARG = -1,    /* bad descriptor / NULL pointer / B <= 0                       */
    LF_ERR_HIP = -2,    /* a HIP runtime call failed (message has the hipError string)   */
    LF_ERR_NOMEM = -3,  /* host or device allocation failed                              */
    LF_ERR_NODEV = -4   /* no gfx950 device visible                                      */
};

/* indices into lf_desc.lims: the *_lims constructor arguments, lumfuncmcmc.py:73-79 */
enum { LF_LIM_LSTAR = 0, LF_LIM_PHISTAR = 1, LF_LIM_SCH_AL = 2, LF_LIM_FLIM = 3, LF_LIM_ALPHA = 4 };

/*
 * Everything lnlike reads, i.e. the outputs of the reference's one-off setup
 * (setDLdVdz / setOmegaLz / setlnsimple / defineFlimOmArr, lumfuncmcmc.py:180-235, :283-288;
 * lumfuncmcmc_z.py:226-305).  Arrays are float64, C-contiguous.
 */
typedef struct lf_desc {
    int32_t variant;       /* LF_FREE | LF_FIXCOMP | LF_ZEVOL                                   */
    int32_t fix_sch_al;    /* 1: Schechter alpha is not in theta (lumfuncmcmc.py:330,333)       */
    int32_t nf;            /* number of fields, 1..LF_MAX_FIELDS (len(Flim), :147)              */
    int32_t S;             /* size_ln: side of the integration grid (101 free, 201 else; :219)  */
    int64_t N;             /* number of sources                                                 */
    const int64_t *field_ind; /* [nf+1] field f = sources field_ind[f] .. field_ind[f+1]-1 (:148) */
    const double *lum;     /* [N] log10 L (erg/s)                                    self.lum   */
    const double *logf;    /* [N] FREE: lum - log10(4 pi (3.086e24 DLf(z))^2)   (the flux of :70) */
    const double *z;       /* [N] ZEVOL: source redshifts                              self.z   */
    const double *om_arr;  /* [N] FIXCOMP, ZEVOL: Omega(lum_i, z_i) at fixed completeness (:235)  */
    const double *omega0;  /* [nf] effective areas in sq arcsec, as configured (float).  The
                              library applies the reference's int truncation for the per-source
                              term (:285) and uses the float value in the integral (:375).       */
    const double *logL;    /* [S*S] row-major [j][k]: j = luminosity index, k = redshift index;
                              the ONE grid every field integrates on (self.logL[-1], :225-232)    */
    const double *zarr;    /* [S]                                                    self.zarr  */
    const double *volume_part; /* [S] FREE: dVc/dz/dOmega at zarr                   (:223)      */
    const double *dl_zarr; /* [S] FREE: DLf(zarr) in Mpc                             (:222)      */
    const double *integ_part;  /* [nf*S*S] FIXCOMP, ZEVOL: volume_part * Omegaf[f].ev (:233-234) */
    const double *flim0;   /* [nf] FIXCOMP: the fixed Flim (prior still tests them, :346-351)   */
    double alpha0;         /* FIXCOMP: the fixed completeness slope                             */
    double sch_al0;        /* value of alpha when fix_sch_al                                    */
    double fcmin;          /* modified-Fleming knee, VmaxLumFunc.py:95 (0 < fcmin < 1)          */
    double lims[5][2];     /* prior boxes, rows LF_LIM_*                                        */
    double pivots[3];      /* ZEVOL: z1, z2, z3                      lumfuncmcmc_z.py:125       */
    int32_t device;        /* HIP device ordinal                                                */
    int32_t max_batch;     /* rows the workspace is sized for up front (grown on demand); 0 = 1024 */
} lf_desc;

typedef struct lf_ctx lf_ctx;

/* ABI version of the loaded library (== LF_ABI_VERSION of the header it was built from). */
int lf_abi_version(void);

/* Host-only helper behind lf_free's deal of its chunks to its 32 virtual workgroups, exported so that
 * the CPU tests can check it: table[0 .. 32] = where rank r's cell chunks start in the list, table[33 .. 65] the same for its
 * flux bins, then the list (cell chunks rank by rank, then bins rank by rank).  table = NULL: returns the number of ints
 * (66 + n_cell_chunks + n_bins); else fills `table` (cap ints) and returns that number.  grid_part / grid_parts as in the
 * "grid_share" option (0, 0: the whole grid). */
int lf_deal_table(int n_cell_chunks, int n_bins, int grid_part, int grid_parts, int32_t *table, int64_t cap);

/* ... and who finishes a tile of lf_free's polling hand-over under that deal: ranks[g] = the physical
 * rank, among the 8 (g + 1) workgroups that serve a tile, with the largest dealt cost (rank r serves the virtual ranks r,
 * r + 8 (g + 1), ...; a bin this share integrates costs 8, a cell chunk 3, the ranks of the group's younger half start 8
 * behind; ties go to the highest rank). */
int lf_deal_finishers(int n_cell_chunks, int n_bins, int grid_part, int grid_parts, int32_t ranks[4]);

/* Replaces the read side of LumFuncMCMC.__init__ / LumFuncMCMCz.__init__ (lumfuncmcmc.py:162-177):
 * copies the catalogue and grids to HBM, derives the parameter-independent per-source and
 * per-node tables.  Returns NULL on failure; lf_last_error(NULL) then holds the reason.
 * What is derived here, beyond the reference's arrays: the catalogue's cells (option "cells" of lf_set_option); for
 * fixed completeness the integration grid summed over its rows when every redshift column has the same luminosity
 * nodes; for the z-evolving model the grid stored column by column.  Two environment variables, read here, switch
 * the last two off for A/B tests - LF_NO_COLLAPSE_GRID, LF_NO_ZGRID_COLS (results agree to rounding either way);
 * LF_DEBUG_OCC prints the occupancy of a kernel instantiation at its first launch. */
lf_ctx *lf_create(const lf_desc *desc);

/* Releases device and host memory of the context. */
void lf_destroy(lf_ctx *ctx);

/* Number of free parameters of the variant (pos.shape[1] at lumfuncmcmc.py:485). */
int lf_ndim(const lf_ctx *ctx);

/* Replaces B serial calls of lnprob / lnprob_fix_comp (lumfuncmcmc.py:395, :411;
 * lumfuncmcmc_z.py:378).  theta: host, [B][ndim] row-major.  out: host, [B].
 * out[i] = -INFINITY where the prior fails or the likelihood underflows; never NaN.
 * Synchronous.  Returns LF_OK or a negative code. */
int lf_lnprob_batch(lf_ctx *ctx, const double *theta, int B, double *out);

/* Same, with theta and out in device memory of ctx's device and the launches enqueued on
 * `hip_stream` (a hipStream_t, NULL = the default stream).  Asynchronous: `out` is complete when
 * the stream reaches this point.  This is the form the multi-GPU path uses (the per-rank slice of
 * lnprob feeds the RCCL all-gather without a host round trip). */
int lf_lnprob_batch_device(lf_ctx *ctx, const double *d_theta, int B, double *d_out, void *hip_stream);

/* K evaluations in one call: block k is theta rows d_theta[k B ndim ..] -> d_out[k B ..], k = 0 .. K-1, enqueued back to back
 * on `hip_stream` (what K calls of lf_lnprob_batch_device enqueue, without K trips through the caller's language: a Python
 * caller spends 7 us per call, this loop 2-3 us per evaluation; the evaluations themselves take 8-21 us each).  For callers
 * with many independent half-ensembles to evaluate (several chains, a tempering ladder); emcee's stretch move itself
 * (lumfuncmcmc.py:489-491) needs block k's result before it can propose block k + 1 - that loop is lf_sampler_run's. */
int lf_lnprob_batch_device_n(lf_ctx *ctx, const double *d_theta, int B, int K, double *d_out, void *hip_stream);

/* Diagnostics for parity tests: the two pieces of lnlike separately (host buffers).
 * outA[i] = per-source log-term sum (lumfuncmcmc.py:370 / :388 / lumfuncmcmc_z.py:371),
 * outB[i] = expected-count integral (:373-377 / :389-392 / _z:373-375).  Rows failing the prior
 * get NaN in both.  Synchronous. */
int lf_lnprob_pieces(lf_ctx *ctx, const double *theta, int B, double *outA, double *outB);

/* The gradient of lnprob = A - B (the two pieces above) with respect to the row's own theta elements, in theta's own units
 * (csrc/lf_grad.h): grad[B][ndim] row-major.  lnprob: [B] or NULL; where given it is what
 * lf_lnprob_batch returns for the same rows, bit for bit (the same path runs first).  A row whose lnprob is -INFINITY (outside
 * the prior, or underflow) gets NaN in every element of its gradient; every other row finite values.  A row's gradient has the
 * same bits whatever B is and wherever the row stands in the batch.  The option "compress" is ignored (the gradient always
 * comes from the real catalogue); a context with "skip_grid" or "grid_share" set gets LF_ERR_ARG (source-sharded gradients are
 * not provided).  Host pointers, synchronous. */
int lf_lnprob_grad_batch(lf_ctx *ctx, const double *theta, int B, double *lnprob, double *grad);

/* Same, with device pointers and the launches enqueued on `hip_stream` (NULL = the default stream), asynchronous like
 * lf_lnprob_batch_device.  d_lnprob may be NULL. */
int lf_lnprob_grad_batch_device(lf_ctx *ctx, const double *d_theta, int B, double *d_lnprob, double *d_grad, void *hip_stream);

/* The flux-error-convolved likelihood (Eddington-bias correction; csrc/lf_deconv.h).  The catalogued
 * log-luminosity of source i is its true one plus Gaussian noise of sigma[i] dex (the source's lum_e), and the completeness acts
 * on the true flux: the expected counts (piece B) are unchanged, and each per-source term ln[phi(L_i) Omega(L_i, z_i)] becomes
 * ln of its convolution with N(0, sigma_i^2), by K-point Gauss-Hermite quadrature.
 * lf_set_lum_err copies sigma[N] (catalogue order, as given to lf_create; the context's own order is applied here) to the device.
 * K: 4, 6, 8, 10, 12, 16, 20, 24 or 32.  Each order is validated (per-source quadrature error below 1e-7 over the prior box's
 * sharpest completeness, tests/test_deconv_cpu.py) up to a largest sigma: 0.01, 0.03, 0.04, 0.05, 0.06, 0.06, 0.07, 0.08, 0.09
 * dex; a larger sigma is refused with a message that states the limit, unless option "deconv_unchecked" = 1 was set before
 * (tests and A/B runs: the value is then the K-point sum, whatever its distance from the integral).
 * FIXCOMP, ZEVOL: logf[N] = log10 of the sources' fluxes (erg cm^-2 s^-1; lum - log10(4 pi DL^2), the FREE variant's
 * lf_desc.logf), flim0[nf] (1e-17 erg cm^-2 s^-1) and alpha0 = the fixed completeness om_arr was made with; FREE: ignored
 * (NULL; the row's own Flim_f and alpha_C are used, and the context has the fluxes).
 * LF_ERR_ARG with a message, nothing uploaded, for: a NULL sigma, a sigma that is not finite or < 0 or above the order's limit,
 * an unsupported K, missing logf / flim0 (FIXCOMP, ZEVOL), and a context whose grid has its own luminosity nodes per redshift
 * column (min_comp_frac > 0.001: a cut on the observed flux would change piece B).  May be called again (synchronises). */
int lf_set_lum_err(lf_ctx *ctx, const double *sigma, int K, const double *logf, const double *flim0, double alpha0);

/* lnprob + Delta for B rows, Delta = sum_i ln sum_k (w_k / sqrt(pi)) exp(t_ik - t_i).  The plain lnprob is computed first by
 * the path of lf_lnprob_batch, bit for bit; a row whose lnprob is -INFINITY stays -INFINITY, NaN becomes -INFINITY; a source
 * with sigma = 0 contributes exactly 0 (all sigma 0: the output is lf_lnprob_batch's, bit for bit).  The correction is summed
 * in one fixed order without atomics: a row's value has the same bits whatever B is and wherever the row stands.  The option
 * "compress" is ignored by the correction.  Option "deconv_tile" = 1 (default 0; FIXCOMP, ZEVOL): the correction's first stage
 * takes a tile of 8 rows per block and makes what depends on the source and the node only once for them
 * (csrc/lf_deconv_tile.h): the same guarantees, values within rounding of the default's; accepted and
 * without effect on a FREE context, and ignored by the gradient entries below.  LF_ERR_ARG with a message, before the device
 * is touched, when no errors are set and for a context with "skip_grid" or "grid_share" set.  Host pointers, synchronous. */
int lf_lnprob_err_batch(lf_ctx *ctx, const double *theta, int B, double *out);

/* Same, with device pointers and the launches enqueued on `hip_stream` (NULL = the default stream), asynchronous like
 * lf_lnprob_batch_device. */
int lf_lnprob_err_batch_device(lf_ctx *ctx, const double *d_theta, int B, double *d_out, void *hip_stream);

/* The convolved lnprob of lf_lnprob_err_batch and its gradient with respect to the row's own theta elements, in theta's own
 * units (csrc/lf_deconv_grad.h): grad[B][ndim] row-major = the gradient of lf_lnprob_grad_batch plus the
 * exact derivative of the K-point sum Delta (its phi* elements are exactly 0).  lnprob_err: [B] or NULL; where given it is what
 * lf_lnprob_err_batch returns for the same rows, bit for bit (the same kernels run on the same plain lnprob).  A row whose plain
 * lnprob is not finite gets NaN in every element of its gradient; a source with sigma = 0 adds exactly 0.  No atomics: a row's
 * gradient has the same bits whatever B is and wherever the row stands.  The option "compress" is ignored.  LF_ERR_ARG with a
 * message, before the device is touched, for a NULL theta or grad or B <= 0, when no errors are set, and for a context with
 * "skip_grid" or "grid_share" set; the context stays usable.  Host pointers, synchronous. */
int lf_lnprob_err_grad_batch(lf_ctx *ctx, const double *theta, int B, double *lnprob_err, double *grad);

/* Same, with device pointers and the launches enqueued on `hip_stream` (NULL = the default stream), asynchronous like
 * lf_lnprob_batch_device.  d_lnprob_err may be NULL. */
int lf_lnprob_err_grad_batch_device(lf_ctx *ctx, const double *d_theta, int B, double *d_lnprob_err, double *d_grad, void *hip_stream);

/* Host-only, exported for tests (touches no GPU): the K-point Gauss-Hermite rule (weight e^(-x^2)) the library derives in
 * extended precision: x[K] ascending, lnw[K] = ln(w_k / sqrt(pi)).  LF_ERR_ARG for a NULL pointer or K outside 2..64. */
int lf_gauss_hermite(int K, double *x, double *lnw);

/* Host-only: the supported orders and the largest sigma each is validated for (up to cap entries; either may be NULL), the
 * default order and the sources per chunk of the correction's fixed summation order.  Returns the number of orders. */
int lf_deconv_info(int32_t *orders, double *sigma_max, int cap, int *default_order, int *chunk);

/* The wide rule (csrc/lf_deconv_wide.h): option "deconv_wide" = 1 (default 0), set BEFORE lf_set_lum_err.
 * Without it nothing changes: sigma above the order's limit is refused (or, with "deconv_unchecked", summed by the order as it
 * is).  With it lf_set_lum_err accepts sigma up to 0.30 dex and refuses larger values with that limit in the message.  A source
 * at or below the order's limit keeps the Gauss-Hermite sum and its bits (no source above it: every result is the one without
 * the option, bit for bit).  A source above it falls into a sigma class (upper edges 0.10, 0.15, 0.20, 0.25, 0.30 dex: the
 * first edge that is not below its sigma) and is integrated by that class's composite Gauss-Legendre rule - panels of 8 nodes,
 * at most 0.25 dex wide, over +-7.5 sigma; 48 to 144 nodes; per-source error below 1e-7 - by kernels of their own whose partial
 * sums enter the same fixed-order second stages: every entry above and both device samplers take it, and a row's bits still
 * depend neither on B nor on its position.  With "deconv_tile" the narrow part is tiled, the wide part is not.  Still refused:
 * source-sharded contexts and min_comp_frac > 0.001.
 * lf_deconv_wide_info: host-only (touches no GPU).  The classes' upper edges and node counts (up to cap entries), the sources
 * per wide chunk, T, the nodes per panel and the widest panel h in dex - any of them may be NULL; with x and lnw the table of
 * class cls in the kernels' form (x_k with delta = sqrt(2) sigma x_k, and the log of the whole weight, the Gaussian density
 * included; nodes[cls] entries each).  Returns the number of classes; LF_ERR_ARG when only one of x, lnw is given or cls is not
 * a class. */
int lf_deconv_wide_info(double *edges, int32_t *nodes, int cap, int *chunk, double *T, int *npanel, double *h, int cls, double *x,
                        double *lnw);

/* The per-source posterior of the TRUE log-luminosity under the convolved model (csrc/lf_lumpost.h),
 * marginalised over R rows of theta: for source i with sigma_i > 0 and row r the nodes delta_k = sqrt(2) sigma_i x_k of the
 * source's rule (the order of lf_set_lum_err, or its wide class under "deconv_wide") carry the weights p_k proportional to
 * exp(ln w_k + t_ik - t_i), the terms of lf_lnprob_err_batch, and
 *     m1[i] = mean over the used rows of sum_k p_k delta_k,   m2[i] = mean of sum_k p_k delta_k^2      (dex, dex^2)
 * in the CALLER's source order: the true value is lum_i + m1[i], its spread sqrt(max(m2[i] - m1[i]^2, 0)).  A row is used when
 * its plain lnprob (lf_lnprob_batch's) is finite; *n_used = R', their number.  A source with sigma_i = 0 gets exactly 0 and 0;
 * with R' = 0 every source with sigma_i > 0 gets NaN.  theta[R][ndim], m1[N], m2[N]: host pointers; synchronous; 1 <= R <= 4096.
 * The summation order is fixed (rows in row order inside tiles of row_tile rows, the tiles' sums in tile order, then one
 * division) and there are no atomics: the same inputs give the same bits, and R = 1 gives that row's own moments exactly.  The
 * workspace does not depend on R.  LF_ERR_ARG with a message, before the device is touched, for a NULL pointer, R outside
 * 1..4096, when no errors are set, and for a context with "skip_grid" or "grid_share" set; the context stays usable.
 * lf_lum_posterior_info: host-only; the rows of a tile and the largest R (either may be NULL). */
int lf_lum_posterior(lf_ctx *ctx, const double *theta, int R, double *m1, double *m2, int *n_used);
int lf_lum_posterior_info(int *row_tile, int *max_rows);

/* The deconvolved 1/Veff points (csrc/lf_vefftrue.h): the sources' posteriors of the TRUE luminosity
 * (lf_lum_posterior's node weights p_irk) binned in luminosity with the completeness at the node's TRUE flux, per row of theta,
 *     values[r][b] = sum_i sum_k [edges[b] <= lum_i + dl_ik < edges[b + 1]] p_irk / (pref0 fc(f_i 10^dl_ik) vol),
 * dl_ik = (sqrt(2) sigma_i) x_k (one rounded product, one rounded add), the bin of a node searchsorted(edges, L, "right") - 1,
 * nodes outside [edges[0], edges[nbin]) dropped; a source with sigma_i = 0 is one node at dl = 0 with p = 1 (lf_veff_draws'
 * term).  FREE takes the row's Flim_f and alpha_C, FIXCOMP and ZEVOL those of lf_set_lum_err.  A row is used when its plain
 * lnprob is finite: *n_used = R'; an unused row gets NaN in values; out[nq][nbin] holds NumPy's percentiles (method, q: as
 * lf_lumfunc_quantiles) of every bin over the R' used rows, NaN when R' = 0.  theta[R][ndim], edges[nbin + 1], out, values
 * (may be NULL): host pointers; synchronous.  No atomics and one fixed order of summation: the same inputs give the same bits,
 * and a row's values do not depend on R, on its place in the batch or on the other rows; the workspace does not grow with R
 * (the rows run in groups of lf_veff_true_info's return value).  LF_ERR_ARG with a message, before the device is touched, for a
 * NULL required pointer, R outside 1..4096, nbin outside 1..1024, edges not finite and strictly ascending, pref0 <= 0 or
 * vol <= 0, a bad nq, q or method, when no errors are set, and for a context with "skip_grid" or "grid_share" set; the
 * context stays usable.
 * lf_veff_true_info: host-only; the largest R and nbin (either may be NULL); returns the rows of a launch group.
 * lf_veff_true_ms: the device times of the last successful call's stages - the node kernel, the chunk sums, the quantiles
 * (hipEvents; summed over the groups); LF_ERR_ARG when there is none. */
int lf_veff_true(lf_ctx *ctx, const double *theta, int R, const double *edges, int nbin, double pref0, double vol, int nq,
                 const double *q, int method, double *out, double *values, int *n_used);
int lf_veff_true_info(int *max_rows, int *max_bins);
int lf_veff_true_ms(double ms[3]);

/* The convolved likelihood under a cut on the OBSERVED flux (csrc/lf_deconv_cut.h): contexts whose grid
 * has its own luminosity nodes per redshift column (min_comp_frac > 0.001).  A source is catalogued when its observed
 * luminosity L_o = L_t + eps, eps ~ N(0, s^2), lies at or above the grid's lower edge Lam(z) = logL[0][.]; s = sigma_f(log10 of
 * the TRUE flux) is field f's error model: linear between nodes[M] (log10 flux, increasing), constant outside, sigma[nf][M] in
 * dex (the mocks' model, lf_mock_set_error_model).  The expected counts become B + Delta B,
 *     Delta B = sum_f sum_j wz_j V_j [ int_{Lam-H}^{Lam} phi Omega Q(-u) dL - int_{Lam}^{min(Lam+H, Lh)} phi Omega Q(u) dL ],
 *     u = (L - Lam_j) / s_f(L - ld2_j),  Q(x) = erfc(x / sqrt 2) / 2,  H = 7.5 max_m sigma[f][m],
 * and every value entry of the convolved likelihood (lf_lnprob_err_batch, _device, both device samplers' convolved likelihood,
 * with "deconv_tile" and "deconv_wide") returns lnprob + Delta - Delta B; the per-source term keeps the catalogued sigma_i.
 * The nodes and whole weights (u does not depend on theta) are host tables in extended precision: panels of 8 Gauss-Legendre
 * nodes laid from the edge outwards, no wider than 2.5 x the smallest sigma on them, 0.25 dex, and the distance to the next
 * node of the error model; per (field, column) the error against the integral is below 1e-7 of the column's plain integral
 * for sigma up to 0.30 dex.  Without this call nothing changes.
 * lf_set_cut_error_model: BEFORE lf_set_lum_err, which then accepts such a context (FIXCOMP, ZEVOL: and makes the tables, with
 * the completeness flim0, alpha0 it is given folded in; the descriptor of such a context must also hold volume_part and
 * dl_zarr).  LF_ERR_ARG with a message for: NULL pointers, M outside 1..64, nodes not finite or not increasing, sigma not
 * finite, < 0 or above 0.30 dex (the limit is stated), a field whose sigma is 0 at some nodes only, a model that needs more
 * than 64 panels on one side of the edge, a context without the cut (separable grid), a source-sharded context, and a call
 * after lf_set_lum_err.  Still refused on such a context, with what is missing in the message: lf_lnprob_err_grad_batch(_device)
 * (the gradient of Delta B; served with the option "deconv_cut_grad", below) and lf_veff_true (per-source volumes; served
 * with the option "deconv_cut_veff", below, by the catalogued volume per node);
 * lf_lum_posterior is served (a source's posterior given that it is catalogued does not involve B).
 * lf_cut_term_batch: Delta B alone for B rows (host pointers, synchronous; after lf_set_lum_err); NaN for a row whose plain
 * lnprob is not finite.  Summed in one fixed order without atomics: a row's bits do not depend on B or on its place.
 * lf_cut_info: the nodes per field and H per field (up to cap entries; either may be NULL), the nodes per block and the number
 * of blocks per row (-1 before the tables are made); returns nf.  FIXCOMP, ZEVOL: until lf_set_lum_err has made the tables the
 * node counts are those of the placement alone; a node whose weight underflows with the completeness folded in is dropped
 * then, so they may shrink.  Option "deconv_cut_limit" = n > 0, set before the tables are
 * made (tests): only the first n nodes of every field are kept. */
int lf_set_cut_error_model(lf_ctx *ctx, const double *nodes, int M, const double *sigma);
int lf_cut_term_batch(lf_ctx *ctx, const double *theta, int B, double *out);
int lf_cut_info(lf_ctx *ctx, int32_t *nnodes, double *H, int cap, int *chunk, int *chunks);

/* The gradient of Delta B (csrc/lf_deconv_cut_grad.h).  u does not depend on theta, so -Delta B =
 * sum_n c_n phi_theta(L_n[, z_j]) [fc^(1/d)_theta: FREE] over the tables above, and its derivatives are those of the expected
 * counts' lattice nodes with c_n as the weight: per node I_n times ln10 (10^x - alpha - 1), ln10, ln10 x (x = L_n - L*) for L*,
 * phi*, alpha (z-evolving: times the Lagrange basis for L_m, phi_m), and for FREE I_n dF_n / Flim_f (the field's nodes only) and
 * I_n dC_n.  First stage: lf_cut_term_batch's grid, chunks and node order, one running sum per element kind, the block's tail
 * as there; second stage: one wave per row, lane l adds chunks l, l + 64, ..., then the shuffle tree.  No atomics: a row's bits
 * do not depend on B or on its place.
 * Option "deconv_cut_grad" (lf_set_option; default 0): with 1, lf_lnprob_err_grad_batch and _device serve a context with the
 * cut model - the value is lf_lnprob_err_batch's, bit for bit (lnprob + Delta - Delta B), and every gradient element is the
 * plain one, plus Delta's, plus that of -Delta B, added in that order; rows whose plain lnprob is not finite: NaN.  With 0 the
 * two entries refuse such a context as before.  Without a cut model the option does nothing; with a cut model of sigma = 0
 * (no nodes) nothing more is launched.  It may be switched between calls.
 * lf_cut_term_grad_batch: Delta B [B] and d Delta B / d theta [B][ndim] for B rows (host pointers, synchronous; after
 * lf_set_lum_err; whatever the option says).  out is lf_cut_term_batch's, bit for bit; a row whose plain lnprob is not finite
 * has NaN in out and in every element. */
int lf_cut_term_grad_batch(lf_ctx *ctx, const double *theta, int B, double *out, double *grad);

/* The deconvolved 1/Veff points under the cut: the catalogued volume per node (csrc/lf_vefftrue_cut.h).
 * Under the cut a true luminosity L of field f is catalogued in the part
 *     g_f(L) = (sum_j wv_j Q(-u_fj(L))) / (sum_j wv_j),  wv_j = wz_j V_j,  u_fj = (L - Lam_j) / s_f(L - ld2_j)
 * of the survey volume (all S columns, the grid and the error model of lf_set_cut_error_model), and node k of source i gets the
 * weight p_irk / (pref0 fc vol g_f(i)(L_ik)).  The sum: columns left to right, no fma contraction; u > 9: a term of exactly
 * wv_j; u < -9: exactly 0; else wv_j 0.5 erfc(-u / sqrt 2); a field whose sigma is 0 at every node: wv_j when L >= Lam_j.  g does
 * not depend on theta: 1 / g is tabulated once per (source, node) at the first call after lf_set_lum_err - 8 bytes per slot, N K
 * for the sources of the Gauss-Hermite order and 144 per source of the wide list (256 MB at 1e6 sources and K = 32) - and kept
 * until lf_set_lum_err, lf_set_cut_error_model or another min_vol_frac; LF_ERR_NOMEM with the size in the message when the
 * table cannot be allocated.  A node with g = 0 or g < min_vol_frac adds exactly 0 to every bin.
 * Option "deconv_cut_veff" (lf_set_option; default 0): with 1, lf_veff_true serves a context with the cut model (min_vol_frac
 * = 0); with 0 it refuses such a context as before.  Without a cut model the option does nothing: lf_veff_true's bits.
 * lf_veff_true_cut: lf_veff_true with min_vol_frac in 0..1 (> 0 only with a cut model); the same host function, the same
 * refusals under the entry's own name.
 * lf_veff_true_cut_info: the table's (source, node) slots, its bytes, and how many nodes were dropped (any may be NULL);
 * LF_ERR_ARG before a table is made.  lf_veff_true_cut_ms: the device time of the kernel that last made the table (hipEvents).
 * lf_cut_volume: g for n caller points (field[n] in 0..nf-1, L[n] finite; host pointers, synchronous; 1 <= n <= 2^24), by the
 * device function the table is made with; needs lf_set_cut_error_model only. */
int lf_veff_true_cut(lf_ctx *ctx, const double *theta, int R, const double *edges, int nbin, double pref0, double vol,
                     double min_vol_frac, int nq, const double *q, int method, double *out, double *values, int *n_used);
int lf_veff_true_cut_info(lf_ctx *ctx, int64_t *slots, int64_t *bytes, int64_t *dropped);
int lf_veff_true_cut_ms(lf_ctx *ctx, double *ms);
int lf_cut_volume(lf_ctx *ctx, const int32_t *field, const double *L, int64_t n, double *g_out);

/* Kernel timing for bench.py: level 1 brackets lf_main, level 2 every launch, with hipEvents on
 * the stream the launch runs on (0 = off; each event pair costs a few microseconds of stream time: the events are
 * barrier packets, and the next launch no longer overlaps the previous one's tail - measured 7.6 us per evaluation
 * of 40 at level 1.  Option "profile_every" = n brackets only every n-th evaluation).  lf_kernel_times reads and clears the accumulated totals:
 * ms[0..3] = {lf_prepare, lf_main (per-source sum + grid integral, one launch), unused (0), lf_finalize},
 * launches[0..3] the launch counts.  Synchronises the recorded events. */
int lf_set_profiling(lf_ctx *ctx, int level);
int lf_kernel_times(lf_ctx *ctx, double ms[4], int64_t launches[4]);

/* Tuning knobs (performance only, never results beyond summation order):
 * key "geometry": index of the launch geometry (sources per lane x walkers per workgroup),
 * -1 = chosen from N and B; "walker_tile": walkers per workgroup, 0 = the geometry's;
 * "taper": 1 gives the last ~B/8 walkers quarter-size tiles, dispatched last, so that the launch drains evenly
 * (bitwise neutral: a tile only decides which workgroup owns a (chunk, walker) sum); +1 % at N = 1e6 but the tail
 * tiles read the catalogue a second time (L2 -> fabric traffic 37 MB instead of 21 MB per launch): off by default.
 * "compress": 1 = take piece A from the COMPRESSED CATALOGUE (FREE, ZEVOL; off by default; never the headline path): the
 * ~N sources of a field are replaced by K = 16 weighted pseudo-sources per bin of the one coordinate the walker-dependent
 * factor of a term depends on (log flux; redshift).  Bins are halved until an ESTIMATE of the relative error of every
 * bin sum is below 1e-16; the estimate is evaluated at sampled walkers of the prior box (FREE: 7 slopes alpha_C x up to
 * 96 shifts of the flux limit, 33 points per bin; ZEVOL: the 8 corners of the (L1, L2, L3) box) - a sampled validation,
 * NOT a bound proven over the whole box (csrc/lf_compress.h).  In addition a freshly built compressed catalogue must
 * reproduce the direct path to 1e-12 on 64 walkers drawn from this context's prior box, or the option is refused
 * (LF_ERR_ARG).  lnprob then costs the grid integral plus a few hundred terms, whatever N is.  Walkers that need the
 * per-source underflow checks are still summed over the real catalogue.  Built at the first call with value 1.
 * With it, FREE contexts whose integration grid is separable (every redshift column has the same luminosity nodes:
 * min_comp_frac = 0) also take piece B over ~40 x 16 shared flux nodes per field instead of the S^2 lattice points
 * (same sampled validation; "compress_grid" = 0 keeps the full grid).
 * "tables": 1 (default) lets the free variant evaluate the term as the product of two tabulated univariate factors,
 * g(num) = ln fc and h(y) = 1 / (1 - e^(-10^y)) (piecewise degree-7 polynomials, relative error <= 8e-15 over their
 * whole domain, lf_tables.h), for (walker, chunk) pairs whose fluxes lie inside the tables and whose lanes of
 * flux-neighbours are narrower than the tables' margins; 0 = always the general form (A/B runs).
 * "persistent": 1 (default) runs the direct path in the persistent kernels - 512-thread workgroups, two per CU, that
 * hold the tables in LDS and serve one tile of 8 walkers per group of workgroups: lf_free (free completeness: whenever
 * the context has cells - every catalogue up to 65 536 sources and every larger one with at least four sources per
 * cell - or else when catalogue and grid give every workgroup about four chunks) and lf_pers (fixed completeness
 * always; z-evolving when the context has cells in redshift, one set of L nodes per redshift column and at most 256
 * columns); 0 = always lf_main; 2 = always the persistent kernel (tests).  "free_st": sources per lane of lf_free, 0 (auto: 8
 * for N >= 3e5, else 4), 2, 4 or 8 (tuning runs).  "cells": 1 (default) lets lf_free sum a walker whose every field lies inside the tables over the
 * catalogue's CELLS instead of its sources: runs of flux-neighbouring sources no wider than 2 rho, kept as their
 * midpoint and power sums S_0 .. S_8; on a table piece the term is a polynomial in the flux offset, so a cell's sum is
 * a dot product of its Taylor coefficients with the power sums, exact up to the orders above 8, whose share is below
 * 2e-18 by the choice of rho (from the prior box's largest alpha_C).  The z-evolving variant has cells too, in
 * redshift: what is left of its term per source is a weight times exp of a parabola in z, summed as a series in the
 * weighted power sums of a run of redshift neighbours (orders above 6 below 1e-17; the cells' width is chosen from the
 * prior box of L1..L3 so that every walker inside it qualifies).  0 = every walker over the sources (A/B runs).
 * "fuse": 1 (default) lets lf_free / lf_pers do lf_prepare's and lf_finalize's work themselves for plain evaluations -
 * one launch instead of three, same bits; 0 = three launches (A/B runs; lf_lnprob_pieces, the census, profiling level 2
 * and the walker-sharded sampler's halves always take three).  "fuse_step": 1 (default) makes a half-step of the
 * device-resident sampler ONE launch of the same kernels (proposal in the prologue, accept / reject and the chain's row
 * by the tile's finishing workgroup); 0 = lf_propose+prepare, kernel, lf_finalize+accept (same chain, bit for bit).
 * "poll": 1 (default) lets a tile of the one-launch form whose walkers need no per-source sums (the normal case) hand its
 * partial sums over by POLLING: every slot of the partial-sum buffers is kept at a reserved NaN pattern between launches,
 * a workgroup writes its sums through and is done, and the tile's finishing workgroup reads the slots until none is
 * empty (at most 2^19 times: then it writes NaN and lf_lnprob_batch returns LF_ERR_HIP); 0 = every tile counts its
 * workgroups (store, wait for the acknowledgement, atomic counter; A/B runs).  Same sums in the same order: same bits.
 * "profile_every": see lf_set_profiling.  "profile_span": n > 1 puts ONE event pair around n consecutive one-launch
 * evaluations (profiling level 1) instead of a pair around a single launch, and lf_kernel_times counts n launches for it:
 * a pair of barrier packets around one 13-us launch adds its dispatch to the figure (16.6 us where the profiler says 13.7).
 * "grid_shortcut": 1 (default) lets lf_free take piece B of a FREE context whose integration grid is separable (every
 * redshift column has the same luminosity nodes: min_comp_frac = 0) over FLUX BINS instead of the S^2 lattice points: the
 * completeness depends on a lattice point only through its log flux L_j - D_k, so per bin the lattice points of a row are
 * replaced by the bin's 64 Chebyshev nodes with weights from the row's moments (exact for polynomials of degree < 64),
 * and the Schechter factor of the rows enters by a dot product.  The bins are made at lf_create such that the
 * interpolation error of the completeness curve is PROVEN (Bernstein-ellipse bound, evaluated for the whole prior box
 * of alpha_C and Flim - csrc/lf_gridbound.h, tests/test_gridbound_cpu.py) to be below 1e-15 of the curve's smallest
 * value in the bin + 1e-30: |piece B (bins) - piece B (lattice)| <= 1e-15 piece B + 1e-30 x (piece B at completeness 1).
 * 16-20 bins x 64 nodes per field instead of 10 201 lattice points.  No proven set of bins (a prior box that reaches
 * alpha_C <= 0, a grid that is not separable) = the lattice; 0 = the lattice (A/B runs).
 * "specialise": 1 (default) lets the free variant take the cheaper form of the term for (walker, chunk) pairs whose
 * every source has f / f_tau > 37.5 (decay factor exactly 1.0 in binary64); 0 = always the general form (A/B runs).
 * Two keys change what is computed, for SOURCE-SHARDED ranks whose lnprob values are summed (all-reduce): "skip_grid" = 1
 * leaves the expected-count integral (piece B) out of lnprob altogether; "grid_share" = part + 65536 * parts makes this
 * context integrate only the node chunks c with c % parts == part, so that the ranks split piece B as well as piece A. */
int lf_set_option(lf_ctx *ctx, const char *key, int64_t value);

/* Census of which form of the per-source term / grid node ran since lf_set_option(ctx, "count_forms", 1) (which also
 * clears it; 0 switches it off again - it costs one atomic per (walker, chunk), so it is off by default).  For
 * bench.py's executed-flop accounting and the tests.  counts[0..8] = (walker, source) terms evaluated in the general
 * form, the general form without the exponential, the table-driven form, the table-driven form without the
 * exponential, the careful (checked) form, terms of walkers that were not evaluated (outside the prior / already
 * -inf); then (walker, node, field) terms of the grid integral in the general and in the bright form; then
 * (walker, cell) evaluations (option "cells": a cell stands for all the sources of a narrow flux interval).  FREE variant,
 * real catalogue.  The z-evolving variant counts its own: [8] (walker, cell in redshift) evaluations, [2] terms of its
 * local form (one exponential per lane of redshift neighbours), [0] per-source exponentials, [4] terms of the careful
 * form, [6] (walker, node) terms of its grid.  (The fixed-completeness variant and the compressed catalogue leave it at 0.)  Synchronises the device. */
int lf_form_counts(lf_ctx *ctx, int64_t counts[9]);

/* Shape of the most recent lf_main launch of this context (measurement only): info[0..7] = sources per lane, walkers
 * per source workgroup and per grid workgroup of the instantiation (template parameters ST, TW, TWB); which kernel ran
 * (0 lf_main, 1 its compressed-catalogue instantiation, 2 lf_free: the persistent kernel of the free variant, 3
 * lf_free in its one-launch form, see "fuse"; 4 lf_pers: the persistent kernel of the other two variants, 5 lf_pers in
 * its one-launch form);
 * workgroups in the launch, catalogue chunks, grid chunks, theta rows. */
int lf_last_launch(const lf_ctx *ctx, int32_t info[8]);

/* How many times this context has uploaded the one-launch lf_free's block of launch-invariant arguments (measurement and
 * tests only): once per sources-per-lane setting on first use, then only when a reallocated buffer or an option changes
 * its bytes - never in steady state. */
int lf_free_block_uploads(const lf_ctx *ctx, int64_t *n);

/*
 * Device-resident ensemble sampler: the Goodman & Weare stretch move in its parallel form (two fixed
 * half-ensembles, as emcee 2.x - the API the reference calls - implements it), with theta, lnprob
 * and the chain kept in HBM.  Replaces
 *     sampler = emcee.EnsembleSampler(nwalkers, ndim, lnprob); sampler.run_mcmc(pos, nsteps)
 *     sampler.chain, sampler.lnprobability, sampler.acceptance_fraction      lumfuncmcmc.py:489-513
 * One step = 2 half-steps of ONE launch each where the persistent kernels serve the context (option "fuse_step"),
 * else 2 x (propose+prepare, main, finalize+accept) = 6 launches; no host round trip either way.
 * Random numbers are Philox4x32-10 keyed by `seed`: the chain is a pure function of (seed, start).
 */
typedef struct lf_sampler lf_sampler;

/* `a` is the stretch scale (emcee default 2.0); capacity_steps sizes the on-device chain. */
lf_sampler *lf_sampler_create(lf_ctx *ctx, int nwalkers, double a, uint64_t seed, int64_t capacity_steps);
void lf_sampler_destroy(lf_sampler *s);
/* pos: host [nwalkers][ndim].  lnprob0: host [nwalkers] or NULL (then evaluated here).  Resets the chain. */
int lf_sampler_start(lf_sampler *s, const double *pos, const double *lnprob0);
/* Enqueue nsteps full ensemble steps on hip_stream (NULL = the context's stream).  Asynchronous. */
int lf_sampler_run(lf_sampler *s, int64_t nsteps, void *hip_stream);
/* Synchronise and copy out; any pointer may be NULL.  chain: [nwalkers][steps][ndim] (emcee's
 * sampler.chain layout), chain_lnprob: [nwalkers][steps], naccepted: [nwalkers], pos / lnprob: current state. */
int lf_sampler_read(lf_sampler *s, double *chain, double *chain_lnprob, int64_t *naccepted, double *pos, double *lnprob);
/* Steps recorded so far. */
int64_t lf_sampler_steps(const lf_sampler *s);
/* Walker-sharded form of one half-step (multi-GPU: one process per GPU, every rank holds the whole
 * ensemble).  half_eval proposes for the whole half (half = 0 or 1) and evaluates lnprob of the
 * proposals lo..hi-1 (indices within the half) into d_newlp[lo..hi-1] (device); the caller all-gathers
 * d_newlp over the ranks (RCCL); half_accept then accepts/rejects the whole half and records the chain
 * (after half 1 the step counter advances).  Both enqueue on hip_stream as given (NULL = the default
 * stream, as in lf_lnprob_batch_device), so that the collective in between is stream-ordered with them.
 * Same random numbers and arithmetic as lf_sampler_run: the chain is identical for any sharding. */
int lf_sampler_half_eval(lf_sampler *s, int half, int lo, int hi, double *d_newlp, void *hip_stream);
int lf_sampler_half_accept(lf_sampler *s, int half, const double *d_newlp, void *hip_stream);
/* Which likelihood the sampler's target is: convolved = 0 the plain lnprob (the default), 1 the flux-error-convolved one
 * (lf_lnprob_err_batch).  With 1 a half-step is lf_propose, the plain evaluation of the proposals,
 * the correction's kernels on them (per the context's option "deconv_tile") and lf_accept, all on the stream and without a
 * host round trip (the option "fuse_step" does not apply); lf_sampler_start with lnprob0 == NULL evaluates the convolved value
 * of the start; lf_sampler_half_eval / lf_sampler_half_accept follow the same setting.  The chain equals the host replay over
 * lf_lnprob_err_batch bit for bit.  Valid before lf_sampler_start, or between a start and the first step (a start whose
 * lnprob0 was NULL is evaluated again; one that was given has to be the chosen likelihood's): LF_ERR_ARG with a message
 * otherwise, and when no errors are set (lf_set_lum_err) or the context is source-sharded.  What the correction needs for the
 * sampler's rows is allocated here, not inside the running chain. */
int lf_sampler_set_likelihood(lf_sampler *s, int convolved);

/* Parallel-tempered device sampler (emcee 2.x's PTSampler: thermodynamic-integration evidence).
 * ntemps T <= 64 temperatures with inverse temperatures betas[0] == 1 > betas[1] > ... > betas[T-1] > 0, nwalkers W
 * (even, 2..4096) walkers each.  The prior is the context's flat box, so the tempered target at beta is beta * lnprob;
 * a step is, per half, the stretch move of all T x W/2 walkers at once (one evaluation of T x W/2 rows, accept on
 * lnq = (ln-z term + beta newl) - beta oldl), then the swaps between neighbouring temperatures from the hottest pair down,
 * then the chain's row.  Philox4x32-10 keyed by seed: temperature 0 draws the numbers lf_sampler_run draws, so T = 1
 * gives the ensemble sampler's chain bit for bit.  The sampler keeps untempered lnlike (= lnprob inside the box). */
typedef struct lf_ptsampler lf_ptsampler;
lf_ptsampler *lf_ptsampler_create(lf_ctx *ctx, int ntemps, int nwalkers, const double *betas, double a, uint64_t seed,
                                  int64_t capacity_steps);
void lf_ptsampler_destroy(lf_ptsampler *s);
/* pos: [T][W][ndim] host; lnlike0: [T][W] or NULL (evaluated then).  Every lnlike must be finite: LF_ERR_ARG otherwise.
 * Resets the chain and the counters. */
int lf_ptsampler_start(lf_ptsampler *s, const double *pos, const double *lnlike0);
/* Enqueue nsteps steps on hip_stream (NULL = the context's stream).  Asynchronous. */
int lf_ptsampler_run(lf_ptsampler *s, int64_t nsteps, void *hip_stream);
/* Synchronise and copy out; any pointer may be NULL.  chain: [T][W][steps][ndim], chain_lnlike: [T][W][steps],
 * mean_lnlike: [T][steps] (the mean of lnlike over the W walkers of a temperature after the step's swaps), naccepted:
 * [T][W] (stretch moves), nswap: [T-1] (entry i-1: swaps accepted between temperatures i and i-1), pos: [T][W][ndim],
 * lnlike: [T][W]. */
int lf_ptsampler_read(lf_ptsampler *s, double *chain, double *chain_lnlike, double *mean_lnlike, int64_t *naccepted,
                      int64_t *nswap, double *pos, double *lnlike);
/* Steps recorded so far. */
int64_t lf_ptsampler_steps(const lf_ptsampler *s);
/* lf_sampler_set_likelihood for the tempered sampler: with convolved = 1 the tempered target is beta x the
 * flux-error-convolved lnprob - the correction's kernels run between lf_pt_propose's plain evaluation and lf_pt_accept, and
 * lf_ptsampler_start with lnlike0 == NULL evaluates the convolved value.  The same validity and refusals. */
int lf_ptsampler_set_likelihood(lf_ptsampler *s, int convolved);

/* Chain diagnostics on the device (csrc/lf_diag.h).  Replace the read-back behind
 *     tau = np.max(sampler.acor); burnin_step = int(tau * 3), at most nsteps // 2          lumfuncmcmc.py:499-501
 * (emcee's acor: the whole chain on the host, one FFT pair per walker and parameter) by direct sums where the chain is.
 * A chain is [W][steps][ndim] (emcee's sampler.chain layout), optionally with its lnprob [W][steps] as one more series
 * (index ndim); the range is steps [t0, t1), n = t1 - t0.  Per series d, in this order of the D = ndim (+ 1) outputs:
 *   acf[d][k] = (1 / W) sum_w a_w[k] / a_w[0],  a_w[k] = sum_{t < n-k} y[t] y[t+k],  y = x - mean(x)  (a walker with a_w[0] <= 0 is
 *     left out of the sum) - the definition of the host's integrated_time, by direct summation in a fixed order: acf[d][k] has
 *     the same bits whatever number of lags is computed and whatever else is in the chain;
 *   tau[d], window[d]: taus[m] = 2 sum_{k <= m} acf[k] - 1, window = the first m with m >= c taus[m], tau = taus[window]; no
 *     window below n: n - 1; a tau that is not finite or not positive: 1.0; n < 4: tau 1.0, window 0;
 *   ess[d] = W n / tau[d];
 *   rhat[d] = split-R-hat (Gelman et al. 2013) over the 2 W half-ranges [0, n/2), [n - n/2, n) of the walkers; NaN for n < 4.
 *     The walkers of an ensemble are not independent chains: a sanity check, not a stopping rule.
 * LF_ERR_ARG, before the device is touched, for: a NULL pointer (lnprob, acf may be NULL), W < 1, ndim < 1, t0 < 0, t1 > steps,
 * t1 <= t0, c <= 0 or NaN, a sampler that has not been started (or has no step at or after t0), a temperature outside the ladder. */

/* Host pointers, synchronous, no context (the form of lf_veff): for chains of the host sampler and for tests.  acf: NULL, or
 * [D][acf_cap] - the first acf_cap lags of every series (zeros past n). */
int lf_chain_diag(int device, const double *chain, const double *lnprob, int W, int64_t steps, int ndim, int64_t t0, int64_t t1,
                  double c, double *tau, int64_t *window, double *ess, double *rhat, double *acf, int64_t acf_cap);
/* The same over steps [t0, lf_sampler_steps) of the sampler's own chain in HBM (with_lnprob != 0: and of its lnprob chain).
 * Synchronises the device; the chain is not copied to the host (per pass D x lags doubles are).  Changes no sampler state. */
int lf_sampler_diag(lf_sampler *s, int64_t t0, double c, int with_lnprob, double *tau, int64_t *window, double *ess, double *rhat);
/* The same for one temperature of the tempered sampler (with_lnlike != 0: and of its untempered lnlike chain). */
int lf_ptsampler_diag(lf_ptsampler *s, int temperature, int64_t t0, double c, int with_lnlike, double *tau, int64_t *window,
                      double *ess, double *rhat);
/* Host-only, exported for tests (touches no GPU): the window rule above on a given curve acf[0 .. M) of a series of n steps.
 * Returns 0 with *tau and *window set, 1 when no window lies below M and M < n (more lags are needed), LF_ERR_ARG for a
 * NULL pointer, n < 1, M < 1 (with n >= 4) or c <= 0. */
int lf_chain_window(const double *acf, int64_t M, double c, int64_t n, double *tau, int64_t *window);
/* Device time in ms of the kernels of the most recent successful diagnostics call in this process (hipEvents around every
 * bracket of launches) and the lags per series it computed (measurement only).  LF_ERR_ARG when there is none. */
int lf_diag_last(double *kernel_ms, int64_t *lags);

/* Host-only helper behind "compress", exported for tests (touches no GPU): compress n coordinates `key` with
 * weights `wt` (NULL = 1) into pseudo-sources.  kind 0 (FREE): params = {|a/(1-a)|, alpha_lo, alpha_hi, flim_lo,
 * flim_hi}; kind 1 (ZEVOL): params = {L_lo, L_hi, z1, z2, z3}.  Returns the number of pseudo-sources (written to
 * node / weight when it is <= cap), or a negative code; *bound = the largest accepted (sampled) error estimate. */
int64_t lf_compress_keys(int kind, const double *params, const double *key, const double *wt, int64_t n,
                         double *node, double *weight, int64_t cap, double *bound);

/* Host-only helper behind the compressed grid, exported for tests: S luminosity nodes L with trapezoid weights wL,
 * S redshift weights ck (trapezoid x dV/dz) and D_k = log10(4 pi DL_k^2); params as for kind 0 of lf_compress_keys.
 * Outputs per bin: 16 node positions u, first row row0, row count nrows, offset off into omega ([row][node], wL
 * folded in).  Returns the number of bins (outputs written when the capacities suffice), or a negative code. */
int64_t lf_compress_grid(const double *params, int S, const double *L, const double *wL, const double *ck,
                         const double *Dk, double *u, int32_t *row0, int32_t *nrows, int32_t *off, double *omega,
                         int64_t cap_bins, int64_t cap_omega, double *bound);

/* Host-only helper behind "grid_shortcut", exported for tests (touches no GPU).  Arguments as lf_compress_grid.  Outputs
 * per bin: edges[2], rec[64][4] = {node x_n, 10^(x_n + 17), L of row row0 + n (the last row again past the bin's rows),
 * 10^(that - 42)}, rows[4] = {row0, nrows, offset into omega, 0}, omega [row][64].  *margin = ln(proven error bound /
 * allowance) of the worst bin, <= 0.  Returns the number of bins (outputs written when the capacities suffice),
 * or a negative code when no proven set of bins exists. */
int64_t lf_grid_bins(const double *params, int S, const double *L, const double *wL, const double *ck, const double *Dk,
                     double *edges, double *rec, int32_t *rows, double *omega, int64_t cap_bins, int64_t cap_omega,
                     double *margin);

/* 1/Veff estimator on the device (post-fit diagnostic, no context needed).  Replaces the per-source loop of
 * LumFuncMCMC.VeffLF (lumfuncmcmc.py:515-525: V.lumfunc, one scipy.quad per source, VmaxLumFunc.py:235-257) and the
 * nboot x nbins masked sums of V.getBootErrLog (VmaxLumFunc.py:304-378).  All arrays host, length n unless noted.
 *   phi[i] = 1 / (pref0 * fleming(flux[i], flim[i], alpha, fcmin) * (vol ? vol[i] : vol_all)),  0 where the volume is <= 0
 *   (pref0 = sum(Omega_0) / sqarcsec; fcmin <= 0 = the unmodified Fleming curve);
 *   sums[(nboot + 1) * nbin]: row 0 = sum of phi per luminosity bin (bin_of[i] in [0, nbin), anything else = no bin),
 *   rows 1..nboot = the same over bootstrap resamples of the catalogue: indices from boot_idx[nboot * n] when given
 *   (a caller replaying a seeded host stream; every index must lie in [0, n): LF_ERR_ARG otherwise), else drawn on the
 *   device (Philox4x32-10 keyed by seed).
 * nbin = 0 skips the binning (bin_of, sums may be NULL).  nbin <= 1024.  Synchronous. */
int lf_veff(int device, int64_t n, const double *flux, const double *flim, const double *vol, double vol_all, double pref0,
            double alpha, double fcmin, const int32_t *bin_of, int32_t nbin, int32_t nboot, const int64_t *boot_idx, uint64_t seed,
            double *phi, double *sums);

/* The 1/Veff points in redshift slices with a bootstrap per slice (post-fit, no context needed; csrc/lf_veffslices.h, DESIGN.md
 * section 3.36) - the device form of VmaxLumFunc.zEvolSteps (VmaxLumFunc.py:611-660).  All arrays host, length n unless noted.
 *   phi[i] = 1 / (pref0 * fleming(flux[i], flim[i], alpha, fcmin) * vol[i]), 0 where vol[i] <= 0: lf_veff's weights with the
 *   volume of the source's own slice (every source gets one, with or without a slice);
 *   slice_of[i] in [0, nslice): the source's slice, anything else = no slice (it enters no sum); bin_of[i] as in lf_veff;
 *   sums[(nboot + 1) * nslice * nbin]: [0][s][b] = the sum of phi over the sources of slice s and bin b; [k][s][b], k = 1..nboot,
 *   the same over resample k of slice s: n_s draws j = 0 .. n_s - 1 among the slice's n_s sources, source number
 *   min(floor(u n_s), n_s - 1) of the slice in the caller's order, u the 53-bit uniform of the first two words of
 *   Philox4x32-10(counter (j, s, k, 0x736c6963), key seed) - or boot_idx[(k - 1) * m + p] when given: m = the number of sources
 *   with a slice, p = the source's position when these are sorted by slice (stable), the value its draw, a source number
 *   within the slice, in [0, n_s): LF_ERR_ARG otherwise;
 *   counts[nslice * nbin]: the catalogue's sources per slice and bin.
 * Every argument is checked before the device is touched: a NULL pointer (boot_idx may be NULL), n <= 0 or above 2^31 - 1,
 * nslice or nbin outside 1..64, nboot outside 0..10000, pref0 <= 0 give LF_ERR_ARG.  The sums are added in one fixed order,
 * without floating-point atomics: the same inputs give the same bits on every call.  Synchronous. */
int lf_veff_slices(int device, int64_t n, const double *flux, const double *flim, const double *vol, double pref0, double alpha,
                   double fcmin, const int32_t *slice_of, int32_t nslice, const int32_t *bin_of, int32_t nbin, int32_t nboot,
                   const int64_t *boot_idx, uint64_t seed, double *phi, double *sums, int64_t *counts);
/* device time in ms of the last lf_veff_slices call's two kernels (veffs_partial, veffs_reduce); -1 before the first */
double lf_veff_slices_ms(void);

/* Percentiles over R posterior draws of the model LF at P points (post-fit; no context needed, synchronous, like lf_veff).
 * Replaces the draw loop + np.median of LumFuncMCMC.set_median_fit (lumfuncmcmc.py:527-567) and gives the bands around it.
 * draws: R x 3 (LF_FREE / LF_FIXCOMP: logLstar, logphistar, alpha) or R x 7 (LF_ZEVOL: aL, bL, cL, aphi, bphi, cphi, alpha -
 * the quadratic coefficients of log L*(z) and log phi*(z), getQuadCoef of lumfuncmcmc_z.py:40-42) host doubles;
 * logL[P]; z[P] (LF_ZEVOL only, else ignored: NULL);
 * q[nq] in [0, 100] (LF_Q_LINEAR; nq <= 32) or ignored with nq == 1 (LF_Q_MEDIAN); out[nq * P] row-major;
 * values[R * P] or NULL (row r = draw r's LF at every point).  1 <= R <= 4096, P >= 1.  LF_ERR_ARG on any violation
 * (checked before touching the device).
 * out[i][p] is what np.percentile(v, q[i], axis=0) (LF_Q_LINEAR) or np.median(v, axis=0) (LF_Q_MEDIAN) returns for the
 * R x P matrix v of the values, bit for bit (a NaN among a point's values gives NaN). */
enum { LF_Q_LINEAR = 0, LF_Q_MEDIAN = 1 };
int lf_lumfunc_quantiles(int device, int variant, int32_t R, const double *draws, int64_t P, const double *logL,
                         const double *z, int32_t nq, const double *q, int32_t method, double *out, double *values);

/* Device time in ms of the kernel of the most recent successful lf_lumfunc_quantiles call in this process (hipEvents
 * around the launch; measurement only).  LF_ERR_ARG when there is none. */
int lf_lumfunc_quantiles_ms(double *ms);

/* Percentiles over R posterior draws of the INTEGRATED LF above P lower limits: the number density
 *   n(>Lmin) = 10^logphistar Gamma(alpha + 1, x)  [Mpc^-3]                       (LF_INT_NUMBER)
 * or the luminosity density
 *   rho(>Lmin) = 10^logphistar 10^logLstar Gamma(alpha + 2, x)  [erg s^-1 Mpc^-3]   (LF_INT_LUMDENS),
 * x = 10^(logLmin - logLstar), Gamma(a, x) the upper incomplete gamma function (csrc/lf_gammainc.h).  Contract, argument
 * checks, quantile rule and NaN rule are lf_lumfunc_quantiles's, with logLmin[P] in the place of logL; in addition
 * LF_ERR_ARG for an unknown kind, a draw whose alpha is not finite or lies outside [-6, 5], and a NaN in logLmin
 * (logLmin = -inf is allowed and means x = 0: the whole integral, +inf where alpha + 1 + kind <= 0). */
enum { LF_INT_NUMBER = 0, LF_INT_LUMDENS = 1 };
int lf_lumfunc_integral_quantiles(int device, int variant, int kind, int32_t R, const double *draws, int64_t P,
                                  const double *logLmin, const double *z, int32_t nq, const double *q, int32_t method,
                                  double *out, double *values);

/* lf_lumfunc_quantiles_ms for lf_lumfunc_integral_quantiles. */
int lf_lumfunc_integral_quantiles_ms(double *ms);

/* The 1/Veff luminosity function marginalised over the completeness posterior (csrc/lf_veffdraws.h; DESIGN.md section
 * 3.17; post-fit, no context needed, synchronous, like lf_veff).  For R draws d_r = (Flim_0 .. Flim_{nf-1}, alpha) of the
 * completeness parameters (draws[R][nf + 1], Flim in erg cm^-2 s^-1) and n sources (flux, field in [0, nf), vol or the shared
 * vol_all when vol is NULL, bin_of in [0, nbin) or anything else for no bin)
 *   values[r][b] = sum_{i : bin_of[i] == b} w_i(d_r),
 *   w_i(d) = vol_i > 0 ? 1 / (pref0 fleming(flux_i, Flim_{field_i}, alpha, fcmin) vol_i) : 0     (lf_veff's phi)
 * and out[k][b] = the percentile q[k] over r of values[r][b]: q, nq, method and the quantile rule (NumPy's, bit for bit,
 * applied to values) are lf_lumfunc_quantiles's.  out[nq * nbin] row-major; values[R * nbin] or NULL.
 * The sums are taken in one fixed order without atomics: two calls with the same inputs give the same bits, and row r of
 * values depends on draw r and the catalogue only - not on R, on r or on the other draws.  A bin without sources is 0.0.
 * LF_ERR_ARG, before the device is touched, for: a NULL pointer (vol, values and - LF_Q_MEDIAN - q may be NULL), n <= 0 or
 * n >= 2^31, nbin outside 1..1024, nf outside 1..16, R outside 1..4096, nq outside 1..32 (LF_Q_MEDIAN: nq != 1), a q outside
 * [0, 100], an unknown method, a field[i] outside [0, nf), pref0 <= 0, a draw that is not finite or has a Flim <= 0 or
 * alpha == 0. */
int lf_veff_draws(int device, int64_t n, const double *flux, const int32_t *field, const double *vol, double vol_all,
                  double pref0, double fcmin, const int32_t *bin_of, int32_t nbin, int32_t nf, int32_t R, const double *draws,
                  int32_t nq, const double *q, int32_t method, double *out, double *values);

/* ms[3]: device times in ms of the three stages (per-chunk sums, per-bin sums, quantiles) of the most recent successful
 * lf_veff_draws or lf_veff_draws_zmax call in this process (hipEvents; measurement only).  LF_ERR_ARG when there is none. */
int lf_veff_draws_ms(double *ms);

/* Sources per chunk of lf_veff_draws's fixed summation order (VEFFD_CHUNK of csrc/lf_veffdraws.h). */
int lf_veff_draws_chunk(void);

/* lf_veff_draws with every source's volume ending at the z_max of the DRAW's own flux cut (csrc/lf_veffdraws.h; DESIGN.md
 * section 3.29): for source i and draw r the luminosity distance at which the source would be seen at the cut is
 *   D_ir = dist[i] * fmin[r][field_i]^(-1/2)  [Mpc],   dist[i] = sqrt(L_i / 4 pi) / Mpc_cm,   fmin[R][nf] in erg cm^-2 s^-1,
 * one rounded product, and vol_i of lf_veff_draws' weight becomes V(D_ir), the comoving volume between zmin and
 * min(zmax, DL^-1(D_ir)), evaluated on the device from the table (vt_head, vt_zc, vt_rec) that lumfuncmcmc_amd/voltable.py
 * builds and validates against the host's integral:
 *   vt_head[8]   D_0 = DL(zmin), D_K = DL(zmax), V_total, 32 / (D_K - D_0), the first node of dV/dz above zmin, 1 / the nodes'
 *                spacing, 0, 0
 *   vt_zc[32][8] z = DL^-1(D) on 32 equal pieces of [D_0, D_K]: coefficients in t = (D - D_0) vt_head[3] - piece, constant first
 *   vt_rec[vt_nrec][8]  one record per interval between the knots zmin < nodes < zmax: D_k, D_k+1, t_k, V(t_k), V(t_k+1),
 *                dV/dz(t_k), half its slope, 0
 * D >= D_K (fmin = 0 is legal and means D = +inf) gives exactly V_total - with every fmin 0 the values are lf_veff_draws'
 * with vol = NULL and vol_all = V_total, bit for bit; D <= D_0 gives 0 and the source drops out of that draw.  Everything
 * else - the sums' fixed order, the quantiles, out and values, the argument checks - is lf_veff_draws'.  In addition
 * LF_ERR_ARG, before the device is touched, for a NULL dist, fmin or table pointer, a dist or fmin that is not finite or is
 * negative, and a malformed table (a non-finite entry, edges that do not increase strictly from D_0 to D_K, volumes that
 * decrease or do not run from 0 to V_total > 0).  lf_veff_draws_ms reports the stages of whichever of the two ran last. */
int lf_veff_draws_zmax(int device, int64_t n, const double *flux, const int32_t *field, const double *dist, double pref0,
                       double fcmin, const int32_t *bin_of, int32_t nbin, int32_t nf, int32_t R, const double *draws,
                       const double *fmin, const double *vt_head, const double *vt_zc, const double *vt_rec, int64_t vt_nrec,
                       int32_t nq, const double *q, int32_t method, double *out, double *values);

/* Mock catalogues drawn from the model on the device (csrc/lf_mock.h).  The intensity is the
 * likelihood's own interpolant: the trapezoid sum of piece B over the integration grid is exactly the integral of
 * f_f(z, L) = sum_{j,k} lambda_f[j][k] hat_k(z) hat_{j,k}(L), so the expected count M_f of field f sums to piece B of
 * lf_lnprob_pieces over the fields.  A mock is the Poisson process of that intensity: n_f ~ Poisson(M_f) exactly, then
 * each source picks a grid node with probability mass / M_f and inverts the two hat functions.  Philox4x32-10 keyed by
 * seed; a row's catalogue depends only on (seed, row_ids[r], theta row r), never on R or the row's position.
 * The handle reads only the grid and model fields of `desc` (variant, fix_sch_al, sch_al0, nf, S, logL, zarr, volume_part,
 * dl_zarr, integ_part, omega0, fcmin, pivots, device; the catalogue arrays may be NULL and N may be 0).
 * theta: host [R][ndim] (the context's layout; any finite values), row_ids: host [R] or NULL (= 0 .. R-1).  Every call is
 * synchronous.  LF_ERR_ARG, with lf_mock_last_error saying why, for: a NULL pointer, R <= 0, a non-finite theta, an
 * expected count that is not finite, negative or above 2^31 (the message names the row and field), a count < 0 or
 * >= 2^32, nbins outside 1..1022, edges that are not finite and non-decreasing.  The handle stays usable after an error. */
typedef struct lf_mock lf_mock;
lf_mock *lf_mock_create(const lf_desc *desc);
void lf_mock_destroy(lf_mock *m);
/* mean, count: [R][nf] expected counts M and their Poisson draws n */
int lf_mock_counts(lf_mock *m, const double *theta, int32_t R, const int64_t *row_ids, uint64_t seed, double *mean, int64_t *count);
/* the sources of every (row, field) in that order, count[r][f] of them (what lf_mock_counts returned; any count gives the
 * leading sources of the same stream): z, logL, field of length sum(count) */
int lf_mock_draw(lf_mock *m, const double *theta, int32_t R, const int64_t *row_ids, uint64_t seed, const int64_t *count,
                 double *z, double *logL, int32_t *field);
/* histogram of logL per (row, field) of the catalogue lf_mock_draw would write, without writing sources:
 * slot = searchsorted(edges, x, side="right"): 0 = below edges[0], nbins + 1 = at or above edges[nbins];
 * edges [nbins + 1], hist [R][nf][nbins + 2] */
int lf_mock_hist(lf_mock *m, const double *theta, int32_t R, const int64_t *row_ids, uint64_t seed, int32_t nbins,
                 const double *edges, int64_t *hist);
/* The observation step of the mocks (csrc/lf_mock_noise.h): the catalogue records
 * L_obs = L_true + sigma n, n ~ N(0, 1), after detection (the generative model of section 3.18), with sigma in dex a function
 * of the field and of the source's true log10 flux (cgs): M nodes logf_nodes [M], strictly ascending and shared by the
 * fields, sigma [nf][M] >= 0, linear between the nodes and constant outside them (M = 1: one value per field).  The flux of a
 * source at (z, L) is log10 f = L - ld2(z), ld2 the linear interpolant over zarr of log10(4 pi (3.086e24 dl_zarr[k])^2);
 * dl_zarr [S] is read by every variant here (lf_mock_create keeps it for FREE only).  n is Box-Muller on the Philox block
 * (row_id, index, purpose 3, field): a block of its own, the true draws keep their bits, and sigma = 0 leaves L_obs ==
 * L_true bit for bit.  M = 0 clears the model (the pointers are not read).  LF_ERR_ARG, with lf_mock_last_error saying why,
 * for: a NULL pointer, M outside 0..64, nodes that are not finite or not strictly ascending, a sigma that is negative or
 * not finite (the message names the field and the node), a dl_zarr entry that is not finite or not > 0.  An error leaves
 * the model that was set in place and the handle usable. */
int lf_mock_set_error_model(lf_mock *m, int32_t M, const double *logf_nodes, const double *sigma, const double *dl_zarr);
/* lf_mock_draw with the observation step: z, logL_true (what lf_mock_draw writes as logL, bit for bit), logL_obs, sigma,
 * field of length sum(count).  Arguments, limits and refusals of lf_mock_draw; LF_ERR_ARG when no error model is set. */
int lf_mock_draw_err(lf_mock *m, const double *theta, int32_t R, const int64_t *row_ids, uint64_t seed, const int64_t *count,
                     double *z, double *logL_true, double *logL_obs, double *sigma, int32_t *field);
/* lf_mock_hist of logL_obs.  Arguments, limits and refusals of lf_mock_hist; LF_ERR_ARG when no error model is set.  With
 * an all-zero sigma the histogram is lf_mock_hist's. */
int lf_mock_hist_err(lf_mock *m, const double *theta, int32_t R, const int64_t *row_ids, uint64_t seed, int32_t nbins,
                     const double *edges, int64_t *hist);
/* Mock catalogues of the cut process (csrc/lf_mock_cut.h): what the convolved likelihood under a cut
 * on the observed flux models (lf_set_cut_error_model).  A source is catalogued when L_obs = L_true + sigma n >= Lam_k =
 * logL[0][k], k the redshift column of the node it picked and sigma = sigma(field, L_true - ld2n[k]).  The candidates are two
 * independent Poisson processes: piece "above", lf_mock_draw_err's sources (the same counts, true draws and deviates n), and
 * piece "below" on a band grid below the edge, on Philox purposes 4-7; both are observed and cut in the same way.
 * lf_mock_set_cut_band: AFTER lf_mock_set_error_model (a new error model clears the band).  logLb [S][S]: column k holds S
 * ascending nodes from Lam_k - H to Lam_k (H: the caller's, 7.5 max sigma covers the error model); integ_part_b [nf][S][S]:
 * FIXCOMP, ZEVOL - volume_part[k] Omega_0[f] / sqarcsec times the fixed completeness curve at the band's nodes; FREE: not read
 * (NULL).  A field whose sigma is 0 at every node gets no band mass.  LF_ERR_ARG with the reason for: no error model, a NULL
 * logLb, a band node that is not finite or a column that does not ascend strictly, row S - 1 of logLb different from row 0 of
 * logL, a missing integ_part_b, an entry of it that is not finite or < 0.
 * lf_mock_draw_cut: n_cand and mean [R][nf][2] (piece "above", piece "below") are always written.  When their total is
 * above cap, or cap is 0, nothing else is (LF_OK: the caller sizes the arrays and calls again).  Otherwise every candidate's z,
 * logL_true, logL_obs, sigma, field and keep flag (1: catalogued): per (row, field) piece "above" in index order, then piece
 * "below"; kept [R][nf] counts the flags set.  lf_mock_hist_cut: lf_mock_hist_err of the kept candidates, and their number per
 * (row, field) in kept [R][nf].  Refusals of lf_mock_draw_err and lf_mock_hist_err; an expected count above 2^31 names its
 * piece; LF_ERR_ARG without a band. */
int lf_mock_set_cut_band(lf_mock *m, const double *logLb, const double *integ_part_b);
int lf_mock_draw_cut(lf_mock *m, const double *theta, int32_t R, const int64_t *row_ids, uint64_t seed, int64_t cap, double *z,
                     double *logL_true, double *logL_obs, double *sigma, int32_t *field, int32_t *keep, int64_t *n_cand,
                     double *mean, int64_t *kept);
int lf_mock_hist_cut(lf_mock *m, const double *theta, int32_t R, const int64_t *row_ids, uint64_t seed, int32_t nbins,
                     const double *edges, int64_t *hist, int64_t *kept);
/* The mocks binned in redshift and luminosity (csrc/lf_mock_hist2.h): the histogram of the pair
 * (z, L) per (row, field) of the catalogue lf_mock_draw, lf_mock_draw_err or lf_mock_draw_cut would write, without writing
 * sources.  L is logL (lf_mock_hist2), logL_obs (lf_mock_hist2_err) or logL_obs of the catalogued candidates
 * (lf_mock_hist2_cut); redshift carries no noise.  Slots as lf_mock_hist on both axes: sz = searchsorted(z_edges, z,
 * side="right") in 0 .. nz + 1, sl = searchsorted(edges, L, side="right") in 0 .. nl + 1; z_edges [nz + 1], edges [nl + 1],
 * hist [R][nf][nz + 2][nl + 2].  Summed over sz the histogram is lf_mock_hist's (lf_mock_hist_err's, lf_mock_hist_cut's) for the
 * same rows and seed, integer for integer; two calls give the same bits (integer atomics).  count: NULL = the Poisson counts
 * lf_mock_counts returns; else [R][nf] as lf_mock_draw takes it.  lf_mock_hist2_cut draws its own counts and returns
 * kept [R][nf] as lf_mock_hist_cut does.  LF_ERR_ARG, with lf_mock_last_error saying why, before the device is touched:
 * everything lf_mock_hist (lf_mock_hist_err, lf_mock_hist_cut) refuses, a count < 0 or >= 2^32, nz or nl outside 1..1022,
 * (nz + 2)(nl + 2) above 8192 slots (the message names the limit), edges on either axis that are not finite and non-decreasing.
 * The handle stays usable after an error. */
int lf_mock_hist2(lf_mock *m, const double *theta, int32_t R, const int64_t *row_ids, uint64_t seed, const int64_t *count,
                  int32_t nz, const double *z_edges, int32_t nl, const double *edges, int64_t *hist);
int lf_mock_hist2_err(lf_mock *m, const double *theta, int32_t R, const int64_t *row_ids, uint64_t seed, const int64_t *count,
                      int32_t nz, const double *z_edges, int32_t nl, const double *edges, int64_t *hist);
int lf_mock_hist2_cut(lf_mock *m, const double *theta, int32_t R, const int64_t *row_ids, uint64_t seed, int32_t nz,
                      const double *z_edges, int32_t nl, const double *edges, int64_t *hist, int64_t *kept);
/* Last error of this handle; m == NULL: of the last failed lf_mock_create.  Never NULL. */
const char *lf_mock_last_error(const lf_mock *m);

/* Last error message of this context (or of lf_create when ctx == NULL).  Never NULL. */
const char *lf_last_error(const lf_ctx *ctx);

#ifdef __cplusplus
}
#endif
#endif /* LFMCMC_H */
