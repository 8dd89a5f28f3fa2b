// grad_probe.hip - test-only translation unit: the completeness forms and the Lagrange basis of csrc/lf_grad.h,
// csrc/lf_deconv.h and csrc/lf_deconv_grad.h one element at a time, and the per-source / per-lattice-node contributions of
// lf_grad_part, lf_deconv_part and lf_deconv_grad_part with the kernels' own rounding.
//
// Compiled by tests/test_gpu_gradterms.py with build.CXXFLAGS and loaded with ctypes; nothing of it is in liblfmcmc.so.
// The thin kernels call the library's own __device__ functions and do no arithmetic of their own.  The *_part kernels are
// launched as they are, on argument structs filled here: the chunk tables put ONE source into each block, and each lattice
// block of GRAD_CH nodes holds one live node, all the others having W = 0 (their integrand is exactly 0 and they are skipped).
// part[row][block][slot] is then that item's contribution: the other 255 threads add exact zeros, and 0 + x is exact in
// wave_sum and in the LDS tree.  Every entry point takes host arrays, checks its counts against its buffers before it
// launches, returns the first HIP error (0: none) and -1 for arguments it refuses.
#include "../include/lfmcmc.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <vector>

#include "../lumfuncmcmc_amd/csrc/lf_deconv_grad.h"
#include "../lumfuncmcmc_amd/csrc/lf_hostprep.h"

using namespace lf;

namespace {

constexpr int TPB = 256;
constexpr int GP_NMAX = 20000;      // elements / items per call (lf_gradproblib.NMAX)
constexpr int GP_ROWS = 8;          // theta rows per call
constexpr int GP_NODES = 512;       // live lattice nodes per call (one block of GRAD_CH nodes each)
static_assert(TPB == BLOCK, "the *_part kernels want 256 threads");

struct Dev {           // one device buffer, freed when the entry point returns
    void* p = nullptr;
    hipError_t err = hipSuccess;
    Dev(const void* host, size_t bytes) {
        if (bytes == 0) bytes = 8;
        err = hipMalloc(&p, bytes);
        if (err != hipSuccess) { p = nullptr; return; }
        err = host ? hipMemcpy(p, host, bytes, hipMemcpyHostToDevice) : hipMemset(p, 0, bytes);
    }
    ~Dev() { if (p) (void)hipFree(p); }
    Dev(const Dev&) = delete;
    Dev& operator=(const Dev&) = delete;
    template <class T> T* as() const { return static_cast<T*>(p); }
};
#define GP_CHECK(e) do { const hipError_t e_ = (e); if (e_ != hipSuccess) return (int)e_; } while (0)
int finish(void* host, const Dev& d, size_t bytes) {
    GP_CHECK(hipGetLastError());
    GP_CHECK(hipDeviceSynchronize());
    GP_CHECK(hipMemcpy(host, d.p, bytes, hipMemcpyDeviceToHost));
    return 0;
}
int blocks_for(long long threads) { return (int)((threads + TPB - 1) / TPB); }

// ---------------------------------------------------------------------------------------------- completeness forms
enum { COMP_GRAD = 0, COMP_DGRAD = 1, COMP_LCOMP = 2 };
// COMP_GRAD:  p = Flim, q = logf, r = U:  grad_comp(grad_comp_row(row, kappa), logf, U)
// COMP_DGRAD: q = y, r = v:               dgrad_comp(aC, aC_ln, kc2, y, v) = comp_form<true>, aC_ln and kc2 out of grad_comp_row
//                                         (the statements deconv_row forms them with)
// COMP_LCOMP: q = y, r = v:               deconv_lcomp(aC, y, v) = comp_form<false>(...).l
// out: {l, dF, dC} per element (COMP_LCOMP: l only, the other two stay 0)
template <int WHICH>
__global__ __launch_bounds__(TPB) void probe_comp(const double* __restrict__ aC, const double* __restrict__ kappa,
                                                  const double* __restrict__ p, const double* __restrict__ q,
                                                  const double* __restrict__ r, double* __restrict__ out, int n) {
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    GradRow row{};
    row.aC = aC[i];
    row.flim = WHICH == COMP_GRAD ? p[i] : 1.0;
    GradComp c{0.0, 0.0, 0.0};
    if (WHICH == COMP_LCOMP) {
        c.l = deconv_lcomp(aC[i], q[i], r[i]);
    } else {
        const GradCompRow cr = grad_comp_row(row, kappa[i]);
        if (WHICH == COMP_GRAD) c = grad_comp(cr, q[i], r[i]);
        else c = dgrad_comp(aC[i], cr.aC_ln, cr.kc2, q[i], r[i]);
    }
    out[3 * (size_t)i] = c.l;
    out[3 * (size_t)i + 1] = c.dF;
    out[3 * (size_t)i + 2] = c.dC;
}

// piv: 3 doubles per element
__global__ __launch_bounds__(TPB) void probe_basis(const double* __restrict__ piv, const double* __restrict__ z,
                                                   double* __restrict__ out, int n) {
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    GradConst gc{};
#pragma unroll
    for (int m = 0; m < 3; ++m) gc.pivots[m] = piv[3 * (size_t)i + m];
    double l[3];
    grad_basis(grad_piv(gc), z[i], l);
#pragma unroll
    for (int m = 0; m < 3; ++m) out[3 * (size_t)i + m] = l[m];
}

// ---------------------------------------------------------------------------------------------- the *_part kernels
int ndim_of(int variant, int fsa) {
    if (variant == LF_FREE) return 2 + (fsa ? 0 : 1) + 1 + 1;       // one field
    if (variant == LF_FIXCOMP) return 2 + (fsa ? 0 : 1);
    return 6 + (fsa ? 0 : 1);
}
GradConst make_gc(int variant, int fsa, double sch_al0, double kappa, double om0, const double* pivots, int nsrc) {
    GradConst gc{};
    gc.variant = variant, gc.fix_sch_al = fsa, gc.nf = 1, gc.ndim = ndim_of(variant, fsa);
    gc.sch_al0 = sch_al0, gc.kappa = kappa;
    gc.om0_grid[0] = om0;
    for (int m = 0; m < 3; ++m) gc.pivots[m] = pivots[m];
    gc.nsrc = (double)nsrc;
    return gc;
}
// one source per block
struct OnePerBlock {
    std::vector<int> start, len, field;
    explicit OnePerBlock(int n) : start((size_t)n), len((size_t)n, 1), field((size_t)n, 0) {
        for (int i = 0; i < n; ++i) start[(size_t)i] = i;
    }
};
bool bad_variant(int v) { return v != LF_FREE && v != LF_FIXCOMP && v != LF_ZEVOL; }

}  // namespace

// ---------------------------------------------------------------------------------------------- entry points
extern "C" {

int gp_comp(int which, const double* aC, const double* kappa, const double* p, const double* q, const double* r, double* out, int n) {
    if (which < COMP_GRAD || which > COMP_LCOMP || n <= 0 || n > GP_NMAX || !aC || !kappa || !q || !r || !out) return -1;
    if (which == COMP_GRAD && !p) return -1;
    const size_t nb = (size_t)n * 8;
    Dev da(aC, nb), dk(kappa, nb), dp(p ? p : aC, nb), dq(q, nb), dr(r, nb), dout(nullptr, 3 * nb);
    for (const Dev* d : {&da, &dk, &dp, &dq, &dr, &dout}) GP_CHECK(d->err);
    const dim3 g(blocks_for(n)), b(TPB);
#define GP_ARGS da.as<double>(), dk.as<double>(), dp.as<double>(), dq.as<double>(), dr.as<double>(), dout.as<double>(), n
    if (which == COMP_GRAD) probe_comp<COMP_GRAD><<<g, b>>>(GP_ARGS);
    else if (which == COMP_DGRAD) probe_comp<COMP_DGRAD><<<g, b>>>(GP_ARGS);
    else probe_comp<COMP_LCOMP><<<g, b>>>(GP_ARGS);
#undef GP_ARGS
    return finish(out, dout, 3 * nb);
}

int gp_basis(const double* piv, const double* z, double* out, int n) {
    if (n <= 0 || n > GP_NMAX || !piv || !z || !out) return -1;
    Dev dp(piv, (size_t)n * 24), dz(z, (size_t)n * 8), dout(nullptr, (size_t)n * 24);
    for (const Dev* d : {&dp, &dz, &dout}) GP_CHECK(d->err);
    probe_basis<<<dim3(blocks_for(n)), dim3(TPB)>>>(dp.as<double>(), dz.as<double>(), dout.as<double>(), n);
    return finish(out, dout, (size_t)n * 24);
}

// lf_grad_part<variant> on `rows` theta rows, nsrc source blocks (one source each; lum, a1, P, U: nsrc doubles, a1 / P / U as
// the variant reads them) and nlive lattice blocks (one live node each: G, PG, W, a3, a4 of the live node; block q holds it at
// offset (37 q) mod GRAD_CH among nodes of W = 0).  part: [rows][nsrc + nlive][GRAD_SLOTS], IN AND OUT: what the kernel does
// not write keeps the host's fill.
int gp_grad_part(int variant, int fsa, double sch_al0, double kappa, double om0, const double* pivots, const double* theta,
                 const double* lnprob, int rows, const double* lum, const double* a1, const double* P, const double* U, int nsrc,
                 const double* G, const double* PG, const double* W, const double* a3, const double* a4, int nlive, double* part) {
    if (bad_variant(variant) || rows < 1 || rows > GP_ROWS || nsrc < 0 || nsrc > GP_NMAX || nlive < 0 || nlive > GP_NODES ||
        nsrc + nlive < 1 || !pivots || !theta || !lnprob || !part)
        return -1;
    if (nsrc > 0 && (!lum || !a1 || !P || !U)) return -1;
    if (nlive > 0 && (!G || !PG || !W || !a3 || !a4)) return -1;
    GradArgs a{};
    a.gc = make_gc(variant, fsa, sch_al0, kappa, om0, pivots, nsrc);
    const int nd = a.gc.ndim, nblk = nsrc + nlive;
    const size_t nn = (size_t)nlive * GRAD_CH;
    // the lattice: benign dead nodes (the first live node's values) with W = 0, the live node of block q at (37 q) mod GRAD_CH
    std::vector<double> hG(nn), hPG(nn), hW(nn, 0.0), h3(nn), h4(nn);
    for (int q = 0; q < nlive; ++q)
        for (int i = 0; i < GRAD_CH; ++i) {
            const size_t g = (size_t)q * GRAD_CH + i;
            const bool live = i == (37 * q) % GRAD_CH;
            const int s = live ? q : 0;
            hG[g] = G[s], hPG[g] = PG[s], h3[g] = a3[s], h4[g] = a4[s];
            if (live) hW[g] = W[q];
        }
    const OnePerBlock ch(nsrc);
    const size_t sb = (size_t)nsrc * 8, pb = (size_t)rows * nblk * GRAD_SLOTS * 8;
    Dev dth(theta, (size_t)rows * nd * 8), dlp(lnprob, (size_t)rows * 8), dpart(part, pb), dl(lum, sb), d1(a1, sb), dP(P, sb), dU(U, sb),
        dcs(ch.start.data(), (size_t)nsrc * 4), dcl(ch.len.data(), (size_t)nsrc * 4), dcf(ch.field.data(), (size_t)nsrc * 4),
        dG(hG.data(), nn * 8), dPG(hPG.data(), nn * 8), dW(hW.data(), nn * 8), d3(h3.data(), nn * 8), d4(h4.data(), nn * 8);
    for (const Dev* d : {&dth, &dlp, &dpart, &dl, &d1, &dP, &dU, &dcs, &dcl, &dcf, &dG, &dPG, &dW, &d3, &d4}) GP_CHECK(d->err);
    a.theta = dth.as<double>(), a.lnprob = dlp.as<double>(), a.part = dpart.as<double>(), a.grad = nullptr;
    a.lum = dl.as<double>(), a.a1 = d1.as<double>(), a.P = dP.as<double>(), a.U = dU.as<double>();
    a.chunk_start = dcs.as<int>(), a.chunk_len = dcl.as<int>(), a.chunk_field = dcf.as<int>();
    a.G = dG.as<double>(), a.PG = dPG.as<double>(), a.W = dW.as<double>(), a.a3 = d3.as<double>(), a.a4 = d4.as<double>();
    a.nnodes = (int)nn, a.nchA = nsrc, a.nchB = nlive, a.nfB = 1;
    const dim3 g((unsigned)nblk, (unsigned)rows), b(TPB);
    if (variant == LF_FREE) lf_grad_part<LF_FREE><<<g, b>>>(a);
    else if (variant == LF_FIXCOMP) lf_grad_part<LF_FIXCOMP><<<g, b>>>(a);
    else lf_grad_part<LF_ZEVOL><<<g, b>>>(a);
    return finish(part, dpart, pb);
}

// lf_deconv_part<variant> and lf_deconv_grad_part<variant> on `rows` theta rows and nsrc blocks of one source each (lum, a1, P,
// logf, U, sigma: nsrc doubles), the node table nodes[2 K] = {x_k}, {ln(w_k / sqrt(pi))}.  FIXCOMP, ZEVOL: the fixed
// completeness (flim0, alpha0).  part: [rows][nsrc], gpart: [rows][nsrc][DGRAD_SLOTS], both IN AND OUT.
int gp_deconv(int variant, int fsa, double sch_al0, double kappa, const double* pivots, double flim0, double alpha0,
              const double* theta, const double* lnprob, int rows, const double* lum, const double* a1, const double* P,
              const double* logf, const double* U, const double* sigma, int nsrc, const double* nodes, int K, double* part,
              double* gpart) {
    if (bad_variant(variant) || rows < 1 || rows > GP_ROWS || nsrc < 1 || nsrc > GP_NMAX || K < 2 || K > DECONV_KMAX || !pivots ||
        !theta || !lnprob || !lum || !a1 || !P || !logf || !U || !sigma || !nodes || !part || !gpart)
        return -1;
    DeconvGradArgs ga{};
    DeconvArgs& a = ga.d;
    a.gc = make_gc(variant, fsa, sch_al0, kappa, 1.0, pivots, nsrc);
    a.dc.K = K, a.dc.alpha0 = alpha0, a.dc.flim0[0] = flim0;
    const int nd = a.gc.ndim;
    const OnePerBlock ch(nsrc);
    const size_t sb = (size_t)nsrc * 8, pb = (size_t)rows * nsrc * 8, gb = pb * DGRAD_SLOTS;
    Dev dth(theta, (size_t)rows * nd * 8), dlp(lnprob, (size_t)rows * 8), dpart(part, pb), dgp(gpart, gb), dl(lum, sb), d1(a1, sb),
        dP(P, sb), dlf(logf, sb), dU(U, sb), dsg(sigma, sb), dn(nodes, (size_t)2 * K * 8), dcs(ch.start.data(), (size_t)nsrc * 4),
        dcl(ch.len.data(), (size_t)nsrc * 4), dcf(ch.field.data(), (size_t)nsrc * 4);
    for (const Dev* d : {&dth, &dlp, &dpart, &dgp, &dl, &d1, &dP, &dlf, &dU, &dsg, &dn, &dcs, &dcl, &dcf}) GP_CHECK(d->err);
    a.theta = dth.as<double>(), a.lnprob = dlp.as<double>(), a.part = dpart.as<double>(), a.out = nullptr;
    a.lum = dl.as<double>(), a.a1 = d1.as<double>(), a.P = dP.as<double>(), a.logf = dlf.as<double>(), a.U = dU.as<double>();
    a.sigma = dsg.as<double>(), a.nodes = dn.as<double>();
    a.chunk_start = dcs.as<int>(), a.chunk_len = dcl.as<int>(), a.chunk_field = dcf.as<int>();
    a.nch = nsrc;
    ga.gpart = dgp.as<double>(), ga.grad = nullptr;
    const dim3 g((unsigned)nsrc, (unsigned)rows), b(TPB);
    if (variant == LF_FREE) {
        lf_deconv_part<LF_FREE><<<g, b>>>(a);
        lf_deconv_grad_part<LF_FREE><<<g, b>>>(ga);
    } else if (variant == LF_FIXCOMP) {
        lf_deconv_part<LF_FIXCOMP><<<g, b>>>(a);
        lf_deconv_grad_part<LF_FIXCOMP><<<g, b>>>(ga);
    } else {
        lf_deconv_part<LF_ZEVOL><<<g, b>>>(a);
        lf_deconv_grad_part<LF_ZEVOL><<<g, b>>>(ga);
    }
    const int rc = finish(part, dpart, pb);
    if (rc) return rc;
    GP_CHECK(hipMemcpy(gpart, dgp.p, gb, hipMemcpyDeviceToHost));
    return 0;
}

// the library's own Gauss-Hermite table (lf_hostprep.h), as lf_set_lum_err uploads it: out[2 K]
int gp_nodes(int K, double* out) {
    if (K < 2 || K > DECONV_KMAX || !out) return -1;
    return lfh::gauss_hermite(K, out, out + K) ? 0 : -1;
}

// kappa as the library's contexts hold it (lf_hostprep.h: grad_const), for a test that compares with a context's own value
double gp_kappa(double fcmin) { return std::sqrt(lfh::fc_ratio(fcmin)); }

int gp_device_count() {
    int n = 0;
    return hipGetDeviceCount(&n) == hipSuccess ? n : 0;
}

}  // extern "C"
