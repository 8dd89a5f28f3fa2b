// conv_probe.hip - test-only translation unit: the per-source values of the wide, tiled, per-source-posterior and binned copies
// of the convolved likelihood's node loop (csrc/lf_deconv_wide.h, csrc/lf_deconv_tile.h, csrc/lf_lumpost.h, csrc/lf_vefftrue.h)
// with the kernels' own rounding.
//
// Compiled once per module by tests/test_gpu_convterms.py with build.CXXFLAGS and loaded with ctypes after the library (one HIP
// runtime per process); nothing of it is in liblfmcmc.so.  It has no kernel of its own: the library's kernels are launched as
// they are, on argument structs filled here, with chunk tables that put ONE source into each block (cp_vefftrue: `per` sources
// when the order of a chunk's sum is the question).  What a block stores is then that source's value: the other threads add
// exact zeros.  Every entry point takes host arrays, checks its counts against its buffers before it launches, returns the
// first HIP error (0: none) and -1 for arguments it refuses.  No index of any launch depends on a value under test: the bins of
// lf_vefftrue_part are tested against [0, nbin) by the kernel itself, everything else is addressed by block, row and lane.
//
// model[10]: variant, fix_sch_al, sch_al0, kappa, pivots[3], flim0, alpha0, pref0 vol (cp_vefftrue only)
// src[6][nsrc]: lum, a1 (FREE, FIXCOMP: unused; ZEVOL: z), 10^(lum - 42), log flux, 10^(log flux + 17), sigma
// nodes[2 K]: x_k, then ln of the whole weight (lf_deconv.h's form)
#include "../include/lfmcmc.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <memory>
#include <vector>

#include "../lumfuncmcmc_amd/csrc/lf_deconv_tile.h"
#include "../lumfuncmcmc_amd/csrc/lf_deconv_wide.h"
#include "../lumfuncmcmc_amd/csrc/lf_hostprep.h"
#include "../lumfuncmcmc_amd/csrc/lf_lumpost.h"
#include "../lumfuncmcmc_amd/csrc/lf_vefftrue.h"

using namespace lf;

namespace {

constexpr int CP_NMAX = 20000;      // sources per call (lf_problib.NMAX)
constexpr int CP_ROWS = 16;         // theta rows per call
static_assert(BLOCK == 256, "the *_part kernels want 256 threads");
static_assert(CP_ROWS <= VEFFT_ROWS && CP_ROWS <= LUMPOST_SLABS, "one launch group");

#define CP_CHECK(e) do { const hipError_t e_ = (e); if (e_ != hipSuccess) return (int)e_; } while (0)

// the device buffers of one call, freed when the entry point returns
struct Pool {
    std::vector<void*> ptrs;
    hipError_t err = hipSuccess;
    ~Pool() { for (void* p : ptrs) (void)hipFree(p); }
    // host != nullptr: a copy of it; else zeros
    template <class T> T* put(const T* host, size_t count) {
        void* p = nullptr;
        const size_t bytes = (count ? count : 1) * sizeof(T);
        if (err != hipSuccess) return nullptr;
        err = hipMalloc(&p, bytes);
        if (err != hipSuccess) return nullptr;
        ptrs.push_back(p);
        err = host ? hipMemcpy(p, host, bytes, hipMemcpyHostToDevice) : hipMemset(p, 0, bytes);
        return static_cast<T*>(p);
    }
};
template <class T> int fetch(T* host, const T* dev, size_t count) {
    CP_CHECK(hipGetLastError());
    CP_CHECK(hipDeviceSynchronize());
    CP_CHECK(hipMemcpy(host, dev, count * sizeof(T), hipMemcpyDeviceToHost));
    return 0;
}

int ndim_of(int variant, int fsa) {
    if (variant == LF_FREE) return 2 + (fsa ? 0 : 1) + 1 + 1;       // one field
    if (variant == LF_FIXCOMP) return 2 + (fsa ? 0 : 1);
    return 6 + (fsa ? 0 : 1);
}
bool bad_variant(int v) { return v != LF_FREE && v != LF_FIXCOMP && v != LF_ZEVOL; }
bool bad_model(const double* m) { return !m || bad_variant((int)m[0]) || !(m[8] != 0.0) || !(m[7] > 0.0); }

// lf_deconv_part's arguments for nsrc sources in chunks of `per` (nsrc a multiple of it), one field; part, out, nodes and dc.K
// are the caller's business
DeconvArgs base_args(Pool& pool, const double* model, const double* theta, const double* lnprob, int rows, const double* src, int nsrc,
                     int per) {
    DeconvArgs a{};
    GradConst& gc = a.gc;
    gc.variant = (int)model[0], gc.fix_sch_al = (int)model[1], gc.nf = 1, gc.ndim = ndim_of(gc.variant, gc.fix_sch_al);
    gc.sch_al0 = model[2], gc.kappa = model[3];
    gc.om0_grid[0] = 1.0;
    for (int m = 0; m < 3; ++m) gc.pivots[m] = model[4 + m];
    gc.nsrc = (double)nsrc;
    a.dc.flim0[0] = model[7], a.dc.alpha0 = model[8];
    const int nch = nsrc / per;
    std::vector<int> start((size_t)nch), len((size_t)nch, per), field((size_t)nch, 0);
    for (int c = 0; c < nch; ++c) start[(size_t)c] = c * per;
    a.theta = pool.put(theta, (size_t)rows * gc.ndim), a.lnprob = pool.put(lnprob, (size_t)rows);
    const double* d = pool.put(src, (size_t)6 * nsrc);
    if (d) a.lum = d, a.a1 = d + nsrc, a.P = d + 2 * (size_t)nsrc, a.logf = d + 3 * (size_t)nsrc, a.U = d + 4 * (size_t)nsrc, a.sigma = d + 5 * (size_t)nsrc;
    a.chunk_start = pool.put(start.data(), start.size()), a.chunk_len = pool.put(len.data(), len.size());
    a.chunk_field = pool.put(field.data(), field.size());
    a.nch = nch;
    return a;
}
// the wide arguments around d: every chunk of class slot 0, whose table is nodes[2 K]
DeconvWideArgs wide_args(Pool& pool, const DeconvArgs& d, const double* nodes, int K) {
    DeconvWideArgs w{};
    w.d = d;
    const std::vector<int> cls((size_t)d.nch, 0);
    w.chunk_class = pool.put(cls.data(), cls.size());
    w.tables = pool.put(nodes, (size_t)2 * K);
    w.K[0] = K, w.off[0] = 0;
    return w;
}

template <template <int> class F, class... A> void by_variant(int variant, A&&... a) {
    if (variant == LF_FREE) F<LF_FREE>::go(a...);
    else if (variant == LF_FIXCOMP) F<LF_FIXCOMP>::go(a...);
    else F<LF_ZEVOL>::go(a...);
}
template <int V> struct GoWide {
    static void go(dim3 g, const DeconvWideGradArgs& ga) {
        lf_deconv_wide_part<V><<<g, dim3(BLOCK)>>>(ga.w);
        lf_deconv_wide_grad_part<V><<<g, dim3(BLOCK)>>>(ga);
    }
};
template <int V> struct GoLumpost {
    static void go(dim3 g, const LumPostArgs& x, int nrows) { lf_lumpost_part<V><<<g, dim3(BLOCK)>>>(x, 0, nrows); }
};
template <int V> struct GoVeffTrue {
    static void go(dim3 g, const VeffTrueArgs& x) { lf_vefftrue_part<V><<<g, dim3(BLOCK), (unsigned)vefft_dyn_lds_bytes(x.nbin)>>>(x, 0); }
};

}  // namespace

extern "C" {

// the library's own table of sigma class cls (lf_hostprep.h: wide_table), as lf_set_lum_err uploads it: out[2 K]; returns K, -1
// for a class there is none of
int cp_table(int cls, double* out) {
    if (cls < 0 || cls >= DECONV_WIDE_NCLASS || !out) return -1;
    const int K = lfh::wide_nodes(cls);
    return lfh::wide_table(cls, out, out + K) == K ? K : -1;
}

// lf_deconv_wide_part<variant> and lf_deconv_wide_grad_part<variant> on `rows` theta rows and nsrc wide chunks of one source
// each.  cls >= 0: the class's table from lfh::wide_table (nodes, K: not read); cls < 0: the caller's nodes[2 K], K <=
// DECONV_WIDE_KMAX.  part: [rows][nsrc], gpart: [rows][nsrc][DGRAD_SLOTS], both IN AND OUT: what the kernels do not write keeps
// the host's fill.  (The wide kernels do not skip a source with sigma = 0: the wide list has none.)
int cp_wide(const double* model, const double* theta, const double* lnprob, int rows, const double* src, int nsrc, int cls,
            const double* nodes, int K, double* part, double* gpart) {
    if (bad_model(model) || rows < 1 || rows > CP_ROWS || nsrc < 1 || nsrc > CP_NMAX || cls >= DECONV_WIDE_NCLASS || !theta || !lnprob ||
        !src || !part || !gpart)
        return -1;
    std::vector<double> tab((size_t)2 * DECONV_WIDE_KMAX);
    if (cls >= 0) {
        K = lfh::wide_nodes(cls);
        if (lfh::wide_table(cls, tab.data(), tab.data() + K) != K) return -1;
        nodes = tab.data();
    } else if (!nodes || K < 2 || K > DECONV_WIDE_KMAX) {
        return -1;
    }
    Pool pool;
    DeconvWideGradArgs ga{};
    ga.w = wide_args(pool, base_args(pool, model, theta, lnprob, rows, src, nsrc, 1), nodes, K);
    const size_t pn = (size_t)rows * nsrc, gn = pn * DGRAD_SLOTS;
    ga.w.d.part = pool.put(part, pn), ga.gpart = pool.put(gpart, gn);
    CP_CHECK(pool.err);
    by_variant<GoWide>((int)model[0], dim3((unsigned)nsrc, (unsigned)rows), ga);
    const int rc = fetch(part, ga.w.d.part, pn);
    return rc ? rc : fetch(gpart, ga.gpart, gn);
}

// lf_deconv_tile<variant> (FIXCOMP, ZEVOL) on nrows theta rows - any of them with lnprob = -inf - and nsrc chunks of one source
// each, the table nodes[2 K], K <= DECONV_KMAX.  part: [nrows][nsrc], IN AND OUT: a dead row's slots keep the host's fill.
int cp_tile(const double* model, const double* theta, const double* lnprob, int nrows, const double* src, int nsrc,
            const double* nodes, int K, double* part) {
    if (bad_model(model) || (int)model[0] == LF_FREE || nrows < 1 || nrows > CP_ROWS || nsrc < 1 || nsrc > CP_NMAX || K < 2 ||
        K > DECONV_KMAX || !theta || !lnprob || !src || !nodes || !part)
        return -1;
    Pool pool;
    DeconvArgs a = base_args(pool, model, theta, lnprob, nrows, src, nsrc, 1);
    a.dc.K = K, a.nodes = pool.put(nodes, (size_t)2 * K);
    const size_t pn = (size_t)nrows * nsrc;
    a.part = pool.put(part, pn);
    CP_CHECK(pool.err);
    const dim3 g((unsigned)nsrc, (unsigned)((nrows + DECONV_RT - 1) / DECONV_RT));
    if ((int)model[0] == LF_FIXCOMP) lf_deconv_tile<LF_FIXCOMP><<<g, dim3(BLOCK)>>>(a, nrows);
    else lf_deconv_tile<LF_ZEVOL><<<g, dim3(BLOCK)>>>(a, nrows);
    return fetch(part, a.part, pn);
}

// lf_lumpost_part<variant> on `rows` theta rows and nsrc chunks of one source each, the chunks narrow (wide = 0: K <= DECONV_KMAX,
// the table where lf_deconv_part's arguments have it) or wide (wide = 1: K <= DECONV_WIDE_KMAX, the table as a class's).  Row j
// is the one live row of tile j, at place j mod LUMPOST_RT among rows of lnprob = -inf, so slab j holds row j's own (e1, e2)
// before any fold.  e1, e2: [rows][nsrc], IN AND OUT: a source with sigma = 0 is skipped and keeps the host's fill.
int cp_lumpost(const double* model, const double* theta, int rows, const double* src, int nsrc, int wide, const double* nodes, int K,
               double* e1, double* e2) {
    if (bad_model(model) || rows < 1 || rows > CP_ROWS || nsrc < 1 || nsrc > CP_NMAX || K < 2 || K > (wide ? DECONV_WIDE_KMAX : DECONV_KMAX) ||
        !theta || !src || !nodes || !e1 || !e2)
        return -1;
    const int nd = ndim_of((int)model[0], (int)model[1]), nrows = rows * LUMPOST_RT;
    std::vector<double> th((size_t)nrows * nd), lp((size_t)nrows, -HUGE_VAL);
    for (int j = 0; j < rows; ++j) {
        for (int r = 0; r < LUMPOST_RT; ++r)
            for (int q = 0; q < nd; ++q) th[((size_t)j * LUMPOST_RT + r) * nd + q] = theta[(size_t)j * nd + q];
        lp[(size_t)j * LUMPOST_RT + j % LUMPOST_RT] = -123.5;
    }
    std::vector<double> slab((size_t)rows * 2 * nsrc);
    for (int j = 0; j < rows; ++j)
        for (int i = 0; i < nsrc; ++i) {
            slab[((size_t)j * 2) * nsrc + i] = e1[(size_t)j * nsrc + i];
            slab[((size_t)j * 2 + 1) * nsrc + i] = e2[(size_t)j * nsrc + i];
        }
    Pool pool;
    LumPostArgs x{};
    DeconvArgs a = base_args(pool, model, th.data(), lp.data(), nrows, src, nsrc, 1);
    a.dc.K = K, a.nodes = pool.put(nodes, (size_t)2 * K);
    x.d = a;
    x.w = wide_args(pool, a, nodes, K);
    x.n0 = wide ? 0 : nsrc, x.nw = wide ? nsrc : 0;
    x.N = wide ? 0 : nsrc, x.nslots = nsrc;
    x.slab = pool.put(slab.data(), slab.size());
    CP_CHECK(pool.err);
    by_variant<GoLumpost>((int)model[0], dim3((unsigned)nsrc, (unsigned)rows), x, nrows);
    const int rc = fetch(slab.data(), x.slab, slab.size());
    if (rc) return rc;
    for (int j = 0; j < rows; ++j)
        for (int i = 0; i < nsrc; ++i) {
            e1[(size_t)j * nsrc + i] = slab[((size_t)j * 2) * nsrc + i];
            e2[(size_t)j * nsrc + i] = slab[((size_t)j * 2 + 1) * nsrc + i];
        }
    return 0;
}

// lf_vefftrue_part<variant> on `rows` theta rows and nsrc / per chunks of `per` <= DECONV_CH sources each (narrow: K <=
// DECONV_KMAX; wide: K <= DECONV_WIDE_KMAX - the library cuts its wide list at DECONV_WIDE_CH sources, the kernel's batch loop
// takes any length), dynamic LDS vefft_dyn_lds_bytes(nbin).  own_edges = 0: one
// launch, edges[nbin + 1]; own_edges = 1: chunk c is launched alone against edges[c][nbin + 1] (the same buffers, the chunk
// table, the classes and the partial sums advanced to it).  partial: [chunks][VEFFT_ROWS][nbin], IN AND OUT; the rows from
// `rows` on are never written.  The edges must ascend strictly.
int cp_vefftrue(const double* model, const double* theta, const double* lnprob, int rows, const double* src, int nsrc, int per, int wide,
                const double* nodes, int K, const double* edges, int nbin, int own_edges, double* partial) {
    if (bad_model(model) || !(model[9] > 0.0) || rows < 1 || rows > CP_ROWS || nsrc < 1 || nsrc > CP_NMAX || per < 1 ||
        per > DECONV_CH || nsrc % per != 0 || K < 2 || K > (wide ? DECONV_WIDE_KMAX : DECONV_KMAX) || nbin < 1 ||
        nbin > VEFFT_MAXBIN || !theta || !lnprob || !src || !nodes || !edges || !partial)
        return -1;
    const int nch = nsrc / per, nsets = own_edges ? nch : 1;
    for (int s = 0; s < nsets; ++s)
        for (int b = 0; b < nbin; ++b)
            if (!(edges[(size_t)s * (nbin + 1) + b] < edges[(size_t)s * (nbin + 1) + b + 1])) return -1;
    Pool pool;
    VeffTrueArgs x{};
    DeconvArgs a = base_args(pool, model, theta, lnprob, rows, src, nsrc, per);
    a.dc.K = K, a.nodes = pool.put(nodes, (size_t)2 * K);
    x.d = a;
    x.w = wide_args(pool, a, nodes, K);
    x.in_wide = pool.put((const int*)nullptr, (size_t)nsrc);
    const double* ded = pool.put(edges, (size_t)nsets * (nbin + 1));
    x.nbin = nbin, x.pv = model[9];
    const size_t pn = (size_t)nch * VEFFT_ROWS * nbin;
    double* dpart = pool.put(partial, pn);
    CP_CHECK(pool.err);
    if (!own_edges) {
        x.n0 = wide ? 0 : nch, x.nw = wide ? nch : 0;
        x.edges = ded, x.partial = dpart;
        by_variant<GoVeffTrue>((int)model[0], dim3((unsigned)nch, (unsigned)rows), x);
    } else {
        x.n0 = wide ? 0 : 1, x.nw = wide ? 1 : 0;
        for (int c = 0; c < nch; ++c) {
            VeffTrueArgs y = x;
            for (DeconvArgs* d : {&y.d, &y.w.d}) d->chunk_start += c, d->chunk_len += c, d->chunk_field += c;
            y.w.chunk_class += c;
            y.edges = ded + (size_t)c * (nbin + 1), y.partial = dpart + (size_t)c * VEFFT_ROWS * nbin;
            by_variant<GoVeffTrue>((int)model[0], dim3(1u, (unsigned)rows), y);
        }
    }
    return fetch(partial, dpart, pn);
}

// what the callers size their buffers by: 0 DGRAD_SLOTS, 1 DECONV_RT, 2 LUMPOST_RT, 3 VEFFT_ROWS, 4 DECONV_KMAX, 5 DECONV_WIDE_KMAX
int cp_layout(int which) {
    const int v[] = {DGRAD_SLOTS, DECONV_RT, LUMPOST_RT, VEFFT_ROWS, DECONV_KMAX, DECONV_WIDE_KMAX};
    return which >= 0 && which < 6 ? v[which] : -1;
}

int cp_device_count() {
    int n = 0;
    return hipGetDeviceCount(&n) == hipSuccess ? n : 0;
}

}  // extern "C"
