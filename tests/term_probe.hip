// term_probe.hip - test-only translation unit: the device math of csrc/lf_math.h and the per-term forms, table lookups,
// cells and reductions of csrc/lf_kernels.h, one element (or one lane, one wave, one workgroup) at a time.
//
// Compiled by tests/test_gpu_terms.py with build.CXXFLAGS and loaded with ctypes; nothing of it is in liblfmcmc.so.
// The probe kernels call the project's own __device__ functions and do no arithmetic of their own: they load the
// arguments, call, and store what came back.  Workgroups have 256 threads, the LDS tables are filled the way the
// kernels fill them (load_tables_256, load_term_tables<256>), and every global access is guarded by the element count.
// Every entry point takes host arrays, returns the first HIP error (0: none) and -1 for arguments it refuses.
#include "../include/lfmcmc.h"

#include <hip/hip_runtime.h>

#include "../lumfuncmcmc_amd/csrc/lf_kernels.h"

using namespace lf;

namespace {

constexpr int TPB = 256;
static_assert(TPB == BLOCK, "reduce_store and load_tables_256 want 256 threads");

// ---------------------------------------------------------------------------------------------- host side: buffers
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
#define TP_CHECK(e) do { const hipError_t e_ = (e); if (e_ != hipSuccess) return (int)e_; } while (0)
int finish(void* host, const Dev& d, size_t bytes) {
    TP_CHECK(hipGetLastError());
    TP_CHECK(hipDeviceSynchronize());
    TP_CHECK(hipMemcpy(host, d.p, bytes, hipMemcpyDeviceToHost));
    return 0;
}
int blocks_for(long long threads) { return (int)((threads + TPB - 1) / TPB); }

// ---------------------------------------------------------------------------------------------- unary
enum { OP_FEXP_T = 0, OP_FEXP_NEG, OP_FEXP_C, OP_FLOG_HALF, OP_FLOG_HALF_UPPER, OP_FRSQRT, OP_LN_FC_FAST, OP_LN_FC_CAREFUL,
       OP_DEXP, OP_DLOG, OP_DRSQRT, OP_COUNT };

template <int OP>
__global__ __launch_bounds__(TPB) void probe_unary(const double* __restrict__ x, double* __restrict__ y, int n) {
    __shared__ MathTables tab;
    load_tables_256(&tab);
    __syncthreads();
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    const double v = x[i];
    double r;
    if (OP == OP_FEXP_T) r = fexp_t(v, &tab);
    else if (OP == OP_FEXP_NEG) r = fexp_neg(v, &tab);
    else if (OP == OP_FEXP_C) r = fexp_c(v, &tab);
    else if (OP == OP_FLOG_HALF) r = flog_half(v, &tab);
    else if (OP == OP_FLOG_HALF_UPPER) r = flog_half_upper(v, &tab);
    else if (OP == OP_FRSQRT) r = frsqrt(v);
    else if (OP == OP_LN_FC_FAST) r = ln_fc_fast(v, &tab);
    else if (OP == OP_LN_FC_CAREFUL) r = ln_fc_careful(v);
    else if (OP == OP_DEXP) r = dexp(v);
    else if (OP == OP_DLOG) r = dlog(v);
    else r = drsqrt(v);
    y[i] = r;
}

// ---------------------------------------------------------------------------------------------- terms
// w: 9 doubles per element, the fields of WFree in order
enum { TERM_FAST = 0, TERM_NOEXP = 1, TERM_CAREFUL = 2 };
template <int FORM>
__global__ __launch_bounds__(TPB) void probe_term_free(const double* __restrict__ w, const double* __restrict__ lum,
                                                       const double* __restrict__ logf, const double* __restrict__ P,
                                                       const double* __restrict__ U, double* __restrict__ y, int n) {
    __shared__ MathTables tab;
    load_tables_256(&tab);
    __syncthreads();
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    const double* q = w + (size_t)i * 9;
    const WFree wf{q[0], q[1], q[2], q[3], q[4], q[5], q[6], q[7], q[8]};
    if (FORM == TERM_FAST) y[i] = term_free_fast(wf, logf[i], U[i], &tab);
    else if (FORM == TERM_NOEXP) y[i] = term_free_noexp(wf, logf[i], &tab);
    else y[i] = term_free_careful(wf, lum[i], logf[i], P[i], U[i]);
}

// w: 8 doubles per element, the fields of WZ in order; y: {lnT, v} per element
template <bool FAST>
__global__ __launch_bounds__(TPB) void probe_zevol(const double* __restrict__ w, const double* __restrict__ lum,
                                                   const double* __restrict__ z, const double* __restrict__ z2,
                                                   double* __restrict__ y, int n) {
    __shared__ MathTables tab;
    load_tables_256(&tab);
    __syncthreads();
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    const double* q = w + (size_t)i * 8;
    const WZ wz{q[0], q[1], q[2], q[3], q[4], q[5], q[6], q[7]};
    double v;
    const double lnT = lnT_zevol<FAST>(wz, lum[i], z[i], z2[i], v, &tab);
    y[2 * i] = lnT;
    y[2 * i + 1] = v;
}

// ---------------------------------------------------------------------------------------------- tables and cells
// wk: 4 doubles per lane {aC, cA, cYs, cYH}; x: ST doubles per lane; coef: 20 doubles per lane, what table_lookup
// left in TabCoef {cg[8], ch[8], sa, sc, dy} (ch = 0 with NOEXP: it is not loaded then) - the host finds the chosen
// pieces by looking the coefficient rows up in the tables - and `last`, the term of slot ST - 1 that the padding takes
// out again: table_terms<1> with the lane's own pieces on that one source (the same instructions on the same values)
constexpr int NCOEF = 20;
template <int ST, bool NOEXP>
__global__ __launch_bounds__(TPB) void probe_table(const double* __restrict__ wk, const double* __restrict__ x,
                                                   const int* __restrict__ npad, double* __restrict__ sum,
                                                   double* __restrict__ coef, int n) {
    __shared__ TermTables tt;
    load_term_tables<TPB>(&tt);
    __syncthreads();
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    const WalkerK p{wk[4 * i], wk[4 * i + 1], wk[4 * i + 2], wk[4 * i + 3], 0, 0, 0, 0, 0};
    double xs[ST];
#pragma unroll
    for (int k = 0; k < ST; ++k) xs[k] = x[(size_t)i * ST + k];
    TabCoef C;
    table_lookup<ST>(C, xs, p, NOEXP, &tt);
    sum[i] = table_terms<ST, NOEXP>(C, xs, npad[i]);
    double* c = coef + (size_t)i * NCOEF;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        c[q] = C.cg[q];
        c[8 + q] = NOEXP ? 0.0 : C.ch[q];
    }
    c[16] = C.sa;
    c[17] = C.sc;
    c[18] = C.dy;
    const double xl[1] = {xs[ST - 1]};
    c[19] = table_terms<1, NOEXP>(C, xl, 0);
}

// cd: CELL_REC doubles per cell {x_c, S_0 .. S_8}
__global__ __launch_bounds__(TPB) void probe_cell(const double* __restrict__ wk, const double* __restrict__ cd,
                                                  double* __restrict__ y, int n) {
    __shared__ TermTables tt;
    load_term_tables<TPB>(&tt);
    __syncthreads();
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    const WalkerK p{wk[4 * i], wk[4 * i + 1], wk[4 * i + 2], wk[4 * i + 3], 0, 0, 0, 0, 0};
    double c[CELL_REC];
#pragma unroll
    for (int k = 0; k < CELL_REC; ++k) c[k] = cd[(size_t)i * CELL_REC + k];
    y[i] = cell_sum(c, p, &tt);
}

// ---------------------------------------------------------------------------------------------- reductions
// one wave per vector of 64 (four vectors per workgroup); a wave is either wholly inside nv or wholly outside
__global__ __launch_bounds__(TPB) void probe_wave(const double* __restrict__ x, double* __restrict__ dpp,
                                                  double* __restrict__ shfl, int nv) {
    const int t = blockIdx.x * TPB + threadIdx.x, v = t >> 6, lane = t & 63;
    const bool live = v < nv;
    const double val = live ? x[t] : 0.0;
    const double a = wave_sum_dpp(val);
    const double b = wave_sum(val);
    if (live && lane == 63) dpp[v] = a;
    if (live && lane == 0) shfl[v] = b;
}
// every lane's result is returned: each of the 8 lanes of a group holds the group's total
__global__ __launch_bounds__(TPB) void probe_group8(const double* __restrict__ x, const int* __restrict__ xi,
                                                    double* __restrict__ ys, int* __restrict__ yo, int nv) {
    const int t = blockIdx.x * TPB + threadIdx.x;
    const bool live = (t >> 6) < nv;
    const double s = group8_sum(live ? x[t] : 0.0);
    const int o = group8_or(live ? xi[t] : 0);
    if (live) {
        ys[t] = s;
        yo[t] = o;
    }
}
// one workgroup per case: red[nw][256] -> out (nout doubles per case, pre-filled by the host)
__global__ __launch_bounds__(TPB) void probe_reduce(const double* __restrict__ redin, int nw, double* __restrict__ out, int nout,
                                                    int stride, int w0, int chunk, const int* __restrict__ widx) {
    __shared__ double red[16 * BLOCK];
    const double* src = redin + (size_t)blockIdx.x * nw * BLOCK;
    for (int i = threadIdx.x; i < nw * BLOCK; i += TPB) red[i] = src[i];
    __syncthreads();
    reduce_store(red, nw, out + (size_t)blockIdx.x * nout, (size_t)stride, w0, chunk, widx);
}

}  // namespace

// ---------------------------------------------------------------------------------------------- entry points
extern "C" {

int tp_unary(int op, const double* x, double* y, int n) {
    if (op < 0 || op >= OP_COUNT || n <= 0) return -1;
    Dev dx(x, (size_t)n * 8), dy(nullptr, (size_t)n * 8);
    TP_CHECK(dx.err);
    TP_CHECK(dy.err);
    const dim3 g(blocks_for(n)), b(TPB);
#define TP_CASE(OP) case OP: probe_unary<OP><<<g, b>>>(dx.as<double>(), dy.as<double>(), n); break;
    switch (op) {
        TP_CASE(OP_FEXP_T) TP_CASE(OP_FEXP_NEG) TP_CASE(OP_FEXP_C) TP_CASE(OP_FLOG_HALF) TP_CASE(OP_FLOG_HALF_UPPER)
        TP_CASE(OP_FRSQRT) TP_CASE(OP_LN_FC_FAST) TP_CASE(OP_LN_FC_CAREFUL) TP_CASE(OP_DEXP) TP_CASE(OP_DLOG) TP_CASE(OP_DRSQRT)
    }
#undef TP_CASE
    return finish(y, dy, (size_t)n * 8);
}

int tp_term_free(int form, const double* w, const double* lum, const double* logf, const double* P, const double* U,
                 double* y, int n) {
    if (form < TERM_FAST || form > TERM_CAREFUL || n <= 0) return -1;
    Dev dw(w, (size_t)n * 72), dl(lum, (size_t)n * 8), df(logf, (size_t)n * 8), dp(P, (size_t)n * 8), du(U, (size_t)n * 8),
        dy(nullptr, (size_t)n * 8);
    for (const Dev* d : {&dw, &dl, &df, &dp, &du, &dy}) TP_CHECK(d->err);
    const dim3 g(blocks_for(n)), b(TPB);
#define TP_ARGS dw.as<double>(), dl.as<double>(), df.as<double>(), dp.as<double>(), du.as<double>(), dy.as<double>(), n
    if (form == TERM_FAST) probe_term_free<TERM_FAST><<<g, b>>>(TP_ARGS);
    else if (form == TERM_NOEXP) probe_term_free<TERM_NOEXP><<<g, b>>>(TP_ARGS);
    else probe_term_free<TERM_CAREFUL><<<g, b>>>(TP_ARGS);
#undef TP_ARGS
    return finish(y, dy, (size_t)n * 8);
}

int tp_zevol(int fast, const double* w, const double* lum, const double* z, const double* z2, double* y, int n) {
    if (n <= 0) return -1;
    Dev dw(w, (size_t)n * 64), dl(lum, (size_t)n * 8), dz(z, (size_t)n * 8), dz2(z2, (size_t)n * 8), dy(nullptr, (size_t)n * 16);
    for (const Dev* d : {&dw, &dl, &dz, &dz2, &dy}) TP_CHECK(d->err);
    const dim3 g(blocks_for(n)), b(TPB);
    if (fast) probe_zevol<true><<<g, b>>>(dw.as<double>(), dl.as<double>(), dz.as<double>(), dz2.as<double>(), dy.as<double>(), n);
    else probe_zevol<false><<<g, b>>>(dw.as<double>(), dl.as<double>(), dz.as<double>(), dz2.as<double>(), dy.as<double>(), n);
    return finish(y, dy, (size_t)n * 16);
}

int tp_table(int st, int noexp, const double* wk, const double* x, const int* npad, double* sum, double* coef, int n) {
    if ((st != 2 && st != 4 && st != 8) || n <= 0) return -1;
    for (int i = 0; i < n; ++i)
        if (npad[i] < 0 || npad[i] > st) return -1;      // (npad = ST: a lane wholly past the end of its chunk)
    Dev dw(wk, (size_t)n * 32), dx(x, (size_t)n * st * 8), dn(npad, (size_t)n * 4), ds(nullptr, (size_t)n * 8),
        dc(nullptr, (size_t)n * NCOEF * 8);
    for (const Dev* d : {&dw, &dx, &dn, &ds, &dc}) TP_CHECK(d->err);
    const dim3 g(blocks_for(n)), b(TPB);
#define TP_ARGS dw.as<double>(), dx.as<double>(), dn.as<int>(), ds.as<double>(), dc.as<double>(), n
    if (st == 2 && noexp) probe_table<2, true><<<g, b>>>(TP_ARGS);
    else if (st == 2) probe_table<2, false><<<g, b>>>(TP_ARGS);
    else if (st == 4 && noexp) probe_table<4, true><<<g, b>>>(TP_ARGS);
    else if (st == 4) probe_table<4, false><<<g, b>>>(TP_ARGS);
    else if (noexp) probe_table<8, true><<<g, b>>>(TP_ARGS);
    else probe_table<8, false><<<g, b>>>(TP_ARGS);
#undef TP_ARGS
    const int rc = finish(sum, ds, (size_t)n * 8);
    if (rc) return rc;
    TP_CHECK(hipMemcpy(coef, dc.p, (size_t)n * NCOEF * 8, hipMemcpyDeviceToHost));
    return 0;
}

int tp_cell(const double* wk, const double* cd, double* y, int n) {
    if (n <= 0) return -1;
    Dev dw(wk, (size_t)n * 32), dc(cd, (size_t)n * CELL_REC * 8), dy(nullptr, (size_t)n * 8);
    for (const Dev* d : {&dw, &dc, &dy}) TP_CHECK(d->err);
    probe_cell<<<dim3(blocks_for(n)), dim3(TPB)>>>(dw.as<double>(), dc.as<double>(), dy.as<double>(), n);
    return finish(y, dy, (size_t)n * 8);
}

// x: nv vectors of 64; dpp[v] = wave_sum_dpp's lane 63, shfl[v] = wave_sum's lane 0
int tp_wave(const double* x, double* dpp, double* shfl, int nv) {
    if (nv <= 0) return -1;
    Dev dx(x, (size_t)nv * 512), da(nullptr, (size_t)nv * 8), db(nullptr, (size_t)nv * 8);
    for (const Dev* d : {&dx, &da, &db}) TP_CHECK(d->err);
    probe_wave<<<dim3(blocks_for((long long)nv * 64)), dim3(TPB)>>>(dx.as<double>(), da.as<double>(), db.as<double>(), nv);
    const int rc = finish(dpp, da, (size_t)nv * 8);
    if (rc) return rc;
    TP_CHECK(hipMemcpy(shfl, db.p, (size_t)nv * 8, hipMemcpyDeviceToHost));
    return 0;
}

// x, xi: nv vectors of 64; ys, yo: every lane's group8_sum / group8_or
int tp_group8(const double* x, const int* xi, double* ys, int* yo, int nv) {
    if (nv <= 0) return -1;
    Dev dx(x, (size_t)nv * 512), di(xi, (size_t)nv * 256), ds(nullptr, (size_t)nv * 512), dq(nullptr, (size_t)nv * 256);
    for (const Dev* d : {&dx, &di, &ds, &dq}) TP_CHECK(d->err);
    probe_group8<<<dim3(blocks_for((long long)nv * 64)), dim3(TPB)>>>(dx.as<double>(), di.as<int>(), ds.as<double>(), dq.as<int>(), nv);
    const int rc = finish(ys, ds, (size_t)nv * 512);
    if (rc) return rc;
    TP_CHECK(hipMemcpy(yo, dq.p, (size_t)nv * 256, hipMemcpyDeviceToHost));
    return 0;
}

// red: ncase x [nw][256]; out: ncase x nout doubles, IN AND OUT (the slots reduce_store does not write keep what the
// host put there); widx: nw walker indices or NULL.  Refused (-1) unless every slot it will write lies inside nout.
int tp_reduce(const double* red, int nw, double* out, int nout, int stride, int w0, int chunk, const int* widx, int ncase) {
    if (nw < 1 || nw > 16 || ncase <= 0 || nout <= 0 || stride <= 0 || chunk < 0 || chunk >= stride || w0 < 0) return -1;
    for (int w = 0; w < nw; ++w) {
        const long long row = widx ? widx[w] : w0 + w;
        if (row < 0 || row * stride + chunk >= nout) return -1;
    }
    Dev dr(red, (size_t)ncase * nw * BLOCK * 8), dout(out, (size_t)ncase * nout * 8), di(widx, widx ? (size_t)nw * 4 : 0);
    for (const Dev* d : {&dr, &dout, &di}) TP_CHECK(d->err);
    probe_reduce<<<dim3(ncase), dim3(TPB)>>>(dr.as<double>(), nw, dout.as<double>(), nout, stride, w0, chunk,
                                            widx ? di.as<int>() : nullptr);
    return finish(out, dout, (size_t)ncase * nout * 8);
}

int tp_device_count() {
    int n = 0;
    return hipGetDeviceCount(&n) == hipSuccess ? n : 0;
}

}  // extern "C"
