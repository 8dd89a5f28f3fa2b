// node_probe.hip - test-only translation unit: the grid-node forms of piece B (csrc/lf_kernels.h), one node at a time.
//
// Compiled by tests/test_gpu_nodeterms.py with build.CXXFLAGS and loaded with ctypes; nothing of it is in liblfmcmc.so.
// The probe kernels call the project's own __device__ functions and do no arithmetic of their own: they load the
// arguments, call, and store what came back.  Workgroups have 256 threads, the LDS tables are filled the way the
// kernels fill them (load_tables_256), and every global access is guarded by the element count.  Every entry point
// takes host arrays, returns the first HIP error (0: none) and -1 for arguments it refuses.
//
// Named functions (field_sum<NF> and field_sum_bright<NF> behind field_sum_nf, walker_vmin, quad_coef, quad_nofma,
// quad_comp, quad_range) are called directly.  The inline expressions of gridsum_body - the Schechter factor of FREE
// and FIXCOMP, the column and the row form of the z-evolving node - are driven through gridsum_body<VARIANT, TW>
// itself on node arrays in which each chunk of 256 has ONE node of weight 1.0 and 255 copies of it of weight 0.0.
// reduce_store (lf_kernels.h) starts its four accumulators at +0.0, adds the 16 columns of a lane to them, then
// (s0 + s1) + (s2 + s3) and four DPP row shifts whose empty lanes add +0.0: every addend but one is +-0.0, x + (+-0.0)
// is x exactly, so the partial it writes is that one node's value, bit for bit (and +0.0 when the node's value is 0).
#include "../include/lfmcmc.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <vector>

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
#define NP_CHECK(e) do { const hipError_t e_ = (e); if (e_ != hipSuccess) return (int)e_; } while (0)
int finish(void* host, const Dev& d, size_t bytes) {
    NP_CHECK(hipGetLastError());
    NP_CHECK(hipDeviceSynchronize());
    NP_CHECK(hipMemcpy(host, d.p, bytes, hipMemcpyDeviceToHost));
    return 0;
}
int blocks_for(long long threads) { return (int)((threads + TPB - 1) / TPB); }

// ---------------------------------------------------------------------------------------------- the node sum
// One record per element: rec[i][REC].  The kernels read a walker's record as wave-uniform values (uni() takes the
// first lane's), so a wave takes its 64 elements one at a time - every lane calls with element e's arguments - and lane
// e keeps what came back.
__global__ __launch_bounds__(TPB) void probe_field_sum(KConst kc, const double* __restrict__ rec, const double* __restrict__ aC,
                                                       const double* __restrict__ a3, const double* __restrict__ a4, int bright,
                                                       double* __restrict__ y, double* __restrict__ vmin, int n) {
    __shared__ MathTables tab;
    load_tables_256(&tab);
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int first = blockIdx.x * TPB + (threadIdx.x - lane);
    double out = 0.0, vm = 0.0;
    for (int e = 0; e < 64; ++e) {
        const int i = first + e;
        if (i >= n) break;                                     // (wave-uniform)
        const double* __restrict__ r = rec + (size_t)i * REC;
        const double s = field_sum_nf(kc, r, aC[i], a3[i], a4[i], &tab, bright != 0);
        const double m = walker_vmin(kc, r);
        if (lane == e) {
            out = s;
            vm = m;
        }
    }
    const int i = first + lane;
    if (i < n) {
        y[i] = out;
        vmin[i] = vm;
    }
}

// ---------------------------------------------------------------------------------------------- the quadratics
// x: 6 doubles per element, y: 3 doubles per element
//   QUAD_COEF   {y1, y2, y3, z1, z2, z3} -> {a, b, c}
//   QUAD_NOFMA  {a, b, c, z, z2, -}      -> {value, -, -}
//   QUAD_COMP   {a, b, c, z, -, -}       -> {value, -, -}
//   QUAD_RANGE  {a, b, c, lo, hi, -}     -> {mn, mx, -}
enum { QUAD_COEF = 0, QUAD_NOFMA, QUAD_COMP, QUAD_RANGE, QUAD_COUNT };
template <int OP>
__global__ __launch_bounds__(TPB) void probe_quad(const double* __restrict__ x, double* __restrict__ y, int n) {
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    const double* q = x + (size_t)i * 6;
    double r0 = 0.0, r1 = 0.0, r2 = 0.0;
    if (OP == QUAD_COEF) quad_coef(q[0], q[1], q[2], q[3], q[4], q[5], r0, r1, r2);
    else if (OP == QUAD_NOFMA) r0 = quad_nofma(q[0], q[1], q[2], q[3], q[4]);
    else if (OP == QUAD_COMP) r0 = quad_comp(q[0], q[1], q[2], q[3]);
    else quad_range(q[0], q[1], q[2], q[3], q[4], r0, r1);
    y[3 * i] = r0;
    y[3 * i + 1] = r1;
    y[3 * i + 2] = r2;
}

// ---------------------------------------------------------------------------------------------- gridsum_body
template <int VARIANT, int TW>
__global__ __launch_bounds__(TPB) void probe_gridsum(KConst kc, NodeArrays na, const double* __restrict__ wrec,
                                                     const int* __restrict__ wmode, int B, int ntiles, int tw,
                                                     double* __restrict__ partial, int pstride) {
    __shared__ MathTables tab;
    __shared__ __attribute__((aligned(16))) double red[TW * BLOCK];
    load_tables_256(&tab);
    __syncthreads();
    gridsum_body<VARIANT, TW>(kc, na, wrec, wmode, B, ntiles, tw, (int)blockIdx.x, partial, pstride, tab, red);
}

template <int VARIANT>
void launch_gridsum(int TW, dim3 g, const KConst& kc, const NodeArrays& na, const double* wrec, const int* wmode, int B, int ntiles,
                    int tw, double* partial, int pstride) {
    if (TW == 16) probe_gridsum<VARIANT, 16><<<g, dim3(TPB)>>>(kc, na, wrec, wmode, B, ntiles, tw, partial, pstride);
    else probe_gridsum<VARIANT, 4><<<g, dim3(TPB)>>>(kc, na, wrec, wmode, B, ntiles, tw, partial, pstride);
}

bool set_om0(KConst& kc, int nf, const double* om0) {
    if (nf < 1 || nf > MAXF || !om0) return false;
    kc.nf = nf;
    for (int f = 0; f < nf; ++f) kc.om0_grid[f] = om0[f];
    return true;
}

}  // namespace

// ---------------------------------------------------------------------------------------------- entry points
extern "C" {

// field_sum_nf(kc, r, aC[i], a3[i], a4[i], tab, bright) and walker_vmin(kc, r) per element; the record r of element i holds
// ca[i][f] at RF(f, F_CA) and v[i][f] at RF(f, F_V) for f < nf and zeros elsewhere.  kc: value-initialised but for nf and
// om0_grid.  om0: nf doubles; ca, v: MAXF doubles per element.
int np_field_sum(int nf, int bright, const double* om0, const double* aC, const double* a3, const double* a4, const double* ca,
                 const double* v, double* y, double* vmin, int n) {
    KConst kc{};
    if (!set_om0(kc, nf, om0) || n <= 0 || n > (1 << 20)) return -1;
    std::vector<double> rec((size_t)n * REC, 0.0);
    for (int i = 0; i < n; ++i)
        for (int f = 0; f < nf; ++f) {
            rec[(size_t)i * REC + RF(f, F_CA)] = ca[(size_t)i * MAXF + f];
            rec[(size_t)i * REC + RF(f, F_V)] = v[(size_t)i * MAXF + f];
        }
    Dev dr(rec.data(), rec.size() * 8), dc(aC, (size_t)n * 8), d3(a3, (size_t)n * 8), d4(a4, (size_t)n * 8), dy(nullptr, (size_t)n * 8),
        dm(nullptr, (size_t)n * 8);
    for (const Dev* d : {&dr, &dc, &d3, &d4, &dy, &dm}) NP_CHECK(d->err);
    probe_field_sum<<<dim3(blocks_for(n)), dim3(TPB)>>>(kc, dr.as<double>(), dc.as<double>(), d3.as<double>(), d4.as<double>(), bright,
                                                        dy.as<double>(), dm.as<double>(), n);
    const int rc = finish(y, dy, (size_t)n * 8);
    if (rc) return rc;
    NP_CHECK(hipMemcpy(vmin, dm.p, (size_t)n * 8, hipMemcpyDeviceToHost));
    return 0;
}

int np_quad(int op, const double* x, double* y, int n) {
    if (op < 0 || op >= QUAD_COUNT || n <= 0) return -1;
    Dev dx(x, (size_t)n * 48), dy(nullptr, (size_t)n * 24);
    NP_CHECK(dx.err);
    NP_CHECK(dy.err);
    const dim3 g(blocks_for(n)), b(TPB);
    if (op == QUAD_COEF) probe_quad<QUAD_COEF><<<g, b>>>(dx.as<double>(), dy.as<double>(), n);
    else if (op == QUAD_NOFMA) probe_quad<QUAD_NOFMA><<<g, b>>>(dx.as<double>(), dy.as<double>(), n);
    else if (op == QUAD_COMP) probe_quad<QUAD_COMP><<<g, b>>>(dx.as<double>(), dy.as<double>(), n);
    else probe_quad<QUAD_RANGE><<<g, b>>>(dx.as<double>(), dy.as<double>(), n);
    return finish(y, dy, (size_t)n * 24);
}

// gridsum_body<variant, TW> on one workgroup per (chunk of 256 nodes, tile of tw walkers).
//   G, PG, W, a3, a4: nnodes doubles; a4min: one per chunk (FREE); wrec: B records of REC doubles; mode: one int per walker
//   (what the kernels read at wmode[w * MAXF * WM]); partial: B x nch doubles, IN AND OUT (slot [w][c] of every walker and
//   chunk is written; the host's fill shows one that was not).
//   kc: value-initialised but for variant, nf, om0_grid, S, zgrid_cols, specialise.
// With zgrid_cols the nodes are the column-major S x S lattice (nnodes = S * S, S >= BLOCK / (ZCOLS - 1)), and a chunk reads
// a3 / a4 at the first node of each of its ZCOLS columns, clamped to the last column; the device copies of a3 and a4 carry
// ZCOLS * S further doubles (NaN), so that every such index lies inside the buffer whether or not it is clamped.
int np_gridsum(int variant, int TW, int tw, int nf, const double* om0, int S, int zgrid_cols, int specialise, const double* G,
               const double* PG, const double* W, const double* a3, const double* a4, const double* a4min, int nnodes,
               const double* wrec, const int* mode, int B, double* partial) {
    KConst kc{};
    if (!set_om0(kc, nf, om0)) return -1;
    if (variant != LF_FREE && variant != LF_FIXCOMP && variant != LF_ZEVOL) return -1;
    if ((TW != 16 && TW != 4) || tw < 1 || tw > TW || B < 1 || B > 4096 || nnodes < 1 || nnodes > (1 << 22) || S < 1 || S > 2048) return -1;
    if (zgrid_cols && (variant != LF_ZEVOL || S < BLOCK / (ZCOLS - 1) || (long long)S * S != nnodes)) return -1;
    const int nch = (nnodes + BLOCK - 1) / BLOCK, ntiles = (B + tw - 1) / tw;
    if ((long long)nch * ntiles > 8192) return -1;
    kc.variant = variant;
    kc.S = S;
    kc.zgrid_cols = zgrid_cols ? 1 : 0;
    kc.specialise = specialise ? 1 : 0;
    std::vector<int> wm((size_t)B * MAXF * WM, 0);
    for (int w = 0; w < B; ++w) {
        if (mode[w] < MODE_FAST || mode[w] > MODE_SKIPSRC) return -1;
        for (int f = 0; f < MAXF; ++f) wm[((size_t)w * MAXF + f) * WM + M_MODE] = mode[w];
    }
    const size_t pad = (size_t)ZCOLS * S;
    std::vector<double> h3((size_t)nnodes + pad, std::nan("")), h4((size_t)nnodes + pad, std::nan(""));
    for (int g = 0; g < nnodes; ++g) {
        h3[g] = a3[g];
        h4[g] = a4[g];
    }
    Dev dG(G, (size_t)nnodes * 8), dP(PG, (size_t)nnodes * 8), dW(W, (size_t)nnodes * 8), d3(h3.data(), h3.size() * 8),
        d4(h4.data(), h4.size() * 8), dmin(a4min, (size_t)nch * 8), dr(wrec, (size_t)B * REC * 8), dm(wm.data(), wm.size() * 4),
        dp(partial, (size_t)B * nch * 8);
    for (const Dev* d : {&dG, &dP, &dW, &d3, &d4, &dmin, &dr, &dm, &dp}) NP_CHECK(d->err);
    const NodeArrays na{dG.as<double>(), dP.as<double>(), dW.as<double>(), d3.as<double>(), d4.as<double>(), dmin.as<double>(), nnodes};
    const dim3 g((unsigned)(nch * ntiles));
    if (variant == LF_FREE) launch_gridsum<LF_FREE>(TW, g, kc, na, dr.as<double>(), dm.as<int>(), B, ntiles, tw, dp.as<double>(), nch);
    else if (variant == LF_FIXCOMP) launch_gridsum<LF_FIXCOMP>(TW, g, kc, na, dr.as<double>(), dm.as<int>(), B, ntiles, tw, dp.as<double>(), nch);
    else launch_gridsum<LF_ZEVOL>(TW, g, kc, na, dr.as<double>(), dm.as<int>(), B, ntiles, tw, dp.as<double>(), nch);
    return finish(partial, dp, (size_t)B * nch * 8);
}

// the project's own layout constants, for the host side of the tests
int np_layout(int what) {
    switch (what) {
        case 0: return REC;
        case 1: return RF(0, F_CA);
        case 2: return RF(0, F_V);
        case 3: return RF(1, F_CA) - RF(0, F_CA);
        case 4: return R_LSTAR;
        case 5: return R_C0;
        case 6: return R_C1;
        case 7: return R_Q;
        case 8: return R_ALPHAC;
        case 9: return Z_AL;
        case 10: return Z_C1;
        case 11: return MODE_SKIP;
        case 12: return ZCOLS;
        default: return -1;
    }
}

int np_device_count() {
    int n = 0;
    return hipGetDeviceCount(&n) == hipSuccess ? n : 0;
}

}  // extern "C"
