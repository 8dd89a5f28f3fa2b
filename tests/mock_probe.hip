// mock_probe.hip - test-only translation unit: the device functions of csrc/lf_mock.h and csrc/lf_mock_noise.h, one element
// (or one workgroup, for the cumulative sums) at a time.
//
// Compiled by tests/test_gpu_mockprobe.py with build.CXXFLAGS and loaded with ctypes; nothing of it is in liblfmcmc.so.
// The probe kernels call the project's own __device__ functions and do no arithmetic of their own: they load the
// arguments, call, and store what came back.  Workgroups have 256 threads and every global access is guarded by the
// element count.  Every entry point takes host arrays, returns the first HIP error (0: none) and -1 for arguments it
// refuses (among them every index that would leave an array).
#include "../include/lfmcmc.h"

#include <hip/hip_runtime.h>

#include "../lumfuncmcmc_amd/csrc/lf_mock_noise.h"

using namespace lf;

namespace {

constexpr int TPB = MOCK_THREADS;

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
#define MP_CHECK(e) do { const hipError_t e_ = (e); if (e_ != hipSuccess) return (int)e_; } while (0)
int finish(void* host, const Dev& d, size_t bytes) {
    MP_CHECK(hipGetLastError());
    MP_CHECK(hipDeviceSynchronize());
    MP_CHECK(hipMemcpy(host, d.p, bytes, hipMemcpyDeviceToHost));
    return 0;
}
int blocks_for(long long threads) { return (int)((threads + TPB - 1) / TPB); }

// one workgroup per array of n masses: the tile loop of lf_mock_mass and lf_mock_total
__global__ __launch_bounds__(TPB) void probe_cdf(const double* __restrict__ x, int n, double* __restrict__ c, double* __restrict__ total) {
    __shared__ double buf[MOCK_THREADS];
    const double* in = x + (size_t)blockIdx.x * n;
    const double tot = mock_cdf(buf, n, [&](int j) { return in[j]; }, c + (size_t)blockIdx.x * n);
    if (threadIdx.x == 0) total[blockIdx.x] = tot;
}

__global__ __launch_bounds__(TPB) void probe_search(const double* __restrict__ v, int n, const double* __restrict__ t,
                                                    int* __restrict__ idx, int nt) {
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i < nt) idx[i] = mock_search(v, n, t[i]);
}

__global__ __launch_bounds__(TPB) void probe_hat(const double* __restrict__ x0, const double* __restrict__ a, const double* __restrict__ b,
                                                 const double* __restrict__ u, double* __restrict__ y, int n) {
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i < n) y[i] = mock_hat(x0[i], a[i], b[i], u[i]);
}

__global__ __launch_bounds__(TPB) void probe_loggam(const double* __restrict__ x, double* __restrict__ y, int n) {
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i < n) y[i] = mock_loggam(x[i]);
}

__global__ __launch_bounds__(TPB) void probe_poisson(const double* __restrict__ mu, const long long* __restrict__ row_id, int f,
                                                     unsigned long long seed, long long* __restrict__ k, int n) {
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i < n) k[i] = mock_poisson(mu[i], (unsigned long long)row_id[i], f, seed);
}

__global__ __launch_bounds__(TPB) void probe_sigma(const double* __restrict__ nodes, const double* __restrict__ sig, int M,
                                                   const double* __restrict__ t, double* __restrict__ y, int n) {
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i < n) y[i] = mock_sigma(nodes, sig, M, t[i]);
}

__global__ __launch_bounds__(TPB) void probe_logflux(const double* __restrict__ zarr, const double* __restrict__ ld2n, int S,
                                                     const double* __restrict__ z, const double* __restrict__ L,
                                                     double* __restrict__ y, int n) {
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i < n) y[i] = mock_logflux(zarr, ld2n, S, z[i], L[i]);
}

__global__ __launch_bounds__(TPB) void probe_noise(const long long* __restrict__ row_id, const unsigned int* __restrict__ index,
                                                   const int* __restrict__ f, unsigned long long seed, double* __restrict__ y, int n) {
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i < n) y[i] = mock_noise((unsigned long long)row_id[i], index[i], f[i], seed);
}

}  // namespace

extern "C" {

// x: narr arrays of n masses; c: their cumulative sums; total: the sum scans' running totals
int mp_cdf(const double* x, int narr, int n, double* c, double* total) {
    if (narr <= 0 || n <= 0) return -1;
    const size_t bytes = (size_t)narr * n * 8;
    Dev dx(x, bytes), dc(nullptr, bytes), dt(nullptr, (size_t)narr * 8);
    for (const Dev* d : {&dx, &dc, &dt}) MP_CHECK(d->err);
    probe_cdf<<<dim3(narr), dim3(TPB)>>>(dx.as<double>(), n, dc.as<double>(), dt.as<double>());
    const int rc = finish(c, dc, bytes);
    if (rc) return rc;
    MP_CHECK(hipMemcpy(total, dt.p, (size_t)narr * 8, hipMemcpyDeviceToHost));
    return 0;
}

int mp_search(const double* v, int n, const double* t, int* idx, int nt) {
    if (n <= 0 || nt <= 0) return -1;
    Dev dv(v, (size_t)n * 8), dt(t, (size_t)nt * 8), di(nullptr, (size_t)nt * 4);
    for (const Dev* d : {&dv, &dt, &di}) MP_CHECK(d->err);
    probe_search<<<dim3(blocks_for(nt)), dim3(TPB)>>>(dv.as<double>(), n, dt.as<double>(), di.as<int>(), nt);
    return finish(idx, di, (size_t)nt * 4);
}

int mp_hat(const double* x0, const double* a, const double* b, const double* u, double* y, int n) {
    if (n <= 0) return -1;
    const size_t bytes = (size_t)n * 8;
    Dev d0(x0, bytes), da(a, bytes), db(b, bytes), du(u, bytes), dy(nullptr, bytes);
    for (const Dev* d : {&d0, &da, &db, &du, &dy}) MP_CHECK(d->err);
    probe_hat<<<dim3(blocks_for(n)), dim3(TPB)>>>(d0.as<double>(), da.as<double>(), db.as<double>(), du.as<double>(), dy.as<double>(), n);
    return finish(y, dy, bytes);
}

int mp_loggam(const double* x, double* y, int n) {
    if (n <= 0) return -1;
    Dev dx(x, (size_t)n * 8), dy(nullptr, (size_t)n * 8);
    for (const Dev* d : {&dx, &dy}) MP_CHECK(d->err);
    probe_loggam<<<dim3(blocks_for(n)), dim3(TPB)>>>(dx.as<double>(), dy.as<double>(), n);
    return finish(y, dy, (size_t)n * 8);
}

int mp_poisson(const double* mu, const long long* row_id, int f, unsigned long long seed, long long* k, int n) {
    if (n <= 0 || f < 0 || f >= LF_MAX_FIELDS) return -1;
    Dev dm(mu, (size_t)n * 8), dr(row_id, (size_t)n * 8), dk(nullptr, (size_t)n * 8);
    for (const Dev* d : {&dm, &dr, &dk}) MP_CHECK(d->err);
    probe_poisson<<<dim3(blocks_for(n)), dim3(TPB)>>>(dm.as<double>(), dr.as<long long>(), f, seed, dk.as<long long>(), n);
    return finish(k, dk, (size_t)n * 8);
}

// nodes, sig: one field's row of the table, M >= 1 values each
int mp_sigma(const double* nodes, const double* sig, int M, const double* t, double* y, int n) {
    if (M < 1 || M > MOCK_MAX_NODES || n <= 0) return -1;
    Dev dn(nodes, (size_t)M * 8), ds(sig, (size_t)M * 8), dt(t, (size_t)n * 8), dy(nullptr, (size_t)n * 8);
    for (const Dev* d : {&dn, &ds, &dt, &dy}) MP_CHECK(d->err);
    probe_sigma<<<dim3(blocks_for(n)), dim3(TPB)>>>(dn.as<double>(), ds.as<double>(), M, dt.as<double>(), dy.as<double>(), n);
    return finish(y, dy, (size_t)n * 8);
}

int mp_logflux(const double* zarr, const double* ld2n, int S, const double* z, const double* L, double* y, int n) {
    if (S < 2 || n <= 0) return -1;
    Dev dz(zarr, (size_t)S * 8), dl(ld2n, (size_t)S * 8), dq(z, (size_t)n * 8), dL(L, (size_t)n * 8), dy(nullptr, (size_t)n * 8);
    for (const Dev* d : {&dz, &dl, &dq, &dL, &dy}) MP_CHECK(d->err);
    probe_logflux<<<dim3(blocks_for(n)), dim3(TPB)>>>(dz.as<double>(), dl.as<double>(), S, dq.as<double>(), dL.as<double>(), dy.as<double>(), n);
    return finish(y, dy, (size_t)n * 8);
}

int mp_noise(const long long* row_id, const unsigned int* index, const int* f, unsigned long long seed, double* y, int n) {
    if (n <= 0) return -1;
    Dev dr(row_id, (size_t)n * 8), di(index, (size_t)n * 4), df(f, (size_t)n * 4), dy(nullptr, (size_t)n * 8);
    for (const Dev* d : {&dr, &di, &df, &dy}) MP_CHECK(d->err);
    probe_noise<<<dim3(blocks_for(n)), dim3(TPB)>>>(dr.as<long long>(), di.as<unsigned int>(), df.as<int>(), seed, dy.as<double>(), n);
    return finish(y, dy, (size_t)n * 8);
}

int mp_device_count() {
    int n = 0;
    return hipGetDeviceCount(&n) == hipSuccess ? n : 0;
}

}  // extern "C"
