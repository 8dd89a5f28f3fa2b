// lf_hostcall.h - what one call of the host layer (lfmcmc.hip) holds while it runs, besides its buffers (lf_devmem.h): the
// call's error state and its few time stamps.  Host only: no exceptions, no allocator, and it does not set the device.
#pragma once

#include <hip/hip_runtime.h>

#include <string>

#include "../../include/lfmcmc.h"
#include "lf_devmem.h"

// For the calls that return at the first HIP error: `o` (a context, a mock generator) takes the message.
#define LF_HIP(o, call)                                                                    \
    do {                                                                                   \
        hipError_t e_ = (call);                                                            \
        if (e_ != hipSuccess) {                                                            \
            (o)->err = std::string(#call) + ": " + hipGetErrorString(e_);                  \
            return LF_ERR_HIP;                                                             \
        }                                                                                  \
    } while (0)

// Replace `b` by a new allocation of n elements (not initialised; the old contents go).  sync: launches enqueued earlier may
// still use the old one - wait for the device first.  `o`: who takes the error (a context, a mock generator).
template <typename Owner, typename T, bool PINNED>
int grow(Owner* o, Buf<T, PINNED>& b, size_t n, bool sync = true) {
    if (sync) LF_HIP(o, hipDeviceSynchronize());
    LF_HIP(o, b.alloc(n));
    return LF_OK;
}

// alloc_all(buffer, n, buffer, n, ...): a new allocation of n elements for each; stops at the first error and returns it
inline hipError_t alloc_all() { return hipSuccess; }
template <typename T, bool PINNED, typename... Rest>
hipError_t alloc_all(Buf<T, PINNED>& b, size_t n, Rest&&... rest) {
    const hipError_t e = b.alloc(n);
    return e != hipSuccess ? e : alloc_all(rest...);
}

// For the calls that go on after a HIP error (they own buffers and events, and report once, at their end): the first failure
// fixes rc = LF_ERR_HIP - and the message, where the call keeps one - while ok() tells every call's own success to the `&&`
// chain it stands in.  The time stamps are events made when they are first recorded and destroyed with the call.
class HostCall {
    static constexpr int NSTAMP = 4;
    hipEvent_t ev_[NSTAMP] = {nullptr, nullptr, nullptr, nullptr};
    std::string* err_;
    const char* prefix_;

  public:
    int rc = LF_OK;

    explicit HostCall(std::string* err = nullptr, const char* prefix = "") : err_(err), prefix_(prefix) {}
    ~HostCall() {
        for (hipEvent_t e : ev_)
            if (e) hipEventDestroy(e);
    }
    HostCall(const HostCall&) = delete;
    HostCall& operator=(const HostCall&) = delete;

    bool ok(hipError_t e) {
        if (e != hipSuccess && rc == LF_OK) {
            rc = LF_ERR_HIP;
            if (err_) *err_ = std::string(prefix_) + hipGetErrorString(e);
        }
        return e == hipSuccess;
    }
    // record stamp i on stream s
    bool stamp(int i, hipStream_t s) {
        if (!ev_[i] && !ok(hipEventCreate(&ev_[i]))) {
            ev_[i] = nullptr;
            return false;
        }
        return ok(hipEventRecord(ev_[i], s));
    }
    // wait until the device has passed stamp i
    bool wait(int i) { return ok(ev_[i] ? hipEventSynchronize(ev_[i]) : hipErrorInvalidHandle); }
    // the milliseconds between stamps i and j, both recorded and passed; false (and *ms untouched) after any failure of the call
    bool elapsed(int i, int j, double* ms) {
        float t = 0.0f;
        if (rc != LF_OK || !ok(ev_[i] && ev_[j] ? hipEventElapsedTime(&t, ev_[i], ev_[j]) : hipErrorInvalidHandle)) return false;
        *ms = t;
        return true;
    }
};
