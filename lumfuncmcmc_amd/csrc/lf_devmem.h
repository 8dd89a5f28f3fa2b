// lf_devmem.h - the one owner of a device or pinned-host allocation of the host layer (lfmcmc.hip).  Host only.
//
// A Buf is freed exactly once, by whoever holds it: move-only, no reference count, no allocator, no exceptions.  It neither
// sets the device nor synchronises: its holder does (as before a context is deleted, or before a buffer in use is replaced).
//
// Style: a Buf converts implicitly to its raw pointer, so it is written wherever the pointer was (kernel arguments, the
// argument structs of the device headers, hipMemcpy, arithmetic, tests for NULL).  get() is for the one place where no
// conversion is looked for: a cast to another pointer type.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>

template <typename T, bool PINNED = false>
class Buf {
    T* p_ = nullptr;
    size_t n_ = 0;          // elements allocated (the capacity)

  public:
    Buf() = default;
    ~Buf() { reset(); }
    Buf(Buf&& o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr, o.n_ = 0; }
    Buf& operator=(Buf&& o) noexcept {
        if (this != &o) {
            reset();
            p_ = o.p_, n_ = o.n_;
            o.p_ = nullptr, o.n_ = 0;
        }
        return *this;
    }
    Buf(const Buf&) = delete;
    Buf& operator=(const Buf&) = delete;

    T* get() const { return p_; }
    operator T*() const { return p_; }
    size_t size() const { return n_; }

    void reset() {
        if (p_ && PINNED) hipHostFree(p_);
        else if (p_) hipFree(p_);
        p_ = nullptr;
        n_ = 0;
    }
    // a new allocation of max(n, 1) elements, not initialised; the old one goes first, and a failure leaves the Buf empty
    hipError_t alloc(size_t n) {
        reset();
        n = std::max<size_t>(n, 1);
        const hipError_t e = PINNED ? hipHostMalloc((void**)&p_, n * sizeof(T), hipHostMallocDefault) : hipMalloc((void**)&p_, n * sizeof(T));
        if (e != hipSuccess) p_ = nullptr;
        else n_ = n;
        return e;
    }
    // alloc(n), then a synchronous copy of n elements from the host
    hipError_t upload(const T* src, size_t n) {
        const hipError_t e = alloc(n);
        return e == hipSuccess && n ? hipMemcpy(p_, src, n * sizeof(T), hipMemcpyHostToDevice) : e;
    }
};
