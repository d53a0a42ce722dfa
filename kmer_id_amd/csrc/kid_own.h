// kid_own.h -- owners of the HIP resources the host library holds (host only, no kernels).
// Each is non-copyable, movable (the source is left empty) and gives its resource back in its destructor, errors
// ignored.  The destructors call the HIP runtime: whoever deletes a handle selects the handle's device first.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

// device memory
struct KidDevBuf {
    void *p = nullptr;
    size_t cap = 0; // bytes
    KidDevBuf() {}
    KidDevBuf(const KidDevBuf &) = delete;
    KidDevBuf &operator=(const KidDevBuf &) = delete;
    KidDevBuf(KidDevBuf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    KidDevBuf &operator=(KidDevBuf &&o) noexcept
    {
        if (this != &o) { reset(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; }
        return *this;
    }
    ~KidDevBuf() { reset(); }
    void reset()
    {
        if (p) (void)hipFree(p);
        p = nullptr; cap = 0;
    }
    hipError_t alloc(size_t nbytes)
    {
        reset();
        if (nbytes == 0) nbytes = 16;
        const hipError_t e = hipMalloc(&p, nbytes);
        if (e == hipSuccess) cap = nbytes;
        else p = nullptr;
        return e;
    }
    // grow-only: room for `need` bytes, `alloc_bytes` (>= need: the caller's slack) of them if it has to be replaced.
    // The contents are not kept, and whether the device must be idle first is the caller's business.
    hipError_t ensure(size_t need, size_t alloc_bytes) { return need <= cap ? hipSuccess : alloc(alloc_bytes); }
    template <class T> T *as() const { return static_cast<T *>(p); }
};

struct KidEvent {
    hipEvent_t e = nullptr;
    KidEvent() {}
    KidEvent(const KidEvent &) = delete;
    KidEvent &operator=(const KidEvent &) = delete;
    KidEvent(KidEvent &&o) noexcept : e(o.e) { o.e = nullptr; }
    KidEvent &operator=(KidEvent &&o) noexcept
    {
        if (this != &o) { reset(); e = o.e; o.e = nullptr; }
        return *this;
    }
    ~KidEvent() { reset(); }
    void reset()
    {
        if (e) (void)hipEventDestroy(e);
        e = nullptr;
    }
    hipError_t create() { reset(); return hipEventCreate(&e); }
    hipError_t create(unsigned flags) { reset(); return hipEventCreateWithFlags(&e, flags); }
};

struct KidStream {
    hipStream_t s = nullptr;
    KidStream() {}
    KidStream(const KidStream &) = delete;
    KidStream &operator=(const KidStream &) = delete;
    ~KidStream() { if (s) (void)hipStreamDestroy(s); }
    hipError_t create(unsigned flags = hipStreamDefault) { return hipStreamCreateWithFlags(&s, flags); }
};

// host memory the device can address (hipHostMalloc)
struct KidMappedHost {
    void *p = nullptr;
    KidMappedHost() {}
    KidMappedHost(const KidMappedHost &) = delete;
    KidMappedHost &operator=(const KidMappedHost &) = delete;
    ~KidMappedHost() { if (p) (void)hipHostFree(p); }
    hipError_t alloc(size_t nbytes, unsigned flags) { return hipHostMalloc(&p, nbytes, flags); }
};
