// dev_owned.h -- the owners of everything a polar_ctx or polar_group holds on the HIP runtime: device buffers, fixed
// tables, pinned host memory, events, streams.  Each type is move-only, releases what it holds in its destructor, and is
// empty after reset() or after it was moved from.  Only HIP runtime calls: nothing of the project is included, so that
// tests/native/owned_selftest.cpp can run these types on the CPU against a stub runtime.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <utility>

#ifndef POLAR_ENOMEM   // the codes of include/polar_hip.h, for a build without it
#define POLAR_OK 0
#define POLAR_ENOMEM (-2)
#define POLAR_EDEVICE (-3)
#endif

// A growable device buffer (ensure() in polar_host.h) and the job counter of the persistent kernels that use it as scratch
// (work_queue() there).
struct Buf {
    void *p = nullptr;
    size_t cap = 0;
    unsigned *queue = nullptr;

    Buf() = default;
    Buf(Buf &&o) noexcept : p(o.p), cap(o.cap), queue(o.queue) { o.forget(); }
    Buf &operator=(Buf &&o) noexcept
    {
        if (this != &o) {
            reset();
            p = o.p, cap = o.cap, queue = o.queue;
            o.forget();
        }
        return *this;
    }
    ~Buf() { reset(); }
    void reset()
    {
        if (p) (void)hipFree(p);
        if (queue) (void)hipFree(queue);
        forget();
    }

private:
    void forget() { p = nullptr, cap = 0, queue = nullptr; }
};

// A device table of fixed size: allocated once, filled from the host.
template <typename T>
struct DevMem {
    DevMem() = default;
    DevMem(DevMem &&o) noexcept : p(std::exchange(o.p, nullptr)) {}
    DevMem &operator=(DevMem &&o) noexcept
    {
        if (this != &o) {
            reset();
            p = std::exchange(o.p, nullptr);
        }
        return *this;
    }
    ~DevMem() { reset(); }
    void reset()
    {
        if (p) (void)hipFree(p);
        p = nullptr;
    }
    T *get() const { return p; }
    operator T *() const { return p; }
    explicit operator bool() const { return p != nullptr; }

    // room for n elements, uninitialised (whatever was held is released first)
    hipError_t alloc(size_t n)
    {
        reset();
        const hipError_t e = hipMalloc(reinterpret_cast<void **>(&p), n * sizeof(T));
        if (e != hipSuccess) p = nullptr;
        return e;
    }
    // host[0..n) -> the table, synchronously; allocates n elements if empty.  POLAR_ENOMEM when the allocation fails,
    // POLAR_EDEVICE when the copy does; both leave the object empty.  *why (optional) receives the runtime's error.
    int upload(const T *host, size_t n, hipError_t *why = nullptr)
    {
        hipError_t e = p ? hipSuccess : alloc(n);
        int rc = e == hipSuccess ? POLAR_OK : POLAR_ENOMEM;
        if (!rc && n && (e = hipMemcpy(p, host, n * sizeof(T), hipMemcpyHostToDevice)) != hipSuccess) {
            reset();
            rc = POLAR_EDEVICE;
        }
        if (why) *why = e;
        return rc;
    }

private:
    T *p = nullptr;
};

// Pinned host memory that only grows.
template <typename T>
struct PinnedMem {
    PinnedMem() = default;
    PinnedMem(PinnedMem &&o) noexcept : p(std::exchange(o.p, nullptr)), bytes(std::exchange(o.bytes, 0)) {}
    PinnedMem &operator=(PinnedMem &&o) noexcept
    {
        if (this != &o) {
            reset();
            p = std::exchange(o.p, nullptr);
            bytes = std::exchange(o.bytes, 0);
        }
        return *this;
    }
    ~PinnedMem() { reset(); }
    void reset()
    {
        if (p) (void)hipHostFree(p);
        p = nullptr;
        bytes = 0;
    }
    T *get() const { return p; }
    operator T *() const { return p; }
    explicit operator bool() const { return p != nullptr; }
    size_t size_bytes() const { return bytes; }

    // at least `need` bytes; the contents are not kept when it grows.  A failure leaves the object empty.
    hipError_t ensure(size_t need)
    {
        if (bytes >= need) return hipSuccess;
        reset();
        const hipError_t e = hipHostMalloc(reinterpret_cast<void **>(&p), need, hipHostMallocDefault);
        if (e != hipSuccess) p = nullptr;
        else bytes = need;
        return e;
    }

private:
    T *p = nullptr;
    size_t bytes = 0;
};

struct Event {
    Event() = default;
    Event(Event &&o) noexcept : e(std::exchange(o.e, nullptr)) {}
    Event &operator=(Event &&o) noexcept
    {
        if (this != &o) {
            reset();
            e = std::exchange(o.e, nullptr);
        }
        return *this;
    }
    ~Event() { reset(); }
    void reset()
    {
        if (e) (void)hipEventDestroy(e);
        e = nullptr;
    }
    hipError_t create(unsigned flags)
    {
        reset();
        const hipError_t r = hipEventCreateWithFlags(&e, flags);
        if (r != hipSuccess) e = nullptr;
        return r;
    }
    hipEvent_t get() const { return e; }
    operator hipEvent_t() const { return e; }
    explicit operator bool() const { return e != nullptr; }

private:
    hipEvent_t e = nullptr;
};

// A stream the object created (owned: destroyed with it) or one it borrows (adopt(): never destroyed here).
struct Stream {
    Stream() = default;
    Stream(Stream &&o) noexcept : s(std::exchange(o.s, nullptr)), owned(std::exchange(o.owned, false)) {}
    Stream &operator=(Stream &&o) noexcept
    {
        if (this != &o) {
            reset();
            s = std::exchange(o.s, nullptr);
            owned = std::exchange(o.owned, false);
        }
        return *this;
    }
    ~Stream() { reset(); }
    void reset()
    {
        if (owned && s) (void)hipStreamDestroy(s);
        s = nullptr;
        owned = false;
    }
    hipError_t create(unsigned flags)
    {
        reset();
        const hipError_t r = hipStreamCreateWithFlags(&s, flags);
        if (r != hipSuccess) s = nullptr;
        owned = s != nullptr;
        return r;
    }
    void adopt(hipStream_t foreign)   // the null stream included
    {
        reset();
        s = foreign;
    }
    bool is_owned() const { return owned; }
    hipStream_t get() const { return s; }
    operator hipStream_t() const { return s; }
    explicit operator bool() const { return s != nullptr; }

private:
    hipStream_t s = nullptr;
    bool owned = false;
};
