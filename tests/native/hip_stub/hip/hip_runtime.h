/* A stand-in for <hip/hip_runtime.h> on the CPU, for tests/native/owned_selftest.cpp only: the runtime calls that
 * csrc/dev_owned.h makes, backed by malloc / free and counted, with a switch that fails the next allocation or copy. */
#pragma once
#include <cstddef>
#include <cstdlib>
#include <cstring>

typedef int hipError_t;
enum { hipSuccess = 0, hipErrorOutOfMemory = 2, hipErrorUnknown = 999 };
enum hipMemcpyKind { hipMemcpyHostToDevice = 1 };
enum { hipHostMallocDefault = 0, hipEventDefault = 0, hipEventDisableTiming = 2, hipStreamNonBlocking = 1 };
typedef struct ihipStream_t *hipStream_t;
typedef struct ihipEvent_t *hipEvent_t;
struct ihipStream_t { int unused; };
struct ihipEvent_t { int unused; };

struct HipStub {
    long dev_alloc = 0, dev_free = 0, host_alloc = 0, host_free = 0;
    long ev_create = 0, ev_destroy = 0, st_create = 0, st_destroy = 0, copies = 0;
    bool fail_next_alloc = false, fail_next_copy = false;
};
inline HipStub &hip_stub()
{
    static HipStub s;
    return s;
}

inline hipError_t hipMalloc(void **p, size_t bytes)
{
    HipStub &s = hip_stub();
    if (s.fail_next_alloc) {
        s.fail_next_alloc = false;
        *p = nullptr;
        return hipErrorOutOfMemory;
    }
    *p = std::malloc(bytes ? bytes : 1);
    ++s.dev_alloc;
    return hipSuccess;
}
inline hipError_t hipFree(void *p)
{
    std::free(p);
    ++hip_stub().dev_free;
    return hipSuccess;
}
inline hipError_t hipHostMalloc(void **p, size_t bytes, unsigned)
{
    HipStub &s = hip_stub();
    if (s.fail_next_alloc) {
        s.fail_next_alloc = false;
        *p = nullptr;
        return hipErrorOutOfMemory;
    }
    *p = std::malloc(bytes ? bytes : 1);
    ++s.host_alloc;
    return hipSuccess;
}
inline hipError_t hipHostFree(void *p)
{
    std::free(p);
    ++hip_stub().host_free;
    return hipSuccess;
}
inline hipError_t hipMemcpy(void *dst, const void *src, size_t bytes, hipMemcpyKind)
{
    HipStub &s = hip_stub();
    if (s.fail_next_copy) {
        s.fail_next_copy = false;
        return hipErrorUnknown;
    }
    std::memcpy(dst, src, bytes);
    ++s.copies;
    return hipSuccess;
}
inline hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned)
{
    *e = new ihipEvent_t{0};
    ++hip_stub().ev_create;
    return hipSuccess;
}
inline hipError_t hipEventDestroy(hipEvent_t e)
{
    delete e;
    ++hip_stub().ev_destroy;
    return hipSuccess;
}
inline hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned)
{
    *s = new ihipStream_t{0};
    ++hip_stub().st_create;
    return hipSuccess;
}
inline hipError_t hipStreamDestroy(hipStream_t s)
{
    delete s;
    ++hip_stub().st_destroy;
    return hipSuccess;
}
