// owned_selftest.cpp -- the owning types of polardecoding_amd/csrc/dev_owned.h on the CPU, against the stub runtime of
// tests/native/hip_stub (malloc / free and counters).  Built with -fsanitize=address,undefined and run as a program of its
// own by tests/test_owned_host.py: a double free, a use after free or a leak ends it with a report, a resource released
// the wrong number of times fails a CHECK.  Prints "owned_selftest: ok".
#include "../../polardecoding_amd/csrc/dev_owned.h"

#include <cstdint>
#include <cstdio>
#include <type_traits>
#include <utility>

#define CHECK(x)                                                          \
    do {                                                                  \
        if (!(x)) {                                                       \
            std::printf("owned_selftest: %s:%d: %s\n", __FILE__, __LINE__, #x); \
            std::exit(1);                                                 \
        }                                                                 \
    } while (0)

template <typename T>
constexpr bool move_only = !std::is_copy_constructible<T>::value && !std::is_copy_assignable<T>::value &&
                           std::is_nothrow_move_constructible<T>::value && std::is_nothrow_move_assignable<T>::value;
static_assert(move_only<Buf> && move_only<DevMem<uint32_t>> && move_only<PinnedMem<double>> && move_only<Event> &&
                  move_only<Stream>,
              "every owner is move-only");

static HipStub &S = hip_stub();

// what ensure() / work_queue() of polar_host.h do to a Buf
static void fill(Buf &b, size_t bytes, bool with_queue)
{
    CHECK(hipMalloc(&b.p, bytes) == hipSuccess);
    b.cap = bytes;
    if (with_queue) CHECK(hipMalloc(reinterpret_cast<void **>(&b.queue), 256) == hipSuccess);
}

static void test_buf()
{
    const long a0 = S.dev_alloc, f0 = S.dev_free;
    {
        Buf empty;   // construct - destroy, empty and full
        Buf b;
        fill(b, 64, true);
    }
    CHECK(S.dev_alloc - a0 == 2 && S.dev_free - f0 == 2);
    {
        Buf a, b;
        fill(a, 32, true);
        fill(b, 48, false);
        void *ap = a.p, *bp = b.p;
        unsigned *aq = a.queue;
        std::swap(a, b);   // nothing is released, everything changes sides
        CHECK(S.dev_free - f0 == 2);
        CHECK(a.p == bp && a.cap == 48 && a.queue == nullptr);
        CHECK(b.p == ap && b.cap == 32 && b.queue == aq);
        Buf c(std::move(b));   // move-construct: b is empty
        CHECK(b.p == nullptr && b.cap == 0 && b.queue == nullptr && c.p == ap && c.queue == aq);
        a = std::move(c);      // move-assign onto a non-empty object: the old buffer is released once
        CHECK(S.dev_free - f0 == 3);
        CHECK(a.p == ap && a.cap == 32 && a.queue == aq && c.p == nullptr && c.queue == nullptr);
        Buf &self = a;
        a = std::move(self);   // onto itself: nothing happens
        CHECK(a.p == ap && S.dev_free - f0 == 3);
        a.reset();
        CHECK(S.dev_free - f0 == 5 && a.p == nullptr && a.cap == 0 && a.queue == nullptr);
        a.reset();             // twice
        CHECK(S.dev_free - f0 == 5);
    }
    CHECK(S.dev_alloc - a0 == 5 && S.dev_free - f0 == 5);
}

static void test_devmem()
{
    const long a0 = S.dev_alloc, f0 = S.dev_free;
    const uint32_t src[4] = {1, 2, 3, 4};
    {
        DevMem<uint32_t> empty;
        CHECK(!empty && empty.get() == nullptr);
        DevMem<uint32_t> t;
        CHECK(t.upload(src, 4) == POLAR_OK && t && t.get()[3] == 4);
        uint32_t *raw = t;   // implicit T*
        CHECK(raw == t.get());
        const uint32_t again[4] = {5, 6, 7, 8};
        CHECK(t.upload(again, 4) == POLAR_OK && t.get() == raw && raw[0] == 5);   // non-empty: copies only
        CHECK(S.dev_alloc - a0 == 1);
        DevMem<uint32_t> u(std::move(t));
        CHECK(!t && u.get() == raw);
        DevMem<uint32_t> v;
        CHECK(v.upload(src, 4) == POLAR_OK);
        v = std::move(u);   // onto a non-empty object
        CHECK(S.dev_free - f0 == 1 && v.get() == raw && !u);
        v.reset();
        v.reset();
        CHECK(S.dev_free - f0 == 2 && !v);
        CHECK(v.alloc(16) == hipSuccess && v);   // alloc, then upload into it
        CHECK(v.upload(src, 0) == POLAR_OK && v);
    }
    CHECK(S.dev_alloc - a0 == 3 && S.dev_free - f0 == 3);
    {
        DevMem<uint32_t> t;
        hipError_t why = hipSuccess;
        S.fail_next_alloc = true;
        CHECK(t.upload(src, 4, &why) == POLAR_ENOMEM && !t && why == hipErrorOutOfMemory);
        CHECK(S.dev_alloc - a0 == 3 && S.dev_free - f0 == 3);
        S.fail_next_copy = true;
        CHECK(t.upload(src, 4, &why) == POLAR_EDEVICE && !t && why == hipErrorUnknown);
        CHECK(S.dev_alloc - a0 == 4 && S.dev_free - f0 == 4);   // the allocation of the failed upload went back
        S.fail_next_alloc = true;
        CHECK(t.alloc(4) == hipErrorOutOfMemory && !t);
    }
    CHECK(S.dev_alloc - a0 == 4 && S.dev_free - f0 == 4);
}

static void test_pinned()
{
    const long a0 = S.host_alloc, f0 = S.host_free;
    {
        PinnedMem<double> empty;
        PinnedMem<double> m;
        CHECK(m.ensure(64) == hipSuccess && m && m.size_bytes() == 64);
        double *p = m;
        CHECK(m.ensure(32) == hipSuccess && m.get() == p);   // large enough already
        CHECK(m.ensure(128) == hipSuccess && m.size_bytes() == 128);
        CHECK(S.host_alloc - a0 == 2 && S.host_free - f0 == 1);
        p = m;
        PinnedMem<double> n(std::move(m));
        CHECK(!m && m.size_bytes() == 0 && n.get() == p);
        PinnedMem<double> o;
        CHECK(o.ensure(8) == hipSuccess);
        o = std::move(n);
        CHECK(S.host_free - f0 == 2 && o.get() == p && o.size_bytes() == 128 && !n);
        S.fail_next_alloc = true;
        CHECK(o.ensure(256) == hipErrorOutOfMemory && !o && o.size_bytes() == 0);
        CHECK(S.host_free - f0 == 3);
        o.reset();
        o.reset();
    }
    CHECK(S.host_alloc - a0 == 3 && S.host_free - f0 == 3);
}

static void test_event()
{
    const long c0 = S.ev_create, d0 = S.ev_destroy;
    {
        Event empty;
        CHECK(!empty);
        Event e;
        CHECK(e.create(hipEventDisableTiming) == hipSuccess && e);
        hipEvent_t raw = e;
        Event f(std::move(e));
        CHECK(!e && f.get() == raw);
        Event g;
        CHECK(g.create(hipEventDefault) == hipSuccess);
        g = std::move(f);
        CHECK(S.ev_destroy - d0 == 1 && g.get() == raw && !f);
        CHECK(g.create(hipEventDefault) == hipSuccess);   // create on a live event: the old one goes first
        CHECK(S.ev_destroy - d0 == 2);
        g.reset();
        g.reset();
        CHECK(S.ev_destroy - d0 == 3 && !g);
    }
    CHECK(S.ev_create - c0 == 3 && S.ev_destroy - d0 == 3);
}

static void test_stream()
{
    const long c0 = S.st_create, d0 = S.st_destroy;
    ihipStream_t foreign_obj{0};
    hipStream_t foreign = &foreign_obj;   // on the stack: destroying it would be an invalid delete
    {
        Stream empty;
        CHECK(!empty && !empty.is_owned());
        Stream s;
        CHECK(s.create(hipStreamNonBlocking) == hipSuccess && s && s.is_owned());
        hipStream_t raw = s;
        Stream t(std::move(s));
        CHECK(!s && !s.is_owned() && t.get() == raw && t.is_owned());
        Stream u;
        CHECK(u.create(hipStreamNonBlocking) == hipSuccess);
        u = std::move(t);
        CHECK(S.st_destroy - d0 == 1 && u.get() == raw && u.is_owned() && !t);
        u.adopt(foreign);   // polar_set_stream: the owned stream is destroyed, the foreign one borrowed
        CHECK(S.st_destroy - d0 == 2 && u.get() == foreign && !u.is_owned());
        Stream v(std::move(u));   // a borrowed stream stays borrowed when moved
        CHECK(v.get() == foreign && !v.is_owned());
        Stream w;
        CHECK(w.create(hipStreamNonBlocking) == hipSuccess);
        std::swap(v, w);          // the lanes swap an owned stream with a borrowed one
        CHECK(v.is_owned() && w.get() == foreign && !w.is_owned() && S.st_destroy - d0 == 2);
        w.reset();
        w.reset();
        CHECK(S.st_destroy - d0 == 2);   // the foreign handle was never destroyed
        w.adopt(foreign);
    }
    CHECK(S.st_create - c0 == 3 && S.st_destroy - d0 == 3);
}

int main()
{
    test_buf();
    test_devmem();
    test_pinned();
    test_event();
    test_stream();
    CHECK(S.dev_alloc == S.dev_free && S.dev_alloc > 0);
    CHECK(S.host_alloc == S.host_free && S.host_alloc > 0);
    CHECK(S.ev_create == S.ev_destroy && S.ev_create > 0);
    CHECK(S.st_create == S.st_destroy && S.st_create > 0);
    std::printf("owned_selftest: ok\n");
    return 0;
}
