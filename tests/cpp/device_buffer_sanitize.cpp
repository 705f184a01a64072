// tests/cpp/device_buffer_sanitize.cpp — the owning buffer types of loc_lib_amd/csrc/device_buffer.hpp against a malloc-backed stand-in
// for the HIP runtime: every block and event the stubs hand out is counted, the k-th allocation or the next copy can be made to fail,
// and what the types do is checked call by call — frees happen once, a failed growth keeps (grow_keep) or empties (alloc) the buffer
// as documented, a group of buffers whose growth failed half-way is complete after the retry. Built with -fsanitize=address,undefined
// by the CPU suite and not linked against the HIP runtime: a block freed twice, leaked or outlived shows up in the sanitizer as well.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>

#include "device_buffer.hpp"

namespace {
int g_live_blocks = 0, g_live_events = 0;
int g_allocs = 0, g_frees = 0, g_events_made = 0, g_events_destroyed = 0, g_syncs = 0;
int g_fail_alloc_in = 0;  // k > 0: the k-th allocation from now fails
bool g_fail_copy = false;

hipError_t stub_alloc(void** p, size_t bytes) {
    if (g_fail_alloc_in > 0 && --g_fail_alloc_in == 0) { *p = nullptr; return hipErrorOutOfMemory; }
    *p = std::malloc(bytes ? bytes : 1);
    ++g_live_blocks;
    ++g_allocs;
    return hipSuccess;
}
hipError_t stub_free(void* p) {
    if (p) { --g_live_blocks; ++g_frees; }
    std::free(p);
    return hipSuccess;
}
}  // namespace

extern "C" {
hipError_t hipMalloc(void** p, size_t bytes) { return stub_alloc(p, bytes); }
hipError_t hipFree(void* p) { return stub_free(p); }
hipError_t hipHostMalloc(void** p, size_t bytes, unsigned int) { return stub_alloc(p, bytes); }
hipError_t hipHostFree(void* p) { return stub_free(p); }
hipError_t hipMemcpyAsync(void* dst, const void* src, size_t bytes, hipMemcpyKind, hipStream_t) {
    if (g_fail_copy) return hipErrorInvalidValue;
    std::memcpy(dst, src, bytes);
    return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t) { ++g_syncs; return hipSuccess; }
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) {
    *e = reinterpret_cast<hipEvent_t>(std::malloc(1));
    ++g_live_events;
    ++g_events_made;
    return hipSuccess;
}
hipError_t hipEventDestroy(hipEvent_t e) {
    --g_live_events;
    ++g_events_destroyed;
    std::free(e);
    return hipSuccess;
}
}

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) { std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); std::exit(1); } \
    } while (0)

using locgpu::DevBuf;
using locgpu::Event;
using locgpu::PinnedBuf;
using locgpu::with_headroom;

template <class Buf>
static void basic_life() {
    const int a0 = g_allocs, f0 = g_frees;
    {
        Buf b;
        CHECK(b.get() == nullptr && b.cap() == 0 && !b);
        CHECK(b.alloc(100) == hipSuccess && b.get() && b.cap() == 100 && g_live_blocks == 1);
        int* p = b.get();
        p[99] = 7;  // the whole block is ours
        CHECK(b.reserve(40) == hipSuccess && b.get() == p && b.cap() == 100 && g_allocs == a0 + 1);  // smaller: nothing happens
        CHECK(b.reserve(100) == hipSuccess && b.get() == p && g_allocs == a0 + 1);
        CHECK(b.reserve(101) == hipSuccess && b.cap() == 101 && g_allocs == a0 + 2 && g_frees == f0 + 1 && g_live_blocks == 1);  // one free, one allocation
        b.get()[100] = 1;
        int* as_pointer = b;  // the implicit conversion kernel launches and argument structs rely on
        CHECK(as_pointer == b.get());
        b.reset();
        CHECK(b.get() == nullptr && b.cap() == 0 && g_live_blocks == 0);
        b.reset();  // idempotent
        CHECK(g_frees == f0 + 2);
        CHECK(b.alloc(8) == hipSuccess);
        // a failed allocation leaves the buffer empty, and the next call simply tries again
        g_fail_alloc_in = 1;
        CHECK(b.reserve(16) == hipErrorOutOfMemory && b.get() == nullptr && b.cap() == 0 && g_live_blocks == 0);
        CHECK(b.reserve(16) == hipSuccess && b.cap() == 16 && g_live_blocks == 1);
    }  // destructor
    CHECK(g_live_blocks == 0);
}

template <class Buf>
static void moves_and_swap() {
    {
        Buf a, b;
        CHECK(a.alloc(10) == hipSuccess && b.alloc(20) == hipSuccess);
        int *pa = a.get(), *pb = b.get();
        Buf c(std::move(a));  // move construction
        CHECK(c.get() == pa && c.cap() == 10 && a.get() == nullptr && a.cap() == 0 && g_live_blocks == 2);
        const int f0 = g_frees;
        b = std::move(c);  // move assignment onto a non-empty buffer: its old block is freed, once
        CHECK(g_frees == f0 + 1 && b.get() == pa && b.cap() == 10 && c.get() == nullptr && c.cap() == 0 && g_live_blocks == 1);
        (void)pb;
        Buf& self = b;
        b = std::move(self);  // self-assignment keeps the block
        CHECK(b.get() == pa && g_live_blocks == 1);
        Buf d;
        CHECK(d.alloc(5) == hipSuccess);
        int* pd = d.get();
        b.swap(d);
        CHECK(b.get() == pd && b.cap() == 5 && d.get() == pa && d.cap() == 10 && g_live_blocks == 2 && g_frees == f0 + 1);
        Buf e;
        e.swap(d);  // with an empty one
        CHECK(e.get() == pa && e.cap() == 10 && d.get() == nullptr && d.cap() == 0);
    }
    CHECK(g_live_blocks == 0);
}

static void grow_keep() {
    {
        DevBuf<int> b;
        const int s0 = g_syncs;
        CHECK(b.grow_keep(4, 0, nullptr) == hipSuccess && b.cap() == 4 && g_syncs == s0);  // nothing to keep: no copy, no synchronisation
        for (int i = 0; i < 4; ++i) b.get()[i] = 10 + i;
        CHECK(b.grow_keep(64, 3, nullptr) == hipSuccess && b.cap() == 64 && g_syncs == s0 + 1 && g_live_blocks == 1);
        CHECK(b.get()[0] == 10 && b.get()[1] == 11 && b.get()[2] == 12);  // the first `used` elements
        b.get()[63] = 1;
        int* p = b.get();
        // the allocation fails: the old block, its contents and cap() are untouched
        g_fail_alloc_in = 1;
        CHECK(b.grow_keep(128, 3, nullptr) == hipErrorOutOfMemory && b.get() == p && b.cap() == 64 && b.get()[2] == 12 && g_live_blocks == 1);
        // the copy fails: the same, and the new block is given back
        g_fail_copy = true;
        CHECK(b.grow_keep(128, 3, nullptr) == hipErrorInvalidValue && b.get() == p && b.cap() == 64 && b.get()[2] == 12 && g_live_blocks == 1);
        g_fail_copy = false;
        CHECK(b.grow_keep(128, 64, nullptr) == hipSuccess && b.cap() == 128 && b.get()[2] == 12 && b.get()[63] == 1 && g_live_blocks == 1);
    }
    CHECK(g_live_blocks == 0);
}

struct Group { DevBuf<int> a, b; PinnedBuf<int> c; DevBuf<double> d, e; };
static hipError_t grow_group(Group& g, size_t n) {  // the shape of the library's ensure_* functions
    LOCGPU_TRY(g.a.alloc(n));
    LOCGPU_TRY(g.b.alloc(n));
    LOCGPU_TRY(g.c.alloc(n));
    LOCGPU_TRY(g.d.alloc(n));
    LOCGPU_TRY(g.e.alloc(n));
    return hipSuccess;
}
static void group_growth() {
    {
        Group g;
        CHECK(grow_group(g, 8) == hipSuccess && g_live_blocks == 5);
        g_fail_alloc_in = 3;
        CHECK(grow_group(g, 32) == hipErrorOutOfMemory);
        CHECK(g.a.cap() == 32 && g.b.cap() == 32 && g.c.cap() == 0 && g.c.get() == nullptr && g.d.cap() == 8 && g.e.cap() == 8 && g_live_blocks == 4);  // nothing leaked
        CHECK(grow_group(g, 32) == hipSuccess);
        CHECK(g.a.cap() == 32 && g.b.cap() == 32 && g.c.cap() == 32 && g.d.cap() == 32 && g.e.cap() == 32 && g_live_blocks == 5);
    }
    CHECK(g_live_blocks == 0);
}

static void events() {
    const int m0 = g_events_made, d0 = g_events_destroyed;
    {
        Event never;
        CHECK(static_cast<hipEvent_t>(never) == nullptr);
        Event e;
        CHECK(e.ensure() == hipSuccess && e.ensure(hipEventDefault) == hipSuccess && g_events_made == m0 + 1 && g_live_events == 1);  // twice: one event
        hipEvent_t raw = e;
        CHECK(raw != nullptr);
        Event f(std::move(e));
        CHECK(static_cast<hipEvent_t>(f) == raw && static_cast<hipEvent_t>(e) == nullptr && g_live_events == 1);
        Event g;
        CHECK(g.ensure() == hipSuccess && g_live_events == 2);
        g = std::move(f);  // g's own event is destroyed, once
        CHECK(static_cast<hipEvent_t>(g) == raw && g_live_events == 1 && g_events_destroyed == d0 + 1);
    }
    CHECK(g_live_events == 0 && g_events_made == m0 + 2 && g_events_destroyed == d0 + 2);  // the one never ensured destroyed nothing
}

int main() {
    basic_life<DevBuf<int>>();
    basic_life<PinnedBuf<int>>();
    moves_and_swap<DevBuf<int>>();
    moves_and_swap<PinnedBuf<int>>();
    grow_keep();
    group_growth();
    events();
    {
        PinnedBuf<int> p;  // the flags argument and the arrow of a host-readable buffer
        CHECK(p.alloc(4, hipHostMallocCoherent) == hipSuccess && p.reserve(2, hipHostMallocCoherent) == hipSuccess && p.cap() == 4);
        struct S { int x; };
        PinnedBuf<S> q;
        CHECK(q.alloc(1) == hipSuccess);
        q->x = 5;
        CHECK(q.get()[0].x == 5);
    }
    static_assert(with_headroom(0) == 1024 && with_headroom(1) == 1025 && with_headroom(300) == 300 + 75 + 1024, "headroom rule");
    const size_t big = (size_t)1 << 31;
    CHECK(with_headroom(0) == 0 + 0 / 4 + 1024 && with_headroom(1) == 1 + 1 / 4 + 1024 && with_headroom(300) == 300 + 300 / 4 + 1024 && with_headroom(big) == big + big / 4 + 1024);
    CHECK(g_live_blocks == 0 && g_live_events == 0 && g_allocs == g_frees && g_events_made == g_events_destroyed);
    std::printf("device_buffer ok: %d blocks, %d events\n", g_allocs, g_events_made);
    return 0;
}
