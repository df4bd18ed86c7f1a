// CPU check of the owner of device allocations (raytracing_weekend_amd/csrc/rtw_devbuf.h DevBuf), compiled with
// g++ -fsanitize=address,undefined and run by tests/test_devbuf_cpu.py. The three runtime functions the header calls are defined
// here, over malloc and free, and keep a record of what was called in which order; no HIP library is linked and no GPU is touched.
// Held: need <= cap does not allocate; growing frees the old block exactly once, after the drain stream was waited for and before
// the new block is made; no stream is waited for when none is given; a refused allocation leaves null and 0 and the next grow
// succeeds; release() twice, destruction after release() and a move free nothing twice; allocations and frees balance at exit
// (the sanitizer's leak check is the second witness). Prints "devbuf_check ok" and returns 0, or says what failed.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <utility>
#include <vector>

#include "../../raytracing_weekend_amd/csrc/rtw_devbuf.h"
using rtwk::DevBuf;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { fails++; fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); } } while (0)

// ---- the stand-ins
struct Event { char what; const void* arg; size_t bytes; };  // 'm' malloc, 'f' free, 's' stream wait
static std::vector<Event> events;
static std::set<const void*> live;
static int refuse_next = 0;                 // that many allocations fail with hipErrorOutOfMemory
static hipError_t sync_result = hipSuccess;  // what a stream wait returns
static size_t n_malloc = 0, n_free = 0, n_sync = 0, bad_frees = 0;

extern "C" hipError_t hipMalloc(void** ptr, size_t size) {
    if (refuse_next > 0) {
        refuse_next--;
        *ptr = (void*)(uintptr_t)0xdead0;  // a refusing runtime may leave anything here
        return hipErrorOutOfMemory;
    }
    *ptr = malloc(size ? size : 1);
    memset(*ptr, 0xab, size);
    live.insert(*ptr);
    events.push_back(Event{'m', *ptr, size});
    n_malloc++;
    return hipSuccess;
}
extern "C" hipError_t hipFree(void* ptr) {
    events.push_back(Event{'f', ptr, 0});
    n_free++;
    if (!live.erase(ptr)) { bad_frees++; return hipErrorInvalidValue; }  // null, twice, or never allocated
    free(ptr);
    return hipSuccess;
}
extern "C" hipError_t hipStreamSynchronize(hipStream_t stream) {
    events.push_back(Event{'s', (const void*)stream, 0});
    n_sync++;
    return sync_result;
}

static const hipStream_t kStreamA = (hipStream_t)(uintptr_t)0x1000, kStreamB = (hipStream_t)(uintptr_t)0x2000;

static void growth() {
    DevBuf b;
    CHECK(!b && b.as<char>() == nullptr && b.cap() == 0);
    CHECK(b.grow(0, 0) == hipSuccess && events.empty() && !b);  // nothing needed, nothing made
    CHECK(b.grow(10, 160) == hipSuccess && b && b.cap() == 10);
    CHECK(events.size() == 1 && events[0].what == 'm' && events[0].bytes == 160 && events[0].arg == b.as<void>());
    float* const first = b.as<float>();
    first[39] = 1.0f;  // the last of the 160 bytes are its own
    // enough already: no call at all, the same block (the capacity's unit is the caller's: 10 of anything, not 160)
    CHECK(b.grow(10, 999) == hipSuccess && b.grow(3, 1) == hipSuccess && b.grow(0, 0) == hipSuccess && b.grow(7, 7, &kStreamA) == hipSuccess);
    CHECK(events.size() == 1 && b.as<float>() == first && b.cap() == 10);
    // more, no drain: the old block freed once, then the new one made; no stream waited for
    events.clear();
    CHECK(b.grow(11, 32) == hipSuccess && b.cap() == 11);
    CHECK(events.size() == 2 && events[0].what == 'f' && events[0].arg == first && events[1].what == 'm' && events[1].bytes == 32);
    CHECK(n_sync == 0);
    // more, with a drain: that stream waited for first, then free, then malloc
    const void* const second = b.as<void>();
    events.clear();
    CHECK(b.grow(100, 64, &kStreamB) == hipSuccess && b.cap() == 100);
    CHECK(events.size() == 3 && events[0].what == 's' && events[0].arg == (const void*)kStreamB && events[1].what == 'f' && events[1].arg == second &&
          events[2].what == 'm' && events[2].bytes == 64 && events[2].arg == b.as<void>());
    // a drain that fails: its error, and the buffer as it was
    const void* const third = b.as<void>();
    events.clear();
    sync_result = hipErrorUnknown;
    CHECK(b.grow(101, 128, &kStreamA) == hipErrorUnknown && b.as<void>() == third && b.cap() == 100);
    CHECK(events.size() == 1 && events[0].what == 's');
    sync_result = hipSuccess;
    CHECK(live.size() == 1);
}  // (the destructor frees the third block)

static void refusal() {
    DevBuf b;
    CHECK(b.grow(4, 64) == hipSuccess);
    const void* const old = b.as<void>();
    events.clear();
    refuse_next = 1;
    CHECK(b.grow(8, 128) == hipErrorOutOfMemory);  // (the code HIP_TRY maps to RTW_ERR_OOM)
    CHECK(!b && b.as<void>() == nullptr && b.cap() == 0);
    CHECK(events.size() == 1 && events[0].what == 'f' && events[0].arg == old && live.empty());
    // the next grow starts from nothing: no free, one allocation, even for less than was held before
    events.clear();
    CHECK(b.grow(2, 16) == hipSuccess && b && b.cap() == 2);
    CHECK(events.size() == 1 && events[0].what == 'm' && events[0].bytes == 16);
    // refused on an empty buffer: still empty, nothing freed
    DevBuf e;
    events.clear();
    refuse_next = 1;
    CHECK(e.grow(1, 1) == hipErrorOutOfMemory && !e && e.cap() == 0 && events.empty());
}

static void release_and_scope() {
    const size_t f0 = n_free;
    {
        DevBuf b;
        CHECK(b.grow(1, 8) == hipSuccess);
        b.release();
        CHECK(!b && b.cap() == 0 && n_free == f0 + 1);
        b.release();
        CHECK(n_free == f0 + 1);  // nothing to free, no call
    }
    CHECK(n_free == f0 + 1);  // nor by the destructor
    {
        DevBuf b;  // never grown
    }
    CHECK(n_free == f0 + 1);
    {   // per-call scratch: every way out of the scope frees it once
        DevBuf a, b;
        CHECK(a.grow(1, 8) == hipSuccess && b.grow(1, 8) == hipSuccess);
    }
    CHECK(n_free == f0 + 3 && live.empty());
    {   // released and used again
        DevBuf b;
        CHECK(b.grow(5, 40) == hipSuccess);
        b.release();
        CHECK(b.grow(1, 8) == hipSuccess && b.cap() == 1);
    }
    CHECK(n_free == f0 + 5 && live.empty());
}

// a struct with a DevBuf member is reset by value (rtw_hip.hip: c->acc = rtw_ctx::Accum{})
struct Session { bool active = false; DevBuf slab; float* view = nullptr; };
static void moves() {
    const size_t f0 = n_free;
    Session s;
    CHECK(s.slab.grow(3, 48) == hipSuccess);
    s.active = true; s.view = s.slab.as<float>();
    s = Session{};
    CHECK(!s.active && !s.slab && s.slab.cap() == 0 && s.view == nullptr && n_free == f0 + 1 && live.empty());
    s = Session{};
    CHECK(n_free == f0 + 1);
    DevBuf a;
    CHECK(a.grow(2, 16) == hipSuccess);
    const void* const p = a.as<void>();
    DevBuf b(std::move(a));
    CHECK(!a && a.cap() == 0 && b.as<void>() == p && b.cap() == 2);
    DevBuf c;
    CHECK(c.grow(1, 8) == hipSuccess);
    c = std::move(b);  // frees what c held, takes b's
    CHECK(!b && c.as<void>() == p && c.cap() == 2 && n_free == f0 + 2 && live.size() == 1);
    DevBuf& self = c;
    c = std::move(self);
    CHECK(c.as<void>() == p && c.cap() == 2 && n_free == f0 + 2);
}

int main() {
    growth();
    CHECK(live.empty());
    refusal();
    CHECK(live.empty());
    release_and_scope();
    moves();
    CHECK(live.empty() && bad_frees == 0);
    CHECK(n_malloc == n_free && n_malloc > 0);  // every block freed, none twice, null never passed
    if (fails) return 1;
    printf("devbuf_check ok (%zu allocations, %zu frees, %zu stream waits)\n", n_malloc, n_free, n_sync);
    return 0;
}
