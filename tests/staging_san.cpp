// Host-only driver of fem-elastoplasticity_amd/csrc/fep_staging.h for the sanitizer builds (tests/test_host_sanitizers.py:
// g++ -fsanitize=address,undefined and -fsanitize=thread, FEP_COPY_THREADS = 1, 3 and 6; CPU only).  The header's seven kinds
// of HIP calls are replaced by the host stand-ins below (FEP_STAGING_HOST_STUB): "device" memory is heap memory, and
// `g_fail_copy_after` / `g_fail_host_malloc` make the n-th copy / the next pinned allocation fail.
//
// The stand-ins DEFER every copy to the latest moment the API allows: hipMemcpyAsync only queues the copy on its stream,
// hipEventRecord notes the queue position, and hipEventSynchronize / hipStreamSynchronize then run the queued copies up to
// that position.  A slot that is refilled without waiting for its event, an event recorded before the copy it guards, or a
// parked chunk that never leaves its slot therefore changes the bytes that arrive, on every run (with synchronous copies none
// of them does).  A "kernel" is a function queued on the stream the same way (stub_launch).
//   1. PinnedCache: reuse by size, double release refused, trim, allocation failure -> idle blocks given back -> retry
//   2. CopyPool: copy / interleave2 from two threads at once (the pool is process-wide; ADVICE r2: jobs overwrote each other)
//   3. Engine: pageable round trips through the ring; a copy that fails after a device -> host chunk was parked must leave
//      no pending destination behind (the failed call's output array is freed right after: ASan sees any later write)
//   4. two engines driven by two threads
//   5. pageable transfers LONGER THAN THE RING, each direction alone and both together, at 0, 1, 8, slot - 8, slot, slot + 8,
//      ring, ring + 8 and 5.5 slots + 1 bytes; h2d_interleave2 at 1, per - 1, per, per + 1, 4 per + 1 and 5 per + 1337 nodes
//   6. a call shaped like return_map_host_impl, made through the scope that function uses (HostCall: seven inputs of unequal
//      sizes, a kernel, five outputs; pinned blocks, views into the middle of one, pageable arrays 8 bytes off their
//      allocation, one pageable array both input and output), four times back to back so that the ring starts at each of
//      its four positions
//   7. small -> large -> small calls on one engine (DeviceStore's grow path), and a buffer that grows while a copy into
//      its old block is still queued
//   8. a call shaped like the mesh host forms (HostCall on a ScopedStore of the call: two pageable inputs, a kernel, three
//      outputs of which one is NULL), four times back to back, the device blocks released after each; then once with a copy
//      that fails after a device -> host chunk was queued, while copies into the call's blocks are still queued
//   9. stream_scratch: a smaller need returns the same block, growth returns a new one and leaves the old one allocated, a
//      capturing stream is refused with nothing allocated
//  10. DeviceArray (fep_solver_levels.h, the solver's device memory; the stand-ins add a synchronous hipMemcpy and
//      `g_fail_dev_malloc_after`, which makes the n-th device allocation from now fail): move-construct and move-assign empty
//      the source and free the overwritten block, a failed alloc leaves the array empty, every block is freed in the end
//  11. the upload of a multigrid level (push_level, with build_transfer_blocks at BF = 2 and 3) on a hierarchy of 12 -> 6 -> 3
//      DOFs: every one of a push's device allocations made to fail in turn — FEP_ENOMEM, the level count and the live blocks
//      as before the call, t0 / q / k32 all set or all empty — then the push itself, the node blocks against the prolongation;
//      a push after the last level (FEP_ESTATE), a column index out of range (FEP_ERANGE, nothing left allocated), drop_levels,
//      and the live blocks back at their starting count after destruction
// Every check of 5 - 8 compares every byte of the result, and every destination ends in a canary block (one slot long, so a
// whole-slot overrun stays inside the allocation) that must come back untouched; sources have no slack, so ASan sees a read
// past their end.
//
// What the checks catch (each mutant of the header built into this program; none is committed):
//   mutant of fep_staging.h                                   first failing check (the same in both builds unless noted)
//   settle(i) removed from Engine::h2d                         [h2d alone, 33554440 bytes] device block differs
//   settle(i) removed from Engine::d2h                         [d2h alone, 33554440 bytes] output differs
//   settle(i) removed from Engine::h2d_interleave2             [interleave2, 2097153 nodes] device block differs
//   hipEventRecord before its hipMemcpyAsync, in h2d            [h2d alone, 33554440 bytes] device block differs
//   hipEventRecord before its hipMemcpyAsync, in d2h            [engine error path] the round trip after the failed call differs
//   hipEventRecord before its hipMemcpyAsync, in interleave2    [interleave2, 2097153 nodes] device block differs
//   finish() synchronises without settling the parked chunks   [engine error path] the round trip after the failed call differs
//   HostCall::run() without the copy back of the inout array    [return-map-shaped call, run 0] ep differs
//   DeviceStore::reserve frees a block without synchronising   [buffer grows while a copy into its old block is queued]: the
//                                                              ASan build reports the queued copy's write into the freed block
//   ScopedStore declared after its HostCall (released before   [mesh-shaped call, a copy fails]: the ASan build reports the queued copy's
//     the scope drains)                                          write into the freed block
//   HostCall::run() without the copy back of its second out()   [return-map-shaped call, run 0] ds differs; with check 6 taken out,
//     array                                                      [mesh-shaped call, run 0] coord_ext differs
//   tail size min(kSlotBytes, bytes - off) -> kSlotBytes        h2d, d2h: [engine error path], interleave2: [interleave2, 1 nodes]:
//     (in h2d, d2h, or min(per, n - off) -> per in interleave2)  the ASan build reports the access past the end of a heap block,
//                                                              deterministically.  The TSan build checks no bounds: there the
//                                                              mutants showed as a race report or a crash in the same place,
//                                                              which is incidental and asserted nowhere; where a run survives
//                                                              the overrun, the one-slot canary behind the destination catches it
//   mutant of fep_solver_levels.h
//   push_level allocates t0 / q / k32 straight into the          [level upload, push 0, allocation 24 of 25 fails] all_or_none(m): t0 stays
//     hierarchy (`if (!m.t0)`, as before the arrays owned          set without q and k32 (the next push would skip all three)
//     their blocks) instead of into locals moved in at the end
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <mutex>
#include <thread>
#include <vector>

#include "../include/fep.h"

#define FEP_STAGING_HOST_STUB 1
#define FEP_STAGING_STUB_CAPTURE 1                      // hipStreamIsCapturing has a stand-in below: the scratch helper is built too
typedef int hipError_t;
enum { hipSuccess = 0, hipErrorOutOfMemory = 2, hipErrorUnknown = 999 };
enum hipMemcpyKind { hipMemcpyHostToDevice = 1, hipMemcpyDeviceToHost = 2 };
enum { hipHostMallocDefault = 0, hipStreamNonBlocking = 1, hipEventDisableTiming = 2 };
// A stream is the queue of its pending operations; positions count operations since the stream was made.
struct StubOp { void* dst; const void* src; size_t bytes; void (*fn)(void*); void* arg; };
struct StubStream {
    std::mutex m;                                        // the two-engine test drives two streams from two threads
    std::deque<StubOp> q;                                // queued and not yet run, oldest first
    size_t queued = 0, done = 0;                         // operations queued / run so far
    bool capturing = false;                              // what hipStreamIsCapturing reports
    void push(const StubOp& op) { std::lock_guard<std::mutex> g(m); q.push_back(op); ++queued; }
    size_t position() { std::lock_guard<std::mutex> g(m); return queued; }
    void run_to(size_t pos) {
        std::lock_guard<std::mutex> g(m);
        while (done < pos && !q.empty()) {
            const StubOp op = q.front();
            q.pop_front();
            if (op.fn) op.fn(op.arg); else std::memcpy(op.dst, op.src, op.bytes);
            ++done;
        }
    }
};
struct StubEvent { StubStream* st = nullptr; size_t pos = 0; };       // never recorded: nothing to wait for
typedef StubStream* hipStream_t;
typedef StubEvent* hipEvent_t;
static thread_local int fep_g_last_hip = 0;
static std::atomic<long> g_copies{0}, g_fail_copy_after{-1};
static std::atomic<int> g_fail_host_malloc{0};
static std::atomic<long> g_dev_live{0};                  // "device" blocks allocated and not freed
static hipError_t hipGetLastError() { return hipSuccess; }
static hipError_t hipHostMalloc(void** p, size_t b, unsigned) {
    if (g_fail_host_malloc.load() > 0) { g_fail_host_malloc.fetch_sub(1); *p = nullptr; return hipErrorOutOfMemory; }
    *p = std::malloc(b);
    return *p ? hipSuccess : hipErrorOutOfMemory;
}
static hipError_t hipHostFree(void* p) { std::free(p); return hipSuccess; }
static std::atomic<long> g_dev_mallocs{0};               // hipMalloc calls so far
static std::atomic<long> g_fail_dev_malloc_after{0};     // n > 0: the n-th hipMalloc from now fails (that one only)
static hipError_t hipMalloc(void** p, size_t b) {
    ++g_dev_mallocs;
    if (g_fail_dev_malloc_after.load() > 0 && g_fail_dev_malloc_after.fetch_sub(1) == 1) { *p = nullptr; return hipErrorOutOfMemory; }
    *p = std::malloc(b);
    if (*p) ++g_dev_live;
    return *p ? hipSuccess : hipErrorOutOfMemory;
}
static hipError_t hipMemcpy(void* d, const void* s, size_t b, hipMemcpyKind) { std::memcpy(d, s, b); return hipSuccess; }   // synchronous
static hipError_t hipFree(void* p) { if (p) --g_dev_live; std::free(p); return hipSuccess; }
enum hipStreamCaptureStatus { hipStreamCaptureStatusNone = 0, hipStreamCaptureStatusActive = 1 };
static hipError_t hipStreamIsCapturing(hipStream_t s, hipStreamCaptureStatus* cs);
static hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned) { *s = new StubStream(); return hipSuccess; }
static hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) { *e = new StubEvent(); return hipSuccess; }
static hipError_t hipStreamSynchronize(hipStream_t s) { s->run_to(s->position()); return hipSuccess; }
static hipError_t hipEventSynchronize(hipEvent_t e) { if (e->st) e->st->run_to(e->pos); return hipSuccess; }
static hipError_t hipEventRecord(hipEvent_t e, hipStream_t s) { e->st = s; e->pos = s->position(); return hipSuccess; }
static hipError_t hipMemcpyAsync(void* d, const void* s, size_t b, hipMemcpyKind, hipStream_t st) {
    const long k = g_copies.fetch_add(1);
    const long f = g_fail_copy_after.load();
    if (f >= 0 && k >= f) return hipErrorUnknown;        // a failing call queues nothing
    st->push(StubOp{d, s, b, nullptr, nullptr});
    return hipSuccess;
}
static hipError_t hipStreamIsCapturing(hipStream_t s, hipStreamCaptureStatus* cs) {
    *cs = s->capturing ? hipStreamCaptureStatusActive : hipStreamCaptureStatusNone;
    return hipSuccess;
}
// a "kernel": fn(arg) runs in stream order, when a synchronise reaches it
static void stub_launch(hipStream_t st, void (*fn)(void*), void* arg) { st->push(StubOp{nullptr, nullptr, 0, fn, arg}); }
#define HIP_TRY(expr) do { hipError_t _e = (expr); if (_e != hipSuccess) { fep_g_last_hip = (int)_e; return _e == hipErrorOutOfMemory ? FEP_ENOMEM : FEP_EHIP; } } while (0)
#define FEP_TRY(expr) do { int _r = (expr); if (_r != FEP_OK) return _r; } while (0)

#include "../fem-elastoplasticity_amd/csrc/fep_staging.h"
#include "../fem-elastoplasticity_amd/csrc/fep_solver_levels.h"

using namespace fep_stage;

static char g_what[96] = "start";                      // the check in progress, printed with a failure
#define WHAT(...) std::snprintf(g_what, sizeof g_what, __VA_ARGS__)
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED [%s] %s:%d: %s\n", g_what, __FILE__, __LINE__, #cond); return 1; } } while (0)

static int test_pinned() {
    WHAT("pinned cache");
    PinnedCache pc;
    void *a = nullptr, *b = nullptr, *c = nullptr;
    CHECK(pc.alloc(&a, 4096) == FEP_OK && pc.alloc(&b, 8192) == FEP_OK);
    CHECK(pc.covers((char*)a + 100, 3000) && !pc.covers((char*)a + 100, 5000));
    CHECK(pc.release(a) == FEP_OK);
    CHECK(pc.release(a) == FEP_EINVAL);                  // released twice: refused, not queued twice
    int dummy;
    CHECK(pc.release(&dummy) == FEP_EINVAL);             // not a block of the cache
    CHECK(pc.alloc(&c, 4096) == FEP_OK && c == a);       // same size: the idle block again
    CHECK(pc.release(c) == FEP_OK && pc.release(b) == FEP_OK && pc.idle_bytes == 4096 + 8192);
    g_fail_host_malloc = 1;                              // the runtime refuses once: idle blocks are given back, then it works
    void* d = nullptr;
    CHECK(pc.alloc(&d, 1 << 20) == FEP_OK && pc.idle_bytes == 0 && pc.idle.empty() && pc.live.size() == 1);
    g_fail_host_malloc = 2;                              // refuses twice: FEP_ENOMEM, nothing leaked
    void* e = nullptr;
    CHECK(pc.alloc(&e, 1 << 20) == FEP_ENOMEM && e == nullptr);
    CHECK(pc.release(d) == FEP_OK && pc.trim() == FEP_OK && pc.live.empty());
    return 0;
}

static int pool_worker(int seed, int* rc) {
    std::vector<double> src((size_t)3 << 18), dst(src.size()), il(2 * ((size_t)1 << 17));
    for (int rep = 0; rep < 12; ++rep) {
        for (size_t i = 0; i < src.size(); ++i) src[i] = (double)(seed * 1000003 + rep * 7919 + (long)i);
        pool().copy(dst.data(), src.data(), src.size() * sizeof(double));              // 6 MiB: split over the pool's threads
        if (std::memcmp(dst.data(), src.data(), src.size() * sizeof(double)) != 0) { *rc = 1; return 1; }
        const size_t n = (size_t)1 << 17;
        pool().interleave2(il.data(), src.data(), src.data() + n, n);
        for (size_t i = 0; i < n; ++i) if (il[2 * i] != src[i] || il[2 * i + 1] != src[n + i]) { *rc = 1; return 1; }
    }
    return 0;
}

static int test_pool_two_callers() {
    WHAT("pool, two callers");
    int rc1 = 0, rc2 = 0;
    std::thread t1(pool_worker, 1, &rc1), t2(pool_worker, 2, &rc2);
    t1.join(); t2.join();
    CHECK(rc1 == 0 && rc2 == 0);
    return 0;
}

static int engine_round_trip(int device, int* rc) {
    Engine* E = nullptr;
    if (engine(device, &E) != FEP_OK) { *rc = 1; return 1; }
    const size_t n = ((size_t)20 << 20) / sizeof(double) + 12345;       // 2.5 ring slots: exercises the wrap-around
    std::vector<double> in(n), out(n, -1.0);
    for (size_t i = 0; i < n; ++i) in[i] = (double)i + device;
    for (int rep = 0; rep < 3; ++rep) {
        EngineCall call(E);
        void* dbuf = nullptr;
        if (E->buffer(0, n * sizeof(double), &dbuf) != FEP_OK) { *rc = 1; return 1; }
        if (E->h2d(dbuf, in.data(), n * sizeof(double)) != FEP_OK) { *rc = 1; return 1; }
        if (E->d2h(out.data(), dbuf, n * sizeof(double)) != FEP_OK) { *rc = 1; return 1; }
        if (call.finish() != FEP_OK) { *rc = 1; return 1; }
        if (std::memcmp(in.data(), out.data(), n * sizeof(double)) != 0) { *rc = 2; return 1; }
        std::fill(out.begin(), out.end(), -1.0);
    }
    return 0;
}

// what a *_host entry point does, with the copy that follows the first device -> host chunk made to fail
static int failing_call(Engine* E, double* out, size_t n, void* dbuf) {
    EngineCall call(E);
    FEP_TRY(E->d2h(out, dbuf, n * sizeof(double)));      // parks chunks in the ring: pend[i].dst points into `out`
    return call.finish();
}

static int test_engine_error_path() {
    WHAT("engine error path");
    Engine* E = nullptr;
    CHECK(engine(7, &E) == FEP_OK);
    const size_t n = ((size_t)20 << 20) / sizeof(double);
    void* dbuf = nullptr;
    CHECK(E->buffer(0, n * sizeof(double), &dbuf) == FEP_OK);
    std::memset(dbuf, 0, n * sizeof(double));
    {
        std::vector<double>* out = new std::vector<double>(n);
        g_fail_copy_after = g_copies.load() + 1;         // first chunk lands in a slot, the second copy fails
        CHECK(failing_call(E, out->data(), n, dbuf) == FEP_EHIP);
        g_fail_copy_after = -1;
        delete out;                                       // the caller frees its output array on the error
    }
    for (int i = 0; i < Engine::kSlots; ++i) CHECK(E->pend[i].dst == nullptr);
    CHECK(E->next == 0);
    int rc = 0;                                           // the next call on the same engine: ASan reports any write into the freed array
    std::vector<double> in(n, 3.0), out2(n, 0.0);
    {
        EngineCall call(E);
        CHECK(E->h2d(dbuf, in.data(), n * sizeof(double)) == FEP_OK);
        CHECK(E->d2h(out2.data(), dbuf, n * sizeof(double)) == FEP_OK);
        CHECK(call.finish() == FEP_OK);
    }
    for (size_t i = 0; i < n; ++i) if (out2[i] != 3.0) rc = 1;
    CHECK(rc == 0);
    return 0;
}

static int test_two_engines() {
    WHAT("two engines");
    int rc1 = 0, rc2 = 0;
    std::thread t1(engine_round_trip, 0, &rc1), t2(engine_round_trip, 1, &rc2);
    t1.join(); t2.join();
    CHECK(rc1 == 0 && rc2 == 0);
    return 0;
}

// ---------------------------------------------------------------------------------------
// transfers longer than the ring
// ---------------------------------------------------------------------------------------
static constexpr size_t kSlot = Engine::kSlotBytes, kRing = Engine::kSlots * Engine::kSlotBytes;
static constexpr size_t kCanary = kSlot;
static constexpr unsigned char kCanaryByte = 0xC5;

static uint64_t mix(uint64_t x) {                        // splitmix64: no period a slot or the ring could share
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
// byte j of the pattern `seed` is byte j % 8 of mix(seed + j / 8); p is 8-byte aligned
static void fill(void* p, size_t bytes, uint64_t seed) {
    uint64_t* w = (uint64_t*)p;
    const size_t nw = bytes / 8;
    for (size_t i = 0; i < nw; ++i) w[i] = mix(seed + i);
    if (bytes % 8) { const uint64_t v = mix(seed + nw); std::memcpy((char*)p + 8 * nw, &v, bytes % 8); }
}
static bool is_fill(const void* p, size_t bytes, uint64_t seed) {
    const uint64_t* w = (const uint64_t*)p;
    const size_t nw = bytes / 8;
    for (size_t i = 0; i < nw; ++i) if (w[i] != mix(seed + i)) return false;
    if (bytes % 8) { const uint64_t v = mix(seed + nw); if (std::memcmp((const char*)p + 8 * nw, &v, bytes % 8) != 0) return false; }
    return true;
}

// [lead][bytes][tail]: p = base + lead.  Pageable: a heap block with p 8 bytes in (8- but not 64-byte aligned).  Pinned: a
// block of the cache with p 4104 bytes in, a view into its middle.  lead and tail hold the canary byte; a source has no tail.
struct Buf {
    char *base = nullptr, *p = nullptr;
    size_t bytes = 0, lead = 0, tail = 0;
    bool pin = false;
    Buf(size_t b, bool pinned_block, size_t tail_bytes) : bytes(b), lead(pinned_block ? 4104 : 8), tail(tail_bytes), pin(pinned_block) {
        void* q = nullptr;
        if (pin) { if (pinned().alloc(&q, lead + bytes + tail) != FEP_OK) q = nullptr; }
        else q = std::malloc(lead + bytes + tail);
        if (!q) { std::printf("FAILED: out of memory\n"); std::exit(1); }
        base = (char*)q; p = base + lead;
        std::memset(base, kCanaryByte, lead);
        if (tail) std::memset(p, 0x3C, bytes);           // a destination starts out as neither the pattern nor the canary
        std::memset(p + bytes, kCanaryByte, tail);
    }
    Buf(const Buf&) = delete;
    Buf& operator=(const Buf&) = delete;
    ~Buf() { if (pin) (void)pinned().release(base); else std::free(base); }
    bool canary_ok() const {
        for (size_t i = 0; i < lead; ++i) if ((unsigned char)base[i] != kCanaryByte) return false;
        const unsigned char* t = (const unsigned char*)p + bytes;
        size_t i = 0;
        for (; i < tail && ((uintptr_t)(t + i) & 7); ++i) if (t[i] != kCanaryByte) return false;
        for (; i + 8 <= tail; i += 8) if (*(const uint64_t*)(t + i) != 0xC5C5C5C5C5C5C5C5ull) return false;
        for (; i < tail; ++i) if (t[i] != kCanaryByte) return false;
        return true;
    }
};

static int round_trips(Engine* E, size_t bytes) {
    const uint64_t seed = 3 * bytes + 1;
    {
        WHAT("h2d alone, %zu bytes", bytes);
        Buf src(bytes, false, 0), dev(bytes, false, kCanary);
        fill(src.p, bytes, seed);
        {
            EngineCall call(E);
            CHECK(E->h2d(dev.p, src.p, bytes) == FEP_OK);
            CHECK(call.finish() == FEP_OK);
        }
        CHECK(is_fill(dev.p, bytes, seed));              // device block differs
        CHECK(dev.canary_ok());
    }
    {
        WHAT("d2h alone, %zu bytes", bytes);
        Buf dev(bytes, false, 0), out(bytes, false, kCanary);
        fill(dev.p, bytes, seed + 1);
        {
            EngineCall call(E);
            CHECK(E->d2h(out.p, dev.p, bytes) == FEP_OK);
            CHECK(call.finish() == FEP_OK);
        }
        CHECK(is_fill(out.p, bytes, seed + 1));          // output differs
        CHECK(out.canary_ok());
    }
    {
        WHAT("h2d + d2h, %zu bytes", bytes);
        Buf src(bytes, false, 0), out(bytes, false, kCanary);
        fill(src.p, bytes, seed + 2);
        {
            EngineCall call(E);
            void* dbuf = nullptr;
            CHECK(E->buffer(0, bytes, &dbuf) == FEP_OK);
            CHECK(E->h2d(dbuf, src.p, bytes) == FEP_OK);
            CHECK(E->d2h(out.p, dbuf, bytes) == FEP_OK);
            CHECK(call.finish() == FEP_OK);
        }
        CHECK(is_fill(out.p, bytes, seed + 2));
        CHECK(out.canary_ok());
    }
    return 0;
}

static int interleave_case(Engine* E, size_t n) {
    WHAT("interleave2, %zu nodes", n);
    Buf src(16 * n, false, 0), dev(16 * n, false, kCanary);
    double* x = (double*)src.p;
    double* y = x + n;
    for (size_t i = 0; i < n; ++i) { x[i] = (double)(mix(5 * n + i) >> 11); y[i] = -(double)(mix(7 * n + i + (1ull << 40)) >> 11); }
    {
        EngineCall call(E);
        CHECK(E->h2d_interleave2(dev.p, x, n) == FEP_OK);
        CHECK(call.finish() == FEP_OK);
    }
    const double* d = (const double*)dev.p;
    size_t bad = 0;
    for (size_t i = 0; i < n; ++i) bad += (d[2 * i] != x[i]) + (d[2 * i + 1] != y[i]);
    CHECK(bad == 0);                                     // device block differs
    CHECK(dev.canary_ok());
    return 0;
}

static int test_longer_than_the_ring() {
    Engine* E = nullptr;
    CHECK(engine(11, &E) == FEP_OK);
    const size_t sizes[] = {0, 1, 8, kSlot - 8, kSlot, kSlot + 8, kRing, kRing + 8, 5 * kSlot + kSlot / 2 + 1};
    for (size_t b : sizes) if (round_trips(E, b)) return 1;
    const size_t per = kSlot / 16;
    const size_t nodes[] = {1, per - 1, per, per + 1, 4 * per + 1, 5 * per + 1337};
    for (size_t n : nodes) if (interleave_case(E, n)) return 1;
    return 0;
}

// ---------------------------------------------------------------------------------------
// a call shaped like return_map_host_impl
// ---------------------------------------------------------------------------------------
// The "return map" on 64-bit words (integers: every bit pattern compares).  Reads all seven inputs, writes the five
// outputs; ep is updated in place after s has read it.
struct RmArgs {
    size_t n;
    const uint64_t *e, *sh, *bu, *et, *cc, *fld;         // 3n, n, n, n, n, 4n
    uint64_t *ep, *s, *ds;                               // 4n (in and out), 4n, 9n
    unsigned char* ip;                                   // n bytes
    uint64_t* cnt;                                       // 2
};
static void rm_compute(void* a) {
    const RmArgs& k = *(const RmArgs*)a;
    const size_t n = k.n;
    for (size_t i = 0; i < 4 * n; ++i) k.s[i] = k.e[i % (3 * n)] ^ (k.ep[i] << 7 | k.ep[i] >> 57) ^ k.sh[i % n];
    for (size_t i = 0; i < 9 * n; ++i) k.ds[i] = (k.bu[i % n] + k.et[(7 * i) % n]) ^ k.fld[i % (4 * n)];
    uint64_t c0 = 0, c1 = 0;
    for (size_t i = 0; i < n; ++i) { k.ip[i] = (unsigned char)(k.cc[i] >> 3); c0 += k.sh[i]; c1 ^= k.fld[3 * n + i]; }
    k.cnt[0] = c0; k.cnt[1] = c1;
    for (size_t i = 0; i < 4 * n; ++i) k.ep[i] = 3 * k.ep[i] + k.fld[i];
}

struct RmHost {                                          // the caller's arrays: pageable (8 bytes off) and pinned, mixed
    static constexpr size_t n = 300007;                  // e 0.86 slots, ep / field / s 1.14, ds 2.57: 7 pageable chunks in, 7 out
    Buf e{3 * n * 8, false, 0}, ep{4 * n * 8, false, kCanary}, sh{n * 8, true, 0}, bu{n * 8, false, 0}, et{n * 8, false, 0},
        cc{n * 8, true, 0}, fld{4 * n * 8, false, 0};
    Buf s{4 * n * 8, true, kCanary}, ds{9 * n * 8, false, kCanary}, ip{n, false, kCanary}, cnt{16, false, kCanary};
    Buf extra{8, false, 0};
};

static constexpr int kRmDevice = 12;                     // the engine of check 6
static int rm_call(Engine* E, RmHost& h, uint64_t seed, bool extra_first, int* start_slot) {
    const size_t n = RmHost::n, nb = n * 8;
    fill(h.e.p, 3 * nb, seed); fill(h.sh.p, nb, seed + 1); fill(h.bu.p, nb, seed + 2); fill(h.et.p, nb, seed + 3);
    fill(h.cc.p, nb, seed + 4); fill(h.fld.p, 4 * nb, seed + 5);
    std::memset(h.s.p, 0x3C, 4 * nb); std::memset(h.ds.p, 0x3C, 9 * nb); std::memset(h.ip.p, 0x3C, n); std::memset(h.cnt.p, 0x3C, 16);
    // what the call must return: the same function on copies of the inputs
    std::vector<uint64_t> r_ep(4 * n), r_s(4 * n), r_ds(9 * n), r_cnt(2);
    std::vector<unsigned char> r_ip(n);
    std::memcpy(r_ep.data(), h.ep.p, 4 * nb);
    RmArgs ref{n, (const uint64_t*)h.e.p, (const uint64_t*)h.sh.p, (const uint64_t*)h.bu.p, (const uint64_t*)h.et.p,
               (const uint64_t*)h.cc.p, (const uint64_t*)h.fld.p, r_ep.data(), r_s.data(), r_ds.data(), r_ip.data(), r_cnt.data()};
    rm_compute(&ref);
    RmArgs dev{};
    {
        enum { kE, kEp, kSh, kBu, kEt, kCc, kS, kDs, kIp, kCnt, kFld, kExtra };
        HostCall call(kRmDevice);
        CHECK(call.status() == FEP_OK);
        if (extra_first) call.in(kExtra, (const uint64_t*)h.extra.p, 1);    // one more chunk: the ring starts one slot further on
        *start_slot = E->next;
        dev.n = n;
        dev.e = call.in(kE, (const uint64_t*)h.e.p, 3 * n);
        dev.ep = call.inout(kEp, (uint64_t*)h.ep.p, 4 * n, true);
        dev.sh = call.in(kSh, (const uint64_t*)h.sh.p, n);
        dev.bu = call.in(kBu, (const uint64_t*)h.bu.p, n);
        dev.et = call.in(kEt, (const uint64_t*)h.et.p, n);
        dev.cc = call.in(kCc, (const uint64_t*)h.cc.p, n);
        dev.fld = call.in(kFld, (const uint64_t*)h.fld.p, 4 * n);
        dev.s = call.out(kS, (uint64_t*)h.s.p, 4 * n);
        dev.ds = call.out(kDs, (uint64_t*)h.ds.p, 9 * n);
        dev.ip = call.out(kIp, (unsigned char*)h.ip.p, n);
        dev.cnt = call.scratch<uint64_t>(kCnt, 2);
        call.out(kCnt, (uint64_t*)h.cnt.p, 2);
        CHECK(call.run([&] { stub_launch(call.stream(), rm_compute, &dev); return (int)FEP_OK; }) == FEP_OK);
    }
    CHECK(std::memcmp(h.s.p, r_s.data(), 4 * nb) == 0);
    CHECK(std::memcmp(h.ds.p, r_ds.data(), 9 * nb) == 0);
    CHECK(std::memcmp(h.ip.p, r_ip.data(), n) == 0);
    CHECK(std::memcmp(h.cnt.p, r_cnt.data(), 16) == 0);
    CHECK(std::memcmp(h.ep.p, r_ep.data(), 4 * nb) == 0);
    CHECK(h.s.canary_ok() && h.ds.canary_ok() && h.ip.canary_ok() && h.cnt.canary_ok() && h.ep.canary_ok());
    // the inputs are the caller's: untouched
    CHECK(is_fill(h.e.p, 3 * nb, seed) && is_fill(h.sh.p, nb, seed + 1) && is_fill(h.bu.p, nb, seed + 2));
    CHECK(is_fill(h.et.p, nb, seed + 3) && is_fill(h.cc.p, nb, seed + 4) && is_fill(h.fld.p, 4 * nb, seed + 5));
    return 0;
}

static int test_return_map_shaped_calls() {
    Engine* E = nullptr;
    CHECK(engine(kRmDevice, &E) == FEP_OK);              // the engine HostCall(kRmDevice) finds: its ring position is read below
    RmHost h;
    fill(h.ep.p, 4 * RmHost::n * 8, 99);
    fill(h.extra.p, 8, 98);
    unsigned starts = 0;
    for (int run = 0; run < 4; ++run) {
        WHAT("return-map-shaped call, run %d", run);
        int start = -1;
        if (rm_call(E, h, 1000 * (uint64_t)(run + 1), run > 0, &start)) return 1;
        starts |= 1u << start;
    }
    WHAT("return-map-shaped calls: ring start positions");
    CHECK(starts == (1u << Engine::kSlots) - 1);         // 14 pageable chunks per call + 1: starts at slots 0, 3, 2, 1
    return 0;
}

// ---------------------------------------------------------------------------------------
// DeviceStore's grow path
// ---------------------------------------------------------------------------------------
static int sized_round_trip(Engine* E, size_t bytes, uint64_t seed, bool check_rest, size_t rest) {
    Buf src(bytes, false, 0), out(bytes, false, kCanary);
    fill(src.p, bytes, seed);
    void* dbuf = nullptr;
    {
        EngineCall call(E);
        CHECK(E->buffer(0, bytes, &dbuf) == FEP_OK);
        if (check_rest) { CHECK(E->dev[0].second == bytes + rest); std::memset((char*)dbuf + bytes, kCanaryByte, rest); }
        CHECK(E->h2d(dbuf, src.p, bytes) == FEP_OK);
        CHECK(E->d2h(out.p, dbuf, bytes) == FEP_OK);
        CHECK(call.finish() == FEP_OK);
    }
    CHECK(is_fill(out.p, bytes, seed));
    CHECK(out.canary_ok());
    if (check_rest)                                      // the block kept its larger size: nothing written past the small call's end
        for (size_t i = 0; i < rest; ++i) CHECK(((unsigned char*)dbuf)[bytes + i] == kCanaryByte);
    return 0;
}

static int test_buffer_growth() {
    Engine* E = nullptr;
    CHECK(engine(13, &E) == FEP_OK);
    const size_t small = 8000, large = 5 * kSlot + kSlot / 2 + 1;
    WHAT("small call on a new engine");
    if (sized_round_trip(E, small, 1, false, 0)) return 1;
    WHAT("large call after the small one");
    if (sized_round_trip(E, large, 2, false, 0)) return 1;
    WHAT("small call after the large one");
    if (sized_round_trip(E, small, 3, true, large - small)) return 1;
    WHAT("buffer grows while a copy into its old block is queued");
    Buf src(small, false, 0), out(2 * small, false, kCanary);
    fill(src.p, small, 4);
    fill(out.p, 2 * small, 5);
    {
        EngineCall call(E);
        void *a = nullptr, *b = nullptr;
        CHECK(E->buffer(1, small, &a) == FEP_OK);
        CHECK(E->h2d(a, src.p, small) == FEP_OK);        // queued; the block is freed by the next line: it must synchronise first
        CHECK(E->buffer(1, 2 * small, &b) == FEP_OK);
        CHECK(E->h2d(b, out.p, 2 * small) == FEP_OK);
        CHECK(E->d2h(out.p, b, 2 * small) == FEP_OK);
        CHECK(call.finish() == FEP_OK);
    }
    CHECK(is_fill(out.p, 2 * small, 5) && out.canary_ok());
    return 0;
}

// ---------------------------------------------------------------------------------------
// a call shaped like the mesh host forms: device blocks of the call
// ---------------------------------------------------------------------------------------
struct MeshArgs {
    size_t ne, nc, nch, nx, np;
    const uint64_t *elem, *coord;                        // ne, nc
    uint64_t *child, *coord_ext, *parent;                // nch, nx, np (parent may be NULL)
};
static void mesh_compute(void* a) {
    const MeshArgs& k = *(const MeshArgs*)a;
    for (size_t i = 0; i < k.nch; ++i) k.child[i] = k.elem[i % k.ne] ^ (k.coord[i % k.nc] << 9 | k.coord[i % k.nc] >> 55);
    for (size_t i = 0; i < k.nx; ++i) k.coord_ext[i] = k.coord[i % k.nc] + k.elem[(5 * i) % k.ne];
    if (k.parent) for (size_t i = 0; i < k.np; ++i) k.parent[i] = k.elem[i % k.ne] >> 3;
}

// words: elem 1.25 slots + 3 (2 chunks), coord half a slot + 1 (1), child 2.3 slots (3), coord_ext 0.7 slots (1): 7 pageable
// chunks per call, so four calls start the ring at slots 0, 3, 2, 1
static constexpr size_t kMeshNe = 1310723, kMeshNc = 524289, kMeshNch = 2411725, kMeshNx = 734003, kMeshNp = 1000;
static constexpr int kMeshDevice = 14;

// `child_h`, `coord_ext_h`: the caller's output arrays (8 bytes into their allocations)
static int mesh_call(const Buf& elem, const Buf& coord, uint64_t* child_h, uint64_t* coord_ext_h, int* start_slot, long fail_after) {
    enum { kElem, kCoord, kChild, kCoordExt, kParent };
    MeshArgs dev{kMeshNe, kMeshNc, kMeshNch, kMeshNx, kMeshNp, nullptr, nullptr, nullptr, nullptr, nullptr};
    ScopedStore store;                                   // before the call: released after its scope has finished or drained
    HostCall call(kMeshDevice, &store);
    FEP_TRY(call.status());
    Engine* E = nullptr;
    FEP_TRY(engine(kMeshDevice, &E));
    *start_slot = E->next;
    if (fail_after >= 0) g_fail_copy_after = g_copies.load() + fail_after;
    dev.elem = call.in(kElem, (const uint64_t*)elem.p, kMeshNe);
    dev.coord = call.in(kCoord, (const uint64_t*)coord.p, kMeshNc);
    dev.child = call.out(kChild, child_h, kMeshNch);
    dev.coord_ext = call.out(kCoordExt, coord_ext_h, kMeshNx);
    dev.parent = call.out(kParent, (uint64_t*)nullptr, kMeshNp);
    if (dev.parent || store.blocks.size() > (size_t)kParent) return FEP_ESTATE;     // a NULL array: no block, no transfer
    return call.run([&] { stub_launch(call.stream(), mesh_compute, &dev); return (int)FEP_OK; });
}

static int test_mesh_shaped_calls() {
    Engine* E = nullptr;
    CHECK(engine(kMeshDevice, &E) == FEP_OK);
    const long live0 = g_dev_live.load();
    Buf elem(kMeshNe * 8, false, 0), coord(kMeshNc * 8, false, 0);
    std::vector<uint64_t> r_child(kMeshNch), r_x(kMeshNx);
    unsigned starts = 0;
    for (int run = 0; run < 4; ++run) {
        WHAT("mesh-shaped call, run %d", run);
        fill(elem.p, kMeshNe * 8, 77 + run);
        fill(coord.p, kMeshNc * 8, 177 + run);
        MeshArgs ref{kMeshNe, kMeshNc, kMeshNch, kMeshNx, kMeshNp, (const uint64_t*)elem.p, (const uint64_t*)coord.p, r_child.data(),
                     r_x.data(), nullptr};
        mesh_compute(&ref);
        Buf child(kMeshNch * 8, false, kCanary), x(kMeshNx * 8, false, kCanary);
        int start = -1;
        CHECK(mesh_call(elem, coord, (uint64_t*)child.p, (uint64_t*)x.p, &start, -1) == FEP_OK);
        starts |= 1u << start;
        CHECK(std::memcmp(child.p, r_child.data(), kMeshNch * 8) == 0);            // child differs
        CHECK(std::memcmp(x.p, r_x.data(), kMeshNx * 8) == 0);                     // coord_ext differs
        CHECK(child.canary_ok() && x.canary_ok());
        CHECK(is_fill(elem.p, kMeshNe * 8, 77 + run) && is_fill(coord.p, kMeshNc * 8, 177 + run));
        CHECK(g_dev_live.load() == live0);               // the call's device blocks are gone
    }
    WHAT("mesh-shaped calls: ring start positions");
    CHECK(starts == (1u << Engine::kSlots) - 1);
    WHAT("mesh-shaped call, a copy fails");
    {
        // three chunks in, the first chunk of child out, then the failure: the copies into the call's blocks and the kernel
        // are still queued when the call gives up, and run when its scope drains the engine, before the blocks are released
        std::vector<uint64_t>*child = new std::vector<uint64_t>(kMeshNch + 1), *x = new std::vector<uint64_t>(kMeshNx + 1);
        int start = -1;
        CHECK(mesh_call(elem, coord, child->data() + 1, x->data() + 1, &start, 4) == FEP_EHIP);
        g_fail_copy_after = -1;
        delete child;                                     // the caller frees its output arrays on the error
        delete x;
    }
    for (int i = 0; i < Engine::kSlots; ++i) CHECK(E->pend[i].dst == nullptr);
    CHECK(E->next == 0 && g_dev_live.load() == live0);
    WHAT("mesh-shaped call after the failed one");
    {
        MeshArgs ref{kMeshNe, kMeshNc, kMeshNch, kMeshNx, kMeshNp, (const uint64_t*)elem.p, (const uint64_t*)coord.p, r_child.data(),
                     r_x.data(), nullptr};
        mesh_compute(&ref);
        Buf child(kMeshNch * 8, false, kCanary), x(kMeshNx * 8, false, kCanary);
        int start = -1;
        CHECK(mesh_call(elem, coord, (uint64_t*)child.p, (uint64_t*)x.p, &start, -1) == FEP_OK);
        CHECK(std::memcmp(child.p, r_child.data(), kMeshNch * 8) == 0 && std::memcmp(x.p, r_x.data(), kMeshNx * 8) == 0);
        CHECK(child.canary_ok() && x.canary_ok());
    }
    return 0;
}

// ---------------------------------------------------------------------------------------
// kernel scratch per (device, stream)
// ---------------------------------------------------------------------------------------
static int test_stream_scratch() {
    WHAT("stream scratch");
    StubStream st, other, cap;
    const long live0 = g_dev_live.load();
    void *a = nullptr, *b = nullptr, *c = nullptr, *d = nullptr;
    CHECK(stream_scratch(kScratchArea, 0, &st, 1000, 1500, &a) == FEP_OK && a && g_dev_live.load() == live0 + 1);
    CHECK(stream_scratch(kScratchArea, 0, &st, 800, 1200, &b) == FEP_OK && b == a);          // a smaller need: the same block
    CHECK(stream_scratch(kScratchArea, 0, &st, 1500, 1875, &b) == FEP_OK && b == a);         // up to what growing allocated
    CHECK(g_dev_live.load() == live0 + 1);
    CHECK(stream_scratch(kScratchArea, 0, &st, 1501, 2000, &c) == FEP_OK && c && c != a);    // growth: a new block
    CHECK(g_dev_live.load() == live0 + 2);
    std::memset(a, 0x11, 1500);                           // the old one is still allocated (a captured graph may name it)
    std::memset(c, 0x22, 2000);
    // another tag, stream or device: blocks of their own
    CHECK(stream_scratch(kScratchIndicator, 0, &st, 64, 64, &d) == FEP_OK && d != c && d != a);
    CHECK(stream_scratch(kScratchArea, 0, &other, 64, 64, &b) == FEP_OK && b != c && b != d);
    CHECK(stream_scratch(kScratchArea, 1, &st, 64, 64, &b) == FEP_OK && b != c && b != d);
    CHECK(g_dev_live.load() == live0 + 5);
    WHAT("stream scratch, capturing");
    cap.capturing = true;
    void* e = nullptr;
    CHECK(stream_scratch(kScratchArea, 0, &cap, 100, 100, &e) == FEP_ESTATE && e == nullptr && g_dev_live.load() == live0 + 5);
    cap.capturing = false;                                // the same call once outside the capture ...
    CHECK(stream_scratch(kScratchArea, 0, &cap, 100, 100, &e) == FEP_OK && e && g_dev_live.load() == live0 + 6);
    cap.capturing = true;                                 // ... then it needs no allocation; a larger one is still refused
    void* f = nullptr;
    CHECK(stream_scratch(kScratchArea, 0, &cap, 100, 100, &f) == FEP_OK && f == e);
    f = nullptr;
    CHECK(stream_scratch(kScratchArea, 0, &cap, 101, 200, &f) == FEP_ESTATE && f == nullptr && g_dev_live.load() == live0 + 6);
    WHAT("stream scratch, growth rule below the need");
    void* g = nullptr;                                    // never a block smaller than the need
    CHECK(stream_scratch(kScratchRmCounts, 0, &st, 4096, 16, &g) == FEP_OK && g);
    std::memset(g, 0x33, 4096);
    void* h = nullptr;
    CHECK(stream_scratch(kScratchRmCounts, 0, &st, 4096, 16, &h) == FEP_OK && h == g && g_dev_live.load() == live0 + 7);
    return 0;
}

// ---------------------------------------------------------------------------------------
// the solver's device arrays and the upload of a multigrid level (fep_solver_levels.h)
// ---------------------------------------------------------------------------------------
using fep_levels::DeviceArray;

static int test_device_array() {
    WHAT("device array");
    const long live0 = g_dev_live.load();
    {
        DeviceArray<double> a, b;
        CHECK(!a && a.size() == 0);
        CHECK(a.alloc(0) == FEP_OK && a && a.size() == 1);                   // at least one element
        CHECK(a.alloc(100) == FEP_OK && a.size() == 100 && g_dev_live.load() == live0 + 1);     // the former block is freed
        const std::vector<double> v{1.0, 2.0, 3.0};
        CHECK(b.upload(v) == FEP_OK && b.size() == 3 && std::memcmp(b, v.data(), 24) == 0);
        double* pb = b;
        DeviceArray<double> c(std::move(b));                                // move-construct: the source is empty
        CHECK(!b && b.size() == 0 && c == pb && c.size() == 3 && g_dev_live.load() == live0 + 2);
        a = std::move(c);                                                   // move-assign: the overwritten block is freed
        CHECK(!c && c.size() == 0 && a == pb && a.size() == 3 && g_dev_live.load() == live0 + 1);
        a = std::move(*&a);                                                 // onto itself: nothing happens
        CHECK(a == pb && g_dev_live.load() == live0 + 1);
        g_fail_dev_malloc_after = 1;                                        // a failed alloc leaves the array empty
        fep_g_last_hip = 0;
        CHECK(a.alloc(50) == FEP_ENOMEM && !a && a.size() == 0 && g_dev_live.load() == live0 && fep_g_last_hip == hipErrorOutOfMemory);
        g_fail_dev_malloc_after = 1;
        CHECK(c.upload(v) == FEP_ENOMEM && !c);
        CHECK(c.upload(v.data(), 0) == FEP_OK && c && c.size() == 1);       // nothing to copy: one element, no read of the source
        a.reset();
        CHECK(!a && g_dev_live.load() == live0 + 1);
    }
    CHECK(g_dev_live.load() == live0);                                      // the destructors freed the rest
    return 0;
}

struct HostCsr {
    int64_t n_rows = 0, n_cols = 0;
    std::vector<int32_t> ip, ix;
    std::vector<double> v;
    HostCsr(int64_t r, int64_t c) : n_rows(r), n_cols(c), ip(1, 0) {}
    void entry(int32_t col, double val) { ix.push_back(col); v.push_back(val); }
    void end_row() { ip.push_back((int32_t)ix.size()); }
    HostCsr transposed() const {
        HostCsr t(n_cols, n_rows);
        for (int64_t c = 0; c < n_cols; ++c) {
            for (int64_t r = 0; r < n_rows; ++r)
                for (int32_t k = ip[(size_t)r]; k < ip[(size_t)r + 1]; ++k) if (ix[(size_t)k] == c) t.entry((int32_t)r, v[(size_t)k]);
            t.end_row();
        }
        return t;
    }
    double at(int64_t r, int64_t c) const {
        for (int32_t k = ip[(size_t)r]; k < ip[(size_t)r + 1]; ++k) if (ix[(size_t)k] == c) return v[(size_t)k];
        return 0.0;
    }
};
static HostCsr dense_csr(int64_t n, double diag, double off) {
    HostCsr a(n, n);
    for (int64_t r = 0; r < n; ++r) { for (int64_t c = 0; c < n; ++c) a.entry((int32_t)c, r == c ? diag : off); a.end_row(); }
    return a;
}
// The hierarchy of check 11: 6 mesh nodes (12 DOFs) -> 2 coarse nodes (6 DOFs) -> 1 (3 DOFs); every value is exact in float
struct TinyHierarchy {
    static constexpr int64_t kDof = 12, kBlk = 16;
    HostCsr P0{12, 6}, R0{6, 12}, A1 = dense_csr(6, 4.0, -0.5), D1{6, 6}, P1{6, 3}, R1{3, 6}, A2 = dense_csr(3, 2.0, 0.25);
    TinyHierarchy() {
        for (int i = 0; i < 12; ++i) {                   // DOF i = (node i / 2, component i % 2) -> aggregate node / 3: its
            const int a = i / 6, c = i % 2;              // own component and the rotation
            P0.entry(3 * a + c, 1.0); P0.entry(3 * a + 2, 0.25 * (i + 1)); P0.end_row();
        }
        R0 = P0.transposed();
        for (int r = 0; r < 6; ++r) { for (int c = 0; c < 3; ++c) D1.entry(3 * (r / 3) + c, r % 3 == c ? 0.5 : 0.125); D1.end_row(); }
        for (int i = 0; i < 6; ++i) { P1.entry(i % 3, 1.0); if (i % 3 != 2) P1.entry(2, 0.5 * (i + 1)); P1.end_row(); }
        R1 = P1.transposed();
    }
    int push(fep_levels::Multigrid& m, int level, const HostCsr* p = nullptr, const HostCsr* a = nullptr) const {
        const HostCsr &P = p ? *p : (level == 0 ? P0 : P1), &R = level == 0 ? R0 : R1, &A = a ? *a : (level == 0 ? A1 : A2);
        return fep_levels::push_level(m, 0, kDof, kBlk, P.n_rows, P.n_cols, P.ip.data(), P.ix.data(), P.v.data(), R.ip.data(), R.ix.data(),
                                      R.v.data(), A.ip.data(), A.ix.data(), A.v.data(), level == 0 ? D1.ip.data() : nullptr,
                                      level == 0 ? D1.ix.data() : nullptr, level == 0 ? D1.v.data() : nullptr, 0.7, level == 1);
    }
};
static bool all_or_none(const fep_levels::Multigrid& m) {
    const int set = (m.t0 ? 1 : 0) + (m.q ? 1 : 0) + (m.k32 ? 1 : 0);
    return set == 0 || set == 3;
}
// the node blocks of a level's transfers hold exactly the prolongation (and the restriction its transposes)
static bool blocks_match(const fep_levels::Level& l, const HostCsr& P, int bf) {
    const fep_levels::Blocks& B = l.tb;
    if (B.bf != bf || B.nf != P.n_rows / bf || B.nc != P.n_cols / 3 || B.pptr[B.nf] != B.nblk || B.rptr[B.nc] != B.nblk) return false;
    std::vector<double> dp((size_t)(P.n_rows * P.n_cols), 0.0), dr(dp.size(), 0.0);
    for (int64_t i = 0; i < B.nf; ++i)
        for (int32_t t = B.pptr[i]; t < B.pptr[i + 1]; ++t)
            for (int r = 0; r < bf; ++r)
                for (int c = 0; c < 3; ++c) dp[(size_t)((bf * i + r) * P.n_cols + 3 * B.pcol[t] + c)] = B.pval[(int64_t)t * 3 * bf + 3 * r + c];
    for (int64_t J = 0; J < B.nc; ++J)
        for (int32_t t = B.rptr[J]; t < B.rptr[J + 1]; ++t)
            for (int c = 0; c < 3; ++c)
                for (int r = 0; r < bf; ++r) dr[(size_t)((bf * B.rcol[t] + r) * P.n_cols + 3 * J + c)] = B.rval[(int64_t)t * 3 * bf + c * bf + r];
    for (int64_t r = 0; r < P.n_rows; ++r)
        for (int64_t c = 0; c < P.n_cols; ++c)
            if (dp[(size_t)(r * P.n_cols + c)] != P.at(r, c) || dr[(size_t)(r * P.n_cols + c)] != P.at(r, c)) return false;
    return true;
}

static int test_level_upload() {
    const TinyHierarchy H;
    const long live0 = g_dev_live.load();
    {
        fep_levels::Multigrid m;                         // (block transfers and the single-precision copy are on by default)
        CHECK(m.block_transfers && m.fp32);
        for (int level = 0; level < 2; ++level) {
            // how many device allocations the push makes: from a push into a copy of the state that is thrown away
            long n_alloc = 0;
            {
                fep_levels::Multigrid probe;
                if (level == 1) { WHAT("level upload, probe"); CHECK(H.push(probe, 0) == FEP_OK); }
                const long before = g_dev_mallocs.load();
                WHAT("level upload, probe of push %d", level);
                CHECK(H.push(probe, level) == FEP_OK);
                n_alloc = g_dev_mallocs.load() - before;
            }
            CHECK(n_alloc == (level == 0 ? 4 * 3 + 6 + 4 + 3 : 3 * 3 + 6 + 4));     // P R A D, blocks, vectors, t0 q k32 / P R A, ...
            for (long k = 1; k <= n_alloc; ++k) {
                WHAT("level upload, push %d, allocation %ld of %ld fails", level, k, n_alloc);
                const long live = g_dev_live.load();
                g_fail_dev_malloc_after = k;
                const int rc = H.push(m, level);
                CHECK(g_fail_dev_malloc_after.load() == 0);                   // the failure was reached
                CHECK(rc == FEP_ENOMEM);
                CHECK((int)m.levels.size() == level);
                CHECK(all_or_none(m));                                        // t0, q, k32: all set or all empty
                CHECK(level == 0 ? !m.t0 : !!m.t0);
                CHECK(g_dev_live.load() == live);
            }
            WHAT("level upload, push %d", level);
            CHECK(H.push(m, level) == FEP_OK && (int)m.levels.size() == level + 1);
            CHECK(m.t0 && m.q && m.k32 && m.t0.size() == H.kDof && m.q.size() == H.kDof && m.k32.size() == 4 * H.kBlk);
            CHECK(blocks_match(m.levels[(size_t)level], level == 0 ? H.P0 : H.P1, level == 0 ? 2 : 3));
            const fep_levels::Level& l = m.levels[(size_t)level];
            CHECK(l.last == (level == 1) && l.A.nnz == l.n_coarse * l.n_coarse && l.x.size() == l.n_coarse && !l.D.vals == (level == 1));
            CHECK(std::memcmp(l.P.vals, (level == 0 ? H.P0 : H.P1).v.data(), (size_t)l.P.nnz * 8) == 0 && l.hPi == (level == 0 ? H.P0 : H.P1).ix);
        }
        WHAT("level upload, push after the last level");
        const long live = g_dev_live.load();
        CHECK(H.push(m, 1) == FEP_ESTATE && m.levels.size() == 2 && g_dev_live.load() == live);
        WHAT("level upload, drop all levels");
        fep_levels::drop_levels(m);
        CHECK(m.levels.empty() && !m.refresh && m.t0 && g_dev_live.load() == live0 + 3);        // t0, q, k32 stay for the next hierarchy
        WHAT("level upload, column index out of range");
        HostCsr badP = H.P0, badA = H.A1;
        badP.ix[5] = 6;                                  // P has 6 columns: refused before anything is allocated
        badA.ix[7] = -1;                                 // A is checked after P and R are on the device: they are freed again
        CHECK(H.push(m, 0, &badP, nullptr) == FEP_ERANGE && m.levels.empty() && g_dev_live.load() == live0 + 3);
        CHECK(H.push(m, 0, nullptr, &badA) == FEP_ERANGE && m.levels.empty() && g_dev_live.load() == live0 + 3);
        WHAT("level upload, a hierarchy after the dropped one");
        CHECK(H.push(m, 0) == FEP_OK && H.push(m, 1) == FEP_OK && m.levels.size() == 2);
    }
    WHAT("level upload, destruction");
    CHECK(g_dev_live.load() == live0);
    return 0;
}

int main() {
    if (test_pinned()) return 1;
    if (test_pool_two_callers()) return 1;
    if (test_engine_error_path()) return 1;
    if (test_two_engines()) return 1;
    if (test_longer_than_the_ring()) return 1;
    if (test_return_map_shaped_calls()) return 1;
    if (test_buffer_growth()) return 1;
    if (test_mesh_shaped_calls()) return 1;
    if (test_stream_scratch()) return 1;
    if (test_device_array()) return 1;
    if (test_level_upload()) return 1;
    if (pinned().trim() != FEP_OK) return 1;             // the callers' pinned arrays went back to the cache: unpin them
    std::printf("staging ok\n");
    return 0;
}
