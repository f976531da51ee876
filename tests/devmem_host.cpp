// devmem_host.cpp -- the owners of csrc/demc_devmem.hpp on the CPU: the HIP entry points the header calls are counting stubs over
// malloc / free, so every create and every release is seen, and a release too many or too few is a miscount here and a
// double free or a leak to the address sanitizer the program is built with (tests/test_devmem_host.py).  No HIP runtime is linked.
// The end of a call (finish) and the pass timer of the diagnostic variant (PassTrace) run over stubs as well: a stream on which
// nothing is pending, events that carry the time of their mark.  StagedList runs over the same stubs, which count its waits.
#define DEMC_PASS_TRACE  // the variant that measures; without it PassTrace is two empty functions
#include "demc_devmem.hpp"

#include <cstring>

#include <cstdio>
#include <cstdlib>

namespace {
enum Kind { DEV, PIN, EVT, MOD, N_KINDS };
int made[N_KINDS], freed[N_KINDS];
int dev_allocs_left = -1;  // hipMalloc fails once this many have succeeded (-1: never)
hipError_t launch_error = hipSuccess, sync_error = hipSuccess;  // what hipGetLastError / hipStreamSynchronize answer
int copies = 0, copies_left = -1;  // hipMemcpy fails once this many have succeeded (-1: never)
int events_left = -1;              // likewise hipEventCreateWithFlags
float now_ms = 0.f;                // the time an event records
int pin_allocs_left = -1;          // likewise hipHostMalloc
int event_waits = 0, stream_waits = 0, async_copies = 0;  // hipEventSynchronize / hipStreamSynchronize / hipMemcpyAsync calls seen
hipError_t event_wait_error = hipSuccess;

hipError_t make(Kind k, void** out, size_t bytes) {
    if (k == DEV && dev_allocs_left == 0) return hipErrorOutOfMemory;
    if (k == DEV && dev_allocs_left > 0) --dev_allocs_left;
    if (k == PIN && pin_allocs_left == 0) return hipErrorOutOfMemory;
    if (k == PIN && pin_allocs_left > 0) --pin_allocs_left;
    *out = std::malloc(bytes ? bytes : 1);
    ++made[k];
    return hipSuccess;
}
hipError_t release(Kind k, void* p) {
    std::free(p);
    ++freed[k];
    return hipSuccess;
}
}  // namespace

extern "C" {
hipError_t hipMalloc(void** p, size_t n) { return make(DEV, p, n); }
hipError_t hipFree(void* p) { return release(DEV, p); }
hipError_t hipHostMalloc(void** p, size_t n, unsigned) { return make(PIN, p, n); }
hipError_t hipHostFree(void* p) { return release(PIN, p); }
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) {
    if (events_left == 0) return hipErrorOutOfMemory;
    if (events_left > 0) --events_left;
    return make(EVT, (void**)e, sizeof(float));
}
hipError_t hipEventRecord(hipEvent_t e, hipStream_t) { std::memcpy((void*)e, &now_ms, sizeof now_ms); return hipSuccess; }
hipError_t hipEventElapsedTime(float* ms, hipEvent_t a, hipEvent_t b) {
    float ta, tb;
    std::memcpy(&ta, (void*)a, sizeof ta); std::memcpy(&tb, (void*)b, sizeof tb);
    *ms = tb - ta;
    return hipSuccess;
}
hipError_t hipGetLastError() { return launch_error; }
hipError_t hipStreamSynchronize(hipStream_t) { ++stream_waits; return sync_error; }
hipError_t hipEventSynchronize(hipEvent_t) { ++event_waits; return event_wait_error; }
hipError_t hipMemcpyAsync(void* dst, const void* src, size_t n, hipMemcpyKind, hipStream_t) {
    std::memcpy(dst, src, n);
    ++async_copies;
    return hipSuccess;
}
hipError_t hipMemcpy(void* dst, const void* src, size_t n, hipMemcpyKind) {
    if (copies_left == 0) return hipErrorInvalidValue;
    if (copies_left > 0) --copies_left;
    std::memcpy(dst, src, n);
    ++copies;
    return hipSuccess;
}
const char* hipGetErrorString(hipError_t e) { return e == hipErrorOutOfMemory ? "out of memory" : e == hipErrorInvalidValue ? "invalid argument" : "other"; }
hipError_t hipEventDestroy(hipEvent_t e) { return release(EVT, (void*)e); }
hipError_t hipModuleLoadData(hipModule_t* m, const void*) { return make(MOD, (void**)m, 1); }
hipError_t hipModuleUnload(hipModule_t m) { return release(MOD, (void*)m); }
}

namespace {
int failures = 0;
#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) {                                                               \
            std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                              \
        }                                                                            \
    } while (0)

using namespace demc;

int live(Kind k) { return made[k] - freed[k]; }

struct Record {  // a record of owners beside plain fields, as the handle's Model is
    int family = -1;
    DevBuf<double> data, table;
    DevBuf<long long> dims;
    PinnedBuf<int> pin;
    Event ev;
    Module mod;
    double c[2] = {0, 0};
};

void fill(Record& r) {
    r.family = 3;
    CHECK(r.data.alloc(10) == hipSuccess && r.table.alloc(4) == hipSuccess && r.dims.alloc(8) == hipSuccess);
    CHECK(r.pin.alloc(16, 0) == hipSuccess && r.ev.create(0) == hipSuccess && r.mod.load("image") == hipSuccess);
    r.c[1] = 2.5;
}

void alloc_reset_destructor() {
    const int m0 = made[DEV], f0 = freed[DEV];
    {
        DevBuf<double> a;
        CHECK(!a && a.get() == nullptr);
        CHECK(a.alloc(100) == hipSuccess && a.get() != nullptr);
        a.get()[99] = 1.0;  // (the allocation is n elements, not n bytes)
        double* p = a;      // the conversion
        CHECK(p == a.get());
    }
    CHECK(made[DEV] == m0 + 1 && freed[DEV] == f0 + 1);  // the destructor, once
    {
        DevBuf<int> a;
        CHECK(a.alloc(3) == hipSuccess);
        a.reset();
        CHECK(freed[DEV] == f0 + 2 && a.get() == nullptr);
        a.reset();  // nothing held: nothing freed
        CHECK(freed[DEV] == f0 + 2);
    }
    CHECK(freed[DEV] == f0 + 2);  // ... nor by the destructor afterwards
    {
        DevBuf<int> a;
        CHECK(a.alloc(3) == hipSuccess);
        CHECK(a.alloc(5) == hipSuccess);  // over a live buffer: the old one goes
        CHECK(made[DEV] == m0 + 4 && freed[DEV] == f0 + 3);
    }
    CHECK(freed[DEV] == f0 + 4);
}

void moves() {
    const int f0 = freed[DEV];
    {
        DevBuf<double> a;
        CHECK(a.alloc(7) == hipSuccess);
        double* p = a.get();
        DevBuf<double> b(std::move(a));
        CHECK(b.get() == p && a.get() == nullptr && freed[DEV] == f0);
        DevBuf<double> c;
        CHECK(c.alloc(2) == hipSuccess);
        c = std::move(b);  // over a live buffer: it is freed, there and then
        CHECK(freed[DEV] == f0 + 1 && c.get() == p && b.get() == nullptr);
        DevBuf<double>& self = c;
        c = std::move(self);
        CHECK(freed[DEV] == f0 + 1 && c.get() == p);
        c = DevBuf<double>();  // an empty one moved over it: released
        CHECK(freed[DEV] == f0 + 2 && !c);
    }
    CHECK(freed[DEV] == f0 + 2);
    Event e;
    CHECK(e.create(0) == hipSuccess);
    Event f(std::move(e));
    CHECK(live(EVT) == 1 && !e && f);
    f = Event();
    CHECK(live(EVT) == 0);
}

void record_assignment() {
    Record r;
    fill(r);
    CHECK(live(DEV) == 3 && live(PIN) == 1 && live(EVT) == 1 && live(MOD) == 1);
    r = Record{};  // the whole record at once: every owner releases, every field is back at its default
    CHECK(live(DEV) == 0 && live(PIN) == 0 && live(EVT) == 0 && live(MOD) == 0);
    CHECK(r.family == -1 && !r.data && !r.table && !r.dims && !r.pin && !r.ev && !r.mod && r.c[1] == 0.0);
    fill(r);
    fill(r);  // set again without clearing: each creation releases what was held
    CHECK(live(DEV) == 3 && live(PIN) == 1 && live(EVT) == 1 && live(MOD) == 1);
    Record* heap = new Record;
    fill(*heap);
    delete heap;  // as `delete h` does for the handle
    CHECK(live(DEV) == 3);
}  // (r goes out of scope holding a model)

void failed_allocations() {
    const int live0 = live(DEV);
    {
        Scratch s;
        double *a = nullptr, *b = nullptr;
        int* c = nullptr;
        dev_allocs_left = 2;
        CHECK(s.get(&a, 100) && s.get(&b, 0) && a && b);
        CHECK(!s.get(&c, 50) && c == nullptr);  // the third fails: the call returns, the two before it are still owned
        CHECK(live(DEV) == live0 + 2);
    }
    CHECK(live(DEV) == live0);
    DevBuf<double> d;
    dev_allocs_left = 1;
    CHECK(d.alloc(4) == hipSuccess);
    CHECK(d.alloc(4) == hipErrorOutOfMemory);  // a failed allocation over a live buffer: the old one is gone, nothing is held
    CHECK(!d && live(DEV) == live0);
    dev_allocs_left = -1;
}

void call_endings() {
    const double src[3] = {1.5, 2.5, 3.5};
    double a[3] = {0, 0, 0}, b[2] = {0, 0};
    std::string err;
    CHECK(hip_ok("who", hipSuccess, err) && err.empty());
    CHECK(!hip_ok("demc_x", hipErrorOutOfMemory, err) && err == "demc_x: out of memory");
    err.clear();
    CHECK(finish("demc_x", nullptr, {{a, src, sizeof a}, {nullptr, src, sizeof a}, {b, src + 1, sizeof b}}, err) && err.empty());
    CHECK(copies == 2 && a[2] == 3.5 && b[0] == 2.5 && b[1] == 3.5);  // in order; the one that was not asked for is skipped
    // a launch error, a stream error, a failed copy: nothing (more) is copied, and the message names the call
    launch_error = hipErrorInvalidValue;
    CHECK(!finish("demc_x", nullptr, {{a, src, sizeof a}}, err) && err == "demc_x: invalid argument" && copies == 2);
    launch_error = hipSuccess; sync_error = hipErrorOutOfMemory;
    CHECK(!finish("demc_y", nullptr, {{a, src, sizeof a}}, err) && err == "demc_y: out of memory" && copies == 2);
    sync_error = hipSuccess; copies_left = 1;
    CHECK(!finish("demc_z", nullptr, {{a, src, sizeof a}, {b, src, sizeof b}, {a, src, sizeof a}}, err) && err == "demc_z: invalid argument" && copies == 3);
    copies_left = -1;
}

void pass_trace() {
    const int f0 = freed[EVT];
    {
        PassTrace tr;  // marks at 1, 3, 6 and 10 ms: passes of 2, 3 and 4 ms between consecutive marks, of 2 and 4 ms between pairs
        for (float t : {1.f, 3.f, 6.f, 10.f}) { now_ms = t; CHECK(tr.mark(nullptr)); }
        CHECK(tr.ev.size() == 4 && live(EVT) == 4);
        tr.print("devmem_host consecutive", 3, 1);
        tr.print("devmem_host pairs", 2, 2);
        events_left = 0;
        CHECK(!tr.mark(nullptr) && tr.ev.size() == 4);  // an event that cannot be created: nothing is kept
        events_left = -1;
    }
    CHECK(freed[EVT] == f0 + 4);
}

// StagedList: a device copy, a pinned host copy and the event between them, with their capacities
void staged_list() {
    const int dev0 = live(DEV), pin0 = live(PIN), evt0 = live(EVT);
    {
        StagedList<int> l;
        CHECK(!l.dev && !l.pin && !l.ev && l.dev_cap == 0 && l.pin_cap == 0);
        int* host = nullptr;
        int waits = event_waits, drains = stream_waits;
        CHECK(l.stage(4, nullptr, &host) == hipSuccess && host && host == l.pin.get() && l.dev && l.ev && l.dev_cap == 4 && l.pin_cap == 4);
        CHECK(live(DEV) == dev0 + 1 && live(PIN) == pin0 + 1 && live(EVT) == evt0 + 1);
        CHECK(event_waits == waits + 1 && stream_waits == drains);  // (no device buffer yet: no kernel to wait for)
        for (int i = 0; i < 4; ++i) host[i] = 10 + i;
        const int copied = async_copies;
        CHECK(l.send(4, nullptr) == hipSuccess && async_copies == copied + 1 && l.dev.get()[3] == 13);
        // the staging pointer again: the event is waited for before the caller rewrites the host buffer; nothing is allocated
        const int made_dev = made[DEV], made_pin = made[PIN], made_evt = made[EVT];
        waits = event_waits;
        CHECK(l.stage(3, nullptr, &host) == hipSuccess && host == l.pin.get() && event_waits == waits + 1);
        CHECK(made[DEV] == made_dev && made[PIN] == made_pin && made[EVT] == made_evt && stream_waits == drains && l.dev_cap == 4);
        // growing: the stream is waited for before the device buffer a kernel may still read goes; each old buffer is released once
        const int freed_dev = freed[DEV], freed_pin = freed[PIN];
        CHECK(l.stage(10, nullptr, &host) == hipSuccess && host && l.dev_cap == 10 && l.pin_cap == 10);
        CHECK(stream_waits == drains + 1 && freed[DEV] == freed_dev + 1 && freed[PIN] == freed_pin + 1 && live(DEV) == dev0 + 1 && live(PIN) == pin0 + 1);
        host[9] = 99;
        CHECK(l.send(10, nullptr) == hipSuccess && l.dev.get()[9] == 99);
        // an event that cannot be waited for, a stream that cannot: reported, nothing changed
        event_wait_error = hipErrorInvalidValue;
        CHECK(l.stage(2, nullptr, &host) == hipErrorInvalidValue && host == nullptr && l.dev_cap == 10 && l.pin_cap == 10 && l.dev && l.pin);
        event_wait_error = hipSuccess; sync_error = hipErrorInvalidValue;
        CHECK(l.stage(11, nullptr, &host) == hipErrorInvalidValue && host == nullptr && l.dev_cap == 10 && l.pin_cap == 10 && l.dev && l.pin);
        sync_error = hipSuccess;
        // a failed hipMalloc: the device side is empty with no capacity, the host side unchanged; the next call allocates again
        dev_allocs_left = 0;
        CHECK(l.stage(20, nullptr, &host) == hipErrorOutOfMemory && host == nullptr && !l.dev && l.dev_cap == 0 && l.pin && l.pin_cap == 10);
        CHECK(live(DEV) == dev0 && live(PIN) == pin0 + 1);
        dev_allocs_left = -1;
        drains = stream_waits;
        CHECK(l.stage(5, nullptr, &host) == hipSuccess && host && l.dev_cap == 5 && l.pin_cap == 10 && stream_waits == drains);
        // a failed hipHostMalloc: the host side is empty with no capacity, and no pointer is handed out
        pin_allocs_left = 0;
        CHECK(l.stage(30, nullptr, &host) == hipErrorOutOfMemory && host == nullptr && l.dev_cap == 30 && !l.pin && l.pin_cap == 0);
        pin_allocs_left = -1;
        CHECK(l.stage(30, nullptr, &host) == hipSuccess && host && l.pin_cap == 30 && live(DEV) == dev0 + 1 && live(PIN) == pin0 + 1);
    }
    CHECK(live(DEV) == dev0 && live(PIN) == pin0 && live(EVT) == evt0);  // destroyed: everything released
    {
        StagedList<int> l;  // an event that cannot be created: nothing is allocated
        int* host = nullptr;
        events_left = 0;
        CHECK(l.stage(4, nullptr, &host) == hipErrorOutOfMemory && host == nullptr && !l.ev && !l.dev && !l.pin && l.dev_cap == 0 && l.pin_cap == 0);
        events_left = -1;
        CHECK(live(DEV) == dev0 && live(PIN) == pin0 && live(EVT) == evt0);
        StagedList<int> ring[3];  // a ring sized once, as the handle's group lists are
        for (StagedList<int>& r : ring) CHECK(r.stage(7, nullptr, &host) == hipSuccess);
        CHECK(live(DEV) == dev0 + 3 && live(PIN) == pin0 + 3 && live(EVT) == evt0 + 3);
    }
    CHECK(live(DEV) == dev0 && live(PIN) == pin0 && live(EVT) == evt0);
}
}  // namespace

int main() {
    alloc_reset_destructor();
    moves();
    record_assignment();
    failed_allocations();
    call_endings();
    pass_trace();
    staged_list();
    for (int k = 0; k < N_KINDS; ++k) {
        CHECK(made[k] > 0);
        CHECK(live((Kind)k) == 0);
    }
    if (failures) std::fprintf(stderr, "%d check(s) failed\n", failures);
    else std::printf("devmem owners ok: %d device, %d pinned, %d event, %d module resources created and released\n", made[DEV], made[PIN], made[EVT], made[MOD]);
    return failures ? 1 : 0;
}
