// devmem_host.cpp -- the owners of csrc/demc_devmem.hpp on the CPU: the HIP entry points the header calls are counting stubs over
// malloc / free, so every create and every release is seen, and a release too many or too few is a miscount here and a
// double free or a leak to the address sanitizer the program is built with (tests/test_devmem_host.py).  No HIP runtime is linked.
#include "demc_devmem.hpp"

#include <cstdio>
#include <cstdlib>

namespace {
enum Kind { DEV, PIN, EVT, MOD, N_KINDS };
int made[N_KINDS], freed[N_KINDS];
int dev_allocs_left = -1;  // hipMalloc fails once this many have succeeded (-1: never)

hipError_t make(Kind k, void** out, size_t bytes) {
    if (k == DEV && dev_allocs_left == 0) return hipErrorOutOfMemory;
    if (k == DEV && dev_allocs_left > 0) --dev_allocs_left;
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
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) { return make(EVT, (void**)e, 1); }
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
}  // namespace

int main() {
    alloc_reset_destructor();
    moves();
    record_assignment();
    failed_allocations();
    for (int k = 0; k < N_KINDS; ++k) {
        CHECK(made[k] > 0);
        CHECK(live((Kind)k) == 0);
    }
    if (failures) std::fprintf(stderr, "%d check(s) failed\n", failures);
    else std::printf("devmem owners ok: %d device, %d pinned, %d event, %d module resources created and released\n", made[DEV], made[PIN], made[EVT], made[MOD]);
    return failures ? 1 : 0;
}
