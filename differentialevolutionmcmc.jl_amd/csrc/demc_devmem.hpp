// demc_devmem.hpp -- move-only owners of the HIP resources the host runtime holds, and on top of them the two things every
// posterior-statistics call does alike: its end (finish) and the timing of its passes (PassTrace).  Host code only: no kernel, no
// device function.
//
// Each owner holds one resource and releases it exactly once: in its destructor, in reset(), or when another owner is moved
// over it.  A record of owners (the handle's Model, its Replay) is therefore released by assigning a fresh record over it, and
// a handle by `delete`; nothing keeps a list of what to free.  The owners carry no size, no stream and no allocator: whoever
// frees memory that a stream may still read synchronises that stream first.  StagedList, built of three of them, is the one that
// knows its capacities and is told the stream: a list that reaches the device through pinned memory.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdio>
#include <initializer_list>
#include <string>
#include <utility>
#include <vector>

namespace demc {

struct FreeDevice { void operator()(void* p) const { (void)hipFree(p); } };
struct FreePinned { void operator()(void* p) const { (void)hipHostFree(p); } };
struct FreeEvent { void operator()(hipEvent_t e) const { (void)hipEventDestroy(e); } };
struct FreeModule { void operator()(hipModule_t m) const { (void)hipModuleUnload(m); } };

template <typename P, typename Free>  // P: a pointer or an opaque HIP handle (null: nothing held)
class Owned {
  public:
    Owned() = default;
    Owned(Owned&& o) noexcept : p_(o.p_) { o.p_ = nullptr; }
    Owned& operator=(Owned&& o) noexcept {
        if (this != &o) {
            reset();
            p_ = o.p_;
            o.p_ = nullptr;
        }
        return *this;
    }
    Owned(const Owned&) = delete;
    Owned& operator=(const Owned&) = delete;
    ~Owned() { reset(); }
    void reset() {
        if (p_) Free()(p_);
        p_ = nullptr;
    }
    P get() const { return p_; }
    operator P() const { return p_; }

  protected:
    template <typename F>
    hipError_t make(F&& create) {  // what was held before goes first; a failed creation leaves nothing held
        reset();
        const hipError_t e = create(&p_);
        if (e != hipSuccess) p_ = nullptr;
        return e;
    }

  private:
    P p_ = nullptr;
};

template <typename T>
struct DevBuf : Owned<T*, FreeDevice> {  // one hipMalloc allocation of n elements (not filled)
    hipError_t alloc(size_t n) { return this->make([&](T** p) { return hipMalloc((void**)p, n * sizeof(T)); }); }
};
template <typename T>
struct PinnedBuf : Owned<T*, FreePinned> {  // one hipHostMalloc allocation
    hipError_t alloc(size_t n, unsigned flags) { return this->make([&](T** p) { return hipHostMalloc((void**)p, n * sizeof(T), flags); }); }
};
struct Event : Owned<hipEvent_t, FreeEvent> {
    hipError_t create(unsigned flags) { return make([&](hipEvent_t* e) { return hipEventCreateWithFlags(e, flags); }); }
};
struct Module : Owned<hipModule_t, FreeModule> {
    hipError_t load(const void* image) { return make([&](hipModule_t* m) { return hipModuleLoadData(m, image); }); }
};

// A list staged through pinned memory: a device copy kernels read, a pinned host copy the next content is written into, and an
// event that says the last copy out of the host buffer has been consumed -- so refilling it is asynchronous for the host too (a
// pageable source would make the copy wait for everything queued on the stream), and the buffers outlive the call.  A failure
// leaves the owner empty or unchanged, never with a capacity it does not have.
template <typename T>
struct StagedList {
    DevBuf<T> dev;
    PinnedBuf<T> pin;
    Event ev;
    size_t dev_cap = 0, pin_cap = 0;
    // The host buffer, with room for n elements on both sides and free to be rewritten (the event has been waited for).  A device
    // buffer too small is replaced only once `st`, whose kernels may still read it, has been waited for.
    hipError_t stage(size_t n, hipStream_t st, T** host) {
        *host = nullptr;
        hipError_t e = ev ? hipSuccess : ev.create(hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventSynchronize(ev);
        if (e == hipSuccess && n > dev_cap) {
            if (dev) e = hipStreamSynchronize(st);
            if (e == hipSuccess) {
                dev_cap = 0;
                if ((e = dev.alloc(n)) == hipSuccess) dev_cap = n;
            }
        }
        if (e == hipSuccess && n > pin_cap) {
            pin_cap = 0;
            if ((e = pin.alloc(n, hipHostMallocDefault)) == hipSuccess) pin_cap = n;
        }
        if (e == hipSuccess) *host = pin;
        return e;
    }
    // the first n staged elements to the device, on `st`: behind every kernel of it that still reads the previous content
    hipError_t send(size_t n, hipStream_t st) {
        const hipError_t e = hipMemcpyAsync(dev, pin, n * sizeof(T), hipMemcpyHostToDevice, st);
        return e == hipSuccess ? hipEventRecord(ev, st) : e;
    }
};

struct Scratch {  // device allocations of one call, freed however it ends
    std::vector<DevBuf<char>> bufs;
    template <typename T>
    bool get(T** out, size_t n) {
        DevBuf<char> b;
        if (b.alloc((n ? n : 1) * sizeof(T)) != hipSuccess) return false;
        *out = (T*)b.get();
        bufs.push_back(std::move(b));
        return true;
    }
};

// How a call that has launched its kernels ends: their launch errors, the stream, then the copies to the host in order (a null
// dst was not asked for).  false: `err` is "<who>: <hip error>".
struct Download { void* dst; const void* src; size_t bytes; };
inline bool hip_ok(const char* who, hipError_t e, std::string& err) {
    if (e != hipSuccess) err = std::string(who) + ": " + hipGetErrorString(e);
    return e == hipSuccess;
}
inline bool finish(const char* who, hipStream_t st, std::initializer_list<Download> copies, std::string& err) {
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    for (const Download& c : copies)
        if (e == hipSuccess && c.dst) e = hipMemcpy(c.dst, c.src, c.bytes, hipMemcpyDeviceToHost);
    return hip_ok(who, e, err);
}

// Device time of the passes of a call, between marks on its stream.  Only the diagnostic variant of the library measures
// (make TRACE=1: -DDEMC_PASS_TRACE; tools/quantile_bench.py, tools/cov_bench.py); in the product both calls are empty.
struct PassTrace {
#ifdef DEMC_PASS_TRACE
    std::vector<Event> ev;
    bool mark(hipStream_t st) {
        Event e;
        if (e.create(hipEventDefault) != hipSuccess) return false;
        ev.push_back(std::move(e));
        return hipEventRecord(ev.back(), st) == hipSuccess;
    }
    // "<who> pass_ms a b ..." to stderr: pass i ran from mark i * stride to the one after it (the stream has been waited for)
    void print(const char* who, int passes, int stride) const {
        std::string line = std::string(who) + " pass_ms";
        for (int i = 0; i < passes; ++i) {
            float ms = 0.f;
            (void)hipEventElapsedTime(&ms, ev[(size_t)i * stride], ev[(size_t)i * stride + 1]);
            char buf[32];
            std::snprintf(buf, sizeof buf, " %.4f", ms);
            line += buf;
        }
        std::fprintf(stderr, "%s\n", line.c_str());
    }
#else
    bool mark(hipStream_t) { return true; }
    void print(const char*, int, int) const {}
#endif
};

}  // namespace demc
