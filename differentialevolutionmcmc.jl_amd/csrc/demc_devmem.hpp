// demc_devmem.hpp -- move-only owners of the HIP resources the host runtime holds.  Host code only: no kernel, no device function.
//
// Each owner holds one resource and releases it exactly once: in its destructor, in reset(), or when another owner is moved
// over it.  A record of owners (the handle's Model, its Replay) is therefore released by assigning a fresh record over it, and
// a handle by `delete`; nothing keeps a list of what to free.  The owners carry no size, no stream and no allocator: whoever
// frees memory that a stream may still read synchronises that stream first.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstddef>
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

}  // namespace demc
