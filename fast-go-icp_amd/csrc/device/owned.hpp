// Move-only owners of what a context, a batch or a one-shot call holds on the device: a field whose type releases it cannot be forgotten.
//   Dev<T>      a device array                            Mapped<T>   pinned host memory and, if mapped, its device alias
//   Stream      a stream it created, or one it borrows    Event       an event
// Each converts to the raw pointer / handle it wraps, so a field keeps its name at every use.  A create that fails leaves the handle empty
// and returns the hipError_t.  The four live counts (fgoicp_test_live_resources) say how many of each kind the process's handles hold.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstddef>
#include <cstdint>
#include <utility>

namespace fgoicp {
namespace live {  // {device allocations, pinned allocations, streams, events} held by handles
inline std::atomic<uint64_t> dev{0}, pinned{0}, streams{0}, events{0};
}
struct NoExtra {};
template <class T> void release_dev(T* p, NoExtra) { (void)hipFree(p); --live::dev; }
template <class T> void release_pinned(T* p, T* /*alias*/) { (void)hipHostFree(p); --live::pinned; }
inline void release_event(hipEvent_t e, NoExtra) { (void)hipEventDestroy(e); --live::events; }
inline void release_stream(hipStream_t s, bool owned) {  // an owned stream is drained, then destroyed; a borrowed one is only forgotten
    if (owned) { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); --live::streams; }
}

// what the four share: one raw handle and what goes with it (Mapped: the device alias; Stream: whether it is owned), moved together, given
// back together by Release; a moved-from or reset handle holds {nullptr, Extra{}}
template <class Raw, class Extra, void (*Release)(Raw, Extra)>
class Owner {
  protected:
    Raw h_ = nullptr;
    Extra x_{};
    hipError_t adopt(hipError_t e, std::atomic<uint64_t>& count) {  // after a create into h_: empty on failure, counted on success
        if (e != hipSuccess) h_ = nullptr;
        if (h_) ++count;
        return e;
    }

  public:
    Owner() = default;
    Owner(Owner&& o) noexcept : h_(std::exchange(o.h_, nullptr)), x_(std::exchange(o.x_, Extra{})) {}
    Owner& operator=(Owner&& o) noexcept {
        if (this != &o) { reset(); h_ = std::exchange(o.h_, nullptr); x_ = std::exchange(o.x_, Extra{}); }
        return *this;
    }
    ~Owner() { reset(); }
    void reset() {
        if (h_) Release(h_, x_);
        h_ = nullptr;
        x_ = Extra{};
    }
    Raw get() const { return h_; }
    operator Raw() const { return h_; }
    explicit operator bool() const { return h_ != nullptr; }
};

template <class T>
struct Dev : Owner<T*, NoExtra, release_dev<T>> {
    hipError_t alloc(size_t count) {  // releases what it held first
        this->reset();
        return this->adopt(hipMalloc(&this->h_, sizeof(T) * count), live::dev);
    }
    hipError_t ensure(size_t count) { return this->h_ ? hipSuccess : alloc(count); }  // only if empty: a call that failed half-way can be repeated
};

template <class T>
struct Mapped : Owner<T*, T*, release_pinned<T>> {
    hipError_t alloc(size_t count, unsigned flags = hipHostMallocMapped) {  // the alias only where the flags map the memory
        this->reset();
        hipError_t e = this->adopt(hipHostMalloc((void**)&this->h_, sizeof(T) * count, flags), live::pinned);
        if (e == hipSuccess && (flags & hipHostMallocMapped)) e = hipHostGetDevicePointer((void**)&this->x_, this->h_, 0);
        if (e != hipSuccess) this->reset();
        return e;
    }
    hipError_t ensure(size_t count, unsigned flags = hipHostMallocMapped) { return this->h_ ? hipSuccess : alloc(count, flags); }
    T* dev() const { return this->x_; }  // the device alias
};

struct Stream : Owner<hipStream_t, bool, release_stream> {
    hipError_t create(unsigned flags) { reset(); return own(hipStreamCreateWithFlags(&h_, flags)); }
    hipError_t create(unsigned flags, int priority) { reset(); return own(hipStreamCreateWithPriority(&h_, flags, priority)); }
    void borrow(hipStream_t s) { reset(); h_ = s; }  // someone else's: never synchronised or destroyed here
    void sync() const { if (h_ && x_) (void)hipStreamSynchronize(h_); }
    bool owned() const { return x_; }

  private:
    hipError_t own(hipError_t e) { e = adopt(e, live::streams); x_ = h_ != nullptr; return e; }
};

struct Event : Owner<hipEvent_t, NoExtra, release_event> {
    hipError_t create(unsigned flags = hipEventDefault) { reset(); return adopt(hipEventCreateWithFlags(&h_, flags), live::events); }
};

}  // namespace fgoicp
