// loc_lib_amd/csrc/device_buffer.hpp — who owns device memory, pinned host memory and events: every handle and workspace of the
// library holds its buffers as one of the three move-only types below, which free in their destructor. Buffers are grow-only and a
// growth discards the contents unless it is a grow_keep. A failed allocation leaves a buffer empty (get() == nullptr, cap() == 0),
// so the next call simply tries again. Host code only; pointers that do not own their memory stay raw `const T*`.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <utility>

#define LOCGPU_TRY(expr)                   \
    do {                                   \
        const hipError_t e_ = (expr);      \
        if (e_ != hipSuccess) return e_;   \
    } while (0)

namespace locgpu {

// the room a grow-only buffer is given beyond the n elements that made it grow
constexpr size_t with_headroom(size_t n) { return n + n / 4 + 1024; }

// hipMalloc memory; capacity in elements
template <typename T>
class DevBuf {
  public:
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr; o.cap_ = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) { reset(); swap(o); }
        return *this;
    }
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { reset(); }

    T* get() const { return p_; }
    operator T*() const { return p_; }
    size_t cap() const { return cap_; }
    void reset() {
        if (p_) (void)hipFree(p_);
        p_ = nullptr;
        cap_ = 0;
    }
    void swap(DevBuf& o) noexcept { std::swap(p_, o.p_); std::swap(cap_, o.cap_); }
    // exactly `count` elements, the old block freed first (peak memory = the larger of the two)
    hipError_t alloc(size_t count) {
        reset();
        LOCGPU_TRY(hipMalloc((void**)&p_, count * sizeof(T)));
        cap_ = count;
        return hipSuccess;
    }
    hipError_t reserve(size_t count) { return count <= cap_ ? hipSuccess : alloc(count); }
    // `count` elements of which the first `used` are the old block's: copied on `s`, `s` synchronised, then the old block freed.
    // On failure the old block stays as it was.
    hipError_t grow_keep(size_t count, size_t used, hipStream_t s) {
        T* q = nullptr;
        LOCGPU_TRY(hipMalloc((void**)&q, count * sizeof(T)));
        if (p_ && used) {
            hipError_t e = hipMemcpyAsync(q, p_, used * sizeof(T), hipMemcpyDeviceToDevice, s);
            if (e == hipSuccess) e = hipStreamSynchronize(s);
            if (e != hipSuccess) { (void)hipFree(q); return e; }
        }
        if (p_) (void)hipFree(p_);
        p_ = q;
        cap_ = count;
        return hipSuccess;
    }

  private:
    T* p_ = nullptr;
    size_t cap_ = 0;
};

// hipHostMalloc memory; capacity in elements
template <typename T>
class PinnedBuf {
  public:
    PinnedBuf() = default;
    PinnedBuf(PinnedBuf&& o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr; o.cap_ = 0; }
    PinnedBuf& operator=(PinnedBuf&& o) noexcept {
        if (this != &o) { reset(); swap(o); }
        return *this;
    }
    PinnedBuf(const PinnedBuf&) = delete;
    PinnedBuf& operator=(const PinnedBuf&) = delete;
    ~PinnedBuf() { reset(); }

    T* get() const { return p_; }
    operator T*() const { return p_; }
    T* operator->() const { return p_; }
    size_t cap() const { return cap_; }
    void reset() {
        if (p_) (void)hipHostFree(p_);
        p_ = nullptr;
        cap_ = 0;
    }
    void swap(PinnedBuf& o) noexcept { std::swap(p_, o.p_); std::swap(cap_, o.cap_); }
    hipError_t alloc(size_t count, unsigned flags = hipHostMallocDefault) {
        reset();
        LOCGPU_TRY(hipHostMalloc((void**)&p_, count * sizeof(T), flags));
        cap_ = count;
        return hipSuccess;
    }
    hipError_t reserve(size_t count, unsigned flags = hipHostMallocDefault) { return count <= cap_ ? hipSuccess : alloc(count, flags); }

  private:
    T* p_ = nullptr;
    size_t cap_ = 0;
};

// a hipEvent_t created on first use
class Event {
  public:
    Event() = default;
    Event(Event&& o) noexcept : ev_(o.ev_) { o.ev_ = nullptr; }
    Event& operator=(Event&& o) noexcept {
        if (this != &o) { reset(); std::swap(ev_, o.ev_); }
        return *this;
    }
    Event(const Event&) = delete;
    Event& operator=(const Event&) = delete;
    ~Event() { reset(); }

    operator hipEvent_t() const { return ev_; }
    hipError_t ensure(unsigned flags = hipEventDisableTiming) { return ev_ ? hipSuccess : hipEventCreateWithFlags(&ev_, flags); }
    void reset() {
        if (ev_) (void)hipEventDestroy(ev_);
        ev_ = nullptr;
    }

  private:
    hipEvent_t ev_ = nullptr;
};

}  // namespace locgpu
