// Owners of the GPU resources the host code holds: one device or pinned allocation, one event, one stream each.  Move-only,
// released by the destructor.  Every raw allocation / release call of the library is in this file, and so is the only code
// that touches the four live-resource counters (lwp_debug_live_resources): what a handle took and what it gave back can be
// compared from outside.  Host-only; nothing here knows about lwp_context.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstddef>
#include <cstdint>
#include <utility>

namespace lwp {

struct LiveResources { std::atomic<int64_t> dev_bytes{0}, pin_bytes{0}, events{0}, streams{0}; };
inline LiveResources& live_resources() { static LiveResources r; return r; }

struct DeviceMem {
    static hipError_t alloc(void** p, size_t bytes) { return hipMalloc(p, bytes); }
    static hipError_t release(void* p) { return hipFree(p); }
    static std::atomic<int64_t>& live() { return live_resources().dev_bytes; }
};
struct PinnedMem {
    static hipError_t alloc(void** p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
    static hipError_t release(void* p) { return hipHostFree(p); }
    static std::atomic<int64_t>& live() { return live_resources().pin_bytes; }
};

template <class Mem>
class Buf {
public:
    Buf() = default;
    Buf(const Buf&) = delete;
    Buf& operator=(const Buf&) = delete;
    Buf(Buf&& o) noexcept : p_(std::exchange(o.p_, nullptr)), bytes_(std::exchange(o.bytes_, 0)) {}
    Buf& operator=(Buf&& o) noexcept {
        if (this != &o) { (void)reset(); p_ = std::exchange(o.p_, nullptr); bytes_ = std::exchange(o.bytes_, 0); }
        return *this;
    }
    ~Buf() { (void)reset(); }

    // grow-only: nothing happens while `bytes` fits, else the old allocation is released and a new one made (contents are
    // not kept).  After a failure the buffer is empty.
    hipError_t ensure(size_t bytes) {
        if (bytes <= bytes_) return hipSuccess;
        hipError_t e = reset();
        if (e != hipSuccess) return e;
        e = Mem::alloc(&p_, bytes);
        if (e != hipSuccess) { p_ = nullptr; return e; }
        bytes_ = bytes;
        Mem::live() += (int64_t)bytes;
        return hipSuccess;
    }
    hipError_t reset() {
        if (!p_) return hipSuccess;
        Mem::live() -= (int64_t)bytes_;
        const hipError_t e = Mem::release(p_);
        p_ = nullptr; bytes_ = 0;
        return e;
    }
    template <class T> T* as() const { return static_cast<T*>(p_); }
    size_t size() const { return bytes_; }
    explicit operator bool() const { return p_ != nullptr; }

private:
    void* p_ = nullptr;
    size_t bytes_ = 0;
};
using DevBuf = Buf<DeviceMem>;     // one hipMalloc allocation
using PinBuf = Buf<PinnedMem>;     // one pinned host allocation (hipHostMallocDefault)

// created by the first ensure(), with the flags of that call site
class Event {
public:
    Event() = default;
    Event(const Event&) = delete;
    Event& operator=(const Event&) = delete;
    Event(Event&& o) noexcept : e_(std::exchange(o.e_, nullptr)) {}
    Event& operator=(Event&& o) noexcept {
        if (this != &o) { reset(); e_ = std::exchange(o.e_, nullptr); }
        return *this;
    }
    ~Event() { reset(); }
    hipError_t ensure(unsigned flags = hipEventDefault) {
        if (e_) return hipSuccess;
        const hipError_t e = hipEventCreateWithFlags(&e_, flags);
        if (e != hipSuccess) { e_ = nullptr; return e; }
        live_resources().events += 1;
        return hipSuccess;
    }
    void reset() {
        if (!e_) return;
        live_resources().events -= 1;
        (void)hipEventDestroy(e_);
        e_ = nullptr;
    }
    operator hipEvent_t() const { return e_; }

private:
    hipEvent_t e_ = nullptr;
};

// a non-blocking stream, created by the first ensure()
class Stream {
public:
    Stream() = default;
    Stream(const Stream&) = delete;
    Stream& operator=(const Stream&) = delete;
    ~Stream() {
        if (!s_) return;
        live_resources().streams -= 1;
        (void)hipStreamDestroy(s_);
    }
    hipError_t ensure() {
        if (s_) return hipSuccess;
        const hipError_t e = hipStreamCreateWithFlags(&s_, hipStreamNonBlocking);
        if (e != hipSuccess) { s_ = nullptr; return e; }
        live_resources().streams += 1;
        return hipSuccess;
    }
    operator hipStream_t() const { return s_; }

private:
    hipStream_t s_ = nullptr;
};

}  // namespace lwp
