// tmpt_device.h -- the owners of everything the host code gets from HIP:
// device memory, pinned host memory, events and streams (DESIGN.md "Owners").
// The allocation and creation calls appear in this header and nowhere else
// in csrc/ (tests/test_device_owners.py); a buffer, event or stream is a
// member or a local of one of these types and is released when that goes out
// of scope, on every return path and through TMPT_GUARD's exceptions.
// Host-only, move-only (a buffer can also be move-assigned: the old one is
// freed, then the new one taken).  Each owner converts to the raw pointer or
// handle it holds, so launches and HIP calls read as before; kernels see raw
// pointers.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>
#include <utility>

namespace tmpt {

// live device allocations + pinned allocations + events + streams of the
// process (tmpt_scene_get_option "live_device_objects"); only the owners below
// change it
inline std::atomic<int64_t> g_live_device_objects{0};

// "num/den of the free device memory, plus what the caller already holds (and
// would free first)": the arithmetic of every kept buffer's budget.  The
// fraction, the buffers counted as held and the option cap are each site's own.
inline size_t free_budget(size_t num, size_t den, size_t already_held)
{
    size_t fr = 0, tot = 0;
    if (hipMemGetInfo(&fr, &tot) != hipSuccess) fr = 0;
    return fr / den * num + already_held;
}

// Device memory: a pointer and its size in bytes (all sizes here are bytes,
// whatever T is).
template <typename T = void>
class DeviceBuffer {
public:
    DeviceBuffer() = default;
    DeviceBuffer(DeviceBuffer&& o) noexcept : p_(std::exchange(o.p_, nullptr)), bytes_(std::exchange(o.bytes_, 0)) {}
    DeviceBuffer& operator=(DeviceBuffer&& o) noexcept
    {
        if (this != &o) {
            reset();
            p_ = std::exchange(o.p_, nullptr);
            bytes_ = std::exchange(o.bytes_, 0);
        }
        return *this;
    }
    ~DeviceBuffer() { reset(); }
    T* get() const { return p_; }
    operator T*() const { return p_; }
    template <typename U>
    U* as() const  // a DeviceBuffer<>'s bytes as U
    {
        return static_cast<U*>(p_);
    }
    size_t bytes() const { return bytes_; }
    void reset()
    {
        if (p_) {
            (void)hipFree(p_);
            --g_live_device_objects;
        }
        p_ = nullptr;
        bytes_ = 0;
    }
    // frees what is held, then allocates; false (owner empty, HIP's error
    // cleared) when the allocation fails
    bool alloc(size_t bytes)
    {
        reset();
        void* p = nullptr;
        if (hipMalloc(&p, bytes) != hipSuccess) {
            (void)hipGetLastError();
            return false;
        }
        p_ = static_cast<T*>(p);
        bytes_ = bytes;
        if (p_) ++g_live_device_objects;  // (0 bytes: success and no allocation)
        return true;
    }
    // nothing when the buffer is already that large, else alloc: the old
    // buffer is freed before the new one is made, so the peak is the larger
    bool reserve(size_t bytes) { return bytes_ >= bytes || alloc(bytes); }

private:
    T* p_ = nullptr;
    size_t bytes_ = 0;
};

// Pinned host memory (hipHostMallocDefault), made once.
template <typename T>
class PinnedBuffer {
public:
    PinnedBuffer() = default;
    PinnedBuffer(PinnedBuffer&& o) noexcept : p_(std::exchange(o.p_, nullptr)) {}
    ~PinnedBuffer() { reset(); }
    T* get() const { return p_; }
    operator T*() const { return p_; }
    void reset()
    {
        if (p_) {
            (void)hipHostFree(p_);
            --g_live_device_objects;
        }
        p_ = nullptr;
    }
    hipError_t ensure(size_t bytes)
    {
        if (p_) return hipSuccess;
        void* p = nullptr;
        const hipError_t e = hipHostMalloc(&p, bytes, hipHostMallocDefault);
        if (e != hipSuccess) return e;
        p_ = static_cast<T*>(p);
        ++g_live_device_objects;
        return hipSuccess;
    }

private:
    T* p_ = nullptr;
};

// An event and a stream, each created on first use by ensure(flags).
class Event {
public:
    Event() = default;
    Event(Event&& o) noexcept : h_(std::exchange(o.h_, nullptr)) {}
    ~Event() { reset(); }
    hipEvent_t get() const { return h_; }
    operator hipEvent_t() const { return h_; }
    void reset()
    {
        if (h_) {
            (void)hipEventDestroy(h_);
            --g_live_device_objects;
        }
        h_ = nullptr;
    }
    hipError_t ensure(unsigned flags = hipEventDefault)
    {
        if (h_) return hipSuccess;
        const hipError_t e = hipEventCreateWithFlags(&h_, flags);
        if (e != hipSuccess) {
            h_ = nullptr;
            return e;
        }
        ++g_live_device_objects;
        return hipSuccess;
    }

private:
    hipEvent_t h_ = nullptr;
};

class Stream {
public:
    Stream() = default;
    Stream(Stream&& o) noexcept : h_(std::exchange(o.h_, nullptr)) {}
    ~Stream() { reset(); }
    hipStream_t get() const { return h_; }
    operator hipStream_t() const { return h_; }
    void reset()
    {
        if (h_) {
            (void)hipStreamDestroy(h_);
            --g_live_device_objects;
        }
        h_ = nullptr;
    }
    hipError_t ensure(unsigned flags = hipStreamNonBlocking)
    {
        if (h_) return hipSuccess;
        const hipError_t e = hipStreamCreateWithFlags(&h_, flags);
        if (e != hipSuccess) {
            h_ = nullptr;
            return e;
        }
        ++g_live_device_objects;
        return hipSuccess;
    }

private:
    hipStream_t h_ = nullptr;
};

}  // namespace tmpt
