// How the host code owns device memory: one move-only owner of one allocation, and its stream-ordered twin for the scratch
// of a single call.  Header-only and free of HIP: the runtime calls come from a policy (HipMemory in host_common.hpp; a
// counting heap in tests/native/device_buffer.cpp), so that a host compiler can build and check the logic.
//
// A policy has: error_t, ok, stream_t, alloc(void**, bytes), free(void*), copy_in(dst, src, bytes), zero(dst, bytes),
// alloc_async(void**, bytes, stream), free_async(void*, stream), clear_error().
//
// Build-then-commit: a function that replaces several buffers of a handle fills LOCAL buffers first and moves them into the
// handle only when every one exists.  A failure on the way returns with the handle untouched, and the locals' destructors
// release what was built.
#pragma once
#include <cstddef>

namespace fx {

template <class T, class Policy>
class DeviceBuffer {
public:
    using error_t = typename Policy::error_t;

    DeviceBuffer() = default;
    DeviceBuffer(DeviceBuffer&& o) noexcept : p_(o.p_) { o.p_ = nullptr; }
    DeviceBuffer& operator=(DeviceBuffer&& o) noexcept {
        if (this != &o) {
            (void)reset();
            p_ = o.p_;
            o.p_ = nullptr;
        }
        return *this;
    }
    DeviceBuffer(const DeviceBuffer&) = delete;
    DeviceBuffer& operator=(const DeviceBuffer&) = delete;
    ~DeviceBuffer() { (void)reset(); }

    T* get() const { return p_; }
    explicit operator bool() const { return p_ != nullptr; }

    // frees the allocation, if there is one; the buffer is empty afterwards whatever the runtime answered
    error_t reset() {
        T* p = p_;
        p_ = nullptr;
        return p ? Policy::free(p) : Policy::ok;
    }

    // `count` elements, zeroed on request.  On failure the buffer is empty and the runtime's sticky error is cleared.
    error_t alloc(size_t count, bool zeroed = false) {
        (void)reset();
        void* p = nullptr;
        error_t e = Policy::alloc(&p, count * sizeof(T));
        if (e == Policy::ok && zeroed) e = Policy::zero(p, count * sizeof(T));
        return adopt(p, e);
    }

    // max(count, room) elements with the first `count` copied from the host (nothing is copied where count is 0); same contract
    error_t upload(const T* src, size_t count, size_t room = 0) {
        (void)reset();
        void* p = nullptr;
        error_t e = Policy::alloc(&p, (count > room ? count : room) * sizeof(T));
        if (e == Policy::ok && count) e = Policy::copy_in(p, src, count * sizeof(T));
        return adopt(p, e);
    }

private:
    error_t adopt(void* p, error_t e) {
        if (e == Policy::ok) {
            p_ = static_cast<T*>(p);
        } else {
            if (p) (void)Policy::free(p);
            Policy::clear_error();
        }
        return e;
    }
    T* p_ = nullptr;
};

// Scratch of one call, allocated and released in stream order: the memory returns to the pool only after the work enqueued
// on the stream before the end of the scope has read it.  Neither copied nor moved: it lives in the scope that made it.
template <class T, class Policy>
class StreamScratch {
public:
    using error_t = typename Policy::error_t;
    using stream_t = typename Policy::stream_t;

    StreamScratch() = default;
    StreamScratch(const StreamScratch&) = delete;
    StreamScratch& operator=(const StreamScratch&) = delete;
    ~StreamScratch() {
        if (p_) (void)Policy::free_async(p_, s_);
    }

    T* get() const { return p_; }

    // once per object; on failure it stays empty and the runtime's sticky error is cleared
    error_t alloc(size_t count, stream_t s) {
        void* p = nullptr;
        error_t e = Policy::alloc_async(&p, count * sizeof(T), s);
        if (e != Policy::ok) {
            Policy::clear_error();
            return e;
        }
        p_ = static_cast<T*>(p);
        s_ = s;
        return e;
    }

private:
    T* p_ = nullptr;
    stream_t s_{};
};

}  // namespace fx
