// dev_buf.hpp - owning types for device and pinned-host allocations: every hipMalloc / hipFree / hipHostMalloc / hipHostFree
// of the library is in this file.  Plain C++ over those four calls (and hipError_t / hipSuccess), which the includer declares:
// the HIP runtime in the library, counting stand-ins in tests/host/dev_buf_main.cpp (g++ -fsanitize=address,undefined).
#pragma once
#include <cstddef>
#include <cstdint>

// Move-only owner of `cap` elements at `p` (PINNED: page-locked host memory instead of device memory).  The raw pointer is
// spelled `.p` at every use.  hipFree waits for the whole device, so nothing here frees behind the caller's back: only
// release(), the destructor, a move assignment, and grow() beyond the capacity.
template <class T, bool PINNED = false>
struct DevBuf {
    T* p = nullptr;
    size_t cap = 0;  // elements
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr, o.cap = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) {
            release();
            p = o.p, cap = o.cap;
            o.p = nullptr, o.cap = 0;
        }
        return *this;
    }
    ~DevBuf() { release(); }
    void release() {
        if (p) (void)(PINNED ? hipHostFree(p) : hipFree(p));
        p = nullptr, cap = 0;
    }
    // n elements in place of whatever the buffer held (released first); on failure the buffer is empty
    hipError_t alloc(size_t n) {
        release();
        void* q = nullptr;
        const hipError_t e = PINNED ? hipHostMalloc(&q, sizeof(T) * n) : hipMalloc(&q, sizeof(T) * n);
        if (e != hipSuccess) return e;
        p = static_cast<T*>(q), cap = n;
        return hipSuccess;
    }
    // grow-only: nothing happens while n fits; otherwise release, then allocate (bounds the peak; contents are not kept)
    hipError_t grow(size_t n) { return n <= cap ? hipSuccess : alloc(n); }
};
template <class T>
using PinnedBuf = DevBuf<T, true>;
