// device_buffer.hpp -- the one owner of device memory: every table, workspace and scratch of the library is a DeviceBuffer member of the
// object that uses it, and is freed when that object is deleted.  Host code; the HIP runtime's declarations only, so that the CPU suite can
// run it against a runtime of its own (tests/cpp/device_buffer_check.cpp).
//
// Who owns: the context its tables and workspaces, a family's table struct its tables and scratch, a live ring, view, image or filterbank
// its own buffers.  Nothing is shared: kernels get raw pointers from get(), in their Params.
// When the stream is waited for: a buffer that enqueued work may still read is never freed under it -- grow() waits for the stream it is
// given, and whoever replaces or deletes tables synchronizes first (sgx_destroy, upload_palette, sgx_magnitude_in, the destroy calls of
// the objects above).  The buffer itself never synchronizes on destruction.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <vector>

namespace sgx {

template <typename T>
class DeviceBuffer {
public:
    DeviceBuffer() = default;
    DeviceBuffer(const DeviceBuffer &) = delete;
    DeviceBuffer &operator=(const DeviceBuffer &) = delete;
    DeviceBuffer(DeviceBuffer &&o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr; o.n_ = 0; }
    DeviceBuffer &operator=(DeviceBuffer &&o) noexcept
    {
        if (this != &o) {
            reset();
            p_ = o.p_; n_ = o.n_;
            o.p_ = nullptr; o.n_ = 0;
        }
        return *this;
    }
    ~DeviceBuffer() { reset(); }

    T *get() const { return p_; }
    size_t size() const { return n_; }   // elements
    void reset()
    {
        if (p_) (void)hipFree(p_);
        p_ = nullptr;
        n_ = 0;
    }

    // n elements, uninitialised, in place of what the buffer held (n == 0: none, a null pointer)
    hipError_t alloc(size_t n)
    {
        reset();
        if (n == 0) return hipSuccess;
        const hipError_t e = hipMalloc(reinterpret_cast<void **>(&p_), n * sizeof(T));
        if (e != hipSuccess) { p_ = nullptr; return e; }
        n_ = n;
        return hipSuccess;
    }
    // a host table, allocated and copied synchronously.  An EMPTY table leaves a null pointer: predicates and kernels test for it.
    hipError_t upload(const T *src, size_t n)
    {
        const hipError_t e = alloc(n);
        return e != hipSuccess || n == 0 ? e : hipMemcpy(p_, src, n * sizeof(T), hipMemcpyHostToDevice);
    }
    hipError_t upload(const std::vector<T> &v) { return upload(v.data(), v.size()); }
    // the same for a table whose kernel takes a valid pointer whatever its length: an empty table gets one element, which nothing reads
    hipError_t upload_at_least_one(const std::vector<T> &v)
    {
        const hipError_t e = alloc(v.size() ? v.size() : 1);
        return e != hipSuccess || v.empty() ? e : hipMemcpy(p_, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
    }
    // Scratch that launches on `stream` may still use, to `want` elements at least: nothing where it holds them; else wait for the stream,
    // free, allocate.  A failed allocation leaves the buffer null and its size 0.  The contents are not kept.
    hipError_t grow(hipStream_t stream, size_t want)
    {
        if (want <= n_) return hipSuccess;
        const hipError_t e = hipStreamSynchronize(stream);
        return e != hipSuccess ? e : alloc(want);
    }

private:
    T *p_ = nullptr;
    size_t n_ = 0;
};

}  // namespace sgx
