// emi_device_array.hpp -- move-only owner of one array in device memory (or, Pinned, in page-locked host memory).
//
// The workspaces of the library are reused across problems of different sizes: a buffer grows when a problem needs more than it
// holds and is never shrunk.  reserve() is that rule, the destructor is the matching free: a buffer that is a member of a
// workspace cannot be forgotten in a hand-kept list when the workspace goes.  The owner of the workspace makes the right device
// current and drains its streams before it destroys it.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>

namespace emi {

template <class T, bool Pinned = false>
struct DeviceArray {
    T* p = nullptr;
    size_t cap = 0;             // elements allocated

    DeviceArray() = default;
    DeviceArray(const DeviceArray&) = delete;
    DeviceArray& operator=(const DeviceArray&) = delete;
    DeviceArray(DeviceArray&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    DeviceArray& operator=(DeviceArray&& o) noexcept {
        if (this != &o) {
            (void)release();
            p = o.p; cap = o.cap;
            o.p = nullptr; o.cap = 0;
        }
        return *this;
    }
    ~DeviceArray() { (void)release(); }

    size_t bytes() const { return cap * sizeof(T); }

    hipError_t release() {
        T* old = p;
        p = nullptr;
        cap = 0;
        if (!old) return hipSuccess;
        return Pinned ? hipHostFree(old) : hipFree(old);
    }
    // Room for `count` elements.  A buffer that is large enough stays as it is; one that is not is freed and allocated anew at
    // exactly `count` (the contents are NOT kept; growth policies belong to the caller).  *moved: whether that happened.
    hipError_t reserve(size_t count, bool* moved = nullptr) {
        if (moved) *moved = false;
        if (cap >= count) return hipSuccess;
        hipError_t e = release();
        if (e != hipSuccess) return e;
        e = Pinned ? hipHostMalloc((void**)&p, count * sizeof(T), hipHostMallocDefault) : hipMalloc((void**)&p, count * sizeof(T));
        if (e != hipSuccess) { p = nullptr; return e; }
        cap = count;
        if (moved) *moved = true;
        return hipSuccess;
    }
};
template <class T>
using PinnedArray = DeviceArray<T, true>;

}  // namespace emi
