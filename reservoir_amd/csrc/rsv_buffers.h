// rsv_buffers.h -- owning buffers over the resource pool (rsv_pool.h).
//
// A buffer holds one pool block and its own capacity in entries; the two change together only.  After a
// failed call a buffer is as it was, or empty with capacity 0 -- never a stale capacity over a null
// pointer.  A group of buffers that must all hold n entries has no capacity of its own: it is
// group_cap(members), the minimum, so a growth that failed half way is simply seen as too small by the
// next call.  The buffers choose no sizes: the growth policy (grown_capacity and each site's limit) stays
// with the caller.  Uses nothing of HIP but its types: a host program links it against stub pool functions.
#pragma once
#include <string.h>

#include <algorithm>
#include <utility>

#include "rsv_pool.h"

namespace rsv {

// n entries of T in device memory.  Growth synchronizes `st` before the old block goes back to the pool
// (pool_device_grow); the first allocation and a call within the capacity touch no stream.
template <typename T>
struct DevBuf {
    T* p = nullptr;
    int64_t cap = 0;  // entries

    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr, o.cap = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) release(), swap(o);
        return *this;
    }
    ~DevBuf() { release(); }  // the owner's stream is idle
    void swap(DevBuf& o) noexcept { std::swap(p, o.p), std::swap(cap, o.cap); }
    operator T*() const { return p; }

    // room for n entries, the first `used` kept
    hipError_t reserve_keep(int64_t n, int64_t used, hipStream_t st) {
        if (n <= cap) return hipSuccess;
        hipError_t e = pool_device_grow((void**)&p, (size_t)used * sizeof(T), (size_t)n * sizeof(T), used > 0, st);
        if (e == hipSuccess) cap = n;
        return e;
    }
    hipError_t reserve(int64_t n, hipStream_t st) { return reserve_keep(n, 0, st); }  // contents discarded
    void release() {
        pool_device_free(p);
        p = nullptr, cap = 0;
    }
};

// n entries of T in pinned host memory.  No queued copy may touch the block when it grows; `st` is
// taken for symmetry with DevBuf and not used.
template <typename T>
struct HostBuf {
    T* p = nullptr;
    int64_t cap = 0;

    HostBuf() = default;
    HostBuf(HostBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr, o.cap = 0; }
    HostBuf& operator=(HostBuf&& o) noexcept {
        if (this != &o) release(), swap(o);
        return *this;
    }
    ~HostBuf() { release(); }
    void swap(HostBuf& o) noexcept { std::swap(p, o.p), std::swap(cap, o.cap); }
    operator T*() const { return p; }

    hipError_t reserve_keep(int64_t n, int64_t used, hipStream_t = nullptr) {
        if (n <= cap) return hipSuccess;
        void* q = nullptr;
        if (hipError_t e = pool_host_alloc(&q, (size_t)n * sizeof(T), hipHostMallocDefault)) return e;
        if (used > 0) memcpy(q, p, (size_t)used * sizeof(T));
        pool_host_free(p);
        p = (T*)q, cap = n;
        return hipSuccess;
    }
    hipError_t reserve(int64_t n, hipStream_t = nullptr) { return reserve_keep(n, 0); }
    void release() {
        pool_host_free(p);
        p = nullptr, cap = 0;
    }
};

// a coherent, device-mapped host block of fixed size with its device alias (flag words and the few
// values a kernel publishes to a spinning host)
template <typename T>
struct MappedBuf {
    T* p = nullptr;
    T* dev = nullptr;
    int64_t cap = 0;

    MappedBuf() = default;
    MappedBuf(MappedBuf&& o) noexcept : p(o.p), dev(o.dev), cap(o.cap) { o.p = o.dev = nullptr, o.cap = 0; }
    MappedBuf& operator=(MappedBuf&& o) noexcept {
        if (this != &o) release(), swap(o);
        return *this;
    }
    ~MappedBuf() { release(); }
    void swap(MappedBuf& o) noexcept { std::swap(p, o.p), std::swap(dev, o.dev), std::swap(cap, o.cap); }
    operator T*() const { return p; }

    hipError_t reserve(int64_t n, hipStream_t = nullptr) {
        if (n <= cap) return hipSuccess;
        void *q = nullptr, *qd = nullptr;
        if (hipError_t e = pool_host_alloc_mapped(&q, &qd, (size_t)n * sizeof(T))) return e;
        pool_host_free(p);
        p = (T*)q, dev = (T*)qd, cap = n;
        return hipSuccess;
    }
    void release() {
        pool_host_free(p);
        p = dev = nullptr, cap = 0;
    }
    T* detach() {  // the block leaves its owner (pool_host_free is the new owner's to call)
        T* q = p;
        p = dev = nullptr, cap = 0;
        return q;
    }
};

// device scratch in bytes (rocPRIM's temporary storage): as large as the largest request so far
struct Scratch {
    DevBuf<unsigned char> b;
    void* p() const { return b.p; }
    size_t bytes() const { return (size_t)b.cap; }
    hipError_t reserve(size_t n, hipStream_t st) { return b.reserve((int64_t)n, st); }
};

// the capacity of a group of buffers that are sized together: what every member holds
template <typename B, typename... Bs>
int64_t group_cap(const B& b, const Bs&... bs) {
    int64_t c = b.cap;
    ((c = std::min<int64_t>(c, bs.cap)), ...);
    return c;
}

// every member to n entries (contents discarded), stopping at the first failure
template <typename... Bs>
hipError_t reserve_all(int64_t n, hipStream_t st, Bs&... bs) {
    hipError_t e = hipSuccess;
    ((e = e == hipSuccess ? bs.reserve(n, st) : e), ...);
    return e;
}

}  // namespace rsv
