// rsv_buffers.h -- owning buffers over the resource pool (rsv_pool.h).
//
// A buffer holds one pool block and its own capacity in entries; the two change together only.  After a
// failed call a buffer is as it was, or empty with capacity 0 -- never a stale capacity over a null
// pointer.  A group of buffers that must all hold n entries has no capacity of its own: it is
// group_cap(members), the minimum, so a growth that failed half way is simply seen as too small by the
// next call.  The buffers choose no sizes: the growth policy (grown_capacity and each site's limit) stays
// with the caller.  Behind the buffers, three types of the sampler handle (rsv_runtime.hip): its host landing
// zones, its pool events and its work clock.  Uses nothing of HIP but its types: a host program links it
// against stub pool functions.
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

// A host landing zone: entries of host memory a kernel delivers into.  Published form: a coherent, mapped
// block with a 64-byte flag line behind the entries, into which the kernel stores the generation after
// them (the host spins on it); pinned form: the target of a D2H copy and a stream synchronize.  The first
// ensure chooses the form; afterwards the form is which of the two owners holds a block.
struct Landing {
    MappedBuf<uint8_t> pub;
    HostBuf<uint8_t> pin;
    uint32_t gen = 0;  // the newest generation issued (the flag starts there: nothing published yet)

    bool published() const { return pub.p != nullptr; }
    void* host() const { return pub.p ? (void*)pub.p : (void*)pin.p; }
    void* dev() const { return pub.dev; }
    uint32_t* flag() const { return (uint32_t*)(pub.p + pub.cap - 64); }
    uint32_t* flag_dev() const { return (uint32_t*)(pub.dev + pub.cap - 64); }
    uint32_t next_gen() { return ++gen; }
    hipError_t ensure(size_t bytes, bool may_publish) {
        if (host()) return hipSuccess;
        if (!may_publish) return pin.reserve((int64_t)bytes);
        if (hipError_t e = pub.reserve((int64_t)((bytes + 63) & ~(size_t)63) + 64)) return e;
        *flag() = gen;
        return hipSuccess;
    }
    void* give() { return pub.detach(); }  // the published block leaves (pool_host_free is the taker's to call)
};

// A pool event with its device and flags: taken at first use, returned with its owner -- whose queued work
// has completed by then.
struct PoolEvent {
    hipEvent_t e = nullptr;
    int device = 0;
    unsigned flags = 0;

    PoolEvent() = default;
    PoolEvent(PoolEvent&& o) noexcept : e(o.e), device(o.device), flags(o.flags) { o.e = nullptr; }
    PoolEvent& operator=(PoolEvent&& o) noexcept {
        if (this != &o) release(), std::swap(e, o.e), device = o.device, flags = o.flags;
        return *this;
    }
    ~PoolEvent() { release(); }
    operator hipEvent_t() const { return e; }
    hipError_t ensure(int dev, unsigned fl) {  // on the current device, which is `dev`
        if (e) return hipSuccess;
        device = dev, flags = fl;
        return pool_event(&e, fl);
    }
    void release() {
        if (e) pool_release_event(device, e, flags);
        e = nullptr;
    }
};

// A handle's work clock.  Device work is enqueued on the handle's stream in groups (`ops`); `ops_done` are the
// groups known complete.  A launch may publish the reservoir into the result's landing zone: pub_ops / pub_gen
// are that launch's group and generation, and pub_valid says that nothing has changed the slots since.
struct WorkClock {
    uint64_t ops = 0, ops_done = 0, pub_ops = 0;
    uint32_t pub_gen = 0;
    bool pub_valid = false;

    void group() { ++ops; }             // a new group of device work
    void drained() { ops_done = ops; }  // a stream synchronize returned: everything enqueued is complete
    bool idle() const { return ops == ops_done; }
    // a launch of the current group changed the slots and published them as generation g, or (!did) not at all
    void published(bool did, uint32_t g) {
        pub_valid = did;
        if (did) pub_ops = ops, pub_gen = g;
    }
    void invalidate() { pub_valid = false; }  // the slots changed behind the publication
    bool holds() const { return pub_valid; }  // the publication has the current slots
    bool current() const { return pub_valid && pub_ops == ops; }  // ... and no group of work came after it
    // the host has seen generation g of a landing zone whose newest is `newest`, stored as the last memory
    // operation of group `at`: where that is the last group, everything is complete
    void seen(uint64_t at, uint32_t g, uint32_t newest) {
        if (at == ops && g == newest) ops_done = ops;
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
