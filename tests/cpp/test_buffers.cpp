// The owning buffers of reservoir_amd/csrc/rsv_buffers.h over stub pool functions (malloc, a live-block
// count, an allocation that can be told to fail): capacity and pointer change together, a group's capacity
// never runs ahead of a member, and every block goes back to the pool.  Then the sampler handle's types from
// the same header: the landing zone, the event owner (stub events, counted the same way) and the work clock.
// Host only: no HIP library is linked.
#include <assert.h>
#include <stdio.h>
#include <stdlib.h>

#include <set>

#include "rsv_buffers.h"

namespace {
std::set<void*> g_live;
long g_allocs = 0;      // allocations asked for since the last arm()
long g_fail_at = 0;     // the g_fail_at-th allocation after arm() fails (0: none)
void arm(long n) { g_allocs = 0, g_fail_at = n; }

hipError_t stub_alloc(void** p, size_t bytes) {
    if (++g_allocs == g_fail_at) return hipErrorOutOfMemory;
    *p = malloc(bytes ? bytes : 16);
    g_live.insert(*p);
    return hipSuccess;
}
void stub_free(void* p) {
    if (!p) return;
    assert(g_live.erase(p) == 1);  // ours, and freed once
    free(p);
}
}  // namespace

namespace rsv {
hipError_t pool_device_alloc(void** p, size_t bytes) { return stub_alloc(p, bytes); }
void pool_device_free(void* p) { stub_free(p); }
hipError_t pool_device_grow(void** p, size_t old_bytes, size_t new_bytes, bool keep, hipStream_t) {
    void* q = nullptr;
    if (hipError_t e = stub_alloc(&q, new_bytes)) return e;
    if (keep && *p && old_bytes) memcpy(q, *p, old_bytes);
    stub_free(*p);
    *p = q;
    return hipSuccess;
}
hipError_t pool_host_alloc(void** p, size_t bytes, unsigned) { return stub_alloc(p, bytes); }
hipError_t pool_host_alloc_mapped(void** p, void** dev_alias, size_t bytes) {
    if (hipError_t e = stub_alloc(p, bytes)) return e;
    *dev_alias = *p;
    return hipSuccess;
}
void pool_host_free(void* p) { stub_free(p); }
// events: a live set like the blocks', with the device and flags each was taken with
hipError_t pool_event(hipEvent_t* out, unsigned flags) {
    void* p = nullptr;
    if (hipError_t e = stub_alloc(&p, sizeof(unsigned))) return e;
    *(unsigned*)p = flags;
    *out = (hipEvent_t)p;
    return hipSuccess;
}
void pool_release_event(int device, hipEvent_t e, unsigned flags) {
    assert(e && device == 3 && *(unsigned*)e == flags);  // returned as taken
    stub_free(e);
}
}  // namespace rsv

using namespace rsv;

// a group sized together, like an engine's replay staging: two device arrays and two pinned copies
struct Group {
    DevBuf<uint32_t> perm;
    DevBuf<int64_t> h;
    HostBuf<int64_t> ph;
    HostBuf<uint8_t> flag;
    static constexpr int kMembers = 4;
    int64_t cap() const { return group_cap(perm, h, ph, flag); }
    hipError_t reserve(int64_t n) { return reserve_all(n, nullptr, perm, h, ph, flag); }
    template <typename F>
    void each(F&& f) const {
        f(perm.p, perm.cap), f(h.p, h.cap), f(ph.p, ph.cap), f(flag.p, flag.cap);
    }
};

#define CHECK(x)                                                        \
    do {                                                                \
        if (!(x)) {                                                     \
            fprintf(stderr, "%s:%d: failed: %s\n", __FILE__, __LINE__, #x); \
            return 1;                                                   \
        }                                                               \
    } while (0)

static int run() {
    {  // reserve below the capacity allocates nothing; release empties
        DevBuf<int64_t> a;
        HostBuf<int32_t> b;
        Scratch s;
        arm(0);
        CHECK(a.reserve(100, nullptr) == hipSuccess && a.cap == 100 && a.p);
        CHECK(b.reserve(100) == hipSuccess && b.cap == 100 && b.p);
        CHECK(s.reserve(4096, nullptr) == hipSuccess && s.bytes() == 4096);
        const long n0 = g_allocs;
        int64_t* pa = a.p;
        CHECK(a.reserve(100, nullptr) == hipSuccess && a.reserve(7, nullptr) == hipSuccess);
        CHECK(b.reserve(99) == hipSuccess && s.reserve(100, nullptr) == hipSuccess);
        CHECK(g_allocs == n0 && a.p == pa && a.cap == 100 && s.bytes() == 4096);
        CHECK(s.reserve(8192, nullptr) == hipSuccess && s.bytes() == 8192);  // the largest asked so far
        a.release();
        CHECK(!a.p && a.cap == 0 && g_live.size() == 2);
    }
    CHECK(g_live.empty());
    {  // reserve_keep: the first `used` entries survive two growths, device and host
        DevBuf<int64_t> a;
        HostBuf<int64_t> b;
        CHECK(a.reserve(8, nullptr) == hipSuccess && b.reserve(8) == hipSuccess);
        for (int i = 0; i < 8; ++i) a.p[i] = 100 + i, b.p[i] = 200 + i;
        CHECK(a.reserve_keep(64, 8, nullptr) == hipSuccess && b.reserve_keep(64, 8) == hipSuccess);
        for (int i = 8; i < 64; ++i) a.p[i] = 100 + i, b.p[i] = 200 + i;
        CHECK(a.reserve_keep(1000, 64, nullptr) == hipSuccess && b.reserve_keep(1000, 64) == hipSuccess);
        CHECK(a.cap == 1000 && b.cap == 1000);
        for (int i = 0; i < 64; ++i) CHECK(a.p[i] == 100 + i && b.p[i] == 200 + i);
        a.p[999] = b.p[999] = 1;  // the whole new block is there (checked by the sanitizer)
    }
    CHECK(g_live.empty());
    // A grouped reserve with its N-th allocation failing, for every N: each member is as before or empty with
    // capacity 0, the group's capacity is above no member's, and a later reserve of a SMALLER size than the
    // failed one allocates again exactly where a member is short of it.
    for (long n = 1; n <= Group::kMembers; ++n) {
        Group g;
        CHECK(g.reserve(16) == hipSuccess && g.cap() == 16);
        void* before[Group::kMembers];
        int i = 0;
        g.each([&](const void* p, int64_t) { before[i++] = (void*)p; });
        arm(n);
        CHECK(g.reserve(1000) == hipErrorOutOfMemory);
        i = 0;
        int short_of_500 = 0;
        bool ok = true;
        g.each([&](const void* p, int64_t cap) {
            const bool unchanged = p == before[i] && cap == 16, empty = !p && cap == 0, grown = p && cap == 1000;
            ok = ok && (unchanged || empty || grown) && g.cap() <= cap;
            short_of_500 += cap < 500;
            ++i;
        });
        CHECK(ok && g.cap() < 1000 && short_of_500 == Group::kMembers - (n - 1));
        arm(0);
        CHECK(g.reserve(500) == hipSuccess && g_allocs == short_of_500 && g.cap() >= 500);
        g.each([&](const void* p, int64_t cap) { ok = ok && p && cap >= 500; });
        CHECK(ok);
    }
    CHECK(g_live.empty());
    {  // a failed first allocation leaves an empty buffer; the mapped block carries its alias
        DevBuf<int32_t> a;
        HostBuf<int32_t> b;
        MappedBuf<int64_t> m;
        arm(1);
        CHECK(a.reserve(10, nullptr) == hipErrorOutOfMemory && !a.p && a.cap == 0);
        arm(1);
        CHECK(b.reserve(10) == hipErrorOutOfMemory && !b.p && b.cap == 0);
        arm(1);
        CHECK(m.reserve(16) == hipErrorOutOfMemory && !m.p && !m.dev && m.cap == 0);
        arm(0);
        CHECK(m.reserve(16) == hipSuccess && m.p && m.dev == m.p && m.cap == 16);
    }
    CHECK(g_live.empty());
    {  // move and swap transfer ownership
        DevBuf<int64_t> a, b;
        CHECK(a.reserve(10, nullptr) == hipSuccess && b.reserve(20, nullptr) == hipSuccess);
        int64_t *pa = a.p, *pb = b.p;
        a.swap(b);
        CHECK(a.p == pb && a.cap == 20 && b.p == pa && b.cap == 10);
        std::swap(a, b);
        CHECK(a.p == pa && a.cap == 10 && b.p == pb && b.cap == 20);
        DevBuf<int64_t> c(std::move(a));
        CHECK(c.p == pa && c.cap == 10 && !a.p && a.cap == 0 && g_live.size() == 2);
        b = std::move(c);  // b's own block goes back to the pool
        CHECK(b.p == pa && b.cap == 10 && !c.p && g_live.size() == 1 && g_live.count(pa));
        HostBuf<int32_t> h1, h2;
        CHECK(h1.reserve(4) == hipSuccess);
        int32_t* ph = h1.p;
        h2 = std::move(h1);
        CHECK(h2.p == ph && !h1.p && h1.cap == 0);
        MappedBuf<int64_t> m1, m2;
        CHECK(m1.reserve(16) == hipSuccess);
        m2.swap(m1);
        CHECK(m2.p && m2.dev == m2.p && !m1.p && !m1.dev);
        int64_t* gone = m2.detach();  // the block leaves its owner, who frees it through the pool
        CHECK(gone && !m2.p && !m2.dev && m2.cap == 0 && g_live.count(gone));
        pool_host_free(gone);
    }
    CHECK(g_live.empty());
    // The landing zone takes each form once, from a byte size and the caller's "may publish"; with its only
    // allocation failing it stays empty -- no form, no alias -- and the next ensure chooses again.
    for (int may = 0; may < 2; ++may) {
        Landing z;
        z.gen = 7;
        arm(1);
        CHECK(z.ensure(1000, may) == hipErrorOutOfMemory);
        CHECK(!z.host() && !z.dev() && !z.published() && !z.pub.p && !z.pin.p && z.gen == 7 && g_live.empty());
        arm(0);
        CHECK(z.ensure(1000, may) == hipSuccess && z.host() && z.published() == (may == 1) && g_live.size() == 1);
        void* h = z.host();
        if (may) {  // the flag line lies behind the entries on a 64-byte boundary, inside the block, and starts at gen
            CHECK(z.dev() == h && (uint8_t*)z.flag() == (uint8_t*)h + 1024 && z.flag_dev() == z.flag());
            CHECK(z.pub.cap == 1024 + 64 && *z.flag() == 7);
            z.flag()[15] = 1;  // the whole line is there (checked by the sanitizer)
        } else {
            CHECK(!z.dev() && z.pin.cap == 1000);
            ((uint8_t*)h)[999] = 1;
        }
        CHECK(z.next_gen() == 8 && z.gen == 8);
        CHECK(z.ensure(1000, !may) == hipSuccess && z.host() == h && z.published() == (may == 1));  // chosen once
        CHECK(g_allocs == 1);
        if (may) {  // given away, it holds nothing: the taker frees the block, the generation stays
            void* gone = z.give();
            CHECK(gone == h && !z.host() && !z.dev() && !z.published() && z.pub.cap == 0 && z.gen == 8);
            CHECK(g_live.size() == 1 && g_live.count(gone));
            pool_host_free(gone);
        }
    }
    CHECK(g_live.empty());
    {  // the event owner: taken at first use, returned exactly once with its device and flags, moves included
        PoolEvent a, never;
        arm(1);
        CHECK(a.ensure(3, 2) == hipErrorOutOfMemory && !a.e && g_live.empty());
        arm(0);
        CHECK(a.ensure(3, 2) == hipSuccess && a.e && g_live.size() == 1);
        hipEvent_t e = a;
        CHECK(a.ensure(3, 2) == hipSuccess && a.e == e && g_allocs == 1);
        PoolEvent b(std::move(a));
        CHECK(!a.e && b.e == e && b.device == 3 && b.flags == 2);
        PoolEvent c;
        CHECK(c.ensure(3, 0) == hipSuccess && g_live.size() == 2);
        c = std::move(b);  // c's own event goes back to the pool
        CHECK(c.e == e && !b.e && c.flags == 2 && g_live.size() == 1);
        c.release();
        CHECK(!c.e && g_live.empty());
        c.release();
        CHECK(c.ensure(3, 2) == hipSuccess);  // and can be taken again; returned by the destructor
    }
    CHECK(g_live.empty());
    {  // the work clock, as rules
        WorkClock c;
        CHECK(c.idle() && !c.holds() && !c.current());
        c.group();
        CHECK(!c.idle());
        c.drained();  // (1) drained after a drain ...
        CHECK(c.idle());
        c.group();
        c.published(true, 5);
        CHECK(c.holds() && c.current() && c.pub_gen == 5 && !c.idle());
        c.seen(c.pub_ops, 4, 5);  // ... not when the host saw an older generation than the newest issued,
        CHECK(!c.idle());
        c.seen(c.pub_ops, 5, 5);  // ... and when it saw the generation of a publication that was the last group
        CHECK(c.idle());
        c.group();  // (2) the next group: the publication still has the slots, is no longer current,
        CHECK(c.holds() && !c.current() && !c.idle());
        c.seen(c.pub_ops, 5, 5);  // and seeing it again drains nothing
        CHECK(!c.idle());
        c.published(true, 6);
        CHECK(c.current());
        c.invalidate();  // (2) ... or an invalidation
        CHECK(!c.holds() && !c.current() && c.pub_gen == 6);
        c.published(true, 7);
        c.published(false, 9);  // (3) recording "no publication" invalidates and records nothing
        CHECK(!c.holds() && !c.current() && c.pub_gen == 7);
        c.seen(c.ops, 9, 9);  // a landing zone of its own (the index-only offsets), published by the last group
        CHECK(c.idle());
    }
    return 0;
}

int main() {
    if (run()) return 1;
    printf("ok buffers: every block returned to the pool\n");
    return 0;
}
