// rsv_objects.hip -- Sampler.distinct for ANY B (RandomValues, Sampler.scala:383-412): the candidate
// pass over the hashes alone.  The caller keeps the elements (a String, a case class, a tuple) and the
// reference's heap and Set[B]; the engine reads hash(map(x)), 8 B per element, and returns the few
// batch positions the reference could still admit.  The caller replays RandomValues over those only.
//
// The reference admits an element only if its scrambled hash h = byteswap64(r1 ^ byteswap64(r0 ^ hash))
// is below maxHash once the set is full (Sampler.scala:403).  The engine never sees a B, so it bounds
// maxHash from the hashes:
//   shadow   the <= k smallest DISTINCT hash values seen, ascending.  Equal elements have equal
//            hashes, so k distinct hash values mean >= k distinct elements: the reference's set is
//            full and its maxHash (the k-th smallest hash over distinct elements) is <= T, the
//            shadow's k-th value.  Any k distinct hashes that were seen give such a bound.
//   caller   after replaying a batch the caller reports its exact set size and maxHash
//            (rsv_candidates_commit); with size == k the next batch opens at min(T, maxHash).
// A batch runs as a chunk loop: chunk c is filtered (h < bound, strict, the bound read from device
// memory) against the bound left by chunk c - 1, its candidates are merged into the shadow, and the
// new bound is written where the next filter reads it -- no host round trip once a bound exists.
// Chunks then grow geometrically (each ~4 seen lengths long), so a chunk yields ~4k candidates and a
// batch ~k g log_{1+g}(n / k).  While no bound exists (the fill phase: fewer than k distinct hashes
// and no full caller set) every element is a candidate, chunks stay max(4k, 1024) long so that the
// sort area holds them, and the host reads the open flag back after each.
//   filter   obj_filter: one streaming pass, 16-B non-temporal loads, (h, batch offset) staged per
//            wave in LDS and appended under one reservation atomic per 128 candidates
//   shadow   obj_gather (shadow + the chunk's candidate hashes + padding into the sort area) ->
//            bitonic sort (obj_sort_tile / obj_sort_step) -> obj_compact (drop equal values, keep the
//            first k, write the bound)
//   order    the batch's candidates by offset (rocPRIM radix sort: arrival order, whatever order the
//            atomics ran in)
// The candidate room is a capacity sized from the expected count, not from n: writes past it are
// dropped and counted, and the host regrows the room and reruns the batch from the kept shadow.
// The shadow has two buffers: a batch works in the spare one, rsv_candidates_commit swaps them and
// rsv_candidates_abort leaves the committed one as it was.
//
// Known limit: every repeat of a current member has a hash under the bound, comes back as a
// candidate and is rejected by the caller's `contains`.  With fewer than k distinct hash values in a
// batch (and no caller bound) every element is a candidate: the cost is the reference's plus a copy.
#include <rocprim/device/device_radix_sort.hpp>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../include/reservoir_hip.h"
#include "rsv_cand.h"
#include "rsv_device.h"
#include "rsv_internal.h"

namespace rsv {

namespace {

constexpr int kOBlock = 256;
constexpr int kOU = 8;              // 16-B loads in flight per lane in the filter
constexpr int64_t kOGrid = 2048;    // filter workgroups at most (grid-stride beyond)
constexpr int kSortTile = 1024;     // elements one workgroup sorts in LDS
constexpr int kCompactBlock = 1024;
constexpr int64_t kGrow = 4;        // a chunk is ~kGrow seen lengths long
constexpr int64_t kPinned = 1 << 18;  // hashes per pinned staging buffer (host batches)

// device control words
enum : int {
    kCtlBound = 0,    // candidates: h < bound ...
    kCtlOpen = 1,     // ... or everything while nonzero (no bound known yet)
    kCtlM = 2,        // the working shadow's size
    kCtlCount = 3,    // candidates appended in this batch (dropped ones included)
    kCtlBegin = 4,    // the current chunk's first candidate
    kCtlSpill = 5,    // a chunk's candidates did not fit the sort area
    kCtlCallerBound = 6,
    kCtlCallerOpen = 7,
    kCtlWords = 8
};

using ObjQueue = OffsetQueue<kOBlock / 64>;

// The filter over n hashes (a chunk of the batch starting at batch offset `base`): 16-B non-temporal
// loads (two hashes each), kOU in flight per lane; the <= 1 head element before the first 16-B
// boundary and the odd tail go through the scalar loops.  Loop bounds are wave-uniform (tile
// starts), so the ballots see every lane.  The bound comes from ctl, where the previous chunk's
// shadow update left it.
__global__ __launch_bounds__(kOBlock) void obj_filter(const int64_t* __restrict__ hashes, int64_t n, int64_t base,
                                                      int64_t r0, int64_t r1, int64_t* __restrict__ ctl,
                                                      int64_t* __restrict__ cand_h, int64_t* __restrict__ cand_i,
                                                      int64_t cap) {
    __shared__ int64_t sh_h[kOBlock / 64][ObjQueue::Q];
    __shared__ int64_t sh_i[kOBlock / 64][ObjQueue::Q];
    __shared__ uint32_t s_q[kOBlock / 64];
    __shared__ unsigned long long s_base;
    ObjQueue out{sh_h[threadIdx.x >> 6], sh_i[threadIdx.x >> 6], 0u, cand_h, cand_i,
                 (unsigned long long*)(ctl + kCtlCount), cap};
    const int64_t bound = ctl[kCtlBound];
    const bool open = ctl[kCtlOpen] != 0;
    const int64_t T = (int64_t)gridDim.x * blockDim.x;
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t head = std::min<int64_t>(n, (int64_t)(((16u - ((uintptr_t)hashes & 15u)) & 15u) / 8u));
    const i64x2* hv = reinterpret_cast<const i64x2*>(hashes + head);
    const int64_t n_vec = (n - head) / 2;
    for (int64_t t0 = 0; t0 < n_vec; t0 += T * kOU) {
        i64x2 x[kOU];
#pragma unroll
        for (int u = 0; u < kOU; ++u) {
            const int64_t v = t0 + u * T + tid;
            x[u] = __builtin_nontemporal_load(hv + (v < n_vec ? v : n_vec - 1));
        }
        int64_t h[kOU][2];
        bool c[kOU][2];
        bool any = false;
#pragma unroll
        for (int u = 0; u < kOU; ++u) {
            const bool ok = t0 + u * T + tid < n_vec;
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                h[u][e] = scramble(r0, r1, x[u][e]);
                c[u][e] = ok && (open || h[u][e] < bound);
                any |= c[u][e];
            }
        }
        if (__any(any)) {
#pragma unroll
            for (int u = 0; u < kOU; ++u)
#pragma unroll
                for (int e = 0; e < 2; ++e) out.push(c[u][e], h[u][e], base + head + (t0 + u * T + tid) * 2 + e);
        }
    }
    for (int64_t i0 = 0; i0 < head; i0 += T) {
        const int64_t i = i0 + tid;
        const int64_t hh = i < head ? scramble(r0, r1, hashes[i]) : 0;
        out.push(i < head && (open || hh < bound), hh, base + i);
    }
    for (int64_t i0 = head + 2 * n_vec; i0 < n; i0 += T) {
        const int64_t i = i0 + tid;
        const int64_t hh = i < n ? scramble(r0, r1, hashes[i]) : 0;
        out.push(i < n && (open || hh < bound), hh, base + i);
    }
    out.flush_block(s_q, &s_base);
}

// a batch starts: the committed shadow's size and bound, the caller's bound, no candidates
__global__ void obj_begin(int64_t* __restrict__ ctl, int64_t m, int64_t open, int64_t bound, int64_t caller_open,
                          int64_t caller_bound) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    ctl[kCtlBound] = bound;
    ctl[kCtlOpen] = open;
    ctl[kCtlM] = m;
    ctl[kCtlCount] = 0;
    ctl[kCtlBegin] = 0;
    ctl[kCtlSpill] = 0;
    ctl[kCtlCallerBound] = caller_bound;
    ctl[kCtlCallerOpen] = caller_open;
}

// the entries a chunk's shadow update sorts: the shadow's m values, then the chunk's candidate
// hashes (as many as the area of S entries holds; more raise the spill flag), the rest padding
__device__ __forceinline__ int64_t chunk_cands(const int64_t* ctl, int64_t cap, int64_t S, int64_t* begin) {
    const int64_t m = ctl[kCtlM];
    const int64_t b = ctl[kCtlBegin];
    const int64_t e = std::min<int64_t>(ctl[kCtlCount], cap);
    *begin = b;
    return std::min<int64_t>(std::max<int64_t>(e - b, 0), S - m);
}

__global__ __launch_bounds__(kOBlock) void obj_gather(int64_t* __restrict__ ctl, const int64_t* __restrict__ shadow,
                                                      const int64_t* __restrict__ cand_h, int64_t cap,
                                                      int64_t* __restrict__ area, int64_t S) {
    const int64_t m = ctl[kCtlM];
    int64_t begin;
    const int64_t c = chunk_cands(ctl, cap, S, &begin);
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t == 0 && std::min<int64_t>(ctl[kCtlCount], cap) - begin > S - m) ctl[kCtlSpill] = 1;
    for (int64_t i = t; i < S; i += stride)
        area[i] = i < m ? shadow[i] : i < m + c ? cand_h[begin + (i - m)] : INT64_MAX;
}

// Bitonic sort of the area (S a power of two >= kSortTile), ascending.  obj_sort_tile runs every
// step whose partner distance is below the tile inside LDS: all steps of the sizes up to the tile
// (first = 1), or the tail steps of one larger size; obj_sort_step is one step across tiles.
__device__ __forceinline__ void cmpswap(int64_t& a, int64_t& b, bool asc) {
    if ((a > b) == asc) {
        const int64_t t = a;
        a = b;
        b = t;
    }
}

__global__ __launch_bounds__(kSortTile / 2) void obj_sort_tile(int64_t* __restrict__ area, int64_t size, int first) {
    __shared__ int64_t s[kSortTile];
    const int64_t base = (int64_t)blockIdx.x * kSortTile;
    const uint32_t t = threadIdx.x;
    s[t] = area[base + t];
    s[t + kSortTile / 2] = area[base + t + kSortTile / 2];
    __syncthreads();
    for (int64_t sz = first ? 2 : size; sz <= size; sz <<= 1) {
        for (uint32_t j = (uint32_t)std::min<int64_t>(sz >> 1, kSortTile / 2); j > 0; j >>= 1) {
            const uint32_t l = ((t & ~(j - 1)) << 1) | (t & (j - 1));
            const bool asc = ((base + l) & sz) == 0;
            int64_t a = s[l], b = s[l + j];
            cmpswap(a, b, asc);
            s[l] = a;
            s[l + j] = b;
            __syncthreads();
        }
    }
    area[base + t] = s[t];
    area[base + t + kSortTile / 2] = s[t + kSortTile / 2];
}

__global__ __launch_bounds__(kOBlock) void obj_sort_step(int64_t* __restrict__ area, int64_t S, int64_t size, int64_t j) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= S / 2) return;
    const int64_t l = ((t & ~(j - 1)) << 1) | (t & (j - 1));
    const bool asc = (l & size) == 0;
    int64_t a = area[l], b = area[l + j];
    if ((a > b) == asc) {
        area[l] = b;
        area[l + j] = a;
    }
}

// The sorted area's first k distinct values are the new shadow; with k of them the k-th is the
// shadow bound T.  One workgroup (the scan is sequential over tiles and stops at k values); it also
// leaves the next chunk's bound min(T, caller bound) and candidate start in ctl.
__global__ __launch_bounds__(kCompactBlock) void obj_compact(int64_t* __restrict__ ctl, const int64_t* __restrict__ area,
                                                             int64_t cap, int64_t S, int64_t* __restrict__ shadow,
                                                             int64_t k) {
    constexpr int E = 4;
    __shared__ uint32_t s_w[kCompactBlock / 64];
    __shared__ int64_t s_T;
    int64_t begin;
    const int64_t c = chunk_cands(ctl, cap, S, &begin);
    const int64_t total = ctl[kCtlM] + c;
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int64_t done = 0;  // distinct values written so far (uniform)
    for (int64_t i0 = 0; i0 < total && done < k; i0 += (int64_t)kCompactBlock * E) {
        int64_t v[E];
        bool f[E];
        uint32_t cnt = 0;
        const int64_t i = i0 + (int64_t)threadIdx.x * E;
        int64_t prev = i > 0 && i - 1 < total ? area[i - 1] : 0;
#pragma unroll
        for (int e = 0; e < E; ++e) {
            v[e] = i + e < total ? area[i + e] : 0;
            f[e] = i + e < total && (i + e == 0 || v[e] != prev);
            prev = v[e];
            cnt += f[e];
        }
        uint32_t inc = cnt;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t o = __shfl_up(inc, d);
            if (lane >= (uint32_t)d) inc += o;
        }
        if (lane == 63) s_w[w] = inc;
        __syncthreads();
        uint32_t pre = 0, all = 0;
        for (uint32_t q = 0; q < kCompactBlock / 64; ++q) {
            pre += q < w ? s_w[q] : 0;
            all += s_w[q];
        }
        int64_t pos = done + pre + inc - cnt;
#pragma unroll
        for (int e = 0; e < E; ++e) {
            if (f[e]) {
                if (pos < k) shadow[pos] = v[e];
                if (pos == k - 1) s_T = v[e];
                ++pos;
            }
        }
        done += all;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const bool full = done >= k;
        const bool copen = ctl[kCtlCallerOpen] != 0;
        const int64_t cb = ctl[kCtlCallerBound];
        ctl[kCtlM] = full ? k : done;
        ctl[kCtlOpen] = !full && copen;
        ctl[kCtlBound] = full ? (copen ? s_T : std::min<int64_t>(s_T, cb)) : cb;
        ctl[kCtlBegin] = std::min<int64_t>(ctl[kCtlCount], cap);
    }
}

#define OBJ_TRY(expr)                                      \
    do {                                                   \
        hipError_t _e = (expr);                            \
        if (_e != hipSuccess) return hip_status(_e, #expr);  \
    } while (0)

int64_t pow2_ceil(int64_t v) {
    int64_t p = kSortTile;
    while (p < v) p <<= 1;
    return p;
}

}  // namespace

struct ObjDistinct {
    int64_t k = 0;
    int64_t r0 = 0, r1 = 0;
    KernelTimer* timer = nullptr;
    // the shadow: sh[cur] is the committed one (c_m values, bound c_T when c_m == k)
    DevBuf<int64_t> sh[2];
    int cur = 0;
    int64_t c_m = 0, c_T = 0;
    // the caller's replica after the last committed batch
    bool caller_open = true;
    int64_t caller_bound = 0;
    // the pending batch
    bool ran = false;  // it ran chunks: sh[cur ^ 1] and p_m / p_T hold its shadow
    int64_t p_m = 0, p_T = 0;
    int64_t n_cand = 0;
    // the buffers (rsv_buffers.h)
    DevBuf<int64_t> ctl;
    HostBuf<int64_t> ctl_h;     // pinned copy of ctl
    DevBuf<int64_t> cand_h;     // the room: (h, offset) in the atomics' order
    DevBuf<int64_t> cand_i;
    DevBuf<int64_t> out_h;      // the same in offset order
    DevBuf<int64_t> out_i;
    int64_t room() const { return group_cap(cand_h, cand_i, out_h, out_i); }
    DevBuf<int64_t> area;       // sort area, area.cap entries
    Scratch temp;
    DevBuf<int64_t> hash_d;     // a host batch's hashes
    HostBuf<int64_t> pin[2];
    hipEvent_t pin_free[2] = {nullptr, nullptr};
    int64_t room_first = 0;  // RSV_OBJ_ROOM: the first batch's room (tests force an overflow with it)
};

namespace {

// The sort area holds the shadow (<= k) and one chunk's candidates: ~kGrow k expected (each seen
// length contributes ~k), room for >= 7k; the fill chunk (every element while no bound is known)
// fits as well.  A power of two for the bitonic sort: 8k when k is one.
int64_t first_chunk(const ObjDistinct* d) { return std::max<int64_t>(kGrow * d->k, 1024); }
int64_t area_size(const ObjDistinct* d) { return pow2_ceil(std::max<int64_t>(2 * kGrow * d->k, 2 * kSortTile)); }
int64_t chunk_room(const ObjDistinct* d) { return area_size(d) - d->k; }

// Chunk lengths: while no bound is known every element is a candidate, so a chunk is as long as
// the sort area surely holds (and the host reads the open flag back after it: the fill phase only);
// then each chunk is ~kGrow seen lengths long and the loop runs without a host round trip.
int64_t chunk_len(const ObjDistinct* d, bool open, int64_t seen, int64_t left) {
    return std::min<int64_t>(open ? first_chunk(d) : std::max<int64_t>(first_chunk(d), kGrow * seen), left);
}

// The old blocks go back to the pool before the new ones are taken (after one wait for the stream), so
// a retry with twice the room does not hold both.
int ensure_room(ObjDistinct* d, int64_t room, hipStream_t st) {
    if (room <= d->room()) return RSV_OK;
    OBJ_TRY(hipStreamSynchronize(st));
    d->cand_h.release(), d->cand_i.release(), d->out_h.release(), d->out_i.release();
    OBJ_TRY(reserve_all(room, st, d->cand_h, d->cand_i, d->out_h, d->out_i));
    return RSV_OK;
}

int ensure_area(ObjDistinct* d, int64_t S, hipStream_t st) {
    if (S <= d->area.cap) return RSV_OK;
    OBJ_TRY(hipStreamSynchronize(st));
    d->area.release();
    OBJ_TRY(d->area.reserve(S, st));
    return RSV_OK;
}

// the batch's chunk loop on the stream; ends with ctl in ctl_h
int run_chunks(ObjDistinct* d, const int64_t* hashes, int64_t n, int64_t seen, hipStream_t st) {
    const bool sh_open = d->c_m < d->k;
    bool open = sh_open && d->caller_open;
    const int64_t bound = sh_open ? d->caller_bound
                                  : d->caller_open ? d->c_T : std::min(d->c_T, d->caller_bound);
    hipLaunchKernelGGL(obj_begin, dim3(1), dim3(64), 0, st, d->ctl, d->c_m, (int64_t)open, bound,
                       (int64_t)d->caller_open, d->caller_bound);
    const int64_t S = d->area.cap;
    bool first = true;
    for (int64_t off = 0; off < n;) {
        const int64_t len = chunk_len(d, open, seen, n - off);
        const int64_t blocks =
            std::min<int64_t>(std::max<int64_t>((len / 2 + kOBlock * kOU - 1) / (kOBlock * kOU), 1), kOGrid);
        if (d->timer) d->timer->mark(st);
        hipLaunchKernelGGL(obj_filter, dim3((unsigned)blocks), dim3(kOBlock), 0, st, hashes + off, len, off, d->r0, d->r1,
                           d->ctl, d->cand_h, d->cand_i, d->room());
        if (d->timer) d->timer->mark(st);
        // shadow update: the committed shadow is read by the first chunk only
        const int64_t* src = first ? d->sh[d->cur] : d->sh[d->cur ^ 1];
        first = false;
        hipLaunchKernelGGL(obj_gather, dim3((unsigned)std::min<int64_t>((S + kOBlock - 1) / kOBlock, 4096)), dim3(kOBlock), 0,
                           st, d->ctl, src, d->cand_h, d->room(), d->area, S);
        hipLaunchKernelGGL(obj_sort_tile, dim3((unsigned)(S / kSortTile)), dim3(kSortTile / 2), 0, st, d->area,
                           (int64_t)kSortTile, 1);
        for (int64_t size = 2 * kSortTile; size <= S; size <<= 1) {
            for (int64_t j = size >> 1; j >= kSortTile; j >>= 1)
                hipLaunchKernelGGL(obj_sort_step, dim3((unsigned)(S / 2 / kOBlock)), dim3(kOBlock), 0, st, d->area, S,
                                   size, j);
            hipLaunchKernelGGL(obj_sort_tile, dim3((unsigned)(S / kSortTile)), dim3(kSortTile / 2), 0, st, d->area,
                               size, 0);
        }
        hipLaunchKernelGGL(obj_compact, dim3(1), dim3(kCompactBlock), 0, st, d->ctl, d->area, d->room(), S,
                           d->sh[d->cur ^ 1], d->k);
        OBJ_TRY(hipGetLastError());
        off += len;
        seen += len;
        if (open && off < n) {  // the fill phase: is there a bound yet, and is the room still enough
            OBJ_TRY(hipMemcpyAsync(d->ctl_h, d->ctl, kCtlWords * 8, hipMemcpyDeviceToHost, st));
            OBJ_TRY(hipStreamSynchronize(st));
            open = d->ctl_h[kCtlOpen] != 0;
            if (d->ctl_h[kCtlCount] > d->room()) return RSV_OK;
        }
    }
    OBJ_TRY(hipMemcpyAsync(d->ctl_h, d->ctl, kCtlWords * 8, hipMemcpyDeviceToHost, st));
    OBJ_TRY(hipStreamSynchronize(st));
    return RSV_OK;
}

}  // namespace

ObjDistinct* obj_create(int32_t k, int64_t r0, int64_t r1, int* status) {
    ObjDistinct* d = new ObjDistinct();
    d->k = k;
    d->r0 = r0;
    d->r1 = r1;
    if (const char* e = std::getenv("RSV_OBJ_ROOM")) d->room_first = std::max<int64_t>(std::atoll(e), 0);
    hipError_t e = d->ctl.reserve(kCtlWords, 0);
    if (e == hipSuccess) e = d->ctl_h.reserve(kCtlWords);
    for (int b = 0; b < 2 && e == hipSuccess; ++b) e = d->sh[b].reserve(k, 0);
    if (e != hipSuccess) {
        *status = hip_status(e, "allocating the hash shadow");
        obj_destroy(d);
        return nullptr;
    }
    *status = RSV_OK;
    return d;
}

void obj_destroy(ObjDistinct* d) {
    if (!d) return;
    // the caller has synchronized the stream: the buffers return their blocks
    for (hipEvent_t e : d->pin_free)
        if (e) (void)hipEventDestroy(e);
    delete d;
}

void obj_set_timer(ObjDistinct* d, KernelTimer* t) { d->timer = t; }

int obj_candidates(ObjDistinct* d, const int64_t* hashes, int64_t n, bool on_device, int64_t seen, hipStream_t st,
                   int64_t* n_cand) {
    d->ran = false;
    d->n_cand = 0;
    *n_cand = 0;
    if (n == 0) return RSV_OK;
    if (!on_device) {  // through the pinned staging pair into a device copy of the batch's hashes
        if (n > d->hash_d.cap) {
            OBJ_TRY(hipStreamSynchronize(st));
            d->hash_d.release();
            OBJ_TRY(d->hash_d.reserve(n, st));
        }
        for (int b = 0; b < 2; ++b)
            if (!d->pin[b]) {
                OBJ_TRY(d->pin[b].reserve(kPinned));
                OBJ_TRY(hipEventCreateWithFlags(&d->pin_free[b], hipEventDisableTiming));
            }
        int b = 0;
        for (int64_t off = 0; off < n; off += kPinned, b ^= 1) {
            const int64_t c = std::min(kPinned, n - off);
            if (off >= 2 * kPinned) OBJ_TRY(hipEventSynchronize(d->pin_free[b]));
            memcpy(d->pin[b], hashes + off, (size_t)c * 8);
            OBJ_TRY(hipMemcpyAsync(d->hash_d + off, d->pin[b], (size_t)c * 8, hipMemcpyHostToDevice, st));
            OBJ_TRY(hipEventRecord(d->pin_free[b], st));
        }
        hashes = d->hash_d;
    }
    // the room: the expected candidates of every chunk (twice over), the fill chunk whole
    const bool fill = d->c_m < d->k && d->caller_open;
    int64_t chunks = 0;  // (taking the fill phase for one chunk)
    for (int64_t off = 0, sn = seen; off < n; ++chunks) {
        const int64_t len = chunk_len(d, fill && off == 0, sn, n - off);
        off += len;
        sn += len;
    }
    int64_t room = std::min<int64_t>(n, chunks * chunk_room(d) + (fill ? first_chunk(d) : 0));
    if (d->room_first > 0) {
        room = std::min(room, d->room_first);
        d->room_first = 0;
    }
    int64_t S = area_size(d);
    for (;;) {
        if (int rc = ensure_room(d, room, st)) return rc;
        if (int rc = ensure_area(d, S, st)) return rc;
        if (int rc = run_chunks(d, hashes, n, seen, st)) return rc;
        const int64_t got = d->ctl_h[kCtlCount];
        if (got <= d->room() && !d->ctl_h[kCtlSpill]) break;
        // candidates were dropped (and counted): a larger room / sort area, and the batch again from
        // the committed shadow.  Still no bound at the end: every element is a candidate.
        if (d->ctl_h[kCtlSpill]) S = 2 * d->area.cap;
        if (got > d->room())
            room = d->ctl_h[kCtlOpen] ? n : std::min<int64_t>(n, std::max<int64_t>(2 * d->room(), chunks * chunk_room(d)));
    }
    d->ran = true;
    d->p_m = d->ctl_h[kCtlM];
    d->p_T = d->p_m == d->k ? d->ctl_h[kCtlBound] : 0;
    d->n_cand = d->ctl_h[kCtlCount];
    if (d->p_m == d->k && !d->caller_open) {
        // ctl's bound is min(T, caller bound): T itself is the shadow's last value
        OBJ_TRY(hipMemcpyAsync(d->ctl_h, d->sh[d->cur ^ 1] + (d->k - 1), 8, hipMemcpyDeviceToHost, st));
        OBJ_TRY(hipStreamSynchronize(st));
        d->p_T = d->ctl_h[0];
    }
    if (d->n_cand > 0) {  // arrival order
        int bits = 1;
        while (bits < 63 && (n >> bits) != 0) ++bits;
        size_t need = 0;
        OBJ_TRY(rocprim::radix_sort_pairs(nullptr, need, d->cand_i.p, d->out_i.p, d->cand_h.p, d->out_h.p,
                                          (size_t)d->n_cand, 0, (unsigned)bits, st));
        OBJ_TRY(d->temp.reserve(need, st));  // (a growth waits for the stream, idle here since run_chunks)
        OBJ_TRY(rocprim::radix_sort_pairs(d->temp.p(), need, d->cand_i.p, d->out_i.p, d->cand_h.p, d->out_h.p,
                                          (size_t)d->n_cand, 0, (unsigned)bits, st));
        OBJ_TRY(hipStreamSynchronize(st));
    }
    *n_cand = d->n_cand;
    return RSV_OK;
}

int obj_read(ObjDistinct* d, int64_t* offsets_host, int64_t* hashes_host, hipStream_t st) {
    if (d->n_cand == 0) return RSV_OK;
    OBJ_TRY(hipMemcpyAsync(offsets_host, d->out_i, (size_t)d->n_cand * 8, hipMemcpyDeviceToHost, st));
    OBJ_TRY(hipMemcpyAsync(hashes_host, d->out_h, (size_t)d->n_cand * 8, hipMemcpyDeviceToHost, st));
    OBJ_TRY(hipStreamSynchronize(st));
    return RSV_OK;
}

int64_t obj_pending_candidates(const ObjDistinct* d) { return d->n_cand; }

void obj_commit(ObjDistinct* d, int64_t set_size, int64_t max_hash) {
    if (d->ran) {
        d->cur ^= 1;
        d->c_m = d->p_m;
        d->c_T = d->p_T;
    }
    d->caller_open = set_size < d->k;
    d->caller_bound = d->caller_open ? 0 : max_hash;
    d->ran = false;
    d->n_cand = 0;
}

void obj_abort(ObjDistinct* d) {
    d->ran = false;
    d->n_cand = 0;
}

}  // namespace rsv
