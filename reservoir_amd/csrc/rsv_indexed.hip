// rsv_indexed.hip -- the keyless K2 kernels: Sampler.apply over S streams whose elements never reach the device.
// Launched by rsv_segmented.hip (launch_segmented_indexed*); declared in rsv_k2_indexed.h, which says why they
// are compiled apart from the keyed kernels.
//
#include "rsv_k2.h"
#include "rsv_k2_indexed.h"

namespace rsv {
namespace k2 {

// rsv_sample_segmented_indexed / _update / _merge.  The element loops of rsv_k2.h in their RES mode decide every
// winner without a key; these kernels stop there and publish indices: the stateless form each slot's
// stream-relative source (slot_source with off = 0), the update each replaced slot's position inside its
// segment (hits), the merge the part each slot came from (src).  The host keeps the elements.
//
// The split form (stateless only): without keys a launch is pure Philox work and a stream can be far longer
// than any tensor, so one wave (workgroup) per stream would leave the device idle beside a long one.  A
// stream longer than C indices (C a multiple of 1024: a piece starts on an iteration boundary of the element
// loops) is taken as pieces [pC, min(len, (p+1)C)).  The first kernel does every stream's piece 0 and stores
// the whole row -- -1 where piece 0 has neither a writer nor the fill index -- and records (stream, len) in a
// bounded device list, one atomic per long stream; a stream the list has no room for is done whole.  The
// second kernel, after it on the same HIP stream, walks the list: every wave (workgroup) strides over the
// remaining pieces of all entries, the start rotated by the pieces of the entries before, and folds each
// piece's table into the row with a 64-bit atomicMax.  Largest index per slot wins -- the update's rule, the
// fill rule included: a fill index belongs to the piece that contains it -- so the result does not depend on
// how the stream was cut.

// one thread per stream: true if (s, len) was recorded, so its caller does piece 0 only
__device__ __forceinline__ bool split_append(const SplitList& sl, int64_t s, int64_t len) {
    const unsigned long long e = atomicAdd(sl.count, 1ull);
    if (e >= sl.cap) return false;
    sl.ent[2 * e] = s;
    sl.ent[2 * e + 1] = len;
    return true;
}

// the list walk of the second kernel for worker w of nw: f(s, len, n0, nend) for each of its pieces
template <typename F>
__device__ __forceinline__ void split_pieces(const SplitList& sl, uint64_t n, uint32_t w, uint32_t nw, F f) {
    uint32_t acc = 0;  // pieces of the entries before, mod nw
    for (uint64_t e = 0; e < n; ++e) {
        const int64_t s = uniform64(sl.ent[2 * e]), len = uniform64(sl.ent[2 * e + 1]);
        const uint64_t rem = (uint64_t)(len - 1) / (uint64_t)sl.C;  // pieces after the first (len > C)
        for (uint64_t t = w >= acc ? w - acc : w + nw - acc; t < rem; t += nw) {
            const int64_t n0 = (int64_t)(t + 1) * sl.C;
            f(s, len, n0, std::min<int64_t>(len, n0 + sl.C));
        }
        acc = (uint32_t)((acc + rem) % nw);
    }
}

// slot j of a piece [n0, nend) into the stream's row: its winner w (0: none) or its fill index
__device__ __forceinline__ void piece_slot(int64_t* row, uint32_t j, uint64_t w, int64_t n0, int64_t nend) {
    int64_t at = (int64_t)w;
    if (!w) at = ((int64_t)j >= n0 && (int64_t)j < nend) ? (int64_t)j : -1;
    if (at >= 0) atomicMax((long long*)&row[j], (long long)at);
}

__global__ __launch_bounds__(64 * kWaves) void k2_indexed(const int64_t* __restrict__ offsets, int64_t S, uint32_t k,
                                                          uint32_t k0, uint32_t k1, uint64_t stream_base,
                                                          int64_t* __restrict__ out_idx, int64_t* __restrict__ counts,
                                                          uint32_t fifo_cap, SplitList sl) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    build_lut((uint16_t*)lds, 256ull * k);
    __syncthreads();
    const Wave W = wave_frame(lds, k, k0, k1, fifo_cap);
    const uint32_t lane = W.lane;
    const void* tab = W.tab;
    const int64_t wave_stride = (int64_t)gridDim.x * kWaves;
    for (int64_t s = (int64_t)blockIdx.x * kWaves + W.wave; s < S; s += wave_stride) {
        const int64_t len = std::max<int64_t>(uniform64(offsets[s + 1]) - uniform64(offsets[s]), 0);
        int64_t plen = len;  // piece 0
        if (sl.C > 0 && len > sl.C) {
            uint32_t rec = 0;
            if (lane == 0) rec = split_append(sl, s, len) ? 1u : 0u;
            if (__builtin_amdgcn_readfirstlane((int)rec)) plen = sl.C;
        }
        const uint64_t stream = stream_base + (uint64_t)s;
        const bool small = plen < kSmallLen;
        if (small) k2_stream<int64_t, true, false, true>(W, nullptr, 0, plen, stream, nullptr, 0);
        else k2_stream<int64_t, false, false, true>(W, nullptr, 0, plen, stream, nullptr, 0);
        int64_t* o = out_idx + s * (int64_t)k;
        for (uint32_t j = lane; j < k; j += 64)
            o[j] = slot_source(small ? (uint64_t)((const uint32_t*)tab)[j] : ((const uint64_t*)tab)[j], j, 0, plen);
        if (lane == 0) counts[s] = len < (int64_t)k ? len : (int64_t)k;
        __builtin_amdgcn_wave_barrier();  // the table is read before the next stream zeroes it
    }
}

// the second kernel of the split form, one wave per piece
__global__ __launch_bounds__(64 * kWaves) void k2_indexed_pieces(uint32_t k, uint32_t k0, uint32_t k1,
                                                                 uint64_t stream_base, int64_t* out_idx,
                                                                 uint32_t fifo_cap, SplitList sl) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const uint64_t n = std::min<uint64_t>(*sl.count, sl.cap);
    if (n == 0) return;  // (every thread of the grid: no stream was split)
    build_lut((uint16_t*)lds, 256ull * k);
    __syncthreads();
    const Wave W = wave_frame(lds, k, k0, k1, fifo_cap);
    const uint32_t lane = W.lane;
    const void* tab = W.tab;
    split_pieces(sl, n, blockIdx.x * kWaves + W.wave, gridDim.x * kWaves,
                 [&](int64_t s, int64_t, int64_t n0, int64_t nend) {
                     const uint64_t stream = stream_base + (uint64_t)s;
                     int64_t* o = out_idx + s * (int64_t)k;
                     if (nend < kSmallLen) {
                         k2_stream<int64_t, true, false, true>(W, nullptr, 0, nend - n0, stream, nullptr, n0);
                         for (uint32_t j = lane; j < k; j += 64) piece_slot(o, j, ((const uint32_t*)tab)[j], n0, nend);
                     } else {
                         k2_stream<int64_t, false, false, true>(W, nullptr, 0, nend - n0, stream, nullptr, n0);
                         for (uint32_t j = lane; j < k; j += 64) piece_slot(o, j, ((const uint64_t*)tab)[j], n0, nend);
                     }
                     __builtin_amdgcn_wave_barrier();  // the table is read before the next piece zeroes it
                 });
}

// stateless, one workgroup per stream (k >= kWGMinK), as k2_segmented_wg.  Only the LDS-table form splits: the
// answer of split_append reaches the workgroup through tab[0], before the table is zeroed.
template <typename TabT, bool GT>
__global__ __launch_bounds__(64 * kWavesWG) void k2_indexed_wg(const int64_t* __restrict__ offsets, int64_t S,
                                                               uint32_t k, uint32_t k0, uint32_t k1,
                                                               uint64_t stream_base, int64_t* __restrict__ out_idx,
                                                               int64_t* __restrict__ counts, uint32_t fifo_cap,
                                                               TabT* __restrict__ gtab, SplitList sl) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    build_lut((uint16_t*)lds, 256ull * k);
    const Wave W = wg_frame<GT>(lds, k, k0, k1, fifo_cap, gtab);
    TabT* tab = (TabT*)W.tab;
    const uint32_t nthr = 64u * kWavesWG;
    for (int64_t s = blockIdx.x; s < S; s += gridDim.x) {
        const int64_t len = std::max<int64_t>(uniform64(offsets[s + 1]) - uniform64(offsets[s]), 0);
        int64_t plen = len;  // piece 0
        if constexpr (!GT) {
            if (sl.C > 0 && len > sl.C) {
                if (threadIdx.x == 0) tab[0] = split_append(sl, s, len) ? 1 : 0;
                __syncthreads();
                if (tab[0]) plen = sl.C;
                plen = uniform64(plen);
                __syncthreads();  // every thread has read the answer before the table is zeroed
            }
            for (uint32_t j = threadIdx.x; j < k; j += nthr) tab[j] = 0;
        }
        __syncthreads();  // the table is zero (GT: the previous stream's gather left it so)
        const uint64_t stream = stream_base + (uint64_t)s;
        if (plen < kSmallLen) k2_part<TabT, true, GT, true>(W, tab, plen, stream, W.wave, 0);
        else k2_part<TabT, false, GT, true>(W, tab, plen, stream, W.wave, 0);
        if constexpr (GT) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");  // this wave's table atomics
        __syncthreads();
        if constexpr (GT) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");  // every wave's, before they are read
        int64_t* o = out_idx + s * (int64_t)k;
        for (uint32_t j = threadIdx.x; j < k; j += nthr) {
            TabT wi;
            if constexpr (GT) wi = __hip_atomic_exchange(&tab[j], (TabT)0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            else wi = tab[j];
            o[j] = slot_source(wi, j, 0, plen);
        }
        if (threadIdx.x == 0) counts[s] = len < (int64_t)k ? len : (int64_t)k;
        __syncthreads();  // the table has been read before the next stream writes it
    }
}

// the second kernel of the split form, one workgroup per piece (the table in LDS)
template <typename TabT>
__global__ __launch_bounds__(64 * kWavesWG) void k2_indexed_pieces_wg(uint32_t k, uint32_t k0, uint32_t k1,
                                                                      uint64_t stream_base, int64_t* out_idx,
                                                                      uint32_t fifo_cap, SplitList sl) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const uint64_t n = std::min<uint64_t>(*sl.count, sl.cap);
    if (n == 0) return;  // (every thread of the grid: no stream was split)
    build_lut((uint16_t*)lds, 256ull * k);
    const Wave W = wg_frame(lds, k, k0, k1, fifo_cap, (TabT*)nullptr);
    TabT* tab = (TabT*)W.tab;
    const uint32_t nthr = 64u * kWavesWG;
    split_pieces(sl, n, blockIdx.x, gridDim.x, [&](int64_t s, int64_t, int64_t n0, int64_t nend) {
        for (uint32_t j = threadIdx.x; j < k; j += nthr) tab[j] = 0;
        __syncthreads();  // the table is zero and the lut built
        const uint64_t stream = stream_base + (uint64_t)s;
        if (nend < kSmallLen) k2_part<TabT, true, false, true>(W, tab, nend - n0, stream, W.wave, n0);
        else k2_part<TabT, false, false, true>(W, tab, nend - n0, stream, W.wave, n0);
        __syncthreads();
        int64_t* o = out_idx + s * (int64_t)k;
        for (uint32_t j = threadIdx.x; j < k; j += nthr) piece_slot(o, j, tab[j], n0, nend);
        __syncthreads();  // the table has been read before the next piece zeroes it
    });
}

// resumed: the state is (idx, next).  update_slot_rows leaves 1 + the position inside the segment in the table
// entry of every slot the segment replaced (0: it stood), which is hits[j] + 1; hit_counts[b] counts them.  A
// skipped segment still gets its row of -1 and its count of 0: the host reads both without a mask.
__global__ __launch_bounds__(64 * kWaves) void k2_indexed_update(
    const int64_t* __restrict__ offsets, const int64_t* __restrict__ ids, const int64_t* __restrict__ bases, int64_t B,
    int64_t S, uint32_t k, uint32_t k0, uint32_t k1, uint64_t stream_base, int64_t* __restrict__ state_idx,
    int64_t* __restrict__ state_next, int64_t* __restrict__ hits, int64_t* __restrict__ hit_counts,
    uint32_t fifo_cap) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    build_lut((uint16_t*)lds, 256ull * k);
    __syncthreads();
    const Wave W = wave_frame(lds, k, k0, k1, fifo_cap);
    const uint32_t lane = W.lane;
    void* tab = W.tab;
    const int64_t wave_stride = (int64_t)gridDim.x * kWaves;
    for (int64_t b = (int64_t)blockIdx.x * kWaves + W.wave; b < B; b += wave_stride) {
        Segment g;
        int64_t* h = hits + b * (int64_t)k;
        if (!read_segment(g, offsets, ids, bases, state_next, b, S)) {
            for (uint32_t j = lane; j < k; j += 64) h[j] = -1;
            if (lane == 0) hit_counts[b] = 0;
            continue;
        }
        const uint64_t stream = stream_base + (uint64_t)g.r;
        int64_t* si = state_idx + g.r * (int64_t)k;
        const bool small = g.nend < kSmallLen;
        if (small) k2_stream<int64_t, true, false, true>(W, nullptr, 0, g.len, stream, nullptr, g.n0);
        else k2_stream<int64_t, false, false, true>(W, nullptr, 0, g.len, stream, nullptr, g.n0);
        uint32_t n = 0;
        for (uint32_t j0 = 0; j0 < k; j0 += 64) {  // (a wave-uniform trip count: the ballot counts the hits)
            const uint32_t j = j0 + lane;
            uint64_t e = 0;
            if (j < k) {
                if (small) {
                    update_slot_rows((uint32_t*)tab, g.n0, g.nend, j, si);
                    e = ((const uint32_t*)tab)[j];
                } else {
                    update_slot_rows((uint64_t*)tab, g.n0, g.nend, j, si);
                    e = ((const uint64_t*)tab)[j];
                }
                h[j] = (int64_t)e - 1;
            }
            n += (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(e != 0));
        }
        if (lane == 0) {
            hit_counts[b] = n;
            if (state_next[g.r] < g.nend) state_next[g.r] = g.nend;
        }
        __builtin_amdgcn_wave_barrier();  // the table is read before the next segment zeroes it
    }
}

// the workgroup form of k2_indexed_update (k >= kWGMinK), as k2_segmented_update_wg; the waves' hit counts meet
// in the first entries of the table once every slot's entry has been read
__global__ __launch_bounds__(64 * kWavesWG) void k2_indexed_update_wg(
    const int64_t* __restrict__ offsets, const int64_t* __restrict__ ids, const int64_t* __restrict__ bases, int64_t B,
    int64_t S, uint32_t k, uint32_t k0, uint32_t k1, uint64_t stream_base, int64_t* __restrict__ state_idx,
    int64_t* __restrict__ state_next, int64_t* __restrict__ hits, int64_t* __restrict__ hit_counts,
    uint32_t fifo_cap) {
    using TabT = unsigned long long;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    build_lut((uint16_t*)lds, 256ull * k);
    const Wave W = wg_frame(lds, k, k0, k1, fifo_cap);
    TabT* tab = (TabT*)W.tab;
    const uint32_t nthr = 64u * kWavesWG;
    for (int64_t b = blockIdx.x; b < B; b += gridDim.x) {
        Segment g;
        int64_t* h = hits + b * (int64_t)k;
        if (!read_segment(g, offsets, ids, bases, state_next, b, S)) {
            for (uint32_t j = threadIdx.x; j < k; j += nthr) h[j] = -1;
            if (threadIdx.x == 0) hit_counts[b] = 0;
            continue;
        }
        for (uint32_t j = threadIdx.x; j < k; j += nthr) tab[j] = 0;
        __syncthreads();  // the table is zero, the lut built, and n0 read by every wave
        const uint64_t stream = stream_base + (uint64_t)g.r;
        if (g.nend < kSmallLen) k2_part<TabT, true, false, true>(W, tab, g.len, stream, W.wave, g.n0);
        else k2_part<TabT, false, false, true>(W, tab, g.len, stream, W.wave, g.n0);
        __syncthreads();
        int64_t* si = state_idx + g.r * (int64_t)k;
        uint32_t mine = 0;
        for (uint32_t j = threadIdx.x; j < k; j += nthr) {
            update_slot_rows(tab, g.n0, g.nend, j, si);
            const TabT e = tab[j];
            h[j] = (int64_t)e - 1;
            mine += e != 0;
        }
        const uint32_t wave_hits = (uint32_t)__builtin_amdgcn_readlane((int)wave_incl_scan(mine), 63);
        __syncthreads();  // every entry has been read
        if (W.lane == 0) tab[W.wave] = wave_hits;
        __syncthreads();
        if (threadIdx.x == 0) {
            TabT n = 0;
            for (int w = 0; w < kWavesWG; ++w) n += tab[w];
            hit_counts[b] = (int64_t)n;
            if (state_next[g.r] < g.nend) state_next[g.r] = g.nend;
        }
        __syncthreads();  // the counts have been read before the next segment zeroes the table
    }
}

// rsv_sample_segmented_indexed_merge: merge_pick over idx and next alone; src[t] is the part entry t was
// taken from (the lowest of those that hold the largest index), -1 where the row's own entry stood
__global__ __launch_bounds__(256) void k2_indexed_merge(const int64_t* part_idx, const int64_t* part_next, int32_t P,
                                                        int64_t S, uint32_t k, int64_t* state_idx, int64_t* state_next,
                                                        int32_t* src) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= S * (int64_t)k) return;
    src[t] = merge_pick(part_idx, part_next, P, S, k, t, state_idx, state_next, [](int32_t) {});
}


// the instantiations rsv_segmented.hip launches
template __global__ void k2_indexed_wg<uint32_t, false>(const int64_t*, int64_t, uint32_t, uint32_t, uint32_t, uint64_t,
                                                        int64_t*, int64_t*, uint32_t, uint32_t*, SplitList);
template __global__ void k2_indexed_wg<uint32_t, true>(const int64_t*, int64_t, uint32_t, uint32_t, uint32_t, uint64_t,
                                                       int64_t*, int64_t*, uint32_t, uint32_t*, SplitList);
template __global__ void k2_indexed_wg<unsigned long long, false>(const int64_t*, int64_t, uint32_t, uint32_t, uint32_t,
                                                                  uint64_t, int64_t*, int64_t*, uint32_t,
                                                                  unsigned long long*, SplitList);
template __global__ void k2_indexed_wg<unsigned long long, true>(const int64_t*, int64_t, uint32_t, uint32_t, uint32_t,
                                                                 uint64_t, int64_t*, int64_t*, uint32_t,
                                                                 unsigned long long*, SplitList);
template __global__ void k2_indexed_pieces_wg<uint32_t>(uint32_t, uint32_t, uint32_t, uint64_t, int64_t*, uint32_t,
                                                        SplitList);
template __global__ void k2_indexed_pieces_wg<unsigned long long>(uint32_t, uint32_t, uint32_t, uint64_t, int64_t*,
                                                                  uint32_t, SplitList);

}  // namespace k2
}  // namespace rsv
