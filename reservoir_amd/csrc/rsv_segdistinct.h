// rsv_segdistinct.h -- what the K5 kernels share: the stateless rsv_distinct_segmented
// (rsv_segdistinct.hip) and the resumable update / merge (rsv_segdistinct_state.hip).
// The LDS entry, the per-stream java.util.Random seeding and the team's sort + dedup + trim.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace rsv {
namespace segd {

constexpr int kU = 4;  // elements per lane and iteration
constexpr int64_t kMaxI64 = INT64_MAX;

// java.util.Random(seed): the first two nextLong() (RandomValues r0, r1, Sampler.scala:385-388)
__device__ __forceinline__ void java_r0r1(uint64_t seed, int64_t& r0, int64_t& r1) {
    constexpr uint64_t kMul = 0x5DEECE66DULL, kMask = (1ULL << 48) - 1;
    uint64_t st = (seed ^ kMul) & kMask;
    int64_t w[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        st = (st * kMul + 0xBULL) & kMask;
        w[i] = (int64_t)(int32_t)(uint32_t)(st >> 16);
    }
    r0 = (int64_t)(((uint64_t)w[0] << 32) + (uint64_t)w[1]);
    r1 = (int64_t)(((uint64_t)w[2] << 32) + (uint64_t)w[3]);
}

// one LDS entry: 16 bytes, moved with one ds_read_b128 / ds_write_b128
struct alignas(16) Ent {
    int64_t h, key;
};

__device__ __forceinline__ bool ent_less(const Ent& a, const Ent& b) { return a.h < b.h || (a.h == b.h && a.key < b.key); }
__device__ __forceinline__ bool ent_eq(const Ent& a, const Ent& b) { return a.h == b.h && a.key == b.key; }

// Sort + dedup + trim of the team's first n entries; returns the new set size min(k, distinct).
template <int NT>
__device__ __forceinline__ uint32_t merge_set(Ent* __restrict__ se, uint32_t n, uint32_t k, uint32_t* __restrict__ s_scan) {
    const uint32_t tid = threadIdx.x;
    if (n == 0) return 0;
    uint32_t sz2 = 2;
    while (sz2 < n) sz2 <<= 1;
    for (uint32_t i = n + tid; i < sz2; i += NT) se[i] = Ent{kMaxI64, kMaxI64};
    __syncthreads();
    for (uint32_t sz = 2; sz <= sz2; sz <<= 1) {
        for (uint32_t j = sz >> 1; j > 0; j >>= 1) {
            for (uint32_t t = tid; t < (sz2 >> 1); t += NT) {
                const uint32_t l = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                const bool asc = (l & sz) == 0;
                const Ent a = se[l], b = se[l + j];
                if (ent_less(b, a) == asc && !ent_eq(a, b)) {
                    se[l] = b;
                    se[l + j] = a;
                }
            }
            __syncthreads();
        }
    }
    // in-place compaction of the first occurrences, NT entries per round.  An entry moves to a
    // position <= its own, and entry base - 1 is only ever overwritten by itself, so the next
    // round's look-behind reads what the sort left.
    constexpr uint32_t kWavesT = NT / 64;
    uint32_t run = 0;
    for (uint32_t base = 0; base < n && run < k; base += NT) {
        const uint32_t i = base + tid;
        Ent e{0, 0};
        bool first = false;
        if (i < n) {
            e = se[i];
            first = i == 0 || !ent_eq(e, se[i - 1]);
        }
        const uint64_t mask = __ballot(first);
        uint32_t pre = (uint32_t)__popcll(mask & ((1ULL << (tid & 63)) - 1));
        uint32_t total = (uint32_t)__popcll(mask);
        if constexpr (kWavesT > 1) {
            if ((tid & 63) == 0) s_scan[tid >> 6] = total;
            __syncthreads();  // also: every read of this round is done
            uint32_t before = 0;
            total = 0;
            for (uint32_t w = 0; w < kWavesT; ++w) {
                const uint32_t c = s_scan[w];
                if (w < (tid >> 6)) before += c;
                total += c;
            }
            pre += before;
        } else {
            __syncthreads();
        }
        const uint32_t pos = run + pre;
        if (first && pos < k) se[pos] = e;
        run += total;
        __syncthreads();
    }
    return run < k ? run : k;
}

}  // namespace segd
}  // namespace rsv
