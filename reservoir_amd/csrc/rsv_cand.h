// rsv_cand.h -- the candidate queues of the distinct engines' filter passes, side by side: each wave
// stages its candidates in LDS and appends them a batch at a time under one reservation atomic.
// OffsetQueue carries (h, batch offset) (rsv_wide.hip, rsv_objects.hip), CandOut (h, key[, index])
// (rsv_distinct.hip's K3).  Device-only; each kernel declares the __shared__ arrays and hands them in.
#pragma once
#include "rsv_device.h"

namespace rsv {

typedef long long i64x2 __attribute__((ext_vector_type(2)));

// Candidate output of a hash filter: each wave stages (h, offset) in LDS and appends B at a time under
// one reservation atomic (the counter is a single contended word); the workgroup's leftovers go out
// under one atomic at the end.  Places at or past the room `cap` (>= 0) are counted, not written.
template <int WAVES>
struct OffsetQueue {
    static constexpr uint32_t B = 128;
    static constexpr uint32_t Q = B + 64;
    int64_t* qh;  // LDS: Q hashes of this wave
    int64_t* qi;  // LDS: Q offsets
    uint32_t qn;  // wave-uniform fill
    int64_t* cand_h;
    int64_t* cand_i;
    unsigned long long* counter;
    int64_t cap;

    __device__ __forceinline__ void write_at(unsigned long long base, uint32_t from, uint32_t cnt) {
        const uint32_t lane = threadIdx.x & 63;
        for (uint32_t j = lane; j < cnt; j += 64) {
            const unsigned long long pos = base + j;
            if ((int64_t)pos < cap) {
                cand_h[pos] = qh[from + j];
                cand_i[pos] = qi[from + j];
            }
        }
    }
    __device__ __forceinline__ void push(bool c, int64_t h, int64_t idx) {
        const unsigned long long bal = __ballot(c);
        if (bal == 0) return;
        if (c) {
            const uint32_t pos = qn + __popcll(bal & lanemask_lt64());
            qh[pos] = h;
            qi[pos] = idx;
        }
        qn += (uint32_t)__popcll(bal);
        if (qn >= B) {
            qn -= B;
            __builtin_amdgcn_wave_barrier();
            unsigned long long base = 0;
            if ((threadIdx.x & 63) == 0) base = atomicAdd(counter, (unsigned long long)B);
            base = __shfl(base, 0);
            write_at(base, qn, B);
            __builtin_amdgcn_wave_barrier();
        }
    }
    __device__ __forceinline__ void flush_block(uint32_t* s_q, unsigned long long* s_base) {
        const uint32_t w = threadIdx.x >> 6;
        __builtin_amdgcn_wave_barrier();
        if ((threadIdx.x & 63) == 0) s_q[w] = qn;
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t tot = 0;
            for (int i = 0; i < WAVES; ++i) tot += s_q[i];
            *s_base = tot ? atomicAdd(counter, (unsigned long long)tot) : 0ull;
        }
        __syncthreads();
        uint32_t pre = 0;
        for (uint32_t i = 0; i < w; ++i) pre += s_q[i];
        if (qn) write_at(*s_base + pre, 0, qn);
        qn = 0;
    }
};

// K3's candidate output (rsv_distinct.hip): the same staging for (h, key) pairs of Int / Long keys,
// written B at a time so the global reservation counter sees one atomic per B candidates (a single
// contended word sustains ~88 atomics/us: one atomic per candidate cost 1.5 ms at 132k candidates).
// IDX: each candidate also carries its pass-relative index (the ordered mode's arrival order); its
// chunks run at ~3k candidates per pass, so it stages B = 256 (64: ~35 us of atomics per short chunk).
template <typename KeyT, bool IDX = false>
struct CandOut {
    static constexpr uint32_t B = IDX ? 256 : 64;  // batch; the LDS queue holds B + 64
    int64_t* qh;  // LDS: B + 64 hashes of this wave
    KeyT* qk;     // LDS: B + 64 keys
    uint32_t qn;  // wave-uniform fill
    int64_t* cand_h;
    KeyT* cand_k;
    unsigned long long* counter;
    int64_t cap;
    uint32_t* qi = nullptr;      // LDS: B + 64 indices (IDX)
    uint32_t* cand_i = nullptr;  // (IDX)

    __device__ __forceinline__ void write_at(unsigned long long base, uint32_t from, uint32_t cnt) {
        const uint32_t lane = threadIdx.x & 63;
#pragma unroll
        for (uint32_t j0 = 0; j0 < B; j0 += 64) {
            const uint32_t j = j0 + lane;
            if (j < cnt) {
                const unsigned long long pos = base + j;
                if ((int64_t)pos < cap) {
                    cand_h[pos] = qh[from + j];
                    cand_k[pos] = qk[from + j];
                    if constexpr (IDX) cand_i[pos] = qi[from + j];
                }
            }
        }
    }
    __device__ __forceinline__ void push(bool c, int64_t h, KeyT key, uint32_t idx) {
        const unsigned long long bal = __ballot(c);
        if (bal == 0) return;
        if (c) {
            const uint32_t pos = qn + __popcll(bal & lanemask_lt64());
            qh[pos] = h;
            qk[pos] = key;
            if constexpr (IDX) qi[pos] = idx;
        }
        qn += (uint32_t)__popcll(bal);
        if (qn >= B) {
            qn -= B;
            __builtin_amdgcn_wave_barrier();
            unsigned long long base = 0;
            if ((threadIdx.x & 63) == 0) base = atomicAdd(counter, (unsigned long long)B);
            base = __shfl(base, 0);
            write_at(base, qn, B);
            __builtin_amdgcn_wave_barrier();
        }
    }
    // the final flush of every wave of the workgroup under ONE reservation atomic: the counter is
    // a single contended word (~88 atomics/us), and a pass whose waves each end with a few staged
    // candidates (the ordered mode's short chunks) was bound by one atomic per wave
    template <int WAVES>
    __device__ __forceinline__ void flush_block(uint32_t* s_q, unsigned long long* s_base) {
        const uint32_t w = threadIdx.x >> 6;
        if ((threadIdx.x & 63) == 0) s_q[w] = qn;
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t tot = 0;
#pragma unroll
            for (int i = 0; i < WAVES; ++i) tot += s_q[i];
            *s_base = tot ? atomicAdd(counter, (unsigned long long)tot) : 0ull;
        }
        __syncthreads();
        uint32_t pre = 0;
        for (uint32_t i = 0; i < w; ++i) pre += s_q[i];
        if (qn) write_at(*s_base + pre, 0, qn);
        qn = 0;
    }
};

}  // namespace rsv
