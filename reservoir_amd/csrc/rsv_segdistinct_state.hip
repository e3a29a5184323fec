// rsv_segdistinct_state.hip -- K5 resumed: rsv_distinct_segmented_update / _merge.
// The state is the caller's: per row r counts[r] entries (h, key) ascending, in the layout
// rsv_distinct_segmented writes.  Bottom-k by (h, key) over distinct keys is a function of the key
// set alone, so bottomk(A u B) = bottomk(bottomk(A) u B): a row resumed from its stored set and fed
// the next piece ends where one stateless launch over the concatenation ends.
//
// The team, P, the LDS budget, the admission test and merge_set are K5's (rsv_segdistinct.hip,
// rsv_segdistinct.h).  What this kernel adds:
//   prologue   m0 = clamp(counts[r], 0, k); the row's pairs into se[0, m0) (coalesced global loads,
//              one 16-byte LDS write per entry); s_cnt = n_tot = m = m0; T = se[k-1] when m0 == k,
//              so a full row rejects from its first element on.
//   input      UPDATE: segment b = keys[offsets[b], offsets[b+1]) hashed and scrambled with the
//              row's (r0, r1), row r = stream_ids[b] (or b).  MERGE: for every part p the first
//              clamp(part_counts[p][r], 0, k) slots of its row r, h taken as stored.
//   epilogue   in place, behind the barrier after the last LDS read of the team; a row with no
//              input, and a row whose input admitted nothing, writes nothing (a full row in steady
//              state moves no state bytes out).
// Nothing read from the state or from the ids indexes memory unclamped: the count is clamped into
// [0, k], an id outside [0, num_states) skips the segment.
#include <algorithm>

#include "../../include/reservoir_hip.h"
#include "rsv_device.h"
#include "rsv_internal.h"
#include "rsv_segdistinct.h"

namespace rsv {

namespace {

using namespace segd;

// the team's registers across the pieces of one row (uniform over the team)
struct Team {
    uint32_t m;      // set size
    uint32_t n_tot;  // set + waiting candidates (= s_cnt, read between two barriers)
    int64_t Th, Tk;  // admission threshold: the k-th entry, or (max, max) below k entries
    bool dirty;      // something was appended since the prologue
};

// K5's element loop over one piece [lo, hi) of keys (and hashes).  SCRAMBLE: h = scramble(r0, r1,
// hash(key)); otherwise h = hashes[i] as stored.
template <typename KeyT, int NT, bool SCRAMBLE>
__device__ __forceinline__ void take_piece(Ent* __restrict__ se, uint32_t* __restrict__ s_cnt, uint32_t* __restrict__ s_scan,
                                           const KeyT* __restrict__ keys, const int64_t* __restrict__ hashes, int64_t lo,
                                           int64_t hi, uint32_t k, uint32_t P, int hash_kind, int64_t r0, int64_t r1,
                                           Team& t) {
    const uint32_t tid = threadIdx.x;
    constexpr int64_t kChunk = (int64_t)NT * kU;
    for (int64_t base = lo; base < hi; base += kChunk) {
        // the loads first: kU in flight per lane
        int64_t key[kU], hv[kU];
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            const int64_t i = base + (int64_t)u * NT + tid;
            key[u] = 0;
            hv[u] = 0;
            if (i < hi) {
                key[u] = (int64_t)keys[i];
                if (!SCRAMBLE || hash_kind == kHashPrecomputed) hv[u] = hashes[i];
            }
        }
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            const int64_t i = base + (int64_t)u * NT + tid;
            if (base + (int64_t)u * NT >= hi) break;  // uniform: the tail chunk's empty steps
            if (t.n_tot + NT > P || (t.m < k && t.n_tot >= 4 * k)) {
                t.m = merge_set<NT>(se, t.n_tot, k, s_scan);
                if (t.m == k) {
                    t.Th = se[k - 1].h;
                    t.Tk = se[k - 1].key;
                }
                __syncthreads();  // T is read before the appends below overwrite anything
                if (tid == 0) *s_cnt = t.m;
                t.n_tot = t.m;
                __syncthreads();
            }
            int64_t h;
            if constexpr (SCRAMBLE) {
                int64_t hashed;
                if (hash_kind == kHashPrecomputed)
                    hashed = hv[u];
                else if (hash_kind == kHashJavaLong)
                    hashed = hash_of<int64_t, kHashJavaLong>(key[u]);
                else if (hash_kind == kHashJavaInt)
                    hashed = hash_of<int64_t, kHashJavaInt>(key[u]);
                else
                    hashed = key[u];  // identity: the sign-extended key
                h = scramble(r0, r1, hashed);
            } else {
                h = hv[u];
            }
            const bool pass = i < hi && (h < t.Th || (h == t.Th && key[u] <= t.Tk));
            const uint64_t mask = __ballot(pass);
            if (mask) {
                uint32_t b = 0;
                if ((tid & 63) == (uint32_t)(__ffsll((long long)mask) - 1)) b = atomicAdd(s_cnt, (uint32_t)__popcll(mask));
                b = (uint32_t)__shfl((int)b, __ffsll((long long)mask) - 1);
                if (pass) se[b + (uint32_t)__popcll(mask & ((1ULL << (tid & 63)) - 1))] = Ent{h, key[u]};
            }
            // every wave reads the same count: no append of the next step runs before the
            // second barrier
            __syncthreads();
            const uint32_t c = *s_cnt;
            t.dirty |= c != t.n_tot;
            t.n_tot = c;
            __syncthreads();
        }
    }
}

// MERGE = false: in = the batch's keys / hashes / offsets, ids = stream ids or null, teams = segments.
// MERGE = true:  in = the parts' keys / hashes, part_counts, teams = num_states (row r = team index).
template <typename KeyT, int NT, bool MERGE>
__global__ __launch_bounds__(NT) void segstate_kernel(const KeyT* in_keys, const int64_t* in_hashes,
                                                      const int64_t* __restrict__ offsets,
                                                      const int64_t* __restrict__ ids, const int64_t* part_counts,
                                                      int64_t teams, int64_t num_states, int32_t parts, uint32_t k,
                                                      uint32_t P, int hash_kind, uint64_t seed0, KeyT* state_keys,
                                                      int64_t* state_hashes, int64_t* state_counts) {
    extern __shared__ __align__(16) unsigned char seg_lds[];
    Ent* const se = (Ent*)seg_lds;
    __shared__ uint32_t s_cnt;
    __shared__ uint32_t s_scan[NT / 64 > 1 ? NT / 64 : 1];
    const uint32_t tid = threadIdx.x;

    for (int64_t b = blockIdx.x; b < teams; b += gridDim.x) {
        // everything that decides the control flow below is uniform over the team
        int64_t r = b, lo = 0, hi = 0;
        if constexpr (!MERGE) {
            if (ids) r = ids[b];
            if (r < 0 || r >= num_states) continue;  // an id outside the state: no row is addressed
            lo = offsets[b];
            hi = offsets[b + 1];
            if (hi <= lo) continue;  // an empty segment leaves its row as it is
        }
        const int64_t ob = r * (int64_t)k;
        const int64_t c0 = state_counts[r];
        const uint32_t m0 = c0 <= 0 ? 0u : (c0 >= (int64_t)k ? k : (uint32_t)c0);
        __syncthreads();  // the previous row's output reads are done
        for (uint32_t i = tid; i < m0; i += NT) se[i] = Ent{state_hashes[ob + i], (int64_t)state_keys[ob + i]};
        if (tid == 0) s_cnt = m0;
        __syncthreads();
        Team t{m0, m0, kMaxI64, kMaxI64, false};
        if (m0 == k) {
            t.Th = se[k - 1].h;
            t.Tk = se[k - 1].key;
        }
        // (no barrier needed before the first append: it lands at se[m0] or behind, and a merge
        // has its own)
        if constexpr (MERGE) {
            for (int32_t p = 0; p < parts; ++p) {
                const int64_t row = (int64_t)p * num_states + r;
                const int64_t pc = part_counts[row];
                const int64_t n = pc <= 0 ? 0 : (pc >= (int64_t)k ? (int64_t)k : pc);
                const int64_t pb = row * (int64_t)k;
                take_piece<KeyT, NT, false>(se, &s_cnt, s_scan, in_keys, in_hashes, pb, pb + n, k, P, hash_kind, 0, 0, t);
            }
        } else {
            int64_t r0, r1;
            java_r0r1(seed0 + (uint64_t)r, r0, r1);
            take_piece<KeyT, NT, true>(se, &s_cnt, s_scan, in_keys, in_hashes, lo, hi, k, P, hash_kind, r0, r1, t);
        }
        if (!t.dirty) continue;  // nothing admitted: the row stands as it is
        if (t.n_tot != t.m) t.m = merge_set<NT>(se, t.n_tot, k, s_scan);
        __syncthreads();
        for (uint32_t i = tid; i < k; i += NT) {
            const Ent e = i < t.m ? se[i] : Ent{0, 0};
            state_keys[ob + i] = (KeyT)e.key;
            state_hashes[ob + i] = e.h;
        }
        if (tid == 0) state_counts[r] = t.m;
    }
}

// the teams the 256 CUs hold at once (LDS and 32 waves per CU), four times over: K5's grid
unsigned team_grid(int64_t teams, size_t lds, int nt) {
    const uint64_t per_cu = std::max<uint64_t>(1, std::min<uint64_t>((160 * 1024) / (lds + 256), 32 / (nt / 64)));
    return (unsigned)std::min<uint64_t>((uint64_t)teams, 256ull * per_cu * 4);
}

template <typename KeyT, int NT, bool MERGE>
hipError_t launch_form(const void* in_keys, const int64_t* in_hashes, const int64_t* offsets, const int64_t* ids,
                       const int64_t* part_counts, int64_t teams, int64_t num_states, int32_t parts, uint32_t k, uint32_t P,
                       int hash_kind, uint64_t seed0, void* state_keys, int64_t* state_hashes, int64_t* state_counts,
                       hipStream_t st) {
    const size_t lds = (size_t)P * 16;
    if (lds > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute((const void*)segstate_kernel<KeyT, NT, MERGE>,
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((segstate_kernel<KeyT, NT, MERGE>), dim3(team_grid(teams, lds, NT)), dim3(NT), lds, st,
                       (const KeyT*)in_keys, in_hashes, offsets, ids, part_counts, teams, num_states, parts, k, P,
                       hash_kind, seed0, (KeyT*)state_keys, state_hashes, state_counts);
    return hipGetLastError();
}

// K5's forms: the same NT and P per k (rsv_segdistinct.hip)
template <typename KeyT, bool MERGE>
hipError_t launch_keyed(const void* in_keys, const int64_t* in_hashes, const int64_t* offsets, const int64_t* ids,
                        const int64_t* part_counts, int64_t teams, int64_t num_states, int32_t parts, uint32_t k,
                        int hash_kind, uint64_t seed0, void* state_keys, int64_t* state_hashes, int64_t* state_counts,
                        hipStream_t st) {
    if (k <= kSegDistinctWaveMaxK)
        return launch_form<KeyT, 64, MERGE>(in_keys, in_hashes, offsets, ids, part_counts, teams, num_states, parts, k,
                                            k <= 64 ? 256 : 512, hash_kind, seed0, state_keys, state_hashes, state_counts,
                                            st);
    if (k <= 1024)
        return launch_form<KeyT, 256, MERGE>(in_keys, in_hashes, offsets, ids, part_counts, teams, num_states, parts, k,
                                             2048, hash_kind, seed0, state_keys, state_hashes, state_counts, st);
    return launch_form<KeyT, 1024, MERGE>(in_keys, in_hashes, offsets, ids, part_counts, teams, num_states, parts, k, 8192,
                                          hash_kind, seed0, state_keys, state_hashes, state_counts, st);
}

}  // namespace

hipError_t launch_segdistinct_update(const void* keys, int key_width, const int64_t* hashes, const int64_t* offsets,
                                     const int64_t* stream_ids, int64_t num_segments, int64_t num_states, uint32_t k,
                                     int hash_kind, uint64_t seed0, void* state_keys, int64_t* state_hashes,
                                     int64_t* state_counts, hipStream_t st) {
    if (num_segments <= 0 || num_states <= 0) return hipSuccess;
    if (key_width == 8)
        return launch_keyed<int64_t, false>(keys, hashes, offsets, stream_ids, nullptr, num_segments, num_states, 0, k,
                                            hash_kind, seed0, state_keys, state_hashes, state_counts, st);
    return launch_keyed<int32_t, false>(keys, hashes, offsets, stream_ids, nullptr, num_segments, num_states, 0, k,
                                        hash_kind, seed0, state_keys, state_hashes, state_counts, st);
}

hipError_t launch_segdistinct_merge(const void* part_keys, int key_width, const int64_t* part_hashes,
                                    const int64_t* part_counts, int32_t parts, int64_t num_states, uint32_t k,
                                    void* state_keys, int64_t* state_hashes, int64_t* state_counts, hipStream_t st) {
    if (parts <= 0 || num_states <= 0) return hipSuccess;
    if (key_width == 8)
        return launch_keyed<int64_t, true>(part_keys, part_hashes, nullptr, nullptr, part_counts, num_states, num_states,
                                           parts, k, kHashPrecomputed, 0, state_keys, state_hashes, state_counts, st);
    return launch_keyed<int32_t, true>(part_keys, part_hashes, nullptr, nullptr, part_counts, num_states, num_states, parts,
                                       k, kHashPrecomputed, 0, state_keys, state_hashes, state_counts, st);
}

}  // namespace rsv
