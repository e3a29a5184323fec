// rsv_segdistinct.hip -- K5: S independent Sampler.distinct streams per launch (rsv_distinct_segmented).
// No reference counterpart; = S separate RandomValues instances (Sampler.scala:383-412), each seeded
// with java.util.Random(seed + stream_base + s), in the engine's set order (RSV_DISTINCT_SET): stream
// s keeps the min(k, D_s) distinct keys with the smallest (scrambled hash, key), written ascending.
// The reference's arrival-order tie replay (RSV_DISTINCT_ORDERED) is out of scope here: a caller
// that needs it for a colliding hash keeps separate handles.
//
// One TEAM of NT threads per stream, streams taken grid-stride.  The team holds P 16-byte entries
// (h, key) in LDS: the current set [0, m) ascending by (h, key), and behind it the candidates
// admitted since the last merge.  Per iteration it loads NT x kU elements (coalesced 8-/4-byte loads,
// kU in flight per lane) and takes them in kU steps of NT: h = scramble(r0, r1, hash(key)), admitted
// when (h, key) <= T, where T = (INT64_MAX, INT64_MAX) while the set holds fewer than k entries, else
// its k-th entry.  `<=`, not `h < T`: a distinct key with the boundary hash and a smaller key must
// get in; repeats of members pass too and fall out as adjacent equals in the merge.  Admitted
// entries are appended at one LDS atomicAdd per wave (ballot + prefix count); their order in the
// buffer does not matter, because the merge sorts by the whole (h, key) and equal entries are the
// same element.  The count is re-read by every wave between two barriers after each step, so the
// decision to merge is uniform.
// A merge runs when the buffer cannot take another full step (P >= k + NT, so one always fits
// afterwards), when 4k entries wait and no threshold is known yet, and at the end of the stream:
// bitonic sort of the first pow2ceil(m + c) entries in LDS (padded with the largest value -- a real
// entry equal to the pad sorts among the pads and is still inside the first m + c), drop of adjacent
// equals with an in-place block scan, keep the first k, reload T.
//
// Forms (DESIGN.md "Segmented distinct"):
//   k <= 64    NT = 64 (one wave per stream), P = 256: 4 KB of LDS, 32 streams resident per CU
//   k <= 256   NT = 64, P = 512: 8 KB, 19 streams per CU
//   k <= 1024  NT = 256, P = 2048: 32 KB, 4 workgroups per CU
//   k <= 4096  NT = 1024, P = 8192: 128 KB, one workgroup per CU
// The smaller P for k <= 64 is deliberate: a buffer that fills sooner gives a fresher T, so fewer
// entries are admitted, and a sort of 256 costs 0.4 of a sort of 512.
#include <algorithm>

#include "../../include/reservoir_hip.h"
#include "rsv_device.h"
#include "rsv_internal.h"
#include "rsv_segdistinct.h"

namespace rsv {

namespace {

using namespace segd;

template <typename KeyT, int NT>
__global__ __launch_bounds__(NT) void segdistinct_kernel(const KeyT* __restrict__ keys, const int64_t* __restrict__ hashes,
                                                         const int64_t* __restrict__ offsets, int64_t S, uint32_t k,
                                                         uint32_t P, int hash_kind, uint64_t seed0,
                                                         KeyT* __restrict__ out_keys, int64_t* __restrict__ out_hashes,
                                                         int64_t* __restrict__ counts) {
    extern __shared__ __align__(16) unsigned char seg_lds[];
    Ent* const se = (Ent*)seg_lds;
    __shared__ uint32_t s_cnt;
    __shared__ uint32_t s_scan[NT / 64 > 1 ? NT / 64 : 1];
    const uint32_t tid = threadIdx.x;
    constexpr int64_t kChunk = (int64_t)NT * kU;

    for (int64_t s = blockIdx.x; s < S; s += gridDim.x) {
        const int64_t lo = offsets[s], hi = offsets[s + 1];
        int64_t r0, r1;
        java_r0r1(seed0 + (uint64_t)s, r0, r1);
        uint32_t m = 0;      // set size
        uint32_t n_tot = 0;  // set + waiting candidates (= s_cnt, read between two barriers)
        int64_t Th = kMaxI64, Tk = kMaxI64;
        __syncthreads();  // the previous stream's output reads are done
        if (tid == 0) s_cnt = 0;
        __syncthreads();
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
                    if (hash_kind == kHashPrecomputed) hv[u] = hashes[i];
                }
            }
#pragma unroll
            for (int u = 0; u < kU; ++u) {
                const int64_t i = base + (int64_t)u * NT + tid;
                if (base + (int64_t)u * NT >= hi) break;  // uniform: the tail chunk's empty steps
                if (n_tot + NT > P || (m < k && n_tot >= 4 * k)) {
                    m = merge_set<NT>(se, n_tot, k, s_scan);
                    if (m == k) {
                        Th = se[k - 1].h;
                        Tk = se[k - 1].key;
                    }
                    __syncthreads();  // T is read before the appends below overwrite anything
                    if (tid == 0) s_cnt = m;
                    n_tot = m;
                    __syncthreads();
                }
                int64_t hashed;
                if (hash_kind == kHashPrecomputed)
                    hashed = hv[u];
                else if (hash_kind == kHashJavaLong)
                    hashed = hash_of<int64_t, kHashJavaLong>(key[u]);
                else if (hash_kind == kHashJavaInt)
                    hashed = hash_of<int64_t, kHashJavaInt>(key[u]);
                else
                    hashed = key[u];  // identity: the sign-extended key
                const int64_t h = scramble(r0, r1, hashed);
                const bool pass = i < hi && (h < Th || (h == Th && key[u] <= Tk));
                const uint64_t mask = __ballot(pass);
                if (mask) {
                    uint32_t b = 0;
                    if ((tid & 63) == (uint32_t)(__ffsll((long long)mask) - 1)) b = atomicAdd(&s_cnt, (uint32_t)__popcll(mask));
                    b = (uint32_t)__shfl((int)b, __ffsll((long long)mask) - 1);
                    if (pass) se[b + (uint32_t)__popcll(mask & ((1ULL << (tid & 63)) - 1))] = Ent{h, key[u]};
                }
                // every wave reads the same count: no append of the next step runs before the
                // second barrier
                __syncthreads();
                n_tot = s_cnt;
                __syncthreads();
            }
        }
        if (n_tot != m || m == 0) m = merge_set<NT>(se, n_tot, k, s_scan);
        __syncthreads();
        const int64_t ob = s * (int64_t)k;
        for (uint32_t i = tid; i < k; i += NT) {
            const Ent e = i < m ? se[i] : Ent{0, 0};
            out_keys[ob + i] = (KeyT)e.key;
            if (out_hashes) out_hashes[ob + i] = e.h;
        }
        if (tid == 0) counts[s] = m;
    }
}

template <typename KeyT, int NT>
hipError_t launch_form(const void* keys, const int64_t* hashes, const int64_t* offsets, int64_t S, uint32_t k, uint32_t P,
                       int hash_kind, uint64_t seed0, void* out_keys, int64_t* out_hashes, int64_t* counts,
                       hipStream_t st) {
    const size_t lds = (size_t)P * 16;
    if (lds > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute((const void*)segdistinct_kernel<KeyT, NT>,
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    // the teams the 256 CUs hold at once (LDS and 32 waves per CU), four times over
    const uint64_t per_cu = std::max<uint64_t>(1, std::min<uint64_t>((160 * 1024) / (lds + 256), 32 / (NT / 64)));
    const unsigned grid = (unsigned)std::min<uint64_t>((uint64_t)S, 256ull * per_cu * 4);
    hipLaunchKernelGGL((segdistinct_kernel<KeyT, NT>), dim3(grid), dim3(NT), lds, st, (const KeyT*)keys, hashes, offsets,
                       S, k, P, hash_kind, seed0, (KeyT*)out_keys, out_hashes, counts);
    return hipGetLastError();
}

template <typename KeyT>
hipError_t launch_keyed(const void* keys, const int64_t* hashes, const int64_t* offsets, int64_t S, uint32_t k,
                        int hash_kind, uint64_t seed0, void* out_keys, int64_t* out_hashes, int64_t* counts,
                        hipStream_t st) {
    if (k <= kSegDistinctWaveMaxK)  // P >= k + 192: three steps of 64 fit behind a full set
        return launch_form<KeyT, 64>(keys, hashes, offsets, S, k, k <= 64 ? 256 : 512, hash_kind, seed0, out_keys,
                                     out_hashes, counts, st);
    if (k <= 1024)
        return launch_form<KeyT, 256>(keys, hashes, offsets, S, k, 2048, hash_kind, seed0, out_keys, out_hashes, counts, st);
    return launch_form<KeyT, 1024>(keys, hashes, offsets, S, k, 8192, hash_kind, seed0, out_keys, out_hashes, counts, st);
}

}  // namespace

hipError_t launch_segdistinct(const void* keys, int key_width, const int64_t* hashes, const int64_t* offsets, int64_t S,
                              uint32_t k, int hash_kind, uint64_t seed0, void* out_keys, int64_t* out_hashes,
                              int64_t* counts, hipStream_t st) {
    if (S <= 0) return hipSuccess;
    if (key_width == 8)
        return launch_keyed<int64_t>(keys, hashes, offsets, S, k, hash_kind, seed0, out_keys, out_hashes, counts, st);
    return launch_keyed<int32_t>(keys, hashes, offsets, S, k, hash_kind, seed0, out_keys, out_hashes, counts, st);
}

}  // namespace rsv
