// rsv_group.hip -- the grouping pass (rsv_group_by_stream): a micro-batch tagged with state
// rows in arrival order becomes the dense CSR the segmented update entry points take -- offsets[num_states + 1]
// and order[n], the batch positions row by row, each row's in arrival order.
//
// A stable LSD radix partition over the low bits of the id only: bin = id inside [0, S), else S (the dropped
// elements, which so land behind the last row in arrival order), bits = the width of S, P = ceil(bits / 8)
// passes of ceil(bits / P) <= 8 bits each.  A pass carries (bin, position), 4 + 4 bytes; the first reads the
// ids themselves with the position implicit, the last writes its positions into `order`.  Per pass:
//   group_hist     one workgroup per tile of 4096 elements counts the tile's digits into hist[digit][tile]
//   scan_*         the exclusive scan of hist as one array (digit-major, so a digit's tiles follow each other
//                  in tile order): block sums, their scan by one workgroup, the scan within blocks
//   group_scatter  the tile again: every element's rank among the tile's elements of its digit, then the
//                  element goes to hist[digit][tile] + rank
// The rank decides the order, and nothing in it depends on timing: a tile is laid out (wave, round, lane), a
// round's equal digits are found with ballots (rank inside the round = the peers in lower lanes), a wave's
// earlier rounds are counted per digit in the wave's own LDS row, and the waves' rows are summed in wave
// order after a barrier.  The only atomics are the counts of group_hist, and a count does not depend on the
// order of its increments.  After the last pass the bins lie sorted beside `order`, and offsets[r] is the
// lower bound of r among them: one thread per row, a binary search each.
//
// Stream-ordered, no host wait: the scratch (two bin arrays, one position array, hist and its block sums; 12
// bytes per element and 0.25 for hist from two passes on, 4.25 for one pass) comes from hipMallocAsync and goes
// back with hipFreeAsync.
#include <algorithm>
#include <type_traits>

#include "rsv_internal.h"

namespace rsv {

namespace {
#define RSV_HIP_RET(expr)                      \
    do {                                       \
        const hipError_t _e = (expr);          \
        if (_e != hipSuccess) return _e;       \
    } while (0)

constexpr uint32_t kThreads = 256, kWavesG = 4, kItems = 16;
constexpr uint32_t kTile = kThreads * kItems;  // elements per workgroup and pass
constexpr uint32_t kRadix = 256;               // digit values a pass can hold (8 bits)
constexpr uint32_t kScanItems = 8, kScanChunk = kThreads * kScanItems;  // hist entries per scan workgroup

// the bin of an id: its row, or S for an id outside [0, S)
template <typename IdT>
__device__ __forceinline__ uint32_t bin_of(IdT id, uint32_t S) {
    return (id >= 0 && (uint64_t)id < (uint64_t)S) ? (uint32_t)id : S;
}

// element i of a pass's input: the ids (first pass: SrcT is their signed type) or the carried bins (uint32_t)
template <typename SrcT>
__device__ __forceinline__ uint32_t load_bin(const SrcT* __restrict__ src, uint32_t i, uint32_t S) {
    if constexpr (std::is_signed<SrcT>::value) return bin_of(src[i], S);
    else return src[i];
}

template <typename SrcT>
__global__ __launch_bounds__(kThreads) void group_hist(const SrcT* __restrict__ src, uint32_t n, uint32_t S,
                                                       uint32_t shift, uint32_t mask, uint32_t* __restrict__ hist,
                                                       uint32_t tiles) {
    __shared__ uint32_t h[kRadix];
    h[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t base = blockIdx.x * kTile;
#pragma unroll 4
    for (uint32_t t = threadIdx.x; t < kTile; t += kThreads) {
        const uint32_t i = base + t;
        if (i < n) atomicAdd(&h[(load_bin(src, i, S) >> shift) & mask], 1u);
    }
    __syncthreads();
    if (threadIdx.x <= mask) hist[threadIdx.x * tiles + blockIdx.x] = h[threadIdx.x];
}

// the exclusive prefix of v over the workgroup's 256 threads and their total; sh: kWavesG words of LDS
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t v, uint32_t* total, uint32_t* sh) {
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t x = v;
#pragma unroll
    for (uint32_t o = 1; o < 64; o <<= 1) {
        const uint32_t y = __shfl_up(x, o);
        if (lane >= o) x += y;
    }
    if (lane == 63) sh[wave] = x;
    __syncthreads();
    uint32_t before = 0, tot = 0;
#pragma unroll
    for (uint32_t w = 0; w < kWavesG; ++w) {
        const uint32_t t = sh[w];
        before += w < wave ? t : 0u;
        tot += t;
    }
    __syncthreads();  // sh may be written again
    *total = tot;
    return before + x - v;
}

__global__ __launch_bounds__(kThreads) void scan_sums(const uint32_t* __restrict__ a, uint32_t m,
                                                      uint32_t* __restrict__ sums) {
    __shared__ uint32_t sh[kWavesG];
    const uint32_t i0 = blockIdx.x * kScanChunk + threadIdx.x * kScanItems;
    uint32_t v = 0;
#pragma unroll
    for (uint32_t u = 0; u < kScanItems; ++u) v += i0 + u < m ? a[i0 + u] : 0u;
    uint32_t tot;
    block_excl_scan(v, &tot, sh);
    if (threadIdx.x == 0) sums[blockIdx.x] = tot;
}

// one workgroup: sums[0, nb) to their exclusive scan, 256 at a time with a carry
__global__ __launch_bounds__(kThreads) void scan_of_sums(uint32_t* __restrict__ sums, uint32_t nb) {
    __shared__ uint32_t sh[kWavesG];
    uint32_t carry = 0;
    for (uint32_t c = 0; c < nb; c += kThreads) {
        const uint32_t i = c + threadIdx.x;
        const uint32_t v = i < nb ? sums[i] : 0u;
        uint32_t tot;
        const uint32_t e = block_excl_scan(v, &tot, sh);
        if (i < nb) sums[i] = carry + e;
        carry += tot;
    }
}

__global__ __launch_bounds__(kThreads) void scan_apply(uint32_t* __restrict__ a, uint32_t m,
                                                       const uint32_t* __restrict__ sums) {
    __shared__ uint32_t sh[kWavesG];
    const uint32_t i0 = blockIdx.x * kScanChunk + threadIdx.x * kScanItems;
    uint32_t x[kScanItems], v = 0;
#pragma unroll
    for (uint32_t u = 0; u < kScanItems; ++u) {
        x[u] = i0 + u < m ? a[i0 + u] : 0u;
        v += x[u];
    }
    uint32_t tot;
    uint32_t run = sums[blockIdx.x] + block_excl_scan(v, &tot, sh);
#pragma unroll
    for (uint32_t u = 0; u < kScanItems; ++u) {
        if (i0 + u < m) a[i0 + u] = run;
        run += x[u];
    }
}

// hist: scanned, so hist[d * tiles + tile] is where the tile's first element of digit d goes
template <typename SrcT>
__global__ __launch_bounds__(kThreads) void group_scatter(const SrcT* __restrict__ src,
                                                          const uint32_t* __restrict__ pos_in, uint32_t n, uint32_t S,
                                                          uint32_t shift, uint32_t mask,
                                                          const uint32_t* __restrict__ hist, uint32_t tiles,
                                                          uint32_t* __restrict__ bins_out,
                                                          uint32_t* __restrict__ pos_out) {
    constexpr bool FIRST = std::is_signed<SrcT>::value;  // the position is the element's own index
    __shared__ uint32_t cnt[kWavesG][kRadix];  // per wave: its elements of each digit so far, then its base
    __shared__ uint32_t bin_base[kRadix];      // the tile's first destination per digit
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
#pragma unroll
    for (uint32_t w = 0; w < kWavesG; ++w) cnt[w][tid] = 0;
    __syncthreads();
    // the tile in (wave, round, lane) order: round r of this wave is 64 consecutive elements
    const uint32_t base = blockIdx.x * kTile + wave * (kItems * 64) + lane;
    uint32_t bin[kItems], pos[kItems], rank[kItems];
#pragma unroll
    for (uint32_t r = 0; r < kItems; ++r) {
        const uint32_t i = base + r * 64;
        const bool valid = i < n;
        bin[r] = valid ? load_bin(src, i, S) : 0u;
        if constexpr (FIRST) pos[r] = i;
        else pos[r] = valid ? pos_in[i] : 0u;
    }
    volatile uint32_t* mine = cnt[wave];
    const unsigned long long lower = (1ull << lane) - 1ull;
#pragma unroll
    for (uint32_t r = 0; r < kItems; ++r) {
        const bool valid = base + r * 64 < n;
        const uint32_t d = (bin[r] >> shift) & mask;
        // the lanes of this round that hold the same digit
        unsigned long long peers = __builtin_amdgcn_ballot_w64(valid);
#pragma unroll
        for (uint32_t b = 0; b < 8; ++b) {
            const bool bit = (d >> b) & 1u;
            const unsigned long long bal = __builtin_amdgcn_ballot_w64(valid && bit);
            peers &= bit ? bal : ~bal;
        }
        const uint32_t below = (uint32_t)__popcll(peers & lower), group = (uint32_t)__popcll(peers);
        // one wave's LDS operations complete in order: every peer reads the count before the last peer moves it
        const uint32_t before = valid ? mine[d] : 0u;
        __builtin_amdgcn_wave_barrier();
        if (valid && below + 1 == group) mine[d] = before + group;
        __builtin_amdgcn_wave_barrier();
        rank[r] = before + below;
    }
    __syncthreads();
    {  // thread d: the waves' counts of digit d to their exclusive sums in wave order
        uint32_t run = 0;
#pragma unroll
        for (uint32_t w = 0; w < kWavesG; ++w) {
            const uint32_t t = cnt[w][tid];
            cnt[w][tid] = run;
            run += t;
        }
        bin_base[tid] = tid <= mask ? hist[tid * tiles + blockIdx.x] : 0u;
    }
    __syncthreads();
#pragma unroll
    for (uint32_t r = 0; r < kItems; ++r) {
        if (base + r * 64 < n) {
            const uint32_t d = (bin[r] >> shift) & mask;
            const uint32_t dst = bin_base[d] + cnt[wave][d] + rank[r];
            if (dst < n) {  // always, for a hist of this input
                bins_out[dst] = bin[r];
                pos_out[dst] = pos[r];
            }
        }
    }
}

// offsets[r] = the first position whose bin is >= r, r in [0, S]
__global__ __launch_bounds__(kThreads) void group_offsets(const uint32_t* __restrict__ bins, uint32_t n, uint32_t S,
                                                          int64_t* __restrict__ offsets) {
    const uint64_t r = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (r > S) return;
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (bins[mid] < r) lo = mid + 1;
        else hi = mid;
    }
    offsets[r] = (int64_t)lo;
}

size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

template <typename SrcT>
hipError_t launch_pass(const SrcT* src, const uint32_t* pos_in, uint32_t n, uint32_t S, uint32_t shift, uint32_t mask,
                       uint32_t* hist, uint32_t* sums, uint32_t tiles, uint32_t* bins_out, uint32_t* pos_out,
                       hipStream_t st) {
    const uint32_t m = (mask + 1) * tiles, nb = (m + kScanChunk - 1) / kScanChunk;
    hipLaunchKernelGGL(group_hist<SrcT>, dim3(tiles), dim3(kThreads), 0, st, src, n, S, shift, mask, hist, tiles);
    hipLaunchKernelGGL(scan_sums, dim3(nb), dim3(kThreads), 0, st, hist, m, sums);
    hipLaunchKernelGGL(scan_of_sums, dim3(1), dim3(kThreads), 0, st, sums, nb);
    hipLaunchKernelGGL(scan_apply, dim3(nb), dim3(kThreads), 0, st, hist, m, sums);
    hipLaunchKernelGGL(group_scatter<SrcT>, dim3(tiles), dim3(kThreads), 0, st, src, pos_in, n, S, shift, mask, hist,
                       tiles, bins_out, pos_out);
    return hipGetLastError();
}

// the passes over num_states rows and the bits each takes
void group_plan(int64_t num_states, int* passes, int* digit_bits) {
    int bits = 1;
    while (bits < 32 && ((uint64_t)num_states >> bits) != 0) ++bits;  // the width of the largest bin, num_states
    *passes = (bits + 7) / 8;
    *digit_bits = (bits + *passes - 1) / *passes;
}
}  // namespace

hipError_t launch_group_by_stream(const void* ids, int id_width, int64_t n64, int64_t num_states, int64_t* offsets,
                                  int32_t* order, hipStream_t st) {
    if (n64 <= 0) return hipMemsetAsync(offsets, 0, (size_t)(num_states + 1) * sizeof(int64_t), st);
    const uint32_t n = (uint32_t)n64, S = (uint32_t)num_states;
    int passes = 0, db = 0;
    group_plan(num_states, &passes, &db);
    const uint32_t mask = (1u << db) - 1u;
    const uint32_t tiles = (n + kTile - 1) / kTile;
    const uint32_t m = (mask + 1) * tiles, nb = (m + kScanChunk - 1) / kScanChunk;
    // scratch: bins A | bins B | positions | hist | block sums (B and the positions from two passes on)
    const size_t arr = align256((size_t)n * 4), more = passes > 1 ? 1 : 0;
    const size_t o_b = arr, o_p = o_b + more * arr, o_h = o_p + more * arr, o_s = o_h + align256((size_t)m * 4);
    unsigned char* scratch = nullptr;
    RSV_HIP_RET(hipMallocAsync((void**)&scratch, o_s + align256((size_t)nb * 4), st));
    uint32_t* bins[2] = {(uint32_t*)scratch, (uint32_t*)(scratch + o_b)};
    uint32_t* spare = (uint32_t*)(scratch + o_p);
    uint32_t* hist = (uint32_t*)(scratch + o_h);
    uint32_t* sums = (uint32_t*)(scratch + o_s);
    hipError_t e = hipSuccess;
    const uint32_t* pos_in = nullptr;
    for (int p = 0; p < passes && e == hipSuccess; ++p) {
        // the positions alternate between `order` and the spare array so that the last pass writes `order`
        uint32_t* pos_out = (passes - 1 - p) % 2 == 0 ? (uint32_t*)order : spare;
        uint32_t* bins_out = bins[p & 1];
        const uint32_t shift = (uint32_t)(p * db);
        if (p == 0)
            e = id_width == 8 ? launch_pass((const int64_t*)ids, pos_in, n, S, shift, mask, hist, sums, tiles, bins_out,
                                            pos_out, st)
                              : launch_pass((const int32_t*)ids, pos_in, n, S, shift, mask, hist, sums, tiles, bins_out,
                                            pos_out, st);
        else
            e = launch_pass((const uint32_t*)bins[(p - 1) & 1], pos_in, n, S, shift, mask, hist, sums, tiles, bins_out,
                            pos_out, st);
        pos_in = pos_out;
    }
    if (e == hipSuccess) {
        const uint64_t rows = (uint64_t)S + 1;
        hipLaunchKernelGGL(group_offsets, dim3((unsigned)((rows + kThreads - 1) / kThreads)), dim3(kThreads), 0, st,
                           (const uint32_t*)bins[(passes - 1) & 1], n, S, offsets);
        e = hipGetLastError();
    }
    const hipError_t f = hipFreeAsync(scratch, st);
    return e == hipSuccess ? f : e;
}

}  // namespace rsv
