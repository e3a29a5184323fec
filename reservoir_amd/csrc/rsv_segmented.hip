// rsv_segmented.hip -- K2: S independent Algorithm-R samplers per launch (rsv_sample_segmented), one
// wave per stream; the reference counterpart is S separate Sampler instances (Sampler.scala:196-332).
//
// Work per stream of n elements (draw format R2, rsv_device.h): one level-0 Philox per 16-index block
// of [k, n) and one level-1 Philox per index whose level-0 byte leaves j_i < k possible
// (b_i (i+1) < 256 k).  At C3's shape (4096 elements, k = 64) every block is in the dense region: the
// candidates (~270 per stream, 9/10 of them real hits) crowd the head -- the first block holds ~15 of
// its 16 indices, the last ~0.1.
//
// Per iteration the wave evaluates 64 level-0 blocks (one per lane, Philox with the counter's high
// words wave-uniform), takes each block's candidate mask with a bit-sliced compare b < T (T from the
// block's first index), and appends the candidates -- 16-bit references (ring slot, lane, byte) into
// the block words it stashed in LDS -- to a per-wave FIFO at offsets from ONE wave prefix sum of the
// per-lane counts (5 ballots).  Whenever 64 candidates wait, every lane resolves one: it decodes its
// byte from the stashed block, runs the level-1 Philox and, on a hit, takes an LDS atomicMax on the
// stream's k-slot last-writer table.  (The previous form pushed candidates one per lane per ballot
// round and decoded the byte inside the round: ~1700 wave-instructions per C3 stream, PMC
// SQ_INSTS_VALU; this form ~4x fewer)  The winners' keys are gathered at the end.
//
// k >= 512 (k2::kWGMinK): one WORKGROUP of 8 waves per stream with one shared winner table
// (k2_segmented_wg, rsv_k2.h) -- per-wave tables would leave a CU one or two workgroups, and beyond
// k = 4416 not fit at all.  The table is u32 when the streams span < 2^32 elements (the host reads
// offsets[0] and offsets[S] once), in LDS while it fits beside the waves' rings (k <= ~29.5k), else
// the workgroup's slice of a per-device global scratch that is zeroed once and left zero by every
// launch -- no allocation or fill per call.
//
// Resumed (rsv_sample_segmented_update / _merge): the S streams are rows of caller-held
// state (keys, idx = each slot's last writer, next), a launch feeds each named row one more segment
// of its stream from any start index, and the largest index per slot wins.  The same two forms
// (k2_segmented_update, k2_segmented_update_wg) over the same element loops; the workgroup form keeps
// 64-bit table entries in LDS, so k <= kSegSampleStateMaxK.
//
// Byte keys (rsv_sample_segmented_rows / _rows_update / _rows_merge): the elements are
// rows of 16..256 bytes.  The same element loops find the winners without reading a row; separate
// kernels (k2_segmented_rows*, rsv_k2.h) then gather whole rows, lanes side by side on a row's 16- or
// 8-byte granules, with 64-bit byte offsets.  The key-typed kernels above are not instantiated for rows.
#include <algorithm>
#include <cstdlib>
#include <mutex>

#include "rsv_internal.h"
#include "rsv_k2.h"

namespace rsv {

using namespace k2;

namespace {
#define RSV_HIP_RET(expr)                      \
    do {                                       \
        const hipError_t _e = (expr);          \
        if (_e != hipSuccess) return _e;       \
    } while (0)

// The workgroup form's global tables (k too large for LDS): one scratch per device, zeroed ONCE when
// allocated and left zero by every launch (its gather swaps each entry back to 0), reused by the next
// launch on the same stream, or on any stream once the last launch's event has completed; a launch
// that finds it busy on another stream takes a private zeroed block instead.
struct GtScratch {
    void* p = nullptr;
    size_t bytes = 0;
    hipStream_t st = nullptr;
    hipEvent_t done = nullptr;
};
std::mutex g_gt_mu;
GtScratch g_gt[64];

hipError_t gt_acquire(int dev, size_t bytes, hipStream_t st, void** out, bool* priv) {
    GtScratch& c = g_gt[dev & 63];
    *priv = false;
    const bool idle = !c.p || c.st == st || !c.done || hipEventQuery(c.done) == hipSuccess;
    if (c.p && idle && bytes <= c.bytes) {
        *out = c.p;
        return hipSuccess;
    }
    if (!idle) {  // another stream's launch may still use it
        *priv = true;
        hipError_t e = hipMallocAsync(out, bytes, st);
        return e == hipSuccess ? hipMemsetAsync(*out, 0, bytes, st) : e;
    }
    if (c.p) {  // idle but too small: replaced (its last user finished or is this stream)
        hipError_t e = hipStreamSynchronize(st);
        if (e == hipSuccess) e = hipFree(c.p);
        c.p = nullptr;
        c.bytes = 0;
        if (e != hipSuccess) return e;
    }
    hipError_t e = hipMalloc(&c.p, bytes);
    if (e != hipSuccess) return e;
    c.bytes = bytes;
    *out = c.p;
    return hipMemsetAsync(c.p, 0, bytes, st);
}

void gt_release(int dev, hipStream_t st, bool priv, void* p) {
    if (priv) {
        (void)hipFreeAsync(p, st);
        return;
    }
    GtScratch& c = g_gt[dev & 63];
    if (!c.done && hipEventCreateWithFlags(&c.done, hipEventDisableTiming) != hipSuccess) c.done = nullptr;
    if (c.done) (void)hipEventRecord(c.done, st);
    c.st = st;
}

// RSV_K2_FIFO_CAP (tests, read once per process): a lower bulk-append limit, so the ballot-
// round overflow path runs
uint32_t env_fifo_cap() {
    static const uint32_t fifo_cap = [] {
        const char* e = std::getenv("RSV_K2_FIFO_CAP");
        return e ? (uint32_t)std::atoi(e) : k2::kQCap;
    }();
    return fifo_cap;
}

template <typename KeyT, typename TabT>
hipError_t launch_wg(const KeyT* keys, const int64_t* offsets, int64_t S, uint32_t k, const DrawParams& dp,
                     KeyT* out, int64_t* counts, hipStream_t st, uint32_t fifo_cap) {
    const uint32_t k0 = (uint32_t)dp.seed, k1 = (uint32_t)(dp.seed >> 32);
    const size_t lds = k2::lds_bytes_wg(k, sizeof(TabT), false);
    if (lds <= k2::kLdsMax) {
        // as many workgroups as the CUs hold at once, twice over (streams are taken grid-stride)
        const uint64_t per_cu = std::max<uint64_t>(1, k2::kLdsMax / lds);
        const unsigned grid = (unsigned)std::min<uint64_t>((uint64_t)S, 256ull * per_cu * 2);
        hipLaunchKernelGGL((k2_segmented_wg<KeyT, TabT, false>), dim3(grid), dim3(64 * kWavesWG), lds, st, keys,
                           offsets, S, k, k0, k1, dp.stream, out, counts, fifo_cap, (TabT*)nullptr);
        return hipGetLastError();
    }
    int dev = 0;
    RSV_HIP_RET(hipGetDevice(&dev));
    const unsigned grid = (unsigned)std::min<uint64_t>((uint64_t)S, 512);
    const size_t bytes = (size_t)grid * k * sizeof(TabT);
    std::lock_guard<std::mutex> lk(g_gt_mu);
    void* gt = nullptr;
    bool priv = false;
    RSV_HIP_RET(gt_acquire(dev, bytes, st, &gt, &priv));
    hipLaunchKernelGGL((k2_segmented_wg<KeyT, TabT, true>), dim3(grid), dim3(64 * kWavesWG),
                       k2::lds_bytes_wg(k, sizeof(TabT), true), st, keys, offsets, S, k, k0, k1, dp.stream, out,
                       counts, fifo_cap, (TabT*)gt);
    const hipError_t e = hipGetLastError();
    gt_release(dev, st, priv, gt);
    return e;
}
}  // namespace

hipError_t launch_segmented(const void* keys, int key_width, const int64_t* offsets, int64_t S, uint32_t k,
                            const DrawParams& dp, void* out, int64_t* counts, hipStream_t st) {
    if (S <= 0) return hipSuccess;
    const uint32_t fifo_cap = env_fifo_cap();
    if (k >= k2::kWGMinK) {  // one workgroup per stream
        // every index fits 32 bits when the streams together span < 2^32 elements: u32 tables
        int64_t ends[2] = {0, 0};
        RSV_HIP_RET(hipMemcpyAsync(&ends[0], offsets, 8, hipMemcpyDeviceToHost, st));
        RSV_HIP_RET(hipMemcpyAsync(&ends[1], offsets + S, 8, hipMemcpyDeviceToHost, st));
        RSV_HIP_RET(hipStreamSynchronize(st));
        const bool t32 = ends[1] - ends[0] < ((int64_t)1 << 32);
        if (key_width == 8)
            return t32 ? launch_wg<int64_t, uint32_t>((const int64_t*)keys, offsets, S, k, dp, (int64_t*)out, counts, st, fifo_cap)
                       : launch_wg<int64_t, unsigned long long>((const int64_t*)keys, offsets, S, k, dp, (int64_t*)out,
                                                                counts, st, fifo_cap);
        return t32 ? launch_wg<int32_t, uint32_t>((const int32_t*)keys, offsets, S, k, dp, (int32_t*)out, counts, st, fifo_cap)
                   : launch_wg<int32_t, unsigned long long>((const int32_t*)keys, offsets, S, k, dp, (int32_t*)out,
                                                            counts, st, fifo_cap);
    }
    const size_t lds = k2::lds_bytes(k);
    const uint32_t k0 = (uint32_t)dp.seed, k1 = (uint32_t)(dp.seed >> 32);
    // up to 128 four-wave workgroups per CU over the launch (C3: 8 streams per wave): tools/micro_k2 G
    // (r03ai) 1.78 ms at 4096 workgroups, 1.71 at 16384, 1.65 at 32768, 1.66-1.68 at 65536, 1.84 at
    // one stream per wave (262144: every workgroup rebuilds the threshold table)
    const uint64_t blocks = ((uint64_t)S + kWaves - 1) / kWaves;
    const unsigned grid = (unsigned)std::min<uint64_t>(blocks, 256ull * 128);
    if (key_width == 8)
        hipLaunchKernelGGL(k2_segmented<int64_t>, dim3(grid), dim3(64 * kWaves), lds, st, (const int64_t*)keys,
                           offsets, S, k, k0, k1, dp.stream, (int64_t*)out, counts, fifo_cap);
    else
        hipLaunchKernelGGL(k2_segmented<int32_t>, dim3(grid), dim3(64 * kWaves), lds, st, (const int32_t*)keys,
                           offsets, S, k, k0, k1, dp.stream, (int32_t*)out, counts, fifo_cap);
    return hipGetLastError();
}

// the largest k whose 64-bit winner table fits one workgroup's LDS beside the waves' rings
static_assert(k2::lds_bytes_wg(kSegSampleStateMaxK, 8, false) <= k2::kLdsMax &&
                  k2::lds_bytes_wg(kSegSampleStateMaxK + 1, 8, false) > k2::kLdsMax,
              "kSegSampleStateMaxK is the LDS limit of k2_segmented_update_wg");

namespace {
template <typename KeyT>
hipError_t launch_update(const KeyT* keys, const int64_t* offsets, const int64_t* ids, const int64_t* bases, int64_t B,
                         int64_t S, uint32_t k, const DrawParams& dp, KeyT* state_keys, int64_t* state_idx,
                         int64_t* state_next, hipStream_t st) {
    const uint32_t k0 = (uint32_t)dp.seed, k1 = (uint32_t)(dp.seed >> 32);
    const uint32_t fifo_cap = env_fifo_cap();
    if (k >= k2::kWGMinK) {  // one workgroup per segment, grids as launch_wg
        const size_t lds = k2::lds_bytes_wg(k, 8, false);
        const uint64_t per_cu = std::max<uint64_t>(1, k2::kLdsMax / lds);
        const unsigned grid = (unsigned)std::min<uint64_t>((uint64_t)B, 256ull * per_cu * 2);
        hipLaunchKernelGGL(k2_segmented_update_wg<KeyT>, dim3(grid), dim3(64 * kWavesWG), lds, st, keys, offsets, ids,
                           bases, B, S, k, k0, k1, dp.stream, state_keys, state_idx, state_next, fifo_cap);
        return hipGetLastError();
    }
    const uint64_t blocks = ((uint64_t)B + kWaves - 1) / kWaves;  // grids as launch_segmented
    const unsigned grid = (unsigned)std::min<uint64_t>(blocks, 256ull * 128);
    hipLaunchKernelGGL(k2_segmented_update<KeyT>, dim3(grid), dim3(64 * kWaves), k2::lds_bytes(k), st, keys, offsets,
                       ids, bases, B, S, k, k0, k1, dp.stream, state_keys, state_idx, state_next, fifo_cap);
    return hipGetLastError();
}
}  // namespace

hipError_t launch_segmented_update(const void* keys, int key_width, const int64_t* offsets, const int64_t* stream_ids,
                                   const int64_t* bases, int64_t num_segments, int64_t num_states, uint32_t k,
                                   const DrawParams& dp, void* state_keys, int64_t* state_idx, int64_t* state_next,
                                   hipStream_t st) {
    if (num_segments <= 0 || num_states <= 0) return hipSuccess;
    if (k > kSegSampleStateMaxK) return hipErrorInvalidValue;
    if (key_width == 8)
        return launch_update<int64_t>((const int64_t*)keys, offsets, stream_ids, bases, num_segments, num_states, k, dp,
                                      (int64_t*)state_keys, state_idx, state_next, st);
    return launch_update<int32_t>((const int32_t*)keys, offsets, stream_ids, bases, num_segments, num_states, k, dp,
                                  (int32_t*)state_keys, state_idx, state_next, st);
}

hipError_t launch_segmented_merge(const void* part_keys, int key_width, const int64_t* part_idx,
                                  const int64_t* part_next, int32_t parts, int64_t num_states, uint32_t k,
                                  void* state_keys, int64_t* state_idx, int64_t* state_next, hipStream_t st) {
    if (parts <= 0 || num_states <= 0) return hipSuccess;
    const uint64_t blocks = ((uint64_t)num_states * k + 255) / 256;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    if (key_width == 8)
        hipLaunchKernelGGL(k2_segmented_merge<int64_t>, dim3((unsigned)blocks), dim3(256), 0, st,
                           (const int64_t*)part_keys, part_idx, part_next, parts, num_states, k, (int64_t*)state_keys,
                           state_idx, state_next);
    else
        hipLaunchKernelGGL(k2_segmented_merge<int32_t>, dim3((unsigned)blocks), dim3(256), 0, st,
                           (const int32_t*)part_keys, part_idx, part_next, parts, num_states, k, (int32_t*)state_keys,
                           state_idx, state_next);
    return hipGetLastError();
}

// ---- byte keys (rows) ----------------------------------------------------------------------------
namespace {
// 16-byte granules where every row of every buffer sits on a 16-byte boundary, else 8-byte ones
bool rows_vec16(int key_width, const void* a, const void* b) {
    return key_width % 16 == 0 && (((uintptr_t)a | (uintptr_t)b) & 15) == 0;
}

template <typename G, typename TabT>
hipError_t launch_rows_wg(const unsigned char* rows, uint32_t C, const int64_t* offsets, int64_t S, uint32_t k,
                          const DrawParams& dp, unsigned char* out, int64_t* counts, hipStream_t st,
                          uint32_t fifo_cap) {
    const uint32_t k0 = (uint32_t)dp.seed, k1 = (uint32_t)(dp.seed >> 32);
    const size_t lds = k2::lds_bytes_wg(k, sizeof(TabT), false);
    if (lds <= k2::kLdsMax) {  // grids as launch_wg
        const uint64_t per_cu = std::max<uint64_t>(1, k2::kLdsMax / lds);
        const unsigned grid = (unsigned)std::min<uint64_t>((uint64_t)S, 256ull * per_cu * 2);
        hipLaunchKernelGGL((k2_segmented_rows_wg<G, TabT, false>), dim3(grid), dim3(64 * kWavesWG), lds, st, rows,
                           offsets, S, k, C, k0, k1, dp.stream, out, counts, fifo_cap, (TabT*)nullptr);
        return hipGetLastError();
    }
    int dev = 0;
    RSV_HIP_RET(hipGetDevice(&dev));
    const unsigned grid = (unsigned)std::min<uint64_t>((uint64_t)S, 512);
    const size_t bytes = (size_t)grid * k * sizeof(TabT);
    std::lock_guard<std::mutex> lk(g_gt_mu);
    void* gt = nullptr;
    bool priv = false;
    RSV_HIP_RET(gt_acquire(dev, bytes, st, &gt, &priv));
    hipLaunchKernelGGL((k2_segmented_rows_wg<G, TabT, true>), dim3(grid), dim3(64 * kWavesWG),
                       k2::lds_bytes_wg(k, sizeof(TabT), true), st, rows, offsets, S, k, C, k0, k1, dp.stream, out,
                       counts, fifo_cap, (TabT*)gt);
    const hipError_t e = hipGetLastError();
    gt_release(dev, st, priv, gt);
    return e;
}

template <typename G>
hipError_t launch_rows(const unsigned char* rows, int key_width, const int64_t* offsets, int64_t S, uint32_t k,
                       const DrawParams& dp, unsigned char* out, int64_t* counts, hipStream_t st) {
    const uint32_t C = (uint32_t)key_width / (uint32_t)sizeof(G);
    const uint32_t fifo_cap = env_fifo_cap();
    if (k >= k2::kWGMinK) {  // one workgroup per stream; u32 tables by the rule of launch_segmented
        int64_t ends[2] = {0, 0};
        RSV_HIP_RET(hipMemcpyAsync(&ends[0], offsets, 8, hipMemcpyDeviceToHost, st));
        RSV_HIP_RET(hipMemcpyAsync(&ends[1], offsets + S, 8, hipMemcpyDeviceToHost, st));
        RSV_HIP_RET(hipStreamSynchronize(st));
        if (ends[1] - ends[0] < ((int64_t)1 << 32))
            return launch_rows_wg<G, uint32_t>(rows, C, offsets, S, k, dp, out, counts, st, fifo_cap);
        return launch_rows_wg<G, unsigned long long>(rows, C, offsets, S, k, dp, out, counts, st, fifo_cap);
    }
    const uint32_t k0 = (uint32_t)dp.seed, k1 = (uint32_t)(dp.seed >> 32);
    const uint64_t blocks = ((uint64_t)S + kWaves - 1) / kWaves;  // grids as launch_segmented
    const unsigned grid = (unsigned)std::min<uint64_t>(blocks, 256ull * 128);
    // one (slot, granule) pair per lane: the gather is deferred past the next stream's draws (C3 with UUID
    // rows: 1.79 ms against 1.85 ms plain, profiles/segmented_rows/bench.json).  RSV_K2_ROWS_DEFER=0 (read
    // once per process) keeps the plain gather, for that A/B in tools/bench_segmented_rows.py.
    static const bool defer = [] {
        const char* e = std::getenv("RSV_K2_ROWS_DEFER");
        return !e || std::atoi(e) != 0;
    }();
    if (defer && (uint64_t)k * C <= 64)
        hipLaunchKernelGGL((k2_segmented_rows<G, true>), dim3(grid), dim3(64 * kWaves), k2::lds_bytes(k), st, rows,
                           offsets, S, k, C, k0, k1, dp.stream, out, counts, fifo_cap);
    else
        hipLaunchKernelGGL((k2_segmented_rows<G, false>), dim3(grid), dim3(64 * kWaves), k2::lds_bytes(k), st, rows,
                           offsets, S, k, C, k0, k1, dp.stream, out, counts, fifo_cap);
    return hipGetLastError();
}

template <typename G>
hipError_t launch_rows_update(const unsigned char* rows, int key_width, const int64_t* offsets, const int64_t* ids,
                              const int64_t* bases, int64_t B, int64_t S, uint32_t k, const DrawParams& dp,
                              unsigned char* state_rows, int64_t* state_idx, int64_t* state_next, hipStream_t st) {
    const uint32_t C = (uint32_t)key_width / (uint32_t)sizeof(G);
    const uint32_t k0 = (uint32_t)dp.seed, k1 = (uint32_t)(dp.seed >> 32);
    const uint32_t fifo_cap = env_fifo_cap();
    if (k >= k2::kWGMinK) {  // grids as launch_update
        const size_t lds = k2::lds_bytes_wg(k, 8, false);
        const uint64_t per_cu = std::max<uint64_t>(1, k2::kLdsMax / lds);
        const unsigned grid = (unsigned)std::min<uint64_t>((uint64_t)B, 256ull * per_cu * 2);
        hipLaunchKernelGGL(k2_segmented_rows_update_wg<G>, dim3(grid), dim3(64 * kWavesWG), lds, st, rows, offsets,
                           ids, bases, B, S, k, C, k0, k1, dp.stream, state_rows, state_idx, state_next, fifo_cap);
        return hipGetLastError();
    }
    const uint64_t blocks = ((uint64_t)B + kWaves - 1) / kWaves;
    const unsigned grid = (unsigned)std::min<uint64_t>(blocks, 256ull * 128);
    hipLaunchKernelGGL(k2_segmented_rows_update<G>, dim3(grid), dim3(64 * kWaves), k2::lds_bytes(k), st, rows, offsets,
                       ids, bases, B, S, k, C, k0, k1, dp.stream, state_rows, state_idx, state_next, fifo_cap);
    return hipGetLastError();
}
}  // namespace

hipError_t launch_segmented_rows(const void* rows, int key_width, const int64_t* offsets, int64_t S, uint32_t k,
                                 const DrawParams& dp, void* out_rows, int64_t* counts, hipStream_t st) {
    if (S <= 0) return hipSuccess;
    if (rows_vec16(key_width, rows, out_rows))
        return launch_rows<uint4>((const unsigned char*)rows, key_width, offsets, S, k, dp, (unsigned char*)out_rows,
                                  counts, st);
    return launch_rows<uint64_t>((const unsigned char*)rows, key_width, offsets, S, k, dp, (unsigned char*)out_rows,
                                 counts, st);
}

hipError_t launch_segmented_rows_update(const void* rows, int key_width, const int64_t* offsets,
                                        const int64_t* stream_ids, const int64_t* bases, int64_t num_segments,
                                        int64_t num_states, uint32_t k, const DrawParams& dp, void* state_rows,
                                        int64_t* state_idx, int64_t* state_next, hipStream_t st) {
    if (num_segments <= 0 || num_states <= 0) return hipSuccess;
    if (k > kSegSampleStateMaxK) return hipErrorInvalidValue;
    if (rows_vec16(key_width, rows, state_rows))
        return launch_rows_update<uint4>((const unsigned char*)rows, key_width, offsets, stream_ids, bases,
                                         num_segments, num_states, k, dp, (unsigned char*)state_rows, state_idx,
                                         state_next, st);
    return launch_rows_update<uint64_t>((const unsigned char*)rows, key_width, offsets, stream_ids, bases, num_segments,
                                        num_states, k, dp, (unsigned char*)state_rows, state_idx, state_next, st);
}

hipError_t launch_segmented_rows_merge(const void* part_rows, int key_width, const int64_t* part_idx,
                                       const int64_t* part_next, int32_t parts, int64_t num_states, uint32_t k,
                                       void* state_rows, int64_t* state_idx, int64_t* state_next, hipStream_t st) {
    if (parts <= 0 || num_states <= 0) return hipSuccess;
    const uint64_t blocks = ((uint64_t)num_states * k + 255) / 256;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    if (rows_vec16(key_width, part_rows, state_rows))
        hipLaunchKernelGGL(k2_segmented_rows_merge<uint4>, dim3((unsigned)blocks), dim3(256), 0, st,
                           (const unsigned char*)part_rows, part_idx, part_next, parts, num_states, k,
                           (uint32_t)key_width / 16u, (unsigned char*)state_rows, state_idx, state_next);
    else
        hipLaunchKernelGGL(k2_segmented_rows_merge<uint64_t>, dim3((unsigned)blocks), dim3(256), 0, st,
                           (const unsigned char*)part_rows, part_idx, part_next, parts, num_states, k,
                           (uint32_t)key_width / 8u, (unsigned char*)state_rows, state_idx, state_next);
    return hipGetLastError();
}

}  // namespace rsv
