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
//
// Keyless (rsv_sample_segmented_indexed / _update / _merge): only the streams' lengths reach the
// device and indices come back.  The kernels (rsv_indexed.hip, declared in rsv_k2_indexed.h) run the same element
// loops and forms; the launchers are at the end of this file, with the split form of the stateless launch.
//
// Through a permutation (rsv_sample_segmented_update_indirect / _rows_update_indirect): the two
// resumed launches with segment b's p-th element at keys[order[offsets[b] + p]], `order` being what
// rsv_group_by_stream (rsv_group.hip) writes for a batch in arrival order.  Kernels of their own beside the direct
// ones (k2_segmented_update_indirect*, k2_segmented_rows_update_indirect*), the same two forms over the same
// element loops; only their write-back reads `order`.
//
// What the nine keyed kernels and six launchers share exists once.  Device (rsv_k2.h): build_lut, the frames
// wave_frame / wg_frame (the Wave over the workgroup's LDS and its winner table), read_segment (an update's
// segment header and its skip rules), slot_source (the stateless slot rule) and merge_pick.  Host (below):
// SeedWords, wave_grid / wg_grid, tables_fit_u32, with_global_table (gt_acquire .. gt_release around a
// launch), with_key / with_granule (each kernel launch is written once, in a generic lambda), launch_wg
// (the stateless workgroup form of both families), launch_update and merge_grid.
#include <algorithm>
#include <cstdlib>
#include <mutex>

#include "rsv_internal.h"
#include "rsv_k2.h"
#include "rsv_k2_indexed.h"

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

// ---- the launch plan: what every launcher below shares -------------------------------------------
// the Philox key words of a launch
struct SeedWords {
    uint32_t k0, k1;
    explicit SeedWords(const DrawParams& dp) : k0((uint32_t)dp.seed), k1((uint32_t)(dp.seed >> 32)) {}
};

// The wave form's grid over n streams or segments: up to 128 four-wave workgroups per CU over the launch
// (C3: 8 streams per wave): tools/micro_k2 G (r03ai) 1.78 ms at 4096 workgroups, 1.71 at 16384, 1.65 at
// 32768, 1.66-1.68 at 65536, 1.84 at one stream per wave (262144: every workgroup rebuilds the threshold table)
unsigned wave_grid(int64_t n) {
    return (unsigned)std::min<uint64_t>(((uint64_t)n + kWaves - 1) / kWaves, 256ull * 128);
}

// the workgroup form's grid: as many workgroups as the CUs hold at once, twice over (taken grid-stride)
unsigned wg_grid(int64_t n, size_t lds) {
    const uint64_t per_cu = std::max<uint64_t>(1, k2::kLdsMax / lds);
    return (unsigned)std::min<uint64_t>((uint64_t)n, 256ull * per_cu * 2);
}

// every index fits 32 bits when the streams together span < 2^32 elements: u32 tables (one host read)
hipError_t tables_fit_u32(const int64_t* offsets, int64_t S, hipStream_t st, bool* fit) {
    int64_t ends[2] = {0, 0};
    RSV_HIP_RET(hipMemcpyAsync(&ends[0], offsets, 8, hipMemcpyDeviceToHost, st));
    RSV_HIP_RET(hipMemcpyAsync(&ends[1], offsets + S, 8, hipMemcpyDeviceToHost, st));
    RSV_HIP_RET(hipStreamSynchronize(st));
    *fit = ends[1] - ends[0] < ((int64_t)1 << 32);
    return hipSuccess;
}

// the global-table path: launch(table) under g_gt_mu between gt_acquire and gt_release; the launch's error
template <typename Launch>
hipError_t with_global_table(size_t bytes, hipStream_t st, Launch launch) {
    int dev = 0;
    RSV_HIP_RET(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lk(g_gt_mu);
    void* gt = nullptr;
    bool priv = false;
    RSV_HIP_RET(gt_acquire(dev, bytes, st, &gt, &priv));
    launch(gt);
    const hipError_t e = hipGetLastError();
    gt_release(dev, st, priv, gt);
    return e;
}

// f(KeyT{}) for the key width, f(G{}) for the rows' granule: each kernel launch below is written once
template <typename F>
hipError_t with_key(int key_width, F f) {
    return key_width == 8 ? f(int64_t{}) : f(int32_t{});
}
template <typename F>
hipError_t with_granule(bool vec16, F f) {
    return vec16 ? f(uint4{}) : f(uint64_t{});
}
// 16-byte granules where every row of every buffer sits on a 16-byte boundary, else 8-byte ones
bool rows_vec16(int key_width, const void* a, const void* b) {
    return key_width % 16 == 0 && (((uintptr_t)a | (uintptr_t)b) & 15) == 0;
}

// The stateless workgroup form (k >= kWGMinK) of either kernel family: go(GT, grid, lds, table) launches
// the kernel's <TabT, GT> instantiation -- the table in LDS while it fits, else in the global scratch.
template <typename TabT, typename Go>
hipError_t launch_wg_tab(int64_t S, uint32_t k, hipStream_t st, Go go) {
    const size_t lds = k2::lds_bytes_wg(k, sizeof(TabT), false);
    if (lds <= k2::kLdsMax) {
        go(std::false_type{}, wg_grid(S, lds), lds, (TabT*)nullptr);
        return hipGetLastError();
    }
    const unsigned grid = (unsigned)std::min<uint64_t>((uint64_t)S, 512);
    return with_global_table((size_t)grid * k * sizeof(TabT), st, [&](void* gt) {
        go(std::true_type{}, grid, k2::lds_bytes_wg(k, sizeof(TabT), true), (TabT*)gt);
    });
}
template <typename Go>
hipError_t launch_wg(const int64_t* offsets, int64_t S, uint32_t k, hipStream_t st, Go go) {
    bool t32 = false;
    RSV_HIP_RET(tables_fit_u32(offsets, S, st, &t32));
    return t32 ? launch_wg_tab<uint32_t>(S, k, st, go) : launch_wg_tab<unsigned long long>(S, k, st, go);
}

// the largest k whose 64-bit winner table fits one workgroup's LDS beside the waves' rings
static_assert(k2::lds_bytes_wg(kSegSampleStateMaxK, 8, false) <= k2::kLdsMax &&
                  k2::lds_bytes_wg(kSegSampleStateMaxK + 1, 8, false) > k2::kLdsMax,
              "kSegSampleStateMaxK is the LDS limit of k2_segmented_update_wg");

// The resumed launch of either family: wg(grid, lds) launches the workgroup form (k >= kWGMinK, one workgroup
// per segment, 64-bit table in LDS), wave(grid, lds) the wave form.
template <typename Wg, typename Wave>
hipError_t launch_update(int64_t B, uint32_t k, Wg wg, Wave wave) {
    if (k >= k2::kWGMinK) {
        const size_t lds = k2::lds_bytes_wg(k, 8, false);
        wg(wg_grid(B, lds), lds);
    } else {
        wave(wave_grid(B), k2::lds_bytes(k));
    }
    return hipGetLastError();
}

// one thread per (row, slot) entry, 256 a workgroup
hipError_t merge_grid(int64_t num_states, uint32_t k, unsigned* grid) {
    const uint64_t blocks = ((uint64_t)num_states * k + 255) / 256;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    *grid = (unsigned)blocks;
    return hipSuccess;
}
}  // namespace

hipError_t launch_segmented(const void* keys, int key_width, const int64_t* offsets, int64_t S, uint32_t k,
                            const DrawParams& dp, void* out, int64_t* counts, hipStream_t st) {
    if (S <= 0) return hipSuccess;
    const uint32_t fifo_cap = env_fifo_cap();
    const SeedWords sw(dp);
    return with_key(key_width, [&](auto key) {
        using KeyT = decltype(key);
        if (k >= k2::kWGMinK)  // one workgroup per stream
            return launch_wg(offsets, S, k, st, [&](auto gt, unsigned grid, size_t lds, auto* tab) {
                using TabT = std::remove_pointer_t<decltype(tab)>;
                hipLaunchKernelGGL((k2_segmented_wg<KeyT, TabT, decltype(gt)::value>), dim3(grid), dim3(64 * kWavesWG),
                                   lds, st, (const KeyT*)keys, offsets, S, k, sw.k0, sw.k1, dp.stream, (KeyT*)out,
                                   counts, fifo_cap, tab);
            });
        hipLaunchKernelGGL(k2_segmented<KeyT>, dim3(wave_grid(S)), dim3(64 * kWaves), k2::lds_bytes(k), st,
                           (const KeyT*)keys, offsets, S, k, sw.k0, sw.k1, dp.stream, (KeyT*)out, counts, fifo_cap);
        return hipGetLastError();
    });
}

hipError_t launch_segmented_update(const void* keys, int key_width, const int64_t* offsets, const int64_t* stream_ids,
                                   const int64_t* bases, int64_t num_segments, int64_t num_states, uint32_t k,
                                   const DrawParams& dp, void* state_keys, int64_t* state_idx, int64_t* state_next,
                                   hipStream_t st) {
    if (num_segments <= 0 || num_states <= 0) return hipSuccess;
    if (k > kSegSampleStateMaxK) return hipErrorInvalidValue;
    const SeedWords sw(dp);
    const uint32_t fifo_cap = env_fifo_cap();
    return with_key(key_width, [&](auto key) {
        using KeyT = decltype(key);
        auto launch = [&](auto kernel, int waves) {
            return [&, kernel, waves](unsigned grid, size_t lds) {
                hipLaunchKernelGGL(kernel, dim3(grid), dim3(64 * waves), lds, st, (const KeyT*)keys, offsets, stream_ids,
                                   bases, num_segments, num_states, k, sw.k0, sw.k1, dp.stream, (KeyT*)state_keys,
                                   state_idx, state_next, fifo_cap);
            };
        };
        return launch_update(num_segments, k, launch(k2_segmented_update_wg<KeyT>, kWavesWG),
                             launch(k2_segmented_update<KeyT>, kWaves));
    });
}

hipError_t launch_segmented_update_indirect(const void* keys, int64_t n_keys, const int32_t* order, int key_width,
                                            const int64_t* offsets, const int64_t* stream_ids, const int64_t* bases,
                                            int64_t num_segments, int64_t num_states, uint32_t k, const DrawParams& dp,
                                            void* state_keys, int64_t* state_idx, int64_t* state_next,
                                            hipStream_t st) {
    if (num_segments <= 0 || num_states <= 0) return hipSuccess;
    if (k > kSegSampleStateMaxK) return hipErrorInvalidValue;
    const SeedWords sw(dp);
    const uint32_t fifo_cap = env_fifo_cap();
    return with_key(key_width, [&](auto key) {
        using KeyT = decltype(key);
        auto launch = [&](auto kernel, int waves) {
            return [&, kernel, waves](unsigned grid, size_t lds) {
                hipLaunchKernelGGL(kernel, dim3(grid), dim3(64 * waves), lds, st, (const KeyT*)keys, n_keys, order,
                                   offsets, stream_ids, bases, num_segments, num_states, k, sw.k0, sw.k1, dp.stream,
                                   (KeyT*)state_keys, state_idx, state_next, fifo_cap);
            };
        };
        return launch_update(num_segments, k, launch(k2_segmented_update_indirect_wg<KeyT>, kWavesWG),
                             launch(k2_segmented_update_indirect<KeyT>, kWaves));
    });
}

hipError_t launch_segmented_merge(const void* part_keys, int key_width, const int64_t* part_idx,
                                  const int64_t* part_next, int32_t parts, int64_t num_states, uint32_t k,
                                  void* state_keys, int64_t* state_idx, int64_t* state_next, hipStream_t st) {
    if (parts <= 0 || num_states <= 0) return hipSuccess;
    unsigned grid = 0;
    RSV_HIP_RET(merge_grid(num_states, k, &grid));
    return with_key(key_width, [&](auto key) {
        using KeyT = decltype(key);
        hipLaunchKernelGGL(k2_segmented_merge<KeyT>, dim3(grid), dim3(256), 0, st, (const KeyT*)part_keys, part_idx,
                           part_next, parts, num_states, k, (KeyT*)state_keys, state_idx, state_next);
        return hipGetLastError();
    });
}

// ---- byte keys (rows): C granules of sizeof(G) bytes a row ---------------------------------------
hipError_t launch_segmented_rows(const void* rows_, int key_width, const int64_t* offsets, int64_t S, uint32_t k,
                                 const DrawParams& dp, void* out_rows, int64_t* counts, hipStream_t st) {
    if (S <= 0) return hipSuccess;
    const unsigned char* rows = (const unsigned char*)rows_;
    unsigned char* out = (unsigned char*)out_rows;
    return with_granule(rows_vec16(key_width, rows, out), [&](auto granule) {
        using G = decltype(granule);
        const uint32_t C = (uint32_t)key_width / (uint32_t)sizeof(G);
        const uint32_t fifo_cap = env_fifo_cap();
        const SeedWords sw(dp);
        if (k >= k2::kWGMinK)  // one workgroup per stream; u32 tables by the rule of launch_segmented
            return launch_wg(offsets, S, k, st, [&](auto gt, unsigned grid, size_t lds, auto* tab) {
                using TabT = std::remove_pointer_t<decltype(tab)>;
                hipLaunchKernelGGL((k2_segmented_rows_wg<G, TabT, decltype(gt)::value>), dim3(grid),
                                   dim3(64 * kWavesWG), lds, st, rows, offsets, S, k, C, sw.k0, sw.k1, dp.stream, out,
                                   counts, fifo_cap, tab);
            });
        // one (slot, granule) pair per lane: the gather is deferred past the next stream's draws (C3 with UUID
        // rows: 1.79 ms against 1.85 ms plain, profiles/segmented_rows/bench.json).  RSV_K2_ROWS_DEFER=0 (read
        // once per process) keeps the plain gather, for that A/B in tools/bench_segmented_rows.py.
        static const bool defer = [] {
            const char* e = std::getenv("RSV_K2_ROWS_DEFER");
            return !e || std::atoi(e) != 0;
        }();
        auto launch = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, dim3(wave_grid(S)), dim3(64 * kWaves), k2::lds_bytes(k), st, rows, offsets, S, k,
                               C, sw.k0, sw.k1, dp.stream, out, counts, fifo_cap);
            return hipGetLastError();
        };
        return defer && (uint64_t)k * C <= 64 ? launch(k2_segmented_rows<G, true>) : launch(k2_segmented_rows<G, false>);
    });
}

hipError_t launch_segmented_rows_update(const void* rows_, int key_width, const int64_t* offsets,
                                        const int64_t* stream_ids, const int64_t* bases, int64_t num_segments,
                                        int64_t num_states, uint32_t k, const DrawParams& dp, void* state_rows_,
                                        int64_t* state_idx, int64_t* state_next, hipStream_t st) {
    if (num_segments <= 0 || num_states <= 0) return hipSuccess;
    if (k > kSegSampleStateMaxK) return hipErrorInvalidValue;
    const unsigned char* rows = (const unsigned char*)rows_;
    unsigned char* state_rows = (unsigned char*)state_rows_;
    return with_granule(rows_vec16(key_width, rows, state_rows), [&](auto granule) {
        using G = decltype(granule);
        const uint32_t C = (uint32_t)key_width / (uint32_t)sizeof(G);
        const SeedWords sw(dp);
        const uint32_t fifo_cap = env_fifo_cap();
        auto launch = [&](auto kernel, int waves) {
            return [&, kernel, waves](unsigned grid, size_t lds) {
                hipLaunchKernelGGL(kernel, dim3(grid), dim3(64 * waves), lds, st, rows, offsets, stream_ids, bases,
                                   num_segments, num_states, k, C, sw.k0, sw.k1, dp.stream, state_rows, state_idx,
                                   state_next, fifo_cap);
            };
        };
        return launch_update(num_segments, k, launch(k2_segmented_rows_update_wg<G>, kWavesWG),
                             launch(k2_segmented_rows_update<G>, kWaves));
    });
}

hipError_t launch_segmented_rows_update_indirect(const void* rows_, int64_t n_rows, const int32_t* order, int key_width,
                                                 const int64_t* offsets, const int64_t* stream_ids,
                                                 const int64_t* bases, int64_t num_segments, int64_t num_states,
                                                 uint32_t k, const DrawParams& dp, void* state_rows_,
                                                 int64_t* state_idx, int64_t* state_next, hipStream_t st) {
    if (num_segments <= 0 || num_states <= 0) return hipSuccess;
    if (k > kSegSampleStateMaxK) return hipErrorInvalidValue;
    const unsigned char* rows = (const unsigned char*)rows_;
    unsigned char* state_rows = (unsigned char*)state_rows_;
    return with_granule(rows_vec16(key_width, rows, state_rows), [&](auto granule) {
        using G = decltype(granule);
        const uint32_t C = (uint32_t)key_width / (uint32_t)sizeof(G);
        const SeedWords sw(dp);
        const uint32_t fifo_cap = env_fifo_cap();
        auto launch = [&](auto kernel, int waves) {
            return [&, kernel, waves](unsigned grid, size_t lds) {
                hipLaunchKernelGGL(kernel, dim3(grid), dim3(64 * waves), lds, st, rows, n_rows, order, offsets,
                                   stream_ids, bases, num_segments, num_states, k, C, sw.k0, sw.k1, dp.stream,
                                   state_rows, state_idx, state_next, fifo_cap);
            };
        };
        return launch_update(num_segments, k, launch(k2_segmented_rows_update_indirect_wg<G>, kWavesWG),
                             launch(k2_segmented_rows_update_indirect<G>, kWaves));
    });
}

hipError_t launch_segmented_rows_merge(const void* part_rows, int key_width, const int64_t* part_idx,
                                       const int64_t* part_next, int32_t parts, int64_t num_states, uint32_t k,
                                       void* state_rows, int64_t* state_idx, int64_t* state_next, hipStream_t st) {
    if (parts <= 0 || num_states <= 0) return hipSuccess;
    unsigned grid = 0;
    RSV_HIP_RET(merge_grid(num_states, k, &grid));
    return with_granule(rows_vec16(key_width, part_rows, state_rows), [&](auto granule) {
        using G = decltype(granule);
        hipLaunchKernelGGL(k2_segmented_rows_merge<G>, dim3(grid), dim3(256), 0, st, (const unsigned char*)part_rows,
                           part_idx, part_next, parts, num_states, k, (uint32_t)key_width / (uint32_t)sizeof(G),
                           (unsigned char*)state_rows, state_idx, state_next);
        return hipGetLastError();
    });
}

// ---- keyless: lengths in, indices out ------------------------------------------------------------
namespace {
// The split length of the stateless keyless launch (rsv_indexed.hip), in indices.  RSV_K2_SPLIT_LEN (read once per
// process) overrides it, rounded down to a multiple of 1024; 0 disables the split.  2^18 was the fastest of 2^18,
// 2^20 and 2^22 on 2^16 streams x 4096 beside one stream of 2^32 indices (k = 64: 1.19 / 1.82 / 5.37 ms, unsplit
// 2630 ms; k = 1024: 1.68 / 1.69 / 1.74 ms, unsplit 426 ms), and at C3's shape, where no stream is split, the
// launch stays inside the run-to-run spread of the launch without it (profiles/segmented_indexed/bench.json).
constexpr int64_t kSplitLenDefault = 1ll << 18;
constexpr uint32_t kSplitListCap = 1024;  // streams whose pieces a launch records; the others stay whole
int64_t env_split_len() {
    static const int64_t split_len = [] {
        const char* e = std::getenv("RSV_K2_SPLIT_LEN");
        const long long v = e ? std::atoll(e) : (long long)kSplitLenDefault;
        return v < 1024 ? (int64_t)0 : (int64_t)(v & ~1023ll);
    }();
    return split_len;
}

// the second kernel's grid: what the device holds at once (8 waves a SIMD, one workgroup's LDS), whatever S is
unsigned resident_grid(size_t lds, int waves) {
    const uint64_t by_waves = 8 * 4 / (uint64_t)waves;
    return (unsigned)(256 * std::max<uint64_t>(1, std::min<uint64_t>(by_waves, k2::kLdsMax / lds)));
}
}  // namespace

hipError_t launch_segmented_indexed(const int64_t* offsets, int64_t S, uint32_t k, const DrawParams& dp,
                                    int64_t* out_idx, int64_t* counts, hipStream_t st) {
    if (S <= 0) return hipSuccess;
    const uint32_t fifo_cap = env_fifo_cap();
    const SeedWords sw(dp);
    const bool wg = k >= k2::kWGMinK;
    // the list of the split form: stream-ordered memory, its count zeroed ahead of the first kernel; the
    // global-table form (no u32 table of k entries fits LDS) stays unsplit
    SplitList sl{nullptr, nullptr, 0, 0};
    void* list = nullptr;
    if (env_split_len() > 0 && (!wg || k2::lds_bytes_wg(k, 4, false) <= k2::kLdsMax)) {
        RSV_HIP_RET(hipMallocAsync(&list, 16 + (size_t)kSplitListCap * 16, st));
        sl = SplitList{(unsigned long long*)list, (int64_t*)((unsigned char*)list + 16), kSplitListCap, env_split_len()};
    }
    hipError_t e = list ? hipMemsetAsync(list, 0, 16, st) : hipSuccess;
    if (e == hipSuccess && wg) {  // one workgroup per stream, and per piece
        e = launch_wg(offsets, S, k, st, [&](auto gt, unsigned grid, size_t lds, auto* tab) {
            using TabT = std::remove_pointer_t<decltype(tab)>;
            hipLaunchKernelGGL((k2_indexed_wg<TabT, decltype(gt)::value>), dim3(grid), dim3(64 * kWavesWG), lds, st,
                               offsets, S, k, sw.k0, sw.k1, dp.stream, out_idx, counts, fifo_cap, tab, sl);
            if constexpr (!decltype(gt)::value)
                if (sl.C > 0)
                    hipLaunchKernelGGL(k2_indexed_pieces_wg<TabT>, dim3(resident_grid(lds, kWavesWG)),
                                       dim3(64 * kWavesWG), lds, st, k, sw.k0, sw.k1, dp.stream, out_idx, fifo_cap, sl);
        });
    } else if (e == hipSuccess) {
        const size_t lds = k2::lds_bytes(k);
        hipLaunchKernelGGL(k2_indexed, dim3(wave_grid(S)), dim3(64 * kWaves), lds, st, offsets, S, k, sw.k0, sw.k1,
                           dp.stream, out_idx, counts, fifo_cap, sl);
        if (sl.C > 0)
            hipLaunchKernelGGL(k2_indexed_pieces, dim3(resident_grid(lds, kWaves)), dim3(64 * kWaves), lds, st, k, sw.k0,
                               sw.k1, dp.stream, out_idx, fifo_cap, sl);
        e = hipGetLastError();
    }
    if (list) {
        const hipError_t f = hipFreeAsync(list, st);
        if (e == hipSuccess) e = f;
    }
    return e;
}

hipError_t launch_segmented_indexed_update(const int64_t* offsets, const int64_t* stream_ids, const int64_t* bases,
                                           int64_t num_segments, int64_t num_states, uint32_t k, const DrawParams& dp,
                                           int64_t* state_idx, int64_t* state_next, int64_t* hits, int64_t* hit_counts,
                                           hipStream_t st) {
    if (num_segments <= 0 || num_states <= 0) return hipSuccess;
    if (k > kSegSampleStateMaxK) return hipErrorInvalidValue;
    const SeedWords sw(dp);
    const uint32_t fifo_cap = env_fifo_cap();
    auto launch = [&](auto kernel, int waves) {
        return [&, kernel, waves](unsigned grid, size_t lds) {
            hipLaunchKernelGGL(kernel, dim3(grid), dim3(64 * waves), lds, st, offsets, stream_ids, bases, num_segments,
                               num_states, k, sw.k0, sw.k1, dp.stream, state_idx, state_next, hits, hit_counts, fifo_cap);
        };
    };
    return launch_update(num_segments, k, launch(k2_indexed_update_wg, kWavesWG), launch(k2_indexed_update, kWaves));
}

hipError_t launch_segmented_indexed_merge(const int64_t* part_idx, const int64_t* part_next, int32_t parts,
                                          int64_t num_states, uint32_t k, int64_t* state_idx, int64_t* state_next,
                                          int32_t* src, hipStream_t st) {
    if (parts <= 0 || num_states <= 0) return hipSuccess;
    unsigned grid = 0;
    RSV_HIP_RET(merge_grid(num_states, k, &grid));
    hipLaunchKernelGGL(k2_indexed_merge, dim3(grid), dim3(256), 0, st, part_idx, part_next, parts, num_states, k,
                       state_idx, state_next, src);
    return hipGetLastError();
}

}  // namespace rsv
