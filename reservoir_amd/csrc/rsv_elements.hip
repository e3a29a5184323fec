// rsv_elements.hip -- gfx950 kernels for the element sampler (Sampler.apply, Sampler.scala:196-332)
// reformulated as data-parallel Algorithm R with counter-based draws (format R2, rsv_device.h).
//
//   K1  k1_last_writer   single stream: per-slot last writer (max index) of an index range
//   --  resolve          fill phase + gather of the winning keys into the reservoir
//   K1' replay_events    the reference's Algorithm-L eviction events -> per-slot last writer
//   --  merge_slots      multi-GPU combine of exported partial reservoirs (last writer wins)
//
// None of these kernels streams the key array: a draw depends only on (seed, stream, index), so
// only the k winning keys are ever read (DESIGN.md "Roofline").
#include <algorithm>

#include "rsv_device.h"
#include "rsv_internal.h"
#include "rsv_scan.h"

namespace rsv {

namespace {

constexpr int kBlock = 256;

// K1: grid-stride over level-0 blocks (16 indices each), two per lane per iteration; a pair with a
// zero byte is appended at once to the wave's LDS queue -- with its 32-bit zero-byte fold, so a
// sparse-region resolve needs no level-0 recompute -- and after every half window of 6 iterations
// the level-1 draws run 64 at a time, all lanes busy (rsv_scan.h k1_body_q).  Hits (k ln(n/k) of
// them) go straight to global atomicMax on the k-slot winner table: 14k atomics per 1e9 indices at k = 1024.
constexpr int kK1Unroll = 2;  // level-0 blocks per lane per iteration (two Philox chains in flight)

// ~20 four-wave workgroups per CU (6 resident: .sgpr_count 104 then, 106 now): tools/micro_k1o r03ae/r03af, 1e9
// draws, 12-iteration windows: 85.0-85.5 us at 5086 workgroups (2 whole windows per wave) vs
// 87.5-89 us at 3072, 3390 (3 windows), 4096, 6144, 7629 and 10172 (1 window)
constexpr unsigned kK1Grid = 256 * 20;

// per-wave LDS of k1_body_q: pair queue (< 64 waiting + half a window of appends), the per-
// candidate queue, the append's `top` word.  12 iterations per window: tools/micro_k1o (r05k, 1e9 indices, grid 5086)
// 83.1-83.6 us vs 83.4-83.8 for 8 and 84.7-84.8 for 16, and 84.9-85.8 for the round-4 body
// (k1_body_p: window bits pushed in ballot rounds, tools/k1_dev_bodies.h), winners identical.
constexpr int kK1Win = 12;
struct K1Lds {
    uint64_t q[kBlock / 64][k1q_cap<kK1Win>()];
    uint64_t cq[kBlock / 64][kQueue];
    uint32_t top[kBlock / 64];  // per wave: the byte address of its next free queue entry (k1_body_q TOP)
};

// One kernel per form (FAST: rsv_scan.h): the host picks the instantiation from K1Launch::flags
// (k1_fast_form), so no kernel tests the flag.  With both bodies behind one launch-uniform branch the
// kernel spilled 29 SGPRs to VGPR lanes, 8-9 lane moves in every unit of the steady loop; alone the
// FAST body spills none and the general body 5 (profiles/k1_forms/resources.tsv).
template <bool FAST>
__global__ __launch_bounds__(kBlock) void k1_last_writer(DrawKey dk, uint32_t k, uint64_t lo,
                                                         uint64_t hi, uint64_t g_begin,
                                                         uint64_t n_groups,
                                                         unsigned long long* __restrict__ win, K1Launch P) {
    __shared__ K1Lds L;
    const int w = threadIdx.x >> 6;
    k1_body_q<kK1Win, FAST, kBlock, true>(dk, k, lo, hi, g_begin, n_groups, win, L.q[w], L.cq[w], P, nullptr,
                                          &L.top[w]);
}

// ---- the slot rule ----------------------------------------------------------------------------
// What the batch [base, base + n) does to slot j, given the batch's last writer wi = win[j] (0: none).
// The first case that holds:
//   winner  wi != 0: the last eviction into slot j in this batch (Sampler.scala:243-246) -- the slot
//           takes element wi, and the caller clears win[j]
//   fill    base <= j < base + n: the fill phase (Sampler.scala:253-255) -- the slot takes element j
//   empty   fresh (the first batch of a handle whose slots were never initialised): idx -1, key zero
//   keep    the slot keeps what it holds
// The rule calls exactly one of
//   take(off, idx, winner)  winner, fill: the element at offset `off` of the batch, the slot's new slot_idx
//   empty(idx)              the empty slot's slot_idx
//   keep()
// so a form's code for a case stands in the branch of that case, as when each kernel spelled the
// cases out.  Two things kept k1_resolve_publish<long> at its 51 VGPRs: the rule calls back instead of
// returning the case as a value (53), and callbacks that only store capture by value -- behind a
// by-reference closure the pointers lose __restrict__, which keys and indices of one type need (57).
// Every resolve form below goes through this function; none spells the cases out again.
template <typename Take, typename Empty, typename Keep>
__device__ __forceinline__ void slot_rule(int64_t j, unsigned long long wi, int64_t base, int64_t n, int fresh,
                                          Take&& take, Empty&& empty, Keep&& keep) {
    if (wi) take((int64_t)wi - base, (int64_t)wi, true);
    else if (j >= base && j < base + n) take(j - base, j, false);
    else if (fresh) empty((int64_t)-1);
    else keep();
}

// The registers-first resolve + publication by one 256-thread workgroup, R slots per lane (k <= 256 R):
// all R winner loads are issued before any key load, and every load before any store; then the first
// m final slot keys go to coherent host memory `dst` and `gen` to the host flag.  kAgentWin: win[] was
// written by other workgroups of this launch (k1_resolve_publish), so it is read with agent-scope
// atomic loads -- a plain load there may be served from a stale line.
template <typename KeyT, int R, bool kAgentWin>
__device__ __forceinline__ void resolve_registers_first(const KeyT* __restrict__ keys, int64_t base, int64_t n,
                                                        uint32_t k, unsigned long long* __restrict__ win,
                                                        KeyT* __restrict__ slot_key, int64_t* __restrict__ slot_idx,
                                                        int fresh, int64_t m, KeyT* dst, uint32_t* flag, uint32_t gen) {
    unsigned long long wi[R];
    KeyT v[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const uint32_t j = threadIdx.x + r * kBlock;
        if (j >= k) wi[r] = 0ull;
        else if (kAgentWin) wi[r] = __hip_atomic_load(&win[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else wi[r] = win[j];
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int64_t j = threadIdx.x + r * kBlock;
        if (j >= k) continue;
        KeyT x;
        slot_rule(
            j, wi[r], base, n, fresh, [&](int64_t off, int64_t, bool) { x = keys[off]; }, [&](int64_t) { x = 0; },
            [&] { x = slot_key[j]; });
        v[r] = x;
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int64_t j = threadIdx.x + r * kBlock;
        if (j >= k) continue;
        const KeyT x = v[r];
        slot_rule(
            j, wi[r], base, n, fresh,
            [=](int64_t, int64_t idx, bool winner) {
                slot_key[j] = x;
                slot_idx[j] = idx;
                if (winner) win[j] = 0;
            },
            [=](int64_t idx) {
                slot_key[j] = 0;
                slot_idx[j] = idx;
            },
            [] {});
        if (j < m) dst[j] = x;
    }
    publish_flag(flag, gen);
}

// K1 + resolve_publish in one dispatch (single-launch batches, k <= kK1FusedMaxK): every
// workgroup takes a ticket after its winner atomics; the last one -- which then sees all of them --
// runs the resolve over the k slots (all loads of a lane issued before any store) and publishes
// the reservoir into coherent host memory, then re-arms the ticket.  Saves the kernel boundary
// and the resolve dispatch of the two-kernel form.
constexpr uint32_t kK1FusedMaxK = 8 * kBlock;

// What the tail takes.  It is the kernel's FIRST argument and the kernel never names it: the tail reads it
// from the kernarg segment (offset 0) behind K1, through an address the compiler cannot trace to the segment
// (it waits in the LDS meanwhile).  As plain arguments these 20 SGPRs were loaded at entry and held through
// K1, which has none to spare: the FAST form spilled 10 of them to VGPR lanes (the K1-only kernel none); the
// segment's address or gridDim.x held through K1 would be spilled the same way, so the grid is here too.
template <typename KeyT>
struct K1Tail {
    uint32_t* ticket;
    const KeyT* keys;
    int64_t base, n;
    KeyT* slot_key;
    int64_t* slot_idx;
    int64_t m;
    KeyT* dst;
    uint32_t* flag;
    uint32_t gen;
    int fresh;
    uint32_t grid;  // workgroups of the launch
};

template <typename KeyT, bool FAST>
__global__ __launch_bounds__(kBlock) void k1_resolve_publish(K1Tail<KeyT>, DrawKey dk, uint32_t k, uint64_t lo,
                                                             uint64_t hi, uint64_t g_begin, uint64_t n_groups,
                                                             unsigned long long* __restrict__ win, K1Launch P) {
    __shared__ K1Lds L;
    __shared__ uint32_t last;
    __shared__ uint64_t tail_at;
    const int w = threadIdx.x >> 6;
    // every wave stores the same address and reads it back behind its own store
    tail_at = (uint64_t)__builtin_amdgcn_kernarg_segment_ptr();
    k1_body_q<kK1Win, FAST, kBlock, true>(dk, k, lo, hi, g_begin, n_groups, win, L.q[w], L.cq[w], P, nullptr,
                                          &L.top[w]);
    asm volatile("" ::: "memory");
    const uint64_t at = tail_at;
    const uint64_t args = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(at >> 32)) << 32) |
                          (uint32_t)__builtin_amdgcn_readfirstlane((int)at);
    const auto* T = (const __attribute__((address_space(4))) K1Tail<KeyT>*)args;  // constant memory: scalar loads
    // This wave's winner atomics are performed once vmcnt drains: on gfx942/gfx950 a global atomic
    // without return still counts in vmcnt until the memory system acknowledges it (there is no
    // separate vscnt), and an agent-scope atomic is performed at the agent's coherence point (the
    // sc1 atomic path, LLVM AMDGPUUsage "Memory Model GFX942": agent-scope atomics bypass the
    // non-coherent per-XCD L2 state), where the last workgroup's agent-scope loads below read.
    // K1 makes no plain global stores, so there are no dirty L2 lines a release would have to
    // write back.  Measured alternatives: an agent-scope release/acquire fence per wave (a
    // buffer_wbl2 per wave + buffer_inv per workgroup) took the launch from 112 to 211 us at C2.
    // Only the last workgroup acquires (one L2 invalidate) before it reads the winners; the
    // parity tests (test_fused_k1_resolve_publish, the full-size C2 check) exercise this path.
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t prev = __hip_atomic_fetch_add(T->ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        last = prev == T->grid - 1;
        if (last) __hip_atomic_store(T->ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    if (!last) return;  // workgroup-uniform
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    resolve_registers_first<KeyT, kK1FusedMaxK / kBlock, true>(T->keys, T->base, T->n, k, win, T->slot_key, T->slot_idx,
                                                               T->fresh, T->m, T->dst, T->flag, T->gen);
}

// The batch's resolve of 4- / 8-byte keys: the slot rule per slot j, the keys gathered from the batch.
// kPublish: one workgroup (reservoirs of <= 8192 keys) that also writes the first m final slot keys
// straight into coherent host memory and publishes `gen` in the host flag with a system-scope release
// (as publish_kernel); else one slot per thread of a k-wide grid, with m / dst / flag / gen unused.
// The two forms have different launch bounds, so the publication is a compile-time case: the
// one-workgroup form is what bench.py's two-dispatch step runs.  slot_idx is null only for
// rsv_replay_events (a caller's bare reservoir, never published).
// j + stride stays below 2^32: k < 2^31, and no grid is wider than k rounded up to the block.
template <typename KeyT, bool kPublish>
__global__ __launch_bounds__(kPublish ? 1024 : kBlock) void resolve_kernel(const KeyT* __restrict__ keys, int64_t base,
                                                                         int64_t n, uint32_t k,
                                                                         unsigned long long* __restrict__ win,
                                                                         KeyT* __restrict__ slot_key,
                                                                         int64_t* __restrict__ slot_idx, int fresh,
                                                                         int64_t m, KeyT* dst, uint32_t* flag,
                                                                         uint32_t gen) {
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < k; j += stride) {
        KeyT v = 0;
        slot_rule(
            j, win[j], base, n, fresh,
            [&](int64_t off, int64_t idx, bool winner) {
                slot_key[j] = v = keys[off];
                if (kPublish || slot_idx) slot_idx[j] = idx;
                if (winner) win[j] = 0;
            },
            [=](int64_t idx) {
                slot_key[j] = 0;
                if (kPublish || slot_idx) slot_idx[j] = idx;
            },
            [&] {
                if (kPublish) v = slot_key[j];
            });
        if (kPublish && (int64_t)j < m) dst[j] = v;
    }
    if (kPublish) publish_flag(flag, gen);
}

// The publishing resolve as one 256-thread workgroup (k <= 256 R).  For a resolve forked onto a second
// stream beside the next batch's K1 (rsv_set_resolve_stream): 4 waves fit beside K1's six workgroups on
// a CU, where the 1024-thread form's 16 waves displace one of them (K1's first-generation schedule then
// ends late).
template <typename KeyT, int R>
__global__ __launch_bounds__(kBlock) void resolve_publish_small_kernel(const KeyT* __restrict__ keys, int64_t base,
                                                                       int64_t n, uint32_t k,
                                                                       unsigned long long* __restrict__ win,
                                                                       KeyT* __restrict__ slot_key,
                                                                       int64_t* __restrict__ slot_idx, int fresh,
                                                                       int64_t m, KeyT* dst, uint32_t* flag, uint32_t gen) {
    resolve_registers_first<KeyT, R, false>(keys, base, n, k, win, slot_key, slot_idx, fresh, m, dst, flag, gen);
}

__global__ __launch_bounds__(kBlock) void replay_kernel(const int64_t* __restrict__ ev_pos,
                                                        const int32_t* __restrict__ ev_slot,
                                                        int64_t n_events, uint32_t k,
                                                        unsigned long long* __restrict__ win) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_events) return;
    const int32_t s = ev_slot[e];
    const int64_t p = ev_pos[e];
    if (s >= 0 && (uint32_t)s < k && p >= 2) atomicMax(&win[s], (unsigned long long)(p - 1));
}

__global__ __launch_bounds__(kBlock) void export_draws_kernel(DrawKey dk, uint64_t i0, int64_t n,
                                                              uint64_t* __restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const uint64_t i = i0 + (uint64_t)t;
    const u32x4 w = level0(dk, i >> 4);
    out[t] = exact_j(dk, i, level0_byte(w, (uint32_t)(i & 15)));
}

// ---- the merge rule (multi-GPU combine of exported reservoirs) ---------------------------------
// Where part p's index and key for slot j live -- index(p, j), and take(p, j, slot_key) moves the key
// into the slot.  Strided arrays (rsv_merge: idx_parts[p][part_len], key_parts[p][part_len]):
template <typename KeyT>
struct StridedParts {
    using Key = KeyT;
    const int64_t* idx;
    const KeyT* key;
    int64_t part_len;
    __device__ int64_t index(int32_t p, uint32_t j) const { return idx[(int64_t)p * part_len + j]; }
    __device__ void take(int32_t p, uint32_t j, KeyT* slot_key) const { slot_key[j] = key[(int64_t)p * part_len + j]; }
};

// packed multi-GPU rows, `stride` words apart: [slot_idx(k) | keys widened to int64 (k)]
template <typename KeyT>
struct PackedRows {
    using Key = KeyT;
    const int64_t* rows;
    int64_t stride;
    uint32_t k;
    __device__ int64_t index(int32_t p, uint32_t j) const { return rows[(int64_t)p * stride + j]; }
    __device__ void take(int32_t p, uint32_t j, KeyT* slot_key) const {
        slot_key[j] = (KeyT)rows[(int64_t)p * stride + k + j];
    }
};

// the same two layouts for fixed-width byte keys, `words` 32-bit words each, moved word by word
// (packed rows: [slot_idx(k) | k keys of `words` words])
struct StridedWideParts {
    using Key = uint32_t;
    const int64_t* idx;
    const uint32_t* key;
    int64_t part_len;
    uint32_t words;
    __device__ int64_t index(int32_t p, uint32_t j) const { return idx[(int64_t)p * part_len + j]; }
    __device__ void take(int32_t p, uint32_t j, uint32_t* slot_key) const {
        const uint32_t* src = key + ((size_t)p * part_len + j) * words;
        for (uint32_t q = 0; q < words; ++q) slot_key[(size_t)j * words + q] = src[q];
    }
};

struct PackedWideRows {
    using Key = uint32_t;
    const int64_t* rows;
    int64_t stride;
    uint32_t k, words;
    __device__ int64_t index(int32_t p, uint32_t j) const { return rows[(int64_t)p * stride + j]; }
    __device__ void take(int32_t p, uint32_t j, uint32_t* slot_key) const {
        const uint32_t* src = (const uint32_t*)(rows + (int64_t)p * stride + k) + (size_t)j * words;
        for (uint32_t q = 0; q < words; ++q) slot_key[(size_t)j * words + q] = src[q];
    }
};

// The rule: a part's larger index is the later writer.  The first part whose index for slot j is above
// `best` and above every other part's wins: its number is returned and `best` becomes its index.  -1:
// the slot keeps what it holds (no part, none newer, or a tie -- equal indices carry equal keys).
template <typename Src>
__device__ __forceinline__ int32_t merge_winner(const Src& src, int32_t parts, uint32_t j, int64_t& best) {
    int32_t from = -1;
    for (int32_t p = 0; p < parts; ++p) {
        const int64_t idx = src.index(p, j);
        if (idx > best) {
            best = idx;
            from = p;
        }
    }
    return from;
}

// The merge of `parts` parts into the slots.  kPublish (k <= 8192, Int / Long keys): one workgroup that
// also publishes the first m slot keys, the multi-GPU combine's last step before result(), as the
// publishing resolve_kernel is for a batch; else one slot per thread of a k-wide grid.
template <typename Src, bool kPublish>
__global__ __launch_bounds__(kPublish ? 1024 : kBlock) void merge_kernel(Src src, int32_t parts, uint32_t k,
                                                                       int64_t* __restrict__ slot_idx,
                                                                       typename Src::Key* __restrict__ slot_key,
                                                                       int64_t m, typename Src::Key* dst,
                                                                       uint32_t* flag, uint32_t gen) {
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < k; j += stride) {
        int64_t best = slot_idx[j];
        const int32_t from = merge_winner(src, parts, j, best);
        if (from >= 0) {
            slot_idx[j] = best;
            src.take(from, j, slot_key);
        }
        if (kPublish && (int64_t)j < m) dst[j] = slot_key[j];
    }
    if (kPublish) publish_flag(flag, gen);
}

// packed multi-GPU row: [slot_idx(k) | keys widened to int64 (k)]
template <typename KeyT>
__global__ __launch_bounds__(kBlock) void export_packed_kernel(const int64_t* __restrict__ slot_idx,
                                                               const KeyT* __restrict__ slot_key, uint32_t k,
                                                               int64_t* __restrict__ row) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= k) return;
    row[j] = slot_idx[j];
    row[k + j] = (int64_t)slot_key[j];
}

// ---- fixed-width byte keys (key_width a multiple of 8 above 8: UUIDs, composite keys) ----------
// The element sampler never looks inside a key, so wide keys only change the copies: each slot's
// key is `words` 32-bit words, moved word by word.  The slot rule as in resolve_kernel (one kernel;
// `dst` non-null = publish, launched as one workgroup).
__global__ __launch_bounds__(1024) void resolve_wide_kernel(const uint32_t* __restrict__ keys, int64_t base,
                                                            int64_t n, uint32_t k, uint32_t words,
                                                            unsigned long long* __restrict__ win,
                                                            uint32_t* __restrict__ slot_key,
                                                            int64_t* __restrict__ slot_idx, int fresh, int64_t m,
                                                            uint32_t* dst, uint32_t* flag, uint32_t gen) {
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < k; j += stride) {
        const uint32_t* src = nullptr;  // the batch's key for the slot, if it takes one
        bool write = true;              // all cases but keep rewrite the slot's key
        slot_rule(
            j, win[j], base, n, fresh,
            [&](int64_t off, int64_t idx, bool winner) {
                src = keys + (size_t)off * words;
                slot_idx[j] = idx;
                if (winner) win[j] = 0;
            },
            [=](int64_t idx) { slot_idx[j] = idx; }, [&] { write = false; });
        uint32_t* o = slot_key + (size_t)j * words;
        const bool out = dst && (int64_t)j < m;
        for (uint32_t q = 0; q < words; ++q) {
            const uint32_t v = src ? src[q] : (write ? 0u : o[q]);
            if (write) o[q] = v;
            if (out) dst[(size_t)j * words + q] = v;
        }
    }
    if (dst) publish_flag(flag, gen);
}

// packed rows of wide keys: [slot_idx(k) | k keys of `words` 32-bit words]
__global__ __launch_bounds__(kBlock) void export_packed_wide_kernel(const int64_t* __restrict__ slot_idx,
                                                                    const uint32_t* __restrict__ slot_key, uint32_t k,
                                                                    uint32_t words, int64_t* __restrict__ row) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= k) return;
    row[j] = slot_idx[j];
    uint32_t* o = (uint32_t*)(row + k) + (size_t)j * words;
    for (uint32_t q = 0; q < words; ++q) o[q] = slot_key[(size_t)j * words + q];
}

inline DrawKey make_key(const DrawParams& dp) {
    return DrawKey{(uint32_t)dp.seed, (uint32_t)(dp.seed >> 32), (uint32_t)dp.stream,
                   (uint32_t)(dp.stream >> 32)};
}

inline unsigned grid_for(uint64_t items, unsigned cap = ~0u) {
    uint64_t b = (items + kBlock - 1) / kBlock;
    if (b < 1) b = 1;
    return (unsigned)(b < cap ? b : cap);
}

// K1's grid: a wave's last window, when partial, takes the per-block path (clip and dense
// checks, ~30 more VALU per iteration); so the grid is sized for whole windows per wave --
// m windows, m nearest to what kK1Grid workgroups would run -- where the launch is large enough
// (1e9 draws: 5086 workgroups, 2 windows of 12 iterations per wave)
inline unsigned k1_grid(uint64_t n_groups) {
    constexpr uint64_t per_window = (uint64_t)kK1Unroll * kBlock * kK1Win;  // blocks per workgroup-window
    // below ~3 whole-window workgroups per CU, every CU gets work instead (partial windows)
    if (n_groups < per_window * 768) return grid_for((n_groups + kK1Unroll - 1) / kK1Unroll, kK1Grid);
    const uint64_t m = std::max<uint64_t>(1, (n_groups + per_window * kK1Grid / 2) / (per_window * kK1Grid));
    return (unsigned)std::max<uint64_t>(1, n_groups / (per_window * m));
}

// The two-group schedule (k1_body_q): the first kK1W1 waves (one generation of resident waves: 6 four-
// wave workgroups per CU) take A steady half windows each, the rest go two per wave.  The launch's slow
// iterations (its dense head, its clipped ends) are no units: the first group's waves take them round-
// robin ahead of their units (k1_launch).
// A: the second group keeps kK1Rest .. kK1Rest + kK1W1 units (0.44 .. 0.94 of a generation at two per
// wave) and the first group takes all the others.  tools/micro_k1o s (K1O_N for the size), best A per
// size, us: 6e8 7 (48.5; 6: 50.5), 9.5e8 11 (74.0; 10: 74.8, 12: 74.4), 1e9 12 (77.3-77.5; 10: 78.4-78.7,
// 11: 80.0, 13: 80.3 -- 1.5 k units left for the second group), 1.2e9 15 (91.9; 14: 92.8), 1.5e9 18
// (114.1; 17: 115.2, 19: 115.4), 2e9 25 (150.0; 24: 151.2, 20: 153.7) -- each the A of this rule; the
// 75.5 % share it replaces gave 6, 9, 10, 12, 15 and 20.  B = 1 or 3 and 5120 or 4096 first-group waves
// were no better at 1e9 (profiles/k1_fixed_cost/micro_k1o_sched.jsonl).
// From kK1MinA units per first-group wave (4.44e8 draws at k = 1024); grid-stride against the schedule,
// micro_k1o n: 4.5e8 43.4 vs 42.0 us, 6e8 56.4 vs 55.7, 7.5e8 67.2 vs 63.8, 9e8 75.5 vs 72.4 (these
// four still with the 75.5 % share), 1e9 79.1 vs 78.1, 2e9 153.8 vs 151.9; below 4.5e8 not measured.
constexpr uint32_t kK1W1 = 256 * 6 * (kBlock / 64);
constexpr uint32_t kK1Rest = 5400, kK1MinA = 5;
inline unsigned k1_plan(uint32_t k, uint64_t lo, uint64_t hi, uint64_t g_begin, uint64_t n_groups, K1Launch& P) {
    const unsigned stride_grid = k1_grid(n_groups);
    P = k1_launch<kK1Win>(k, lo, hi, g_begin, n_groups, stride_grid, kBlock);
    // a launch with too few steady units (small, or nearly all dense: 256 k near its end) runs grid-stride
    if (P.units < kK1MinA * kK1W1 + kK1Rest) return stride_grid;
    const unsigned grid = k1_schedule(P, kK1W1, (P.units - kK1Rest) / kK1W1, 2, kBlock);
    return grid ? grid : stride_grid;
}

// the instantiation a planned launch runs (tests/cpp/test_k1_forms.cpp pins the choice on both sides of 2^33 and 2^40)
inline auto k1_last_writer_for(const K1Launch& P) { return k1_fast_form(P) ? k1_last_writer<true> : k1_last_writer<false>; }
template <typename KeyT>
inline auto k1_resolve_publish_for(const K1Launch& P) {
    return k1_fast_form(P) ? k1_resolve_publish<KeyT, true> : k1_resolve_publish<KeyT, false>;
}

// f(KeyT{}) with the key type of a 4- / 8-byte key_width (f launches a kernel); the launch's error
template <typename F>
hipError_t with_key_type(int key_width, F&& f) {
    if (key_width == 8) f(int64_t{});
    else f(int32_t{});
    return hipGetLastError();
}

// threads of a one-workgroup form over k slots: whole waves, at most 1024
inline unsigned one_group_threads(uint32_t k) {
    return std::min<unsigned>(1024, std::max<unsigned>(64, (k + 63) / 64 * 64));
}

}  // namespace

hipError_t launch_k1_last_writer(const DrawParams& dp, uint32_t k, uint64_t lo, uint64_t hi,
                                 unsigned long long* batch_win, hipStream_t st) {
    if (hi <= lo) return hipSuccess;
    const uint64_t g_end = (hi + 15) >> 4;
    constexpr uint64_t kMaxGroups = 1ull << 31;  // block offsets are 32-bit queue entries
    uint64_t n_groups = 0;
    for (uint64_t g_begin = lo >> 4; g_begin < g_end; g_begin += n_groups) {
        // and no launch crosses a multiple of 2^32 blocks: the counter's high word is a scalar
        const uint64_t g_wrap = ((g_begin >> 32) + 1) << 32;
        n_groups = std::min<uint64_t>(std::min<uint64_t>(g_end, g_wrap) - g_begin, kMaxGroups);
        K1Launch P;
        const unsigned grid = k1_plan(k, lo, hi, g_begin, n_groups, P);
        const auto kernel = k1_last_writer_for(P);
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(kBlock), 0, st, make_key(dp), k, lo, hi, g_begin, n_groups,
                           batch_win, P);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

bool k1_fused_ok(uint64_t lo, uint64_t hi, uint32_t k, int key_width) {
    if (hi <= lo || k > kK1FusedMaxK || (key_width != 8 && key_width != 4)) return false;
    const uint64_t g_begin = lo >> 4, g_end = (hi + 15) >> 4;
    // one launch of launch_k1_last_writer: no 2^32-block crossing, fewer than 2^31 blocks
    return g_end - g_begin <= (1ull << 31) && g_end <= ((g_begin >> 32) + 1) << 32;
}

hipError_t launch_k1_resolve_publish(const DrawParams& dp, uint64_t lo, uint64_t hi, const SlotBlock& sb,
                                     uint32_t* ticket, const Batch& b, const Publication& pub, hipStream_t st) {
    if (!k1_fused_ok(lo, hi, sb.k, sb.key_width)) return hipErrorInvalidValue;
    const uint64_t g_begin = lo >> 4, n_groups = ((hi + 15) >> 4) - g_begin;
    K1Launch P;
    const unsigned grid = k1_plan(sb.k, lo, hi, g_begin, n_groups, P);
    return with_key_type(sb.key_width, [&](auto t) {
        using T = decltype(t);
        const auto kernel = k1_resolve_publish_for<T>(P);
        const K1Tail<T> tail{ticket, (const T*)b.keys, b.base, b.n,  (T*)sb.slot_key, sb.slot_idx,
                             pub.m,  (T*)pub.dst,      pub.flag, pub.gen, (int)b.fresh, grid};
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(kBlock), 0, st, tail, make_key(dp), sb.k, lo, hi, g_begin, n_groups,
                           sb.win, P);
    });
}

hipError_t launch_resolve(const SlotBlock& sb, const Batch& b, const Publication& pub, hipStream_t st, bool small) {
    const uint32_t k = sb.k;
    if (sb.key_width > 8) {  // one kernel: a k-wide grid (capped, it strides), or one publishing workgroup
        const unsigned grid = pub.dst ? 1 : grid_for(k, 256 * 64);
        hipLaunchKernelGGL(resolve_wide_kernel, dim3(grid), dim3(pub.dst ? one_group_threads(k) : kBlock), 0, st,
                           (const uint32_t*)b.keys, b.base, b.n, k, (uint32_t)sb.key_width / 4, sb.win,
                           (uint32_t*)sb.slot_key, sb.slot_idx, (int)b.fresh, pub.m, (uint32_t*)pub.dst, pub.flag,
                           pub.gen);
        return hipGetLastError();
    }
    return with_key_type(sb.key_width, [&](auto t) {
        using T = decltype(t);
        auto go = [&](auto kernel, unsigned grid, unsigned threads) {
            hipLaunchKernelGGL(kernel, dim3(grid), dim3(threads), 0, st, (const T*)b.keys, b.base, b.n, k, sb.win,
                               (T*)sb.slot_key, sb.slot_idx, (int)b.fresh, pub.m, (T*)pub.dst, pub.flag, pub.gen);
        };
        if (!pub.dst) go(resolve_kernel<T, false>, grid_for(k), kBlock);
        else if (!(small && k <= 8 * kBlock)) go(resolve_kernel<T, true>, 1, one_group_threads(k));
        else if (k <= 2 * kBlock) go(resolve_publish_small_kernel<T, 2>, 1, kBlock);
        else if (k <= 4 * kBlock) go(resolve_publish_small_kernel<T, 4>, 1, kBlock);
        else go(resolve_publish_small_kernel<T, 8>, 1, kBlock);
    });
}

// fresh handle: batch_win = 0, slot_idx = -1 (empty), slot_key = 0
__global__ __launch_bounds__(kBlock) void init_slots_kernel(uint8_t* slot_key, int key_width, int64_t* slot_idx,
                                                            unsigned long long* win, uint32_t k, uint32_t* ticket) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    if (ticket && blockIdx.x == 0 && threadIdx.x == 0) *ticket = 0;
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < k; j += stride) {
        win[j] = 0;
        slot_idx[j] = -1;
        if (key_width == 8)
            ((int64_t*)slot_key)[j] = 0;
        else if (key_width == 4)
            ((int32_t*)slot_key)[j] = 0;
        else
            for (int q = 0; q < key_width / 4; ++q) ((uint32_t*)slot_key)[(size_t)j * (key_width / 4) + q] = 0;
    }
}

hipError_t launch_init_slots(const SlotBlock& sb, hipStream_t st, uint32_t* ticket) {
    hipLaunchKernelGGL(init_slots_kernel, dim3(grid_for(sb.k, 256 * 64)), dim3(kBlock), 0, st, (uint8_t*)sb.slot_key,
                       sb.key_width, sb.slot_idx, sb.win, sb.k, ticket);
    return hipGetLastError();
}

// result() tail: copy the k-slot reservoir straight into coherent pinned host memory, then publish
// `gen` in the host flag with a system-scope release.  The host spins on the flag: ~7 us less
// than hipMemcpyAsync D2H + hipStreamSynchronize for an 8 KB reservoir (tools/probe_latency.hip).
__global__ __launch_bounds__(1024) void publish_kernel(const uint32_t* __restrict__ src, uint32_t* dst,
                                                      int64_t words, uint32_t* flag, uint32_t gen) {
    // 16-B stores: a quarter of the PCIe write transactions of 4-B ones (both ends 16-B aligned)
    const int64_t vecs = words >> 2;
    for (int64_t i = threadIdx.x; i < vecs; i += blockDim.x)
        ((uint4*)dst)[i] = ((const uint4*)src)[i];
    for (int64_t i = (vecs << 2) + threadIdx.x; i < words; i += blockDim.x) dst[i] = src[i];
    publish_flag(flag, gen);
}

// Publication of a large buffer (a distinct set: up to 512 KB at k = 65536) by several workgroups:
// one workgroup's posted PCIe writes run at ~20 GB/s.  Each workgroup releases its stores at system
// scope and takes a ticket; the last one stores the flag (and re-arms the ticket).
__global__ __launch_bounds__(1024) void publish_multi_kernel(const uint32_t* __restrict__ src, uint32_t* dst,
                                                            int64_t words, uint32_t* flag, uint32_t gen,
                                                            uint32_t* ticket) {
    const int64_t vecs = words >> 2;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (int64_t i = t0; i < vecs; i += stride) ((uint4*)dst)[i] = ((const uint4*)src)[i];
    for (int64_t i = (vecs << 2) + t0; i < words; i += stride) dst[i] = src[i];
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        __threadfence_system();
        const uint32_t prev = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        if (prev == gridDim.x - 1) {
            __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __threadfence_system();
            __hip_atomic_store(flag, gen, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}

hipError_t launch_publish_multi(const void* src, int64_t bytes, void* dst_host_dev, uint32_t* flag_dev, uint32_t gen,
                                uint32_t* ticket_dev, hipStream_t st) {
    const int64_t per = 32 * 1024;  // bytes per workgroup
    const unsigned grid = (unsigned)std::min<int64_t>(32, std::max<int64_t>(1, (bytes + per - 1) / per));
    hipLaunchKernelGGL(publish_multi_kernel, dim3(grid), dim3(1024), 0, st, (const uint32_t*)src,
                       (uint32_t*)dst_host_dev, bytes / 4, flag_dev, gen, ticket_dev);
    return hipGetLastError();
}

hipError_t launch_publish(const void* src, int64_t bytes, void* dst_host_dev, uint32_t* flag_dev, uint32_t gen,
                          hipStream_t st) {
    hipLaunchKernelGGL(publish_kernel, dim3(1), dim3(1024), 0, st, (const uint32_t*)src, (uint32_t*)dst_host_dev,
                       bytes / 4, flag_dev, gen);
    return hipGetLastError();
}

// ---- index-only batches (rsv_sample_indexed / rsv_fill_slots) -------------------------------
// The resolve of a batch sampled by index alone: the slot rule for slot j with no key read --
// slot_idx[j] = the winner or the fill; returns its offset in the batch (-1: the slot took no
// element).  The keys arrive later from the caller (fill_slots_kernel).
__device__ __forceinline__ int64_t resolve_index_slot(uint64_t j, int64_t base, int64_t n, unsigned long long* win,
                                                      int64_t* slot_idx, int fresh, uint8_t* slot_key, int key_width) {
    int64_t off = -1;
    slot_rule(
        (int64_t)j, win[j], base, n, fresh,
        [&](int64_t o, int64_t idx, bool winner) {
            slot_idx[j] = idx;
            if (winner) win[j] = 0;
            off = o;
        },
        [=](int64_t idx) {
            slot_idx[j] = idx;
            for (int q = 0; q < key_width; ++q) slot_key[j * key_width + q] = 0;
        },
        [] {});
    return off;
}

__global__ __launch_bounds__(kBlock) void resolve_indices_kernel(int64_t base, int64_t n, uint32_t k,
                                                                 unsigned long long* __restrict__ win,
                                                                 int64_t* __restrict__ slot_idx, int fresh,
                                                                 uint8_t* __restrict__ slot_key, int key_width,
                                                                 int64_t* __restrict__ offs) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < k; j += stride)
        offs[j] = resolve_index_slot(j, base, n, win, slot_idx, fresh, slot_key, key_width);
}

// keys[j] (host-supplied, one per slot, slot order) into every slot the index-only batch changed
__global__ __launch_bounds__(kBlock) void fill_slots_kernel(const int64_t* __restrict__ offs, const uint8_t* __restrict__ keys,
                                                            uint32_t k, int key_width, uint8_t* __restrict__ slot_key) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < k; j += stride) {
        if (offs[j] < 0) continue;
        if (key_width == 8) ((int64_t*)slot_key)[j] = ((const int64_t*)keys)[j];
        else if (key_width == 4) ((int32_t*)slot_key)[j] = ((const int32_t*)keys)[j];
        else
            for (int q = 0; q < key_width; ++q) slot_key[j * key_width + q] = keys[j * key_width + q];
    }
}

// The two publishing forms below are kernels of their own, not a compile-time case of the two above.
// Merged (resolve_indices_kernel<kPublish>: 50 -> 56 SGPRs, 14 -> 18 VGPRs; fill_slots_kernel<kPublish>
// with the key type as a run-time branch: 28 -> 52 SGPRs, 8 -> 14 VGPRs) the winners-only host batch
// on philox_r (tools/bench_paths.py c2h), whose latency path they are on, measured 0.11309 ms against
// the parent's 0.11088 - 0.11230 and 0.11335 ms against 0.11080 - 0.11290 in two sessions
// (profiles/elements_shared/refactor_ab.jsonl, "s1" and "s2").

// resolve_indices_kernel + publication of offs[] into coherent host memory (flag = gen) in one
// dispatch, for k <= kIdxPublishMaxK: the host spins on the flag instead of a D2H copy + stream
// synchronize (the winners-only host batches and rsv_sample_indexed)
constexpr uint32_t kIdxPublishMaxK = 8192;

__global__ __launch_bounds__(1024) void resolve_indices_publish_kernel(int64_t base, int64_t n, uint32_t k,
                                                                       unsigned long long* __restrict__ win,
                                                                       int64_t* __restrict__ slot_idx, int fresh,
                                                                       uint8_t* __restrict__ slot_key, int key_width,
                                                                       int64_t* __restrict__ offs, int64_t* offs_host,
                                                                       uint32_t* flag, uint32_t gen) {
    for (uint32_t j = threadIdx.x; j < k; j += blockDim.x) {
        const int64_t off = resolve_index_slot(j, base, n, win, slot_idx, fresh, slot_key, key_width);
        offs[j] = off;
        offs_host[j] = off;
    }
    publish_flag(flag, gen);
}

// fill_slots_kernel + publication of the first m slot keys (the publishing resolve_kernel's form) for
// k <= 8192 and 4- / 8-byte keys: the host-keyed batch's reservoir is published with its last kernel
template <typename KeyT>
__global__ __launch_bounds__(1024) void fill_slots_publish_kernel(const int64_t* __restrict__ offs,
                                                                  const KeyT* __restrict__ keys, uint32_t k,
                                                                  KeyT* __restrict__ slot_key, int64_t m, KeyT* dst,
                                                                  uint32_t* flag, uint32_t gen) {
    for (uint32_t j = threadIdx.x; j < k; j += blockDim.x) {
        KeyT v;
        if (offs[j] >= 0) {
            v = keys[j];
            slot_key[j] = v;
        } else {
            v = slot_key[j];
        }
        if ((int64_t)j < m) dst[j] = v;
    }
    publish_flag(flag, gen);
}

bool resolve_indices_publish_ok(uint32_t k) { return k <= kIdxPublishMaxK; }

hipError_t launch_resolve_indices(const SlotBlock& sb, const Batch& b, int64_t* offs, const Publication& pub,
                                  hipStream_t st) {
    if (!pub.dst)
        hipLaunchKernelGGL(resolve_indices_kernel, dim3(grid_for(sb.k, 256 * 64)), dim3(kBlock), 0, st, b.base, b.n, sb.k,
                           sb.win, sb.slot_idx, (int)b.fresh, (uint8_t*)sb.slot_key, sb.key_width, offs);
    else if (!resolve_indices_publish_ok(sb.k))
        return hipErrorInvalidValue;
    else
        hipLaunchKernelGGL(resolve_indices_publish_kernel, dim3(1), dim3(one_group_threads(sb.k)), 0, st, b.base, b.n,
                           sb.k, sb.win, sb.slot_idx, (int)b.fresh, (uint8_t*)sb.slot_key, sb.key_width, offs,
                           (int64_t*)pub.dst, pub.flag, pub.gen);
    return hipGetLastError();
}

bool fill_slots_publish_ok(uint32_t k, int key_width) {
    return k <= kIdxPublishMaxK && (key_width == 4 || key_width == 8);
}

hipError_t launch_fill_slots(const int64_t* offs, const void* keys, const SlotBlock& sb, const Publication& pub,
                             hipStream_t st) {
    if (!pub.dst) {
        hipLaunchKernelGGL(fill_slots_kernel, dim3(grid_for(sb.k, 256 * 64)), dim3(kBlock), 0, st, offs,
                           (const uint8_t*)keys, sb.k, sb.key_width, (uint8_t*)sb.slot_key);
        return hipGetLastError();
    }
    if (!fill_slots_publish_ok(sb.k, sb.key_width)) return hipErrorInvalidValue;
    return with_key_type(sb.key_width, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(fill_slots_publish_kernel<T>, dim3(1), dim3(one_group_threads(sb.k)), 0, st, offs,
                           (const T*)keys, sb.k, (T*)sb.slot_key, pub.m, (T*)pub.dst, pub.flag, pub.gen);
    });
}

hipError_t launch_replay_events(const int64_t* ev_pos, const int32_t* ev_slot, int64_t n_events,
                                uint32_t k, unsigned long long* batch_win, hipStream_t st) {
    if (n_events <= 0) return hipSuccess;
    const unsigned grid = (unsigned)((n_events + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(replay_kernel, dim3(grid), dim3(kBlock), 0, st, ev_pos, ev_slot, n_events, k,
                       batch_win);
    return hipGetLastError();
}

hipError_t launch_export_draws(const DrawParams& dp, uint64_t i0, int64_t n, uint64_t* j,
                               hipStream_t st) {
    if (n <= 0) return hipSuccess;
    const unsigned grid = (unsigned)((n + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(export_draws_kernel, dim3(grid), dim3(kBlock), 0, st, make_key(dp), i0, n, j);
    return hipGetLastError();
}

namespace {

// one merge_kernel launch over the source `src`: a k-wide grid, or the one publishing workgroup
template <bool kPublish, typename Src>
void launch_merge(const Src& src, int32_t parts, const SlotBlock& sb, const Publication& pub, hipStream_t st) {
    using Key = typename Src::Key;
    hipLaunchKernelGGL((merge_kernel<Src, kPublish>), dim3(kPublish ? 1 : grid_for(sb.k)),
                       dim3(kPublish ? one_group_threads(sb.k) : kBlock), 0, st, src, parts, sb.k, sb.slot_idx,
                       (Key*)sb.slot_key, pub.m, (Key*)pub.dst, pub.flag, pub.gen);
}

}  // namespace

hipError_t launch_merge_slots(const int64_t* idx_parts, const void* key_parts, int32_t parts, int64_t part_len,
                              const SlotBlock& sb, hipStream_t st) {
    if (sb.key_width > 8) {
        const StridedWideParts src{idx_parts, (const uint32_t*)key_parts, part_len, (uint32_t)sb.key_width / 4};
        launch_merge<false>(src, parts, sb, Publication{}, st);
        return hipGetLastError();
    }
    return with_key_type(sb.key_width, [&](auto t) {
        using T = decltype(t);
        launch_merge<false>(StridedParts<T>{idx_parts, (const T*)key_parts, part_len}, parts, sb, Publication{}, st);
    });
}

hipError_t launch_export_packed(const SlotBlock& sb, int64_t* row, hipStream_t st) {
    if (sb.key_width > 8) {
        hipLaunchKernelGGL(export_packed_wide_kernel, dim3(grid_for(sb.k)), dim3(kBlock), 0, st, sb.slot_idx,
                           (const uint32_t*)sb.slot_key, sb.k, (uint32_t)sb.key_width / 4, row);
        return hipGetLastError();
    }
    return with_key_type(sb.key_width, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(export_packed_kernel<T>, dim3(grid_for(sb.k)), dim3(kBlock), 0, st, sb.slot_idx,
                           (const T*)sb.slot_key, sb.k, row);
    });
}

hipError_t launch_merge_packed(const int64_t* rows, int32_t parts, int64_t stride, const SlotBlock& sb,
                               const Publication& pub, hipStream_t st) {
    if (sb.key_width > 8) {  // byte keys are merged without a publication (the caller never asks for one)
        if (pub.dst) return hipErrorInvalidValue;
        launch_merge<false>(PackedWideRows{rows, stride, sb.k, (uint32_t)sb.key_width / 4}, parts, sb, pub, st);
        return hipGetLastError();
    }
    return with_key_type(sb.key_width, [&](auto t) {
        using T = decltype(t);
        const PackedRows<T> src{rows, stride, sb.k};
        if (pub.dst) launch_merge<true>(src, parts, sb, pub, st);
        else launch_merge<false>(src, parts, sb, pub, st);
    });
}

}  // namespace rsv
