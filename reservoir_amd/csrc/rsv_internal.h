// rsv_internal.h -- host-side declarations shared between the runtime and the kernel translation
// units of libreservoir_hip.so.  Not part of the public ABI (that is include/reservoir_hip.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "rsv_buffers.h"  // the resource pool (rsv_pool.h) and the owning buffers over it

namespace rsv {

// thread-local last error (rsv_last_error)
void set_error(const std::string& msg);
// a failed HIP call as the last error, "<what>: <the HIP error string>"; returns its status
// (RSV_E_OUT_OF_MEMORY for hipErrorOutOfMemory, else RSV_E_DEVICE)
int hip_status(hipError_t e, const char* what);

#define RSV_HIP_TRY(expr)                                                                     \
    do {                                                                                      \
        hipError_t _e = (expr);                                                               \
        if (_e != hipSuccess) {                                                               \
            ::rsv::set_error(std::string(#expr) + ": " + hipGetErrorString(_e));              \
            return _e == hipErrorOutOfMemory ? RSV_E_OUT_OF_MEMORY : RSV_E_DEVICE;            \
        }                                                                                     \
    } while (0)

// HIP-event timing of a handle's hot kernel (rsv_profile_enable / rsv_profile_read)
struct KernelTimer {
    bool on = false;
    int device = 0;
    std::vector<hipEvent_t> ev;  // start/stop pairs, recycled after each drain
    size_t used = 0;
    double total_ms = 0;
    int64_t launches = 0;
    // Timing-only events (hipEventDisableSystemFence): each record skips the system-scope fence,
    // which costs the timed stream ~5 us per step less than default events and ~9 us less than
    // hipExtLaunchKernelGGL's start/stop events (tools/probe_events.hip, MI355X).
    static constexpr unsigned kFlags = hipEventDisableSystemFence;
    void mark(hipStream_t st) {
        if (!on) return;
        if (used == ev.size()) {
            hipEvent_t e;
            if (pool_event(&e, kFlags) != hipSuccess) return;
            ev.push_back(e);
        }
        (void)hipEventRecord(ev[used++], st);
    }
    hipError_t drain() {
        for (size_t i = 0; i + 1 < used; i += 2) {
            hipError_t e = hipEventSynchronize(ev[i + 1]);
            if (e != hipSuccess) return e;
            float ms = 0;
            e = hipEventElapsedTime(&ms, ev[i], ev[i + 1]);
            if (e != hipSuccess) return e;
            total_ms += ms;
            launches++;
        }
        used = 0;
        return hipSuccess;
    }
    ~KernelTimer() {
        for (hipEvent_t e : ev) pool_release_event(device, e, kFlags);
    }
};

struct DrawParams {
    uint64_t seed;
    uint64_t stream;
};

// ---- elements (Algorithm R, draw format R2) -------------------------------------------------
// Argument bundles of the element launchers (plain data: no ownership, no checks).
// A handle's slot block: batch_win[k] (0 = no writer in this batch), slot_idx[k] (-1 = empty), the keys.
struct SlotBlock {
    unsigned long long* win;
    int64_t* slot_idx;
    void* slot_key;
    uint32_t k;
    int key_width;
};
// One batch: n elements at global indices [base, base + n); keys null for an index-only batch; fresh:
// the first batch of a handle whose slots were never initialised (untouched slots become empty).
struct Batch {
    const void* keys;
    int64_t base, n;
    bool fresh;
};
// What a launch publishes besides its own work: the first m slot keys (or the k offsets of an index-only
// batch) into coherent host memory dst (device alias), then flag = gen.  dst null: no publication.
struct Publication {
    int64_t m = 0;
    void* dst = nullptr;
    uint32_t* flag = nullptr;
    uint32_t gen = 0;
};

// K1: per-slot last writer of the index range [lo, hi) (only indices >= k can evict) into
// batch_win[k] (atomicMax keeps the largest index).
hipError_t launch_k1_last_writer(const DrawParams& dp, uint32_t k, uint64_t lo, uint64_t hi,
                                 unsigned long long* batch_win, hipStream_t st);
// K1 + the publishing resolve as one dispatch, when k1_fused_ok: a batch whose range K1 covers in one
// launch, k <= 2048, 4- or 8-byte keys.  ticket: a zeroed device word, re-armed by the launch.
bool k1_fused_ok(uint64_t lo, uint64_t hi, uint32_t k, int key_width);
hipError_t launch_k1_resolve_publish(const DrawParams& dp, uint64_t lo, uint64_t hi, const SlotBlock& sb,
                                     uint32_t* ticket, const Batch& b, const Publication& pub, hipStream_t st);
// init_slots also zeroes `ticket` when non-null.
hipError_t launch_init_slots(const SlotBlock& sb, hipStream_t st, uint32_t* ticket = nullptr);
hipError_t launch_publish(const void* src, int64_t bytes, void* dst_host_dev, uint32_t* flag_dev, uint32_t gen,
                          hipStream_t st);
// the same from up to 32 workgroups (large buffers); ticket_dev: a zeroed device word, re-armed
hipError_t launch_publish_multi(const void* src, int64_t bytes, void* dst_host_dev, uint32_t* flag_dev, uint32_t gen,
                                uint32_t* ticket_dev, hipStream_t st);
// Resolve: fill phase for slots in [base, base+n) and winners of batch_win; resets batch_win.  With a
// publication (k <= 8192) one workgroup does it and publishes; small: as one 256-thread workgroup where
// k <= 2048 (a resolve running beside K1 on a second stream).  sb.slot_idx may be null without one, for
// 4- / 8-byte keys only.
hipError_t launch_resolve(const SlotBlock& sb, const Batch& b, const Publication& pub, hipStream_t st,
                          bool small = false);
// index-only batches: resolve into slot_idx with offs[k] = the batch offset of each slot's new element
// (-1: none), published too (pub.dst takes the k offsets, pub.m unused) when resolve_indices_publish_ok;
// then the caller's keys into the changed slots, with the first pub.m slot keys published when
// fill_slots_publish_ok (k <= 8192; 4- / 8-byte keys)
bool resolve_indices_publish_ok(uint32_t k);
hipError_t launch_resolve_indices(const SlotBlock& sb, const Batch& b, int64_t* offs, const Publication& pub,
                                  hipStream_t st);
bool fill_slots_publish_ok(uint32_t k, int key_width);
hipError_t launch_fill_slots(const int64_t* offs, const void* keys, const SlotBlock& sb, const Publication& pub,
                             hipStream_t st);
// K1': events (1-based pos, slot) -> batch_win
hipError_t launch_replay_events(const int64_t* ev_pos, const int32_t* ev_slot, int64_t n_events,
                                uint32_t k, unsigned long long* batch_win, hipStream_t st);
hipError_t launch_export_draws(const DrawParams& dp, uint64_t i0, int64_t n, uint64_t* j,
                               hipStream_t st);
// K2: segmented
hipError_t launch_segmented(const void* keys, int key_width, const int64_t* offsets, int64_t S,
                            uint32_t k, const DrawParams& dp, void* out, int64_t* counts,
                            hipStream_t st);
// K2 resumed (rsv_segmented.hip): the streams as rows of caller-held state (keys[num_states*k], idx = the
// global index of each slot's last writer or -1, next[num_states]); per slot the largest index wins.
// update: segment b holds the indices [bases[b] (null: next[r]), + len) of row r = stream_ids[b] (null: b),
// Philox stream dp.stream + r; merge: parts laid out [parts][num_states][k], [..][k], [parts][num_states].
// k <= kSegSampleStateMaxK: the workgroup form's 64-bit winner table has to fit LDS (k2::lds_bytes_wg).
constexpr uint32_t kSegSampleStateMaxK = 15104;
hipError_t launch_segmented_update(const void* keys, int key_width, const int64_t* offsets, const int64_t* stream_ids,
                                   const int64_t* bases, int64_t num_segments, int64_t num_states, uint32_t k,
                                   const DrawParams& dp, void* state_keys, int64_t* state_idx, int64_t* state_next,
                                   hipStream_t st);
hipError_t launch_segmented_merge(const void* part_keys, int key_width, const int64_t* part_idx,
                                  const int64_t* part_next, int32_t parts, int64_t num_states, uint32_t k,
                                  void* state_keys, int64_t* state_idx, int64_t* state_next, hipStream_t st);
// K2 over byte keys (rsv_segmented.hip, the same element loops and forms): rows of key_width bytes (16..256, a
// multiple of 8; every rows buffer 8-byte aligned), offsets and indices count rows.  out_rows[S*k] rows, zero
// beyond counts[s]; the resumed state is rows[num_states*k], idx, next as above (k <= kSegSampleStateMaxK);
// part_rows is [parts][num_states][k] rows.  The gather moves 16-byte granules where key_width % 16 == 0 and
// both buffers are 16-byte aligned, else 8-byte ones.
hipError_t launch_segmented_rows(const void* rows, int key_width, const int64_t* offsets, int64_t S, uint32_t k,
                                 const DrawParams& dp, void* out_rows, int64_t* counts, hipStream_t st);
hipError_t launch_segmented_rows_update(const void* rows, int key_width, const int64_t* offsets,
                                        const int64_t* stream_ids, const int64_t* bases, int64_t num_segments,
                                        int64_t num_states, uint32_t k, const DrawParams& dp, void* state_rows,
                                        int64_t* state_idx, int64_t* state_next, hipStream_t st);
hipError_t launch_segmented_rows_merge(const void* part_rows, int key_width, const int64_t* part_idx,
                                       const int64_t* part_next, int32_t parts, int64_t num_states, uint32_t k,
                                       void* state_rows, int64_t* state_idx, int64_t* state_next, hipStream_t st);
// The grouping pass (rsv_group.hip): ids[n] (int64 or int32 by id_width), the state row of each
// element in arrival order, to the dense CSR over num_states rows -- offsets[num_states + 1] and order[n], a
// permutation of [0, n): row r's positions in arrival order at order[offsets[r], offsets[r+1]), the positions whose
// id lies outside [0, num_states) behind offsets[num_states], in arrival order too.  A stable radix partition over
// the low bits of the id (the width of num_states); stream-ordered, scratch from hipMallocAsync.  n <= kGroupMaxN,
// num_states <= kGroupMaxStates (the host checks).
constexpr int64_t kGroupMaxN = 0x7FFFFFFFll, kGroupMaxStates = 0xFFFFFFFEll;
hipError_t launch_group_by_stream(const void* ids, int id_width, int64_t n, int64_t num_states, int64_t* offsets,
                                  int32_t* order, hipStream_t st);
// K2 resumed through a permutation (rsv_segmented.hip): launch_segmented_update / _rows_update with segment b's
// p-th element at keys[order[offsets[b] + p]] (order: n_keys entries in [0, n_keys)).  Only the write-back reads
// order, for the slots it replaces; a slot whose entry lies outside the range keeps its key and idx.
hipError_t launch_segmented_update_indirect(const void* keys, int64_t n_keys, const int32_t* order, int key_width,
                                            const int64_t* offsets, const int64_t* stream_ids, const int64_t* bases,
                                            int64_t num_segments, int64_t num_states, uint32_t k, const DrawParams& dp,
                                            void* state_keys, int64_t* state_idx, int64_t* state_next, hipStream_t st);
hipError_t launch_segmented_rows_update_indirect(const void* rows, int64_t n_rows, const int32_t* order, int key_width,
                                                 const int64_t* offsets, const int64_t* stream_ids,
                                                 const int64_t* bases, int64_t num_segments, int64_t num_states,
                                                 uint32_t k, const DrawParams& dp, void* state_rows,
                                                 int64_t* state_idx, int64_t* state_next, hipStream_t st);
// K2 keyless (rsv_segmented.hip, the same element loops and forms): no element reaches the device.  Stateless:
// out_idx[S*k] takes each slot's stream-relative source index (-1: empty), streams longer than the split length
// (RSV_K2_SPLIT_LEN) in pieces over the whole device.  The resumed state is (idx, next) as above; update also
// writes hits[num_segments*k] (the position inside the segment of each slot it replaced, else -1) and
// hit_counts[num_segments], for skipped segments too; merge writes src[num_states*k], the part each slot was
// taken from (-1: the row's own entry stood).
hipError_t launch_segmented_indexed(const int64_t* offsets, int64_t S, uint32_t k, const DrawParams& dp,
                                    int64_t* out_idx, int64_t* counts, hipStream_t st);
hipError_t launch_segmented_indexed_update(const int64_t* offsets, const int64_t* stream_ids, const int64_t* bases,
                                           int64_t num_segments, int64_t num_states, uint32_t k, const DrawParams& dp,
                                           int64_t* state_idx, int64_t* state_next, int64_t* hits, int64_t* hit_counts,
                                           hipStream_t st);
hipError_t launch_segmented_indexed_merge(const int64_t* part_idx, const int64_t* part_next, int32_t parts,
                                          int64_t num_states, uint32_t k, int64_t* state_idx, int64_t* state_next,
                                          int32_t* src, hipStream_t st);
// K5: segmented distinct (rsv_segdistinct.hip): per stream the bottom-k by (scrambled hash, key),
// (r0, r1) from java.util.Random(seed0 + s); hashes only for kHashPrecomputed, out_hashes may be null.
// k <= kSegDistinctMaxK; one wave per stream up to kSegDistinctWaveMaxK, one workgroup above.
constexpr uint32_t kSegDistinctWaveMaxK = 256;
constexpr uint32_t kSegDistinctMaxK = 4096;
hipError_t launch_segdistinct(const void* keys, int key_width, const int64_t* hashes, const int64_t* offsets, int64_t S,
                              uint32_t k, int hash_kind, uint64_t seed0, void* out_keys, int64_t* out_hashes,
                              int64_t* counts, hipStream_t st);
// K5 ordered (rsv_segdistinct.hip): launch_segdistinct with tied[s] = 1 iff the set is full and a distinct key
// outside it has its maximum hash, then a second kernel on the same stream that replays RandomValues over the tied
// streams in arrival order and rewrites their rows (ascending by (h, key) like the others).  No allocation.
hipError_t launch_segdistinct_ordered(const void* keys, int key_width, const int64_t* hashes, const int64_t* offsets,
                                      int64_t S, uint32_t k, int hash_kind, uint64_t seed0, void* out_keys,
                                      int64_t* out_hashes, int64_t* counts, int32_t* tied, hipStream_t st);
// K5 over byte keys (rsv_segdistinct.hip, the same element loop and forms): rows of key_width bytes (16..256, a
// multiple of 8; rows and out_rows 8-byte aligned), the bottom-k by (scrambled hash, row words unsigned).
// hashes: one per row, or null for UUID.hashCode of 16-byte rows.
hipError_t launch_segdistinct_rows(const void* rows, int key_width, const int64_t* hashes, const int64_t* offsets,
                                   int64_t S, uint32_t k, uint64_t seed0, void* out_rows, int64_t* out_hashes,
                                   int64_t* counts, hipStream_t st);
// K5 over byte keys, ordered (rsv_segdistinct.hip): launch_segdistinct_rows with tied[s] as for
// launch_segdistinct_ordered ("key" read as "row"), then the replay of RandomValues over the tied streams on the
// same stream, entries (h, row index), rows read from `rows` on equal hashes only.  No allocation.
hipError_t launch_segdistinct_rows_ordered(const void* rows, int key_width, const int64_t* hashes, const int64_t* offsets,
                                           int64_t S, uint32_t k, uint64_t seed0, void* out_rows, int64_t* out_hashes,
                                           int64_t* counts, int32_t* tied, hipStream_t st);
// K5 resumed (rsv_segdistinct.hip, the same element loop and forms): the teams started from the caller's state rows
// (keys[num_states*k], hashes, counts; ascending by (h, key) as launch_segdistinct writes them) and
// written back in place.  update: segment b into row stream_ids[b] (null: row b), seeded seed0 + row;
// merge: row r takes the valid entries of row r of every part ([parts][num_states][k]), hashes as stored.
hipError_t launch_segdistinct_update(const void* keys, int key_width, const int64_t* hashes, const int64_t* offsets,
                                     const int64_t* stream_ids, int64_t num_segments, int64_t num_states, uint32_t k,
                                     int hash_kind, uint64_t seed0, void* state_keys, int64_t* state_hashes,
                                     int64_t* state_counts, hipStream_t st);
hipError_t launch_segdistinct_merge(const void* part_keys, int key_width, const int64_t* part_hashes,
                                    const int64_t* part_counts, int32_t parts, int64_t num_states, uint32_t k,
                                    void* state_keys, int64_t* state_hashes, int64_t* state_counts, hipStream_t st);
// K5 ordered, resumed (rsv_segdistinct.hip): the state rows hold RandomValues' heap, counts[r] entries (h, key) in
// scala 2.13 mutable.PriorityQueue array order (entry j of the 1-indexed queue in slot j - 1), not ascending; one
// wave per segment continues the reference from them and writes them back in array order.  Segments, ids and
// seeding as launch_segdistinct_update.  No allocation.
hipError_t launch_segdistinct_ordered_update(const void* keys, int key_width, const int64_t* hashes, const int64_t* offsets,
                                             const int64_t* stream_ids, int64_t num_segments, int64_t num_states,
                                             uint32_t k, int hash_kind, uint64_t seed0, void* state_keys,
                                             int64_t* state_hashes, int64_t* state_counts, hipStream_t st);
// K5 ordered, resumed over byte keys (rsv_segdistinct.hip): the heap array holds references.  hashes and slots
// [num_states*k] are the queue's array order as for launch_segdistinct_ordered_update, the row of the entry at
// position p lies in slot slots[p] of the row's block of state_rows (storage, in no order; an admission takes slot
// n when the heap grows from n, else the evicted root's).  rows and state_rows 8-byte aligned, no input may alias
// the state.  hashes as for launch_segdistinct_rows.  No allocation.
hipError_t launch_segdistinct_rows_ordered_update(const void* rows, int key_width, const int64_t* hashes,
                                                  const int64_t* offsets, const int64_t* stream_ids, int64_t num_segments,
                                                  int64_t num_states, uint32_t k, uint64_t seed0, void* state_rows,
                                                  int64_t* state_hashes, int32_t* state_slots, int64_t* state_counts,
                                                  hipStream_t st);
// Candidates by hash for S object-key streams (rsv_segdistinct.hip, K5's forms and merge): segment b into the hash
// shadow of row stream_ids[b] (null: row b; shadow_hashes[num_states*k] ascending, shadow_counts), seeded seed0 + row;
// the positions with h below min(the shadow's k-th value, max_hashes[row] when set_sizes[row] >= k) -- every
// position while neither is known -- as (index into hashes, h) at out[b*cap + j], j < cap, the number found in
// out_counts[b].  A row whose segment overflowed cap is not written.  set_sizes and max_hashes: both or null.
hipError_t launch_segdistinct_candidates(const int64_t* hashes, const int64_t* offsets, const int64_t* stream_ids,
                                         int64_t num_segments, int64_t num_states, uint32_t k, uint64_t seed0,
                                         int64_t* shadow_hashes, int64_t* shadow_counts, const int64_t* set_sizes,
                                         const int64_t* max_hashes, int64_t* out_pos, int64_t* out_hashes, int64_t cap,
                                         int64_t* out_counts, hipStream_t st);
// K5 resumed over byte keys (rsv_segdistinct.hip): the state is rows[num_states*k] of key_width bytes, hashes,
// counts, as launch_segdistinct_rows writes them, moved in place.  rows / part_rows ([parts][num_states][k] rows)
// and state_rows 8-byte aligned, and no input may alias the state.  hashes as for launch_segdistinct_rows.
hipError_t launch_segdistinct_rows_update(const void* rows, int key_width, const int64_t* hashes, const int64_t* offsets,
                                          const int64_t* stream_ids, int64_t num_segments, int64_t num_states,
                                          uint32_t k, uint64_t seed0, void* state_rows, int64_t* state_hashes,
                                          int64_t* state_counts, hipStream_t st);
hipError_t launch_segdistinct_rows_merge(const void* part_rows, int key_width, const int64_t* part_hashes,
                                         const int64_t* part_counts, int32_t parts, int64_t num_states, uint32_t k,
                                         void* state_rows, int64_t* state_hashes, int64_t* state_counts,
                                         hipStream_t st);
// merge of exported element states: per slot the largest index among the parts and the current state
hipError_t launch_merge_slots(const int64_t* idx_parts, const void* key_parts, int32_t parts, int64_t part_len,
                              const SlotBlock& sb, hipStream_t st);

// packed combine rows: [slot_idx(k) | keys as int64 (k)] (byte keys: k keys of key_width / 4 words);
// the merge publishes the first pub.m keys too (k <= 8192, key_width 4 / 8)
hipError_t launch_export_packed(const SlotBlock& sb, int64_t* row, hipStream_t st);
hipError_t launch_merge_packed(const int64_t* rows, int32_t parts, int64_t stride, const SlotBlock& sb,
                               const Publication& pub, hipStream_t st);

// ---- distinct (bottom-k over the scrambled hash) --------------------------------------------
// The target of a speculative publication: the engine enqueues the merged set's publication into
// dst + flag (generation ++*gen_ctr) right behind a merge it expects to be the batch's last.
struct SpecPublish {
    void* dst = nullptr;          // coherent host buffer (device alias)
    uint32_t* flag = nullptr;
    uint32_t* gen_ctr = nullptr;  // the handle's publication generation counter
    bool arm = false;             // the next merge enqueues the publication behind it
    bool ok = false;              // the last enqueued publication holds the batch's final set
    uint32_t gen = 0;
    void target(void* dst_host_dev, uint32_t* flag_dev, uint32_t* gen_counter) {
        dst = dst_host_dev;
        flag = flag_dev;
        gen_ctr = gen_counter;
        ok = false;
    }
    // whether the last publication holds the batch's final set (its generation in *g); clears the target
    bool take(uint32_t* g) {
        const bool held = ok && dst;
        if (held) *g = gen;
        dst = nullptr;
        arm = ok = false;
        return held;
    }
};

// rsv_export_log's output rule: the candidates under `bound` (all of them for INT64_MAX) are stored
// while they fit `cap` and counted past it
struct LogEmit {
    int64_t bound, cap, cnt = 0;
    template <typename Store>  // store(i): the candidate into entry i of the caller's buffers
    void operator()(int64_t h, Store&& store) {
        if (bound == INT64_MAX || h < bound) {
            if (cnt < cap) store(cnt);
            ++cnt;
        }
    }
    int finish(int64_t* out_n) const;  // *out_n = the count; RSV_E_ILLEGAL_ARGUMENT past a cap > 0
};

// One distinct sampler behind the C ABI: NarrowDistinct<int64_t> / <int32_t> (Long / Int keys,
// rsv_distinct.hip) or WideDistinct (fixed-width byte keys, rsv_wide.hip).  keys / hashes are device
// pointers of the engine's key type (rows of key_width / 8 int64 words for byte keys).  A byte-key
// engine completes its device work before every call returns; a Long / Int engine may leave a rows
// merge pending (merge_rows) and settles it at the top of every other call.
struct DistinctEngine {
    // ordered: RSV_DISTINCT_ORDERED semantics (exact sequential replay; see rsv_distinct.hip)
    bool ordered = false;
    int64_t seen = 0;  // elements sampled so far (chunk sizing)
    SpecPublish spec;
    // Log retention (rsv_retain_log / rsv_export_log): `retain` is the caller's opt-in, `arch_ok` says
    // the host archive still holds every candidate consumed since creation, `merged` that the log
    // describes the history before a merge (sampling again drops it).
    bool retain = false;
    bool arch_ok = true;
    bool merged = false;

    virtual ~DistinctEngine() = default;
    virtual void set_timer(KernelTimer* t) = 0;
    virtual int sample_device(const void* keys, const int64_t* hashes, int64_t n, hipStream_t st) = 0;
    virtual int64_t size() const = 0;
    // RSV_DISTINCT_ORDERED: bring the set arrays to the reference's set (host replay of the logged
    // candidates when the tie bucket requires it); a no-op otherwise.  Before size / export / publish.
    virtual int finalize(hipStream_t st) = 0;
    virtual const void* keys_dev() const = 0;  // the current set's keys (size() of them)
    // the set's keys into coherent host memory (device-mapped pointer) + flag = gen
    virtual int publish(void* dst_host_dev, uint32_t* flag_dev, uint32_t gen, hipStream_t st) = 0;
    // Speculative publication (large batches): the next sample_device enqueues the merged set's
    // publication into dst_host_dev + flag_dev (generation ++*gen_counter) right behind its merge;
    // spec_take says whether the last one holds the batch's final set (its generation in *gen) and
    // clears the target.
    virtual void spec_target(void* dst_host_dev, uint32_t* flag_dev, uint32_t* gen_counter) = 0;
    virtual int64_t spec_min() const = 0;  // smallest batch that publishes speculatively
    bool spec_take(uint32_t* gen) { return spec.take(gen); }
    // copies the set (ascending hash) to device buffers; either may be null
    virtual int export_set(void* keys_dev, int64_t* hash_dev, hipStream_t st) = 0;
    // merge `parts` external (key, hash) runs (device; run p at p * part_len) into the set
    virtual int merge_parts(const void* keys_dev, const int64_t* hash_dev, const int64_t* part_n, int32_t parts,
                            int64_t part_len, hipStream_t st) = 0;
    virtual void info(int32_t* ordered, int32_t* tied, int32_t* retained, int64_t* size, int64_t* max_hash,
                      int64_t* log_entries, int64_t* sched_passes, int64_t* sched_fallbacks) const = 0;
    // ordered samplers: every logged candidate with h < bound (all of them for bound = INT64_MAX) in
    // arrival order into host buffers; the exact replay of a concatenated candidate run
    virtual int log_export(int64_t bound, int64_t* out_h, void* out_k, int64_t cap, int64_t* out_n,
                           hipStream_t st) = 0;
    virtual int log_merge(const int64_t* h, const void* keys, int64_t n, int64_t seen, hipStream_t st) = 0;
    // packed rows [keys as int64 words (k) | hashes (k) | n, count, tied, max_hash, log_retained, ordered]:
    // export of the set (count = the handle's element count), and the device merge of `parts` rows into
    // the set -- a Long / Int engine enqueues it without a host wait; `rows` must stay valid until the
    // next call on the engine, which settles the merge (settle; every other call settles first)
    virtual int export_row(int64_t* row, int64_t count, hipStream_t st) = 0;
    virtual int merge_rows(const int64_t* rows, int32_t parts, int64_t stride, hipStream_t st) = 0;
    virtual int settle(hipStream_t st) = 0;
    // ordered samplers: keep every replayed candidate on the host for rsv_export_log (opt-in);
    // switched on after sampling, the log is not retained; switched off, the archive goes
    void retain_log(bool on) {
        if (on && !retain && seen > 0) arch_ok = false;  // earlier candidates are gone
        retain = on;
        if (!on) drop_archive();
    }

    bool retained() const { return ordered && retain && arch_ok; }  // rsv_export_log can serve the log
    // rsv_export_log's precondition: RSV_OK, or RSV_E_UNSUPPORTED with the reason as the last error
    int log_export_check() const;

    virtual void drop_archive() = 0;  // release the host archive (retain_log(false))
};

// The engine for a key width: Long (8), Int (4) or byte keys (16..256, a multiple of 8; hashes
// precomputed, or UUID.hashCode of 16-byte rows for kHashUuid).  Null with *status set on failure.
DistinctEngine* distinct_create(int32_t k, int key_width, int hash_kind, int64_t r0, int64_t r1, bool ordered,
                                int* status);
// distinct_create's byte-key case: WideDistinct is defined in rsv_wide.hip, so its construction is too
// (src: kWideSrcHashes or kWideSrcUuid)
DistinctEngine* new_wide_distinct(int32_t k, int key_width, int src, int64_t r0, int64_t r1, bool ordered,
                                  int* status);

// ---- distinct for any B: the hash-only candidate pass (rsv_objects.hip) ---------------------------
// The engine sees scrambled-hash inputs only; the caller keeps the elements and replays RandomValues
// over the returned candidates.  hashes: device (on_device) or host memory; seen = the elements
// before the batch.  Every call completes its device work before it returns.
struct ObjDistinct;
ObjDistinct* obj_create(int32_t k, int64_t r0, int64_t r1, int* status);
void obj_destroy(ObjDistinct* d);
void obj_set_timer(ObjDistinct* d, KernelTimer* t);  // brackets obj_filter
int obj_candidates(ObjDistinct* d, const int64_t* hashes, int64_t n, bool on_device, int64_t seen, hipStream_t st,
                   int64_t* n_cand);
int64_t obj_pending_candidates(const ObjDistinct* d);
// the pending batch's candidates (offsets ascending, scrambled hashes) into host buffers
int obj_read(ObjDistinct* d, int64_t* offsets_host, int64_t* hashes_host, hipStream_t st);
// accept the pending batch (the caller's replica: its size and largest hash) / drop it
void obj_commit(ObjDistinct* d, int64_t set_size, int64_t max_hash);
void obj_abort(ObjDistinct* d);

}  // namespace rsv
