/*
 * reservoir_hip.h -- C ABI of libreservoir_hip.so, the MI355X (gfx950) reservoir-sampling engine.
 *
 * This is the drop-in boundary behind the lgbt.princess.reservoir API.  Every entry point names
 * the reference interface it replaces (paths relative to NthPortal/reservoir):
 *   S  = core/src/main/scala/lgbt/princess/reservoir/Sampler.scala
 *   SI = akka-stream/src/main/scala/lgbt/princess/reservoir/akkasupport/SampleImpl.scala
 * A Scala binding (Panama FFM downcalls or JNI) is shown in INTEGRATION.md.
 *
 * Conventions
 *   - plain C: no C++ or torch types; opaque handle; every call returns rsv_status.
 *   - keys are primitive fixed-width values (Int -> key_width 4, Long -> key_width 8, or
 *     fixed-width byte keys of 16..256 bytes in steps of 8: java.util.UUID -> 16 bytes laid out
 *     [mostSigBits | leastSigBits] as little-endian Longs, or a case class of primitives) that the
 *     host extracted with the sampler's `map` (S:115-116: map may be called more than k times).
 *     Byte keys must have value equality (B.equals = equal bytes): a distinct sampler dedups by
 *     the bytes, as the reference's `elements.contains` (S:398, S:403) does for such a B.  An
 *     Array[Byte] (reference equality in a Scala Set) must stay on the JVM sampler.
 *   - "device" pointers are HIP device pointers on the handle's device; "host" pointers are
 *     ordinary (pageable or pinned) memory.  The caller owns every buffer it passes in.
 *   - one handle is single-threaded (S:18-19); distinct handles are independent.
 *   - errors: rsv_last_error() returns a thread-local message for the last failing call.
 */
#ifndef RESERVOIR_HIP_H
#define RESERVOIR_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RSV_ABI_VERSION 1

/* Status codes; a JVM binding maps them 1:1 onto the reference's exceptions. */
typedef enum rsv_status {
    RSV_OK = 0,
    RSV_E_ILLEGAL_ARGUMENT = 1, /* IllegalArgumentException: k <= 0 or k > Int.MaxValue-2 (S:80-81) */
    RSV_E_ILLEGAL_STATE = 2,    /* IllegalStateException "use of sampler after calling `result()`" (S:186) */
    RSV_E_NULL_POINTER = 3,     /* NullPointerException: a required pointer is NULL (S:82, S:94) */
    RSV_E_DEVICE = 4,           /* HIP runtime / kernel failure -> RuntimeException (fails the akka Future, SI:43-46) */
    RSV_E_OUT_OF_MEMORY = 5,    /* device or pinned allocation failed -> OutOfMemoryError */
    RSV_E_UNSUPPORTED = 6       /* request this build does not implement (message says which): a key_width
                                 * other than 4, 8, 16..256 in steps of 8; a hash kind byte keys lack */
} rsv_status;

typedef enum rsv_kind {
    RSV_KIND_ELEMENTS = 0, /* Sampler.apply   (S:128-136): equal-probability sample, duplicates kept */
    RSV_KIND_DISTINCT = 1  /* Sampler.distinct (S:171-180): bottom-k over the scrambled hash     */
} rsv_kind;

typedef enum rsv_engine {
    /* Algorithm R, data-parallel: element i >= k replaces slot j_i = floor(U_i (i+1) / 2^64) when
     * j_i < k, U_i a counter-based Philox4x32-10 draw of (seed, stream_id, i) (draw
     * format R2).  Bit-identical for any batching and any index-range split over GPUs. */
    RSV_ENGINE_PHILOX_R = 0,
    /* The reference's own Algorithm L (S:224-246) driven by java.util.Random(seed), exactly as
     * SamplerTest.useConsistentRandom seeds it; the eviction events are replayed on the GPU.
     * Bit-identical to the reference Sampler for the same seed. */
    RSV_ENGINE_JAVA_L = 1
} rsv_engine;

typedef enum rsv_hash_kind {
    RSV_HASH_DEFAULT = 0,     /* B#hashCode().toLong (S:75): JAVA_INT for key_width 4, JAVA_LONG for 8,
                               * java.util.UUID.hashCode for 16 ((int)(hilo >>> 32) ^ (int)hilo, hilo =
                               * msb ^ lsb); other byte widths take PRECOMPUTED */
    RSV_HASH_IDENTITY = 1,    /* hash = key as a signed Long (a bijection: bit-exact distinct sets) */
    RSV_HASH_JAVA_LONG = 2,   /* java.lang.Long.hashCode: (int)(v ^ v>>>32), sign-extended */
    RSV_HASH_JAVA_INT = 3,    /* java.lang.Integer.hashCode: v, sign-extended */
    RSV_HASH_PRECOMPUTED = 4  /* caller passes int64 hashes beside the keys (arbitrary JVM `hash`) */
} rsv_hash_kind;

/* How a DISTINCT sampler resolves elements whose scrambled hashes tie.  The reference keeps the
 * elements of its max-heap (S:389-409): with an injective hash that is the bottom-k of the hashes,
 * independent of arrival order; with a colliding hash (Long#hashCode folds to 32 bits) the members of
 * the boundary hash bucket depend on arrival order and on PriorityQueue tie-breaking. */
typedef enum rsv_distinct_order {
    /* ORDERED for RSV_HASH_JAVA_LONG / PRECOMPUTED (may collide), SET for IDENTITY / JAVA_INT */
    RSV_DISTINCT_AUTO = 0,
    /* bottom-k by (hash, key): order-independent and mergeable across GPUs; equal to the
     * reference's set whenever no distinct elements share the final maximum hash */
    RSV_DISTINCT_SET = 1,
    /* the reference's sequential semantics for any hash: the GPU filters each chunk of the batch
     * against the current maximum (a superset of what the reference inserts), the host replays
     * the survivors in arrival order through an exact RandomValues replica (heap + hash set) */
    RSV_DISTINCT_ORDERED = 2
} rsv_distinct_order;

typedef enum rsv_mem { RSV_MEM_HOST = 0, RSV_MEM_DEVICE = 1 } rsv_mem;

typedef struct rsv_config {
    uint32_t struct_size;     /* = sizeof(rsv_config) */
    int32_t  kind;            /* rsv_kind */
    int32_t  max_sample_size; /* k: S:130 maxSampleSize / S:173 */
    int32_t  key_width;       /* 4 (Int), 8 (Long), or fixed-width byte keys: a multiple of 8 in 16..256 */
    int32_t  reusable;        /* S:130/S:173 reusable: result() may be called repeatedly (S:353-381, S:430-433) */
    int32_t  pre_allocate;    /* S:130 preAllocate: accepted; device slots are always preallocated */
    int32_t  engine;          /* rsv_engine (ELEMENTS only) */
    int32_t  hash_kind;       /* rsv_hash_kind (DISTINCT only) */
    int32_t  device;          /* HIP device ordinal; -1 = the calling thread's current device */
    int32_t  distinct_order;  /* rsv_distinct_order (DISTINCT only) */
    uint64_t seed;            /* PHILOX_R: Philox key; JAVA_L / DISTINCT: java.util.Random seed (S:199, S:385-388) */
    uint64_t stream_id;       /* PHILOX_R: Philox stream (independent sampler id) */
} rsv_config;

typedef struct rsv_sampler rsv_sampler;

/* Library / error plumbing */
int32_t     rsv_abi_version(void);
const char* rsv_last_error(void);
const char* rsv_status_string(rsv_status s);
rsv_status  rsv_config_init(rsv_config* cfg); /* defaults: ELEMENTS, k=1, key_width 8, PHILOX_R */

/* Construction = Sampler.apply / Sampler.distinct (S:128-136, S:171-180) incl. validation
 * validateSharedParams (S:77-83).  `map`/`hash` nullness is checked on the JVM side. */
rsv_status rsv_create(const rsv_config* cfg, rsv_sampler** out);
void       rsv_destroy(rsv_sampler* s);

/* Sampler.sample(element) (S:37-38; RandomElements.sampleImpl S:248-259; RandomValues.sample
 * S:394-409).  The key is staged in a pinned host batch and flushed to the GPU in bulk; `hash`
 * is read only for RSV_HASH_PRECOMPUTED (may be NULL otherwise). */
rsv_status rsv_sample(rsv_sampler* s, const void* key, const int64_t* hash);

/* Zero-copy pinned batches (the north-star JVM path: keys extracted straight into pinned memory,
 * e.g. a Panama MemorySegment over the returned pointer).  rsv_stage_acquire returns the free tail
 * of the handle's current pinned staging buffer -- room for *capacity keys (and hashes, for
 * RSV_HASH_PRECOMPUTED, else *hashes_out = NULL) -- and rsv_stage_commit(n) appends the first n
 * keys written there, exactly as n rsv_sample calls would.  A full buffer is flushed to the GPU
 * asynchronously and the next acquire returns the other buffer (double buffering).  The pointers
 * are valid until the next call on the handle. */
rsv_status rsv_stage_acquire(rsv_sampler* s, void** keys_out, int64_t** hashes_out, int64_t* capacity);
rsv_status rsv_stage_commit(rsv_sampler* s, int64_t n);

/* Sampler.sampleAll(elements) (S:49-50, S:289-316): appends n keys at global indices
 * [count, count+n).  mem says where `keys` (and `hashes`) live.  Identical results to n calls of
 * rsv_sample, for any split into batches (SamplerTest.scala:117-142). */
rsv_status rsv_sample_batch(rsv_sampler* s, const void* keys, int64_t n, int32_t mem,
                            const int64_t* hashes);

/* Sampler.sampleAll over a known-size IndexedSeq WITHOUT its keys (sampleAllImpl S:289-312 ->
 * sampleIndexed S:261-273, which reads only seq(nextSampleCount - count - 1) per eviction): the n
 * elements at global indices [count, count+n) are sampled by index alone -- a draw depends only on
 * the index (PHILOX_R), or the eviction events come from java.util.Random (JAVA_L) -- so only the
 * elements that end up in the reservoir need `map`.  slot_offsets_host[k] receives, per slot, the
 * offset in [0, n) of the element that now holds it (fill phase S:253-255 included), or -1 where
 * the slot did not change.  The caller maps exactly those elements (seq(offset)) and passes their
 * keys to rsv_fill_slots; until then (or rsv_abort_indexed / rsv_commit_indexed) every other sampling,
 * staging, result, seek, export and merge call on the handle returns RSV_E_ILLEGAL_STATE and leaves
 * it as it was (the plumbing calls -- see "Plumbing calls" below -- are still taken).
 * ELEMENTS samplers only (Sampler.distinct maps every element: its sampleAll is the trait default,
 * S:50).  One K1 pass over the index range, k x 8 B back over PCIe -- no key crosses the link.
 * `map` then runs once per slot that changed, on its final holder: for a pure map the reservoir is
 * the reference's.  The reference calls map on every fill-phase element and on every evicting
 * element in order (S:241, :244, :269), so an impure map (side effects, call counts) or one that
 * throws midway observes fewer calls here; such a map belongs on the keyed path (rsv_sample_batch
 * with its keys), and a throw while keys are owed is undone with rsv_abort_indexed. */
rsv_status rsv_sample_indexed(rsv_sampler* s, int64_t n, int64_t* slot_offsets_host);
/* The keys owed after rsv_sample_indexed: keys_host holds k keys in slot order; entry j is read
 * only where slot_offsets_host[j] >= 0 (the rest may be anything). */
rsv_status rsv_fill_slots(rsv_sampler* s, const void* keys_host);
/* Drop the pending rsv_sample_indexed batch (the caller's `map` threw on an element it owed the
 * engine): the handle returns to its state before that call -- count, slots, result -- and takes
 * calls again; a binding then rethrows the exception, as the reference's sampleIndexed propagates
 * it (S:261-273).  The batch goes as a whole, where the reference keeps what it mapped before the
 * throw: after a throwing `map` the two differ in which of the batch's elements count.
 * RSV_E_ILLEGAL_STATE without a pending rsv_sample_indexed. */
rsv_status rsv_abort_indexed(rsv_sampler* s);
/* Accept the pending rsv_sample_indexed batch without keys: the caller keeps the elements itself.
 * For a `Sampler[A, B]` whose B has no fixed-width key (a case class, a String, any JVM object:
 * S:128-136 takes any B with a ClassTag), the binding holds the k-slot array of B references
 * (RandomElements.samples, S:200-202) and writes slots[j] = map(seq(slot_offsets[j])) (or the
 * already mapped element of a buffered batch) -- the engine decides WHICH element each slot holds
 * from the indices alone and never sees a B.  Afterwards the handle's slots hold no keys:
 * rsv_result / rsv_result_device / rsv_export_* return RSV_E_ILLEGAL_STATE, and every further batch
 * must be index-only (rsv_sample_indexed + rsv_commit_indexed or rsv_abort_indexed).
 * ELEMENTS samplers; RSV_E_ILLEGAL_STATE without a pending rsv_sample_indexed. */
rsv_status rsv_commit_indexed(rsv_sampler* s);

/* Sampler.distinct for ANY B (S:171-180; RandomValues S:383-412) WITHOUT the elements: the hash-only
 * candidate pass.  RandomValues.sample needs the element itself only for `elements.contains` (S:398,
 * S:403); the admission test `elemHash < maxHash` (S:403) needs only the hash.  The caller passes
 * hash(map(x)) of the next n elements, 8 B each, and keeps the reference's heap and Set[B] itself; the
 * engine returns the batch offsets the reference could still admit -- a superset of its admissions,
 * in arrival order, with their scrambled hashes (S:396) -- and the caller replays RandomValues.sample
 * over those elements only.  The engine never sees a B: it bounds maxHash by the k-th smallest
 * DISTINCT scrambled hash seen so far (k distinct hashes mean k distinct elements, so the reference's
 * set is full and its maxHash is no larger; DESIGN.md has the proof) and by the caller's own maxHash
 * as of the last commit.  Every repeat of a current member comes back as a candidate (its hash is
 * under the bound; the caller's `contains` rejects it), and while fewer than k distinct hash values
 * were seen and the caller's set is not full every element is a candidate: then the cost is the
 * reference's plus a copy.
 * A DISTINCT handle with RSV_HASH_PRECOMPUTED (key_width is ignored; another hash kind returns
 * RSV_E_UNSUPPORTED).  The first call on a handle that has sampled nothing makes it index-only, as
 * rsv_commit_indexed does: keyed calls, rsv_result*, rsv_export_*, rsv_merge_*, rsv_get_distinct_info
 * and the log calls then return RSV_E_ILLEGAL_STATE; on a handle that already holds keys this call
 * returns RSV_E_ILLEGAL_STATE.  mem says where `hashes` live (host hashes travel through pinned
 * staging); n == 0 is a valid empty batch; *n_cand receives the candidate count.  The call returns
 * with its device work done, on a caller stream too.  Until rsv_candidates_commit or
 * rsv_candidates_abort every call but those two, rsv_candidates_read, rsv_is_open, rsv_count,
 * rsv_get_stream and rsv_destroy returns RSV_E_ILLEGAL_STATE.  Multi-GPU merging of such samplers is not provided. */
rsv_status rsv_distinct_candidates(rsv_sampler* s, const int64_t* hashes, int64_t n, int32_t mem, int64_t* n_cand);
/* The pending batch's candidates into host buffers of cap entries: offsets strictly ascending in
 * [0, n), the scrambled hash of each beside it (the elemHash of S:396).  The same for any order the
 * device found them in.  RSV_E_ILLEGAL_ARGUMENT when cap is below the count; may be repeated. */
rsv_status rsv_candidates_read(rsv_sampler* s, int64_t* offsets_host, int64_t* hashes_host, int64_t cap);
/* Accept the pending batch: rsv_count grows by its n.  set_size and max_hash are the caller's
 * replica after replaying the candidates (samples.size and maxHash, S:389-392): with set_size == k
 * the next batch is filtered against min(the engine's bound, max_hash), which keeps a hash with
 * fewer than k distinct values efficient across batches; max_hash is not read otherwise. */
rsv_status rsv_candidates_commit(rsv_sampler* s, int64_t set_size, int64_t max_hash);
/* Drop the pending batch (the caller's `map` or `hash` threw): count, the engine's hash shadow and
 * its bound are as before the batch, and the next batch's candidates are what they would have been
 * without it.  A binding then rethrows, as the reference's sample propagates it (S:394-395). */
rsv_status rsv_candidates_abort(rsv_sampler* s);

/* Sampler.result() (S:59-60; resultImpl S:318-331; RandomValues.result S:411).  Writes
 * min(count, k) keys (ELEMENTS: slot order, which is part of the reference result) or the distinct
 * set (DISTINCT: ascending scrambled hash; the reference's order is HashSet order) into host
 * memory `out` of `cap` keys, and the count into *out_n.  Single-use samplers close (S:345-350):
 * every later sampling, staging, result, seek, export, merge and distinct-info / log call returns
 * RSV_E_ILLEGAL_STATE (checkOpen comes before any other work, S:185-186); the plumbing calls below
 * stay valid until rsv_destroy. */
rsv_status rsv_result(rsv_sampler* s, void* out, int64_t cap, int64_t* out_n);
/* Same, into device memory (no host round trip of the keys). */
rsv_status rsv_result_device(rsv_sampler* s, void* out_dev, int64_t cap, int64_t* out_n);
/* Same as rsv_result, without the host copy: a single-use sampler whose result is published into
 * its pinned result buffer (ELEMENTS and DISTINCT, k x key_width <= 1 MB) hands that buffer over.
 * *buf holds the *out_n keys (as rsv_result writes them) and belongs to the caller until
 * rsv_host_release(*buf); the sampler closes as after rsv_result.  The copy it saves is a read of
 * memory the GPU just wrote (k = 65536: ~22 us from DRAM).  Anything else (reusable samplers, larger
 * results) returns RSV_E_UNSUPPORTED with the sampler untouched: call rsv_result instead. */
rsv_status rsv_result_take(rsv_sampler* s, void** buf, int64_t* out_n);
void       rsv_host_release(void* buf);

int32_t    rsv_is_open(const rsv_sampler* s); /* Sampler.isOpen (S:67, S:193, S:380) */
int64_t    rsv_count(const rsv_sampler* s);   /* elements sampled so far (S:203) */

/* Plumbing calls: rsv_is_open, rsv_count, rsv_get_stream, rsv_set_stream, rsv_set_resolve_stream,
 * rsv_synchronize, rsv_profile_enable, rsv_profile_read and rsv_destroy neither read nor change the
 * sample, so the lifecycle does not gate them: they are taken on a closed single-use handle (a
 * caller still synchronizes, reads its kernel times or hands the stream back after result()), while
 * keys are owed after rsv_sample_indexed, and after rsv_commit_indexed.  The one exception is a
 * pending candidate batch (rsv_distinct_candidates): until its commit or abort the calls among them
 * that return a status -- rsv_set_stream, rsv_set_resolve_stream, rsv_synchronize, rsv_profile_* --
 * return RSV_E_ILLEGAL_STATE, as that call's text says.  rsv_count includes the keys staged by
 * rsv_sample / rsv_stage_commit; a closed handle keeps reporting its final count. */

/* Streams: every handle owns a non-blocking HIP stream; a caller may substitute its own.  On the
 * handle's own stream every call returns with its device work finished (ownership of caller
 * buffers returns at once); on a caller stream, calls that take or fill DEVICE buffers
 * (rsv_sample_batch with RSV_MEM_DEVICE, rsv_export_state, rsv_merge_state, rsv_result_device) are
 * stream-ordered and return without a host wait.  rsv_set_stream orders the work already queued
 * on the previous stream before the new stream's next work (an event wait, no host wait). */
rsv_status rsv_set_stream(rsv_sampler* s, void* hip_stream);
void*      rsv_get_stream(const rsv_sampler* s);
/* Pipelining several samplers on one stream (ELEMENTS, batches whose K1 runs as its own dispatch:
 * > 2^27 draws): each batch's slot resolve and result publication (a one-workgroup dispatch of a few
 * microseconds) run on `hip_stream` instead, after the batch's K1 (an event), so the NEXT sampler's
 * K1 on the handle's stream does not wait behind them.  The handle's own later work waits for them
 * (an event), and rsv_result waits for the publication as always.  The keys of such a batch are read
 * on `hip_stream`: the caller keeps them unchanged until rsv_result (or rsv_synchronize) returns.
 * NULL = resolve on the handle's stream (the default). */
rsv_status rsv_set_resolve_stream(rsv_sampler* s, void* hip_stream);
rsv_status rsv_synchronize(rsv_sampler* s);

/* Kernel timing: while enabled, HIP events bracket every launch of the handle's hot kernel (K1
 * for PHILOX_R, the event replay K1' for JAVA_L, the K3 filter for DISTINCT, the hash-only filter
 * of rsv_distinct_candidates) on its stream.
 * rsv_profile_read synchronizes and returns the summed kernel time and the launch count. */
rsv_status rsv_profile_enable(rsv_sampler* s, int32_t on);
rsv_status rsv_profile_read(rsv_sampler* s, double* total_ms, int64_t* launches);
/* Process-wide form (bench.py): while on, the hot-kernel launches of every ELEMENTS handle without
 * its own timing are bracketed by events kept in one process-wide list, so a timed loop that creates and
 * closes samplers pays no per-handle enable/read; rsv_profile_global_read synchronizes those events,
 * returns the totals since the last read and starts a new window.  `on` = 0 turns it off; N > 0
 * times every N-th launch from now on (1 = every launch; a larger N keeps the event packets off
 * most launches of a tight loop while the average stays a live measurement). */
rsv_status rsv_profile_global(int32_t on);
rsv_status rsv_profile_global_read(double* total_ms, int64_t* launches);

/* ---- Multi-GPU (index-range split of one stream; RSV_ENGINE_PHILOX_R / DISTINCT) ---------- */
/* Declare that the next sampled element has global index `index` (>= count): the elements in
 * between belong to other ranks.  PHILOX_R only. */
rsv_status rsv_seek(rsv_sampler* s, int64_t index);
/* Export the partial state into caller device buffers.
 *   ELEMENTS: idx_dev[k] = global index held by each slot (-1 = empty), keys_dev[k].
 *   DISTINCT: up to k (key, hash) pairs in ascending hash order, *out_n = count; idx_dev unused. */
rsv_status rsv_export_state(rsv_sampler* s, int64_t* idx_dev, void* keys_dev, int64_t* hash_dev,
                            int64_t* out_n);
/* Merge `parts` exported states (laid out back to back, `part_len` entries each, e.g. gathered
 * from every rank) into this sampler.  ELEMENTS: per slot the largest global index wins (last
 * writer).  DISTINCT: bottom-k of the union by (hash, key).  total_count sets the merged element
 * count.  An RSV_DISTINCT_ORDERED sampler merges the same way, which is the reference's set
 * unless the boundary hash bucket is oversubscribed (rsv_get_distinct_info `tied`); then the
 * exact set comes from rsv_export_log / rsv_merge_log below (reservoir_amd/distributed.py does
 * both).  With an injective hash the result is always identical. */
rsv_status rsv_merge_state(rsv_sampler* s, const int64_t* idx_dev, const void* keys_dev,
                           const int64_t* hash_dev, const int64_t* part_n_host, int32_t parts,
                           int64_t part_len, int64_t total_count);

/* ---- Exact multi-rank merge of ORDERED distinct samplers (the reference's default hash) ----- *
 * A stream split across ranks in order (rank r holds the r-th contiguous piece) is, to the
 * reference, one sequential RandomValues run (S:394-409): under a colliding hash the members of the
 * boundary hash bucket depend on that run's arrival order and heap ties.  rsv_merge_state gives the
 * (hash, key) bottom-k of the union; when rsv_get_distinct_info then reports `tied` (or a rank's own
 * set was tied at the merged maximum), the exact set comes from replaying every rank's logged
 * candidates in rank order: a rank's log is a superset of what the global run admits from its
 * piece (its local maximum is never below the global one), and the global heap's maximum inside
 * rank r's piece is below the k-th smallest hash of the pieces before it, so rank r exports only
 * candidates under that bound (reservoir_amd/distributed.py computes the bounds). */
typedef struct rsv_distinct_info {
    uint32_t struct_size;  /* = sizeof(rsv_distinct_info) */
    int32_t  ordered;      /* RSV_DISTINCT_ORDERED sampler */
    int32_t  tied;         /* set full and more distinct elements share its maximum hash than it keeps
                            * (ordered: of those the reference could admit; after rsv_merge_state: of
                            * the merged union) -- the boundary bucket needs the arrival order */
    int32_t  log_retained; /* ordered: rsv_export_log can return every candidate logged since creation */
    int64_t  size;         /* set size */
    int64_t  max_hash;     /* the set's largest scrambled hash (INT64_MIN when empty) */
    int64_t  log_entries;  /* ordered: upper bound on rsv_export_log's count */
    int64_t  sched_passes;    /* ordered: batches taken by one verified scheduled pass */
    int64_t  sched_fallbacks; /* ordered: scheduled passes that failed verification or overflowed and
                               * left the batch to the chunk loop (the set restored) */
} rsv_distinct_info;
rsv_status rsv_get_distinct_info(rsv_sampler* s, rsv_distinct_info* out);
/* Keep every logged candidate on the host for rsv_export_log (ORDERED samplers; off by default: the
 * archive holds 12-16 B per replayed candidate, up to 2^27 of them).  Call it before the first
 * sample -- switched on later, the log is reported as not retained. */
rsv_status rsv_retain_log(rsv_sampler* s, int32_t on);
/* Every logged candidate with scrambled hash < bound (all of them for bound = INT64_MAX), in
 * arrival order, into host buffers of cap entries (keys as key_width values); *out_n = the count
 * (RSV_E_ILLEGAL_ARGUMENT when it exceeds cap; cap = 0 is a count-only query, the buffers may be
 * NULL).  RSV_E_UNSUPPORTED if the log was not retained (rsv_retain_log).
 * Stays available after rsv_merge_state until the sampler samples again. */
rsv_status rsv_export_log(rsv_sampler* s, int64_t bound, int64_t* hashes_host, void* keys_host, int64_t cap,
                          int64_t* out_n);
/* Replace the state by a fresh RandomValues replica run over n candidates (host, in global arrival
 * order: rank 0's export, then rank 1's, ...), as if the sampler had seen the whole stream. */
rsv_status rsv_merge_log(rsv_sampler* s, const int64_t* hashes_host, const void* keys_host, int64_t n,
                         int64_t total_count);

/* Packed form of rsv_export_state / rsv_merge_state, the one-collective combine of
 * reservoir_amd/distributed.py.  One kernel, no host wait on a caller stream.
 *   ELEMENTS: row_dev[0..k) = global index per slot (-1 = empty), row_dev[k..2k) = the slot's key
 *     widened to int64 (sign-extended for 4-byte keys); for wide keys (key_width > 8) the k keys
 *     follow as key_width/8 int64 words each.
 *   DISTINCT: [keys (k) | scrambled hashes (k) | n, count, tied, max_hash, log_retained, ordered] --
 *     the set ascending by (hash, key), n entries valid; keys widened to int64 (2k + 6 words), or for
 *     byte keys key_width / 8 words each (k (key_width / 8 + 1) + 6 words, ascending by (hash, key
 *     words compared as unsigned 64-bit, word 0 first)). */
rsv_status rsv_export_packed(rsv_sampler* s, int64_t* row_dev);
/* Merge `parts` packed rows (row p at rows_dev + p*row_stride, row_stride >= the row length), e.g. the output
 * of an all-gather of every rank's rsv_export_packed row.
 *   ELEMENTS: per slot the largest global index wins.
 *   DISTINCT: the bottom-k by (hash, key) of the union with the sampler's set, on the device (four
 *     kernels, no host wait: the set's size and tie state are read back at the next call on the
 *     handle); `tied` as rsv_merge_state.  The rows are the caller's again once the merge has run
 *     in stream order (the engine keeps its own copy for a degenerate hash that overflows the
 *     merge's buckets, redone at the next call).  Byte-key DISTINCT samplers merge before the call
 *     returns (the host reads the rows' meta words). */
rsv_status rsv_merge_packed(rsv_sampler* s, const int64_t* rows_dev, int32_t parts, int64_t row_stride,
                            int64_t total_count);

/* ---- Stateless batch entry points --------------------------------------------------------- */
/* Segmented sampling: S independent Algorithm-R samplers (no reference counterpart; = S separate
 * Sampler instances, S:196-332).  Stream s samples keys_dev[offsets[s] .. offsets[s+1]) with
 * Philox stream id stream_base + s and writes out_dev[s*k .. s*k+k) (slot order; slots >=
 * counts[s] are zero) and counts_dev[s] = min(len, k).  All pointers are device pointers. */
rsv_status rsv_sample_segmented(const void* keys_dev, const int64_t* offsets_dev, int64_t num_streams,
                                int32_t key_width, int32_t k, uint64_t seed, uint64_t stream_base,
                                void* out_dev, int64_t* counts_dev, void* hip_stream);

/* Segmented sampling, resumed: long-lived Algorithm-R samplers advanced by one launch per batch.  The
 * state is the caller's device memory: state_keys_dev[num_states*k] (key_width values),
 * state_idx_dev[num_states*k] (int64: the global index of each slot's last writer, -1 = empty slot,
 * the convention of rsv_export_state) and state_next_dev[num_states] (int64: one past the highest
 * index the row has consumed).  A fresh state is idx = -1, next = 0, keys anything.
 * For stream (seed, stream id) let slot(i) = i for i < k, else the draw j_i (format R2) if j_i < k;
 * slot j of a row that has consumed the index set I holds the key of max{i in I : slot(i) = j}.
 * That max is associative and commutative: any sequence of updates and merges whose pieces cover
 * [0, n) leaves keys and idx exactly as one rsv_sample_segmented launch over the whole stream does.
 * Segment b = keys_dev[offsets[b] .. offsets[b+1]) goes into row r = stream_ids_dev[b], or r = b when
 * stream_ids_dev is NULL (then num_segments <= num_states), with Philox stream id stream_base + r.
 * Its first element has global index bases_dev[b], or state_next_dev[r] when bases_dev is NULL.  A slot
 * is written (key and idx) only where the segment's last writer w -- fill indices < k included -- has
 * state_idx < w; state_next[r] = max(state_next[r], base + len).  A segment whose id lies outside
 * [0, num_states), whose base is negative or that is empty is skipped; rows that no segment names
 * are not touched.  The ids of one launch must be distinct (the caller's contract).
 * key_width 4 or 8; 1 <= k <= 15104 (the 64-bit winner table of the one-workgroup-per-stream form
 * has to fit LDS; larger: RSV_E_UNSUPPORTED).  Stateless and stream-ordered on hip_stream: no host
 * wait, no allocation.  All pointers are device pointers. */
rsv_status rsv_sample_segmented_update(const void* keys_dev, const int64_t* offsets_dev, const int64_t* stream_ids_dev,
                                       const int64_t* bases_dev, int64_t num_segments, int64_t num_states,
                                       int32_t key_width, int32_t k, uint64_t seed, uint64_t stream_base,
                                       void* state_keys_dev, int64_t* state_idx_dev, int64_t* state_next_dev,
                                       void* hip_stream);

/* Combine of segmented sampler states: part_* are `parts` states laid back to back
 * ([parts][num_states][k] keys and idx, [parts][num_states] next: what an all-gather of every rank's
 * state tensors gives).  Per slot the largest idx among the row and the parts wins (a slot that no
 * part beats is not written); next becomes the max over the row and the parts.  All parts and the
 * state must come from the same seed and stream_base (the caller's contract).  Stateless and
 * stream-ordered like the update. */
rsv_status rsv_sample_segmented_merge(const void* part_keys_dev, const int64_t* part_idx_dev,
                                      const int64_t* part_next_dev, int32_t parts, int64_t num_states,
                                      int32_t key_width, int32_t k, void* state_keys_dev, int64_t* state_idx_dev,
                                      int64_t* state_next_dev, void* hip_stream);

/* Segmented sampling over fixed-width byte keys (java.util.UUID, case classes of primitives): as
 * rsv_sample_segmented, the elements being rows of key_width bytes -- a multiple of 8 in 16..256;
 * offsets_dev counts rows, and rows_dev and out_rows_dev are 8-byte aligned.  Stream s samples the rows
 * [offsets[s], offsets[s+1]) with Philox stream id stream_base + s and writes the k rows at
 * out_rows_dev[(s*k + j) * key_width ..) (slot order: slot j holds the row at its last writer, row j of
 * the stream where no replacement hit it, zeros for j >= counts[s]) and counts_dev[s] = min(len, k):
 * stream s is bit-identical to a single ELEMENTS handle of that key_width on RSV_ENGINE_PHILOX_R fed the
 * same rows.  Every slot and every count is written.  key_width 4 or 8: RSV_E_UNSUPPORTED (use
 * rsv_sample_segmented).  No row is read before its stream's winners are known; the gather moves
 * 16-byte granules where key_width % 16 == 0 and both buffers are 16-byte aligned, else 8-byte ones.
 * All pointers are device pointers. */
rsv_status rsv_sample_segmented_rows(const void* rows_dev, const int64_t* offsets_dev, int64_t num_streams,
                                     int32_t key_width, int32_t k, uint64_t seed, uint64_t stream_base,
                                     void* out_rows_dev, int64_t* counts_dev, void* hip_stream);

/* rsv_sample_segmented_update over byte keys: the state is state_rows_dev[num_states*k] rows of key_width
 * bytes, state_idx_dev and state_next_dev as there (a fresh state is idx = -1, next = 0, rows anything).
 * Segments, stream_ids_dev, bases_dev and the skipped segments as rsv_sample_segmented_update; a slot's
 * row is rewritten only where the segment's last writer or fill index is later than its idx, so any
 * sequence of updates and merges whose pieces cover [0, n) leaves rows and idx as one
 * rsv_sample_segmented_rows launch over the whole stream does.  rows_dev must not overlap the state; both
 * are 8-byte aligned.  key_width a multiple of 8 in 16..256 (4 or 8: RSV_E_UNSUPPORTED, use
 * rsv_sample_segmented_update); 1 <= k <= 15104 (larger: RSV_E_UNSUPPORTED).  Stateless and
 * stream-ordered on hip_stream: no host wait, no allocation. */
rsv_status rsv_sample_segmented_rows_update(const void* rows_dev, const int64_t* offsets_dev,
                                            const int64_t* stream_ids_dev, const int64_t* bases_dev,
                                            int64_t num_segments, int64_t num_states, int32_t key_width, int32_t k,
                                            uint64_t seed, uint64_t stream_base, void* state_rows_dev,
                                            int64_t* state_idx_dev, int64_t* state_next_dev, void* hip_stream);

/* rsv_sample_segmented_merge over byte keys: part_rows_dev is [parts][num_states][k] rows of key_width
 * bytes, part_idx_dev and part_next_dev as there.  Per slot the part with the largest idx wins if it
 * beats the state's, and its key_width bytes are copied (a slot that no part beats is not written); next
 * becomes the max over the row and the parts.  A state may be merged into itself.  Widths and k as
 * rsv_sample_segmented_rows_update. */
rsv_status rsv_sample_segmented_rows_merge(const void* part_rows_dev, const int64_t* part_idx_dev,
                                           const int64_t* part_next_dev, int32_t parts, int64_t num_states,
                                           int32_t key_width, int32_t k, void* state_rows_dev,
                                           int64_t* state_idx_dev, int64_t* state_next_dev, void* hip_stream);

/* The grouping pass: a micro-batch in arrival order, each element tagged with its state row, to the dense
 * CSR the segmented update entry points take.  ids_dev[i] (int64 for id_width 8, the stream_ids convention,
 * or int32 for id_width 4) is the state row of the batch's i-th element.  offsets_dev[num_states + 1]:
 * [offsets[r], offsets[r+1]) is row r's range in order_dev, empty for a row the batch does not name;
 * offsets[0] = 0.  order_dev[n]: order[offsets[r] + p] is the position in the batch of row r's p-th element
 * in arrival order.  An id outside [0, num_states) is not an error: those elements are dropped,
 * offsets[num_states] is the number of kept elements, and the dropped positions follow at
 * order[offsets[num_states] .. n) in arrival order, so order_dev is always a permutation of [0, n).
 * The result is a function of the input alone (a stable partition: no arrival order is decided by an
 * atomic).  Because the CSR is dense the number of rows present never reaches the host: the update
 * entry points take it with stream_ids_dev = NULL and num_segments = num_states, and skip the empty
 * segments.  Stream-ordered on hip_stream without a host wait; scratch of at most 12.25 bytes per element
 * comes from the stream-ordered allocator and returns to it.  Checked in this order, before anything
 * touches the device: offsets_dev NULL, then order_dev / ids_dev NULL with n > 0: RSV_E_NULL_POINTER;
 * n < 0 or num_states < 1: RSV_E_ILLEGAL_ARGUMENT; id_width not 4 or 8: RSV_E_UNSUPPORTED;
 * n > 2^31 - 1 (order_dev is int32) or num_states > 2^32 - 2: RSV_E_UNSUPPORTED.  n = 0 writes every
 * offset as 0. */
rsv_status rsv_group_by_stream(const void* ids_dev, int32_t id_width, int64_t n, int64_t num_states,
                               int64_t* offsets_dev, int32_t* order_dev, void* hip_stream);

/* rsv_sample_segmented_update through a permutation: segment b's p-th element is
 * keys_dev[order_dev[offsets[b] + p]] instead of keys_dev[offsets[b] + p]; everything else -- segments,
 * stream_ids_dev, bases_dev, the skipped segments, widths, k and the state -- is as there.  keys_dev holds
 * n_keys keys in arrival order and order_dev n_keys entries in [0, n_keys), what rsv_group_by_stream
 * writes; with its offsets, stream_ids_dev = NULL, bases_dev = NULL and num_segments = num_states this
 * is the by-id update.  order_dev is read only for the slots a segment replaces (at most k entries per
 * segment) and no other key is read or moved.  A slot whose entry lies outside [0, n_keys) is left as it
 * is, key and idx, rather than dereferenced.  order_dev NULL: RSV_E_NULL_POINTER. */
rsv_status rsv_sample_segmented_update_indirect(const void* keys_dev, int64_t n_keys, const int32_t* order_dev,
                                                const int64_t* offsets_dev, const int64_t* stream_ids_dev,
                                                const int64_t* bases_dev, int64_t num_segments, int64_t num_states,
                                                int32_t key_width, int32_t k, uint64_t seed, uint64_t stream_base,
                                                void* state_keys_dev, int64_t* state_idx_dev, int64_t* state_next_dev,
                                                void* hip_stream);

/* rsv_sample_segmented_rows_update through a permutation, as rsv_sample_segmented_update_indirect:
 * segment b's p-th row is row order_dev[offsets[b] + p] of rows_dev (n_rows rows of key_width bytes). */
rsv_status rsv_sample_segmented_rows_update_indirect(const void* rows_dev, int64_t n_rows, const int32_t* order_dev,
                                                     const int64_t* offsets_dev, const int64_t* stream_ids_dev,
                                                     const int64_t* bases_dev, int64_t num_segments,
                                                     int64_t num_states, int32_t key_width, int32_t k, uint64_t seed,
                                                     uint64_t stream_base, void* state_rows_dev,
                                                     int64_t* state_idx_dev, int64_t* state_next_dev,
                                                     void* hip_stream);

/* Segmented sampling without keys (Sampler.apply for any B over S streams): the elements stay with the
 * caller, only the streams' lengths reach the device.  Stream s has len = offsets[s+1] - offsets[s]
 * elements (offsets_dev is read for its differences alone) and Philox stream id stream_base + s;
 * out_idx_dev[s*k + j] is the stream-relative index of the element slot j holds -- the slot's last
 * writer, else j where j < len, else -1 -- and counts_dev[s] = min(len, k): stream s holds what a single
 * ELEMENTS handle on RSV_ENGINE_PHILOX_R fed len elements through rsv_sample_indexed holds.  Every slot
 * and every count is written.  k as rsv_sample_segmented.  A stream longer than the split length (a
 * multiple of 1024 indices; RSV_K2_SPLIT_LEN, read once per process, overrides it, 0 disables it) is
 * taken in pieces spread over the whole device and combined per slot by the largest index; the result
 * does not depend on the split.  Stream-ordered on hip_stream; the split form takes its work list from
 * the stream-ordered allocator and adds no host wait.  All pointers are device pointers. */
rsv_status rsv_sample_segmented_indexed(const int64_t* offsets_dev, int64_t num_streams, int32_t k, uint64_t seed,
                                        uint64_t stream_base, int64_t* out_idx_dev, int64_t* counts_dev,
                                        void* hip_stream);

/* rsv_sample_segmented_update without keys: the state is state_idx_dev[num_states*k] and
 * state_next_dev[num_states] as there (a fresh state is idx = -1, next = 0).  Segments (offsets_dev: their
 * lengths), stream_ids_dev, bases_dev and the skipped segments as rsv_sample_segmented_update; the
 * stream_ids of one call must be distinct (the caller's contract).  A slot's idx is replaced only where the
 * segment's last writer or fill index is later.  hits_dev[b*k + j] (int64) is, for each slot j that segment b
 * replaced, the position inside the segment of the element the slot now holds (its global index minus the
 * segment's base), and -1 for every other slot; hit_counts_dev[b] is the number of replaced slots.  Both are
 * written for every segment, skipped ones included (a row of -1, a count of 0): the caller keeps its elements
 * in step by storing segment b's element hits[b*k + j] into slot j of row stream_ids[b].  1 <= k <= 15104
 * (larger: RSV_E_UNSUPPORTED).  Stateless and stream-ordered on hip_stream: no host wait, no allocation. */
rsv_status rsv_sample_segmented_indexed_update(const int64_t* offsets_dev, const int64_t* stream_ids_dev,
                                               const int64_t* bases_dev, int64_t num_segments, int64_t num_states,
                                               int32_t k, uint64_t seed, uint64_t stream_base, int64_t* state_idx_dev,
                                               int64_t* state_next_dev, int64_t* hits_dev, int64_t* hit_counts_dev,
                                               void* hip_stream);

/* rsv_sample_segmented_merge without keys: part_idx_dev is [parts][num_states][k], part_next_dev
 * [parts][num_states].  Per slot the part with the largest idx wins if it beats the state's; next becomes the
 * max over the row and the parts.  src_dev[r*k + j] (int32) is the part slot j of row r was taken from -- the
 * lowest of the parts that hold the largest idx -- or -1 where the row's own entry stood: the caller copies its
 * element from slot j of row r of that part.  k as rsv_sample_segmented_indexed_update. */
rsv_status rsv_sample_segmented_indexed_merge(const int64_t* part_idx_dev, const int64_t* part_next_dev, int32_t parts,
                                              int64_t num_states, int32_t k, int64_t* state_idx_dev,
                                              int64_t* state_next_dev, int32_t* src_dev, void* hip_stream);

/* Segmented distinct: S independent Sampler.distinct samplers (no reference counterpart; = S separate
 * RandomValues instances, S:383-412).  Stream s covers keys_dev[offsets[s] .. offsets[s+1]) and is
 * seeded like a single DISTINCT handle with java.util.Random(seed + stream_base + s) (wrapping to a
 * signed 64-bit value): (r0, r1) are its first two nextLong() (S:385-388) and h = the scrambled hash
 * (S:396) of hash(key).  The result is the engine's set order (RSV_DISTINCT_SET): the min(k, D_s)
 * distinct keys with the smallest (h, key) -- the key compared as a signed 64-bit value, 4-byte keys
 * sign-extended -- written ascending by (h, key) into out_keys_dev[s*k ..] (and their h into
 * out_hashes_dev when not NULL), counts_dev[s] = min(k, D_s), slots beyond it zero.  That is the
 * reference's set whenever no two distinct keys share the final maximum hash (always under an
 * injective hash), whatever the arrival order.  The reference's arrival-order tie replay
 * (RSV_DISTINCT_ORDERED) is rsv_distinct_segmented_ordered below.
 * hash_kind: IDENTITY, JAVA_LONG, JAVA_INT, DEFAULT (JAVA_INT for key_width 4, JAVA_LONG for 8), or
 * PRECOMPUTED with hashes_dev, one int64 per key, indexed like keys_dev (NULL otherwise).
 * key_width 4 or 8 (byte keys: RSV_E_UNSUPPORTED); 1 <= k <= 4096 (larger: RSV_E_UNSUPPORTED).
 * Stateless and stream-ordered on hip_stream: no host wait, no allocation.  All pointers are device
 * pointers. */
rsv_status rsv_distinct_segmented(const void* keys_dev, const int64_t* hashes_dev, const int64_t* offsets_dev,
                                  int64_t num_streams, int32_t key_width, int32_t k, int32_t hash_kind, uint64_t seed,
                                  uint64_t stream_base, void* out_keys_dev, int64_t* out_hashes_dev,
                                  int64_t* counts_dev, void* hip_stream);

/* Segmented distinct in the reference's order (RSV_DISTINCT_ORDERED): inputs, seeding, hash kinds, key
 * widths and k as rsv_distinct_segmented.  Stream s ends holding exactly the set a RandomValues instance
 * (S:383-412) holds after sample() over keys_dev[offsets[s] .. offsets[s+1]) in that order, for any hash:
 * where more than k distinct keys have a hash <= the set's maximum hash M, the members with h = M are the
 * ones the reference's heap keeps (arrival order and scala 2.13 PriorityQueue's tie behaviour), not the
 * smallest keys.  The reference's own result order is a HashSet's and unspecified; the output is written
 * as rsv_distinct_segmented writes it: ascending by (h, key), counts_dev[s] = min(k, D_s), zeros beyond.
 * tied_dev[num_streams] (required; it is also the channel between the launch's two kernels):
 * tied_dev[s] = 1 iff the set is full and some distinct key of the stream outside the bottom-k by (h, key)
 * has hash M -- rsv_distinct_info.tied per stream, exact also for M = INT64_MAX or INT64_MIN -- else 0.  A
 * stream with tied_dev[s] == 0 is bit-identical to rsv_distinct_segmented's row.
 * out_hashes_dev may be NULL.  Byte keys: RSV_E_UNSUPPORTED; 1 <= k <= 4096 (larger:
 * RSV_E_UNSUPPORTED).  Stateless and stream-ordered on hip_stream: no host wait, no allocation.
 * Byte-key rows in this order: rsv_distinct_segmented_rows_ordered below.  Resumed from caller-held state:
 * rsv_distinct_segmented_ordered_update below -- a state of k entries kept sorted cannot carry the heap's
 * history, a state of k entries kept in the queue's array order is the heap, and that is its state
 * (rsv_distinct_segmented_rows_ordered_update for byte-key rows).  Not provided in ordered form: merge and
 * k > 4096: such callers keep separate handles. */
rsv_status rsv_distinct_segmented_ordered(const void* keys_dev, const int64_t* hashes_dev, const int64_t* offsets_dev,
                                          int64_t num_streams, int32_t key_width, int32_t k, int32_t hash_kind,
                                          uint64_t seed, uint64_t stream_base, void* out_keys_dev,
                                          int64_t* out_hashes_dev, int64_t* counts_dev, int32_t* tied_dev,
                                          void* hip_stream);

/* Segmented distinct over fixed-width byte keys (java.util.UUID, case classes of primitives): what
 * rsv_distinct_segmented is for 4- and 8-byte keys.  Stream s is rows [offsets[s], offsets[s+1]) of
 * rows_dev -- offsets count rows, not bytes; a row is key_width bytes, a multiple of 8 in 16..256,
 * read as key_width / 8 little-endian 64-bit words (a UUID: [mostSigBits | leastSigBits]).  Two
 * elements are one element iff all their bytes are equal; equal rows must carry equal hashes (the
 * caller's contract, as for a byte-key handle).  Seeding and h as rsv_distinct_segmented.
 * hash_kind: PRECOMPUTED with hashes_dev, one int64 per row, indexed like the rows; or DEFAULT at
 * key_width 16, java.util.UUID.hashCode computed on the device (hashes_dev unused).  The other kinds,
 * and DEFAULT at another width, are RSV_E_UNSUPPORTED; key_width 4 or 8 is RSV_E_UNSUPPORTED (use
 * rsv_distinct_segmented); 1 <= k <= 4096 (larger: RSV_E_UNSUPPORTED).
 * The result is the engine's set order (RSV_DISTINCT_SET), as rsv_export_packed documents it for
 * byte keys: the min(k, D_s) distinct rows with the smallest (h, words compared as unsigned 64-bit
 * values, word 0 first), written ascending into out_rows_dev[(s*k + j) * key_width ..], their h
 * into out_hashes_dev[s*k + j] when not NULL, counts_dev[s] = min(k, D_s); rows and hashes beyond
 * the count are zero.  It does not depend on the arrival order, equals a single RSV_DISTINCT_SET
 * handle per stream, and under an injective hash the reference's set.
 * rows_dev and out_rows_dev must be 8-byte aligned (RSV_E_ILLEGAL_ARGUMENT); rows_dev may be NULL
 * when every stream is empty.  Stateless and stream-ordered on hip_stream: no host wait, no
 * allocation.  All pointers are device pointers.  Resumed and combined:
 * rsv_distinct_segmented_rows_update / rsv_distinct_segmented_rows_merge below. */
rsv_status rsv_distinct_segmented_rows(const void* rows_dev, const int64_t* hashes_dev, const int64_t* offsets_dev,
                                       int64_t num_streams, int32_t key_width, int32_t k, int32_t hash_kind,
                                       uint64_t seed, uint64_t stream_base, void* out_rows_dev,
                                       int64_t* out_hashes_dev, int64_t* counts_dev, void* hip_stream);

/* Segmented distinct over byte keys in the reference's order (RSV_DISTINCT_ORDERED): what
 * rsv_distinct_segmented_ordered is for 4- and 8-byte keys.  Inputs, seeding, hash kinds (PRECOMPUTED at any
 * width, DEFAULT = UUID.hashCode at key_width 16), key widths, k, the alignment of rows_dev and out_rows_dev
 * and every check are rsv_distinct_segmented_rows': the same bad arguments give the same status in the same
 * order.  Stream s ends holding exactly the rows a RandomValues instance (S:383-412) over byte keys holds
 * after sample() over rows [offsets[s], offsets[s+1]) in that order, equality being equality of all bytes --
 * for any hash, UUID.hashCode's 32 bits included: where more than k distinct rows have a hash <= the set's
 * maximum hash M, the members with h = M are the ones the reference's heap keeps (arrival order and scala
 * 2.13 PriorityQueue's tie behaviour), not the smallest rows.  The output is laid out as
 * rsv_distinct_segmented_rows writes it: rows ascending by (h, words as unsigned 64-bit values, word 0
 * first), their h into out_hashes_dev when not NULL, counts_dev[s] = min(k, D_s), rows and hashes beyond
 * the count zero.
 * tied_dev[num_streams] (required, RSV_E_NULL_POINTER; it is also the channel between the launch's two
 * kernels): tied_dev[s] = 1 iff the set is full and some distinct row of the stream outside the bottom-k by
 * (h, row) has hash M, exact also for M = INT64_MAX or INT64_MIN, else 0.  A stream with tied_dev[s] == 0 is
 * bit-identical to rsv_distinct_segmented_rows' row block.
 * Stateless and stream-ordered on hip_stream: no host wait, no allocation.  Resumed from caller-held state:
 * rsv_distinct_segmented_rows_ordered_update below.  Merge and k > 4096 have no ordered form. */
rsv_status rsv_distinct_segmented_rows_ordered(const void* rows_dev, const int64_t* hashes_dev,
                                               const int64_t* offsets_dev, int64_t num_streams, int32_t key_width,
                                               int32_t k, int32_t hash_kind, uint64_t seed, uint64_t stream_base,
                                               void* out_rows_dev, int64_t* out_hashes_dev, int64_t* counts_dev,
                                               int32_t* tied_dev, void* hip_stream);

/* Segmented distinct, resumed: long-lived distinct samplers advanced by one launch per batch.  The
 * state is the caller's device memory: state_keys_dev[num_states*k] (key_width values),
 * state_hashes_dev[num_states*k] and state_counts_dev[num_states] (int64).  Row r holds counts[r]
 * entries ascending by (h, key): exactly what rsv_distinct_segmented writes into out_keys_dev /
 * out_hashes_dev / counts_dev, so a stateless result is a valid state; a row with counts[r] == 0 is
 * the empty sampler, whatever its slots hold.  Bottom-k by (h, key) over distinct keys is a function
 * of the key set alone, so a row fed a stream in pieces, in any number of launches, ends bit-identical
 * to one rsv_distinct_segmented launch over the concatenated stream (the three entry points run one
 * element loop with one table of thread counts and buffer sizes per k, and share their k, key_width
 * and hash_kind checks).
 * Segment b = keys_dev[offsets[b] .. offsets[b+1]) goes into row r = stream_ids_dev[b], or r = b when
 * stream_ids_dev is NULL (then num_segments <= num_states).  Row r is seeded as
 * java.util.Random(seed + stream_base + r); hash kinds, key widths and k as rsv_distinct_segmented.
 * Afterwards row r holds the bottom-k of (its previous entries u the segment's distinct keys),
 * ascending, slots beyond the count zero.  The ids of one launch must be distinct (two segments on
 * one row race: the caller's contract); a segment whose id lies outside [0, num_states) is skipped.
 * Rows that no segment names, and rows whose segment is empty, are not touched.  A row's count is
 * clamped into [0, k] before use and nothing else read from the state indexes memory: rows that are
 * not ascending give an unspecified set, never an out-of-range access.
 * Stateless and stream-ordered on hip_stream: no host wait, no allocation.  All pointers are device
 * pointers. */
rsv_status rsv_distinct_segmented_update(const void* keys_dev, const int64_t* hashes_dev, const int64_t* offsets_dev,
                                         const int64_t* stream_ids_dev, int64_t num_segments, int64_t num_states,
                                         int32_t key_width, int32_t k, int32_t hash_kind, uint64_t seed,
                                         uint64_t stream_base, void* state_keys_dev, int64_t* state_hashes_dev,
                                         int64_t* state_counts_dev, void* hip_stream);

/* Segmented distinct in the reference's order, resumed: what rsv_distinct_segmented_update is for the engine's
 * set order, for RSV_DISTINCT_ORDERED.  The state is the caller's device memory: state_keys_dev[num_states*k]
 * (key_width values), state_hashes_dev[num_states*k] (int64, required: the heap is ordered by them) and
 * state_counts_dev[num_states] (int64).  Row r holds counts[r] entries in scala 2.13 mutable.PriorityQueue
 * array order: entry j of the 1-indexed queue of a RandomValues instance (S:383-412) sits in slot j - 1, its
 * scrambled hash beside it; a row with counts[r] == 0 is the empty sampler, whatever its slots hold.  That
 * array and its length are the whole sampler: RandomValues' set holds the array's keys, its maxHash is the
 * root's hash at every moment (below k entries the running maximum, which a max-heap keeps at its root), and
 * addOne/fixUp and dequeue/fixDown are functions of the array alone.
 * THIS IS NOT THE LAYOUT OF rsv_distinct_segmented_update.  A row sorted ascending by (h, key) -- what
 * rsv_distinct_segmented, rsv_distinct_segmented_ordered and rsv_distinct_segmented_update write -- is not a
 * valid ordered state (sorted ascending it is not even a max-heap, and sorted descending it is another heap
 * than the reference's, which continues differently in exactly the tied streams); the two kinds of state must
 * not be mixed, and neither call accepts the other's rows.  Start a state with zeroed counts.
 * Segment b = keys_dev[offsets[b] .. offsets[b+1]) goes into row r = stream_ids_dev[b], or r = b when
 * stream_ids_dev is NULL (then num_segments <= num_states).  Row r is seeded as
 * java.util.Random(seed + stream_base + r); hash kinds, key widths (4 and 8; byte keys: RSV_E_UNSUPPORTED) and
 * 1 <= k <= 4096 as rsv_distinct_segmented_ordered.  Afterwards row r is exactly the array a RandomValues
 * instance holds after sample() over everything the row has been fed, across all launches, in that order, for
 * any hash; a fresh state fed a whole stream in one launch therefore holds the set
 * rsv_distinct_segmented_ordered returns (sort the row by (h, key) to compare).
 * The ids of one launch must be distinct (two segments on one row race: the caller's contract); a segment
 * whose id lies outside [0, num_states) is skipped.  Rows that no segment names, and rows whose segment is
 * empty, are not touched; a row in which nothing was admitted is not written at all; a row that is written
 * gets zeros beyond its count.  A row's count is clamped into [0, k] before use and nothing else read from
 * the state indexes memory: a row that is not a heap gives an unspecified set, never an out-of-range access.
 * The checks run before any device call, in rsv_distinct_segmented_update's order; state_hashes_dev NULL is
 * RSV_E_NULL_POINTER with the parameter named in rsv_last_error.
 * No merge: two heaps over disjoint parts of a stream do not determine the reference's heap over the whole
 * stream (who of the bucket at the maximum hash stays depends on the order in which all of it arrived).
 * Callers of the set order keep rsv_distinct_segmented_merge.  Byte-key rows in this form:
 * rsv_distinct_segmented_rows_ordered_update below.
 * Stateless and stream-ordered on hip_stream: no host wait, no allocation.  All pointers are device
 * pointers. */
rsv_status rsv_distinct_segmented_ordered_update(const void* keys_dev, const int64_t* hashes_dev,
                                                 const int64_t* offsets_dev, const int64_t* stream_ids_dev,
                                                 int64_t num_segments, int64_t num_states, int32_t key_width,
                                                 int32_t k, int32_t hash_kind, uint64_t seed, uint64_t stream_base,
                                                 void* state_keys_dev, int64_t* state_hashes_dev,
                                                 int64_t* state_counts_dev, void* hip_stream);

/* Combine of segmented distinct states: part_* are `parts` states laid back to back
 * ([parts][num_states][k] keys and hashes, [parts][num_states] counts: what an all-gather of every
 * rank's state tensors gives).  Row r becomes the bottom-k of (row r u the first
 * clamp(part_counts[p][r], 0, k) entries of row r of every part p); equal (h, key) pairs collapse.
 * The parts' hashes are final (already scrambled): nothing is hashed again, so all parts and the
 * state must come from the same seed, stream_base and hash (the caller's contract).  A row whose
 * parts are all empty is not touched.  Stateless and stream-ordered like the update. */
rsv_status rsv_distinct_segmented_merge(const void* part_keys_dev, const int64_t* part_hashes_dev,
                                        const int64_t* part_counts_dev, int32_t parts, int64_t num_states,
                                        int32_t key_width, int32_t k, void* state_keys_dev, int64_t* state_hashes_dev,
                                        int64_t* state_counts_dev, void* hip_stream);

/* Segmented distinct over byte keys, resumed: what rsv_distinct_segmented_update is for 4- and 8-byte
 * keys.  The state is the caller's device memory in exactly the layout rsv_distinct_segmented_rows
 * writes, so a stateless result is a valid state: state_rows_dev[num_states*k] rows of key_width bytes
 * (8-byte aligned), state_hashes_dev[num_states*k] and state_counts_dev[num_states] (int64).  Row r
 * holds counts[r] entries ascending by (h, words as unsigned 64-bit values, word 0 first), no row
 * twice; a row with counts[r] == 0 is the empty sampler, whatever its slots hold.  A row fed a stream
 * in pieces, in any number of launches, ends bit-identical to one rsv_distinct_segmented_rows launch
 * over the concatenated stream (one element loop, one table of thread counts and buffer sizes per k,
 * one set of k, key_width and hash_kind checks).
 * Segment b = rows [offsets[b], offsets[b+1]) of rows_dev goes into row r = stream_ids_dev[b], or
 * r = b when stream_ids_dev is NULL (then num_segments <= num_states).  Row r is seeded as
 * java.util.Random(seed + stream_base + r); key widths, hash kinds (PRECOMPUTED with hashes_dev, or
 * DEFAULT = UUID.hashCode at key_width 16) and k as rsv_distinct_segmented_rows; key_width 4 or 8 is
 * RSV_E_UNSUPPORTED (use rsv_distinct_segmented_update).  Afterwards row r holds the bottom-k of (its
 * previous rows u the segment's distinct rows), ascending.  The row block is rewritten in place, and
 * only where it changes: a row that admitted nothing is not written at all, an entry that keeps its
 * slot is not moved.  Rows and hashes beyond the new count are zero whenever the row was empty before
 * or its count had to be clamped; a row that held entries keeps what it had there, which is zero in
 * every state these entry points or rsv_distinct_segmented_rows wrote.
 * The ids of one launch must be distinct (two segments on one row race: the caller's contract); a
 * segment whose id lies outside [0, num_states) is skipped.  Rows that no segment names, and rows
 * whose segment is empty, are not touched.  rows_dev and hashes_dev must not overlap the state (the
 * caller's contract); rows_dev may be NULL when every segment is empty.  A row's count is clamped into
 * [0, k] before use and nothing else read from the state addresses memory: rows that are not
 * ascending, or that hold a row twice, give an unspecified set, never an out-of-range access.
 * rows_dev and state_rows_dev must be 8-byte aligned (RSV_E_ILLEGAL_ARGUMENT); a NULL state pointer
 * is RSV_E_NULL_POINTER; zero segments or states return RSV_OK with nothing launched.
 * Stateless and stream-ordered on hip_stream: no host wait, no allocation.  All pointers are device
 * pointers. */
rsv_status rsv_distinct_segmented_rows_update(const void* rows_dev, const int64_t* hashes_dev,
                                              const int64_t* offsets_dev, const int64_t* stream_ids_dev,
                                              int64_t num_segments, int64_t num_states, int32_t key_width, int32_t k,
                                              int32_t hash_kind, uint64_t seed, uint64_t stream_base,
                                              void* state_rows_dev, int64_t* state_hashes_dev,
                                              int64_t* state_counts_dev, void* hip_stream);

/* Combine of segmented distinct states over byte keys: part_* are `parts` states laid back to back
 * ([parts][num_states][k] rows of key_width bytes and hashes, [parts][num_states] counts: what an
 * all-gather of every rank's state tensors gives).  Row r becomes the bottom-k of (row r u the first
 * clamp(part_counts[p][r], 0, k) entries of row r of every part p); equal rows are one element.  The
 * parts' hashes are final (already scrambled): nothing is hashed again, so all parts and the state
 * must come from the same seed, stream_base and hash (the caller's contract), and the parts must not
 * overlap the state.  A row whose parts are all empty, or add nothing, is not touched.  part_rows_dev
 * and state_rows_dev must be 8-byte aligned.  Checks (without a hash kind), in-place writes and
 * stream order as the update. */
rsv_status rsv_distinct_segmented_rows_merge(const void* part_rows_dev, const int64_t* part_hashes_dev,
                                             const int64_t* part_counts_dev, int32_t parts, int64_t num_states,
                                             int32_t key_width, int32_t k, void* state_rows_dev,
                                             int64_t* state_hashes_dev, int64_t* state_counts_dev, void* hip_stream);

/* Segmented distinct over byte keys in the reference's order, resumed: what rsv_distinct_segmented_ordered_update
 * is for 4- and 8-byte keys, and what rsv_distinct_segmented_rows_update is for the engine's set order.  The state
 * is the queue's array of a RandomValues instance (S:383-412) over byte keys, and as on the JVM the array holds
 * references: the rows stay where they were put.  It is the caller's device memory, four parts per row r:
 *   state_rows_dev[num_states*k]    rows of key_width bytes (8-byte aligned).  Storage only: the order of the k
 *                                   slots of a row's block means nothing.
 *   state_hashes_dev[num_states*k]  int64, in scala 2.13 mutable.PriorityQueue array order: the scrambled hash of
 *                                   entry j of the 1-indexed queue sits at position j - 1.
 *   state_slots_dev[num_states*k]   int32, same positions: the row of the entry at position p lies in slot
 *                                   slots[r*k + p] of row r's own block, at state_rows_dev[(r*k + slot) * key_width].
 *   state_counts_dev[num_states]    int64: the queue's length; 0 is the empty sampler, whatever the rest holds.
 * Slot rule (part of the contract): an admission that grows the heap from n to n + 1 entries takes slot n; an
 * admission into a full heap takes the slot of the root it evicts.  So a row with n < k entries uses exactly the
 * slots 0..n-1, a full row's slots are a permutation of 0..k-1, no surviving row is ever moved, and the whole
 * state -- hashes, slots, counts and the rows in their slots -- is a function of what the row has been fed, in
 * that order, however it was cut into launches.  The array, its length and the rows it refers to are the whole
 * sampler, for the reason given at rsv_distinct_segmented_ordered_update.
 * THIS IS NOT rsv_distinct_segmented_rows_update's layout.  A row block sorted ascending by (h, words) with its
 * hashes beside it -- what rsv_distinct_segmented_rows, rsv_distinct_segmented_rows_ordered and
 * rsv_distinct_segmented_rows_update write -- is not a valid ordered state, with or without slots 0..k-1 added:
 * it is another heap than the reference's and continues differently in exactly the tied streams.  The two kinds
 * of state must not be mixed.  Start a state with zeroed counts.
 * Segment b = rows [offsets[b], offsets[b+1]) of rows_dev goes into row r = stream_ids_dev[b], or r = b when
 * stream_ids_dev is NULL (then num_segments <= num_states).  Row r is seeded as
 * java.util.Random(seed + stream_base + r); key widths, hash kinds (PRECOMPUTED with hashes_dev, or DEFAULT =
 * UUID.hashCode at key_width 16), 1 <= k <= 4096 and the equal-rows-equal-hashes contract as
 * rsv_distinct_segmented_rows_ordered.  Afterwards row r is exactly the array a RandomValues instance holds after
 * sample() over everything the row has been fed, across all launches, in that order, for any hash; a fresh state
 * fed a whole stream in one launch holds the set rsv_distinct_segmented_rows_ordered returns (gather the rows by
 * their slots and sort by (h, words) to compare).
 * A launch writes into the row block only the rows it admitted that are still members at its end, each into its
 * slot; hashes and slots are written over [0, k) with zeros beyond the count.  A row in which nothing was admitted
 * is not written at all.  Row slots [count, k) are zeroed whenever the row was empty before or its count had to
 * be clamped; a row that held entries keeps what it had there, which is zero in every state this entry point
 * wrote.  The ids of one launch must be distinct (two segments on one row race: the caller's contract); a
 * segment whose id lies outside [0, num_states) is skipped.  Rows that no segment names, and rows whose segment
 * is empty, are not touched.  rows_dev and hashes_dev must not overlap the state (the caller's contract);
 * rows_dev may be NULL when every segment is empty.
 * A row's count is clamped into [0, k] and every slot below k before use, and nothing else read from the state
 * addresses memory: slots out of range or repeated, a row that is no heap and a wrong count give an unspecified
 * set, never an out-of-range access.
 * The checks run before any device call and are rsv_distinct_segmented_rows_update's in its order (the same bad
 * arguments give the same status); state_slots_dev NULL is RSV_E_NULL_POINTER with the parameter named in
 * rsv_last_error.  No merge, for the reason given at rsv_distinct_segmented_ordered_update: callers of the set
 * order keep rsv_distinct_segmented_rows_merge.
 * Stateless and stream-ordered on hip_stream: no host wait, no allocation.  All pointers are device pointers. */
rsv_status rsv_distinct_segmented_rows_ordered_update(const void* rows_dev, const int64_t* hashes_dev,
                                                      const int64_t* offsets_dev, const int64_t* stream_ids_dev,
                                                      int64_t num_segments, int64_t num_states, int32_t key_width,
                                                      int32_t k, int32_t hash_kind, uint64_t seed, uint64_t stream_base,
                                                      void* state_rows_dev, int64_t* state_hashes_dev,
                                                      int32_t* state_slots_dev, int64_t* state_counts_dev,
                                                      void* hip_stream);

/* Segmented distinct for any B (Strings, case classes, tuples): the hash-only candidate pass of
 * rsv_distinct_candidates for many streams in one launch, on caller-held state.  The engine reads
 * hashes_dev[i] = hash(map(x_i)) alone, 8 bytes per element, and returns per segment, in arrival order, the
 * positions RandomValues (S:383-412) could still admit; the caller keeps one exact replica per row (heap, set,
 * maxHash), replays the candidates' elements into it and tells the next launch the replica's size and maxHash.
 * State, the caller's device memory: shadow_hashes_dev[num_states*k] and shadow_counts_dev[num_states] (int64).
 * Row r holds counts[r] distinct scrambled hashes ascending, the smallest the row has returned as candidates; a
 * row with counts[r] == 0 is the empty sampler whatever its slots hold, so a stateless call is a call on zeroed
 * counts.  set_sizes_dev / max_hashes_dev [num_states] (both or neither: exactly one is
 * RSV_E_ILLEGAL_ARGUMENT) are the replicas' size and maxHash as of their last replay, read once per row.
 * Segment b = hashes_dev[offsets[b] .. offsets[b+1]) goes into row r = stream_ids_dev[b], or r = b when
 * stream_ids_dev is NULL (then num_segments <= num_states), seeded as java.util.Random(seed + stream_base + r):
 * h = scramble(r0, r1, hash).  While the shadow holds fewer than k values and set_sizes[r] < k (or none is
 * given) every element is a candidate, whatever its h.  Otherwise element i is a candidate iff h_i < bound,
 * strictly, bound being the smaller of the shadow's k-th value (when it holds k) and max_hashes[r] (when
 * set_sizes[r] >= k).  The shadow is merged lazily, so its k-th value may lag the exact one by up to one buffer of
 * candidates (256 / 512 / 2048 / 8192 entries for k <= 64 / 256 / 1024 / 4096): more candidates, never fewer.
 * Every element the reference admits is among them, and replaying them in order gives the reference's heap.
 * Candidate j of segment b is written as (absolute index into hashes_dev, h) to out_pos_dev[b*cap + j] and
 * out_hashes_dev[b*cap + j] ([num_segments*cap] each), j ascending with the index, while j < cap;
 * out_counts_dev[b] receives the number found, stored or not, and 0 for a skipped segment (an id outside
 * [0, num_states), or no elements).  A segment with out_counts[b] > cap overflowed: its state row is not
 * written, and a rerun of that segment with cap >= out_counts[b] returns exactly out_counts[b] candidates.
 * Otherwise the row's shadow and count are advanced in place (zeros beyond the count); a row that returned no
 * candidate is not written.  The ids of one launch must be distinct (the caller's contract); rows no segment
 * names are not touched.  A count is clamped into [0, k] before use and nothing else read from the state indexes
 * memory.
 * Abort rule: the state advances in place.  A caller that may drop a batch (a throwing map) keeps a copy of the
 * rows the launch names and puts it back: a shadow that has seen hashes the replica never sampled is no longer a
 * valid bound.
 * Checks, before any device call: k out of range RSV_E_ILLEGAL_ARGUMENT; k > 4096 RSV_E_UNSUPPORTED; negative
 * counts, cap < 1 or more segments than rows without ids RSV_E_ILLEGAL_ARGUMENT; num_segments == 0 RSV_OK with
 * nothing touched; a NULL buffer RSV_E_NULL_POINTER (hashes_dev may be NULL only when every segment is empty,
 * the state only when num_states == 0); one of set_sizes_dev / max_hashes_dev without the other.
 * Stateless and stream-ordered on hip_stream: no host wait, no allocation.  All pointers are device pointers. */
rsv_status rsv_distinct_segmented_candidates(const int64_t* hashes_dev, const int64_t* offsets_dev,
                                             const int64_t* stream_ids_dev, int64_t num_segments, int64_t num_states,
                                             int32_t k, uint64_t seed, uint64_t stream_base, int64_t* shadow_hashes_dev,
                                             int64_t* shadow_counts_dev, const int64_t* set_sizes_dev,
                                             const int64_t* max_hashes_dev, int64_t* out_pos_dev, int64_t* out_hashes_dev,
                                             int64_t cap, int64_t* out_counts_dev, void* hip_stream);

/* Event replay (K1'): apply eviction events (1-based position, slot) -- the
 * `samples(rand.nextInt(k)) = map(element)` writes of S:243-246 -- for elements at global indices
 * [base_index, base_index+n) held in keys_dev, onto reservoir_dev[k] (in/out, device).  Also
 * performs the fill phase (S:253-255) for indices < k.  The last event per slot wins. */
rsv_status rsv_replay_events(const void* keys_dev, int64_t n, int32_t key_width, int64_t base_index,
                             const int64_t* ev_pos_dev, const int32_t* ev_slot_dev, int64_t n_events,
                             int32_t k, void* reservoir_dev, void* hip_stream);

/* Export the per-element draw sequence j_i (format R2) for indices [i0, i0+n) into j_dev. */
rsv_status rsv_export_draws(uint64_t seed, uint64_t stream_id, uint64_t i0, int64_t n,
                            uint64_t* j_dev, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* RESERVOIR_HIP_H */
