// rsv_runtime.hip -- implementation of the C ABI (include/reservoir_hip.h): sampler handles,
// lifecycle (SingleUse / MultiResult, Sampler.scala:182-194, :334-381, :414-433), staging of
// per-element calls into pinned batches, host->device batching, engine dispatch, multi-GPU
// state export/merge.  All data-parallel work runs in the kernels of rsv_elements.hip and
// rsv_distinct.hip; there is no CPU compute path.
#include <cstdlib>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <mutex>
#include <cmath>
#include <string>
#include <vector>

#include "../../include/reservoir_hip.h"
#include "rsv_device.h"
#include "rsv_internal.h"

namespace rsv {

static thread_local std::string g_last_error;
void set_error(const std::string& msg) { g_last_error = msg; }

int hip_status(hipError_t e, const char* what) {
    set_error(std::string(what) + ": " + hipGetErrorString(e));
    return e == hipErrorOutOfMemory ? RSV_E_OUT_OF_MEMORY : RSV_E_DEVICE;
}

// ---- the log-retention rules every distinct engine shares (rsv_internal.h DistinctEngine) -----
int DistinctEngine::log_export_check() const {
    if (retained()) return RSV_OK;
    set_error(!ordered  ? "rsv_export_log needs an RSV_DISTINCT_ORDERED sampler"
              : !retain ? "rsv_export_log: the candidate log was not retained (rsv_retain_log before sampling)"
                        : "rsv_export_log: the candidate log was not retained (archive limit, or sampled "
                          "after a merge)");
    return RSV_E_UNSUPPORTED;
}

int LogEmit::finish(int64_t* out_n) const {
    *out_n = cnt;
    if (cnt > cap && cap > 0) {  // (cap 0: a count-only query)
        set_error("rsv_export_log: cap is smaller than the number of candidates (*out_n)");
        return RSV_E_ILLEGAL_ARGUMENT;
    }
    return RSV_OK;
}

// ---------------------------------------------------------------------------------------------
// java.util.Random + Algorithm L event generator for RSV_ENGINE_JAVA_L (product implementation;
// the oracle under oracle/ is an independent restatement used only by the tests).
struct JavaRandom {
    uint64_t seed = 0;
    void init(int64_t s) { seed = ((uint64_t)s ^ 0x5DEECE66DULL) & ((1ULL << 48) - 1); }
    int32_t next(int bits) {
        seed = (seed * 0x5DEECE66DULL + 0xBULL) & ((1ULL << 48) - 1);
        return (int32_t)(uint32_t)(seed >> (48 - bits));
    }
    double next_double() {  // java.util.Random.nextDouble
        const int64_t a = next(26), b = next(27);
        return (double)((a << 27) + b) * 0x1.0p-53;
    }
    int32_t next_int(int32_t bound) {  // java.util.Random.nextInt(int)
        int32_t r = next(31);
        const int32_t m = bound - 1;
        if ((bound & m) == 0) return (int32_t)(((int64_t)bound * (int64_t)r) >> 31);
        for (int32_t u = r;; u = next(31)) {
            r = u % bound;
            if ((int32_t)((uint32_t)u - (uint32_t)r + (uint32_t)m) >= 0) break;
        }
        return r;
    }
    int64_t next_long() {
        const int64_t hi = next(32), lo = next(32);
        return (int64_t)(((uint64_t)hi << 32) + (uint64_t)lo);
    }
};

struct AlgoLState {  // RandomElements' private state (Sampler.scala:199-205)
    JavaRandom rand;
    int32_t k = 0;
    double W = 1.0;
    int64_t next_sample_count = 0;

    static int64_t d2l(double d) {  // JVM double -> long (saturating, NaN -> 0)
        if (d != d) return 0;
        if (d >= 9223372036854775807.0) return INT64_MAX;
        if (d <= -9223372036854775808.0) return INT64_MIN;
        return (int64_t)d;
    }
    void update() {  // updateNextSampleCount, Sampler.scala:228-236
        W = W * std::exp(std::log(rand.next_double()) / (double)k);
        const double skip = std::floor(std::log(rand.next_double()) / std::log(1.0 - W));
        next_sample_count = (int64_t)((uint64_t)next_sample_count + (uint64_t)d2l(skip) + 1ULL);
    }
    void init(int32_t kk, int64_t seed) {  // as SamplerTest.useConsistentRandom re-seeds it
        k = kk;
        rand.init(seed);
        W = 1.0;
        next_sample_count = kk;
        update();
    }
    // eviction events for 1-based positions (base, base+n] -- the per-element rule of
    // sampleImpl (Sampler.scala:248-259): position c > k evicts iff c >= nextSampleCount.
    void events(int64_t base, int64_t n, std::vector<int64_t>& pos, std::vector<int32_t>& slot) {
        int64_t cur = base + 1;
        const int64_t end = base + n;
        if (cur <= k) cur = (int64_t)k + 1;
        while (cur <= end) {
            const int64_t p = std::max(next_sample_count, cur);
            if (p > end) break;
            pos.push_back(p);
            slot.push_back(rand.next_int(k));  // sampleWithEviction, Sampler.scala:243-246
            update();
            cur = p + 1;
        }
    }
};

}  // namespace rsv

using namespace rsv;

static_assert(__BYTE_ORDER__ == __ORDER_LITTLE_ENDIAN__ && sizeof(bool) == 1, "rsv_sampler::gate reads four bools as a word");
constexpr uint32_t kGateReady = 1;  // bytes {open = 1, keys_owed = 0, keys_external = 0, cand_pending = 0}

// One pinned staging buffer of per-element calls (rsv_sample, rsv_stage_acquire); a full one is flushed
// asynchronously (H2D + kernels, no host wait) while the other fills.
struct alignas(64) Stage {
    MappedBuf<uint8_t> keys;  // coherent + mapped: a winners-only flush reads them in place through the alias
    HostBuf<int64_t> hashes;
    // java_l flushes: the batch's Algorithm-L events in pinned memory (free again with `free`), so their
    // H2D copies need no host wait
    HostBuf<int64_t> ev_pos;
    HostBuf<int32_t> ev_slot;
    PoolEvent free;        // recorded behind the flush's last read of the buffer
    bool pending = false;  // a flush is queued: wait for `free` before the buffer fills again
};

// The ELEMENTS slot block, one raw pool block (kernels take its views by value, and the clean-slot cache
// outlives handles): batch_win[k] | slot_idx[k] | slot_key[k] | k1_ticket.
struct Slots {
    void* block = nullptr;
    SlotBlock sb{};              // win, slot_idx, slot_key, k, key width
    uint32_t* ticket = nullptr;  // fused K1 + resolve_publish: zero between launches
    // device-state knowledge, in stream order: batch_win all zero (resolve leaves it so) / slot arrays
    // initialised.  Creation enqueues no device work; the first batch initialises.
    bool win_zero = false, init = false;
};

struct rsv_sampler {
    rsv_config cfg{};
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    // The lifecycle flags, also readable as one word: rsv_sample / rsv_stage_acquire / rsv_stage_commit
    // go ahead iff `gate == kGateReady` (open, no keys owed, slots hold keys, no candidate batch) -- one
    // load and compare per element; every other state goes through check_keyed for its message.
    //   keys_owed      rsv_sample_indexed: the caller still owes the new holders' keys (rsv_fill_slots)
    //   keys_external  rsv_commit_indexed / rsv_distinct_candidates: the caller keeps the elements (any
    //                  JVM B); the slots hold no keys
    //   cand_pending   rsv_distinct_candidates: the caller owes a commit or abort
    union {
        struct {
            bool open, keys_owed, keys_external, cand_pending;
        };
        uint32_t gate = 1;  // open
    };
    int64_t count = 0;
    int kw = 8;
    uint32_t k = 0;
    int hash_kind = kHashIdentity;
    // host staging of per-element calls: stage[stage_cur] fills, stage_n of stage_cap keys so far
    int stage_cur = 0;
    int64_t stage_n = 0;
    int64_t stage_cap = 0;
    Stage stage[2];
    Slots slots;  // ELEMENTS
    struct {      // java_l: the reference's Algorithm-L state, and a batch's events on the host and the device
        AlgoLState algo;
        std::vector<int64_t> pos_h;
        std::vector<int32_t> slot_h;
        DevBuf<int64_t> pos_d;
        DevBuf<int32_t> slot_d;
    } jl;
    struct {  // the index-only batch (rsv_sample_indexed) and what rsv_abort_indexed restores
        DevBuf<int64_t> offs_d;  // per slot the batch offset of its new element
        DevBuf<int64_t> bak_d;   // the slot indices before the pending batch
        bool fresh = false;
        int64_t base = 0;    // the pending batch's start
        AlgoLState algo;     // JAVA_L: java.util.Random and W before the batch's events
        // the offsets in host memory: published by the resolve kernel where resolve_indices_publish_ok(k)
        Landing offs;
        // the winners' keys in slot order (host gather of a winners-only batch, rsv_fill_slots): read by the
        // fill kernel across PCIe (no H2D copy, no host wait)
        MappedBuf<uint8_t> gath;
    } idx;
    DistinctEngine* distinct = nullptr;  // DISTINCT
    // distinct for any B (rsv_distinct_candidates): the hash-only candidate pass; the caller keeps the
    // elements (keys_external) and owes a commit or abort while cand_pending
    ObjDistinct* obj = nullptr;
    int64_t cand_batch = 0;  // the pending batch's element count
    struct {                 // the device chunk of host batches and copied flushes (kChunkKeys keys)
        DevBuf<uint8_t> keys;
        DevBuf<int64_t> hashes;
    } chunk;
    // result(): k keys; up to kPublishMaxBytes published -- by publish_kernel, or by a batch's own resolve
    // (small reservoirs), so that result() only waits for generation clock.pub_gen while clock.holds()
    Landing result;
    WorkClock clock;
    KernelTimer timer;
    PoolEvent handover;  // rsv_set_stream's event (kept until destroy: see there)
    // rsv_set_resolve_stream: each batch's resolve + publication on this caller stream, forked from
    // `stream` after K1 (fork) and joined back (join) before the handle's next device work
    struct {
        hipStream_t rstream = nullptr;
        PoolEvent fork, join;
        bool pending = false;
    } side;
};

namespace {

// process-wide hot-kernel timer (rsv_profile_global); guarded by g_prof_mu
std::mutex g_prof_mu;
std::atomic<bool> g_prof_on{false};
KernelTimer& global_timer() {
    static auto* t = new KernelTimer();  // leaked on purpose, like the pool
    return *t;
}

// the forked resolve (rsv_set_resolve_stream) ordered before the handle's next work on its stream
inline void join_side(rsv_sampler* s) {
    if (!s->side.pending) return;
    (void)hipStreamWaitEvent(s->stream, s->side.join, 0);
    s->side.pending = false;
}
// a new group of device work on the handle's stream / everything enqueued so far is complete
inline void touch(rsv_sampler* s) {
    join_side(s);
    s->clock.group();
}
inline hipError_t sync_stream(rsv_sampler* s) {
    join_side(s);
    hipError_t e = hipStreamSynchronize(s->stream);
    if (e == hipSuccess) s->clock.drained();
    return e;
}

// Timing marks around the handle's hot kernel: its own timer (every launch), else the process-wide
// one, which times every g_prof_every-th launch (rsv_profile_global).  prof_begin's return value
// goes to the matching prof_end.
std::atomic<int64_t> g_prof_every{1};
int64_t g_prof_seq = 0;  // guarded by g_prof_mu

bool prof_begin(rsv_sampler* s, hipStream_t st) {
    if (s->timer.on) {
        s->timer.mark(st);
        return true;
    }
    if (!g_prof_on) return false;
    std::lock_guard<std::mutex> lk(g_prof_mu);
    if (g_prof_seq++ % g_prof_every != 0) return false;
    KernelTimer& t = global_timer();
    t.on = true;
    t.device = s->device;
    t.mark(st);
    return true;
}

void prof_end(rsv_sampler* s, hipStream_t st, bool marked) {
    if (!marked) return;
    if (s->timer.on) {
        s->timer.mark(st);
        return;
    }
    std::lock_guard<std::mutex> lk(g_prof_mu);
    global_timer().mark(st);
}

constexpr int32_t kMaxSize = 2147483647 - 2;  // Sampler.scala:71 (hotspot VM array limit)
constexpr int64_t kStageKeys = 1 << 20;
constexpr int64_t kChunkKeys = 1 << 22;

struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) (void)hipSetDevice(dev);
    }
    ~DeviceGuard() {
        int cur = -1;
        if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
    }
};

rsv_status fail(rsv_status st, const std::string& msg) {
    set_error(msg);
    return st;
}

rsv_status check_open(const rsv_sampler* s) {  // SingleUse.checkOpen, Sampler.scala:185-186
    if (!s) return fail(RSV_E_NULL_POINTER, "sampler is NULL");
    if (!s->open) return fail(RSV_E_ILLEGAL_STATE, "use of sampler after calling `result()`");
    if (s->keys_owed) return fail(RSV_E_ILLEGAL_STATE, "rsv_fill_slots is pending after rsv_sample_indexed");
    if (s->cand_pending)
        return fail(RSV_E_ILLEGAL_STATE, "a candidate batch is pending: rsv_candidates_commit or rsv_candidates_abort");
    return RSV_OK;
}

// the calls that skip check_open: none of them while a candidate batch is pending
rsv_status check_no_batch(const rsv_sampler* s) {
    if (!s) return fail(RSV_E_NULL_POINTER, "sampler is NULL");
    if (s->cand_pending)
        return fail(RSV_E_ILLEGAL_STATE, "a candidate batch is pending: rsv_candidates_commit or rsv_candidates_abort");
    return RSV_OK;
}

// entry points that read or write keys: not on a handle whose caller keeps the elements
rsv_status check_keyed(const rsv_sampler* s) {
    if (rsv_status st = check_open(s)) return st;
    if (s->keys_external)
        return fail(RSV_E_ILLEGAL_STATE, s->obj ? "the handle holds no keys (rsv_distinct_candidates): hash-only batches only"
                                                : "the slots hold no keys (rsv_commit_indexed): index-only batches only");
    return RSV_OK;
}

rsv_status ensure_events(rsv_sampler* s, int64_t n) {
    const int64_t cur = group_cap(s->jl.pos_d, s->jl.slot_d);
    if (n <= cur) return RSV_OK;
    if (s->jl.pos_d || s->jl.slot_d) RSV_HIP_TRY(sync_stream(s));  // before reuse elsewhere
    s->jl.pos_d.release(), s->jl.slot_d.release();
    RSV_HIP_TRY(reserve_all(std::max<int64_t>(n, 2 * cur), s->stream, s->jl.pos_d, s->jl.slot_d));
    return RSV_OK;
}

inline const SlotBlock& slot_block(const rsv_sampler* s) { return s->slots.sb; }

// slot arrays of a fresh handle: slot_key = 0, slot_idx = -1 (empty), batch_win = 0, on the
// handle's current stream before its first use (creation itself enqueues no device work)
rsv_status ensure_slots(rsv_sampler* s) {
    if (s->slots.init || s->cfg.kind != RSV_KIND_ELEMENTS) return RSV_OK;
    touch(s);
    RSV_HIP_TRY(launch_init_slots(slot_block(s), s->stream, s->slots.ticket));
    s->slots.init = s->slots.win_zero = true;
    s->clock.invalidate();
    return RSV_OK;
}

// Slot blocks whose batch_win is known zero (their last sampler ended on a resolve): a new handle
// of the same (k, key width) takes one and skips the init kernel -- its first resolve marks the
// untouched slots empty instead (resolve_kernel `fresh`).
struct CleanSlots {
    void* p;
    uint32_t k;
    int kw;
    int device;
};
std::mutex g_clean_mu;
std::vector<CleanSlots>& clean_slots() {
    static auto* v = new std::vector<CleanSlots>();  // leaked on purpose, like the pool
    return *v;
}

void* take_clean_slots(uint32_t k, int kw, int device) {
    std::lock_guard<std::mutex> lk(g_clean_mu);
    auto& v = clean_slots();
    for (size_t i = v.size(); i-- > 0;)
        if (v[i].k == k && v[i].kw == kw && v[i].device == device) {
            void* p = v[i].p;
            v.erase(v.begin() + (ptrdiff_t)i);
            return p;
        }
    return nullptr;
}

bool give_clean_slots(void* p, uint32_t k, int kw, int device) {
    if ((uint64_t)k * (16 + kw) > (64ull << 20)) return false;
    std::lock_guard<std::mutex> lk(g_clean_mu);
    auto& v = clean_slots();
    if (v.size() >= 32) return false;
    v.push_back(CleanSlots{p, k, kw, device});
    return true;
}

// a handle's slot block and its views: a clean one of the same shape (batch_win known zero), else a new one
hipError_t acquire_slots(Slots& sl, uint32_t k32, int kw, int device) {
    const size_t k = k32, keys = (k * kw + 7) & ~(size_t)7;
    sl.block = take_clean_slots(k32, kw, device);
    sl.win_zero = sl.block != nullptr;
    if (!sl.block)
        if (hipError_t e = pool_device_alloc(&sl.block, k * 16 + keys + 8)) return e;
    uint8_t* b = (uint8_t*)sl.block;
    sl.sb = SlotBlock{(unsigned long long*)b, (int64_t*)(b + k * 8), b + k * 16, k32, kw};
    sl.ticket = (uint32_t*)(b + k * 16 + keys);
    return hipSuccess;
}

// the block back to the clean-slot cache when batch_win is known zero, else to the pool; the caller has
// synchronized the stream
void recycle_slots(Slots& sl, int device) {
    if (!(sl.block && sl.win_zero && give_clean_slots(sl.block, sl.sb.k, sl.sb.key_width, device)))
        pool_device_free(sl.block);
    sl = Slots{};
}

constexpr int64_t kPublishMaxBytes = 1 << 20;

// the result's landing zone: published up to kPublishMaxBytes
rsv_status ensure_result_buffer(rsv_sampler* s) {
    const size_t bytes = (size_t)s->k * s->kw;
    RSV_HIP_TRY(s->result.ensure(bytes, (int64_t)bytes <= kPublishMaxBytes));
    return RSV_OK;
}

// The publish step of a launch that can also publish the reservoir's first min(count, k) keys.
// begin_publish: may it (`allowed`: the form's own limit on k and key width; then a coherent result
// buffer has to exist), and if so with which target and generation -- *pub, none when it may not.
// record_publish, once the launch is enqueued: what result() can rely on.
rsv_status begin_publish(rsv_sampler* s, bool allowed, int64_t count, Publication* pub) {
    *pub = Publication{};
    if (!allowed) return RSV_OK;
    if (rsv_status st = ensure_result_buffer(s)) return st;
    Landing& r = s->result;
    if (r.published()) *pub = Publication{std::min<int64_t>(count, (int64_t)s->k), r.dev(), r.flag_dev(), r.next_gen()};
    return RSV_OK;
}

// (the publication is the last work of the current group)
void record_publish(rsv_sampler* s, const Publication& pub) { s->clock.published(pub.dst != nullptr, pub.gen); }

constexpr uint32_t kFusedPublishMaxK = 8192;  // resolve_publish: one workgroup, <= 8 slots per lane

// a resolve forked onto the resolve stream runs as ONE 256-thread workgroup (beside the next K1;
// RSV_RESOLVE_SMALL=0: the 1024-thread form, for A/B)
bool resolve_small() {
    static const bool v = [] {
        const char* e = std::getenv("RSV_RESOLVE_SMALL");
        return !(e && e[0] == '0');
    }();
    return v;
}

// The batch's resolve: fill phase + winners into the slots; for reservoirs of <= 8192 keys it
// also writes the first min(count, k) keys into the coherent result buffer and publishes
// generation result.next_gen() there (one dispatch instead of resolve now + publish at result()).
rsv_status resolve_batch(rsv_sampler* s, const void* keys, int64_t base, int64_t n, bool fresh,
                         hipStream_t rst = nullptr) {
    if (!rst) rst = s->stream;
    Publication pub;
    if (rsv_status st = begin_publish(s, s->k <= kFusedPublishMaxK, base + n, &pub)) return st;
    RSV_HIP_TRY(launch_resolve(slot_block(s), Batch{keys, base, n, fresh}, pub, rst,
                               rst != s->stream && resolve_small()));
    record_publish(s, pub);
    return RSV_OK;
}

// The frame of one element batch at global indices [count, count + n).  begin: a new group of device
// work; a never-used slot block gets its full init; *fresh says that the slots were never initialised
// (a recycled clean block: the resolve marks the untouched ones empty); batch_win is no longer known
// zero until the batch's resolve is enqueued, which is where end stands.
rsv_status begin_element_batch(rsv_sampler* s, bool* fresh) {
    touch(s);
    if (!s->slots.win_zero) {  // never-used block: full init
        RSV_HIP_TRY(launch_init_slots(slot_block(s), s->stream, s->slots.ticket));
        s->slots.init = s->slots.win_zero = true;
    }
    *fresh = !s->slots.init;
    s->slots.win_zero = false;
    return RSV_OK;
}

void end_element_batch(rsv_sampler* s, int64_t n) {
    s->slots.init = s->slots.win_zero = true;
    s->count += n;
}

// java_l: the reference's own Algorithm-L events of the batch [base, base + n) (S:261-273 skips by
// them), computed on the host, uploaded and replayed into batch_win; *n_events of them.  stage: the batch
// is that staging buffer, and the uploads read its pinned event buffers -- its previous flush has
// completed (stage_slow waited for it), and its `free` event releases them.  Null: they read the handle's
// pageable event vectors, which the next batch reuses.
rsv_status replay_java_l(rsv_sampler* s, int64_t base, int64_t n, Stage* stage, int64_t* n_events) {
    auto& jl = s->jl;
    jl.pos_h.clear();
    jl.slot_h.clear();
    jl.algo.events(base, n, jl.pos_h, jl.slot_h);
    const int64_t ne = *n_events = (int64_t)jl.pos_h.size();
    if (!ne) return RSV_OK;
    if (rsv_status st = ensure_events(s, ne)) return st;
    const void* pos_src = jl.pos_h.data();
    const void* slot_src = jl.slot_h.data();
    if (stage) {
        const int64_t cur = group_cap(stage->ev_pos, stage->ev_slot);
        if (cur < ne) RSV_HIP_TRY(reserve_all(std::max<int64_t>(ne, 2 * cur), nullptr, stage->ev_pos, stage->ev_slot));
        memcpy(stage->ev_pos, pos_src, ne * 8);
        memcpy(stage->ev_slot, slot_src, ne * 4);
        pos_src = stage->ev_pos;
        slot_src = stage->ev_slot;
    }
    RSV_HIP_TRY(hipMemcpyAsync(jl.pos_d, pos_src, ne * 8, hipMemcpyHostToDevice, s->stream));
    RSV_HIP_TRY(hipMemcpyAsync(jl.slot_d, slot_src, ne * 4, hipMemcpyHostToDevice, s->stream));
    const bool pm = prof_begin(s, s->stream);
    RSV_HIP_TRY(launch_replay_events(jl.pos_d, jl.slot_d, ne, s->k, s->slots.sb.win, s->stream));
    prof_end(s, s->stream, pm);
    return RSV_OK;
}

// one batch of n keys already in device memory, at global indices [count, count+n); stage: the batch
// is that staging buffer, whose pinned event buffers carry java_l's events
rsv_status process_device_batch(rsv_sampler* s, const void* keys, const int64_t* hashes, int64_t n,
                                Stage* stage = nullptr) {
    if (n <= 0) return RSV_OK;
    if (s->cfg.kind == RSV_KIND_DISTINCT) {
        touch(s);
        // large batches publish the merged set speculatively (DistinctEngine::spec_target: set mode behind
        // its last merge, ordered mode behind the scheduled pass) -- only where a publication can
        // happen at all (a coherent result buffer of k keys); other samplers (huge k, device-only
        // consumers) keep the result buffer lazy
        if ((int64_t)s->k * s->kw <= kPublishMaxBytes && n >= s->distinct->spec_min()) {
            if (rsv_status st = ensure_result_buffer(s)) return st;
            Landing& r = s->result;
            if (r.published()) s->distinct->spec_target(r.dev(), r.flag_dev(), &r.gen);
        }
        int rc = s->distinct->sample_device(keys, hashes, n, s->stream);
        uint32_t gen = 0;
        const bool published = s->distinct->spec_take(&gen);
        if (rc != RSV_OK) return (rsv_status)rc;
        s->clock.published(published, gen);  // result() waits for it instead of publishing
        s->count += n;
        return RSV_OK;
    }
    const int64_t base = s->count;
    bool fresh;
    if (rsv_status st = begin_element_batch(s, &fresh)) return st;
    if (s->cfg.engine == RSV_ENGINE_JAVA_L) {
        int64_t ne = 0;
        if (rsv_status st = replay_java_l(s, base, n, stage, &ne)) return st;
        if (rsv_status st = resolve_batch(s, keys, base, n, fresh)) return st;
        // pageable host event vectors are reused by the next batch (a staged batch's pinned copies
        // are released by its `free` event instead)
        if (ne && !stage) RSV_HIP_TRY(sync_stream(s));
    } else {
        const DrawParams dp{s->cfg.seed, s->cfg.stream_id};
        const uint64_t lo = std::max<uint64_t>((uint64_t)base, s->k), hi = (uint64_t)(base + n);
        // Fused (one dispatch, the last workgroup resolves) for batches up to 2^27 draws, where the
        // saved dispatch is a visible share of the step; above that the two-dispatch form is faster
        // (C2: 112.5 vs 114.0 us per step, r02aa: the fused tail runs on one workgroup of the
        // otherwise idle chip, while the publishing resolve_kernel's dispatch overlaps K1's drain; round 6,
        // the two-group K1: 96.7 vs 83.0-83.7 us per launch, 97.2 vs 88.6-89.5 us per step --
        // every workgroup's ticket wait holds its slot, profiles/r06/bench_k1_fuse_ab.jsonl).
        // RSV_K1_FUSE=0 / =1 forces either form (A/B measurements).
        static const int fuse_mode = [] {
            const char* e = std::getenv("RSV_K1_FUSE");
            return e && e[0] == '0' ? 0 : e && e[0] == '1' ? 1 : 2;
        }();
        constexpr uint64_t kFuseMaxDraws = 1ull << 27;
        const bool fuse = (fuse_mode == 1 || (fuse_mode == 2 && (hi <= lo || hi - lo <= kFuseMaxDraws))) &&
                          k1_fused_ok(lo, hi, s->k, s->kw);
        Publication pub;
        if (rsv_status st = begin_publish(s, fuse, base + n, &pub)) return st;
        if (pub.dst) {
            // one dispatch: K1, then the last workgroup resolves and publishes (resolve_batch's form)
            const bool pm = prof_begin(s, s->stream);
            RSV_HIP_TRY(launch_k1_resolve_publish(dp, lo, hi, slot_block(s), s->slots.ticket, Batch{keys, base, n, fresh},
                                                  pub, s->stream));
            prof_end(s, s->stream, pm);
            record_publish(s, pub);
        } else {
            const bool pm = prof_begin(s, s->stream);
            RSV_HIP_TRY(launch_k1_last_writer(dp, s->k, lo, hi, s->slots.sb.win, s->stream));
            prof_end(s, s->stream, pm);
            if (auto& sd = s->side; sd.rstream) {  // the resolve + publication forked onto the resolve stream (see there)
                RSV_HIP_TRY(sd.fork.ensure(s->device, hipEventDisableTiming));
                RSV_HIP_TRY(sd.join.ensure(s->device, hipEventDisableTiming));
                RSV_HIP_TRY(hipEventRecord(sd.fork, s->stream));
                RSV_HIP_TRY(hipStreamWaitEvent(sd.rstream, sd.fork, 0));
                if (rsv_status st = resolve_batch(s, keys, base, n, fresh, sd.rstream)) return st;
                RSV_HIP_TRY(hipEventRecord(sd.join, sd.rstream));
                sd.pending = true;
            } else if (rsv_status st = resolve_batch(s, keys, base, n, fresh)) {
                return st;
            }
        }
    }
    end_element_batch(s, n);
    return RSV_OK;
}

rsv_status ensure_chunk(rsv_sampler* s) {
    RSV_HIP_TRY(s->chunk.keys.reserve(kChunkKeys * s->kw, s->stream));
    if (s->cfg.kind == RSV_KIND_DISTINCT && s->hash_kind == kHashPrecomputed)
        RSV_HIP_TRY(s->chunk.hashes.reserve(kChunkKeys, s->stream));
    return RSV_OK;
}

// Wait until a kernel has published `gen` into the coherent host word `flag` (acquire).  Spins for
// up to ~2 ms -- the K1 pass of a 1e9-element batch still in flight ahead of it is ~0.1 ms -- then
// falls back to a blocking stream synchronize, which also reports a failed kernel instead of
// waiting forever.
rsv_status spin_flag(rsv_sampler* s, const uint32_t* flag, uint32_t gen, const char* what) {
    const auto t0 = std::chrono::steady_clock::now();
    for (uint32_t spin = 1;; ++spin) {
        if (__atomic_load_n(flag, __ATOMIC_ACQUIRE) == gen) return RSV_OK;
        __builtin_ia32_pause();
        if ((spin & 1023) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(2)) break;
    }
    RSV_HIP_TRY(sync_stream(s));
    if (__atomic_load_n(flag, __ATOMIC_ACQUIRE) == gen) return RSV_OK;
    return fail(RSV_E_DEVICE, std::string(what) + " flag not set after stream synchronize");
}

// One index-only batch of n elements at global indices [count, count + n) (the reference's
// sampleIndexed, Sampler.scala:261-273, which reads only the elements it keeps): K1 (philox_r) or
// the host's Algorithm-L events (java_l) over the indices alone, the resolve into slot_idx, and per
// slot the batch offset of its new element (-1: unchanged) in host memory, *offs_out (k entries,
// valid until the handle's next index-only batch).  No key is read.  The caller then supplies the
// winners' keys (fill_gathered) or undoes the batch (rsv_abort_indexed).
rsv_status index_batch(rsv_sampler* s, int64_t n, const int64_t** offs_out) {
    auto& ix = s->idx;
    RSV_HIP_TRY(reserve_all(s->k, s->stream, ix.offs_d, ix.bak_d));
    RSV_HIP_TRY(ix.offs.ensure((size_t)s->k * 8, resolve_indices_publish_ok(s->k)));
    const int64_t base = s->count;
    bool fresh;
    if (rsv_status st = begin_element_batch(s, &fresh)) return st;
    // the state rsv_abort_indexed restores (a throwing `map` leaves the slots consistent)
    ix.fresh = fresh;
    ix.base = base;
    ix.algo = s->jl.algo;
    if (!fresh)
        RSV_HIP_TRY(hipMemcpyAsync(ix.bak_d, s->slots.sb.slot_idx, (size_t)s->k * 8, hipMemcpyDeviceToDevice, s->stream));
    if (s->cfg.engine == RSV_ENGINE_JAVA_L) {
        int64_t ne = 0;  // the event vectors are read by copies that precede the waits below in stream order
        if (rsv_status st = replay_java_l(s, base, n, nullptr, &ne)) return st;
    } else {
        const DrawParams dp{s->cfg.seed, s->cfg.stream_id};
        const uint64_t lo = std::max<uint64_t>((uint64_t)base, s->k), hi = (uint64_t)(base + n);
        const bool pm = prof_begin(s, s->stream);
        RSV_HIP_TRY(launch_k1_last_writer(dp, s->k, lo, hi, s->slots.sb.win, s->stream));
        prof_end(s, s->stream, pm);
    }
    const Batch batch{nullptr, base, n, fresh};
    if (ix.offs.published()) {  // the offsets straight into coherent host memory + flag: no copy, no stream sync
        const uint32_t gen = ix.offs.next_gen();
        RSV_HIP_TRY(launch_resolve_indices(slot_block(s), batch, ix.offs_d,
                                           Publication{0, ix.offs.dev(), ix.offs.flag_dev(), gen}, s->stream));
        if (rsv_status st = spin_flag(s, ix.offs.flag(), gen, "index batch")) return st;
        s->clock.seen(s->clock.ops, gen, ix.offs.gen);  // the publication was this handle's last work
    } else {
        RSV_HIP_TRY(launch_resolve_indices(slot_block(s), batch, ix.offs_d, Publication{}, s->stream));
        RSV_HIP_TRY(hipMemcpyAsync(ix.offs.host(), ix.offs_d, (size_t)s->k * 8, hipMemcpyDeviceToHost, s->stream));
        RSV_HIP_TRY(sync_stream(s));
    }
    end_element_batch(s, n);
    s->clock.invalidate();
    *offs_out = (const int64_t*)ix.offs.host();
    return RSV_OK;
}

rsv_status ensure_gather(rsv_sampler* s) {
    RSV_HIP_TRY(s->idx.gath.reserve((int64_t)s->k * s->kw));
    return RSV_OK;
}

// The winners' keys, gathered by the host into idx.gath (slot order; only the slots index_batch
// changed are read), into the reservoir: one kernel reading them across PCIe, which for small
// reservoirs also publishes the result -- enqueued, no host wait.  The gather buffer is rewritten
// only after the handle's next index_batch has waited for its own publication, which follows this
// kernel in stream order.
rsv_status fill_gathered(rsv_sampler* s) {
    touch(s);
    Publication pub;
    if (rsv_status st = begin_publish(s, fill_slots_publish_ok(s->k, s->kw), s->count, &pub)) return st;
    RSV_HIP_TRY(launch_fill_slots(s->idx.offs_d, s->idx.gath.dev, slot_block(s), pub, s->stream));
    record_publish(s, pub);
    s->keys_owed = false;
    return RSV_OK;
}

// A host batch of an ELEMENTS sampler moves only its winners: the batch is sampled by index
// (index_batch), the host copies the <= k winning keys out of the caller's buffer, and they reach
// the slots across PCIe (fill_gathered) -- 8 B per winner instead of 8 B per element.
rsv_status host_batch_elements(rsv_sampler* s, const void* keys, int64_t n) {
    const int64_t* offs = nullptr;
    if (rsv_status st = index_batch(s, n, &offs)) return st;
    if (rsv_status st = ensure_gather(s)) return st;
    const uint8_t* src = (const uint8_t*)keys;
    uint8_t* gath = s->idx.gath;
    const size_t kw = (size_t)s->kw;
    if (kw == 8) {
        for (uint32_t j = 0; j < s->k; ++j)
            if (offs[j] >= 0) memcpy(gath + (size_t)j * 8, src + (size_t)offs[j] * 8, 8);
    } else {
        for (uint32_t j = 0; j < s->k; ++j)
            if (offs[j] >= 0) memcpy(gath + (size_t)j * kw, src + (size_t)offs[j] * kw, kw);
    }
    return fill_gathered(s);
}

rsv_status process_host_batch(rsv_sampler* s, const void* keys, const int64_t* hashes, int64_t n) {
    if (n <= 0) return RSV_OK;
    if (s->cfg.kind == RSV_KIND_ELEMENTS) return host_batch_elements(s, keys, n);
    if (rsv_status st = ensure_chunk(s)) return st;
    join_side(s);  // (a forked resolve reads its batch's keys; none for DISTINCT, kept for symmetry)
    for (int64_t off = 0; off < n; off += (int64_t)kChunkKeys) {
        const int64_t c = std::min((int64_t)kChunkKeys, n - off);
        RSV_HIP_TRY(hipMemcpyAsync(s->chunk.keys, (const uint8_t*)keys + off * s->kw, c * s->kw,
                                   hipMemcpyHostToDevice, s->stream));
        if (s->chunk.hashes && hashes)
            RSV_HIP_TRY(hipMemcpyAsync(s->chunk.hashes, hashes + off, c * 8, hipMemcpyHostToDevice, s->stream));
        if (rsv_status st = process_device_batch(s, s->chunk.keys, s->chunk.hashes, c)) return st;
    }
    // the caller may reuse its buffer after return (ownership stays with the caller)
    RSV_HIP_TRY(sync_stream(s));
    return RSV_OK;
}

// Flush the current staging buffer: H2D into the device chunk, record "buffer free", launch the
// batch's kernels -- all stream-ordered, no host wait -- and switch to the other buffer.
// Expected number of slots a batch of n elements at global indices [base, base + n) changes: the
// fill of slots [base, k), then ~k/(i+1) evictions per index i >= k (Algorithm R; Algorithm L has
// the same expectation), at most k.
double expected_changes(const rsv_sampler* s, int64_t base, int64_t n) {
    const double k = s->k;
    const double fill = std::min<double>(std::max<double>(k - (double)base, 0.0), (double)n);
    const double lo = std::max<double>((double)base, k), hi = (double)base + (double)n;
    const double ev = hi > lo ? k * std::log(hi / lo) : 0.0;
    return std::min(fill + ev, std::min<double>((double)n, k));
}

// A staged batch of an ELEMENTS sampler is sampled in place when its expected winners are few
// against its size: the resolve reads the <= k winning keys straight from the pinned staging
// buffer across PCIe instead of a DMA of the whole batch.  RSV_STAGE_ZC_RATIO (default 16): in
// place when expected changes x ratio <= n; 0 = always copy.
bool stage_in_place(const rsv_sampler* s, int64_t n) {
    static const double ratio = [] {
        const char* e = std::getenv("RSV_STAGE_ZC_RATIO");
        return e ? std::atof(e) : 16.0;
    }();
    if (s->cfg.kind != RSV_KIND_ELEMENTS || ratio <= 0) return false;
    return expected_changes(s, s->count, n) * ratio <= (double)n;
}

rsv_status flush_stage(rsv_sampler* s) {
    if (s->stage_n == 0) return RSV_OK;
    const int64_t n = s->stage_n;
    Stage& sg = s->stage[s->stage_cur];
    s->stage_n = 0;
    if (stage_in_place(s, n)) {
        sg.pending = true;
        s->stage_cur ^= 1;
        if (rsv_status st = process_device_batch(s, sg.keys.dev, nullptr, n, &sg)) return st;
        // the buffer is free once the resolve that reads it has run (on the resolve stream if forked)
        RSV_HIP_TRY(hipEventRecord(sg.free, s->side.pending ? s->side.rstream : s->stream));
        return RSV_OK;
    }
    if (rsv_status st = ensure_chunk(s)) return st;
    join_side(s);  // a forked resolve may still read the chunk's previous batch
    RSV_HIP_TRY(hipMemcpyAsync(s->chunk.keys, sg.keys, n * s->kw, hipMemcpyHostToDevice, s->stream));
    if (s->chunk.hashes && sg.hashes)
        RSV_HIP_TRY(hipMemcpyAsync(s->chunk.hashes, sg.hashes, n * 8, hipMemcpyHostToDevice, s->stream));
    sg.pending = true;
    s->stage_cur ^= 1;
    if (s->cfg.kind == RSV_KIND_ELEMENTS && s->cfg.engine == RSV_ENGINE_JAVA_L) {
        // the batch's events travel from the stage's pinned event buffers: free after their copies
        if (rsv_status st = process_device_batch(s, s->chunk.keys, nullptr, n, &sg)) return st;
        RSV_HIP_TRY(hipEventRecord(sg.free, s->stream));
        return RSV_OK;
    }
    RSV_HIP_TRY(hipEventRecord(sg.free, s->stream));
    return process_device_batch(s, s->chunk.keys, s->chunk.hashes, n);
}

// what the handle's members do not own (they go back with the handle itself); callers have synchronized
// the stream, or seen the handle's last publication: nothing queued touches any of it any more
void free_all(rsv_sampler* s) {
    recycle_slots(s->slots, s->device);
    delete s->distinct;
    if (s->obj) obj_destroy(s->obj);
    if (s->stream && s->own_stream) pool_release_stream(s->device, s->stream);
}

int resolve_hash_kind(int32_t hk, int kw) {
    switch (hk) {
    case RSV_HASH_IDENTITY: return kHashIdentity;
    case RSV_HASH_JAVA_LONG: return kHashJavaLong;
    case RSV_HASH_JAVA_INT: return kHashJavaInt;
    case RSV_HASH_PRECOMPUTED: return kHashPrecomputed;
    default:  // B#hashCode (Sampler.scala:75): Integer / Long / java.util.UUID
        return kw == 4 ? kHashJavaInt : kw == 16 ? kHashUuid : kHashJavaLong;
    }
}

}  // namespace

extern "C" {

int32_t rsv_abi_version(void) { return RSV_ABI_VERSION; }

const char* rsv_last_error(void) { return g_last_error.c_str(); }

const char* rsv_status_string(rsv_status s) {
    switch (s) {
    case RSV_OK: return "ok";
    case RSV_E_ILLEGAL_ARGUMENT: return "illegal argument";
    case RSV_E_ILLEGAL_STATE: return "illegal state";
    case RSV_E_NULL_POINTER: return "null pointer";
    case RSV_E_DEVICE: return "device error";
    case RSV_E_OUT_OF_MEMORY: return "out of memory";
    case RSV_E_UNSUPPORTED: return "unsupported";
    }
    return "unknown status";
}

rsv_status rsv_config_init(rsv_config* cfg) {
    if (!cfg) return fail(RSV_E_NULL_POINTER, "config is NULL");
    memset(cfg, 0, sizeof(*cfg));
    cfg->struct_size = sizeof(rsv_config);
    cfg->kind = RSV_KIND_ELEMENTS;
    cfg->max_sample_size = 1;
    cfg->key_width = 8;
    cfg->engine = RSV_ENGINE_PHILOX_R;
    cfg->hash_kind = RSV_HASH_DEFAULT;
    cfg->device = -1;
    return RSV_OK;
}

rsv_status rsv_create(const rsv_config* cfg, rsv_sampler** out) {
    if (!cfg || !out) return fail(RSV_E_NULL_POINTER, "config/out is NULL");
    *out = nullptr;
    if (cfg->struct_size != sizeof(rsv_config))
        return fail(RSV_E_ILLEGAL_ARGUMENT, "rsv_config.struct_size mismatch (ABI version)");
    // validateSharedParams, Sampler.scala:79-83
    if (cfg->max_sample_size > kMaxSize) return fail(RSV_E_ILLEGAL_ARGUMENT, "maxSampleSize exceeds VM limit");
    if (cfg->max_sample_size <= 0) return fail(RSV_E_ILLEGAL_ARGUMENT, "maxSampleSize must be positive");
    if (cfg->kind != RSV_KIND_ELEMENTS && cfg->kind != RSV_KIND_DISTINCT)
        return fail(RSV_E_ILLEGAL_ARGUMENT, "unknown sampler kind");
    // key widths: Int (4), Long (8), fixed-width byte keys (a multiple of 8 in 16..256: UUID = 16).
    // Any other width is a request this build does not implement (the reference has no width).
    const bool wide = cfg->key_width > 8 && cfg->key_width <= 256 && cfg->key_width % 8 == 0;
    if (cfg->key_width != 4 && cfg->key_width != 8 && !wide)
        return fail(RSV_E_UNSUPPORTED, "key_width must be 4, 8 or a multiple of 8 in 16..256 bytes");
    // byte keys have no Long/Int hashCode: DISTINCT takes the caller's hash (PRECOMPUTED) or, for
    // 16-byte keys, java.util.UUID.hashCode (DEFAULT)
    if (wide && cfg->kind == RSV_KIND_DISTINCT && cfg->hash_kind != RSV_HASH_PRECOMPUTED &&
        !(cfg->hash_kind == RSV_HASH_DEFAULT && cfg->key_width == 16))
        return fail(RSV_E_UNSUPPORTED, "DISTINCT over byte keys needs RSV_HASH_PRECOMPUTED (or RSV_HASH_DEFAULT = "
                                       "java.util.UUID.hashCode for 16-byte keys)");
    if (cfg->kind == RSV_KIND_ELEMENTS && cfg->engine != RSV_ENGINE_PHILOX_R && cfg->engine != RSV_ENGINE_JAVA_L)
        return fail(RSV_E_ILLEGAL_ARGUMENT, "unknown engine");
    if (cfg->hash_kind < RSV_HASH_DEFAULT || cfg->hash_kind > RSV_HASH_PRECOMPUTED)
        return fail(RSV_E_ILLEGAL_ARGUMENT, "unknown hash kind");
    if (cfg->distinct_order < RSV_DISTINCT_AUTO || cfg->distinct_order > RSV_DISTINCT_ORDERED)
        return fail(RSV_E_ILLEGAL_ARGUMENT, "unknown distinct order");

    rsv_sampler* s = new rsv_sampler();
    s->cfg = *cfg;
    s->kw = cfg->key_width;
    s->k = (uint32_t)cfg->max_sample_size;
    int dev = cfg->device;
    if (dev < 0 && hipGetDevice(&dev) != hipSuccess) dev = 0;
    s->device = dev;
    DeviceGuard g(dev);
    auto bail = [&](rsv_status st, const std::string& msg) {
        free_all(s);
        delete s;
        return fail(st, msg);
    };
    s->timer.device = dev;
    hipError_t e = pool_stream(&s->stream);
    if (e != hipSuccess) return bail(RSV_E_DEVICE, std::string("hipStreamCreate: ") + hipGetErrorString(e));
    s->own_stream = true;
    if (cfg->kind == RSV_KIND_ELEMENTS) {
        e = acquire_slots(s->slots, s->k, s->kw, dev);
        if (e != hipSuccess)
            return bail(e == hipErrorOutOfMemory ? RSV_E_OUT_OF_MEMORY : RSV_E_DEVICE,
                        std::string("allocating reservoir: ") + hipGetErrorString(e));
        if (cfg->engine == RSV_ENGINE_JAVA_L) s->jl.algo.init((int32_t)s->k, (int64_t)cfg->seed);
    } else {
        // RandomValues r0, r1 (Sampler.scala:385-388) from java.util.Random(seed)
        JavaRandom r;
        r.init((int64_t)cfg->seed);
        const int64_t r0 = r.next_long(), r1 = r.next_long();
        s->hash_kind = resolve_hash_kind(cfg->hash_kind, s->kw);
        int st = RSV_OK;
        bool ordered;
        switch (cfg->distinct_order) {
        case RSV_DISTINCT_SET: ordered = false; break;
        case RSV_DISTINCT_ORDERED: ordered = true; break;
        default:  // hashes that may collide
            ordered = s->hash_kind == kHashJavaLong || s->hash_kind == kHashPrecomputed || s->hash_kind == kHashUuid;
        }
        s->distinct = distinct_create((int32_t)s->k, s->kw, s->hash_kind, r0, r1, ordered, &st);
        if (!s->distinct) {
            std::string msg = g_last_error;
            return bail((rsv_status)st, msg);
        }
        s->distinct->set_timer(&s->timer);
    }
    *out = s;
    return RSV_OK;
}

void rsv_destroy(rsv_sampler* s) {
    if (!s) return;
    DeviceGuard g(s->device);
    // the buffers go back to the pool: nothing this handle enqueued may still touch them.  On a
    // caller stream whose last group of work was a publication the host has seen, that holds
    // already (the flag store is the last memory operation of that group).
    if (s->stream && (s->own_stream || !s->clock.idle())) {
        join_side(s);
        (void)hipStreamSynchronize(s->stream);
    } else if (s->side.pending && s->side.rstream) {
        // the publication was seen (its flag store is the resolve's last memory operation): only the
        // events and buffers remain, and they outlive the queued work by the join below
        (void)hipEventSynchronize(s->side.join);
    }
    free_all(s);
    delete s;  // the members' buffers and events (the hand-over event too: see rsv_set_stream) go back now
}

// Slow part of rsv_sample: (re)arm a staging buffer, or flush a full one.  Runs once per batch.
static rsv_status stage_slow(rsv_sampler* s, bool pre) {
    DeviceGuard g(s->device);
    if (s->stage_n == s->stage_cap && s->stage_cap) {
        if (rsv_status st = flush_stage(s)) return st;
    }
    if (!s->stage_cap) {  // (every step a no-op where an earlier, failed call got that far)
        for (Stage& sg : s->stage) {
            RSV_HIP_TRY(sg.keys.reserve(kStageKeys * s->kw));
            if (pre) RSV_HIP_TRY(sg.hashes.reserve(kStageKeys));
            RSV_HIP_TRY(sg.free.ensure(s->device, hipEventDisableTiming));
        }
        s->stage_cap = kStageKeys;
    }
    Stage& sg = s->stage[s->stage_cur];
    if (s->stage_n == 0 && sg.pending) {  // its previous batch's H2D must have read it
        RSV_HIP_TRY(hipEventSynchronize(sg.free));
        sg.pending = false;
    }
    return RSV_OK;
}

rsv_status rsv_sample(rsv_sampler* s, const void* key, const int64_t* hash) {
    // per-element hot path (the akka operator calls this per element): no HIP call here
    if (!s || s->gate != kGateReady) return check_keyed(s);
    if (!key) return fail(RSV_E_NULL_POINTER, "key is NULL");
    const bool pre = s->hash_kind == kHashPrecomputed && s->cfg.kind == RSV_KIND_DISTINCT;
    if (pre && !hash) return fail(RSV_E_NULL_POINTER, "hash is NULL for RSV_HASH_PRECOMPUTED");
    if (s->stage_n == 0 || s->stage_n == s->stage_cap) {
        if (rsv_status st = stage_slow(s, pre)) return st;
    }
    Stage& sg = s->stage[s->stage_cur];
    if (s->kw == 8) memcpy(sg.keys + s->stage_n * 8, key, 8);
    else if (s->kw == 4) memcpy(sg.keys + s->stage_n * 4, key, 4);
    else memcpy(sg.keys + s->stage_n * s->kw, key, (size_t)s->kw);
    if (pre) sg.hashes[s->stage_n] = *hash;
    ++s->stage_n;
    return RSV_OK;
}

rsv_status rsv_stage_acquire(rsv_sampler* s, void** keys_out, int64_t** hashes_out, int64_t* capacity) {
    if (!s || s->gate != kGateReady) return check_keyed(s);
    if (!keys_out || !capacity) return fail(RSV_E_NULL_POINTER, "keys_out/capacity is NULL");
    const bool pre = s->hash_kind == kHashPrecomputed && s->cfg.kind == RSV_KIND_DISTINCT;
    if (s->stage_n == 0 || s->stage_n == s->stage_cap) {
        if (rsv_status st = stage_slow(s, pre)) return st;
    }
    Stage& sg = s->stage[s->stage_cur];
    *keys_out = sg.keys + s->stage_n * s->kw;
    if (hashes_out) *hashes_out = pre ? sg.hashes + s->stage_n : nullptr;
    *capacity = s->stage_cap - s->stage_n;
    return RSV_OK;
}

rsv_status rsv_stage_commit(rsv_sampler* s, int64_t n) {
    if (!s || s->gate != kGateReady) return check_keyed(s);
    if (n < 0 || n > s->stage_cap - s->stage_n)
        return fail(RSV_E_ILLEGAL_ARGUMENT, "commit exceeds the acquired staging capacity");
    s->stage_n += n;
    if (s->stage_n == s->stage_cap && n > 0) {  // full: start its flush now, overlapping the next fill
        DeviceGuard g(s->device);
        if (rsv_status st = flush_stage(s)) return st;
    }
    return RSV_OK;
}

rsv_status rsv_sample_batch(rsv_sampler* s, const void* keys, int64_t n, int32_t mem, const int64_t* hashes) {
    if (rsv_status st = check_keyed(s)) return st;
    if (n < 0) return fail(RSV_E_ILLEGAL_ARGUMENT, "negative batch size");
    if (n == 0) return RSV_OK;
    if (!keys) return fail(RSV_E_NULL_POINTER, "keys is NULL");
    const bool pre = s->cfg.kind == RSV_KIND_DISTINCT && s->hash_kind == kHashPrecomputed;
    if (pre && !hashes) return fail(RSV_E_NULL_POINTER, "hashes is NULL for RSV_HASH_PRECOMPUTED");
    DeviceGuard g(s->device);
    if (rsv_status st = flush_stage(s)) return st;  // keep global index order
    if (mem == RSV_MEM_DEVICE) return process_device_batch(s, keys, pre ? hashes : nullptr, n);
    if (mem == RSV_MEM_HOST) return process_host_batch(s, keys, pre ? hashes : nullptr, n);
    return fail(RSV_E_ILLEGAL_ARGUMENT, "mem must be RSV_MEM_HOST or RSV_MEM_DEVICE");
}

rsv_status rsv_sample_indexed(rsv_sampler* s, int64_t n, int64_t* slot_offsets_host) {
    if (rsv_status st = check_open(s)) return st;
    if (s->cfg.kind != RSV_KIND_ELEMENTS)
        return fail(RSV_E_UNSUPPORTED, "rsv_sample_indexed needs an ELEMENTS sampler (distinct maps every element, S:50)");
    if (n < 0) return fail(RSV_E_ILLEGAL_ARGUMENT, "negative batch size");
    if (!slot_offsets_host) return fail(RSV_E_NULL_POINTER, "slot_offsets_host is NULL");
    if (n == 0) {
        for (uint32_t j = 0; j < s->k; ++j) slot_offsets_host[j] = -1;
        return RSV_OK;
    }
    DeviceGuard g(s->device);
    if (rsv_status st = flush_stage(s)) return st;  // keep global index order
    const int64_t* offs = nullptr;
    if (rsv_status st = index_batch(s, n, &offs)) return st;
    memcpy(slot_offsets_host, offs, (size_t)s->k * 8);
    s->keys_owed = true;
    return RSV_OK;
}

rsv_status rsv_fill_slots(rsv_sampler* s, const void* keys_host) {
    if (!s) return fail(RSV_E_NULL_POINTER, "sampler is NULL");
    if (!s->keys_owed) return fail(RSV_E_ILLEGAL_STATE, "rsv_fill_slots without a pending rsv_sample_indexed");
    if (s->keys_external)
        return fail(RSV_E_ILLEGAL_STATE, "the slots hold no keys (rsv_commit_indexed): commit or abort the batch");
    if (!keys_host) return fail(RSV_E_NULL_POINTER, "keys_host is NULL");
    DeviceGuard g(s->device);
    if (rsv_status st = ensure_gather(s)) return st;
    // the changed slots' keys into the pinned gather buffer: the caller's buffer is theirs again on
    // return, and no copy or host wait follows
    const int64_t* offs = (const int64_t*)s->idx.offs.host();
    const size_t kw = (size_t)s->kw;
    const uint8_t* src = (const uint8_t*)keys_host;
    for (uint32_t j = 0; j < s->k; ++j)
        if (offs[j] >= 0) memcpy(s->idx.gath + (size_t)j * kw, src + (size_t)j * kw, kw);
    return fill_gathered(s);
}

rsv_status rsv_abort_indexed(rsv_sampler* s) {
    if (!s) return fail(RSV_E_NULL_POINTER, "sampler is NULL");
    if (!s->keys_owed) return fail(RSV_E_ILLEGAL_STATE, "rsv_abort_indexed without a pending rsv_sample_indexed");
    DeviceGuard g(s->device);
    touch(s);
    if (s->idx.fresh)  // the slots were never initialised before the batch: empty them again
        RSV_HIP_TRY(launch_init_slots(slot_block(s), s->stream, s->slots.ticket));
    else  // the changed slots still hold their old keys: their old indices make them whole again
        RSV_HIP_TRY(hipMemcpyAsync(s->slots.sb.slot_idx, s->idx.bak_d, (size_t)s->k * 8, hipMemcpyDeviceToDevice, s->stream));
    RSV_HIP_TRY(sync_stream(s));
    s->slots.init = s->slots.win_zero = true;
    s->clock.invalidate();
    s->count = s->idx.base;
    s->jl.algo = s->idx.algo;
    s->keys_owed = false;
    return RSV_OK;
}

rsv_status rsv_commit_indexed(rsv_sampler* s) {
    if (!s) return fail(RSV_E_NULL_POINTER, "sampler is NULL");
    if (!s->keys_owed) return fail(RSV_E_ILLEGAL_STATE, "rsv_commit_indexed without a pending rsv_sample_indexed");
    // the slot indices are final (index_batch); the keys stay with the caller
    s->keys_owed = false;
    s->keys_external = true;
    s->clock.invalidate();
    return RSV_OK;
}

rsv_status rsv_distinct_candidates(rsv_sampler* s, const int64_t* hashes, int64_t n, int32_t mem, int64_t* n_cand) {
    if (rsv_status st = check_open(s)) return st;
    if (s->cfg.kind != RSV_KIND_DISTINCT)
        return fail(RSV_E_UNSUPPORTED, "rsv_distinct_candidates needs a DISTINCT sampler");
    if (s->cfg.hash_kind != RSV_HASH_PRECOMPUTED)
        return fail(RSV_E_UNSUPPORTED, "rsv_distinct_candidates needs RSV_HASH_PRECOMPUTED (the caller's hash of each element)");
    if (n < 0) return fail(RSV_E_ILLEGAL_ARGUMENT, "negative batch size");
    if (!n_cand) return fail(RSV_E_NULL_POINTER, "n_cand is NULL");
    if (n > 0 && !hashes) return fail(RSV_E_NULL_POINTER, "hashes is NULL");
    if (mem != RSV_MEM_HOST && mem != RSV_MEM_DEVICE)
        return fail(RSV_E_ILLEGAL_ARGUMENT, "mem must be RSV_MEM_HOST or RSV_MEM_DEVICE");
    DeviceGuard g(s->device);
    if (!s->obj) {
        // the first hash-only batch of a handle that has sampled nothing makes it index-only
        if (s->count + s->stage_n > 0)
            return fail(RSV_E_ILLEGAL_STATE, "rsv_distinct_candidates on a sampler that holds keys");
        JavaRandom r;  // RandomValues r0, r1 (Sampler.scala:385-388), as rsv_create draws them
        r.init((int64_t)s->cfg.seed);
        const int64_t r0 = r.next_long(), r1 = r.next_long();
        int st = RSV_OK;
        s->obj = obj_create((int32_t)s->k, r0, r1, &st);
        if (!s->obj) return (rsv_status)st;
        obj_set_timer(s->obj, &s->timer);
        s->keys_external = true;
    }
    touch(s);
    if (int rc = obj_candidates(s->obj, hashes, n, mem == RSV_MEM_DEVICE, s->count, s->stream, n_cand)) return (rsv_status)rc;
    s->clock.drained();  // obj_candidates returns with the stream drained
    s->cand_pending = true;
    s->cand_batch = n;
    return RSV_OK;
}

rsv_status rsv_candidates_read(rsv_sampler* s, int64_t* offsets_host, int64_t* hashes_host, int64_t cap) {
    if (!s) return fail(RSV_E_NULL_POINTER, "sampler is NULL");
    if (!s->cand_pending) return fail(RSV_E_ILLEGAL_STATE, "rsv_candidates_read without a pending rsv_distinct_candidates");
    const int64_t c = obj_pending_candidates(s->obj);
    if (cap < c) return fail(RSV_E_ILLEGAL_ARGUMENT, "cap is below the batch's candidate count");
    if (c > 0 && (!offsets_host || !hashes_host)) return fail(RSV_E_NULL_POINTER, "offsets_host/hashes_host is NULL");
    DeviceGuard g(s->device);
    return (rsv_status)obj_read(s->obj, offsets_host, hashes_host, s->stream);
}

rsv_status rsv_candidates_commit(rsv_sampler* s, int64_t set_size, int64_t max_hash) {
    if (!s) return fail(RSV_E_NULL_POINTER, "sampler is NULL");
    if (!s->cand_pending) return fail(RSV_E_ILLEGAL_STATE, "rsv_candidates_commit without a pending rsv_distinct_candidates");
    if (set_size < 0 || set_size > (int64_t)s->k) return fail(RSV_E_ILLEGAL_ARGUMENT, "set_size must be in [0, k]");
    obj_commit(s->obj, set_size, max_hash);
    s->count += s->cand_batch;
    s->cand_pending = false;
    return RSV_OK;
}

rsv_status rsv_candidates_abort(rsv_sampler* s) {
    if (!s) return fail(RSV_E_NULL_POINTER, "sampler is NULL");
    if (!s->cand_pending) return fail(RSV_E_ILLEGAL_STATE, "rsv_candidates_abort without a pending rsv_distinct_candidates");
    obj_abort(s->obj);
    s->cand_pending = false;
    return RSV_OK;
}

// result() / resultDevice() / the taken result: the first m keys of the set (DISTINCT) or of the slots
// (ELEMENTS; resultImpl, Sampler.scala:318-331) to the caller.  To the host they travel through the
// result's landing zone: published (flag wait, no copy, no stream synchronize) or pinned (D2H copy + stream
// synchronize).  The two kinds differ in their source, in how they publish when no recorded publication can
// be served, and in two rules of serving one:
//   need_last   DISTINCT serves a recorded (speculative) publication only while no group of work came after
//               it -- not every call that changes the set invalidates; ELEMENTS invalidates at each change of
//               the slots, so its publications outlive read-only groups (exports, a moved stream)
//   serve_once  DISTINCT serves a publication once: the next result() publishes again
static rsv_status result_impl(rsv_sampler* s, void* out, int64_t cap, int64_t* out_n, bool device_out,
                              bool take = false) {
    if (rsv_status st = check_keyed(s)) return st;
    if (!out_n) return fail(RSV_E_NULL_POINTER, "out_n is NULL");
    DeviceGuard g(s->device);
    if (rsv_status st = flush_stage(s)) return st;
    const bool distinct = s->cfg.kind == RSV_KIND_DISTINCT, need_last = distinct, serve_once = distinct;
    if (distinct)
        if (int rc = s->distinct->finalize(s->stream)) return (rsv_status)rc;
    const int64_t m = distinct ? s->distinct->size() : std::min<int64_t>(s->count, (int64_t)s->k);
    if (m > cap) return fail(RSV_E_ILLEGAL_ARGUMENT, "result buffer too small");
    if (m && !out && !take) return fail(RSV_E_NULL_POINTER, "out is NULL");
    // ELEMENTS with a count that came from rsv_seek alone: the slots were never written, and a recycled
    // block still holds its last sampler's keys -- the result is m empty (zero) slots
    if (m && !distinct)
        if (rsv_status st = ensure_slots(s)) return st;
    Landing& r = s->result;
    bool waited = false;
    if (m && device_out) {
        if (distinct) {
            if (int rc = s->distinct->export_set(out, nullptr, s->stream)) return (rsv_status)rc;
        } else {
            touch(s);
            RSV_HIP_TRY(hipMemcpyAsync(out, s->slots.sb.slot_key, m * s->kw, hipMemcpyDeviceToDevice, s->stream));
        }
    } else if (m) {
        if (rsv_status st = ensure_result_buffer(s)) return st;
        const void* src = distinct ? s->distinct->keys_dev() : s->slots.sb.slot_key;
        if (r.published()) {
            uint32_t gen = s->clock.pub_gen;
            if (!(need_last ? s->clock.current() : s->clock.holds())) {  // no publication of it: the publish launch
                touch(s);
                Publication pub;
                if (rsv_status st = begin_publish(s, true, m, &pub)) return st;
                gen = pub.gen;
                if (distinct) {
                    if (int rc = s->distinct->publish(pub.dst, pub.flag, gen, s->stream)) return (rsv_status)rc;
                } else {
                    RSV_HIP_TRY(launch_publish(src, m * s->kw, pub.dst, pub.flag, gen, s->stream));
                }
                record_publish(s, pub);
            }
            if (serve_once) s->clock.invalidate();
            if (rsv_status st = spin_flag(s, r.flag(), gen, "result publish")) return st;
            s->clock.seen(s->clock.pub_ops, gen, r.gen);  // the handle's last work: no stream synchronize
            waited = true;
        } else {  // large reservoirs through a pinned buffer: a pageable D2H costs a staged copy
            touch(s);
            RSV_HIP_TRY(hipMemcpyAsync(r.host(), src, m * s->kw, hipMemcpyDeviceToHost, s->stream));
        }
    }
    if (!waited) RSV_HIP_TRY(sync_stream(s));
    if (m && !device_out && !take) memcpy(out, r.host(), (size_t)m * s->kw);
    *out_n = m;
    if (!s->cfg.reusable) s->open = false;  // SingleUse.close, Sampler.scala:188-191, :345-350
    return RSV_OK;
}

rsv_status rsv_result(rsv_sampler* s, void* out, int64_t cap, int64_t* out_n) {
    return result_impl(s, out, cap, out_n, false);
}

rsv_status rsv_result_device(rsv_sampler* s, void* out_dev, int64_t cap, int64_t* out_n) {
    return result_impl(s, out_dev, cap, out_n, true);
}

rsv_status rsv_result_take(rsv_sampler* s, void** buf, int64_t* out_n) {
    if (rsv_status st = check_keyed(s)) return st;
    if (!buf || !out_n) return fail(RSV_E_NULL_POINTER, "buf / out_n is NULL");
    if (s->cfg.reusable || (int64_t)s->k * s->kw > kPublishMaxBytes)
        return fail(RSV_E_UNSUPPORTED, "rsv_result_take: single-use samplers with a published result only");
    {
        DeviceGuard g(s->device);
        if (rsv_status st = ensure_result_buffer(s)) return st;
    }
    // the published path of rsv_result, with the block handed over instead of copied: the caller's now
    // (rsv_host_release); a closed single-use handle publishes nothing more
    if (rsv_status st = result_impl(s, nullptr, s->k, out_n, false, /*take=*/true)) return st;
    *buf = s->result.give();
    return RSV_OK;
}

void rsv_host_release(void* buf) {
    if (buf) pool_host_free(buf);
}

int32_t rsv_is_open(const rsv_sampler* s) { return s && s->open ? 1 : 0; }

int64_t rsv_count(const rsv_sampler* s) { return s ? s->count + s->stage_n : 0; }

rsv_status rsv_set_stream(rsv_sampler* s, void* hip_stream) {
    if (rsv_status st = check_no_batch(s)) return st;
    DeviceGuard g(s->device);
    if (s->side.pending) touch(s);  // the hand-over covers the forked resolve too
    if (!s->clock.idle() && (hipStream_t)hip_stream != s->stream) {
        // stream-ordered hand-over, no host wait: the new stream waits for the work queued so far
        // (e.g. a combine moved to a communication stream while the next batch samples on the
        // first).  The event is the handle's own until rsv_destroy: handed back to the pool at
        // once, its next record elsewhere could land before the wait binds
        RSV_HIP_TRY(s->handover.ensure(s->device, hipEventDisableTiming));
        RSV_HIP_TRY(hipEventRecord(s->handover, s->stream));
        RSV_HIP_TRY(hipStreamWaitEvent((hipStream_t)hip_stream, s->handover, 0));
    }
    if (s->own_stream) pool_release_stream(s->device, s->stream);
    s->stream = (hipStream_t)hip_stream;
    s->own_stream = false;
    return RSV_OK;
}

void* rsv_get_stream(const rsv_sampler* s) { return s ? (void*)s->stream : nullptr; }

rsv_status rsv_set_resolve_stream(rsv_sampler* s, void* hip_stream) {
    if (rsv_status st = check_no_batch(s)) return st;
    if (s->cfg.kind != RSV_KIND_ELEMENTS) return fail(RSV_E_UNSUPPORTED, "rsv_set_resolve_stream: ELEMENTS samplers only");
    DeviceGuard g(s->device);
    if (s->side.pending) touch(s);
    s->side.rstream = (hipStream_t)hip_stream;
    return RSV_OK;
}

rsv_status rsv_synchronize(rsv_sampler* s) {
    if (rsv_status st = check_no_batch(s)) return st;
    DeviceGuard g(s->device);
    RSV_HIP_TRY(sync_stream(s));
    return RSV_OK;
}

rsv_status rsv_profile_enable(rsv_sampler* s, int32_t on) {
    if (rsv_status st = check_no_batch(s)) return st;
    s->timer.on = on != 0;
    return RSV_OK;
}

rsv_status rsv_profile_read(rsv_sampler* s, double* total_ms, int64_t* launches) {
    if (!s || !total_ms || !launches) return fail(RSV_E_NULL_POINTER, "NULL argument");
    if (rsv_status st = check_no_batch(s)) return st;
    DeviceGuard g(s->device);
    RSV_HIP_TRY(s->timer.drain());
    *total_ms = s->timer.total_ms;
    *launches = s->timer.launches;
    return RSV_OK;
}

rsv_status rsv_profile_global(int32_t on) {
    if (on < 0) return fail(RSV_E_ILLEGAL_ARGUMENT, "rsv_profile_global: negative sampling stride");
    std::lock_guard<std::mutex> lk(g_prof_mu);
    if (on) {
        g_prof_every = on;
        // the first timed launch is the (on / 2)-th, not the first: a region's first launch finds the
        // GPU idle, so its start event is stamped before the host has even submitted the kernel and
        // the pair would time the host's launch latency too (the 20-step bench: ~85 vs ~83 us)
        g_prof_seq = on - on / 2;
        // the timing events up front (128 pairs, on the current device), so that no event is
        // created inside the region being timed: at a 20-step bench region the lazily created
        // events of its 3 timed launches cost ~3 us per step (tools/probe_region.py)
        KernelTimer& t = global_timer();
        int dev = 0;
        if (hipGetDevice(&dev) == hipSuccess && (t.ev.empty() || t.device == dev)) {
            t.device = dev;
            hipEvent_t last = nullptr;
            while (t.ev.size() < 256) {
                hipEvent_t e;
                if (pool_event(&e, KernelTimer::kFlags) != hipSuccess) break;
                (void)hipEventRecord(e, nullptr);  // an event's first record may set it up
                t.ev.push_back(e);
                last = e;
            }
            if (last) (void)hipEventSynchronize(last);
        }
    }
    g_prof_on = on != 0;
    return RSV_OK;
}

rsv_status rsv_profile_global_read(double* total_ms, int64_t* launches) {
    if (!total_ms || !launches) return fail(RSV_E_NULL_POINTER, "NULL argument");
    std::lock_guard<std::mutex> lk(g_prof_mu);
    KernelTimer& t = global_timer();
    DeviceGuard g(t.device);
    RSV_HIP_TRY(t.drain());
    *total_ms = t.total_ms;
    *launches = t.launches;
    t.total_ms = 0;
    t.launches = 0;
    return RSV_OK;
}

rsv_status rsv_seek(rsv_sampler* s, int64_t index) {
    if (rsv_status st = check_open(s)) return st;
    if (s->cfg.kind != RSV_KIND_ELEMENTS || s->cfg.engine != RSV_ENGINE_PHILOX_R)
        return fail(RSV_E_UNSUPPORTED, "rsv_seek needs an ELEMENTS sampler on RSV_ENGINE_PHILOX_R");
    if (s->stage_n) {  // only staged per-element samples need the device here
        DeviceGuard g(s->device);
        if (rsv_status st = flush_stage(s)) return st;
    }
    if (index < s->count) return fail(RSV_E_ILLEGAL_ARGUMENT, "rsv_seek cannot move backwards");
    // a publication holds min(count, k) keys: once the count crosses k it covers too few
    if (std::min<int64_t>(index, s->k) != std::min<int64_t>(s->count, s->k)) s->clock.invalidate();
    s->count = index;
    return RSV_OK;
}

rsv_status rsv_export_state(rsv_sampler* s, int64_t* idx_dev, void* keys_dev, int64_t* hash_dev,
                            int64_t* out_n) {
    if (rsv_status st = check_keyed(s)) return st;
    if (!out_n) return fail(RSV_E_NULL_POINTER, "out_n is NULL");
    DeviceGuard g(s->device);
    touch(s);
    if (rsv_status st = flush_stage(s)) return st;
    if (s->cfg.kind == RSV_KIND_DISTINCT) {
        if (int rc = s->distinct->finalize(s->stream)) return (rsv_status)rc;
        if (int rc = s->distinct->export_set(keys_dev, hash_dev, s->stream)) return (rsv_status)rc;
        *out_n = s->distinct->size();
    } else {
        if (rsv_status st = ensure_slots(s)) return st;
        if (idx_dev) RSV_HIP_TRY(hipMemcpyAsync(idx_dev, s->slots.sb.slot_idx, s->k * 8ull, hipMemcpyDeviceToDevice, s->stream));
        if (keys_dev)
            RSV_HIP_TRY(hipMemcpyAsync(keys_dev, s->slots.sb.slot_key, (size_t)s->k * s->kw, hipMemcpyDeviceToDevice, s->stream));
        *out_n = s->k;
    }
    // on the handle's private stream the caller cannot order against it: wait; on a caller
    // stream (rsv_set_stream) the copies are stream-ordered for the caller's next work
    if (s->own_stream) RSV_HIP_TRY(sync_stream(s));
    return RSV_OK;
}

rsv_status rsv_merge_state(rsv_sampler* s, const int64_t* idx_dev, const void* keys_dev, const int64_t* hash_dev,
                           const int64_t* part_n_host, int32_t parts, int64_t part_len, int64_t total_count) {
    if (rsv_status st = check_keyed(s)) return st;
    if (parts < 0 || part_len < 0) return fail(RSV_E_ILLEGAL_ARGUMENT, "negative parts/part_len");
    if (parts > 0 && !keys_dev) return fail(RSV_E_NULL_POINTER, "keys_dev is NULL");
    DeviceGuard g(s->device);
    touch(s);
    if (rsv_status st = flush_stage(s)) return st;
    if (s->cfg.kind == RSV_KIND_DISTINCT) {
        if (parts > 0 && (!hash_dev || !part_n_host)) return fail(RSV_E_NULL_POINTER, "hash_dev/part_n is NULL");
        if (parts > 0)
            if (int rc = s->distinct->merge_parts(keys_dev, hash_dev, part_n_host, parts, part_len, s->stream))
                return (rsv_status)rc;
    } else {
        if (part_len < (int64_t)s->k) return fail(RSV_E_ILLEGAL_ARGUMENT, "part_len < k");
        if (parts > 0 && !idx_dev) return fail(RSV_E_NULL_POINTER, "idx_dev is NULL");
        if (rsv_status st = ensure_slots(s)) return st;
        RSV_HIP_TRY(launch_merge_slots(idx_dev, keys_dev, parts, part_len, slot_block(s), s->stream));
        s->clock.invalidate();
    }
    if (total_count > s->count) s->count = total_count;
    if (s->own_stream) RSV_HIP_TRY(sync_stream(s));
    return RSV_OK;
}

static rsv_status check_distinct(rsv_sampler* s, const char* what) {
    if (rsv_status st = check_open(s)) return st;
    if (s->cfg.kind != RSV_KIND_DISTINCT) return fail(RSV_E_UNSUPPORTED, std::string(what) + " needs a DISTINCT sampler");
    if (s->obj)  // the set lives with the caller
        return fail(RSV_E_ILLEGAL_STATE, std::string(what) + ": the handle holds no keys (rsv_distinct_candidates)");
    return RSV_OK;
}

rsv_status rsv_get_distinct_info(rsv_sampler* s, rsv_distinct_info* out) {
    if (rsv_status st = check_distinct(s, "rsv_get_distinct_info")) return st;
    if (!out) return fail(RSV_E_NULL_POINTER, "out is NULL");
    if (out->struct_size < sizeof(rsv_distinct_info)) return fail(RSV_E_ILLEGAL_ARGUMENT, "struct_size too small");
    DeviceGuard g(s->device);
    touch(s);
    if (rsv_status st = flush_stage(s)) return st;
    if (int rc = s->distinct->settle(s->stream)) return (rsv_status)rc;
    s->distinct->info(&out->ordered, &out->tied, &out->log_retained, &out->size, &out->max_hash,
                  &out->log_entries, &out->sched_passes, &out->sched_fallbacks);
    return RSV_OK;
}

rsv_status rsv_export_log(rsv_sampler* s, int64_t bound, int64_t* hashes_host, void* keys_host, int64_t cap,
                          int64_t* out_n) {
    if (rsv_status st = check_distinct(s, "rsv_export_log")) return st;
    if (!out_n) return fail(RSV_E_NULL_POINTER, "out_n is NULL");
    if (cap < 0) return fail(RSV_E_ILLEGAL_ARGUMENT, "negative cap");
    if (cap > 0 && (!hashes_host || !keys_host)) return fail(RSV_E_NULL_POINTER, "hashes_host/keys_host is NULL");
    if (cap == 0) hashes_host = nullptr, keys_host = nullptr;  // count-only query
    DeviceGuard g(s->device);
    touch(s);
    if (rsv_status st = flush_stage(s)) return st;
    return (rsv_status)s->distinct->log_export(bound, hashes_host, keys_host, cap, out_n, s->stream);
}

rsv_status rsv_merge_log(rsv_sampler* s, const int64_t* hashes_host, const void* keys_host, int64_t n,
                         int64_t total_count) {
    if (rsv_status st = check_distinct(s, "rsv_merge_log")) return st;
    if (n < 0) return fail(RSV_E_ILLEGAL_ARGUMENT, "negative n");
    if (n > 0 && (!hashes_host || !keys_host)) return fail(RSV_E_NULL_POINTER, "hashes_host/keys_host is NULL");
    DeviceGuard g(s->device);
    touch(s);
    if (rsv_status st = flush_stage(s)) return st;
    if (int rc = s->distinct->log_merge(hashes_host, keys_host, n, total_count, s->stream))
        return (rsv_status)rc;
    if (total_count > s->count) s->count = total_count;
    s->clock.invalidate();
    if (s->own_stream) RSV_HIP_TRY(sync_stream(s));
    return RSV_OK;
}

rsv_status rsv_retain_log(rsv_sampler* s, int32_t on) {
    if (rsv_status st = check_distinct(s, "rsv_retain_log")) return st;
    s->distinct->retain_log(on != 0);
    return RSV_OK;
}

rsv_status rsv_export_packed(rsv_sampler* s, int64_t* row_dev) {
    if (rsv_status st = check_keyed(s)) return st;
    if (!row_dev) return fail(RSV_E_NULL_POINTER, "row_dev is NULL");
    DeviceGuard g(s->device);
    touch(s);
    if (rsv_status st = flush_stage(s)) return st;
    if (s->cfg.kind == RSV_KIND_DISTINCT) {
        if (int rc = s->distinct->export_row(row_dev, s->count, s->stream)) return (rsv_status)rc;
        if (s->own_stream) RSV_HIP_TRY(sync_stream(s));
        return RSV_OK;
    }
    if (rsv_status st = ensure_slots(s)) return st;
    RSV_HIP_TRY(launch_export_packed(slot_block(s), row_dev, s->stream));
    if (s->own_stream) RSV_HIP_TRY(sync_stream(s));
    return RSV_OK;
}

rsv_status rsv_merge_packed(rsv_sampler* s, const int64_t* rows_dev, int32_t parts, int64_t row_stride,
                            int64_t total_count) {
    if (rsv_status st = check_keyed(s)) return st;
    if (parts < 0) return fail(RSV_E_ILLEGAL_ARGUMENT, "negative parts");
    if (s->cfg.kind == RSV_KIND_DISTINCT) {
        // [keys (k, as int64 words: key_width / 8 each for byte keys) | hashes (k) | 6 meta words]
        const int64_t row_len = (int64_t)s->k * (1 + (s->kw > 8 ? s->kw / 8 : 1)) + 6;
        if (row_stride < row_len) return fail(RSV_E_ILLEGAL_ARGUMENT, "row_stride shorter than a packed row");
        if (parts > 0 && !rows_dev) return fail(RSV_E_NULL_POINTER, "rows_dev is NULL");
        DeviceGuard g(s->device);
        touch(s);
        if (rsv_status st = flush_stage(s)) return st;
        if (int rc = s->distinct->merge_rows(rows_dev, parts, row_stride, s->stream)) return (rsv_status)rc;
        if (total_count > s->count) s->count = total_count;
        s->clock.invalidate();
        if (s->own_stream) {  // the call returns with its work done: settle now, while the rows are the caller's
            RSV_HIP_TRY(sync_stream(s));
            if (int rc = s->distinct->settle(s->stream)) return (rsv_status)rc;
        }
        return RSV_OK;
    }
    const int64_t row_min = (int64_t)s->k * (1 + (s->kw > 8 ? s->kw / 8 : 1));  // [idx(k) | keys]
    if (row_stride < row_min) return fail(RSV_E_ILLEGAL_ARGUMENT, "row_stride shorter than a packed row");
    if (parts > 0 && !rows_dev) return fail(RSV_E_NULL_POINTER, "rows_dev is NULL");
    DeviceGuard g(s->device);
    touch(s);
    if (rsv_status st = flush_stage(s)) return st;
    if (rsv_status st = ensure_slots(s)) return st;
    if (total_count > s->count) {
        // a publication holds min(count, k) keys: once the count crosses k it covers too few (rsv_seek)
        if (std::min<int64_t>(total_count, s->k) != std::min<int64_t>(s->count, s->k)) s->clock.invalidate();
        s->count = total_count;
    }
    if (parts > 0) {  // for small reservoirs of Int / Long keys: merge + publish in one dispatch
        Publication pub;
        if (rsv_status st = begin_publish(s, s->k <= kFusedPublishMaxK && s->kw <= 8, s->count, &pub)) return st;
        RSV_HIP_TRY(launch_merge_packed(rows_dev, parts, row_stride, slot_block(s), pub, s->stream));
        record_publish(s, pub);
    }
    if (s->own_stream) RSV_HIP_TRY(sync_stream(s));
    return RSV_OK;
}

// k and key_width of the six K2 entry points (fn: the entry point's name, for the messages; long_fn: for
// the three over byte keys, their counterpart for 4- and 8-byte keys, else NULL; state: the four resumed
// ones, whose k is bounded)
static rsv_status check_segsample_shape(const char* fn, const char* long_fn, int32_t k, int32_t key_width,
                                        bool state) {
    if (k <= 0 || k > kMaxSize) return fail(RSV_E_ILLEGAL_ARGUMENT, "k out of range");
    if (state && k > (int32_t)kSegSampleStateMaxK)
        return fail(RSV_E_UNSUPPORTED, std::string(fn) + " holds k <= " + std::to_string(kSegSampleStateMaxK) +
                                           " per stream; use separate handles beyond");
    if (!long_fn)
        return key_width == 4 || key_width == 8 ? RSV_OK : fail(RSV_E_ILLEGAL_ARGUMENT, "key_width must be 4 or 8");
    if (key_width == 4 || key_width == 8)
        return fail(RSV_E_UNSUPPORTED, std::string(fn) + " takes byte keys; " + long_fn + " takes 4- and 8-byte keys");
    if (key_width < 16 || key_width > 256 || key_width % 8 != 0)
        return fail(RSV_E_ILLEGAL_ARGUMENT, "key_width must be a multiple of 8 in 16..256");
    return RSV_OK;
}

// the counts of the two update and the two merge entry points, after a shape check that left st RSV_OK;
// true: the call returns st -- an error, or RSV_OK because there is nothing to do
static bool segsample_update_done(int64_t num_segments, int64_t num_states, const void* ids_dev, rsv_status& st) {
    if (num_segments < 0 || num_states < 0) st = fail(RSV_E_ILLEGAL_ARGUMENT, "negative segment or state count");
    else if (!ids_dev && num_segments > num_states)
        st = fail(RSV_E_ILLEGAL_ARGUMENT, "more segments than state rows without stream_ids_dev");
    return st || num_segments == 0 || num_states == 0;
}
static bool segsample_merge_done(int32_t parts, int64_t num_states, rsv_status& st) {
    if (parts < 0 || num_states < 0) st = fail(RSV_E_ILLEGAL_ARGUMENT, "negative part or state count");
    return st || parts == 0 || num_states == 0;
}

rsv_status rsv_sample_segmented(const void* keys_dev, const int64_t* offsets_dev, int64_t num_streams,
                                int32_t key_width, int32_t k, uint64_t seed, uint64_t stream_base, void* out_dev,
                                int64_t* counts_dev, void* hip_stream) {
    if (rsv_status st = check_segsample_shape("rsv_sample_segmented", nullptr, k, key_width, false)) return st;
    if (num_streams < 0) return fail(RSV_E_ILLEGAL_ARGUMENT, "negative stream count");
    if (num_streams == 0) return RSV_OK;
    if (!offsets_dev || !out_dev || !counts_dev) return fail(RSV_E_NULL_POINTER, "NULL buffer");
    const DrawParams dp{seed, stream_base};
    RSV_HIP_TRY(launch_segmented(keys_dev, key_width, offsets_dev, num_streams, (uint32_t)k, dp, out_dev, counts_dev,
                                 (hipStream_t)hip_stream));
    return RSV_OK;
}

rsv_status rsv_sample_segmented_update(const void* keys_dev, const int64_t* offsets_dev, const int64_t* stream_ids_dev,
                                       const int64_t* bases_dev, int64_t num_segments, int64_t num_states,
                                       int32_t key_width, int32_t k, uint64_t seed, uint64_t stream_base,
                                       void* state_keys_dev, int64_t* state_idx_dev, int64_t* state_next_dev,
                                       void* hip_stream) {
    rsv_status st = check_segsample_shape("rsv_sample_segmented_update", nullptr, k, key_width, true);
    if (st || segsample_update_done(num_segments, num_states, stream_ids_dev, st)) return st;
    // keys_dev is not checked: a launch whose segments are all empty has no keys
    if (!offsets_dev || !state_keys_dev || !state_idx_dev || !state_next_dev)
        return fail(RSV_E_NULL_POINTER, "NULL buffer");
    const DrawParams dp{seed, stream_base};
    RSV_HIP_TRY(launch_segmented_update(keys_dev, key_width, offsets_dev, stream_ids_dev, bases_dev, num_segments,
                                        num_states, (uint32_t)k, dp, state_keys_dev, state_idx_dev, state_next_dev,
                                        (hipStream_t)hip_stream));
    return RSV_OK;
}

rsv_status rsv_sample_segmented_merge(const void* part_keys_dev, const int64_t* part_idx_dev,
                                      const int64_t* part_next_dev, int32_t parts, int64_t num_states,
                                      int32_t key_width, int32_t k, void* state_keys_dev, int64_t* state_idx_dev,
                                      int64_t* state_next_dev, void* hip_stream) {
    rsv_status st = check_segsample_shape("rsv_sample_segmented_merge", nullptr, k, key_width, true);
    if (st || segsample_merge_done(parts, num_states, st)) return st;
    if (!part_keys_dev || !part_idx_dev || !part_next_dev || !state_keys_dev || !state_idx_dev || !state_next_dev)
        return fail(RSV_E_NULL_POINTER, "NULL buffer");
    RSV_HIP_TRY(launch_segmented_merge(part_keys_dev, key_width, part_idx_dev, part_next_dev, parts, num_states,
                                       (uint32_t)k, state_keys_dev, state_idx_dev, state_next_dev,
                                       (hipStream_t)hip_stream));
    return RSV_OK;
}

rsv_status rsv_sample_segmented_rows(const void* rows_dev, const int64_t* offsets_dev, int64_t num_streams,
                                     int32_t key_width, int32_t k, uint64_t seed, uint64_t stream_base,
                                     void* out_rows_dev, int64_t* counts_dev, void* hip_stream) {
    if (rsv_status st = check_segsample_shape("rsv_sample_segmented_rows", "rsv_sample_segmented", k, key_width, false))
        return st;
    if (num_streams < 0) return fail(RSV_E_ILLEGAL_ARGUMENT, "negative stream count");
    if (num_streams == 0) return RSV_OK;
    // rows_dev is not checked: a launch whose streams are all empty has no rows
    if (!offsets_dev || !out_rows_dev || !counts_dev) return fail(RSV_E_NULL_POINTER, "NULL buffer");
    if (((uintptr_t)rows_dev | (uintptr_t)out_rows_dev) & 7)
        return fail(RSV_E_ILLEGAL_ARGUMENT, "rows_dev and out_rows_dev must be 8-byte aligned");
    const DrawParams dp{seed, stream_base};
    RSV_HIP_TRY(launch_segmented_rows(rows_dev, key_width, offsets_dev, num_streams, (uint32_t)k, dp, out_rows_dev,
                                      counts_dev, (hipStream_t)hip_stream));
    return RSV_OK;
}

rsv_status rsv_sample_segmented_rows_update(const void* rows_dev, const int64_t* offsets_dev,
                                            const int64_t* stream_ids_dev, const int64_t* bases_dev,
                                            int64_t num_segments, int64_t num_states, int32_t key_width, int32_t k,
                                            uint64_t seed, uint64_t stream_base, void* state_rows_dev,
                                            int64_t* state_idx_dev, int64_t* state_next_dev, void* hip_stream) {
    rsv_status st =
        check_segsample_shape("rsv_sample_segmented_rows_update", "rsv_sample_segmented_update", k, key_width, true);
    if (st || segsample_update_done(num_segments, num_states, stream_ids_dev, st)) return st;
    // rows_dev is not checked: a launch whose segments are all empty has no rows
    if (!offsets_dev || !state_rows_dev || !state_idx_dev || !state_next_dev)
        return fail(RSV_E_NULL_POINTER, "NULL buffer");
    if (((uintptr_t)rows_dev | (uintptr_t)state_rows_dev) & 7)
        return fail(RSV_E_ILLEGAL_ARGUMENT, "rows_dev and state_rows_dev must be 8-byte aligned");
    const DrawParams dp{seed, stream_base};
    RSV_HIP_TRY(launch_segmented_rows_update(rows_dev, key_width, offsets_dev, stream_ids_dev, bases_dev, num_segments,
                                             num_states, (uint32_t)k, dp, state_rows_dev, state_idx_dev,
                                             state_next_dev, (hipStream_t)hip_stream));
    return RSV_OK;
}

rsv_status rsv_sample_segmented_rows_merge(const void* part_rows_dev, const int64_t* part_idx_dev,
                                           const int64_t* part_next_dev, int32_t parts, int64_t num_states,
                                           int32_t key_width, int32_t k, void* state_rows_dev, int64_t* state_idx_dev,
                                           int64_t* state_next_dev, void* hip_stream) {
    rsv_status st =
        check_segsample_shape("rsv_sample_segmented_rows_merge", "rsv_sample_segmented_merge", k, key_width, true);
    if (st || segsample_merge_done(parts, num_states, st)) return st;
    if (!part_rows_dev || !part_idx_dev || !part_next_dev || !state_rows_dev || !state_idx_dev || !state_next_dev)
        return fail(RSV_E_NULL_POINTER, "NULL buffer");
    if (((uintptr_t)part_rows_dev | (uintptr_t)state_rows_dev) & 7)
        return fail(RSV_E_ILLEGAL_ARGUMENT, "part_rows_dev and state_rows_dev must be 8-byte aligned");
    RSV_HIP_TRY(launch_segmented_rows_merge(part_rows_dev, key_width, part_idx_dev, part_next_dev, parts, num_states,
                                            (uint32_t)k, state_rows_dev, state_idx_dev, state_next_dev,
                                            (hipStream_t)hip_stream));
    return RSV_OK;
}

// ---- the by-id front door: the grouping pass and the two updates that read through its permutation ----
rsv_status rsv_group_by_stream(const void* ids_dev, int32_t id_width, int64_t n, int64_t num_states,
                               int64_t* offsets_dev, int32_t* order_dev, void* hip_stream) {
    if (!offsets_dev) return fail(RSV_E_NULL_POINTER, "offsets_dev is NULL");
    if (n > 0 && !order_dev) return fail(RSV_E_NULL_POINTER, "order_dev is NULL");
    if (n > 0 && !ids_dev) return fail(RSV_E_NULL_POINTER, "ids_dev is NULL");
    if (n < 0) return fail(RSV_E_ILLEGAL_ARGUMENT, "negative n");
    if (num_states < 1) return fail(RSV_E_ILLEGAL_ARGUMENT, "num_states must be at least 1");
    if (id_width != 4 && id_width != 8) return fail(RSV_E_UNSUPPORTED, "id_width must be 4 (int32) or 8 (int64)");
    if (n > kGroupMaxN)
        return fail(RSV_E_UNSUPPORTED, "rsv_group_by_stream takes n <= 2147483647 (2^31 - 1) per call: order_dev is int32");
    if (num_states > kGroupMaxStates)
        return fail(RSV_E_UNSUPPORTED, "rsv_group_by_stream takes num_states <= 4294967294 (2^32 - 2): the bins are 32-bit");
    RSV_HIP_TRY(launch_group_by_stream(ids_dev, id_width, n, num_states, offsets_dev, order_dev,
                                       (hipStream_t)hip_stream));
    return RSV_OK;
}

rsv_status rsv_sample_segmented_update_indirect(const void* keys_dev, int64_t n_keys, const int32_t* order_dev,
                                                const int64_t* offsets_dev, const int64_t* stream_ids_dev,
                                                const int64_t* bases_dev, int64_t num_segments, int64_t num_states,
                                                int32_t key_width, int32_t k, uint64_t seed, uint64_t stream_base,
                                                void* state_keys_dev, int64_t* state_idx_dev, int64_t* state_next_dev,
                                                void* hip_stream) {
    rsv_status st = check_segsample_shape("rsv_sample_segmented_update_indirect", nullptr, k, key_width, true);
    if (st || segsample_update_done(num_segments, num_states, stream_ids_dev, st)) return st;
    if (n_keys < 0) return fail(RSV_E_ILLEGAL_ARGUMENT, "negative n_keys");
    // keys_dev is not checked: a launch whose segments are all empty has no keys
    if (!order_dev) return fail(RSV_E_NULL_POINTER, "order_dev is NULL");
    if (!offsets_dev || !state_keys_dev || !state_idx_dev || !state_next_dev)
        return fail(RSV_E_NULL_POINTER, "NULL buffer");
    const DrawParams dp{seed, stream_base};
    RSV_HIP_TRY(launch_segmented_update_indirect(keys_dev, n_keys, order_dev, key_width, offsets_dev, stream_ids_dev,
                                                 bases_dev, num_segments, num_states, (uint32_t)k, dp, state_keys_dev,
                                                 state_idx_dev, state_next_dev, (hipStream_t)hip_stream));
    return RSV_OK;
}

rsv_status rsv_sample_segmented_rows_update_indirect(const void* rows_dev, int64_t n_rows, const int32_t* order_dev,
                                                     const int64_t* offsets_dev, const int64_t* stream_ids_dev,
                                                     const int64_t* bases_dev, int64_t num_segments,
                                                     int64_t num_states, int32_t key_width, int32_t k, uint64_t seed,
                                                     uint64_t stream_base, void* state_rows_dev,
                                                     int64_t* state_idx_dev, int64_t* state_next_dev,
                                                     void* hip_stream) {
    rsv_status st = check_segsample_shape("rsv_sample_segmented_rows_update_indirect",
                                          "rsv_sample_segmented_update_indirect", k, key_width, true);
    if (st || segsample_update_done(num_segments, num_states, stream_ids_dev, st)) return st;
    if (n_rows < 0) return fail(RSV_E_ILLEGAL_ARGUMENT, "negative n_rows");
    // rows_dev is not checked: a launch whose segments are all empty has no rows
    if (!order_dev) return fail(RSV_E_NULL_POINTER, "order_dev is NULL");
    if (!offsets_dev || !state_rows_dev || !state_idx_dev || !state_next_dev)
        return fail(RSV_E_NULL_POINTER, "NULL buffer");
    if (((uintptr_t)rows_dev | (uintptr_t)state_rows_dev) & 7)
        return fail(RSV_E_ILLEGAL_ARGUMENT, "rows_dev and state_rows_dev must be 8-byte aligned");
    const DrawParams dp{seed, stream_base};
    RSV_HIP_TRY(launch_segmented_rows_update_indirect(rows_dev, n_rows, order_dev, key_width, offsets_dev,
                                                      stream_ids_dev, bases_dev, num_segments, num_states, (uint32_t)k,
                                                      dp, state_rows_dev, state_idx_dev, state_next_dev,
                                                      (hipStream_t)hip_stream));
    return RSV_OK;
}

// the three keyless entry points: the checks of their keyed siblings, in their order, without a key width
rsv_status rsv_sample_segmented_indexed(const int64_t* offsets_dev, int64_t num_streams, int32_t k, uint64_t seed,
                                        uint64_t stream_base, int64_t* out_idx_dev, int64_t* counts_dev,
                                        void* hip_stream) {
    if (rsv_status st = check_segsample_shape("rsv_sample_segmented_indexed", nullptr, k, 8, false)) return st;
    if (num_streams < 0) return fail(RSV_E_ILLEGAL_ARGUMENT, "negative stream count");
    if (num_streams == 0) return RSV_OK;
    if (!offsets_dev || !out_idx_dev || !counts_dev) return fail(RSV_E_NULL_POINTER, "NULL buffer");
    const DrawParams dp{seed, stream_base};
    RSV_HIP_TRY(launch_segmented_indexed(offsets_dev, num_streams, (uint32_t)k, dp, out_idx_dev, counts_dev,
                                         (hipStream_t)hip_stream));
    return RSV_OK;
}

rsv_status rsv_sample_segmented_indexed_update(const int64_t* offsets_dev, const int64_t* stream_ids_dev,
                                               const int64_t* bases_dev, int64_t num_segments, int64_t num_states,
                                               int32_t k, uint64_t seed, uint64_t stream_base, int64_t* state_idx_dev,
                                               int64_t* state_next_dev, int64_t* hits_dev, int64_t* hit_counts_dev,
                                               void* hip_stream) {
    rsv_status st = check_segsample_shape("rsv_sample_segmented_indexed_update", nullptr, k, 8, true);
    if (st || segsample_update_done(num_segments, num_states, stream_ids_dev, st)) return st;
    if (!offsets_dev || !state_idx_dev || !state_next_dev || !hits_dev || !hit_counts_dev)
        return fail(RSV_E_NULL_POINTER, "NULL buffer");
    const DrawParams dp{seed, stream_base};
    RSV_HIP_TRY(launch_segmented_indexed_update(offsets_dev, stream_ids_dev, bases_dev, num_segments, num_states,
                                                (uint32_t)k, dp, state_idx_dev, state_next_dev, hits_dev,
                                                hit_counts_dev, (hipStream_t)hip_stream));
    return RSV_OK;
}

rsv_status rsv_sample_segmented_indexed_merge(const int64_t* part_idx_dev, const int64_t* part_next_dev, int32_t parts,
                                              int64_t num_states, int32_t k, int64_t* state_idx_dev,
                                              int64_t* state_next_dev, int32_t* src_dev, void* hip_stream) {
    rsv_status st = check_segsample_shape("rsv_sample_segmented_indexed_merge", nullptr, k, 8, true);
    if (st || segsample_merge_done(parts, num_states, st)) return st;
    if (!part_idx_dev || !part_next_dev || !state_idx_dev || !state_next_dev || !src_dev)
        return fail(RSV_E_NULL_POINTER, "NULL buffer");
    RSV_HIP_TRY(launch_segmented_indexed_merge(part_idx_dev, part_next_dev, parts, num_states, (uint32_t)k,
                                               state_idx_dev, state_next_dev, src_dev, (hipStream_t)hip_stream));
    return RSV_OK;
}

// ---- K5: the ten rsv_distinct_segmented* entry points ----
// What an entry point tells its checker about itself, and what the checker tells it (hk, st).  There are three
// checkers, one per kind of call (stateless, update, merge); each holds that kind's checks once, in the one order they
// fire in.
struct SegDistinctCall {
    const char* fn;                 // the entry point's name, for the messages
    const char* long_fn = nullptr;  // over byte keys: its counterpart for 4- and 8-byte keys; NULL: it is that one
    const char* needs = nullptr;    // the one more pointer it requires, as its message names it; NULL: none
    const void* needed = nullptr;   // that pointer
    int hk = RSV_HASH_PRECOMPUTED;  // the hash kind, resolved (a merge takes its hashes as stored)
    rsv_status st = RSV_OK;         // what the call returns when its checker says it is done
    bool rows() const { return long_fn != nullptr; }
};

static rsv_status check_segdistinct_shape(const SegDistinctCall& c, int32_t k, int32_t key_width) {
    if (k <= 0 || k > kMaxSize) return fail(RSV_E_ILLEGAL_ARGUMENT, "k out of range");
    if (k > (int32_t)kSegDistinctMaxK)
        return fail(RSV_E_UNSUPPORTED, std::string(c.fn) + " holds k <= " + std::to_string(kSegDistinctMaxK) +
                                           " per stream; use separate handles beyond");
    if (!c.rows()) {
        if (key_width > 8 && key_width <= 256 && key_width % 8 == 0)
            return fail(RSV_E_UNSUPPORTED, std::string(c.fn) + " takes 4- and 8-byte keys, not byte keys");
        if (key_width != 4 && key_width != 8) return fail(RSV_E_ILLEGAL_ARGUMENT, "key_width must be 4 or 8");
        return RSV_OK;
    }
    if (key_width == 4 || key_width == 8)
        return fail(RSV_E_UNSUPPORTED, std::string(c.fn) + " takes byte keys; " + c.long_fn + " takes 4- and 8-byte keys");
    if (key_width < 16 || key_width > 256 || key_width % 8 != 0)
        return fail(RSV_E_ILLEGAL_ARGUMENT, "key_width must be a multiple of 8 in 16..256");
    return RSV_OK;
}

// the hash kind of the entry points that hash: its range; RSV_HASH_DEFAULT resolved by key width for 4- and 8-byte
// keys; over byte keys PRECOMPUTED, or DEFAULT (UUID.hashCode) at key_width 16
static rsv_status resolve_segdistinct_hash(SegDistinctCall& c, int32_t hash_kind, int32_t key_width) {
    if (hash_kind < RSV_HASH_DEFAULT || hash_kind > RSV_HASH_PRECOMPUTED)
        return fail(RSV_E_ILLEGAL_ARGUMENT, "unknown hash kind");
    c.hk = hash_kind;
    if (!c.rows()) {
        if (hash_kind == RSV_HASH_DEFAULT) c.hk = key_width == 4 ? RSV_HASH_JAVA_INT : RSV_HASH_JAVA_LONG;
        return RSV_OK;
    }
    if (hash_kind != RSV_HASH_DEFAULT && hash_kind != RSV_HASH_PRECOMPUTED)
        return fail(RSV_E_UNSUPPORTED, "byte keys take RSV_HASH_PRECOMPUTED, or RSV_HASH_DEFAULT (UUID.hashCode) at key_width 16");
    if (hash_kind == RSV_HASH_DEFAULT && key_width != 16)
        return fail(RSV_E_UNSUPPORTED, "RSV_HASH_DEFAULT is UUID.hashCode: key_width 16 only");
    return RSV_OK;
}

// the pointers, behind the counts: the buffers every call of the kind needs (present: none of them is NULL; the keys
// or rows of a stateless or update call are not among them: a launch whose streams are all empty has none), the one
// more the entry point names, hashes_dev under RSV_HASH_PRECOMPUTED (otherwise the launch gets NULL for it), and over
// byte keys the alignment of the two row buffers, last
static rsv_status check_segdistinct_buffers(const SegDistinctCall& c, bool present, const int64_t*& hashes_dev,
                                            const void* rows_in, const void* rows_out, const char* unaligned) {
    if (!present) return fail(RSV_E_NULL_POINTER, "NULL buffer");
    if (c.needs && !c.needed) return fail(RSV_E_NULL_POINTER, std::string(c.fn) + " needs " + c.needs);
    if (c.hk != RSV_HASH_PRECOMPUTED) hashes_dev = nullptr;
    else if (!hashes_dev) return fail(RSV_E_NULL_POINTER, "RSV_HASH_PRECOMPUTED needs hashes_dev");
    if (c.rows() && (((uintptr_t)rows_in | (uintptr_t)rows_out) & 7)) return fail(RSV_E_ILLEGAL_ARGUMENT, unaligned);
    return RSV_OK;
}

// The three checkers.  true: the call returns c.st -- an error, or RSV_OK because there is nothing to do.
static bool segdistinct_stateless_done(SegDistinctCall& c, int32_t k, int32_t key_width, int32_t hash_kind,
                                       int64_t num_streams, bool present, const int64_t*& hashes_dev, const void* in_dev,
                                       const void* out_dev) {
    if ((c.st = check_segdistinct_shape(c, k, key_width)) || (c.st = resolve_segdistinct_hash(c, hash_kind, key_width)))
        return true;
    if (num_streams < 0) c.st = fail(RSV_E_ILLEGAL_ARGUMENT, "negative stream count");
    if (c.st || num_streams == 0) return true;
    c.st = check_segdistinct_buffers(c, present, hashes_dev, in_dev, out_dev, "rows_dev and out_rows_dev must be 8-byte aligned");
    return c.st != RSV_OK;
}

static bool segdistinct_update_done(SegDistinctCall& c, int32_t k, int32_t key_width, int32_t hash_kind,
                                    int64_t num_segments, int64_t num_states, const void* ids_dev, bool present,
                                    const int64_t*& hashes_dev, const void* in_dev, const void* state_dev) {
    if ((c.st = check_segdistinct_shape(c, k, key_width)) || (c.st = resolve_segdistinct_hash(c, hash_kind, key_width)))
        return true;
    if (num_segments < 0 || num_states < 0) c.st = fail(RSV_E_ILLEGAL_ARGUMENT, "negative segment or state count");
    else if (!ids_dev && num_segments > num_states)
        c.st = fail(RSV_E_ILLEGAL_ARGUMENT, "more segments than state rows without stream_ids_dev");
    if (c.st || num_segments == 0 || num_states == 0) return true;
    c.st = check_segdistinct_buffers(c, present, hashes_dev, in_dev, state_dev, "rows_dev and state_rows_dev must be 8-byte aligned");
    return c.st != RSV_OK;
}

static bool segdistinct_merge_done(SegDistinctCall& c, int32_t k, int32_t key_width, int32_t parts, int64_t num_states,
                                   bool present, const int64_t* part_hashes_dev, const void* part_dev, const void* state_dev) {
    if ((c.st = check_segdistinct_shape(c, k, key_width))) return true;
    if (parts < 0 || num_states < 0) c.st = fail(RSV_E_ILLEGAL_ARGUMENT, "negative part or state count");
    if (c.st || parts == 0 || num_states == 0) return true;
    c.st = check_segdistinct_buffers(c, present, part_hashes_dev, part_dev, state_dev,
                                     "part_rows_dev and state_rows_dev must be 8-byte aligned");
    return c.st != RSV_OK;
}

rsv_status rsv_distinct_segmented(const void* keys_dev, const int64_t* hashes_dev, const int64_t* offsets_dev,
                                  int64_t num_streams, int32_t key_width, int32_t k, int32_t hash_kind, uint64_t seed,
                                  uint64_t stream_base, void* out_keys_dev, int64_t* out_hashes_dev,
                                  int64_t* counts_dev, void* hip_stream) {
    SegDistinctCall c{"rsv_distinct_segmented"};
    if (segdistinct_stateless_done(c, k, key_width, hash_kind, num_streams, offsets_dev && out_keys_dev && counts_dev,
                                   hashes_dev, keys_dev, out_keys_dev))
        return c.st;
    RSV_HIP_TRY(launch_segdistinct(keys_dev, key_width, hashes_dev, offsets_dev, num_streams, (uint32_t)k, c.hk,
                                   seed + stream_base, out_keys_dev, out_hashes_dev, counts_dev, (hipStream_t)hip_stream));
    return RSV_OK;
}

rsv_status rsv_distinct_segmented_ordered(const void* keys_dev, const int64_t* hashes_dev, const int64_t* offsets_dev,
                                          int64_t num_streams, int32_t key_width, int32_t k, int32_t hash_kind,
                                          uint64_t seed, uint64_t stream_base, void* out_keys_dev,
                                          int64_t* out_hashes_dev, int64_t* counts_dev, int32_t* tied_dev,
                                          void* hip_stream) {
    SegDistinctCall c{"rsv_distinct_segmented_ordered", nullptr, "tied_dev", tied_dev};
    if (segdistinct_stateless_done(c, k, key_width, hash_kind, num_streams, offsets_dev && out_keys_dev && counts_dev,
                                   hashes_dev, keys_dev, out_keys_dev))
        return c.st;
    RSV_HIP_TRY(launch_segdistinct_ordered(keys_dev, key_width, hashes_dev, offsets_dev, num_streams, (uint32_t)k, c.hk,
                                           seed + stream_base, out_keys_dev, out_hashes_dev, counts_dev, tied_dev,
                                           (hipStream_t)hip_stream));
    return RSV_OK;
}

rsv_status rsv_distinct_segmented_rows(const void* rows_dev, const int64_t* hashes_dev, const int64_t* offsets_dev,
                                       int64_t num_streams, int32_t key_width, int32_t k, int32_t hash_kind,
                                       uint64_t seed, uint64_t stream_base, void* out_rows_dev,
                                       int64_t* out_hashes_dev, int64_t* counts_dev, void* hip_stream) {
    SegDistinctCall c{"rsv_distinct_segmented_rows", "rsv_distinct_segmented"};
    if (segdistinct_stateless_done(c, k, key_width, hash_kind, num_streams, offsets_dev && out_rows_dev && counts_dev,
                                   hashes_dev, rows_dev, out_rows_dev))
        return c.st;
    RSV_HIP_TRY(launch_segdistinct_rows(rows_dev, key_width, hashes_dev, offsets_dev, num_streams, (uint32_t)k,
                                        seed + stream_base, out_rows_dev, out_hashes_dev, counts_dev,
                                        (hipStream_t)hip_stream));
    return RSV_OK;
}

rsv_status rsv_distinct_segmented_rows_ordered(const void* rows_dev, const int64_t* hashes_dev, const int64_t* offsets_dev,
                                               int64_t num_streams, int32_t key_width, int32_t k, int32_t hash_kind,
                                               uint64_t seed, uint64_t stream_base, void* out_rows_dev,
                                               int64_t* out_hashes_dev, int64_t* counts_dev, int32_t* tied_dev,
                                               void* hip_stream) {
    SegDistinctCall c{"rsv_distinct_segmented_rows_ordered", "rsv_distinct_segmented_ordered", "tied_dev", tied_dev};
    if (segdistinct_stateless_done(c, k, key_width, hash_kind, num_streams, offsets_dev && out_rows_dev && counts_dev,
                                   hashes_dev, rows_dev, out_rows_dev))
        return c.st;
    RSV_HIP_TRY(launch_segdistinct_rows_ordered(rows_dev, key_width, hashes_dev, offsets_dev, num_streams, (uint32_t)k,
                                                seed + stream_base, out_rows_dev, out_hashes_dev, counts_dev, tied_dev,
                                                (hipStream_t)hip_stream));
    return RSV_OK;
}

rsv_status rsv_distinct_segmented_update(const void* keys_dev, const int64_t* hashes_dev, const int64_t* offsets_dev,
                                         const int64_t* stream_ids_dev, int64_t num_segments, int64_t num_states,
                                         int32_t key_width, int32_t k, int32_t hash_kind, uint64_t seed,
                                         uint64_t stream_base, void* state_keys_dev, int64_t* state_hashes_dev,
                                         int64_t* state_counts_dev, void* hip_stream) {
    SegDistinctCall c{"rsv_distinct_segmented_update"};
    if (segdistinct_update_done(c, k, key_width, hash_kind, num_segments, num_states, stream_ids_dev,
                                offsets_dev && state_keys_dev && state_hashes_dev && state_counts_dev, hashes_dev,
                                keys_dev, state_keys_dev))
        return c.st;
    RSV_HIP_TRY(launch_segdistinct_update(keys_dev, key_width, hashes_dev, offsets_dev, stream_ids_dev, num_segments,
                                          num_states, (uint32_t)k, c.hk, seed + stream_base, state_keys_dev,
                                          state_hashes_dev, state_counts_dev, (hipStream_t)hip_stream));
    return RSV_OK;
}

rsv_status rsv_distinct_segmented_ordered_update(const void* keys_dev, const int64_t* hashes_dev,
                                                 const int64_t* offsets_dev, const int64_t* stream_ids_dev,
                                                 int64_t num_segments, int64_t num_states, int32_t key_width,
                                                 int32_t k, int32_t hash_kind, uint64_t seed, uint64_t stream_base,
                                                 void* state_keys_dev, int64_t* state_hashes_dev,
                                                 int64_t* state_counts_dev, void* hip_stream) {
    // state_hashes_dev by name, behind the other buffers
    SegDistinctCall c{"rsv_distinct_segmented_ordered_update", nullptr,
                            "state_hashes_dev: the heap is ordered by them", state_hashes_dev};
    if (segdistinct_update_done(c, k, key_width, hash_kind, num_segments, num_states, stream_ids_dev,
                                offsets_dev && state_keys_dev && state_counts_dev, hashes_dev, keys_dev, state_keys_dev))
        return c.st;
    RSV_HIP_TRY(launch_segdistinct_ordered_update(keys_dev, key_width, hashes_dev, offsets_dev, stream_ids_dev,
                                                  num_segments, num_states, (uint32_t)k, c.hk, seed + stream_base,
                                                  state_keys_dev, state_hashes_dev, state_counts_dev,
                                                  (hipStream_t)hip_stream));
    return RSV_OK;
}

rsv_status rsv_distinct_segmented_merge(const void* part_keys_dev, const int64_t* part_hashes_dev,
                                        const int64_t* part_counts_dev, int32_t parts, int64_t num_states,
                                        int32_t key_width, int32_t k, void* state_keys_dev, int64_t* state_hashes_dev,
                                        int64_t* state_counts_dev, void* hip_stream) {
    SegDistinctCall c{"rsv_distinct_segmented_merge"};
    if (segdistinct_merge_done(c, k, key_width, parts, num_states,
                               part_keys_dev && part_hashes_dev && part_counts_dev && state_keys_dev &&
                                   state_hashes_dev && state_counts_dev,
                               part_hashes_dev, part_keys_dev, state_keys_dev))
        return c.st;
    RSV_HIP_TRY(launch_segdistinct_merge(part_keys_dev, key_width, part_hashes_dev, part_counts_dev, parts, num_states,
                                         (uint32_t)k, state_keys_dev, state_hashes_dev, state_counts_dev,
                                         (hipStream_t)hip_stream));
    return RSV_OK;
}

rsv_status rsv_distinct_segmented_rows_update(const void* rows_dev, const int64_t* hashes_dev,
                                              const int64_t* offsets_dev, const int64_t* stream_ids_dev,
                                              int64_t num_segments, int64_t num_states, int32_t key_width, int32_t k,
                                              int32_t hash_kind, uint64_t seed, uint64_t stream_base,
                                              void* state_rows_dev, int64_t* state_hashes_dev,
                                              int64_t* state_counts_dev, void* hip_stream) {
    SegDistinctCall c{"rsv_distinct_segmented_rows_update", "rsv_distinct_segmented_update"};
    if (segdistinct_update_done(c, k, key_width, hash_kind, num_segments, num_states, stream_ids_dev,
                                offsets_dev && state_rows_dev && state_hashes_dev && state_counts_dev, hashes_dev,
                                rows_dev, state_rows_dev))
        return c.st;
    RSV_HIP_TRY(launch_segdistinct_rows_update(rows_dev, key_width, hashes_dev, offsets_dev, stream_ids_dev, num_segments,
                                               num_states, (uint32_t)k, seed + stream_base, state_rows_dev,
                                               state_hashes_dev, state_counts_dev, (hipStream_t)hip_stream));
    return RSV_OK;
}

rsv_status rsv_distinct_segmented_rows_ordered_update(const void* rows_dev, const int64_t* hashes_dev,
                                                      const int64_t* offsets_dev, const int64_t* stream_ids_dev,
                                                      int64_t num_segments, int64_t num_states, int32_t key_width,
                                                      int32_t k, int32_t hash_kind, uint64_t seed, uint64_t stream_base,
                                                      void* state_rows_dev, int64_t* state_hashes_dev,
                                                      int32_t* state_slots_dev, int64_t* state_counts_dev,
                                                      void* hip_stream) {
    // state_slots_dev by name, behind the other buffers
    SegDistinctCall c{"rsv_distinct_segmented_rows_ordered_update", "rsv_distinct_segmented_ordered_update",
                            "state_slots_dev: the heap's entries find their rows by them", state_slots_dev};
    if (segdistinct_update_done(c, k, key_width, hash_kind, num_segments, num_states, stream_ids_dev,
                                offsets_dev && state_rows_dev && state_hashes_dev && state_counts_dev, hashes_dev,
                                rows_dev, state_rows_dev))
        return c.st;
    RSV_HIP_TRY(launch_segdistinct_rows_ordered_update(rows_dev, key_width, hashes_dev, offsets_dev, stream_ids_dev,
                                                       num_segments, num_states, (uint32_t)k, seed + stream_base,
                                                       state_rows_dev, state_hashes_dev, state_slots_dev,
                                                       state_counts_dev, (hipStream_t)hip_stream));
    return RSV_OK;
}

rsv_status rsv_distinct_segmented_rows_merge(const void* part_rows_dev, const int64_t* part_hashes_dev,
                                             const int64_t* part_counts_dev, int32_t parts, int64_t num_states,
                                             int32_t key_width, int32_t k, void* state_rows_dev,
                                             int64_t* state_hashes_dev, int64_t* state_counts_dev, void* hip_stream) {
    SegDistinctCall c{"rsv_distinct_segmented_rows_merge", "rsv_distinct_segmented_merge"};
    if (segdistinct_merge_done(c, k, key_width, parts, num_states,
                               part_rows_dev && part_hashes_dev && part_counts_dev && state_rows_dev &&
                                   state_hashes_dev && state_counts_dev,
                               part_hashes_dev, part_rows_dev, state_rows_dev))
        return c.st;
    RSV_HIP_TRY(launch_segdistinct_rows_merge(part_rows_dev, key_width, part_hashes_dev, part_counts_dev, parts,
                                              num_states, (uint32_t)k, state_rows_dev, state_hashes_dev,
                                              state_counts_dev, (hipStream_t)hip_stream));
    return RSV_OK;
}

// The eleventh: candidates by hash for object keys.  No key width and no hash kind; K5's checks in K5's order
// otherwise (hashes_dev is not among the required buffers: a launch whose segments are all empty has none).
rsv_status rsv_distinct_segmented_candidates(const int64_t* hashes_dev, const int64_t* offsets_dev,
                                             const int64_t* stream_ids_dev, int64_t num_segments, int64_t num_states,
                                             int32_t k, uint64_t seed, uint64_t stream_base, int64_t* shadow_hashes_dev,
                                             int64_t* shadow_counts_dev, const int64_t* set_sizes_dev,
                                             const int64_t* max_hashes_dev, int64_t* out_pos_dev, int64_t* out_hashes_dev,
                                             int64_t cap, int64_t* out_counts_dev, void* hip_stream) {
    const SegDistinctCall c{"rsv_distinct_segmented_candidates"};
    if (rsv_status st = check_segdistinct_shape(c, k, 8)) return st;
    if (num_segments < 0 || num_states < 0) return fail(RSV_E_ILLEGAL_ARGUMENT, "negative segment or state count");
    if (cap < 1) return fail(RSV_E_ILLEGAL_ARGUMENT, "cap must be at least 1");
    if (!stream_ids_dev && num_segments > num_states)
        return fail(RSV_E_ILLEGAL_ARGUMENT, "more segments than state rows without stream_ids_dev");
    if (num_segments == 0) return RSV_OK;
    if (!offsets_dev || !out_pos_dev || !out_hashes_dev || !out_counts_dev ||
        (num_states > 0 && (!shadow_hashes_dev || !shadow_counts_dev)))
        return fail(RSV_E_NULL_POINTER, "NULL buffer");
    if (!set_sizes_dev != !max_hashes_dev)
        return fail(RSV_E_ILLEGAL_ARGUMENT, std::string(c.fn) + " takes set_sizes_dev and max_hashes_dev together or neither");
    RSV_HIP_TRY(launch_segdistinct_candidates(hashes_dev, offsets_dev, stream_ids_dev, num_segments, num_states,
                                              (uint32_t)k, seed + stream_base, shadow_hashes_dev, shadow_counts_dev,
                                              set_sizes_dev, max_hashes_dev, out_pos_dev, out_hashes_dev, cap,
                                              out_counts_dev, (hipStream_t)hip_stream));
    return RSV_OK;
}

rsv_status rsv_replay_events(const void* keys_dev, int64_t n, int32_t key_width, int64_t base_index,
                             const int64_t* ev_pos_dev, const int32_t* ev_slot_dev, int64_t n_events, int32_t k,
                             void* reservoir_dev, void* hip_stream) {
    if (k <= 0 || k > kMaxSize) return fail(RSV_E_ILLEGAL_ARGUMENT, "k out of range");
    if (key_width != 4 && key_width != 8) return fail(RSV_E_ILLEGAL_ARGUMENT, "key_width must be 4 or 8");
    if (n < 0 || n_events < 0 || base_index < 0) return fail(RSV_E_ILLEGAL_ARGUMENT, "negative size");
    if (!reservoir_dev || (n && !keys_dev) || (n_events && (!ev_pos_dev || !ev_slot_dev)))
        return fail(RSV_E_NULL_POINTER, "NULL buffer");
    hipStream_t st = (hipStream_t)hip_stream;
    unsigned long long* win = nullptr;
    RSV_HIP_TRY(hipMallocAsync((void**)&win, (size_t)k * 8, st));
    hipError_t e = hipMemsetAsync(win, 0, (size_t)k * 8, st);
    if (e == hipSuccess) e = launch_replay_events(ev_pos_dev, ev_slot_dev, n_events, (uint32_t)k, win, st);
    if (e == hipSuccess) e = launch_resolve(SlotBlock{win, nullptr, reservoir_dev, (uint32_t)k, key_width}, Batch{keys_dev, base_index, n, false},
                           Publication{}, st);
    hipError_t e2 = hipFreeAsync(win, st);
    RSV_HIP_TRY(e);
    RSV_HIP_TRY(e2);
    return RSV_OK;
}

rsv_status rsv_export_draws(uint64_t seed, uint64_t stream_id, uint64_t i0, int64_t n, uint64_t* j_dev,
                            void* hip_stream) {
    if (n < 0) return fail(RSV_E_ILLEGAL_ARGUMENT, "negative n");
    if (n && !j_dev) return fail(RSV_E_NULL_POINTER, "j_dev is NULL");
    const DrawParams dp{seed, stream_id};
    RSV_HIP_TRY(launch_export_draws(dp, i0, n, j_dev, (hipStream_t)hip_stream));
    return RSV_OK;
}

}  // extern "C"
