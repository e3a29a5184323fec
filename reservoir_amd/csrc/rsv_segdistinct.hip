// rsv_segdistinct.hip -- K5: S independent Sampler.distinct streams per launch.  No reference counterpart; = S
// separate RandomValues instances (Sampler.scala:383-412), each seeded with java.util.Random(seed + stream_base + s).
// The ten rsv_distinct_segmented* entry points are two key kinds (4-/8-byte keys; byte-key rows of W = 16..256 bytes,
// W8 = W / 8 little-endian 64-bit words) times
//   set order (RSV_DISTINCT_SET)    stream s keeps the min(k, D_s) distinct keys with the smallest (scrambled hash,
//                                   key), written ascending: stateless, _update, _merge.
//   ordered (RSV_DISTINCT_ORDERED)  the reference's own set where the boundary hash bucket is oversubscribed, its
//                                   members chosen by arrival order and the heap's tie behaviour: stateless, _update
//                                   (DESIGN.md 5c.3 - 5c.6).  Not provided: merge (two heaps over parts of a stream
//                                   do not determine the heap over the whole), k > 4096.
// An eleventh, rsv_distinct_segmented_candidates, is the third key kind, any B: the kernel reads hashes only and
// returns candidate positions (segcand_kernel, behind the resumed set frames; the forms and merge_set are shared).
// The pieces, in the file's order:
//
// Entry.  16 bytes (h, second word) in LDS, for every key kind and width, so every form keeps its LDS budget.
//
// Source policies (Keys, Rows; Tied<> over either): what the second word is -- the one thing the set loop, the merge
// and the heap walk take as a parameter.  Keys: the key itself.  Rows: a ref to the row; order and equality go by h
// first, only two entries with equal h read their rows from global memory, word by word as unsigned values, and equal
// rows are one element whatever their refs.  The sort's pad is (INT64_MAX, INT64_MAX), over rows (INT64_MAX, -1): the
// ref -1 is tested before any row is addressed, is above every row and equal to itself.  T's row sits in LDS (s_trow,
// rewritten by the merge that sets T), so admission reads a row only on the lanes with h == T.h.  Row hashes are
// precomputed (8 bytes per element; the rows are read on ties and for the output only) or UUID.hashCode of 16-byte
// rows (one 16-byte load per element, two 8-byte loads when rows_dev sits at 8 mod 16).  Resumed, a ref names one of
// two row sources, the launch's input or a slot of the row's own state block (RowSrc<true>; at() clamps the slot).
//
// Set loop (take_piece, merge_set).  One TEAM of NT threads per stream, streams taken grid-stride.  The team holds P
// entries: the current set [0, m) ascending, and behind it the candidates admitted since the last merge.  Per
// iteration it loads NT x kU elements (coalesced, kU in flight per lane) and takes them in kU steps of NT:
// h = scramble(r0, r1, hash(key)), admitted when (h, key) <= T, where T is the pad while the set holds fewer than k
// entries, else its k-th entry.  `<=`, not `h < T`: a distinct key with the boundary hash and a smaller key must get
// in; repeats of members pass too and fall out as adjacent equals in the merge.  Admitted entries are appended at one
// LDS atomicAdd per wave (ballot + prefix count); their order in the buffer does not matter, because the merge sorts
// by the whole entry and equal entries are the same element.  The count is re-read by every wave between two barriers
// after each step, so the decision to merge is uniform.  A merge runs when the buffer cannot take another full step
// (P >= k + NT, so one always fits afterwards), when 4k entries wait and no threshold is known yet, and at the end of
// the stream: bitonic sort of the first pow2ceil(m + c) entries (padded -- a real entry equal to the pad sorts among
// the pads and is still inside the first m + c), drop of adjacent equals with an in-place block scan, keep the first
// k, reload T.
// Forms (DESIGN.md "Segmented distinct"; with_form_of below is the only place that names them):
//   k <= 64    NT = 64 (one wave per stream), P = 256: 4 KB of LDS, 32 streams resident per CU
//   k <= 256   NT = 64, P = 512: 8 KB, 19 streams per CU
//   k <= 1024  NT = 256, P = 2048: 32 KB, 4 workgroups per CU
//   k <= 4096  NT = 1024, P = 8192: 128 KB, one workgroup per CU
// The smaller P for k <= 64 is deliberate: a buffer that fills sooner gives a fresher T, so fewer entries are
// admitted, and a sort of 256 costs 0.4 of a sort of 512.
//
// Heap walk (heap_admit, replay_walk): RandomValues itself, one wave per stream, for the ordered entry points.
//
// Four kernel frames:
//   stateless set     segdistinct_kernel / segrows_kernel<.., TIED>: open_stream, take_piece, the row's epilogue
//                     (finish_row; gather_rows).  TIED also notes the streams whose boundary bucket is oversubscribed.
//   resumed set       segstate_kernel / segrowstate_kernel<.., MERGE>: for_resumed_items, the row into se, take_piece
//                     over the segment or the parts, the row back in place.
//   replay            segdistinct_replay_kernel / segrows_replay_kernel: for_tied_streams, replay_walk from an empty
//                     heap, sort, the row over what kernel 1 wrote.
//   resumed heap      segdistinct_heap_kernel / segrows_heap_kernel: for_resumed_items, the row into se as it lies,
//                     replay_walk, the row back as it lies.
//
// State layouts (the caller's memory; nothing read from it or from the ids indexes memory unclamped: a count is clamped
// into [0, k], a slot below k, an id outside [0, num_states) skips its segment -- clamp_count, for_resumed_items,
// RowSrc<true>::at, slot_of):
//   set, keys   per row r counts[r] entries (h, key) ascending, in the layout the stateless launch writes.  Bottom-k by
//               (h, key) over distinct keys is a function of the key set alone, so bottomk(A u B) =
//               bottomk(bottomk(A) u B): a row resumed from its stored set and fed the next piece ends where one
//               stateless launch over the concatenation ends.  UPDATE: segment b hashed and scrambled with the row's
//               (r0, r1), row r = stream_ids[b] (or b).  MERGE: for every part p the first clamp(part_counts[p][r])
//               slots of its row r, h taken as stored.
//   set, rows   rows[num_states][k][W8], hashes and counts as the stateless launch writes them.
//   heap, keys  counts[r] entries (h, key) in the queue's array order: k entries kept sorted cannot carry the heap's
//               history, k entries in array order are the heap.
//   heap, rows  the array holds (hash, slot); the rows stay in their slots of the row's block.
#include <algorithm>
#include <type_traits>

#include "../../include/reservoir_hip.h"
#include "rsv_device.h"
#include "rsv_internal.h"

namespace rsv {

namespace {

constexpr int kU = 4;  // elements per lane and iteration
constexpr int64_t kMaxI64 = INT64_MAX;

// java.util.Random(seed): the first two nextLong() (RandomValues r0, r1, Sampler.scala:385-388)
__device__ __forceinline__ void java_r0r1(uint64_t seed, int64_t& r0, int64_t& r1) {
    constexpr uint64_t kMul = 0x5DEECE66DULL, kMask = (1ULL << 48) - 1;
    uint64_t st = (seed ^ kMul) & kMask;
    int64_t w[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        st = (st * kMul + 0xBULL) & kMask;
        w[i] = (int64_t)(int32_t)(uint32_t)(st >> 16);
    }
    r0 = (int64_t)(((uint64_t)w[0] << 32) + (uint64_t)w[1]);
    r1 = (int64_t)(((uint64_t)w[2] << 32) + (uint64_t)w[3]);
}

// one LDS entry: 16 bytes, moved with one ds_read_b128 / ds_write_b128
struct alignas(16) Ent {
    int64_t h, key;
};

__device__ __forceinline__ bool ent_less(const Ent& a, const Ent& b) { return a.h < b.h || (a.h == b.h && a.key < b.key); }
__device__ __forceinline__ bool ent_eq(const Ent& a, const Ent& b) { return a.h == b.h && a.key == b.key; }

// the team's registers across the pieces of one row (uniform over the team)
struct Team {
    uint32_t m;      // set size
    uint32_t n_tot;  // set + waiting candidates (= s_cnt, read between two barriers)
    int64_t Th, Tk;  // admission threshold: the k-th entry, or the pad below k entries
    bool dirty;      // something was appended since the team started on the row
};

// lane l's value as a scalar (l uniform): two v_readlane, no LDS round trip
__device__ __forceinline__ int64_t read_lane(int64_t v, int l) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, l);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)((uint64_t)v >> 32), l);
    return (int64_t)(((uint64_t)hi << 32) | lo);
}

// ---- Source policies: what an entry's second word is ----
// For the merge (pad, out_of_order, same), for the element loop (load, h_of, admits, set_T, refuse, trimmed; above_T
// for Tied below) and for the heap walk (second_of, scan_word, look).  K5's own: the key itself, sign-extended.
struct KeyOrd {
    static __device__ __forceinline__ Ent pad() { return Ent{kMaxI64, kMaxI64}; }
    __device__ __forceinline__ bool out_of_order(const Ent& a, const Ent& b, bool asc) const {
        return ent_less(b, a) == asc && !ent_eq(a, b);
    }
    __device__ __forceinline__ bool same(const Ent& a, const Ent& b) const { return ent_eq(a, b); }
};

// SCRAMBLE: h = scramble(r0, r1, hash(key)); otherwise h = hashes[i] as stored.
template <typename KeyT, bool SCRAMBLE>
struct Keys : KeyOrd {
    const KeyT* __restrict__ keys;
    const int64_t* __restrict__ hashes;
    int hash_kind;
    int64_t r0, r1;
    __device__ __forceinline__ void load(int64_t i, int64_t& key, int64_t& hv) const {
        key = (int64_t)keys[i];
        if (!SCRAMBLE || hash_kind == kHashPrecomputed) hv = hashes[i];
    }
    __device__ __forceinline__ int64_t h_of(int64_t key, int64_t hv) const {
        if constexpr (SCRAMBLE) {
            int64_t hashed;
            if (hash_kind == kHashPrecomputed)
                hashed = hv;
            else if (hash_kind == kHashJavaLong)
                hashed = hash_of<int64_t, kHashJavaLong>(key);
            else if (hash_kind == kHashJavaInt)
                hashed = hash_of<int64_t, kHashJavaInt>(key);
            else
                hashed = key;  // identity: the sign-extended key
            return scramble(r0, r1, hashed);
        } else {
            return hv;
        }
    }
    __device__ __forceinline__ bool admits(int64_t h, int64_t key, const Team& t) const {
        return h < t.Th || (h == t.Th && key <= t.Tk);
    }
    __device__ __forceinline__ void set_T(const Ent* se, uint32_t k, Team& t) const {
        t.Th = se[k - 1].h;
        t.Tk = se[k - 1].key;
    }
    // what the loop refuses is of no interest here (Tied notes it)
    static __device__ __forceinline__ void refuse(int64_t, const Team&) {}
    template <int NT>
    static __device__ __forceinline__ void trimmed(const Ent*, uint32_t, uint32_t, const Team&) {}
    // e.h == T.h: is e above T
    __device__ __forceinline__ bool above_T(const Ent& e, const Team& t) const { return e.key > t.Tk; }
    // The heap walk's side.  The candidate of lane l: its key.  elements.contains scans the heap's keys.
    static __device__ __forceinline__ int64_t second_of(int64_t key, int64_t, int l) { return read_lane(key, l); }
    static __device__ __forceinline__ int64_t scan_word(const Ent* e) { return e->key; }
    static __device__ __forceinline__ bool look(bool found, int64_t word, const Ent*, const Ent& c) { return found | (word == c.key); }
};

// Byte keys: where an entry's second word (its ref) finds its row of W8 words.  One source, the stateless
// launch: the ref is the row's index into `rows`.  Two sources, the resumed launches: a ref below 2^62 is
// an index into the launch's input (rows_dev, or the parts), a ref with kStateRef set is slot
// ref & (kStateRef - 1) of the block `srow` of the state row the team works on, clamped below k before it
// addresses anything.  Both kinds are >= 0, so the pad's -1 stays what it is.  at() is the only place
// that turns a ref into an address.
constexpr int64_t kStateRef = 1LL << 62;

template <bool TWO>
struct RowSrc;
template <>
struct RowSrc<false> {
    const uint64_t* __restrict__ rows;
    uint32_t W8;
    __device__ __forceinline__ const uint64_t* at(int64_t ref) const { return rows + ref * (int64_t)W8; }
};
template <>
struct RowSrc<true> {
    const uint64_t* rows;  // not __restrict__: the state is read and written through other pointers
    uint32_t W8;
    const uint64_t* srow;
    uint32_t k;
    __device__ __forceinline__ const uint64_t* at(int64_t ref) const {
        if (ref & kStateRef) {
            const uint64_t j = (uint64_t)(ref & (kStateRef - 1));
            return srow + (j < k ? (uint32_t)j : k - 1) * W8;
        }
        return rows + ref * (int64_t)W8;
    }
};

// What a heap entry's second word is in the two ordered kernels over rows.  Stateless (STATE = false): the row's
// index into rows.  Resumed (STATE = true): every entry also carries the storage slot of its row in the state
// block, so that lane 0's sift moves it along in the same 16 bytes: a state entry is
// kStateRef | slot, an entry admitted from the input is slot << kSlotShift | row index (slot < 4096, indices far
// below 2^48).  row_of and slot_of are the only places that take such a word apart; RowSrc<true>::at clamps the
// slot of a state entry below k before it addresses anything.
constexpr int kSlotShift = 48;
constexpr int64_t kRowIndexMask = (1LL << kSlotShift) - 1;

template <bool STATE>
__device__ __forceinline__ const uint64_t* row_of(const RowSrc<STATE>& src, int64_t ref) {
    if constexpr (STATE)
        return src.at((ref & kStateRef) ? ref : (ref & kRowIndexMask));
    else
        return src.at(ref);
}
// (below k whatever the entry holds: a state entry's slot was clamped when it entered LDS, an input entry's is a
// heap size below k or the slot of a root)
__device__ __forceinline__ uint32_t slot_of(int64_t ref, uint32_t k) {
    const uint64_t j = (ref & kStateRef) ? (uint64_t)(ref & (kStateRef - 1)) : (uint64_t)ref >> kSlotShift;
    return j < k ? (uint32_t)j : k - 1;
}

// -1 is the pad's ref.
template <bool TWO>
struct RowOrd : RowSrc<TWO> {
    static __device__ __forceinline__ Ent pad() { return Ent{kMaxI64, -1}; }
    // <0, 0, >0.  Equal refs (two pads among them) and the pad are settled before a row is addressed.
    // Two refs to equal rows, whichever their sources, compare equal: they are one element.
    __device__ __forceinline__ int cmp(const Ent& a, const Ent& b) const {
        if (a.h != b.h) return a.h < b.h ? -1 : 1;
        if (a.key == b.key) return 0;
        if (a.key < 0) return 1;
        if (b.key < 0) return -1;
        const uint64_t* const ra = this->at(a.key);
        const uint64_t* const rb = this->at(b.key);
        for (uint32_t w = 0; w < this->W8; ++w) {
            const uint64_t x = ra[w], y = rb[w];
            if (x != y) return x < y ? -1 : 1;
        }
        return 0;
    }
    __device__ __forceinline__ bool out_of_order(const Ent& a, const Ent& b, bool asc) const {
        const int c = cmp(a, b);
        return c != 0 && (c > 0) == asc;
    }
    __device__ __forceinline__ bool same(const Ent& a, const Ent& b) const { return cmp(a, b) == 0; }
};

// The element loop's side: element i is row i of the input (`rows`), whichever sources the refs have.
// SCRAMBLE as for Keys: otherwise h = hashes[i] as stored (the parts of a merge).
template <bool TWO, bool SCRAMBLE>
struct Rows : RowOrd<TWO> {
    const int64_t* __restrict__ hashes;  // null: UUID.hashCode of the 16-byte row
    bool vec16;                          // rows is 16-byte aligned: a UUID is one 16-byte load
    int64_t r0, r1;
    uint64_t* s_trow;  // LDS: T's row while t.Tk >= 0
    __device__ __forceinline__ void load(int64_t i, int64_t& key, int64_t& hv) const {
        key = i;
        if (hashes) {
            hv = hashes[i];
        } else if (vec16) {
            const ulonglong2 v = *reinterpret_cast<const ulonglong2*>(this->rows + 2 * i);
            hv = uuid_hash_code(v.x, v.y);
        } else {
            hv = uuid_hash_code(this->rows[2 * i], this->rows[2 * i + 1]);
        }
    }
    __device__ __forceinline__ int64_t h_of(int64_t, int64_t hv) const {
        if constexpr (SCRAMBLE)
            return scramble(r0, r1, hv);
        else
            return hv;
    }
    // (h, row i) <= T; below k entries T is the pad, above every row
    __device__ __forceinline__ bool admits(int64_t h, int64_t i, const Team& t) const {
        if (h != t.Th) return h < t.Th;
        if (t.Tk < 0 || i == t.Tk) return true;
        const uint64_t* const r = this->at(i);
        for (uint32_t w = 0; w < this->W8; ++w) {
            const uint64_t x = r[w], y = s_trow[w];
            if (x != y) return x < y;
        }
        return true;
    }
    // between the merge and the two barriers that precede the next admission test
    __device__ __forceinline__ void set_T(const Ent* se, uint32_t k, Team& t) const {
        t.Th = se[k - 1].h;
        t.Tk = se[k - 1].key;
        if (threadIdx.x < this->W8) s_trow[threadIdx.x] = this->at(t.Tk)[threadIdx.x];
    }
    static __device__ __forceinline__ void refuse(int64_t, const Team&) {}
    template <int NT>
    static __device__ __forceinline__ void trimmed(const Ent*, uint32_t, uint32_t, const Team&) {}
    // e.h == T.h: is e's row above T's (not "differs": a repeat of a member may share T.h with a row below T's).
    // Equal refs and the pads are settled before any row is addressed.  set_T writes s_trow from the threads below
    // W8 and no barrier stands between it and trimmed, so T's row is read where set_T read it: at(T.Tk) in global
    // memory.
    __device__ __forceinline__ bool above_T(const Ent& e, const Team& t) const {
        if (e.key == t.Tk || e.key < 0 || t.Tk < 0) return false;
        return this->cmp(e, Ent{e.h, t.Tk}) > 0;
    }
    // The heap walk's side (the refs are the heap's: row_of).  The candidate of lane l: the index of its row, which
    // is its element's.  elements.contains: equal rows carry equal hashes (the caller's contract), so the scan goes
    // over the heap's h and only an entry with the candidate's h has its ref read and its row compared.
    static __device__ __forceinline__ int64_t second_of(int64_t, int64_t i0, int l) { return i0 + l; }
    static __device__ __forceinline__ int64_t scan_word(const Ent* e) { return e->h; }
    // The replay (one source) branches around the row compare: the scan's straight path is then the eight compares
    // alone, which is what a heap of thousands of entries runs.  The resumed kernel (two sources) has the compare in
    // line (`&&`): there the other form measured above the parent's time and this one below it ("One
    // heap, one walk"), as the branch form of the replay did against `&&`.  The two are one test.
    __device__ __forceinline__ bool look(bool found, int64_t word, const Ent* e, const Ent& c) const {
        if constexpr (TWO) return found | (word == c.h && same_row(e->key, c.key));
        if (word == c.h) found |= same_row(e->key, c.key);
        return found;
    }
    // equality of a heap entry's row and row c of the input (W8 >= 2): the first two words of both in flight
    // together, so a UUID costs one round trip, not one per word
    __device__ __forceinline__ bool same_row(int64_t ref, int64_t c) const {
        const uint64_t* const ra = row_of<TWO>(*this, ref);
        const uint64_t* const rb = this->rows + c * (int64_t)this->W8;
        if (ra == rb) return true;
        const uint64_t a0 = ra[0], a1 = ra[1], b0 = rb[0], b1 = rb[1];
        if (a0 != b0 || a1 != b1) return false;
        for (uint32_t w = 2; w < this->W8; ++w)
            if (ra[w] != rb[w]) return false;
        return true;
    }
};

// A source that also notes, per lane, whether the team refused an element whose h is the current T.h: an element
// that fails `admits` ((h, second word) > T), or an entry a merge trims (the entries above the new T among se[k, n):
// the compaction writes below k only, so se[k, n) is what the sort left there, and an entry of distinct rank >= k
// sits at a sorted position >= k).  The note is dropped when a merge lowers T.h.  The comment at "Ordered" below
// says why (m == k && some lane holds a note) is `tied`, exactly.
template <typename Base>
struct Tied : Base {
    mutable bool at_T = false;
    __device__ __forceinline__ void refuse(int64_t h, const Team& t) const { at_T |= h == t.Th; }
    __device__ __forceinline__ void set_T(const Ent* se, uint32_t k, Team& t) const {
        const int64_t was = t.Th;
        Base::set_T(se, k, t);
        if (t.Th != was) at_T = false;
    }
    // behind set_T, and before the barrier that lets the appends go on
    template <int NT>
    __device__ __forceinline__ void trimmed(const Ent* se, uint32_t k, uint32_t n, const Team& t) const {
        for (uint32_t i = k + threadIdx.x; i < n; i += NT) {
            const Ent e = se[i];
            at_T |= e.h == t.Th && this->above_T(e, t);
        }
    }
};

// Sort + dedup + trim of the team's first n entries; returns the new set size min(k, distinct).
template <int NT, typename Ord>
__device__ __forceinline__ uint32_t merge_set(Ent* __restrict__ se, uint32_t n, uint32_t k, uint32_t* __restrict__ s_scan,
                                              const Ord& ord) {
    const uint32_t tid = threadIdx.x;
    if (n == 0) return 0;
    uint32_t sz2 = 2;
    while (sz2 < n) sz2 <<= 1;
    for (uint32_t i = n + tid; i < sz2; i += NT) se[i] = Ord::pad();
    __syncthreads();
    for (uint32_t sz = 2; sz <= sz2; sz <<= 1) {
        for (uint32_t j = sz >> 1; j > 0; j >>= 1) {
            for (uint32_t t = tid; t < (sz2 >> 1); t += NT) {
                const uint32_t l = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                const bool asc = (l & sz) == 0;
                const Ent a = se[l], b = se[l + j];
                if (ord.out_of_order(a, b, asc)) {
                    se[l] = b;
                    se[l + j] = a;
                }
            }
            __syncthreads();
        }
    }
    // in-place compaction of the first occurrences, NT entries per round.  An entry moves to a
    // position <= its own, and entry base - 1 is only ever overwritten by itself, so the next
    // round's look-behind reads what the sort left.
    constexpr uint32_t kWavesT = NT / 64;
    uint32_t run = 0;
    for (uint32_t base = 0; base < n && run < k; base += NT) {
        const uint32_t i = base + tid;
        Ent e{0, 0};
        bool first = false;
        if (i < n) {
            e = se[i];
            first = i == 0 || !ord.same(e, se[i - 1]);
        }
        const uint64_t mask = __ballot(first);
        uint32_t pre = (uint32_t)__popcll(mask & ((1ULL << (tid & 63)) - 1));
        uint32_t total = (uint32_t)__popcll(mask);
        if constexpr (kWavesT > 1) {
            if ((tid & 63) == 0) s_scan[tid >> 6] = total;
            __syncthreads();  // also: every read of this round is done
            uint32_t before = 0;
            total = 0;
            for (uint32_t w = 0; w < kWavesT; ++w) {
                const uint32_t c = s_scan[w];
                if (w < (tid >> 6)) before += c;
                total += c;
            }
            pre += before;
        } else {
            __syncthreads();
        }
        const uint32_t pos = run + pre;
        if (first && pos < k) se[pos] = e;
        run += total;
        __syncthreads();
    }
    return run < k ? run : k;
}

// The element loop over one piece [lo, hi) of src's elements.
template <typename Src, int NT>
__device__ __forceinline__ void take_piece(Ent* __restrict__ se, uint32_t* __restrict__ s_cnt, uint32_t* __restrict__ s_scan,
                                           const Src& src, int64_t lo, int64_t hi, uint32_t k, uint32_t P, Team& t) {
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
            if (i < hi) src.load(i, key[u], hv[u]);
        }
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            const int64_t i = base + (int64_t)u * NT + tid;
            if (base + (int64_t)u * NT >= hi) break;  // uniform: the tail chunk's empty steps
            if (t.n_tot + NT > P || (t.m < k && t.n_tot >= 4 * k)) {
                t.m = merge_set<NT>(se, t.n_tot, k, s_scan, src);
                if (t.m == k) {
                    src.set_T(se, k, t);
                    src.template trimmed<NT>(se, k, t.n_tot, t);
                }
                __syncthreads();  // T is read before the appends below overwrite anything
                if (tid == 0) *s_cnt = t.m;
                t.n_tot = t.m;
                __syncthreads();
            }
            const int64_t h = src.h_of(key[u], hv[u]);
            const bool pass = i < hi && src.admits(h, key[u], t);
            if (i < hi && !pass) src.refuse(h, t);
            const uint64_t mask = __ballot(pass);
            if (mask) {
                const uint32_t lead = (uint32_t)(__ffsll((long long)mask) - 1);  // the wave's first admitting lane
                uint32_t b = 0;
                if ((tid & 63) == lead) b = atomicAdd(s_cnt, (uint32_t)__popcll(mask));
                b = (uint32_t)__shfl((int)b, (int)lead);
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

// The row's epilogue: the last merge (merge_set of nothing is 0, an empty row needs no case of its
// own), then se[0, m) and zeros up to k, then the count.  HASHES_OPTIONAL: hashes may be null (the
// stateless launch's out_hashes; a state always has them, and its kernels carry no test).
template <typename KeyT, int NT, bool HASHES_OPTIONAL>
__device__ __forceinline__ void finish_row(Ent* se, uint32_t* s_scan, Team& t, uint32_t k, int64_t row, KeyT* keys,
                                           int64_t* hashes, int64_t* counts) {
    const uint32_t tid = threadIdx.x;
    if (t.n_tot != t.m) t.m = merge_set<NT>(se, t.n_tot, k, s_scan, KeyOrd{});
    __syncthreads();
    const int64_t ob = row * (int64_t)k;
    for (uint32_t i = tid; i < k; i += NT) {
        const Ent e = i < t.m ? se[i] : Ent{0, 0};
        keys[ob + i] = (KeyT)e.key;
        if (!HASHES_OPTIONAL || hashes) hashes[ob + i] = e.h;
    }
    if (tid == 0) counts[row] = t.m;
}

// ---- The stateless frames: no prologue, row = stream index, every row is written ----
// A stream's start: its (r0, r1), an empty buffer behind the barrier that ends the previous stream's output
// reads, and the empty Team, whose T is the source's pad.
template <typename Ord>
__device__ __forceinline__ Team open_stream(uint64_t seed, uint32_t* s_cnt, int64_t& r0, int64_t& r1) {
    java_r0r1(seed, r0, r1);
    __syncthreads();  // the previous stream's output reads are done
    if (threadIdx.x == 0) *s_cnt = 0;
    __syncthreads();
    return Team{0, 0, Ord::pad().h, Ord::pad().key, false};
}

// TIED's end of a stream: the last merge, made here for what it trims, then tied = (m == k && some lane holds a note).
template <int NT, typename Src>
__device__ __forceinline__ void note_tied(Ent* se, uint32_t* s_scan, const Tied<Src>& src, uint32_t k, Team& t, int32_t* tied) {
    if (t.n_tot != t.m) {
        const uint32_t n = t.n_tot;
        t.m = merge_set<NT>(se, n, k, s_scan, src);
        if (t.m == k) {
            src.set_T(se, k, t);
            src.template trimmed<NT>(se, k, n, t);
        }
        t.n_tot = t.m;
    }
    const int noted = __syncthreads_or(src.at_T);
    if (threadIdx.x == 0) *tied = t.m == k && noted;
}

// TIED: the source is Tied<>, and tied[s] is written (kernel 1 of "Ordered" below); otherwise tied is not read.
template <typename KeyT, int NT, bool TIED>
__global__ __launch_bounds__(NT) void segdistinct_kernel(const KeyT* __restrict__ keys, const int64_t* __restrict__ hashes,
                                                         const int64_t* __restrict__ offsets, int64_t S, uint32_t k,
                                                         uint32_t P, int hash_kind, uint64_t seed0,
                                                         KeyT* __restrict__ out_keys, int64_t* __restrict__ out_hashes,
                                                         int64_t* __restrict__ counts, int32_t* __restrict__ tied) {
    extern __shared__ __align__(16) unsigned char seg_lds[];
    Ent* const se = (Ent*)seg_lds;
    __shared__ uint32_t s_cnt;
    __shared__ uint32_t s_scan[NT / 64 > 1 ? NT / 64 : 1];
    using Base = Keys<KeyT, true>;
    using Src = std::conditional_t<TIED, Tied<Base>, Base>;

    for (int64_t s = blockIdx.x; s < S; s += gridDim.x) {
        int64_t r0, r1;
        Team t = open_stream<Base>(seed0 + (uint64_t)s, &s_cnt, r0, r1);
        const Base base{{}, keys, hashes, hash_kind, r0, r1};
        const Src src{base};
        take_piece<Src, NT>(se, &s_cnt, s_scan, src, offsets[s], offsets[s + 1], k, P, t);
        if constexpr (TIED) note_tied<NT>(se, s_scan, src, k, t, tied + s);
        finish_row<KeyT, NT, true>(se, s_scan, t, k, s, out_keys, out_hashes, counts);
    }
}

// The rows of se[0, m) gathered into a row block, lanes over (entry, word) so that a wave's stores are consecutive
// words of the block, and their hashes (out_hashes may be null).  ZERO_FILL: the block's k entries are written, zeros
// behind m (the first kernel of a launch); otherwise [0, m) only (the replay, over what kernel 1 wrote).
template <int NT, bool ZERO_FILL>
__device__ __forceinline__ void gather_rows(const Ent* se, uint32_t m, uint32_t k, const uint64_t* __restrict__ rows,
                                            uint32_t W8, int64_t ob, uint64_t* __restrict__ out_rows,
                                            int64_t* __restrict__ out_hashes) {
    const uint32_t tid = threadIdx.x;
    const uint32_t top = ZERO_FILL ? k : m;
    for (uint32_t x = tid; x < top * W8; x += NT) {  // k * W8 <= 4096 * 32
        const uint32_t j = x / W8, w = x - j * W8;
        out_rows[ob * W8 + x] = !ZERO_FILL || j < m ? rows[se[j].key * (int64_t)W8 + w] : 0;
    }
    if (out_hashes)
        for (uint32_t i = tid; i < top; i += NT) out_hashes[ob + i] = !ZERO_FILL || i < m ? se[i].h : 0;
}

// Byte keys.  TIED as above.
template <int NT, bool TIED>
__global__ __launch_bounds__(NT) void segrows_kernel(const uint64_t* __restrict__ rows, const int64_t* __restrict__ hashes,
                                                     const int64_t* __restrict__ offsets, int64_t S, uint32_t W8,
                                                     uint32_t k, uint32_t P, uint64_t seed0,
                                                     uint64_t* __restrict__ out_rows, int64_t* __restrict__ out_hashes,
                                                     int64_t* __restrict__ counts, int32_t* __restrict__ tied) {
    extern __shared__ __align__(16) unsigned char seg_lds[];
    Ent* const se = (Ent*)seg_lds;
    __shared__ uint32_t s_cnt;
    __shared__ uint32_t s_scan[NT / 64 > 1 ? NT / 64 : 1];
    __shared__ uint64_t s_trow[32];  // kMaxRowWords
    const bool vec16 = ((uintptr_t)rows & 15) == 0;
    using Base = Rows<false, true>;
    using Src = std::conditional_t<TIED, Tied<Base>, Base>;

    for (int64_t s = blockIdx.x; s < S; s += gridDim.x) {
        int64_t r0, r1;
        Team t = open_stream<Base>(seed0 + (uint64_t)s, &s_cnt, r0, r1);
        const Base base{{{rows, W8}}, hashes, vec16, r0, r1, s_trow};
        const Src src{base};
        take_piece<Src, NT>(se, &s_cnt, s_scan, src, offsets[s], offsets[s + 1], k, P, t);
        if constexpr (TIED) note_tied<NT>(se, s_scan, src, k, t, tied + s);
        if (t.n_tot != t.m) t.m = merge_set<NT>(se, t.n_tot, k, s_scan, src);
        __syncthreads();
        gather_rows<NT, true>(se, t.m, k, rows, W8, s * (int64_t)k, out_rows, out_hashes);
        if (threadIdx.x == 0) counts[s] = t.m;
    }
}

// ---- Resumed: the item a team (or a wave) starts on ----
// A count read from memory, into [0, k]: no count indexes anything unclamped.
__device__ __forceinline__ uint32_t clamp_count(int64_t c, uint32_t k) {
    return c <= 0 ? 0u : (c >= (int64_t)k ? k : (uint32_t)c);
}

// The resumed kernels' frame: items grid-stride, and f(g) for every item b that is not skipped: g.r its state row,
// ids[b] (or b), [g.lo, g.hi) its input, g.c0 the row's stored count as it lies and g.m0 that count clamped.  Everything
// here is uniform over the team, and it decides the control flow of the kernels.  Nothing read from the ids or the
// state indexes memory unclamped: an id outside [0, num_states) skips the item before any row is addressed, and an empty
// segment is skipped too, which leaves its row as it is.  MERGE: item b is row b and its input is the parts' (nothing
// is skipped).
struct Resumed {
    int64_t r, lo, hi, c0;
    uint32_t m0;
};
template <bool MERGE, typename F>
__device__ __forceinline__ void for_resumed_items(int64_t items, const int64_t* __restrict__ ids,
                                                  const int64_t* __restrict__ offsets, int64_t num_states,
                                                  const int64_t* state_counts, uint32_t k, F f) {
    for (int64_t b = blockIdx.x; b < items; b += gridDim.x) {
        int64_t r = b, lo = 0, hi = 0;
        if constexpr (!MERGE) {
            if (ids) r = ids[b];
            if (r < 0 || r >= num_states) continue;
            lo = offsets[b];
            hi = offsets[b + 1];
            if (hi <= lo) continue;
        }
        const int64_t c0 = state_counts[r];
        f(Resumed{r, lo, hi, c0, clamp_count(c0, k)});
    }
}

// ---- The resumed set frames.  The element loop, the forms, the grid and the row's epilogue
// (finish_row) are the stateless kernel's own; around them
//   prologue   the row's m0 pairs into se[0, m0) (coalesced global loads, one 16-byte LDS write per entry);
//              s_cnt = n_tot = m = m0; T = se[k-1] when m0 == k, so a full row rejects from its first element on.
//   epilogue   in place, behind the barrier after the last LDS read of the team; a row with no input, and a row
//              whose input admitted nothing, writes nothing (a full row in steady state moves no state bytes out).
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

    for_resumed_items<MERGE>(teams, ids, offsets, num_states, state_counts, k, [&](const Resumed g) {
        const int64_t r = g.r, lo = g.lo, hi = g.hi, ob = r * (int64_t)k;
        const uint32_t m0 = g.m0;
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
                const int64_t n = clamp_count(part_counts[row], k);
                const int64_t pb = row * (int64_t)k;
                take_piece<Keys<KeyT, false>, NT>(se, &s_cnt, s_scan, Keys<KeyT, false>{{}, in_keys, in_hashes, hash_kind, 0, 0}, pb,
                                                  pb + n, k, P, t);
            }
        } else {
            int64_t r0, r1;
            java_r0r1(seed0 + (uint64_t)r, r0, r1);
            take_piece<Keys<KeyT, true>, NT>(se, &s_cnt, s_scan, Keys<KeyT, true>{{}, in_keys, in_hashes, hash_kind, r0, r1}, lo, hi,
                                             k, P, t);
        }
        if (!t.dirty) return;  // nothing admitted: the row stands as it is
        finish_row<KeyT, NT, false>(se, s_scan, t, k, r, state_keys, state_hashes, state_counts);
    });
}

// Byte keys, resumed: segstate_kernel for rows, MERGE as there (in = rows_dev / hashes / offsets, or the
// parts' rows [parts][num_states][k][W8] and hashes).  A state entry enters LDS as (h, kStateRef | slot),
// so nothing of the row block is read but what a tie on h or T asks for.
// The epilogue moves rows inside the block they are read from.  In a valid state the surviving state
// entries keep their order and inputs are only inserted between them, so the entry of slot j ends at a
// position p >= j and the word it moves goes from j * W8 + w up to p * W8 + w: a destination word x is
// read from a word <= x of the block, or from the input.  The words are therefore walked in chunks from
// the top down; per chunk every lane loads its kMoveWords sources, the team meets at a barrier, then it
// stores.  A chunk [lo, hi) reads below hi only and every earlier chunk wrote at or above hi, so
// nothing is read after it was overwritten.  An entry that stays at its slot moves no word and no hash,
// and a state that is not ascending or repeats a row breaks p >= j only: its set is unspecified, its
// addresses are the same.  Rows and hashes in [m, k) are zeroed where they are not the kernel's own
// zeros already: the row was empty (its slots are the caller's), its count was clamped, or the set
// shrank (an invalid state).
constexpr uint32_t kMoveWords = 4;

template <int NT, bool MERGE>
__global__ __launch_bounds__(NT) void segrowstate_kernel(const uint64_t* in_rows, const int64_t* in_hashes,
                                                         const int64_t* __restrict__ offsets,
                                                         const int64_t* __restrict__ ids, const int64_t* part_counts,
                                                         int64_t teams, int64_t num_states, int32_t parts, uint32_t W8,
                                                         uint32_t k, uint32_t P, uint64_t seed0, uint64_t* state_rows,
                                                         int64_t* state_hashes, int64_t* state_counts) {
    extern __shared__ __align__(16) unsigned char seg_lds[];
    Ent* const se = (Ent*)seg_lds;
    __shared__ uint32_t s_cnt;
    __shared__ uint32_t s_scan[NT / 64 > 1 ? NT / 64 : 1];
    __shared__ uint64_t s_trow[32];  // kMaxRowWords
    const uint32_t tid = threadIdx.x;
    const bool vec16 = ((uintptr_t)in_rows & 15) == 0;

    for_resumed_items<MERGE>(teams, ids, offsets, num_states, state_counts, k, [&](const Resumed g) {
        const int64_t r = g.r, lo = g.lo, hi = g.hi, c0 = g.c0, ob = r * (int64_t)k;
        const uint32_t m0 = g.m0;
        uint64_t* const srow = state_rows + ob * (int64_t)W8;
        __syncthreads();  // the previous row's output reads are done
        for (uint32_t i = tid; i < m0; i += NT) se[i] = Ent{state_hashes[ob + i], kStateRef | (int64_t)i};
        // a full row's T and T's row, before the first admission test
        if (m0 == k && tid < W8) s_trow[tid] = srow[(k - 1) * W8 + tid];
        if (tid == 0) s_cnt = m0;
        __syncthreads();
        Team t{m0, m0, kMaxI64, -1, false};
        if (m0 == k) {
            t.Th = se[k - 1].h;
            t.Tk = kStateRef | (int64_t)(k - 1);
        }
        int64_t r0 = 0, r1 = 0;
        if constexpr (!MERGE) java_r0r1(seed0 + (uint64_t)r, r0, r1);
        const Rows<true, !MERGE> src{{{in_rows, W8, srow, k}}, in_hashes, vec16, r0, r1, s_trow};
        if constexpr (MERGE) {
            for (int32_t p = 0; p < parts; ++p) {
                const int64_t row = (int64_t)p * num_states + r;
                const int64_t n = clamp_count(part_counts[row], k);
                const int64_t pb = row * (int64_t)k;
                take_piece<Rows<true, false>, NT>(se, &s_cnt, s_scan, src, pb, pb + n, k, P, t);
            }
        } else {
            take_piece<Rows<true, true>, NT>(se, &s_cnt, s_scan, src, lo, hi, k, P, t);
        }
        if (!t.dirty) return;  // nothing admitted: the row stands as it is
        if (t.n_tot != t.m) t.m = merge_set<NT>(se, t.n_tot, k, s_scan, src);
        __syncthreads();
        const uint32_t m = t.m;
        // an empty row holds no state ref: its chunks have nothing to wait for
        const bool staged = m0 != 0;
        for (uint32_t top = m * W8; top > 0;) {  // m * W8 <= 4096 * 32
            const uint32_t bot = top > NT * kMoveWords ? top - NT * kMoveWords : 0;
            uint64_t v[kMoveWords];
            bool mv[kMoveWords];
#pragma unroll
            for (uint32_t u = 0; u < kMoveWords; ++u) {
                const uint32_t x = bot + u * NT + tid;
                mv[u] = false;
                v[u] = 0;
                if (x < top) {
                    const uint32_t j = x / W8, w = x - j * W8;
                    const int64_t ref = se[j].key;
                    mv[u] = ref != (kStateRef | (int64_t)j);
                    if (mv[u]) v[u] = src.at(ref)[w];
                }
            }
            if (staged) {
                // the loads have returned before any lane of the team stores
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __syncthreads();
            }
#pragma unroll
            for (uint32_t u = 0; u < kMoveWords; ++u)
                if (mv[u]) srow[bot + u * NT + tid] = v[u];
            top = bot;
        }
        for (uint32_t i = tid; i < m; i += NT) {
            const Ent e = se[i];
            if (e.key != (kStateRef | (int64_t)i)) state_hashes[ob + i] = e.h;
        }
        if (m0 == 0 || c0 != (int64_t)m0 || m < m0) {
            __syncthreads();  // an invalid state may have read above m
            for (uint32_t x = m * W8 + tid; x < k * W8; x += NT) srow[x] = 0;
            for (uint32_t i = m + tid; i < k; i += NT) state_hashes[ob + i] = 0;
        }
        if (tid == 0) state_counts[r] = m;
    });
}

// ---- Candidates by hash (rsv_distinct_segmented_candidates) ----
// Sampler.distinct for any B, S streams per launch: the kernel reads hash(map(x)) alone, 8 bytes per element, and
// emits per segment, in arrival order, the positions RandomValues could still admit; the caller's replica decides
// them.  The row's state is the hash shadow: the <= k smallest distinct scrambled hashes among the candidates the
// row has emitted, ascending, as entries (h, 0) -- so merge_set, the forms and the lazy scheme are the set loop's
// own, and equal hashes are one entry whatever elements carry them.  k distinct hash values seen mean the
// reference's set is full and its maxHash is at most the k-th of them, whichever k seen values
// they are: a full shadow's k-th value T bounds maxHash.
//   bound      min(T when the shadow is full, max_hashes[r] when set_sizes[r] >= k: the caller's replica as of its
//              last replay).  Neither known: the row is open and every element is a candidate, INT64_MAX included.
//              Otherwise a candidate has h < bound, strictly: the reference admits below maxHash only, so a repeat
//              of T itself is none (the set loop's `admits` lets it through; this loop has its own test).
//   lazy T     candidates are appended behind the shadow and merged when the buffer cannot take another step (or
//              4k wait below a full shadow), as in take_piece.  Between two merges T is the last merge's, which is
//              above the exact one: more candidates, never fewer, and at most one buffer of them (P entries: 256 /
//              512 / 2048 / 8192 by form) behind the exact running T.
//   emission   a step's candidates in lane order, the waves' counts summed in wave order through s_wave (two
//              buffers, taken in turn: one barrier per step).  The LDS append uses the same offsets, so the launch
//              is deterministic and takes no atomic.  Entry j of segment b goes to out[b * cap + j] while j < cap;
//              out_counts[b] is the number found, stored or not.
//   epilogue   found > cap: nothing of the row is written, and a rerun with cap >= found starts from the same row
//              and, the merges depending on counts alone, finds the same candidates.  Nothing found: nothing
//              written.  Otherwise the last merge, the shadow and zeros up to k, the count.
// A skipped segment (an id outside [0, num_states), or no elements) gets out_counts[b] = 0 before any row is
// addressed; the count read from the state is clamped, and nothing else read from it indexes memory.
template <int NT>
__global__ __launch_bounds__(NT) void segcand_kernel(const int64_t* __restrict__ hashes, const int64_t* __restrict__ offsets,
                                                     const int64_t* __restrict__ ids, int64_t num_segments,
                                                     int64_t num_states, uint32_t k, uint32_t P, uint64_t seed0,
                                                     int64_t* shadow_hashes, int64_t* shadow_counts,
                                                     const int64_t* __restrict__ set_sizes,
                                                     const int64_t* __restrict__ max_hashes, int64_t* __restrict__ out_pos,
                                                     int64_t* __restrict__ out_hashes, int64_t cap,
                                                     int64_t* __restrict__ out_counts) {
    extern __shared__ __align__(16) unsigned char seg_lds[];
    Ent* const se = (Ent*)seg_lds;
    constexpr uint32_t kWavesT = NT / 64;
    __shared__ uint32_t s_scan[kWavesT > 1 ? kWavesT : 1];
    __shared__ uint32_t s_wave[2][kWavesT > 1 ? kWavesT : 1];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint32_t turn = 0;  // which s_wave buffer the next step writes

    for (int64_t b = blockIdx.x; b < num_segments; b += gridDim.x) {
        const int64_t r = ids ? ids[b] : b;
        const int64_t lo = offsets[b], hi = offsets[b + 1];
        if (r < 0 || r >= num_states || hi <= lo) {
            if (tid == 0) out_counts[b] = 0;
            continue;
        }
        const int64_t ob = r * (int64_t)k, eb = b * cap;
        const uint32_t m0 = clamp_count(shadow_counts[r], k);
        __syncthreads();  // the previous row's output reads are done
        for (uint32_t i = tid; i < m0; i += NT) se[i] = Ent{shadow_hashes[ob + i], 0};
        __syncthreads();
        const bool caller_full = set_sizes && set_sizes[r] >= (int64_t)k;
        const int64_t caller_bound = caller_full ? max_hashes[r] : kMaxI64;
        uint32_t m = m0, n = m0;  // the shadow's size; the shadow and the candidates behind it
        int64_t bound = caller_bound;
        if (m == k) bound = std::min(bound, se[k - 1].h);
        bool open = !caller_full && m < k;
        int64_t r0, r1;
        java_r0r1(seed0 + (uint64_t)r, r0, r1);
        int64_t found = 0;

        constexpr int64_t kChunk = (int64_t)NT * kU;
        for (int64_t base = lo; base < hi; base += kChunk) {
            int64_t hv[kU];
#pragma unroll
            for (int u = 0; u < kU; ++u) {
                const int64_t i = base + (int64_t)u * NT + tid;
                hv[u] = i < hi ? hashes[i] : 0;
            }
#pragma unroll
            for (int u = 0; u < kU; ++u) {
                const int64_t i = base + (int64_t)u * NT + tid;
                if (base + (int64_t)u * NT >= hi) break;  // uniform: the tail chunk's empty steps
                if (n + NT > P || (m < k && n >= 4 * k)) {
                    m = merge_set<NT>(se, n, k, s_scan, KeyOrd{});
                    n = m;
                    if (m == k) {  // (the appends land behind se[k - 1])
                        bound = std::min(caller_bound, se[k - 1].h);
                        open = false;
                    }
                }
                const int64_t h = scramble(r0, r1, hv[u]);
                const bool pass = i < hi && (open || h < bound);
                const uint64_t mask = __ballot(pass);
                uint32_t pre = (uint32_t)__popcll(mask & ((1ULL << lane) - 1));
                uint32_t total = (uint32_t)__popcll(mask);
                if constexpr (kWavesT > 1) {
                    if (lane == 0) s_wave[turn][wave] = total;
                    __syncthreads();
                    total = 0;
                    for (uint32_t w = 0; w < kWavesT; ++w) {
                        const uint32_t c = s_wave[turn][w];
                        if (w < wave) pre += c;
                        total += c;
                    }
                    turn ^= 1;
                }
                if (pass) {  // n + NT <= P
                    se[n + pre] = Ent{h, 0};
                    const int64_t j = found + pre;
                    if (j < cap) {
                        out_pos[eb + j] = i;
                        out_hashes[eb + j] = h;
                    }
                }
                n += total;
                found += total;
            }
        }
        if (tid == 0) out_counts[b] = found;
        if (found == 0 || found > cap) continue;
        if (n != m) m = merge_set<NT>(se, n, k, s_scan, KeyOrd{});
        __syncthreads();
        for (uint32_t i = tid; i < k; i += NT) shadow_hashes[ob + i] = i < m ? se[i].h : 0;
        if (tid == 0) shadow_counts[r] = m;
    }
}

// ---- Ordered (rsv_distinct_segmented_ordered, _rows_ordered) ----
// "Key" below reads "row" over byte keys.  Once RandomValues' heap is full its maximum M is the k-th smallest hash
// over the distinct keys seen and it holds every key with h < M, so its set is the bottom-k by (h, key) unless more
// than k distinct keys have h <= M: only then does the arrival order decide who of the bucket h = M stays.  Two
// kernels: the stateless frame with TIED, which also finds those streams, and a replay of RandomValues for them alone.
//
// Kernel 1, Tied<>.  A refused element is a distinct key outside the final set, for T only falls: a lane that fails
// `admits` at h = T.h holds a key strictly above T's (an equal key, row or ref passes).  And a distinct key x outside
// the final set with h(x) = M, the final maximum, is refused at its first occurrence at the latest, or trimmed, at a
// time when M <= T.h <= h(x), so T.h = M then and ever after and the note stays.  Hence
//   tied = (m == k && some lane holds a note),
// exactly, whatever M is: below k entries T is the pad, which admits everything, and nothing is refused.  This says
// what "the minimum h of everything refused equals se[k-1].h" says (a refused h is never below T.h) at one v_cndmask
// per step: the compare h == T.h is the admission test's own.  Keeping the minimum itself cost 7 VALU per step
// (DESIGN.md 5c.3 has both measurements).
//
// Kernel 2: RandomValues (Sampler.scala:394-409) over the tied streams, one wave per stream (replay_walk from an empty
// heap).  A wave reads the tied words of W consecutive streams at once and replays those that are set, one after the
// other.  At the end the k entries are sorted by (h, key) and written over the row kernel 1 left, over byte keys the m
// rows gathered; count and tied stay.  No row is staged in LDS.

// RandomValues' queue: scala 2.13 mutable.PriorityQueue, rsv_host_values.h's heap, 1-indexed in se[0, k) (entry j at
// se[j - 1]) and ordered by h alone.  Admits c into the heap of n entries and capacity k: at n == k dequeue/fixDown
// first (the root leaves: last entry to the root, sink to the larger child, left on ties, stop when parent >= child),
// then addOne/fixUp (sift up while parent < child).  One lane's work.  The only place that knows the queue's tie rules:
// they decide which member of a bucket of equal hashes survives.  It addresses se below max(n, 1) <= k only (parents
// and children of positions <= n), whatever the entries hold.
__device__ __forceinline__ void heap_admit(Ent* const se, uint32_t n, uint32_t k, const Ent c) {
    if (n == k) {  // dequeue: the root leaves
        const Ent last = se[n - 1];
        --n;
        if (n) {
            uint32_t q = 1;
            while (2 * q <= n) {
                uint32_t ch = 2 * q;
                if (ch + 1 <= n && se[ch - 1].h < se[ch].h) ++ch;
                if (last.h >= se[ch - 1].h) break;
                se[q - 1] = se[ch - 1];
                q = ch;
            }
            se[q - 1] = last;
        }
    }
    uint32_t q = n + 1;  // addOne
    while (q > 1 && se[(q >> 1) - 1].h < c.h) {
        se[q - 1] = se[(q >> 1) - 1];
        q >>= 1;
    }
    se[q - 1] = c;
}

// RandomValues.sample over the elements [lo, hi) of src in arrival order, by one wave, on the heap se[0, n) with maxh
// its root's h (INT64_MIN while it is empty); returns whether anything was admitted.  The one piece of device code all
// four ordered kernels run per stream: the replays from an empty heap, the resumed kernels from the caller's.
// The stream is walked 64 elements a step (kU steps loaded ahead).  Of a step, the first lane whose element passes the
// current test (size < k, or h < maxHash) is taken, looked up among the heap's entries by all lanes
// (elements.contains: n / 64 reads per lane, eight in flight; what is read and compared is the source's), and admitted
// by lane 0 if absent; then the lanes behind it are tested again, against the new maxHash.  maxHash never rises once
// the heap is full and below that every element passes, so a lane that failed once fails for good and the lanes taken
// are in arrival order.  The barriers order lane 0's heap writes and the other lanes' reads; with one wave per
// workgroup they cost no wait.  The heap is left as the last admission wrote it, behind a barrier.
// STATE (rows resumed): an admission takes its slot by the rule: the heap's size when it grows, the evicted root's
// slot when it is full.
template <bool STATE, typename Src>
__device__ __forceinline__ bool replay_walk(Ent* const se, const Src src, int64_t lo, int64_t hi, uint32_t k, uint32_t& n_io,
                                            int64_t& maxh_io) {
    // (locals, written back at the end: with them the replay kernel compiles to the instructions it had when
    // this loop stood in its body; through the references it did not)
    uint32_t n = n_io;
    int64_t maxh = maxh_io;
    const uint32_t lane = threadIdx.x;
    bool admitted = false;
    for (int64_t base = lo; base < hi; base += 64 * kU) {
        int64_t key[kU], hv[kU];
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            const int64_t i = base + (int64_t)u * 64 + lane;
            key[u] = 0;
            hv[u] = 0;
            if (i < hi) src.load(i, key[u], hv[u]);
        }
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            const int64_t i = base + (int64_t)u * 64 + lane;
            if (base + (int64_t)u * 64 >= hi) break;  // uniform
            const int64_t h = src.h_of(key[u], hv[u]);
            bool pend = i < hi;
            for (;;) {
                const uint64_t mask = __ballot(pend && (n < k || h < maxh));
                if (!mask) break;
                const int l = __ffsll((long long)mask) - 1;
                if ((int)lane == l) pend = false;
                Ent c{read_lane(h, l), src.second_of(key[u], base + (int64_t)u * 64, l)};  // the candidate
                bool found = false;
                const uint32_t full = n >> 6;
                uint32_t r = 0;
                for (; r + 8 <= full; r += 8) {
                    int64_t mw[8];
#pragma unroll
                    for (int x = 0; x < 8; ++x) mw[x] = src.scan_word(se + (r + x) * 64 + lane);
#pragma unroll
                    for (int x = 0; x < 8; ++x) found = src.look(found, mw[x], se + (r + x) * 64 + lane, c);
                }
                for (uint32_t j = r * 64 + lane; j < n; j += 64) found = src.look(found, src.scan_word(se + j), se + j, c);
                if (__ballot(found)) continue;  // a member
                if (lane == 0) {
                    if constexpr (STATE) c.key |= (int64_t)(n == k ? slot_of(se[0].key, k) : n) << kSlotShift;
                    heap_admit(se, n, k, c);
                }
                if (n < k) ++n;
                admitted = true;
                __syncthreads();
                maxh = se[0].h;
                __syncthreads();
            }
        }
    }
    n_io = n;
    maxh_io = maxh;
    return admitted;
}

// Kernel 2's frame: f(s) for every stream s whose tied word is set, W consecutive words per step of a wave.
template <typename F>
__device__ __forceinline__ void for_tied_streams(const int32_t* __restrict__ tied, int64_t S, uint32_t W, F f) {
    const uint32_t lane = threadIdx.x;
    const int64_t groups = (S + W - 1) / W;
    for (int64_t g = blockIdx.x; g < groups; g += gridDim.x) {
        const int64_t sl = g * W + lane;
        uint64_t todo = __ballot(lane < W && sl < S && tied[sl] != 0);
        while (todo) {
            const int64_t s = g * W + (__ffsll((long long)todo) - 1);
            todo &= todo - 1;
            f(s);
        }
    }
}

template <typename KeyT>
__global__ __launch_bounds__(64) void segdistinct_replay_kernel(const KeyT* __restrict__ keys, const int64_t* __restrict__ hashes,
                                                                const int64_t* __restrict__ offsets, int64_t S, uint32_t k,
                                                                uint32_t W, int hash_kind, uint64_t seed0,
                                                                KeyT* __restrict__ out_keys, int64_t* __restrict__ out_hashes,
                                                                const int32_t* __restrict__ tied) {
    extern __shared__ __align__(16) unsigned char seg_lds[];
    Ent* const se = (Ent*)seg_lds;
    __shared__ uint32_t s_scan[1];
    const uint32_t lane = threadIdx.x;

    for_tied_streams(tied, S, W, [&](int64_t s) {
        const int64_t lo = offsets[s], hi = offsets[s + 1];
        int64_t r0, r1;
        java_r0r1(seed0 + (uint64_t)s, r0, r1);
        const Keys<KeyT, true> src{{}, keys, hashes, hash_kind, r0, r1};
        uint32_t n = 0;            // heap size (uniform)
        int64_t maxh = INT64_MIN;  // the root's h once anything is in
        __syncthreads();           // the previous stream's output reads are done
        replay_walk<false>(se, src, lo, hi, k, n, maxh);
        const uint32_t m = merge_set<64>(se, n, k, s_scan, KeyOrd{});
        __syncthreads();
        const int64_t ob = s * (int64_t)k;
        for (uint32_t i = lane; i < m; i += 64) {
            const Ent e = se[i];
            out_keys[ob + i] = (KeyT)e.key;
            if (out_hashes) out_hashes[ob + i] = e.h;
        }
    });
}

__global__ __launch_bounds__(64) void segrows_replay_kernel(const uint64_t* __restrict__ rows, const int64_t* __restrict__ hashes,
                                                            const int64_t* __restrict__ offsets, int64_t S, uint32_t W8,
                                                            uint32_t k, uint32_t W, uint64_t seed0,
                                                            uint64_t* __restrict__ out_rows, int64_t* __restrict__ out_hashes,
                                                            const int32_t* __restrict__ tied) {
    extern __shared__ __align__(16) unsigned char seg_lds[];
    Ent* const se = (Ent*)seg_lds;
    __shared__ uint32_t s_scan[1];
    const bool vec16 = ((uintptr_t)rows & 15) == 0;

    for_tied_streams(tied, S, W, [&](int64_t s) {
        const int64_t lo = offsets[s], hi = offsets[s + 1];
        int64_t r0, r1;
        java_r0r1(seed0 + (uint64_t)s, r0, r1);
        const Rows<false, true> src{{{rows, W8}}, hashes, vec16, r0, r1, nullptr};  // no T here: admits is not used
        const RowOrd<false>& ord = src;
        uint32_t n = 0;            // heap size (uniform)
        int64_t maxh = INT64_MIN;  // the root's h once anything is in
        __syncthreads();           // the previous stream's output reads are done
        replay_walk<false>(se, src, lo, hi, k, n, maxh);
        const uint32_t m = merge_set<64>(se, n, k, s_scan, ord);
        __syncthreads();
        gather_rows<64, false>(se, m, k, rows, W8, s * (int64_t)k, out_rows, out_hashes);
    });
}

// ---- Ordered, resumed (rsv_distinct_segmented_ordered_update, _rows_ordered_update) ----
// RandomValues' whole state is the queue's array, a set of the array's keys, and maxHash, which at every moment
// is the root's h: below k entries the running maximum, which a max-heap keeps at its root, at k entries
// samples.head._2.  addOne/fixUp and dequeue/fixDown are functions of the array alone, and the argument does not ask
// what a key is.  So the row's count and its entries in array order -- entry j of the 1-indexed queue in slot j - 1 --
// are the sampler, and replay_walk from them is the reference going on.  A row kept sorted is a heap too, but another
// one: its later dequeues move other entries, and the bucket at the maximum hash ends with other members.
// One wave per segment, segments grid-stride; row r = ids[b] (or b), seeded seed0 + r (for_resumed_items).
//   prologue   n = the clamped count; the row's pairs (h, key) into se[0, n) as they lie; maxh = se[0].h when n > 0.
//   walk       replay_walk, the replay's own.
//   epilogue   only if something was admitted: se[0, n) back as they lie, zeros up to k, the count.  No sort.
// A row that is no heap gives an unspecified set at the same addresses (heap_admit).
template <typename KeyT>
__global__ __launch_bounds__(64) void segdistinct_heap_kernel(const KeyT* __restrict__ keys, const int64_t* __restrict__ hashes,
                                                              const int64_t* __restrict__ offsets,
                                                              const int64_t* __restrict__ ids, int64_t num_segments,
                                                              int64_t num_states, uint32_t k, int hash_kind, uint64_t seed0,
                                                              KeyT* state_keys, int64_t* state_hashes, int64_t* state_counts) {
    extern __shared__ __align__(16) unsigned char seg_lds[];
    Ent* const se = (Ent*)seg_lds;
    const uint32_t lane = threadIdx.x;

    for_resumed_items<false>(num_segments, ids, offsets, num_states, state_counts, k, [&](const Resumed g) {
        const int64_t r = g.r, ob = r * (int64_t)k;
        uint32_t n = g.m0;
        __syncthreads();  // the previous row's output reads are done
        for (uint32_t i = lane; i < n; i += 64) se[i] = Ent{state_hashes[ob + i], (int64_t)state_keys[ob + i]};
        __syncthreads();
        int64_t maxh = INT64_MIN;
        if (n) maxh = se[0].h;
        int64_t r0, r1;
        java_r0r1(seed0 + (uint64_t)r, r0, r1);
        const Keys<KeyT, true> src{{}, keys, hashes, hash_kind, r0, r1};
        if (!replay_walk<false>(se, src, g.lo, g.hi, k, n, maxh)) return;  // nothing admitted: the row stands as it is
        for (uint32_t i = lane; i < k; i += 64) {
            const Ent e = i < n ? se[i] : Ent{0, 0};
            state_keys[ob + i] = (KeyT)e.key;
            state_hashes[ob + i] = e.h;
        }
        if (lane == 0) state_counts[r] = n;
    });
}

// Over byte keys the array holds what it holds on the JVM, references: the row block state_rows[r] is storage whose
// order means nothing, hashes[r][p] and slots[r][p] are position p of the array, and the row of that entry lies in
// slot slots[r][p] of the block.  An admission that grows the heap from n to n + 1 takes slot n, one into a full
// heap takes the slot of the root it evicts: below k the slots in use are {0..n-1}, at k a permutation, and no
// surviving row ever moves.
//   prologue   entry p into se[p] as (hashes[p], kStateRef | slot), the slot clamped below k (every slot, as the
//              count: nothing read from the state indexes memory unclamped); maxh = se[0].h when n > 0.  No row is read.
//   walk       replay_walk; rows are read from the input or from a state slot only for entries with the candidate's
//              hash.
//   epilogue   only if something was admitted: hashes and slots of se[0, n) as they lie and zeros up to k, then for
//              every entry that refers to the input its row into its slot, lanes over (entry, word), then the count.
//              No sort and no staged move: the rows read are the input's, and the slots written are the ones no
//              surviving state entry names (a grown heap's new slots, or slots of evicted roots), so nothing is
//              read after it was overwritten and no member's row is touched.  Slots [n, k) of the block are zeroed
//              when the row was empty before or its count had to be clamped (the caller's bytes), else they are
//              the kernel's own zeros already.
// Repeated or out-of-range slots, a row that is no heap and a wrong count give an unspecified set at the same
// addresses.
__global__ __launch_bounds__(64) void segrows_heap_kernel(const uint64_t* in_rows, const int64_t* __restrict__ hashes,
                                                          const int64_t* __restrict__ offsets,
                                                          const int64_t* __restrict__ ids, int64_t num_segments,
                                                          int64_t num_states, uint32_t W8, uint32_t k, uint64_t seed0,
                                                          uint64_t* state_rows, int64_t* state_hashes,
                                                          int32_t* state_slots, int64_t* state_counts) {
    extern __shared__ __align__(16) unsigned char seg_lds[];
    Ent* const se = (Ent*)seg_lds;
    const uint32_t lane = threadIdx.x;
    const bool vec16 = ((uintptr_t)in_rows & 15) == 0;

    for_resumed_items<false>(num_segments, ids, offsets, num_states, state_counts, k, [&](const Resumed g) {
        const int64_t r = g.r, c0 = g.c0, ob = r * (int64_t)k;
        uint64_t* const srow = state_rows + ob * (int64_t)W8;
        const uint32_t n0 = g.m0;
        uint32_t n = n0;
        __syncthreads();  // the previous row's output reads are done
        for (uint32_t i = lane; i < n; i += 64) {
            const uint32_t j = (uint32_t)state_slots[ob + i];  // a negative slot is a large one
            se[i] = Ent{state_hashes[ob + i], kStateRef | (int64_t)(j < k ? j : k - 1)};
        }
        __syncthreads();
        int64_t maxh = INT64_MIN;
        if (n) maxh = se[0].h;
        int64_t r0, r1;
        java_r0r1(seed0 + (uint64_t)r, r0, r1);
        const Rows<true, true> src{{{in_rows, W8, srow, k}}, hashes, vec16, r0, r1, nullptr};  // no T here
        if (!replay_walk<true>(se, src, g.lo, g.hi, k, n, maxh)) return;  // nothing admitted: the row stands as it is
        if (n0 == 0 || c0 != (int64_t)n0)
            for (uint32_t x = n * W8 + lane; x < k * W8; x += 64) srow[x] = 0;  // k * W8 <= 4096 * 32
        for (uint32_t i = lane; i < k; i += 64) {
            const Ent e = i < n ? se[i] : Ent{0, 0};
            state_hashes[ob + i] = e.h;
            state_slots[ob + i] = i < n ? (int32_t)slot_of(e.key, k) : 0;
        }
        for (uint32_t x = lane; x < n * W8; x += 64) {
            const uint32_t j = x / W8, w = x - j * W8;
            const int64_t ref = se[j].key;
            if (!(ref & kStateRef)) srow[slot_of(ref, k) * W8 + w] = in_rows[(ref & kRowIndexMask) * (int64_t)W8 + w];
        }
        if (lane == 0) state_counts[r] = n;
    });
}

// The forms: f(KeyT{}, NT as an integral_constant, P) for the key width and k of a launch.
template <typename KeyT, typename F>
hipError_t with_form_of(uint32_t k, F& f) {
    if (k <= kSegDistinctWaveMaxK)  // P >= k + 192: three steps of 64 fit behind a full set
        return f(KeyT{}, std::integral_constant<int, 64>{}, k <= 64 ? 256u : 512u);
    if (k <= 1024) return f(KeyT{}, std::integral_constant<int, 256>{}, 2048u);
    return f(KeyT{}, std::integral_constant<int, 1024>{}, 8192u);
}

template <typename F>
hipError_t with_form(int key_width, uint32_t k, F f) {
    return key_width == 8 ? with_form_of<int64_t>(k, f) : with_form_of<int32_t>(k, f);
}

// One team of nt threads with P entries of LDS per item, grid-stride.
template <typename... Params, typename... Args>
hipError_t launch_teams(void (*kernel)(Params...), int nt, int64_t teams, uint32_t P, hipStream_t st, Args... args) {
    const size_t lds = (size_t)P * 16;
    if (lds > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    // the teams the 256 CUs hold at once (LDS and 32 waves per CU), four times over
    const uint64_t per_cu = std::max<uint64_t>(1, std::min<uint64_t>((160 * 1024) / (lds + 256), 32 / (nt / 64)));
    const unsigned grid = (unsigned)std::min<uint64_t>((uint64_t)teams, 256ull * per_cu * 4);
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(nt), lds, st, args...);
    return hipGetLastError();
}

// The ordered kernels' launches: one wave and pow2ceil(k) entries (the heap, and the pads of the replay's final
// sort) per item in flight.  plan_heap_waves gives the LDS of one wave's heap, sets the attribute above 64 KB, and
// gives `cap`, the waves the 256 CUs hold at once, four times over.
hipError_t plan_heap_waves(const void* kernel, uint32_t k, size_t& lds, uint64_t& cap) {
    uint32_t P2 = 2;
    while (P2 < k) P2 <<= 1;
    lds = (size_t)P2 * 16;
    if (lds + 256 > 64 * 1024) {
        const hipError_t a = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (a != hipSuccess) return a;
    }
    const uint64_t per_cu = std::max<uint64_t>(1, std::min<uint64_t>((160 * 1024) / (lds + 256), 32));
    cap = 256ull * per_cu * 4;
    return hipSuccess;
}

// One wave per item, items grid-stride: the resumed ordered launches (there is no tied word to read, every segment
// is walked).
template <typename... Params, typename... Args>
hipError_t launch_heap_waves(void (*kernel)(Params...), int64_t items, uint32_t k, hipStream_t st, Args... args) {
    size_t lds;
    uint64_t cap;
    if (const hipError_t a = plan_heap_waves((const void*)kernel, k, lds, cap); a != hipSuccess) return a;
    const unsigned grid = (unsigned)std::min<uint64_t>((uint64_t)items, cap);
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(64), lds, st, args...);
    return hipGetLastError();
}

// The stateless ordered launches: kernel 1 (`first`, a launch_teams of the TIED frame), then the replay of the tied
// streams.  A wave of the replay looks at W consecutive tied words per step: 64 when there are streams enough to fill
// the grid that way, fewer when not, so that few streams still spread over the CUs.  replay(grid, lds, W) launches it.
template <typename First, typename Replay>
hipError_t launch_tied_then_replay(const void* replay_kernel, int64_t S, uint32_t k, First first, Replay replay) {
    if (const hipError_t e = first(); e != hipSuccess) return e;
    size_t lds;
    uint64_t cap;
    if (const hipError_t a = plan_heap_waves(replay_kernel, k, lds, cap); a != hipSuccess) return a;
    uint32_t W = 1;
    while (W < 64 && (uint64_t)S / (2 * W) >= cap) W <<= 1;
    replay(dim3((unsigned)std::min<uint64_t>(((uint64_t)S + W - 1) / W, cap)), lds, W);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_segdistinct(const void* keys, int key_width, const int64_t* hashes, const int64_t* offsets, int64_t S,
                              uint32_t k, int hash_kind, uint64_t seed0, void* out_keys, int64_t* out_hashes,
                              int64_t* counts, hipStream_t st) {
    if (S <= 0) return hipSuccess;
    return with_form(key_width, k, [&](auto key, auto nt, uint32_t P) {
        using KeyT = decltype(key);
        constexpr int NT = decltype(nt)::value;
        return launch_teams(segdistinct_kernel<KeyT, NT, false>, NT, S, P, st, (const KeyT*)keys, hashes, offsets, S, k, P,
                            hash_kind, seed0, (KeyT*)out_keys, out_hashes, counts, (int32_t*)nullptr);
    });
}

hipError_t launch_segdistinct_ordered(const void* keys, int key_width, const int64_t* hashes, const int64_t* offsets,
                                      int64_t S, uint32_t k, int hash_kind, uint64_t seed0, void* out_keys,
                                      int64_t* out_hashes, int64_t* counts, int32_t* tied, hipStream_t st) {
    if (S <= 0) return hipSuccess;
    return with_form(key_width, k, [&](auto key, auto nt, uint32_t P) {
        using KeyT = decltype(key);
        constexpr int NT = decltype(nt)::value;
        auto* const replay = segdistinct_replay_kernel<KeyT>;
        return launch_tied_then_replay(
            (const void*)replay, S, k,
            [&] {
                return launch_teams(segdistinct_kernel<KeyT, NT, true>, NT, S, P, st, (const KeyT*)keys, hashes, offsets, S, k,
                                    P, hash_kind, seed0, (KeyT*)out_keys, out_hashes, counts, tied);
            },
            [&](dim3 grid, size_t lds, uint32_t W) {
                hipLaunchKernelGGL(replay, grid, dim3(64), lds, st, (const KeyT*)keys, hashes, offsets, S, k, W, hash_kind,
                                   seed0, (KeyT*)out_keys, out_hashes, (const int32_t*)tied);
            });
    });
}

hipError_t launch_segdistinct_rows(const void* rows, int key_width, const int64_t* hashes, const int64_t* offsets,
                                   int64_t S, uint32_t k, uint64_t seed0, void* out_rows, int64_t* out_hashes,
                                   int64_t* counts, hipStream_t st) {
    if (S <= 0) return hipSuccess;
    auto f = [&](int64_t, auto nt, uint32_t P) {
        constexpr int NT = decltype(nt)::value;
        return launch_teams(segrows_kernel<NT, false>, NT, S, P, st, (const uint64_t*)rows, hashes, offsets, S,
                            (uint32_t)key_width / 8, k, P, seed0, (uint64_t*)out_rows, out_hashes, counts,
                            (int32_t*)nullptr);
    };
    return with_form_of<int64_t>(k, f);
}

hipError_t launch_segdistinct_rows_ordered(const void* rows, int key_width, const int64_t* hashes, const int64_t* offsets,
                                           int64_t S, uint32_t k, uint64_t seed0, void* out_rows, int64_t* out_hashes,
                                           int64_t* counts, int32_t* tied, hipStream_t st) {
    if (S <= 0) return hipSuccess;
    const uint32_t W8 = (uint32_t)key_width / 8;
    auto f = [&](int64_t, auto nt, uint32_t P) {
        constexpr int NT = decltype(nt)::value;
        return launch_tied_then_replay(
            (const void*)segrows_replay_kernel, S, k,
            [&] {
                return launch_teams(segrows_kernel<NT, true>, NT, S, P, st, (const uint64_t*)rows, hashes, offsets, S, W8, k,
                                    P, seed0, (uint64_t*)out_rows, out_hashes, counts, tied);
            },
            [&](dim3 grid, size_t lds, uint32_t W) {
                hipLaunchKernelGGL(segrows_replay_kernel, grid, dim3(64), lds, st, (const uint64_t*)rows, hashes, offsets, S,
                                   W8, k, W, seed0, (uint64_t*)out_rows, out_hashes, (const int32_t*)tied);
            });
    };
    return with_form_of<int64_t>(k, f);
}

hipError_t launch_segdistinct_update(const void* keys, int key_width, const int64_t* hashes, const int64_t* offsets,
                                     const int64_t* stream_ids, int64_t num_segments, int64_t num_states, uint32_t k,
                                     int hash_kind, uint64_t seed0, void* state_keys, int64_t* state_hashes,
                                     int64_t* state_counts, hipStream_t st) {
    if (num_segments <= 0 || num_states <= 0) return hipSuccess;
    return with_form(key_width, k, [&](auto key, auto nt, uint32_t P) {
        using KeyT = decltype(key);
        constexpr int NT = decltype(nt)::value;
        return launch_teams(segstate_kernel<KeyT, NT, false>, NT, num_segments, P, st, (const KeyT*)keys, hashes,
                            offsets, stream_ids, (const int64_t*)nullptr, num_segments, num_states, (int32_t)0, k, P,
                            hash_kind, seed0, (KeyT*)state_keys, state_hashes, state_counts);
    });
}

hipError_t launch_segdistinct_ordered_update(const void* keys, int key_width, const int64_t* hashes, const int64_t* offsets,
                                             const int64_t* stream_ids, int64_t num_segments, int64_t num_states,
                                             uint32_t k, int hash_kind, uint64_t seed0, void* state_keys,
                                             int64_t* state_hashes, int64_t* state_counts, hipStream_t st) {
    if (num_segments <= 0 || num_states <= 0) return hipSuccess;
    auto go = [&](auto key) {
        using KeyT = decltype(key);
        return launch_heap_waves(segdistinct_heap_kernel<KeyT>, num_segments, k, st, (const KeyT*)keys, hashes, offsets,
                                 stream_ids, num_segments, num_states, k, hash_kind, seed0, (KeyT*)state_keys, state_hashes,
                                 state_counts);
    };
    return key_width == 8 ? go(int64_t{}) : go(int32_t{});
}

// (the heap's 16-byte entries carry their slots, so the LDS is launch_segdistinct_ordered_update's)
hipError_t launch_segdistinct_rows_ordered_update(const void* rows, int key_width, const int64_t* hashes,
                                                  const int64_t* offsets, const int64_t* stream_ids, int64_t num_segments,
                                                  int64_t num_states, uint32_t k, uint64_t seed0, void* state_rows,
                                                  int64_t* state_hashes, int32_t* state_slots, int64_t* state_counts,
                                                  hipStream_t st) {
    if (num_segments <= 0 || num_states <= 0) return hipSuccess;
    return launch_heap_waves(segrows_heap_kernel, num_segments, k, st, (const uint64_t*)rows, hashes, offsets, stream_ids,
                             num_segments, num_states, (uint32_t)key_width / 8, k, seed0, (uint64_t*)state_rows,
                             state_hashes, state_slots, state_counts);
}

hipError_t launch_segdistinct_merge(const void* part_keys, int key_width, const int64_t* part_hashes,
                                    const int64_t* part_counts, int32_t parts, int64_t num_states, uint32_t k,
                                    void* state_keys, int64_t* state_hashes, int64_t* state_counts, hipStream_t st) {
    if (parts <= 0 || num_states <= 0) return hipSuccess;
    return with_form(key_width, k, [&](auto key, auto nt, uint32_t P) {
        using KeyT = decltype(key);
        constexpr int NT = decltype(nt)::value;
        return launch_teams(segstate_kernel<KeyT, NT, true>, NT, num_states, P, st, (const KeyT*)part_keys,
                            part_hashes, (const int64_t*)nullptr, (const int64_t*)nullptr, part_counts, num_states,
                            num_states, parts, k, P, (int)kHashPrecomputed, (uint64_t)0, (KeyT*)state_keys, state_hashes,
                            state_counts);
    });
}

hipError_t launch_segdistinct_rows_update(const void* rows, int key_width, const int64_t* hashes, const int64_t* offsets,
                                          const int64_t* stream_ids, int64_t num_segments, int64_t num_states,
                                          uint32_t k, uint64_t seed0, void* state_rows, int64_t* state_hashes,
                                          int64_t* state_counts, hipStream_t st) {
    if (num_segments <= 0 || num_states <= 0) return hipSuccess;
    auto f = [&](int64_t, auto nt, uint32_t P) {
        constexpr int NT = decltype(nt)::value;
        return launch_teams(segrowstate_kernel<NT, false>, NT, num_segments, P, st, (const uint64_t*)rows, hashes,
                            offsets, stream_ids, (const int64_t*)nullptr, num_segments, num_states, (int32_t)0,
                            (uint32_t)key_width / 8, k, P, seed0, (uint64_t*)state_rows, state_hashes, state_counts);
    };
    return with_form_of<int64_t>(k, f);
}

hipError_t launch_segdistinct_candidates(const int64_t* hashes, const int64_t* offsets, const int64_t* stream_ids,
                                         int64_t num_segments, int64_t num_states, uint32_t k, uint64_t seed0,
                                         int64_t* shadow_hashes, int64_t* shadow_counts, const int64_t* set_sizes,
                                         const int64_t* max_hashes, int64_t* out_pos, int64_t* out_hashes, int64_t cap,
                                         int64_t* out_counts, hipStream_t st) {
    if (num_segments <= 0) return hipSuccess;
    auto f = [&](int64_t, auto nt, uint32_t P) {
        constexpr int NT = decltype(nt)::value;
        return launch_teams(segcand_kernel<NT>, NT, num_segments, P, st, hashes, offsets, stream_ids, num_segments,
                            num_states, k, P, seed0, shadow_hashes, shadow_counts, set_sizes, max_hashes, out_pos,
                            out_hashes, cap, out_counts);
    };
    return with_form_of<int64_t>(k, f);
}

hipError_t launch_segdistinct_rows_merge(const void* part_rows, int key_width, const int64_t* part_hashes,
                                         const int64_t* part_counts, int32_t parts, int64_t num_states, uint32_t k,
                                         void* state_rows, int64_t* state_hashes, int64_t* state_counts,
                                         hipStream_t st) {
    if (parts <= 0 || num_states <= 0) return hipSuccess;
    auto f = [&](int64_t, auto nt, uint32_t P) {
        constexpr int NT = decltype(nt)::value;
        return launch_teams(segrowstate_kernel<NT, true>, NT, num_states, P, st, (const uint64_t*)part_rows,
                            part_hashes, (const int64_t*)nullptr, (const int64_t*)nullptr, part_counts, num_states,
                            num_states, parts, (uint32_t)key_width / 8, k, P, (uint64_t)0, (uint64_t*)state_rows,
                            state_hashes, state_counts);
    };
    return with_form_of<int64_t>(k, f);
}

}  // namespace rsv
