// rsv_segdistinct.hip -- K5: S independent Sampler.distinct streams per launch, stateless
// (rsv_distinct_segmented) and resumed from caller-held state (rsv_distinct_segmented_update / _merge).
// No reference counterpart; = S separate RandomValues instances (Sampler.scala:383-412), each seeded
// with java.util.Random(seed + stream_base + s), in the engine's set order (RSV_DISTINCT_SET): stream
// s keeps the min(k, D_s) distinct keys with the smallest (scrambled hash, key), written ascending.
// rsv_distinct_segmented_ordered (the last section of this file) is the same launch followed by a
// replay of the streams whose boundary hash bucket is oversubscribed: there the members of that
// bucket are the reference's, chosen by arrival order and the heap's tie behaviour
// (RSV_DISTINCT_ORDERED), not the smallest keys; rsv_distinct_segmented_rows_ordered is that for byte-key
// rows.  rsv_distinct_segmented_ordered_update resumes the ordered form from caller-held state: k entries
// kept sorted cannot carry the heap's history, k entries kept in the queue's array
// order are the heap, and that is the state there; rsv_distinct_segmented_rows_ordered_update
// is that for byte-key rows, the array holding (hash, slot) and the rows staying in their slots of the row's
// block.  Not provided in ordered form: merge (two heaps over parts of a stream do not
// determine the heap over the whole), k > 4096.
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
// Forms (DESIGN.md "Segmented distinct"; with_form below is the only place that names them):
//   k <= 64    NT = 64 (one wave per stream), P = 256: 4 KB of LDS, 32 streams resident per CU
//   k <= 256   NT = 64, P = 512: 8 KB, 19 streams per CU
//   k <= 1024  NT = 256, P = 2048: 32 KB, 4 workgroups per CU
//   k <= 4096  NT = 1024, P = 8192: 128 KB, one workgroup per CU
// The smaller P for k <= 64 is deliberate: a buffer that fills sooner gives a fresher T, so fewer
// entries are admitted, and a sort of 256 costs 0.4 of a sort of 512.
//
// Resumed: the state is the caller's: per row r counts[r] entries (h, key) ascending, in the layout
// the stateless launch writes.  Bottom-k by (h, key) over distinct keys is a function of the key set
// alone, so bottomk(A u B) = bottomk(bottomk(A) u B): a row resumed from its stored set and fed the
// next piece ends where one stateless launch over the concatenation ends.  The
// element loop (take_piece), the forms, the grid and the row's epilogue (finish_row) are the
// stateless kernel's own; segstate_kernel adds
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
//
// Byte keys (rsv_distinct_segmented_rows; rows of W = 16..256 bytes, W8 = W / 8 little-endian 64-bit
// words): the same teams, forms, element loop, merge and grid over entries (h, i), i the row's index
// into rows_dev, so the entry stays 16 bytes and every width keeps the LDS budget above.  What an
// entry's second word means is the one thing the loop and the merge take as a parameter (Keys /
// Rows below).  Order and equality go by h first; only two entries with equal h read their rows
// from global memory, word by word as unsigned values, and equal rows are one element whatever their
// indices.  The sort's pad is (INT64_MAX, -1): the index -1 is tested before any row is addressed,
// is above every row and equal to itself.  T's row sits in LDS (s_trow, rewritten by the merge that
// sets T), so admission reads a row only on the lanes with h == T.h.  Hashes are precomputed (8 bytes
// per element; the rows are read on ties and for the output only) or UUID.hashCode of 16-byte rows
// (one 16-byte load per element, two 8-byte loads when rows_dev sits at 8 mod 16).
//
// Byte keys resumed (rsv_distinct_segmented_rows_update / _merge; segrowstate_kernel): the state is
// rows[num_states][k][W8], hashes and counts as the stateless launch writes them.  An entry's second
// word is then a ref to one of two row sources, the launch's input or a slot of the row's own state
// block (RowSrc<true>), the prologue also loads T's row from the block, and the epilogue moves the rows
// in place from the top down (the comment at the kernel).
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

// What an entry's second word is, for the merge (pad, out_of_order, same) and for the element loop
// (load, h_of, admits, set_T).  K5's own: the key itself, sign-extended.
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
    // what the loop refuses is of no interest here (TiedKeys notes it)
    static __device__ __forceinline__ void refuse(int64_t, const Team&) {}
    template <int NT>
    static __device__ __forceinline__ void trimmed(const Ent*, uint32_t, uint32_t, const Team&) {}
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

// Stateless: no prologue, row = stream index, every row is written.
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

    for (int64_t s = blockIdx.x; s < S; s += gridDim.x) {
        int64_t r0, r1;
        java_r0r1(seed0 + (uint64_t)s, r0, r1);
        __syncthreads();  // the previous stream's output reads are done
        if (threadIdx.x == 0) s_cnt = 0;
        __syncthreads();
        Team t{0, 0, kMaxI64, kMaxI64, false};
        const Keys<KeyT, true> src{{}, keys, hashes, hash_kind, r0, r1};
        take_piece<Keys<KeyT, true>, NT>(se, &s_cnt, s_scan, src, offsets[s], offsets[s + 1], k, P, t);
        finish_row<KeyT, NT, true>(se, s_scan, t, k, s, out_keys, out_hashes, counts);
    }
}

// Byte keys, stateless.  The epilogue gathers the m winning rows with lanes over (entry, word), so a
// wave's stores are consecutive words of the row block, and zeroes the rest of it.
template <int NT>
__global__ __launch_bounds__(NT) void segrows_kernel(const uint64_t* __restrict__ rows, const int64_t* __restrict__ hashes,
                                                     const int64_t* __restrict__ offsets, int64_t S, uint32_t W8,
                                                     uint32_t k, uint32_t P, uint64_t seed0,
                                                     uint64_t* __restrict__ out_rows, int64_t* __restrict__ out_hashes,
                                                     int64_t* __restrict__ counts) {
    extern __shared__ __align__(16) unsigned char seg_lds[];
    Ent* const se = (Ent*)seg_lds;
    __shared__ uint32_t s_cnt;
    __shared__ uint32_t s_scan[NT / 64 > 1 ? NT / 64 : 1];
    __shared__ uint64_t s_trow[32];  // kMaxRowWords
    const uint32_t tid = threadIdx.x;
    const bool vec16 = ((uintptr_t)rows & 15) == 0;

    for (int64_t s = blockIdx.x; s < S; s += gridDim.x) {
        int64_t r0, r1;
        java_r0r1(seed0 + (uint64_t)s, r0, r1);
        __syncthreads();  // the previous stream's output reads are done
        if (tid == 0) s_cnt = 0;
        __syncthreads();
        Team t{0, 0, kMaxI64, -1, false};
        const Rows<false, true> src{{{rows, W8}}, hashes, vec16, r0, r1, s_trow};
        take_piece<Rows<false, true>, NT>(se, &s_cnt, s_scan, src, offsets[s], offsets[s + 1], k, P, t);
        if (t.n_tot != t.m) t.m = merge_set<NT>(se, t.n_tot, k, s_scan, src);
        __syncthreads();
        const int64_t ob = s * (int64_t)k;
        for (uint32_t x = tid; x < k * W8; x += NT) {  // k * W8 <= 4096 * 32
            const uint32_t j = x / W8, w = x - j * W8;
            out_rows[ob * W8 + x] = j < t.m ? rows[se[j].key * (int64_t)W8 + w] : 0;
        }
        if (out_hashes)
            for (uint32_t i = tid; i < k; i += NT) out_hashes[ob + i] = i < t.m ? se[i].h : 0;
        if (tid == 0) counts[s] = t.m;
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
                take_piece<Keys<KeyT, false>, NT>(se, &s_cnt, s_scan, Keys<KeyT, false>{{}, in_keys, in_hashes, hash_kind, 0, 0}, pb,
                                                  pb + n, k, P, t);
            }
        } else {
            int64_t r0, r1;
            java_r0r1(seed0 + (uint64_t)r, r0, r1);
            take_piece<Keys<KeyT, true>, NT>(se, &s_cnt, s_scan, Keys<KeyT, true>{{}, in_keys, in_hashes, hash_kind, r0, r1}, lo, hi,
                                             k, P, t);
        }
        if (!t.dirty) continue;  // nothing admitted: the row stands as it is
        finish_row<KeyT, NT, false>(se, s_scan, t, k, r, state_keys, state_hashes, state_counts);
    }
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
        uint64_t* const srow = state_rows + ob * (int64_t)W8;
        const int64_t c0 = state_counts[r];
        const uint32_t m0 = c0 <= 0 ? 0u : (c0 >= (int64_t)k ? k : (uint32_t)c0);
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
                const int64_t pc = part_counts[row];
                const int64_t n = pc <= 0 ? 0 : (pc >= (int64_t)k ? (int64_t)k : pc);
                const int64_t pb = row * (int64_t)k;
                take_piece<Rows<true, false>, NT>(se, &s_cnt, s_scan, src, pb, pb + n, k, P, t);
            }
        } else {
            take_piece<Rows<true, true>, NT>(se, &s_cnt, s_scan, src, lo, hi, k, P, t);
        }
        if (!t.dirty) continue;  // nothing admitted: the row stands as it is
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
    }
}

// ---- Ordered (rsv_distinct_segmented_ordered) ----
// Once RandomValues' heap is full its maximum M is the k-th smallest hash over the distinct keys seen
// and it holds every key with h < M, so its set is the bottom-k by (h, key) unless more than k distinct
// keys have h <= M: only then does the arrival order decide who of the bucket h = M stays.  Two kernels:
// K5 as above, which also finds those streams (tied), and a replay of RandomValues for them alone.
//
// Kernel 1.  TiedKeys is Keys<KeyT, true> that also notes, per lane, whether the team refused an element
// whose h is the current T.h: an element that fails `admits` ((h, key) > T), or an entry a merge trims
// (the entries above the new T among se[k, n): an entry of distinct rank >= k sits at a sorted position
// >= k, which the compaction does not write).  The note is dropped when a merge lowers T.h.  A refused
// element is a distinct key outside the final set, for T only falls; and a distinct key x outside the
// final set with h(x) = M, the final maximum, is refused at its first occurrence at the latest, at a
// time when M <= T.h <= h(x), so T.h = M then and ever after and the note stays.  Hence
//   tied = (m == k && some lane holds a note),
// exactly, whatever M is: below k entries T is the pad and nothing is refused.  This says what "the
// minimum h of everything refused equals se[k-1].h" says (a refused h is never below T.h) at one
// v_cndmask per step: the compare h == T.h is the admission test's own.  Keeping the minimum itself cost
// 7 VALU per step (DESIGN.md 5c.3 has both measurements).
template <typename KeyT>
struct TiedKeys : Keys<KeyT, true> {
    mutable bool at_T;
    __device__ __forceinline__ void refuse(int64_t h, const Team& t) const { at_T |= h == t.Th; }
    __device__ __forceinline__ void set_T(const Ent* se, uint32_t k, Team& t) const {
        const int64_t was = t.Th;
        Keys<KeyT, true>::set_T(se, k, t);
        if (t.Th != was) at_T = false;
    }
    // behind set_T, and before the barrier that lets the appends go on
    template <int NT>
    __device__ __forceinline__ void trimmed(const Ent* se, uint32_t k, uint32_t n, const Team& t) const {
        for (uint32_t i = k + threadIdx.x; i < n; i += NT) {
            const Ent e = se[i];
            at_T |= e.h == t.Th && e.key > t.Tk;
        }
    }
};

template <typename KeyT, int NT>
__global__ __launch_bounds__(NT) void segdistinct_tied_kernel(const KeyT* __restrict__ keys, const int64_t* __restrict__ hashes,
                                                              const int64_t* __restrict__ offsets, int64_t S, uint32_t k,
                                                              uint32_t P, int hash_kind, uint64_t seed0,
                                                              KeyT* __restrict__ out_keys, int64_t* __restrict__ out_hashes,
                                                              int64_t* __restrict__ counts, int32_t* __restrict__ tied) {
    extern __shared__ __align__(16) unsigned char seg_lds[];
    Ent* const se = (Ent*)seg_lds;
    __shared__ uint32_t s_cnt;
    __shared__ uint32_t s_scan[NT / 64 > 1 ? NT / 64 : 1];
    const uint32_t tid = threadIdx.x;

    for (int64_t s = blockIdx.x; s < S; s += gridDim.x) {
        int64_t r0, r1;
        java_r0r1(seed0 + (uint64_t)s, r0, r1);
        __syncthreads();  // the previous stream's output reads are done
        if (tid == 0) s_cnt = 0;
        __syncthreads();
        Team t{0, 0, kMaxI64, kMaxI64, false};
        const TiedKeys<KeyT> src{{{}, keys, hashes, hash_kind, r0, r1}, false};
        take_piece<TiedKeys<KeyT>, NT>(se, &s_cnt, s_scan, src, offsets[s], offsets[s + 1], k, P, t);
        if (t.n_tot != t.m) {  // the last merge, here for what it trims
            const uint32_t n = t.n_tot;
            t.m = merge_set<NT>(se, n, k, s_scan, KeyOrd{});
            if (t.m == k) {
                src.set_T(se, k, t);
                src.template trimmed<NT>(se, k, n, t);
            }
            t.n_tot = t.m;
        }
        const int noted = __syncthreads_or(src.at_T);
        if (tid == 0) tied[s] = t.m == k && noted;
        finish_row<KeyT, NT, true>(se, s_scan, t, k, s, out_keys, out_hashes, counts);
    }
}

// lane l's value as a scalar (l uniform): two v_readlane, no LDS round trip
__device__ __forceinline__ int64_t read_lane(int64_t v, int l) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, l);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)((uint64_t)v >> 32), l);
    return (int64_t)(((uint64_t)hi << 32) | lo);
}

// RandomValues.sample over the elements [lo, hi) of src in arrival order, by one wave, on the heap se[0, n) with
// maxh its root's h (INT64_MIN while it is empty): what the comment at segdistinct_replay_kernel says of its
// walk.  The one piece of device code both ordered kernels run per stream (segdistinct_replay_kernel from an
// empty heap, segdistinct_heap_kernel from the caller's); with NOTE it returns whether anything was admitted (the
// replay has no use for that).  The heap is left as the last admission wrote it, behind a barrier.
template <bool NOTE, typename KeyT>
__device__ __forceinline__ bool replay_walk(Ent* const se, const Keys<KeyT, true> src, int64_t lo, int64_t hi, uint32_t k,
                                            uint32_t& n_io, int64_t& maxh_io) {
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
                const int64_t ck = read_lane(key[u], l), ch = read_lane(h, l);
                // elements.contains: n / 64 reads per lane, eight in flight
                bool found = false;
                const uint32_t full = n >> 6;
                uint32_t r = 0;
                for (; r + 8 <= full; r += 8) {
                    int64_t mk[8];
#pragma unroll
                    for (int x = 0; x < 8; ++x) mk[x] = se[(r + x) * 64 + lane].key;
#pragma unroll
                    for (int x = 0; x < 8; ++x) found |= mk[x] == ck;
                }
                for (uint32_t j = r * 64 + lane; j < n; j += 64) found |= se[j].key == ck;
                if (__ballot(found)) continue;  // a member
                if (lane == 0) {
                    uint32_t nn = n;
                    if (nn == k) {  // dequeue: the root leaves
                        const Ent last = se[nn - 1];
                        --nn;
                        if (nn) {
                            uint32_t q = 1;
                            while (2 * q <= nn) {
                                uint32_t c = 2 * q;
                                if (c + 1 <= nn && se[c - 1].h < se[c].h) ++c;
                                if (last.h >= se[c - 1].h) break;
                                se[q - 1] = se[c - 1];
                                q = c;
                            }
                            se[q - 1] = last;
                        }
                    }
                    uint32_t q = nn + 1;  // addOne
                    while (q > 1 && se[(q >> 1) - 1].h < ch) {
                        se[q - 1] = se[(q >> 1) - 1];
                        q >>= 1;
                    }
                    se[q - 1] = Ent{ch, ck};
                }
                if (n < k) ++n;
                if constexpr (NOTE) admitted = true;
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

// Kernel 2: RandomValues (Sampler.scala:394-409) over the tied streams, one wave per stream.  A wave
// reads the tied words of W consecutive streams at once and replays those that are set, one after the
// other.  The heap is rsv_host_values.h's, 1-indexed in se[0, k) (entry j at se[j - 1]): scala 2.13
// mutable.PriorityQueue's addOne/fixUp (sift up while parent < child) and dequeue/fixDown (last entry to
// the root, sink to the larger child, left on ties, stop when parent >= child), ordered by h alone.
// The stream is walked in arrival order, 64 elements a step (kU steps loaded ahead).  Of a step, the
// first lane whose element passes the current test (size < k, or h < maxHash) is taken (read_lane), its
// key looked up among the heap's keys by all lanes (elements.contains), and admitted by lane 0 if absent; then the
// lanes behind it are tested again, against the new maxHash.  maxHash never rises once the heap is full
// and below that every element passes, so a lane that failed once fails for good and the lanes taken are
// in arrival order.  The barriers order lane 0's heap writes and the other lanes' reads; with one wave
// per workgroup they cost no wait.  At the end the k entries are sorted by (h, key) and written over the
// row kernel 1 left; count and tied stay.
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
    const int64_t groups = (S + W - 1) / W;

    for (int64_t g = blockIdx.x; g < groups; g += gridDim.x) {
        const int64_t sl = g * W + lane;
        uint64_t todo = __ballot(lane < W && sl < S && tied[sl] != 0);
        while (todo) {
            const int64_t s = g * W + (__ffsll((long long)todo) - 1);
            todo &= todo - 1;
            const int64_t lo = offsets[s], hi = offsets[s + 1];
            int64_t r0, r1;
            java_r0r1(seed0 + (uint64_t)s, r0, r1);
            const Keys<KeyT, true> src{{}, keys, hashes, hash_kind, r0, r1};
            uint32_t n = 0;              // heap size (uniform)
            int64_t maxh = INT64_MIN;    // the root's h once anything is in
            __syncthreads();             // the previous stream's output reads are done
            replay_walk<false>(se, src, lo, hi, k, n, maxh);
            const uint32_t m = merge_set<64>(se, n, k, s_scan, KeyOrd{});
            __syncthreads();
            const int64_t ob = s * (int64_t)k;
            for (uint32_t i = lane; i < m; i += 64) {
                const Ent e = se[i];
                out_keys[ob + i] = (KeyT)e.key;
                if (out_hashes) out_hashes[ob + i] = e.h;
            }
        }
    }
}

// ---- Ordered, resumed (rsv_distinct_segmented_ordered_update) ----
// RandomValues' whole state is the queue's array, a set of the array's keys, and maxHash, which at every moment
// is the root's h: below k entries the running maximum, which a max-heap keeps at its root, at k entries
// samples.head._2.  addOne/fixUp and dequeue/fixDown are functions of the array alone.  So the row's count and
// its entries (h, key) in array order -- entry j of the 1-indexed queue in slot j - 1 -- are the sampler, and
// replay_walk from them is the reference going on.  A row kept sorted is a heap too, but another one: its later
// dequeues move other entries, and the bucket at the maximum hash ends with other members.
// One wave per segment, segments grid-stride; row r = ids[b] (or b), seeded seed0 + r.
//   prologue   n = clamp(counts[r], 0, k); the row's pairs into se[0, n) as they lie; maxh = se[0].h when n > 0.
//   walk       replay_walk, segdistinct_replay_kernel's own.
//   epilogue   only if something was admitted: se[0, n) back as they lie, zeros up to k, the count.  No sort.
// Nothing read from the state or from the ids indexes memory unclamped, and the walk addresses se below
// max(n, 1) <= k only (parents and children of positions <= n), whatever the entries hold: a row that is no heap
// gives an unspecified set at the same addresses.
template <typename KeyT>
__global__ __launch_bounds__(64) void segdistinct_heap_kernel(const KeyT* __restrict__ keys, const int64_t* __restrict__ hashes,
                                                              const int64_t* __restrict__ offsets,
                                                              const int64_t* __restrict__ ids, int64_t num_segments,
                                                              int64_t num_states, uint32_t k, int hash_kind, uint64_t seed0,
                                                              KeyT* state_keys, int64_t* state_hashes, int64_t* state_counts) {
    extern __shared__ __align__(16) unsigned char seg_lds[];
    Ent* const se = (Ent*)seg_lds;
    const uint32_t lane = threadIdx.x;

    for (int64_t b = blockIdx.x; b < num_segments; b += gridDim.x) {
        // everything that decides the control flow below is uniform over the wave
        int64_t r = b;
        if (ids) r = ids[b];
        if (r < 0 || r >= num_states) continue;  // an id outside the state: no row is addressed
        const int64_t lo = offsets[b], hi = offsets[b + 1];
        if (hi <= lo) continue;  // an empty segment leaves its row as it is
        const int64_t ob = r * (int64_t)k;
        const int64_t c0 = state_counts[r];
        uint32_t n = c0 <= 0 ? 0u : (c0 >= (int64_t)k ? k : (uint32_t)c0);
        __syncthreads();  // the previous row's output reads are done
        for (uint32_t i = lane; i < n; i += 64) se[i] = Ent{state_hashes[ob + i], (int64_t)state_keys[ob + i]};
        __syncthreads();
        int64_t maxh = INT64_MIN;
        if (n) maxh = se[0].h;
        int64_t r0, r1;
        java_r0r1(seed0 + (uint64_t)r, r0, r1);
        const Keys<KeyT, true> src{{}, keys, hashes, hash_kind, r0, r1};
        if (!replay_walk<true>(se, src, lo, hi, k, n, maxh)) continue;  // nothing admitted: the row stands as it is
        for (uint32_t i = lane; i < k; i += 64) {
            const Ent e = i < n ? se[i] : Ent{0, 0};
            state_keys[ob + i] = (KeyT)e.key;
            state_hashes[ob + i] = e.h;
        }
        if (lane == 0) state_counts[r] = n;
    }
}

// ---- Ordered over byte keys (rsv_distinct_segmented_rows_ordered) ----
// The argument above with "key" read as "row": once the heap is full its maximum M is the k-th smallest
// hash over the distinct rows seen and it holds every row with h < M, so its set is the bottom-k by
// (h, row words) unless more than k distinct rows have h <= M.  Kernel 1 is segrows_kernel with TiedRows,
// which is Rows<false, true> that also notes, per lane, whether the team refused an element whose h is the
// current T.h.  A lane that fails `admits` at h = T.h holds a row strictly above T's row (an equal row and an
// equal ref pass), so it is a distinct row outside the current set, and outside the final one, for T only
// falls.  A merge trims the entries above the new T among se[k, n): the compaction writes below k only, so
// se[k, n) is what the sort left there, and an entry of distinct rank >= k sits at a sorted position >= k.
// Of those positions the ones below T's own hold repeats of members, which may share T.h with a row below
// T's: the note wants (h == T.h and row > T's row), not "row differs".  Equal refs are settled before any row
// is addressed.  The note is dropped when a merge lowers T.h.  A distinct row x outside the final set with
// h(x) = M is refused at its first occurrence at the latest, or trimmed, at a time when M <= T.h <= h(x), so
// T.h = M then and ever after and the note stays.  Hence tied = (m == k && some lane holds a note), exactly,
// whatever M is: below k entries T is the pad (INT64_MAX, -1), which admits everything.
// Rows::set_T writes s_trow from the threads below W8 and no barrier stands between it and trimmed, so
// trimmed reads T's row where set_T read it: at(T.Tk) in global memory.
struct TiedRows : Rows<false, true> {
    mutable bool at_T;
    __device__ __forceinline__ void refuse(int64_t h, const Team& t) const { at_T |= h == t.Th; }
    __device__ __forceinline__ void set_T(const Ent* se, uint32_t k, Team& t) const {
        const int64_t was = t.Th;
        Rows<false, true>::set_T(se, k, t);
        if (t.Th != was) at_T = false;
    }
    // behind set_T, and before the barrier that lets the appends go on
    template <int NT>
    __device__ __forceinline__ void trimmed(const Ent* se, uint32_t k, uint32_t n, const Team& t) const {
        for (uint32_t i = k + threadIdx.x; i < n; i += NT) {
            const Ent e = se[i];
            if (e.h != t.Th || e.key == t.Tk || e.key < 0 || t.Tk < 0) continue;
            const uint64_t* const r = this->at(e.key);
            const uint64_t* const tr = this->at(t.Tk);
            for (uint32_t w = 0; w < this->W8; ++w) {
                const uint64_t x = r[w], y = tr[w];
                if (x != y) {
                    at_T |= x > y;
                    break;
                }
            }
        }
    }
};

template <int NT>
__global__ __launch_bounds__(NT) void segrows_tied_kernel(const uint64_t* __restrict__ rows, const int64_t* __restrict__ hashes,
                                                          const int64_t* __restrict__ offsets, int64_t S, uint32_t W8,
                                                          uint32_t k, uint32_t P, uint64_t seed0,
                                                          uint64_t* __restrict__ out_rows, int64_t* __restrict__ out_hashes,
                                                          int64_t* __restrict__ counts, int32_t* __restrict__ tied) {
    extern __shared__ __align__(16) unsigned char seg_lds[];
    Ent* const se = (Ent*)seg_lds;
    __shared__ uint32_t s_cnt;
    __shared__ uint32_t s_scan[NT / 64 > 1 ? NT / 64 : 1];
    __shared__ uint64_t s_trow[32];  // kMaxRowWords
    const uint32_t tid = threadIdx.x;
    const bool vec16 = ((uintptr_t)rows & 15) == 0;

    for (int64_t s = blockIdx.x; s < S; s += gridDim.x) {
        int64_t r0, r1;
        java_r0r1(seed0 + (uint64_t)s, r0, r1);
        __syncthreads();  // the previous stream's output reads are done
        if (tid == 0) s_cnt = 0;
        __syncthreads();
        Team t{0, 0, kMaxI64, -1, false};
        const TiedRows src{{{{rows, W8}}, hashes, vec16, r0, r1, s_trow}, false};
        take_piece<TiedRows, NT>(se, &s_cnt, s_scan, src, offsets[s], offsets[s + 1], k, P, t);
        if (t.n_tot != t.m) {  // the last merge, here also for what it trims
            const uint32_t n = t.n_tot;
            t.m = merge_set<NT>(se, n, k, s_scan, src);
            if (t.m == k) {
                src.set_T(se, k, t);
                src.template trimmed<NT>(se, k, n, t);
            }
            t.n_tot = t.m;
        }
        const int noted = __syncthreads_or(src.at_T);
        if (tid == 0) tied[s] = t.m == k && noted;
        const int64_t ob = s * (int64_t)k;
        for (uint32_t x = tid; x < k * W8; x += NT) {  // k * W8 <= 4096 * 32
            const uint32_t j = x / W8, w = x - j * W8;
            out_rows[ob * W8 + x] = j < t.m ? rows[se[j].key * (int64_t)W8 + w] : 0;
        }
        if (out_hashes)
            for (uint32_t i = tid; i < k; i += NT) out_hashes[ob + i] = i < t.m ? se[i].h : 0;
        if (tid == 0) counts[s] = t.m;
    }
}

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

// RandomValues.sample over the rows [lo, hi) of src's input in arrival order, by one wave, on the heap se[0, n)
// with maxh its root's h (INT64_MIN while it is empty): replay_walk for byte keys, what the comment at
// segrows_replay_kernel says of its walk.  The one piece of device code both ordered kernels over rows run per
// stream (segrows_replay_kernel from an empty heap, segrows_heap_kernel from the caller's); it returns whether
// anything was admitted.  With STATE an admission takes its slot by the rule: the heap's size when it grows, the
// evicted root's slot when it is full.  The heap is left as the last admission wrote it, behind a barrier.
template <bool STATE>
__device__ __forceinline__ bool rows_replay_walk(Ent* const se, const Rows<STATE, true> src, int64_t lo, int64_t hi,
                                                 uint32_t k, uint32_t& n_io, int64_t& maxh_io) {
    uint32_t n = n_io;
    int64_t maxh = maxh_io;
    const uint32_t lane = threadIdx.x;
    const uint32_t W8 = src.W8;
    bool admitted = false;
    // equality of a heap entry's row and row c of the input (W8 >= 2): the first two words of both in flight
    // together, so a UUID costs one round trip, not one per word
    const auto same_row = [&](int64_t ref, int64_t c) {
        const uint64_t* const ra = row_of<STATE>(src, ref);
        const uint64_t* const rb = src.rows + c * (int64_t)W8;
        if (ra == rb) return true;
        const uint64_t a0 = ra[0], a1 = ra[1], b0 = rb[0], b1 = rb[1];
        if (a0 != b0 || a1 != b1) return false;
        for (uint32_t w = 2; w < W8; ++w)
            if (ra[w] != rb[w]) return false;
        return true;
    };
    for (int64_t base = lo; base < hi; base += 64 * kU) {
        int64_t ref[kU], hv[kU];
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            const int64_t i = base + (int64_t)u * 64 + lane;
            ref[u] = 0;
            hv[u] = 0;
            if (i < hi) src.load(i, ref[u], hv[u]);
        }
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            const int64_t i = base + (int64_t)u * 64 + lane;
            if (base + (int64_t)u * 64 >= hi) break;  // uniform
            const int64_t h = src.h_of(ref[u], hv[u]);
            bool pend = i < hi;
            for (;;) {
                const uint64_t mask = __ballot(pend && (n < k || h < maxh));
                if (!mask) break;
                const int l = __ffsll((long long)mask) - 1;
                if ((int)lane == l) pend = false;
                Ent c{read_lane(h, l), base + (int64_t)u * 64 + l};  // the candidate: (h, its row's index)
                bool found = false;
                const uint32_t full = n >> 6;
                uint32_t r = 0;
                for (; r + 8 <= full; r += 8) {
                    int64_t mh[8];
#pragma unroll
                    for (int x = 0; x < 8; ++x) mh[x] = se[(r + x) * 64 + lane].h;
#pragma unroll
                    for (int x = 0; x < 8; ++x)
                        if (mh[x] == c.h) found |= same_row(se[(r + x) * 64 + lane].key, c.key);
                }
                for (uint32_t j = r * 64 + lane; j < n; j += 64)
                    if (se[j].h == c.h) found |= same_row(se[j].key, c.key);
                if (__ballot(found)) continue;  // a member
                if (lane == 0) {
                    uint32_t nn = n;
                    if constexpr (STATE) c.key |= (int64_t)(nn == k ? slot_of(se[0].key, k) : nn) << kSlotShift;
                    if (nn == k) {  // dequeue: the root leaves
                        const Ent last = se[nn - 1];
                        --nn;
                        if (nn) {
                            uint32_t q = 1;
                            while (2 * q <= nn) {
                                uint32_t ch = 2 * q;
                                if (ch + 1 <= nn && se[ch - 1].h < se[ch].h) ++ch;
                                if (last.h >= se[ch - 1].h) break;
                                se[q - 1] = se[ch - 1];
                                q = ch;
                            }
                            se[q - 1] = last;
                        }
                    }
                    uint32_t q = nn + 1;  // addOne
                    while (q > 1 && se[(q >> 1) - 1].h < c.h) {
                        se[q - 1] = se[(q >> 1) - 1];
                        q >>= 1;
                    }
                    se[q - 1] = c;
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

// Kernel 2 over byte keys: segdistinct_replay_kernel with entries (h, ref), ref the row's index into rows:
// the same grouping of tied words, heap, walk and serialised admission; no row is staged in LDS.
// elements.contains: equal rows carry equal hashes (the caller's contract), so a member can only be an
// entry whose h is the candidate's.  All lanes scan the heap's h, eight 8-byte reads in flight; only an
// entry with the candidate's h goes further: its ref is read, an equal ref is the candidate's own row,
// otherwise the two rows are read from global memory and compared word by word.  At the end the entries are sorted by (h, row words)
// and the m rows gathered over what kernel 1 wrote, lanes over (entry, word); count and tied stay.
__global__ __launch_bounds__(64) void segrows_replay_kernel(const uint64_t* __restrict__ rows, const int64_t* __restrict__ hashes,
                                                            const int64_t* __restrict__ offsets, int64_t S, uint32_t W8,
                                                            uint32_t k, uint32_t W, uint64_t seed0,
                                                            uint64_t* __restrict__ out_rows, int64_t* __restrict__ out_hashes,
                                                            const int32_t* __restrict__ tied) {
    extern __shared__ __align__(16) unsigned char seg_lds[];
    Ent* const se = (Ent*)seg_lds;
    __shared__ uint32_t s_scan[1];
    const uint32_t lane = threadIdx.x;
    const int64_t groups = (S + W - 1) / W;
    const bool vec16 = ((uintptr_t)rows & 15) == 0;

    for (int64_t g = blockIdx.x; g < groups; g += gridDim.x) {
        const int64_t sl = g * W + lane;
        uint64_t todo = __ballot(lane < W && sl < S && tied[sl] != 0);
        while (todo) {
            const int64_t s = g * W + (__ffsll((long long)todo) - 1);
            todo &= todo - 1;
            const int64_t lo = offsets[s], hi = offsets[s + 1];
            int64_t r0, r1;
            java_r0r1(seed0 + (uint64_t)s, r0, r1);
            const Rows<false, true> src{{{rows, W8}}, hashes, vec16, r0, r1, nullptr};  // no T here: admits is not used
            const RowOrd<false>& ord = src;
            uint32_t n = 0;            // heap size (uniform)
            int64_t maxh = INT64_MIN;  // the root's h once anything is in
            __syncthreads();           // the previous stream's output reads are done
            rows_replay_walk<false>(se, src, lo, hi, k, n, maxh);
            const uint32_t m = merge_set<64>(se, n, k, s_scan, ord);
            __syncthreads();
            const int64_t ob = s * (int64_t)k;
            for (uint32_t x = lane; x < m * W8; x += 64) {  // m * W8 <= 4096 * 32
                const uint32_t j = x / W8, w = x - j * W8;
                out_rows[ob * W8 + x] = rows[se[j].key * (int64_t)W8 + w];
            }
            if (out_hashes)
                for (uint32_t i = lane; i < m; i += 64) out_hashes[ob + i] = se[i].h;
        }
    }
}

// ---- Ordered over byte keys, resumed (rsv_distinct_segmented_rows_ordered_update) ----
// segdistinct_heap_kernel's argument does not ask what a key is: the queue's array in array order is the sampler.
// What the array holds here is what it holds on the JVM, references: the row block state_rows[r] is storage whose
// order means nothing, hashes[r][p] and slots[r][p] are position p of the array, and the row of that entry lies in
// slot slots[r][p] of the block.  An admission that grows the heap from n to n + 1 takes slot n, one into a full
// heap takes the slot of the root it evicts: below k the slots in use are {0..n-1}, at k a permutation, and no
// surviving row ever moves.
// One wave per segment, segments grid-stride; row r = ids[b] (or b), seeded seed0 + r.
//   prologue   n = clamp(counts[r], 0, k); entry p into se[p] as (hashes[p], kStateRef | slot), the slot clamped
//              below k; maxh = se[0].h when n > 0.  No row is read.
//   walk       rows_replay_walk, segrows_replay_kernel's own; rows are read from the input or from a state slot
//              only for entries with the candidate's hash.
//   epilogue   only if something was admitted: hashes and slots of se[0, n) as they lie and zeros up to k, then for
//              every entry that refers to the input its row into its slot, lanes over (entry, word), then the count.
//              No sort and no staged move: the rows read are the input's, and the slots written are the ones no
//              surviving state entry names (a grown heap's new slots, or slots of evicted roots), so nothing is
//              read after it was overwritten and no member's row is touched.  Slots [n, k) of the block are zeroed
//              when the row was empty before or its count had to be clamped (the caller's bytes), else they are
//              the kernel's own zeros already.
// Nothing read from the state or from the ids indexes memory unclamped: the count into [0, k], every slot below k,
// an id outside [0, num_states) skips the segment.  Repeated or out-of-range slots, a row that is no heap and a
// wrong count give an unspecified set at the same addresses.
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

    for (int64_t b = blockIdx.x; b < num_segments; b += gridDim.x) {
        // everything that decides the control flow below is uniform over the wave
        int64_t r = b;
        if (ids) r = ids[b];
        if (r < 0 || r >= num_states) continue;  // an id outside the state: no row is addressed
        const int64_t lo = offsets[b], hi = offsets[b + 1];
        if (hi <= lo) continue;  // an empty segment leaves its row as it is
        const int64_t ob = r * (int64_t)k;
        uint64_t* const srow = state_rows + ob * (int64_t)W8;
        const int64_t c0 = state_counts[r];
        const uint32_t n0 = c0 <= 0 ? 0u : (c0 >= (int64_t)k ? k : (uint32_t)c0);
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
        if (!rows_replay_walk<true>(se, src, lo, hi, k, n, maxh)) continue;  // nothing admitted: the row stands as it is
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
    }
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

// The replay of the tied streams: one wave and pow2ceil(k) entries (the heap, and the pads of its final sort)
// per stream in flight.  A wave looks at W consecutive tied words per step: 64 when there are streams enough to
// fill the grid that way, fewer when not, so that few streams still spread over the CUs.
struct ReplayPlan {
    size_t lds;
    uint32_t W;
    unsigned grid;
};

// (the part both ordered launches share: the LDS of one wave's heap, the attribute above 64 KB, and `cap`, the
// waves the 256 CUs hold at once, four times over)
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

hipError_t plan_replay(const void* kernel, int64_t S, uint32_t k, ReplayPlan& p) {
    uint64_t cap;
    if (const hipError_t a = plan_heap_waves(kernel, k, p.lds, cap); a != hipSuccess) return a;
    p.W = 1;
    while (p.W < 64 && (uint64_t)S / (2 * p.W) >= cap) p.W <<= 1;
    p.grid = (unsigned)std::min<uint64_t>(((uint64_t)S + p.W - 1) / p.W, cap);
    return hipSuccess;
}

}  // namespace

hipError_t launch_segdistinct(const void* keys, int key_width, const int64_t* hashes, const int64_t* offsets, int64_t S,
                              uint32_t k, int hash_kind, uint64_t seed0, void* out_keys, int64_t* out_hashes,
                              int64_t* counts, hipStream_t st) {
    if (S <= 0) return hipSuccess;
    return with_form(key_width, k, [&](auto key, auto nt, uint32_t P) {
        using KeyT = decltype(key);
        constexpr int NT = decltype(nt)::value;
        return launch_teams(segdistinct_kernel<KeyT, NT>, NT, S, P, st, (const KeyT*)keys, hashes, offsets, S, k, P,
                            hash_kind, seed0, (KeyT*)out_keys, out_hashes, counts);
    });
}

hipError_t launch_segdistinct_ordered(const void* keys, int key_width, const int64_t* hashes, const int64_t* offsets,
                                      int64_t S, uint32_t k, int hash_kind, uint64_t seed0, void* out_keys,
                                      int64_t* out_hashes, int64_t* counts, int32_t* tied, hipStream_t st) {
    if (S <= 0) return hipSuccess;
    return with_form(key_width, k, [&](auto key, auto nt, uint32_t P) {
        using KeyT = decltype(key);
        constexpr int NT = decltype(nt)::value;
        const hipError_t e = launch_teams(segdistinct_tied_kernel<KeyT, NT>, NT, S, P, st, (const KeyT*)keys, hashes, offsets,
                                          S, k, P, hash_kind, seed0, (KeyT*)out_keys, out_hashes, counts, tied);
        if (e != hipSuccess) return e;
        ReplayPlan rp;
        auto* const replay = segdistinct_replay_kernel<KeyT>;
        if (const hipError_t a = plan_replay((const void*)replay, S, k, rp); a != hipSuccess) return a;
        hipLaunchKernelGGL(replay, dim3(rp.grid), dim3(64), rp.lds, st, (const KeyT*)keys, hashes, offsets, S, k, rp.W, hash_kind,
                           seed0, (KeyT*)out_keys, out_hashes, (const int32_t*)tied);
        return hipGetLastError();
    });
}

hipError_t launch_segdistinct_rows(const void* rows, int key_width, const int64_t* hashes, const int64_t* offsets,
                                   int64_t S, uint32_t k, uint64_t seed0, void* out_rows, int64_t* out_hashes,
                                   int64_t* counts, hipStream_t st) {
    if (S <= 0) return hipSuccess;
    auto f = [&](int64_t, auto nt, uint32_t P) {
        constexpr int NT = decltype(nt)::value;
        return launch_teams(segrows_kernel<NT>, NT, S, P, st, (const uint64_t*)rows, hashes, offsets, S,
                            (uint32_t)key_width / 8, k, P, seed0, (uint64_t*)out_rows, out_hashes, counts);
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
        const hipError_t e = launch_teams(segrows_tied_kernel<NT>, NT, S, P, st, (const uint64_t*)rows, hashes, offsets, S, W8,
                                          k, P, seed0, (uint64_t*)out_rows, out_hashes, counts, tied);
        if (e != hipSuccess) return e;
        ReplayPlan rp;
        if (const hipError_t a = plan_replay((const void*)segrows_replay_kernel, S, k, rp); a != hipSuccess) return a;
        hipLaunchKernelGGL(segrows_replay_kernel, dim3(rp.grid), dim3(64), rp.lds, st, (const uint64_t*)rows, hashes, offsets,
                           S, W8, k, rp.W, seed0, (uint64_t*)out_rows, out_hashes, (const int32_t*)tied);
        return hipGetLastError();
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

// The resumed ordered launch: plan_replay's LDS and grid with one segment per wave (W = 1: there is no tied word
// to read, every segment is walked).
hipError_t launch_segdistinct_ordered_update(const void* keys, int key_width, const int64_t* hashes, const int64_t* offsets,
                                             const int64_t* stream_ids, int64_t num_segments, int64_t num_states,
                                             uint32_t k, int hash_kind, uint64_t seed0, void* state_keys,
                                             int64_t* state_hashes, int64_t* state_counts, hipStream_t st) {
    if (num_segments <= 0 || num_states <= 0) return hipSuccess;
    auto go = [&](auto key) {
        using KeyT = decltype(key);
        auto* const kernel = segdistinct_heap_kernel<KeyT>;
        size_t lds;
        uint64_t cap;
        if (const hipError_t a = plan_heap_waves((const void*)kernel, k, lds, cap); a != hipSuccess) return a;
        const unsigned grid = (unsigned)std::min<uint64_t>((uint64_t)num_segments, cap);
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(64), lds, st, (const KeyT*)keys, hashes, offsets, stream_ids,
                           num_segments, num_states, k, hash_kind, seed0, (KeyT*)state_keys, state_hashes, state_counts);
        return hipGetLastError();
    };
    return key_width == 8 ? go(int64_t{}) : go(int32_t{});
}

// The resumed ordered launch over byte keys: launch_segdistinct_ordered_update's plan (one segment per wave, the
// heap's 16-byte entries carry their slots, so the LDS is the same).
hipError_t launch_segdistinct_rows_ordered_update(const void* rows, int key_width, const int64_t* hashes,
                                                  const int64_t* offsets, const int64_t* stream_ids, int64_t num_segments,
                                                  int64_t num_states, uint32_t k, uint64_t seed0, void* state_rows,
                                                  int64_t* state_hashes, int32_t* state_slots, int64_t* state_counts,
                                                  hipStream_t st) {
    if (num_segments <= 0 || num_states <= 0) return hipSuccess;
    size_t lds;
    uint64_t cap;
    if (const hipError_t a = plan_heap_waves((const void*)segrows_heap_kernel, k, lds, cap); a != hipSuccess) return a;
    const unsigned grid = (unsigned)std::min<uint64_t>((uint64_t)num_segments, cap);
    hipLaunchKernelGGL(segrows_heap_kernel, dim3(grid), dim3(64), lds, st, (const uint64_t*)rows, hashes, offsets,
                       stream_ids, num_segments, num_states, (uint32_t)key_width / 8, k, seed0, (uint64_t*)state_rows,
                       state_hashes, state_slots, state_counts);
    return hipGetLastError();
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
