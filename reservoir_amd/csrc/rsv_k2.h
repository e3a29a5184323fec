// rsv_k2.h -- the K2 segmented kernel (rsv_segmented.hip launches it).  See rsv_segmented.hip for
// the design.  (The cost-probe variants of earlier rounds live in tools/k2_dev_variants.h.)
#pragma once
#include <algorithm>
#include <type_traits>

#include "rsv_device.h"

namespace rsv {
namespace k2 {

constexpr int kWaves = 4;          // waves per workgroup
constexpr uint32_t kRing = 4;      // level-0 iterations whose block words stay addressable
constexpr uint32_t kQCap = 512;    // FIFO entries (an iteration that would overflow takes ballot rounds)
constexpr uint32_t kStashBytes = kRing * 64 * 16;
constexpr uint32_t kQueueBytes = kQCap * 2;
constexpr uint32_t kLut = 1024;    // blocks (16 indices each) whose threshold T is tabulated per workgroup
constexpr uint32_t kLutBytes = kLut * 2;
constexpr int64_t kSmallLen = 1ll << 27;  // streams shorter than this use 32-bit index arithmetic

// bytes of dynamic LDS per workgroup: T table + per wave (stash | FIFO | k-slot table)
__host__ __device__ inline size_t lds_bytes(uint32_t k) {
    return kLutBytes + (size_t)kWaves * (kStashBytes + kQueueBytes + (size_t)k * 8);
}

constexpr size_t kLdsMax = 160 * 1024;  // one workgroup's LDS

// T = ceil(256 k / (i0 + 1)), the block threshold of the dense region (T > 255: every byte is a
// candidate -> 256); 0 marks the sparse region (i0 + 1 >= 256 k: only b == 0 can hit)
__device__ __forceinline__ uint32_t block_threshold(uint64_t i0, uint64_t dense_lim) {
    if (i0 + 1 >= dense_lim) return 0;
    const uint64_t T = (dense_lim + i0) / (i0 + 1);
    return T > 255 ? 256u : (uint32_t)T;
}

// b_e < T for the 16 bytes of a block (1 <= T <= 255), bit-sliced: the borrow out of (T - 1) - b,
// planes LSB first, one v_bitop3 per plane (borrow' = bit p of T-1 ? plane & borrow : plane | borrow;
// table 0xD4 in the A = 0xF0, B = 0xCC, C = 0xAA convention).  The high 16 bits are don't-care.
__device__ __forceinline__ uint32_t lt_mask16_borrow(const u32x4& w, uint32_t T) {
    const uint32_t M = T - 1;
    const uint32_t words[4] = {w.x, w.y, w.z, w.w};
    uint32_t br = 0;
#pragma unroll
    for (int p = 0; p < 8; ++p) {
        const uint32_t plane = (p & 1) ? (words[p >> 1] >> 16) : words[p >> 1];
        const uint32_t mm = (uint32_t)((int32_t)(M << (31 - p)) >> 31);  // all ones iff bit p of T-1
        br = __builtin_amdgcn_bitop3_b32(plane, br, mm, 0xD4);
    }
    return ~br & 0xFFFFu;
}

// the level-0 bytes of indices e and e + 1 of a block (e even), as level0_byte twice
__device__ __forceinline__ void level0_byte_pair(const u32x4& w, uint32_t e, uint32_t& b0, uint32_t& b1) {
    // bits e, e+1 of the planes 2q (low half) and 2q+1 (high half) of word q, at 2q, 2q+1 / 16+2q, 17+2q
    const uint32_t u = ((w.x >> e) & 0x30003u) | (((w.y >> e) & 0x30003u) << 2) |
                       (((w.z >> e) & 0x30003u) << 4) | (((w.w >> e) & 0x30003u) << 6);
    b0 = (u & 0x55u) | ((u >> 15) & 0xAAu);
    b1 = ((u >> 1) & 0x55u) | ((u >> 16) & 0xAAu);
}

__device__ __forceinline__ uint32_t mask_for(const u32x4& w, uint32_t T) {
    return T == 0 ? zero_byte_mask16(w) : T > 255 ? 0xFFFFu : lt_mask16_borrow(w, T);
}

// mask_for for T <= 16 (T = 0, the sparse region's b == 0, is T = 1): b < T needs planes 4..7 zero
// (the high words' OR) and the low four planes below T -- 4 borrow steps instead of 8
__device__ __forceinline__ uint32_t mask_for_small(const u32x4& w, uint32_t T) {
    const uint32_t M = (T ? T : 1u) - 1u;
    const uint32_t words[2] = {w.x, w.y};
    uint32_t br = 0;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const uint32_t plane = (p & 1) ? (words[p >> 1] >> 16) : words[p >> 1];
        const uint32_t mm = (uint32_t)((int32_t)(M << (31 - p)) >> 31);
        br = __builtin_amdgcn_bitop3_b32(plane, br, mm, 0xD4);
    }
    const uint32_t hi = w.z | w.w;
    return ~(br | hi | (hi >> 16)) & 0xFFFFu;
}

__device__ __forceinline__ uint32_t clip16(uint64_t i0, uint64_t lo, uint64_t hi) {
    uint32_t m = 0xFFFFu;
    if (i0 < lo) m = (lo - i0 >= 16) ? 0u : ((0xFFFFu << (uint32_t)(lo - i0)) & 0xFFFFu);
    if (i0 + 16 > hi) m &= (hi <= i0) ? 0u : (0xFFFFu >> (uint32_t)(16 - (hi - i0)));
    return m;
}

// inclusive prefix sum over the wave (DPP: row shifts within 16-lane rows, then row broadcasts)
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t x) {
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x111, 0xF, 0xF, false);  // row_shr:1
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x112, 0xF, 0xF, false);  // row_shr:2
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x114, 0xF, 0xF, false);  // row_shr:4
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x118, 0xF, 0xF, false);  // row_shr:8
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x142, 0xA, 0xF, false);  // row_bcast:15
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x143, 0xC, 0xF, false);  // row_bcast:31
    return x;
}

// j = floor(((b << 56) | (L >> 8)) (i + 1) / 2^64), L = Lh:Ll
__device__ __forceinline__ uint64_t draw_j(uint32_t b, uint32_t Lh, uint32_t Ll, uint64_t i1, bool small) {
    const uint32_t Uh = __builtin_amdgcn_alignbit(b, Lh, 8), Ul = __builtin_amdgcn_alignbit(Lh, Ll, 8);
    if (small) {  // i + 1 < 2^32: a 64 x 32 product, the high word of its high half
        const uint32_t x = (uint32_t)i1;
        return (uint32_t)(((uint64_t)Uh * x + __umulhi(Ul, x)) >> 32);
    }
    return __umul64hi(((uint64_t)Uh << 32) | Ul, i1);
}

// wave-uniform 64-bit value in scalar registers
__device__ __forceinline__ int64_t uniform64(int64_t v) {
    return ((int64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v)) |
           ((int64_t)__builtin_amdgcn_readfirstlane((int)(v >> 32)) << 32);
}

// The stateless slot rule: slot j of the stream at [off, off + len) takes the element at its last writer wi
// (0: no draw hit it), else the stream's own element j, else none (-1: the slot is zero).
__device__ __forceinline__ int64_t slot_source(uint64_t wi, uint32_t j, int64_t off, int64_t len) {
    return wi ? off + (int64_t)wi : ((int64_t)j < len ? off + (int64_t)j : -1);
}

// the workgroup's table of T for the first kLut blocks, at the start of its LDS (k2_segmented spells it out)
// (32-bit division while the dividend fits: the table is rebuilt by every workgroup, and the
// 64-bit form was ~2.5 % of a C3 launch at 32768 workgroups)
__device__ __forceinline__ void build_lut(uint16_t* lut, uint64_t dense_lim) {
    for (uint32_t g = threadIdx.x; g < kLut; g += blockDim.x) {
        const uint64_t i0 = (uint64_t)g << 4;
        uint32_t T;
        if (i0 + 1 >= dense_lim) T = 0;
        else if (dense_lim + i0 <= 0xFFFFFFFFull) T = std::min<uint32_t>(256u, (uint32_t)(dense_lim + i0) / (uint32_t)(i0 + 1));
        else T = block_threshold(i0, dense_lim);
        lut[g] = (uint16_t)T;
    }
}

struct Wave {
    u32x4* stash;
    uint16_t* q;
    void* tab;
    const uint16_t* lut;
    uint32_t lane, k, k0, k1;
    uint64_t dense_lim;
    uint32_t fifo_cap;  // bulk appends while pending + new <= fifo_cap (<= the FIFO size; tests lower it)
    uint32_t wave;      // the wave's index in its workgroup, in a scalar register
};

// The frame every kernel opens with, over the workgroup's dynamic LDS (its first kLutBytes hold build_lut's
// table): this wave's stash [kRing][64] x 16 B and FIFO kQCap x u16 at base, and the winner table at tab.
__device__ __forceinline__ Wave make_wave(unsigned char* lds, unsigned char* base, void* tab, uint32_t wave,
                                          uint32_t lane, uint32_t k, uint32_t k0, uint32_t k1, uint32_t fifo_cap) {
    return Wave{(u32x4*)base, (uint16_t*)(base + kStashBytes), tab, (const uint16_t*)lds, lane, k, k0, k1,
                256ull * k, std::min<uint32_t>(std::max<uint32_t>(fifo_cap, 128u), kQCap), wave};
}

// the wave form (one wave per stream): per wave stash | FIFO | last-writer table k x (u32 | u64).
// The wave index is a scalar, so stream numbers and the offsets[] loads that follow from it are wave-uniform
// (scalar loads, counted by lgkmcnt -- never waited for together with a deferred key gather).
__device__ __forceinline__ Wave wave_frame(unsigned char* lds, uint32_t k, uint32_t k0, uint32_t k1,
                                           uint32_t fifo_cap) {
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    unsigned char* base = lds + kLutBytes + (size_t)wave * (kStashBytes + kQueueBytes + (size_t)k * 8);
    return make_wave(lds, base, base + kStashBytes + kQueueBytes, wave, lane, k, k0, k1, fifo_cap);
}

// One stream on one wave.  SMALL: n < 2^27 -- 32-bit indices, u32 winner table, and Philox counters
// whose high words are wave-uniform (level 0: g < 2^32; level 1: i/2 < 2^32).
// DEFER (k <= 64): the lane's winner index is returned (-1: none) and the caller gathers its key
// after storing the previous stream's, so the random gather's latency overlaps the next stream's draws.
// (k >= kWGMinK takes the workgroup form below, k2_segmented_wg.)
// RES (k2_segmented_update): the segment holds the stream's indices [n0, n0 + len) -- SMALL then means
// n0 + len < 2^27 -- and only the winner table is built: the caller writes it back into its state row.
template <typename KeyT, bool SMALL, bool DEFER, bool RES = false>
__device__ __forceinline__ int64_t k2_stream(const Wave& W, const KeyT* __restrict__ keys, int64_t off, int64_t len,
                                             uint64_t stream, KeyT* __restrict__ o, int64_t n0 = 0) {
    using IdxT = typename std::conditional<SMALL, uint32_t, uint64_t>::type;
    constexpr uint32_t QC = kQCap, RG = kRing, WIN = RG * 1024;  // WIN: indices in the ring
    const uint32_t lane = W.lane, k = W.k;
    IdxT* tab = (IdxT*)W.tab;
    for (uint32_t j = lane; j < k; j += 64) tab[j] = 0;
    const uint32_t s0 = (uint32_t)stream, s1 = (uint32_t)(stream >> 32);
    const DrawKey dk{W.k0, W.k1, s0, s1};
    // the draws cover [lo, nend): lo = k and nend = len for a whole stream, max(k, n0) and n0 + len resumed
    // (the head spells its stateless bound as (IdxT)k, not lo: the same value, but with lo there the
    // compiler schedules the stateless kernels differently, and their code is to stay as measured)
    const IdxT lo = RES ? (IdxT)std::max<uint64_t>((uint64_t)k, (uint64_t)n0) : (IdxT)k;
    const uint64_t nend = RES ? (uint64_t)n0 + (uint64_t)len : (uint64_t)len;
    const IdxT n_groups = (IdxT)((nend + 15) >> 4);
    uint32_t head = 0, tail = 0;  // FIFO positions (wave-uniform, wrap mod 2^32)
    // iterations start at a multiple of 64 blocks (the blocks below lo >> 4 are clipped: fill, or an
    // earlier segment's), so block g sits in stash slot g mod 256 (ring = (g / 64) mod 4) and a FIFO
    // entry is i mod 4096
    IdxT gb = (IdxT)((k >> 4) & ~63u);
    uint32_t ring = (k >> 10) & (RG - 1);
    if constexpr (RES) {
        gb = (lo >> 4) & ~(IdxT)63;
        ring = (uint32_t)(gb >> 6) & (RG - 1);
    }

    // resolve FIFO entries [head, head + nvalid) (nvalid <= 64), one per lane; last_gb = the most
    // recently stashed iteration: every pending index lies in [16 (last_gb - 192), + 4096)
    auto resolve_round = [&](uint32_t nvalid, IdxT last_gb) {
        __builtin_amdgcn_wave_barrier();
        const bool valid = lane < nvalid;
        const uint32_t ent = valid ? W.q[(head + lane) & (QC - 1)] : 0u;
        const uint32_t e = ent & 15u;
        const u32x4 w = W.stash[ent >> 4];  // block g mod 256
        const IdxT wlo = (last_gb << 4) - (IdxT)(WIN - 1024);
        const IdxT i = wlo + (IdxT)((ent - (uint32_t)wlo) & (WIN - 1));
        const uint32_t b = level0_byte(w, e);
        const IdxT g1 = i >> 1;
        u32x4 w1;
        if constexpr (SMALL) w1 = philox4x32_10_uniform_hi((uint32_t)g1, kDomainLevel1, s0, s1, W.k0, W.k1);
        else w1 = philox4x32_10((uint32_t)g1, (uint32_t)((uint64_t)g1 >> 32) | kDomainLevel1, s0, s1, W.k0, W.k1);
        // all four words, then one select per half (else the compiler selects the last round's
        // operands instead: 7 v_cndmask for the one saved product)
        asm volatile("" : "+v"(w1.x), "+v"(w1.y), "+v"(w1.z), "+v"(w1.w));
        const bool odd = (i & 1) != 0;
        const uint64_t j = draw_j(b, odd ? w1.z : w1.x, odd ? w1.w : w1.y, (uint64_t)i + 1, SMALL);
        if (valid && j < k) atomicMax(&tab[(uint32_t)j], i);
        head += nvalid;
        __builtin_amdgcn_wave_barrier();
    };

    // The dense head [k, hend), hend = min(len, HM k): candidate density >= 256 / HM %, so it skips
    // the FIFO -- each lane takes a PAIR of indices (one level-1 Philox serves both) straight from
    // the stashed level-0 block; the FIFO path covers [hend, len).
    // The head is cut to whole 64-pair rounds (k = 64: [64, 192) instead of [64, 256): its 96 pairs
    // took two rounds, the second half empty; the 64 indices moved to the FIFO add ~20 candidates
    // to rounds it runs anyway): C3 1.75-1.76 -> 1.67-1.69 ms (tools/micro_k2 r, warm clock).
    constexpr uint32_t HM = 4;
    uint64_t hx = (uint64_t)HM * k;
    // (only where the head holds at least one whole round: below k = 43 the cut would remove it and
    // send the 25-100 % dense region through the FIFO)
    if (hx - k >= 128) hx = k + ((hx - k) & ~(uint64_t)127);
    const IdxT hend = (IdxT)std::min<uint64_t>((uint64_t)nend, hx);
    const IdxT flo = std::max<IdxT>(lo, hend);
    for (; gb < n_groups; gb += 64, ring = (ring + 1) & (RG - 1)) {
        // the oldest pending candidate still refers to the ring slot about to be overwritten
        if (tail != head && ((uint32_t)__builtin_amdgcn_readfirstlane((int)W.q[head & (QC - 1)]) >> 10) == ring) {
            while (tail != head) resolve_round(std::min<uint32_t>(64u, tail - head), gb - 64);
        }
        const IdxT g = gb + lane;
        const bool valid = g < n_groups;
        u32x4 w;
        if constexpr (SMALL) w = philox4x32_10_uniform_hi((uint32_t)g, 0u, s0, s1, W.k0, W.k1);
        else w = level0(dk, (uint64_t)g);
        const uint64_t i0 = (uint64_t)g << 4;
        const uint32_t T = g < kLut ? (uint32_t)W.lut[(uint32_t)g] : block_threshold(i0, W.dense_lim);
        // T falls with the block index, so lane 0's (block gb) bounds the iteration's: past the first
        // blocks of a stream every lane has T <= 16 (C3: iterations 1..3) and takes the short compare
        const uint32_t Tmax = (uint32_t)__builtin_amdgcn_readfirstlane((int)T);
        uint32_t mask = valid ? (Tmax <= 16u ? mask_for_small(w, T) : mask_for(w, T)) : 0u;
        bool clip;  // wave-uniform; 32-bit compares for SMALL (scalar: no 64-bit s_cmp_lt)
        if constexpr (SMALL) clip = ((uint32_t)gb << 4) < (uint32_t)flo || (((uint32_t)gb + 64) << 4) > (uint32_t)nend;
        else clip = ((uint64_t)gb << 4) < (uint64_t)flo || (((uint64_t)gb + 64) << 4) > (uint64_t)nend;
        if (clip) mask &= clip16(i0, (uint64_t)flo, (uint64_t)nend);
        W.stash[ring * 64 + lane] = w;
        // this iteration holds head indices (uniform; resumed: only a segment that starts inside the head)
        if (((uint64_t)gb << 4) < (uint64_t)hend && (!RES || lo < hend)) {
            __builtin_amdgcn_wave_barrier();
            const IdxT ia = std::max<IdxT>((RES ? lo : (IdxT)k) & ~(IdxT)1, gb << 4);
            const IdxT ib = std::min<IdxT>(hend, (gb + 64) << 4);
            for (IdxT p0 = ia; p0 < ib; p0 += 128) {
                const IdxT i = p0 + 2 * lane;  // even
                const u32x4 wl = W.stash[(uint32_t)(i >> 4) & (RG * 64 - 1)];
                uint32_t b0, b1;
                level0_byte_pair(wl, (uint32_t)i & 15u, b0, b1);
                const IdxT g1 = i >> 1;
                u32x4 w1;
                if constexpr (SMALL) w1 = philox4x32_10_uniform_hi((uint32_t)g1, kDomainLevel1, s0, s1, W.k0, W.k1);
                else w1 = philox4x32_10((uint32_t)g1, (uint32_t)((uint64_t)g1 >> 32) | kDomainLevel1, s0, s1, W.k0, W.k1);
                asm volatile("" : "+v"(w1.x), "+v"(w1.y), "+v"(w1.z), "+v"(w1.w));
                const uint64_t j0 = draw_j(b0, w1.x, w1.y, (uint64_t)i + 1, SMALL);
                const uint64_t j1 = draw_j(b1, w1.z, w1.w, (uint64_t)i + 2, SMALL);
                if (i < ib && i >= (RES ? lo : (IdxT)k) && j0 < k) atomicMax(&tab[(uint32_t)j0], i);
                if (i + 1 < ib && i + 1 >= (RES ? lo : (IdxT)k) && j1 < k) atomicMax(&tab[(uint32_t)j1], i + 1);
            }
            __builtin_amdgcn_wave_barrier();
        }
        // FIFO offsets: one wave prefix sum of the per-lane candidate counts
        const uint32_t cnt = (uint32_t)__popc(mask);
        const uint32_t incl = wave_incl_scan(cnt);
        const uint32_t tot = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
        const uint32_t tag = (ring << 10) | (lane << 4);  // = (g mod 256) << 4
        if (tail - head + tot <= W.fifo_cap) {  // uniform: the whole iteration fits
            uint32_t pos = tail + incl - cnt;
            if ((tail & (QC - 1)) + tot <= QC) {  // uniform: no ring wrap inside the iteration's span
                // the lane's run is contiguous: one address increment per entry (round 6: no
                // ring mask and address rebuild per entry, ~2 VALU per append-loop trip)
                uint16_t* qp = W.q + (pos & (QC - 1));
                while (mask) {
                    const uint32_t e = __builtin_ctz(mask);
                    mask &= mask - 1;
                    *qp++ = (uint16_t)(tag | e);
                }
            } else {
                while (mask) {
                    const uint32_t e = __builtin_ctz(mask);
                    mask &= mask - 1;
                    W.q[pos & (QC - 1)] = (uint16_t)(tag | e);
                    ++pos;
                }
            }
            tail += tot;
        } else {  // an iteration denser than the FIFO (never at random draws beyond the dense
                  // head: ~4 candidates per block): one candidate per lane per round, resolved
                  // as 64 wait, so at most 127 are ever pending
            for (;;) {
                const bool has = mask != 0;
                const unsigned long long bal = __builtin_amdgcn_ballot_w64(has);
                if (!bal) break;
                if (has) {
                    const uint32_t e = __builtin_ctz(mask);
                    mask &= mask - 1;
                    const uint32_t pos = tail + __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32),
                                                                          __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
                    W.q[pos & (QC - 1)] = (uint16_t)(tag | e);
                }
                tail += (uint32_t)__popcll(bal);
                if (tail - head >= 64) resolve_round(64u, gb);
            }
        }
        while (tail - head >= 64) resolve_round(64u, gb);
    }
    while (tail != head) resolve_round(std::min<uint32_t>(64u, tail - head), gb - 64);
    __builtin_amdgcn_wave_barrier();
    if constexpr (RES) return -1;  // the caller merges the table into its state row
    if constexpr (DEFER) {  // the caller gathers (one load site, see k2_segmented)
        int64_t at = -1;
        if (lane < k) {
            const IdxT wi = tab[lane];
            at = wi ? (int64_t)wi : ((int64_t)lane < len ? (int64_t)lane : -1);
        }
        __builtin_amdgcn_wave_barrier();
        return at;
    }
    for (uint32_t j = lane; j < k; j += 64) {
        // slot_source, spelled out: through the helper k2_segmented (this loop's only caller) compiles to
        // another register allocation, and its stateless launch measured 0.2-0.7 % slower
        const IdxT wi = tab[j];
        o[j] = wi ? keys[off + (int64_t)wi] : ((int64_t)j < len ? keys[off + j] : (KeyT)0);
    }
    __builtin_amdgcn_wave_barrier();
    return -1;
}

template <typename KeyT>
__global__ __launch_bounds__(64 * kWaves) void k2_segmented(const KeyT* __restrict__ keys,
                                                            const int64_t* __restrict__ offsets, int64_t S,
                                                            uint32_t k, uint32_t k0, uint32_t k1, uint64_t stream_base,
                                                            KeyT* __restrict__ out, int64_t* __restrict__ counts,
                                                            uint32_t fifo_cap = kQCap) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    // build_lut, written out: the call moves this kernel's kernel-argument loads and renumbers its scalar
    // registers, and with that its stateless launch measured 0.2-0.7 % slower; with the loop
    // here the kernel is the measured one instruction for instruction
    uint16_t* lut = (uint16_t*)lds;
    const uint64_t dense_lim = 256ull * k;
    for (uint32_t g = threadIdx.x; g < kLut; g += blockDim.x) {
        const uint64_t i0 = (uint64_t)g << 4;
        uint32_t T;
        if (i0 + 1 >= dense_lim) T = 0;
        else if (dense_lim + i0 <= 0xFFFFFFFFull) T = std::min<uint32_t>(256u, (uint32_t)(dense_lim + i0) / (uint32_t)(i0 + 1));
        else T = block_threshold(i0, dense_lim);
        lut[g] = (uint16_t)T;
    }
    __syncthreads();
    const Wave W = wave_frame(lds, k, k0, k1, fifo_cap);
    const uint32_t lane = W.lane;
    const int64_t wave_stride = (int64_t)gridDim.x * kWaves;
    int64_t s = (int64_t)blockIdx.x * kWaves + W.wave;
    int64_t off = 0, end = 0;
    if (s < S) {
        off = offsets[s];
        end = offsets[s + 1];
    }
    if (k <= 64) {
        // Each stream's winner key is gathered at its end and stored TWO streams later, so every
        // wave keeps two streams' gathers in flight (one was measured short of the memory
        // concurrency the random-line rate needs: ~57 lines x 6k waves x 2 / 9 us of in-flight time).
        // The stream loop is unrolled by two so stream t's key lives in register set t & 1 and no
        // register copy of a load in flight exists (no s_waitcnt beyond the one for the store's data).
        KeyT* po[2] = {nullptr, nullptr};
        KeyT pv[2] = {0, 0};
        bool pok[2] = {false, false};
        const __attribute__((address_space(4))) int64_t* co =
            (const __attribute__((address_space(4))) int64_t*)offsets;
        auto one = [&](int u) {
            off = uniform64(off);
            end = uniform64(end);
            const int64_t len = end - off;
            const int64_t s_pf = std::min<int64_t>(s + wave_stride, S - 1);
            // scalar loads (constant address space: offsets[] is read-only here), so that no
            // vmcnt wait for them drains the gathers in flight
            const int64_t off_next = co[s_pf], end_next = co[s_pf + 1];
            const uint64_t stream = stream_base + (uint64_t)s;
            KeyT* o = out + s * (int64_t)k;
            const int64_t at = len < kSmallLen ? k2_stream<KeyT, true, true>(W, keys, off, len, stream, o)
                                               : k2_stream<KeyT, false, true>(W, keys, off, len, stream, o);
            // the gather of stream s - 2*wave_stride (slot u) has had two streams of work to land:
            // after it this wave issued at least two vector-memory ops (the counts store and slot
            // 1-u's gather; the po store too once both slots are live), so vmcnt(2) covers it
            // without waiting for slot 1-u's gather. The loads are asm so that the compiler's own
            // waits (which cannot count past a load it does not see) stay conservative.
            asm volatile("s_waitcnt vmcnt(2)" : "+v"(pv[u]));
            if (po[u] && lane < k) po[u][lane] = pok[u] ? pv[u] : (KeyT)0;
            if (lane == 0) counts[s] = len < (int64_t)k ? len : (int64_t)k;
            po[u] = o;
            pok[u] = at >= 0;  // else an empty slot: the load below reads a valid dummy word
            const KeyT* src = pok[u] ? keys + off + at : (const KeyT*)offsets;
            if constexpr (sizeof(KeyT) == 8)
                asm volatile("global_load_dwordx2 %0, %1, off" : "=&v"(pv[u]) : "v"(src));
            else
                asm volatile("global_load_dword %0, %1, off" : "=&v"(pv[u]) : "v"(src));
            off = off_next;
            end = end_next;
            s += wave_stride;
        };
        for (; s + wave_stride < S;) {  // two streams a trip (wave-uniform), no exit between them
            one(0);
            one(1);
        }
        if (s < S) one(0);
        asm volatile("s_waitcnt vmcnt(0)" : "+v"(pv[0]), "+v"(pv[1]));
#pragma unroll
        for (int u = 0; u < 2; ++u)
            if (po[u] && lane < k) po[u][lane] = pok[u] ? pv[u] : (KeyT)0;
        return;
    }
    for (; s < S; s += wave_stride) {
        // wave-uniform stream bounds (scalar registers: uniform control flow below)
        off = uniform64(off);
        end = uniform64(end);
        const int64_t len = end - off;
        const int64_t s_next = s + wave_stride;
        // prefetch, in flight during this stream's work; unconditional (clamped index), so the
        // loop-top wait for it is vmcnt(1) -- it does not also wait for the deferred gather below
        const int64_t s_pf = std::min<int64_t>(s_next, S - 1);
        const int64_t off_next = offsets[s_pf], end_next = offsets[s_pf + 1];
        const uint64_t stream = stream_base + (uint64_t)s;
        KeyT* o = out + s * (int64_t)k;
        if (len < kSmallLen) {
            k2_stream<KeyT, true, false>(W, keys, off, len, stream, o);
        } else {
            k2_stream<KeyT, false, false>(W, keys, off, len, stream, o);
        }
        if (lane == 0) counts[s] = len < (int64_t)k ? len : (int64_t)k;
        off = off_next;
        end = end_next;
    }
}

// ---- resumed: the streams are rows of caller-held state ------------------------------------------
// rsv_sample_segmented_update: segment b = keys[offsets[b], offsets[b+1]) holds the indices
// [n0, n0 + len) of row r = ids[b] (null: b), Philox stream stream_base + r, n0 = bases[b] (null:
// state_next[r]).  The element loops above run from max(k, n0); the write-back below replaces a slot
// only where this segment's last writer (or its fill index j in [n0, min(k, n0 + len))) is later than
// the row's idx -- the largest index per slot wins, whatever order the segments arrive in.  Segments
// with an id outside [0, S), a negative base or no elements are skipped.


// segment b of an update: keys[off, off + len) are the indices [n0, nend) of state row r
struct Segment {
    int64_t off, len, r, n0, nend;
};

// Reads segment b's header; false: the segment is skipped (empty, an id outside [0, S), a negative base).
// Every thread of the wave -- in the workgroup form, of the workgroup -- reads the same words, and reads
// state_next[r] before anyone writes it.
__device__ __forceinline__ bool read_segment(Segment& g, const int64_t* offsets, const int64_t* ids,
                                             const int64_t* bases, const int64_t* state_next, int64_t b, int64_t S) {
    g.off = uniform64(offsets[b]);
    g.len = uniform64(offsets[b + 1]) - g.off;
    g.r = ids ? uniform64(ids[b]) : b;
    if (g.len <= 0 || g.r < 0 || g.r >= S) return false;
    g.n0 = uniform64(bases ? bases[b] : state_next[g.r]);
    if (g.n0 < 0) return false;
    g.nend = g.n0 + g.len;
    return true;
}

// slot j of a row: winner w (0: none) of the segment [n0, nend) at keys[off ...]
template <typename KeyT>
__device__ __forceinline__ void update_slot(const KeyT* __restrict__ keys, int64_t off, int64_t n0, int64_t nend,
                                            uint32_t j, uint64_t w, KeyT* __restrict__ sk, int64_t* __restrict__ si) {
    int64_t at = (int64_t)w;
    if (!w) at = ((int64_t)j >= n0 && (int64_t)j < nend) ? (int64_t)j : -1;  // a fill index of this segment
    if (at < 0) return;
    if (si[j] < at) {
        sk[j] = keys[off + (at - n0)];
        si[j] = at;
    }
}

template <typename KeyT>
__global__ __launch_bounds__(64 * kWaves) void k2_segmented_update(
    const KeyT* __restrict__ keys, const int64_t* __restrict__ offsets, const int64_t* __restrict__ ids,
    const int64_t* __restrict__ bases, int64_t B, int64_t S, uint32_t k, uint32_t k0, uint32_t k1,
    uint64_t stream_base, KeyT* __restrict__ state_keys, int64_t* __restrict__ state_idx,
    int64_t* __restrict__ state_next, uint32_t fifo_cap) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    build_lut((uint16_t*)lds, 256ull * k);
    __syncthreads();
    const Wave W = wave_frame(lds, k, k0, k1, fifo_cap);
    const uint32_t lane = W.lane;
    const int64_t wave_stride = (int64_t)gridDim.x * kWaves;
    for (int64_t b = (int64_t)blockIdx.x * kWaves + W.wave; b < B; b += wave_stride) {
        Segment g;
        if (!read_segment(g, offsets, ids, bases, state_next, b, S)) continue;
        const uint64_t stream = stream_base + (uint64_t)g.r;
        KeyT* sk = state_keys + g.r * (int64_t)k;
        int64_t* si = state_idx + g.r * (int64_t)k;
        if (g.nend < kSmallLen) {
            k2_stream<KeyT, true, false, true>(W, keys, g.off, g.len, stream, nullptr, g.n0);
            for (uint32_t j = lane; j < k; j += 64)
                update_slot(keys, g.off, g.n0, g.nend, j, ((const uint32_t*)W.tab)[j], sk, si);
        } else {
            k2_stream<KeyT, false, false, true>(W, keys, g.off, g.len, stream, nullptr, g.n0);
            for (uint32_t j = lane; j < k; j += 64)
                update_slot(keys, g.off, g.n0, g.nend, j, ((const uint64_t*)W.tab)[j], sk, si);
        }
        if (lane == 0 && state_next[g.r] < g.nend) state_next[g.r] = g.nend;
        __builtin_amdgcn_wave_barrier();  // the table is read before the next segment zeroes it
    }
}

// ---- large k: one WORKGROUP per stream ------------------------------------------------------------
// Per wave, k2_segmented keeps a k-slot table in LDS: above k ~ 512 the tables cap a CU at one or two
// workgroups (k = 4096: 150 KB, one wave per SIMD) and above k = 4416 they no longer fit at all --
// round 4's global per-wave tables then paid global atomics and a 1 GiB zero fill per call (3.7 ms
// for 4096 x 2^17 at k = 8192).  Here the NW waves of a workgroup share ONE stream and ONE table:
// wave w takes the stream's 64-block iterations w, w + NW, w + 2 NW, ... (interleaved, so the
// candidate-rich dense head is spread over the waves), each with its own stash ring and FIFO, and all
// resolve into the workgroup's table -- in LDS while k * sizeof(TabT) fits beside the waves' rings,
// else the workgroup's slice of a global scratch table that stays zero between streams (the gather
// takes every entry back with an atomic exchange).  TabT = u32 when every stream index fits 32 bits.
constexpr int kWavesWG = 8;
constexpr uint32_t kWGMinK = 512;  // smaller k keep one wave per stream (C3: k = 64)

__host__ __device__ constexpr size_t lds_bytes_wg(uint32_t k, size_t tab_entry, bool GT) {
    return kLutBytes + (size_t)kWavesWG * (kStashBytes + kQueueBytes) + (GT ? 0 : (size_t)k * tab_entry);
}

// the workgroup form's frame: per wave stash | FIFO, then the one table the waves share -- after the
// eight waves' rings, or (GT) the workgroup's slice of the global scratch gtab
template <bool GT = false, typename TabT = unsigned long long>
__device__ __forceinline__ Wave wg_frame(unsigned char* lds, uint32_t k, uint32_t k0, uint32_t k1, uint32_t fifo_cap,
                                         TabT* gtab = nullptr) {
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    unsigned char* base = lds + kLutBytes + (size_t)wave * (kStashBytes + kQueueBytes);
    TabT* tab = GT ? gtab + (size_t)blockIdx.x * k
                   : (TabT*)(lds + kLutBytes + (size_t)kWavesWG * (kStashBytes + kQueueBytes));
    return make_wave(lds, base, tab, wave, lane, k, k0, k1, fifo_cap);
}

// RES (k2_segmented_update_wg): the segment holds the stream's indices [n0, n0 + len), as in k2_stream.
template <typename TabT, bool SMALL, bool GT, bool RES = false>
__device__ __forceinline__ void k2_part(const Wave& W, TabT* tab, int64_t len, uint64_t stream, uint32_t wave,
                                        int64_t n0 = 0) {
    using IdxT = typename std::conditional<SMALL, uint32_t, uint64_t>::type;
    constexpr uint32_t QC = kQCap, RG = kRing;
    constexpr uint32_t STEP = 64u * kWavesWG;  // blocks between this wave's iterations
    const uint32_t lane = W.lane, k = W.k;
    const uint32_t s0 = (uint32_t)stream, s1 = (uint32_t)(stream >> 32);
    const DrawKey dk{W.k0, W.k1, s0, s1};
    const IdxT lo = RES ? (IdxT)std::max<uint64_t>((uint64_t)k, (uint64_t)n0) : (IdxT)k;
    const uint64_t nend = RES ? (uint64_t)n0 + (uint64_t)len : (uint64_t)len;
    const IdxT n_groups = (IdxT)((nend + 15) >> 4);
    uint32_t head = 0, tail = 0;
    IdxT gb = (IdxT)(((k >> 4) & ~63u) + 64u * wave);
    if constexpr (RES) gb = ((lo >> 4) & ~(IdxT)63) + (IdxT)(64u * wave);
    uint32_t ring = 0;
    IdxT slot_gb[RG] = {};  // first block of the iteration each ring slot holds (wave-uniform)

    auto resolve_round = [&](uint32_t nvalid) {
        __builtin_amdgcn_wave_barrier();
        const bool valid = lane < nvalid;
        const uint32_t ent = valid ? W.q[(head + lane) & (QC - 1)] : 0u;
        const uint32_t e = ent & 15u, r = ent >> 10;
        const u32x4 w = W.stash[ent >> 4];
        IdxT g0 = slot_gb[0];
#pragma unroll
        for (uint32_t q = 1; q < RG; ++q) g0 = r == q ? slot_gb[q] : g0;
        const IdxT i = ((g0 + (IdxT)((ent >> 4) & 63u)) << 4) + (IdxT)e;
        const uint32_t b = level0_byte(w, e);
        const IdxT g1 = i >> 1;
        u32x4 w1;
        if constexpr (SMALL) w1 = philox4x32_10_uniform_hi((uint32_t)g1, kDomainLevel1, s0, s1, W.k0, W.k1);
        else w1 = philox4x32_10((uint32_t)g1, (uint32_t)((uint64_t)g1 >> 32) | kDomainLevel1, s0, s1, W.k0, W.k1);
        asm volatile("" : "+v"(w1.x), "+v"(w1.y), "+v"(w1.z), "+v"(w1.w));
        const bool odd = (i & 1) != 0;
        const uint64_t j = draw_j(b, odd ? w1.z : w1.x, odd ? w1.w : w1.y, (uint64_t)i + 1, SMALL);
        if (valid && j < k) atomicMax(&tab[(uint32_t)j], (TabT)i);
        head += nvalid;
        __builtin_amdgcn_wave_barrier();
    };

    // the dense head [k, hend) by index pairs, as k2_stream (each wave takes its iterations' share)
    uint64_t hx = 4ull * k;
    if (hx - k >= 128) hx = k + ((hx - k) & ~(uint64_t)127);
    const IdxT hend = (IdxT)std::min<uint64_t>((uint64_t)nend, hx);
    const IdxT flo = std::max<IdxT>(lo, hend);
    for (; gb < n_groups; gb += STEP, ring = (ring + 1) & (RG - 1)) {
        if (tail != head && ((uint32_t)__builtin_amdgcn_readfirstlane((int)W.q[head & (QC - 1)]) >> 10) == ring) {
            while (tail != head) resolve_round(std::min<uint32_t>(64u, tail - head));
        }
        slot_gb[0] = ring == 0 ? gb : slot_gb[0];
#pragma unroll
        for (uint32_t q = 1; q < RG; ++q) slot_gb[q] = ring == q ? gb : slot_gb[q];
        const IdxT g = gb + lane;
        const bool valid = g < n_groups;
        u32x4 w;
        if constexpr (SMALL) w = philox4x32_10_uniform_hi((uint32_t)g, 0u, s0, s1, W.k0, W.k1);
        else w = level0(dk, (uint64_t)g);
        const uint64_t i0 = (uint64_t)g << 4;
        const uint32_t T = g < kLut ? (uint32_t)W.lut[(uint32_t)g] : block_threshold(i0, W.dense_lim);
        const uint32_t Tmax = (uint32_t)__builtin_amdgcn_readfirstlane((int)T);
        uint32_t mask = valid ? (Tmax <= 16u ? mask_for_small(w, T) : mask_for(w, T)) : 0u;
        const bool clip = ((uint64_t)gb << 4) < (uint64_t)flo || (((uint64_t)gb + 64) << 4) > (uint64_t)nend;
        if (clip) mask &= clip16(i0, (uint64_t)flo, (uint64_t)nend);
        W.stash[ring * 64 + lane] = w;
        // this iteration holds head indices (uniform; resumed: only a segment that starts inside the head)
        if (((uint64_t)gb << 4) < (uint64_t)hend && (!RES || lo < hend)) {
            __builtin_amdgcn_wave_barrier();
            const IdxT ia = std::max<IdxT>((RES ? lo : (IdxT)k) & ~(IdxT)1, gb << 4);
            const IdxT ib = std::min<IdxT>(hend, (gb + 64) << 4);
            for (IdxT p0 = ia; p0 < ib; p0 += 128) {
                const IdxT i = p0 + 2 * lane;  // even
                const u32x4 wl = W.stash[ring * 64 + (uint32_t)((i >> 4) - gb)];
                uint32_t b0, b1;
                level0_byte_pair(wl, (uint32_t)i & 15u, b0, b1);
                const IdxT g1 = i >> 1;
                u32x4 w1;
                if constexpr (SMALL) w1 = philox4x32_10_uniform_hi((uint32_t)g1, kDomainLevel1, s0, s1, W.k0, W.k1);
                else w1 = philox4x32_10((uint32_t)g1, (uint32_t)((uint64_t)g1 >> 32) | kDomainLevel1, s0, s1, W.k0, W.k1);
                asm volatile("" : "+v"(w1.x), "+v"(w1.y), "+v"(w1.z), "+v"(w1.w));
                const uint64_t j0 = draw_j(b0, w1.x, w1.y, (uint64_t)i + 1, SMALL);
                const uint64_t j1 = draw_j(b1, w1.z, w1.w, (uint64_t)i + 2, SMALL);
                if (i < ib && i >= (RES ? lo : (IdxT)k) && j0 < k) atomicMax(&tab[(uint32_t)j0], (TabT)i);
                if (i + 1 < ib && i + 1 >= (RES ? lo : (IdxT)k) && j1 < k) atomicMax(&tab[(uint32_t)j1], (TabT)(i + 1));
            }
            __builtin_amdgcn_wave_barrier();
        }
        const uint32_t cnt = (uint32_t)__popc(mask);
        const uint32_t incl = wave_incl_scan(cnt);
        const uint32_t tot = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
        const uint32_t tag = (ring << 10) | (lane << 4);
        if (tail - head + tot <= W.fifo_cap) {
            uint32_t pos = tail + incl - cnt;
            while (mask) {
                const uint32_t e = __builtin_ctz(mask);
                mask &= mask - 1;
                W.q[pos & (QC - 1)] = (uint16_t)(tag | e);
                ++pos;
            }
            tail += tot;
        } else {  // denser than the FIFO: one candidate per lane per round, resolved 64 at a time
            for (;;) {
                const bool has = mask != 0;
                const unsigned long long bal = __builtin_amdgcn_ballot_w64(has);
                if (!bal) break;
                if (has) {
                    const uint32_t e = __builtin_ctz(mask);
                    mask &= mask - 1;
                    const uint32_t pos = tail + __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32),
                                                                          __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
                    W.q[pos & (QC - 1)] = (uint16_t)(tag | e);
                }
                tail += (uint32_t)__popcll(bal);
                if (tail - head >= 64) resolve_round(64u);
            }
        }
        while (tail - head >= 64) resolve_round(64u);
    }
    while (tail != head) resolve_round(std::min<uint32_t>(64u, tail - head));
    __builtin_amdgcn_wave_barrier();
}

template <typename KeyT, typename TabT, bool GT>
__global__ __launch_bounds__(64 * kWavesWG) void k2_segmented_wg(const KeyT* __restrict__ keys,
                                                                 const int64_t* __restrict__ offsets, int64_t S,
                                                                 uint32_t k, uint32_t k0, uint32_t k1,
                                                                 uint64_t stream_base, KeyT* __restrict__ out,
                                                                 int64_t* __restrict__ counts, uint32_t fifo_cap,
                                                                 TabT* __restrict__ gtab) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    build_lut((uint16_t*)lds, 256ull * k);
    const Wave W = wg_frame<GT>(lds, k, k0, k1, fifo_cap, gtab);
    TabT* tab = (TabT*)W.tab;
    const uint32_t nthr = 64u * kWavesWG;
    for (int64_t s = blockIdx.x; s < S; s += gridDim.x) {
        const int64_t off = offsets[s], len = offsets[s + 1] - off;
        if constexpr (!GT)
            for (uint32_t j = threadIdx.x; j < k; j += nthr) tab[j] = 0;
        __syncthreads();  // the table is zero (GT: the previous stream's gather left it so)
        const uint64_t stream = stream_base + (uint64_t)s;
        if (len < kSmallLen) k2_part<TabT, true, GT>(W, tab, len, stream, W.wave);
        else k2_part<TabT, false, GT>(W, tab, len, stream, W.wave);
        if constexpr (GT) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");  // this wave's table atomics
        __syncthreads();
        if constexpr (GT) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");  // every wave's, before the gather
        KeyT* o = out + s * (int64_t)k;
        for (uint32_t j = threadIdx.x; j < k; j += nthr) {
            TabT wi;
            if constexpr (GT) wi = __hip_atomic_exchange(&tab[j], (TabT)0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            else wi = tab[j];
            const int64_t at = slot_source(wi, j, off, len);
            o[j] = at >= 0 ? keys[at] : (KeyT)0;
        }
        if (threadIdx.x == 0) counts[s] = len < (int64_t)k ? len : (int64_t)k;
        __syncthreads();  // the gather has read the table before the next stream zeroes it
    }
}

// the workgroup form of k2_segmented_update (k >= kWGMinK): one shared table in LDS, always 64-bit
// entries of the absolute index (no launch reads offsets or bases on the host), which bounds k by
// lds_bytes_wg(k, 8, false) <= kLdsMax
template <typename KeyT>
__global__ __launch_bounds__(64 * kWavesWG) void k2_segmented_update_wg(
    const KeyT* __restrict__ keys, const int64_t* __restrict__ offsets, const int64_t* __restrict__ ids,
    const int64_t* __restrict__ bases, int64_t B, int64_t S, uint32_t k, uint32_t k0, uint32_t k1,
    uint64_t stream_base, KeyT* __restrict__ state_keys, int64_t* __restrict__ state_idx,
    int64_t* __restrict__ state_next, uint32_t fifo_cap) {
    using TabT = unsigned long long;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    build_lut((uint16_t*)lds, 256ull * k);
    const Wave W = wg_frame(lds, k, k0, k1, fifo_cap);
    TabT* tab = (TabT*)W.tab;
    const uint32_t nthr = 64u * kWavesWG;
    for (int64_t b = blockIdx.x; b < B; b += gridDim.x) {
        Segment g;
        if (!read_segment(g, offsets, ids, bases, state_next, b, S)) continue;
        for (uint32_t j = threadIdx.x; j < k; j += nthr) tab[j] = 0;
        __syncthreads();  // the table is zero, the lut built, and n0 read by every wave
        const uint64_t stream = stream_base + (uint64_t)g.r;
        if (g.nend < kSmallLen) k2_part<TabT, true, false, true>(W, tab, g.len, stream, W.wave, g.n0);
        else k2_part<TabT, false, false, true>(W, tab, g.len, stream, W.wave, g.n0);
        __syncthreads();
        KeyT* sk = state_keys + g.r * (int64_t)k;
        int64_t* si = state_idx + g.r * (int64_t)k;
        for (uint32_t j = threadIdx.x; j < k; j += nthr) update_slot(keys, g.off, g.n0, g.nend, j, tab[j], sk, si);
        if (threadIdx.x == 0 && state_next[g.r] < g.nend) state_next[g.r] = g.nend;
        __syncthreads();  // the write-back has read the table before the next segment zeroes it
    }
}

// ---- resumed, through a permutation (rsv_sample_segmented_update_indirect) ----------
// Segment b's p-th element is keys[order[offsets[b] + p]]: the batch stays in arrival order and `order`
// (rsv_group_by_stream's) groups it.  The element loops never see a key, so only the write-back changes: it
// reads `order` for the slots it replaces and nothing else.  order has n_keys entries, each in [0, n_keys).

// the batch position of entry p of `order`, or -1 for a p or an entry outside [0, n_keys): such a slot is left
// as it is rather than dereferenced
__device__ __forceinline__ int64_t order_at(const int32_t* __restrict__ order, int64_t p, int64_t n_keys) {
    if (p < 0 || p >= n_keys) return -1;
    const int64_t q = order[p];
    return q < n_keys ? q : -1;  // a negative entry is -1 or below already
}

// update_slot with the segment's elements at keys[order[off ...]]
template <typename KeyT>
__device__ __forceinline__ void update_slot_indirect(const KeyT* __restrict__ keys, int64_t n_keys,
                                                     const int32_t* __restrict__ order, int64_t off, int64_t n0,
                                                     int64_t nend, uint32_t j, uint64_t w, KeyT* __restrict__ sk,
                                                     int64_t* __restrict__ si) {
    int64_t at = (int64_t)w;
    if (!w) at = ((int64_t)j >= n0 && (int64_t)j < nend) ? (int64_t)j : -1;  // a fill index of this segment
    if (at < 0) return;
    if (si[j] < at) {
        const int64_t q = order_at(order, off + (at - n0), n_keys);
        if (q < 0) return;
        sk[j] = keys[q];
        si[j] = at;
    }
}

template <typename KeyT>
__global__ __launch_bounds__(64 * kWaves) void k2_segmented_update_indirect(
    const KeyT* __restrict__ keys, int64_t n_keys, const int32_t* __restrict__ order,
    const int64_t* __restrict__ offsets, const int64_t* __restrict__ ids, const int64_t* __restrict__ bases, int64_t B,
    int64_t S, uint32_t k, uint32_t k0, uint32_t k1, uint64_t stream_base, KeyT* __restrict__ state_keys,
    int64_t* __restrict__ state_idx, int64_t* __restrict__ state_next, uint32_t fifo_cap) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    build_lut((uint16_t*)lds, 256ull * k);
    __syncthreads();
    const Wave W = wave_frame(lds, k, k0, k1, fifo_cap);
    const uint32_t lane = W.lane;
    const int64_t wave_stride = (int64_t)gridDim.x * kWaves;
    for (int64_t b = (int64_t)blockIdx.x * kWaves + W.wave; b < B; b += wave_stride) {
        Segment g;
        if (!read_segment(g, offsets, ids, bases, state_next, b, S)) continue;
        const uint64_t stream = stream_base + (uint64_t)g.r;
        KeyT* sk = state_keys + g.r * (int64_t)k;
        int64_t* si = state_idx + g.r * (int64_t)k;
        if (g.nend < kSmallLen) {
            k2_stream<KeyT, true, false, true>(W, keys, g.off, g.len, stream, nullptr, g.n0);
            for (uint32_t j = lane; j < k; j += 64)
                update_slot_indirect(keys, n_keys, order, g.off, g.n0, g.nend, j, ((const uint32_t*)W.tab)[j], sk, si);
        } else {
            k2_stream<KeyT, false, false, true>(W, keys, g.off, g.len, stream, nullptr, g.n0);
            for (uint32_t j = lane; j < k; j += 64)
                update_slot_indirect(keys, n_keys, order, g.off, g.n0, g.nend, j, ((const uint64_t*)W.tab)[j], sk, si);
        }
        if (lane == 0 && state_next[g.r] < g.nend) state_next[g.r] = g.nend;
        __builtin_amdgcn_wave_barrier();  // the table is read before the next segment zeroes it
    }
}

// the workgroup form (k >= kWGMinK), as k2_segmented_update_wg
template <typename KeyT>
__global__ __launch_bounds__(64 * kWavesWG) void k2_segmented_update_indirect_wg(
    const KeyT* __restrict__ keys, int64_t n_keys, const int32_t* __restrict__ order,
    const int64_t* __restrict__ offsets, const int64_t* __restrict__ ids, const int64_t* __restrict__ bases, int64_t B,
    int64_t S, uint32_t k, uint32_t k0, uint32_t k1, uint64_t stream_base, KeyT* __restrict__ state_keys,
    int64_t* __restrict__ state_idx, int64_t* __restrict__ state_next, uint32_t fifo_cap) {
    using TabT = unsigned long long;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    build_lut((uint16_t*)lds, 256ull * k);
    const Wave W = wg_frame(lds, k, k0, k1, fifo_cap);
    TabT* tab = (TabT*)W.tab;
    const uint32_t nthr = 64u * kWavesWG;
    for (int64_t b = blockIdx.x; b < B; b += gridDim.x) {
        Segment g;
        if (!read_segment(g, offsets, ids, bases, state_next, b, S)) continue;
        for (uint32_t j = threadIdx.x; j < k; j += nthr) tab[j] = 0;
        __syncthreads();  // the table is zero, the lut built, and n0 read by every wave
        const uint64_t stream = stream_base + (uint64_t)g.r;
        if (g.nend < kSmallLen) k2_part<TabT, true, false, true>(W, tab, g.len, stream, W.wave, g.n0);
        else k2_part<TabT, false, false, true>(W, tab, g.len, stream, W.wave, g.n0);
        __syncthreads();
        KeyT* sk = state_keys + g.r * (int64_t)k;
        int64_t* si = state_idx + g.r * (int64_t)k;
        for (uint32_t j = threadIdx.x; j < k; j += nthr)
            update_slot_indirect(keys, n_keys, order, g.off, g.n0, g.nend, j, tab[j], sk, si);
        if (threadIdx.x == 0 && state_next[g.r] < g.nend) state_next[g.r] = g.nend;
        __syncthreads();  // the write-back has read the table before the next segment zeroes it
    }
}

// rsv_sample_segmented_merge: per (row, slot) the part with the largest idx, if it beats the row's;
// next = the max over the row and the parts.  parts: [P][S][k], [P][S][k], [P][S].
// The pick for entry t = (row, slot) of S k: the part with the largest idx if it beats the state's (-1:
// none), and state_idx[t] takes it; the thread of a row's first slot also moves the row's next to the max.
// Only this thread reads or writes the entry's idx.  (No __restrict__ here or in the kernels: a state merged
// into itself names the same memory twice.)
template <typename Move>
__device__ __forceinline__ int32_t merge_pick(const int64_t* part_idx, const int64_t* part_next, int32_t P, int64_t S,
                                              uint32_t k, int64_t t, int64_t* state_idx, int64_t* state_next,
                                              Move move) {
    const int64_t total = S * (int64_t)k;
    int64_t best = state_idx[t];
    int32_t bp = -1;
    for (int32_t p = 0; p < P; ++p) {
        const int64_t pi = part_idx[(int64_t)p * total + t];
        if (pi > best) {
            best = pi;
            bp = p;
        }
    }
    if (bp >= 0) {
        move(bp);
        state_idx[t] = best;
    }
    if (t % k == 0) {
        const int64_t r = t / k;
        const int64_t cn = state_next[r];
        int64_t n = cn;
        for (int32_t p = 0; p < P; ++p) n = std::max<int64_t>(n, part_next[(int64_t)p * S + r]);
        if (n > cn) state_next[r] = n;
    }
    return bp;
}

template <typename KeyT>
__global__ __launch_bounds__(256) void k2_segmented_merge(const KeyT* part_keys, const int64_t* part_idx,
                                                          const int64_t* part_next, int32_t P, int64_t S, uint32_t k,
                                                          KeyT* state_keys, int64_t* state_idx, int64_t* state_next) {
    const int64_t total = S * (int64_t)k;
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    merge_pick(part_idx, part_next, P, S, k, t, state_idx, state_next,
               [&](int32_t bp) { state_keys[t] = part_keys[(int64_t)bp * total + t]; });
}

// ---- byte keys: the streams' elements are rows of W bytes (java.util.UUID: W = 16) ----------------
// rsv_sample_segmented_rows / _update / _merge.  The winners are found by the element loops above in
// their RES mode (only the last-writer table is built; n0 = 0 is a whole stream), so nothing here reads
// a row before its stream's at most k winners are known.  What is new is the gather: a row is C
// granules of sizeof(G) bytes -- uint4 where W % 16 == 0 and every base is 16-byte aligned (the host
// checks), else uint64_t: rows are only 8-byte aligned, W = 24 puts every other row off a 16-byte
// boundary -- and a team of NT threads walks the (slot, granule) pairs t = j C + c in steps of NT, so
// consecutive lanes move consecutive granules of a row.  Four pairs per lane are loaded before the
// first is stored.  Every byte offset is 64-bit, whatever the width of the index arithmetic in the
// element loops: a stream 2^28 rows into a 16-byte-row tensor starts past 4 GiB.

// the pair a thread starts at and its step, t = j C + c advanced by NT without a division per pair
struct PairStep {
    uint32_t j, c, dj, dc;
};
__device__ __forceinline__ PairStep pair_step(uint32_t tid, uint32_t nt, uint32_t C) {
    const uint32_t j = tid / C, dj = nt / C;
    return PairStep{j, tid - j * C, dj, nt - dj * C};
}
__device__ __forceinline__ void pair_next(PairStep& p, uint32_t C) {
    p.j += p.dj;
    p.c += p.dc;
    if (p.c >= C) {
        p.c -= C;
        ++p.j;
    }
}

// dst row j (of k) takes the row src_of(j) names: a row index into rows (64-bit), or -1 for a zero row
// (zero_empty) or a row that stays as it is
template <typename G, bool ZERO_EMPTY, typename SrcOf>
__device__ __forceinline__ void gather_rows(const unsigned char* rows, unsigned char* dst, uint32_t k, uint32_t C,
                                            PairStep p, SrcOf src_of) {
    constexpr int U = 4;
    const uint64_t Wb = (uint64_t)C * sizeof(G);
    while (p.j < k) {
        G v[U];
        G* d[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            d[u] = nullptr;
            v[u] = G{};
            if (p.j < k) {
                const int64_t at = src_of(p.j);
                if (ZERO_EMPTY || at >= 0) d[u] = (G*)(dst + (uint64_t)p.j * Wb) + p.c;
                if (at >= 0) v[u] = ((const G*)(rows + (uint64_t)at * Wb))[p.c];
            }
            pair_next(p, C);
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (d[u]) *d[u] = v[u];
    }
}

// stateless, one wave per stream (k < kWGMinK).  DEFER (k C <= 64: one pair per lane, a compile-time
// count): the lane's granule is loaded at its stream's end and stored after the NEXT stream's draws, so
// the random gather's latency overlaps them.  The load is plain C++ and the wait is the compiler's: it
// waits for everything in flight (vmcnt(0)) before the store, which is why a second register set does
// not put two streams' gathers in flight -- that takes hand-counted waits, as in k2_segmented.
template <typename G, bool DEFER>
__global__ __launch_bounds__(64 * kWaves) void k2_segmented_rows(const unsigned char* __restrict__ rows,
                                                                 const int64_t* __restrict__ offsets, int64_t S,
                                                                 uint32_t k, uint32_t C, uint32_t k0, uint32_t k1,
                                                                 uint64_t stream_base, unsigned char* __restrict__ out,
                                                                 int64_t* __restrict__ counts, uint32_t fifo_cap) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    build_lut((uint16_t*)lds, 256ull * k);
    __syncthreads();
    const Wave W = wave_frame(lds, k, k0, k1, fifo_cap);
    const uint32_t lane = W.lane;
    const void* tab = W.tab;
    const uint64_t Wb = (uint64_t)C * sizeof(G);
    const PairStep p0 = pair_step(lane, 64, C);
    const int64_t wave_stride = (int64_t)gridDim.x * kWaves;
    G pv = G{};       // DEFER: the previous stream's granule, in flight
    G* po = nullptr;  // and where it goes
    for (int64_t s = (int64_t)blockIdx.x * kWaves + W.wave; s < S; s += wave_stride) {
        const int64_t off = uniform64(offsets[s]);
        const int64_t len = std::max<int64_t>(uniform64(offsets[s + 1]) - off, 0);
        const uint64_t stream = stream_base + (uint64_t)s;
        const bool small = len < kSmallLen;
        if (small) k2_stream<int64_t, true, false, true>(W, nullptr, off, len, stream, nullptr, 0);
        else k2_stream<int64_t, false, false, true>(W, nullptr, off, len, stream, nullptr, 0);
        auto src_of = [&](uint32_t j) -> int64_t {
            return slot_source(small ? (uint64_t)((const uint32_t*)tab)[j] : ((const uint64_t*)tab)[j], j, off, len);
        };
        unsigned char* o = out + (uint64_t)s * k * Wb;
        if constexpr (DEFER) {
            if (po) *po = pv;
            po = nullptr;
            if (p0.j < k) {
                const int64_t at = src_of(p0.j);
                po = (G*)(o + (uint64_t)p0.j * Wb) + p0.c;
                pv = G{};
                if (at >= 0) pv = ((const G*)(rows + (uint64_t)at * Wb))[p0.c];
            }
        } else {
            gather_rows<G, true>(rows, o, k, C, p0, src_of);
        }
        if (lane == 0) counts[s] = len < (int64_t)k ? len : (int64_t)k;
        __builtin_amdgcn_wave_barrier();  // the table is read before the next stream zeroes it
    }
    if constexpr (DEFER)
        if (po) *po = pv;
}

// stateless, one workgroup per stream (k >= kWGMinK), as k2_segmented_wg.  GTAB: several threads read a
// slot's entry, so the gather loads the global table and a second pass puts the zeros back.
template <typename G, typename TabT, bool GTAB>
__global__ __launch_bounds__(64 * kWavesWG) void k2_segmented_rows_wg(
    const unsigned char* __restrict__ rows, const int64_t* __restrict__ offsets, int64_t S, uint32_t k, uint32_t C,
    uint32_t k0, uint32_t k1, uint64_t stream_base, unsigned char* __restrict__ out, int64_t* __restrict__ counts,
    uint32_t fifo_cap, TabT* __restrict__ gtab) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    build_lut((uint16_t*)lds, 256ull * k);
    const Wave W = wg_frame<GTAB>(lds, k, k0, k1, fifo_cap, gtab);
    TabT* tab = (TabT*)W.tab;
    const uint32_t nthr = 64u * kWavesWG;
    const uint64_t Wb = (uint64_t)C * sizeof(G);
    const PairStep p0 = pair_step(threadIdx.x, nthr, C);
    for (int64_t s = blockIdx.x; s < S; s += gridDim.x) {
        const int64_t off = uniform64(offsets[s]);
        const int64_t len = std::max<int64_t>(uniform64(offsets[s + 1]) - off, 0);
        if constexpr (!GTAB)
            for (uint32_t j = threadIdx.x; j < k; j += nthr) tab[j] = 0;
        __syncthreads();  // the table is zero (GTAB: the previous stream's second pass left it so)
        const uint64_t stream = stream_base + (uint64_t)s;
        if (len < kSmallLen) k2_part<TabT, true, GTAB, true>(W, tab, len, stream, W.wave, 0);
        else k2_part<TabT, false, GTAB, true>(W, tab, len, stream, W.wave, 0);
        if constexpr (GTAB) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");  // this wave's table atomics
        __syncthreads();
        if constexpr (GTAB) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");  // every wave's, before the gather
        auto src_of = [&](uint32_t j) -> int64_t {
            TabT wi;
            if constexpr (GTAB) wi = __hip_atomic_load(&tab[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            else wi = tab[j];
            return slot_source(wi, j, off, len);
        };
        gather_rows<G, true>(rows, out + (uint64_t)s * k * Wb, k, C, p0, src_of);
        if (threadIdx.x == 0) counts[s] = len < (int64_t)k ? len : (int64_t)k;
        __syncthreads();  // the gather has read the table before anyone zeroes it
        if constexpr (GTAB) {
            for (uint32_t j = threadIdx.x; j < k; j += nthr)
                __hip_atomic_store(&tab[j], (TabT)0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");  // the zeros, before the next stream's atomics
        }
    }
}

// resumed write-back, first pass (one thread per slot): the table entry becomes 1 + the segment-local
// row that slot j takes -- its winner w (0: none) or its fill index, where that is later than the row's
// idx -- else 0, and idx[j] is moved.  Only this thread reads or writes idx[j]; the second pass copies
// the rows the entries name.
template <typename TabT>
__device__ __forceinline__ void update_slot_rows(TabT* tab, int64_t n0, int64_t nend, uint32_t j,
                                                 int64_t* __restrict__ si) {
    const uint64_t w = tab[j];
    int64_t at = (int64_t)w;
    if (!w) at = ((int64_t)j >= n0 && (int64_t)j < nend) ? (int64_t)j : -1;  // a fill index of this segment
    TabT e = 0;
    if (at >= 0 && si[j] < at) {
        si[j] = at;
        e = (TabT)(at - n0 + 1);
    }
    tab[j] = e;
}

template <typename G>
__global__ __launch_bounds__(64 * kWaves) void k2_segmented_rows_update(
    const unsigned char* __restrict__ rows, const int64_t* __restrict__ offsets, const int64_t* __restrict__ ids,
    const int64_t* __restrict__ bases, int64_t B, int64_t S, uint32_t k, uint32_t C, uint32_t k0, uint32_t k1,
    uint64_t stream_base, unsigned char* __restrict__ state_rows, int64_t* __restrict__ state_idx,
    int64_t* __restrict__ state_next, uint32_t fifo_cap) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    build_lut((uint16_t*)lds, 256ull * k);
    __syncthreads();
    const Wave W = wave_frame(lds, k, k0, k1, fifo_cap);
    const uint32_t lane = W.lane;
    void* tab = W.tab;
    const uint64_t Wb = (uint64_t)C * sizeof(G);
    const PairStep p0 = pair_step(lane, 64, C);
    const int64_t wave_stride = (int64_t)gridDim.x * kWaves;
    for (int64_t b = (int64_t)blockIdx.x * kWaves + W.wave; b < B; b += wave_stride) {
        Segment g;
        if (!read_segment(g, offsets, ids, bases, state_next, b, S)) continue;
        const uint64_t stream = stream_base + (uint64_t)g.r;
        int64_t* si = state_idx + g.r * (int64_t)k;
        const bool small = g.nend < kSmallLen;
        if (small) {
            k2_stream<int64_t, true, false, true>(W, nullptr, g.off, g.len, stream, nullptr, g.n0);
            for (uint32_t j = lane; j < k; j += 64) update_slot_rows((uint32_t*)tab, g.n0, g.nend, j, si);
        } else {
            k2_stream<int64_t, false, false, true>(W, nullptr, g.off, g.len, stream, nullptr, g.n0);
            for (uint32_t j = lane; j < k; j += 64) update_slot_rows((uint64_t*)tab, g.n0, g.nend, j, si);
        }
        __builtin_amdgcn_wave_barrier();
        auto src_of = [&](uint32_t j) -> int64_t {
            const uint64_t e = small ? (uint64_t)((const uint32_t*)tab)[j] : ((const uint64_t*)tab)[j];
            return e ? g.off + (int64_t)e - 1 : -1;
        };
        gather_rows<G, false>(rows, state_rows + (uint64_t)g.r * k * Wb, k, C, p0, src_of);
        if (lane == 0 && state_next[g.r] < g.nend) state_next[g.r] = g.nend;
        __builtin_amdgcn_wave_barrier();  // the table is read before the next segment zeroes it
    }
}

// the workgroup form of k2_segmented_rows_update (k >= kWGMinK), as k2_segmented_update_wg
template <typename G>
__global__ __launch_bounds__(64 * kWavesWG) void k2_segmented_rows_update_wg(
    const unsigned char* __restrict__ rows, const int64_t* __restrict__ offsets, const int64_t* __restrict__ ids,
    const int64_t* __restrict__ bases, int64_t B, int64_t S, uint32_t k, uint32_t C, uint32_t k0, uint32_t k1,
    uint64_t stream_base, unsigned char* __restrict__ state_rows, int64_t* __restrict__ state_idx,
    int64_t* __restrict__ state_next, uint32_t fifo_cap) {
    using TabT = unsigned long long;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    build_lut((uint16_t*)lds, 256ull * k);
    const Wave W = wg_frame(lds, k, k0, k1, fifo_cap);
    TabT* tab = (TabT*)W.tab;
    const uint32_t nthr = 64u * kWavesWG;
    const uint64_t Wb = (uint64_t)C * sizeof(G);
    const PairStep p0 = pair_step(threadIdx.x, nthr, C);
    for (int64_t b = blockIdx.x; b < B; b += gridDim.x) {
        Segment g;
        if (!read_segment(g, offsets, ids, bases, state_next, b, S)) continue;
        for (uint32_t j = threadIdx.x; j < k; j += nthr) tab[j] = 0;
        __syncthreads();  // the table is zero, the lut built, and n0 read by every wave
        const uint64_t stream = stream_base + (uint64_t)g.r;
        if (g.nend < kSmallLen) k2_part<TabT, true, false, true>(W, tab, g.len, stream, W.wave, g.n0);
        else k2_part<TabT, false, false, true>(W, tab, g.len, stream, W.wave, g.n0);
        __syncthreads();
        int64_t* si = state_idx + g.r * (int64_t)k;
        for (uint32_t j = threadIdx.x; j < k; j += nthr) update_slot_rows(tab, g.n0, g.nend, j, si);
        __syncthreads();  // every slot's entry names its row (or none)
        auto src_of = [&](uint32_t j) -> int64_t {
            const uint64_t e = tab[j];
            return e ? g.off + (int64_t)e - 1 : -1;
        };
        gather_rows<G, false>(rows, state_rows + (uint64_t)g.r * k * Wb, k, C, p0, src_of);
        if (threadIdx.x == 0 && state_next[g.r] < g.nend) state_next[g.r] = g.nend;
        __syncthreads();  // the write-back has read the table before the next segment zeroes it
    }
}

// ---- resumed over byte keys, through a permutation (rsv_sample_segmented_rows_update_indirect) ----
// update_slot_rows with the segment's rows at rows[order[off ...]]: the entry becomes 1 + the BATCH position
// of the row the slot takes (an int32 entry of `order`, so it fits the 32-bit table too), read through
// order_at here, in the first pass, so that a slot whose entry is bad keeps its idx as well as its row.
template <typename TabT>
__device__ __forceinline__ void update_slot_rows_indirect(TabT* tab, const int32_t* __restrict__ order, int64_t n_rows,
                                                          int64_t off, int64_t n0, int64_t nend, uint32_t j,
                                                          int64_t* __restrict__ si) {
    const uint64_t w = tab[j];
    int64_t at = (int64_t)w;
    if (!w) at = ((int64_t)j >= n0 && (int64_t)j < nend) ? (int64_t)j : -1;  // a fill index of this segment
    TabT e = 0;
    if (at >= 0 && si[j] < at) {
        const int64_t q = order_at(order, off + (at - n0), n_rows);
        if (q >= 0) {
            si[j] = at;
            e = (TabT)(q + 1);
        }
    }
    tab[j] = e;
}

template <typename G>
__global__ __launch_bounds__(64 * kWaves) void k2_segmented_rows_update_indirect(
    const unsigned char* __restrict__ rows, int64_t n_rows, const int32_t* __restrict__ order,
    const int64_t* __restrict__ offsets, const int64_t* __restrict__ ids, const int64_t* __restrict__ bases, int64_t B,
    int64_t S, uint32_t k, uint32_t C, uint32_t k0, uint32_t k1, uint64_t stream_base,
    unsigned char* __restrict__ state_rows, int64_t* __restrict__ state_idx, int64_t* __restrict__ state_next,
    uint32_t fifo_cap) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    build_lut((uint16_t*)lds, 256ull * k);
    __syncthreads();
    const Wave W = wave_frame(lds, k, k0, k1, fifo_cap);
    const uint32_t lane = W.lane;
    void* tab = W.tab;
    const uint64_t Wb = (uint64_t)C * sizeof(G);
    const PairStep p0 = pair_step(lane, 64, C);
    const int64_t wave_stride = (int64_t)gridDim.x * kWaves;
    for (int64_t b = (int64_t)blockIdx.x * kWaves + W.wave; b < B; b += wave_stride) {
        Segment g;
        if (!read_segment(g, offsets, ids, bases, state_next, b, S)) continue;
        const uint64_t stream = stream_base + (uint64_t)g.r;
        int64_t* si = state_idx + g.r * (int64_t)k;
        const bool small = g.nend < kSmallLen;
        if (small) {
            k2_stream<int64_t, true, false, true>(W, nullptr, g.off, g.len, stream, nullptr, g.n0);
            for (uint32_t j = lane; j < k; j += 64)
                update_slot_rows_indirect((uint32_t*)tab, order, n_rows, g.off, g.n0, g.nend, j, si);
        } else {
            k2_stream<int64_t, false, false, true>(W, nullptr, g.off, g.len, stream, nullptr, g.n0);
            for (uint32_t j = lane; j < k; j += 64)
                update_slot_rows_indirect((uint64_t*)tab, order, n_rows, g.off, g.n0, g.nend, j, si);
        }
        __builtin_amdgcn_wave_barrier();
        auto src_of = [&](uint32_t j) -> int64_t {
            const uint64_t e = small ? (uint64_t)((const uint32_t*)tab)[j] : ((const uint64_t*)tab)[j];
            return (int64_t)e - 1;
        };
        gather_rows<G, false>(rows, state_rows + (uint64_t)g.r * k * Wb, k, C, p0, src_of);
        if (lane == 0 && state_next[g.r] < g.nend) state_next[g.r] = g.nend;
        __builtin_amdgcn_wave_barrier();  // the table is read before the next segment zeroes it
    }
}

// the workgroup form (k >= kWGMinK), as k2_segmented_rows_update_wg
template <typename G>
__global__ __launch_bounds__(64 * kWavesWG) void k2_segmented_rows_update_indirect_wg(
    const unsigned char* __restrict__ rows, int64_t n_rows, const int32_t* __restrict__ order,
    const int64_t* __restrict__ offsets, const int64_t* __restrict__ ids, const int64_t* __restrict__ bases, int64_t B,
    int64_t S, uint32_t k, uint32_t C, uint32_t k0, uint32_t k1, uint64_t stream_base,
    unsigned char* __restrict__ state_rows, int64_t* __restrict__ state_idx, int64_t* __restrict__ state_next,
    uint32_t fifo_cap) {
    using TabT = unsigned long long;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    build_lut((uint16_t*)lds, 256ull * k);
    const Wave W = wg_frame(lds, k, k0, k1, fifo_cap);
    TabT* tab = (TabT*)W.tab;
    const uint32_t nthr = 64u * kWavesWG;
    const uint64_t Wb = (uint64_t)C * sizeof(G);
    const PairStep p0 = pair_step(threadIdx.x, nthr, C);
    for (int64_t b = blockIdx.x; b < B; b += gridDim.x) {
        Segment g;
        if (!read_segment(g, offsets, ids, bases, state_next, b, S)) continue;
        for (uint32_t j = threadIdx.x; j < k; j += nthr) tab[j] = 0;
        __syncthreads();  // the table is zero, the lut built, and n0 read by every wave
        const uint64_t stream = stream_base + (uint64_t)g.r;
        if (g.nend < kSmallLen) k2_part<TabT, true, false, true>(W, tab, g.len, stream, W.wave, g.n0);
        else k2_part<TabT, false, false, true>(W, tab, g.len, stream, W.wave, g.n0);
        __syncthreads();
        int64_t* si = state_idx + g.r * (int64_t)k;
        for (uint32_t j = threadIdx.x; j < k; j += nthr)
            update_slot_rows_indirect(tab, order, n_rows, g.off, g.n0, g.nend, j, si);
        __syncthreads();  // every slot's entry names its row (or none)
        auto src_of = [&](uint32_t j) -> int64_t { return (int64_t)tab[j] - 1; };
        gather_rows<G, false>(rows, state_rows + (uint64_t)g.r * k * Wb, k, C, p0, src_of);
        if (threadIdx.x == 0 && state_next[g.r] < g.nend) state_next[g.r] = g.nend;
        __syncthreads();  // the write-back has read the table before the next segment zeroes it
    }
}

// rsv_sample_segmented_rows_merge: a workgroup takes 256 (row, slot) entries.  First pass, one thread per
// entry: the part with the largest idx, if it beats the state's (only this thread reads or writes the
// entry's idx), into LDS; second pass: the winning parts' rows by (entry, granule) pairs.
template <typename G>
__global__ __launch_bounds__(256) void k2_segmented_rows_merge(const unsigned char* part_rows, const int64_t* part_idx,
                                                               const int64_t* part_next, int32_t P, int64_t S,
                                                               uint32_t k, uint32_t C, unsigned char* state_rows,
                                                               int64_t* state_idx, int64_t* state_next) {
    __shared__ int32_t win[256];
    const int64_t total = S * (int64_t)k;
    const int64_t t0 = (int64_t)blockIdx.x * 256, t = t0 + threadIdx.x;
    win[threadIdx.x] = t < total ? merge_pick(part_idx, part_next, P, S, k, t, state_idx, state_next, [](int32_t) {}) : -1;
    __syncthreads();
    const uint32_t here = (uint32_t)std::min<int64_t>(256, total - t0);
    // source row of entry t0 + j: entry t0 + j of part win[j]
    auto src_of = [&](uint32_t j) -> int64_t {
        const int32_t p = win[j];
        return p >= 0 ? (int64_t)p * total + t0 + (int64_t)j : -1;
    };
    gather_rows<G, false>(part_rows, state_rows + (uint64_t)t0 * C * sizeof(G), here, C, pair_step(threadIdx.x, 256, C),
                          src_of);
}

}  // namespace k2
}  // namespace rsv
