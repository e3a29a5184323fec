// rsv_k2_indexed.h -- the keyless K2 kernels (rsv_sample_segmented_indexed / _update / _merge), declared.
// rsv_indexed.hip defines them over rsv_k2.h's element loops and frames; rsv_segmented.hip launches them.  They
// are a translation unit of their own so that the keyed kernels of rsv_segmented.hip compile from the text they
// were measured with: defined beside them, these kernels moved the register allocation of two of the
// k2_segmented_rows_wg instantiations.
#pragma once
#include <cstdint>

#include <hip/hip_runtime.h>

namespace rsv {
namespace k2 {

// the device list of the streams whose pieces 1.. the second kernel of the split form takes
struct SplitList {
    unsigned long long* count;  // appends so far; beyond cap nothing was recorded
    int64_t* ent;               // cap x (stream, len)
    uint32_t cap;
    int64_t C;                  // the split length, a multiple of 1024; 0: no stream is split
};

// stateless: one wave per stream (k < kWGMinK), and the pieces of the streams it recorded
__global__ void k2_indexed(const int64_t* __restrict__ offsets, int64_t S, uint32_t k, uint32_t k0, uint32_t k1,
                           uint64_t stream_base, int64_t* __restrict__ out_idx, int64_t* __restrict__ counts,
                           uint32_t fifo_cap, SplitList sl);
__global__ void k2_indexed_pieces(uint32_t k, uint32_t k0, uint32_t k1, uint64_t stream_base, int64_t* out_idx,
                                  uint32_t fifo_cap, SplitList sl);
// stateless: one workgroup per stream (TabT: uint32_t or unsigned long long; GT: the table in global scratch)
template <typename TabT, bool GT>
__global__ void k2_indexed_wg(const int64_t* __restrict__ offsets, int64_t S, uint32_t k, uint32_t k0, uint32_t k1,
                              uint64_t stream_base, int64_t* __restrict__ out_idx, int64_t* __restrict__ counts,
                              uint32_t fifo_cap, TabT* __restrict__ gtab, SplitList sl);
template <typename TabT>
__global__ void k2_indexed_pieces_wg(uint32_t k, uint32_t k0, uint32_t k1, uint64_t stream_base, int64_t* out_idx,
                                     uint32_t fifo_cap, SplitList sl);
// resumed: the wave and the workgroup form
__global__ void k2_indexed_update(const int64_t* __restrict__ offsets, const int64_t* __restrict__ ids,
                                  const int64_t* __restrict__ bases, int64_t B, int64_t S, uint32_t k, uint32_t k0,
                                  uint32_t k1, uint64_t stream_base, int64_t* __restrict__ state_idx,
                                  int64_t* __restrict__ state_next, int64_t* __restrict__ hits,
                                  int64_t* __restrict__ hit_counts, uint32_t fifo_cap);
__global__ void k2_indexed_update_wg(const int64_t* __restrict__ offsets, const int64_t* __restrict__ ids,
                                     const int64_t* __restrict__ bases, int64_t B, int64_t S, uint32_t k, uint32_t k0,
                                     uint32_t k1, uint64_t stream_base, int64_t* __restrict__ state_idx,
                                     int64_t* __restrict__ state_next, int64_t* __restrict__ hits,
                                     int64_t* __restrict__ hit_counts, uint32_t fifo_cap);
__global__ void k2_indexed_merge(const int64_t* part_idx, const int64_t* part_next, int32_t P, int64_t S, uint32_t k,
                                 int64_t* state_idx, int64_t* state_next, int32_t* src);

}  // namespace k2
}  // namespace rsv
