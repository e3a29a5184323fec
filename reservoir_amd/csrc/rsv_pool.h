// rsv_pool.h -- the resource pool (rsv_pool.hip): device / pinned host blocks, streams, events.
// Engines own their blocks through the buffer types of rsv_buffers.h; only those (and the runtime's
// slot block) call the block functions below.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>

namespace rsv {

// Allocation is on the current device.  A buffer may only be released once no queued work can
// touch it (synchronize its stream first).
hipError_t pool_device_alloc(void** p, size_t bytes);
void pool_device_free(void* p);
// Replace *p (old_bytes in use) by a block of new_bytes, its contents kept when `keep`; the stream is
// synchronized before the old block goes back to the pool.  *p is unchanged on failure.
hipError_t pool_device_grow(void** p, size_t old_bytes, size_t new_bytes, bool keep, hipStream_t st);
// Capacity for `need` entries: `cur` (at least 1024) doubled until it holds them, at most `cap`.
int64_t grown_capacity(int64_t cur, int64_t need, int64_t cap);
hipError_t pool_host_alloc(void** p, size_t bytes, unsigned flags);
// a coherent, device-mapped host block and its device alias
hipError_t pool_host_alloc_mapped(void** p, void** dev_alias, size_t bytes);
void pool_host_free(void* p);
void pool_trim();  // free every idle cached buffer
hipError_t pool_stream(hipStream_t* out);  // non-blocking stream of the current device
void pool_release_stream(int device, hipStream_t st);
hipError_t pool_event(hipEvent_t* out, unsigned flags);
void pool_release_event(int device, hipEvent_t e, unsigned flags);

}  // namespace rsv
