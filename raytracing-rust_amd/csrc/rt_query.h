// rt_query.h -- what rt_query.hip exports to rt_api_query.cpp: the launchers of the batch hit queries and of the trace queue.
#pragma once
#include <hip/hip_runtime.h>
#include "rt_types.h"

namespace rt {
hipError_t launch_check_hit(bool prune, hipStream_t stream, const DevScene &S, const void *rays, uint64_t n, void *out);
hipError_t launch_check_hit_index(bool prune, hipStream_t stream, const DevScene &S, const void *rays, const void *object_index,
                                  uint64_t n, void *out);
#ifdef RT_STATS
hipError_t launch_trace_queue(int waves, uint32_t n_blocks, size_t lds_bytes, hipStream_t stream, const DevScene &S, const void *rays, uint32_t n, void *out,
                              uint32_t *counter, unsigned long long *steps, uint32_t cap, uint32_t ovf_depth, uint32_t *ovf);
#endif
} // namespace rt
