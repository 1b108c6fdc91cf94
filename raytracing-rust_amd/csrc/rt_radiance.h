// rt_radiance.h -- launch interface of the radiance-query kernels (rt_radiance.hip), shared with rt_api_query.cpp.
#pragma once

#include "rt_types.h"

namespace rt {

struct DevRadianceParams {
	const float *rays;       // n_rays x (origin[3], direction[3]): rt_ray_desc, 4-byte aligned
	const uint64_t *streams; // n_rays or null (stream i = i)
	float *out;              // 3 * n_rays
	uint32_t n_rays;         // below 2^31 (the host refuses more)
	uint32_t samples;        // K >= 1
	uint32_t seed_lo, seed_hi, sample_begin_lo, sample_begin_hi;
	uint32_t max_depth, rr_threshold;
};

// waves per SIMD the kernels are compiled for (their __launch_bounds__): with the LDS of the stacks, what a CU holds of them
constexpr uint32_t kRadianceWaves = 4;

// `groups` 256-thread workgroups (the host sizes them: rt_api_internal.h path_lane_groups); every wave works through the 64-ray
// blocks wave, wave + waves, ... of the batch.  (the whole worst-case traversal stack of a workgroup in LDS: four_wave_stack_lds_bytes)
hipError_t launch_radiance(int method, bool prune, hipStream_t stream, const DevScene &S, const DevRadianceParams &P, uint32_t groups);

} // namespace rt
