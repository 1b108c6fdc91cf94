// rt_ao.h -- launch interface of the ambient-occlusion kernel (rt_ao.hip), shared with rt_api_post.cpp.
#pragma once

#include "rt_aov.h"

namespace rt {

constexpr uint32_t kAoMaxRays = 64u; // most AO rays per pass (rt_ao_opts.rays_per_pass)

struct DevAoParams {
	DevAovParams A;         // the camera, the frame and the pass window as the first-hit pass takes them (mask and channels unused)
	uint32_t rays_per_pass; // K, 1..kAoMaxRays
	float t_limit;          // NaN: no limit (radius 0); else the radius, +inf included
	float *visibility;      // w * h or null
	float *bent_normal;     // 3 * w * h or null
};

// (the whole worst-case traversal stack of a 256-thread workgroup in LDS: four_wave_stack_lds_bytes, rt_types.h)
hipError_t launch_ao(bool prune, hipStream_t stream, const DevScene &S, const DevAoParams &P);

} // namespace rt
