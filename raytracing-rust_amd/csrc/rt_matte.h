// rt_matte.h -- launch interface of the ID-matte kernels (rt_matte.hip), shared with rt_api_post.cpp.
#pragma once

#include "rt_aov.h"

namespace rt {

constexpr uint32_t kMatteSlots = 8u;          // RT_MATTE_SLOTS (include/rt_hip.h): (id, count) slots per pixel, and the most layers
constexpr uint64_t kMatteMaxIds = 1ull << 20; // largest selection rt_matte_extract takes

struct DevMatteParams {
	DevAovParams A;     // the camera, the frame, the pass window and prim_desc as the first-hit pass takes them (mask and channels unused)
	uint32_t id_kind;   // rt_matte_id_kind
	uint32_t layers;    // K, 1..kMatteSlots
	uint32_t *ids;      // K * w * h, layer-major
	float *coverage;    // K * w * h
	float *residual;    // w * h or null
};

struct DevMatteExtractParams {
	const uint32_t *ids;   // K * n_px
	const float *coverage; // K * n_px
	const uint32_t *sel;   // n_sel selected IDs, ascending
	uint32_t n_sel;        // <= kMatteMaxIds
	uint32_t layers;       // K
	uint32_t n_px;         // <= 2^31
	float *out;            // n_px
};

// (the whole worst-case traversal stack of a 256-thread workgroup in LDS: four_wave_stack_lds_bytes, rt_types.h)
hipError_t launch_matte(bool prune, hipStream_t stream, const DevScene &S, const DevMatteParams &P);
hipError_t launch_matte_extract(hipStream_t stream, const DevMatteExtractParams &P);

} // namespace rt
