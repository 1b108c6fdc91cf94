// rt_aov.h -- launch interface of the first-hit AOV kernel (rt_aov.hip), shared with rt_api_post.cpp.
#pragma once

#include "rt_types.h"

namespace rt {

// channels of rt_aov_buffers a launch writes (bit set = pointer non-null)
enum : uint32_t {
	kAovAlbedo = 1u,
	kAovNormal = 2u,
	kAovDepth = 4u,
	kAovCoverage = 8u,
	kAovPrimitive = 16u,
	kAovMaterial = 32u
};

struct DevAovParams {
	DevCamera cam;
	uint32_t width, height;
	uint32_t tiles_x, n_tiles;  // 8 x 8 pixel tiles, row-major; one wave per tile
	uint32_t spp;
	uint32_t mask;              // kAov* bits
	uint32_t seed_lo, seed_hi;
	uint32_t sample_begin_lo, sample_begin_hi;
	const uint32_t *prim_desc;  // BVH slot -> index in rt_scene_desc.primitives (needed only for kAovPrimitive)
	float *albedo, *normal, *depth, *coverage;
	uint32_t *primitive, *material;
};

// (the whole worst-case traversal stack of a 256-thread workgroup in LDS: four_wave_stack_lds_bytes, rt_types.h)
hipError_t launch_aov(bool prune, hipStream_t stream, const DevScene &S, const DevAovParams &P);

} // namespace rt
