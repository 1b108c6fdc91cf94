// rt_lens.h -- launch interface of the lens-camera render (rt_lens.hip), shared with rt_api_lens.cpp.
#pragma once

#include "rt_types.h"

namespace rt {

// rt_projection (include/rt_hip.h; rt_api_lens.cpp asserts the values)
constexpr int32_t kProjPerspective = 0, kProjOrthographic = 1, kProjFisheye = 2, kProjEquirect = 3;

// rt_lens_camera as the kernel takes it, then the frame and the fold of rt_render_opts (the fields of DevTilesParams without a list)
struct DevLensParams {
	DevCamera cam;                       // rt_lens_camera.pinhole
	float right[3], up[3], forward[3];   // SimpleCamera::new's u, v and -w
	float lens_radius;                   // PERSPECTIVE: 0 = no lens draw and no lens arithmetic
	float fisheye_half_angle;            // FISHEYE
	int32_t projection;                  // rt_projection, checked by the host
	float *out;                          // the frame, 3 * width * height: every pixel is written
	float *chunk_sums;                   // [split][64 * n_tiles][3] or null
	unsigned long long *rays_shot;       // or null; zeroed ahead of the launch (launch_lens)
	uint32_t width, height, tiles_x, n_tiles; // the 8 x 8 grid of the frame: n_tiles = tiles_x * ceil(height / 8)
	uint32_t spp, split;                 // split resolved, 1 <= split <= spp
	uint32_t item_chunks;                // chunks one work item folds: 1 when the sums go to chunk_sums, else split (the whole pixel)
	uint32_t n_lanes;                    // 64 * items, items = n_tiles * split / item_chunks; below 2^31 (the host refuses more)
	uint32_t seed_lo, seed_hi, sample_begin_lo, sample_begin_hi;
	uint32_t max_depth, rr_threshold;
};

// waves per SIMD lens_kernel is compiled for (as tiles_kernel: with the LDS of the stacks, what a CU holds of them)
constexpr uint32_t kLensWaves = 4;
// dynamic LDS of a workgroup behind its four_wave_stack_lds_bytes: the fold records of its 256 lanes (rt_lens.hip: eleven words a
// lane, tiles_kernel's record)
constexpr uint32_t kLensRecordWords = 11;
constexpr size_t kLensRecordLdsBytes = kLensRecordWords * 256u * sizeof(uint32_t);

// the counter zeroed by a kernel, `groups` 256-thread workgroups of lens_kernel (the host sizes them: rt_api_internal.h
// path_lane_groups) and, when the sums went to chunk_sums, the combine of the frame
hipError_t launch_lens(int method, bool prune, hipStream_t stream, const DevScene &S, const DevLensParams &P, uint32_t groups);

} // namespace rt
