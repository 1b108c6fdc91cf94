// rt_adaptive.h -- launch interface of the tile-list render and the active-tile selection (rt_adaptive.hip), shared with
// rt_api_post.cpp.
#pragma once

#include "rt_types.h"

namespace rt {

struct DevTilesParams {
	DevCamera cam;
	const uint32_t *tiles; // n_tiles indices into the 8 x 8 tile grid of the frame (rt_noise_tiles' grid)
	float *out;            // the FRAME, 3 * width * height: only the listed pixels are written
	float *chunk_sums;     // [split][64 * n_tiles][3] or null
	unsigned long long *rays_shot; // or null; zeroed ahead of the launch (launch_tiles)
	uint32_t n_tiles;      // list length
	uint32_t width, height, tiles_x, tile_count; // tile_count = tiles_x * ceil(height / 8): an index at or past it is skipped
	uint32_t spp, split;   // split resolved, 1 <= split <= spp
	uint32_t item_chunks;  // chunks one work item folds: 1 when the sums go to chunk_sums, else split (the whole pixel)
	uint32_t n_lanes;      // 64 * items, items = n_tiles * split / item_chunks; below 2^31 (the host refuses more)
	uint32_t seed_lo, seed_hi, sample_begin_lo, sample_begin_hi;
	uint32_t max_depth, rr_threshold;
};

struct DevSelectParams {
	const float *tile_error; // n_tiles
	uint32_t *tiles;         // n_tiles: the indices with tile_error > threshold, ascending
	uint32_t *count;         // how many
	uint32_t n_tiles;
	float threshold;
};

// One masked batch of rt_render_adaptive folded into the per-pixel state: one wave a listed tile, one lane a pixel.  The chunk sums
// are rt_render_tiles' ([chunk][64 * slot + place][3]); (lbar_b, var_b) are chunk_stats' and the step M += mean_b, L += lbar_b,
// V += var_b with the planes divided out is chunk_state_step's (rt_chunk_stats.h: the routines noise_chunk_kernel calls), here with
// the pixel's own nb, which it counts up.
struct DevFoldParams {
	const uint32_t *tiles;
	uint32_t n_tiles;      // list length
	uint32_t width, height, tiles_x, tile_count;
	uint32_t split;        // S, 2..64
	uint32_t chunk_passes; // batch / S
	const float *sums;     // 3 * split * 64 * n_tiles
	const float *albedo;   // 3 * w * h or null
	const float *mean_in;  // 3 * w * h: the frame rt_render_tiles wrote (listed pixels)
	float *state_m, *state_l, *state_v;
	uint32_t *nb;          // w * h: batches folded per pixel
	float *out_mean, *out_lum, *out_var;
};
hipError_t launch_adaptive_fold(hipStream_t stream, const DevFoldParams &P);
// n words = value (the per-pixel batch count after a whole-frame batch)
hipError_t launch_fill_u32(hipStream_t stream, uint32_t *p, uint64_t n, uint32_t value);

// waves per SIMD tiles_kernel is compiled for (as radiance_kernel: with the LDS of the stacks, what a CU holds of them)
constexpr uint32_t kTilesWaves = 4;
// dynamic LDS of a workgroup behind its four_wave_stack_lds_bytes: the fold records of its 256 lanes (rt_adaptive.hip: eleven words
// a lane -- what a pixel's fold carries between passes waits there, not in registers the integrator needs)
constexpr uint32_t kTilesRecordWords = 11;
constexpr size_t kTilesRecordLdsBytes = kTilesRecordWords * 256u * sizeof(uint32_t);

// the counter zeroed by a kernel, `groups` 256-thread workgroups of tiles_kernel (the host sizes them: rt_api_internal.h
// path_lane_groups) and, when the sums went to chunk_sums, the combine of the listed pixels
hipError_t launch_tiles(int method, bool prune, hipStream_t stream, const DevScene &S, const DevTilesParams &P, uint32_t groups);
hipError_t launch_select_tiles(hipStream_t stream, const DevSelectParams &P);

} // namespace rt
