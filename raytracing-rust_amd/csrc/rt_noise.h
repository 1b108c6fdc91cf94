// rt_noise.h -- launch interface of the noise-estimate kernels (rt_noise.hip), shared with rt_api_post.cpp.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace rt {

constexpr uint32_t kNoiseMaxSplit = 64u;          // the largest sample_split an estimate is taken from (rt_noise_opts)
constexpr uint32_t kNoiseTileGridBlocks = 2048u;  // the tile kernel's grid: four tiles per workgroup, then it strides
constexpr uint32_t kNoiseSummaryBytes = 16u;      // rt_noise_summary

// Stage one: the chunk sums of ONE render at sample_split = split (the scene's partial buffer, [chunk][work item][3]) -> lbar and
// var of that render, added to the state of a batch sequence and divided out.  The work item -> pixel map is the render kernel's
// for RT_LAYOUT_FRAME and shard_count 1 (frame_work_pixel, rt_chunk_stats.h; the host fills it from frame_tiling, rt_api_internal.h).
struct DevNoiseChunkParams {
	uint32_t width, height, tile_w, tile_h, tiles_x;
	uint32_t n_work;       // work items per chunk, edge-tile padding included
	uint32_t split;        // S, 2..kNoiseMaxSplit
	uint32_t chunk_passes; // n = spp / S
	uint32_t fresh;        // 1: the state starts from this batch (stored), 0: this batch is added to it
	float batches;         // nb, this batch included: what the outputs are divided by
	const float *partial;  // 3 * split * n_work
	const float *albedo;   // 3 * w * h or null
	const float *mean_in;  // 3 * w * h: this render's mean as combine_chunks_kernel wrote it; may be out_mean itself
	float *state_m, *state_l, *state_v; // 3 / 1 / 1 * w * h, or all null: one batch, nothing kept
	float *out_mean, *out_lum, *out_var; // M / nb, L / nb, V / (nb * nb); each may be null
};

// Stage two: per 8 x 8 tile the mean relative error, and the frame summary.
struct DevNoiseTileParams {
	uint32_t width, height, tiles_x, n_tiles;
	float luminance_floor, threshold;
	const float *lum_mean, *variance; // w * h each
	float *tile_error;                // n_tiles or null
	uint32_t *summary;                // 4 words (rt_noise_summary), zeroed before the launch, or null
};

hipError_t launch_noise_chunks(hipStream_t stream, const DevNoiseChunkParams &P);
hipError_t launch_noise_tiles(hipStream_t stream, const DevNoiseTileParams &P);

} // namespace rt
