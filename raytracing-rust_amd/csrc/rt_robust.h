// rt_robust.h -- launch interface of the firefly-robust combine (rt_robust.hip), shared with rt_api_post.cpp.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace rt {

constexpr uint32_t kRobustMaxSplit = 64u;     // the most chunks a pixel is ranked over (rt_robust_opts)
constexpr uint32_t kRobustBlockThreads = 128u; // two waves: 40 KB of LDS at 64 chunks, below the 64 KB a launch gets unasked

// The S chunk sums of a frame -> the rank-trimmed mean of include/rt_hip.h (rt_robust_opts).  Two addressing modes:
//   tile_w != 0  the scene's partial buffer, [chunk][work item][3] in the render kernel's tile work order for RT_LAYOUT_FRAME and
//                shard_count 1 (frame_work_pixel, rt_chunk_stats.h)
//   tile_w == 0  the caller's planes, [chunk][h][w][3] in frame raster: work item = pixel, n_work = width * height
struct DevRobustParams {
	uint32_t width, height, tile_w, tile_h, tiles_x;
	uint32_t n_work;       // work items per chunk, edge-tile padding included
	uint32_t split;        // S, 2..kRobustMaxSplit
	uint32_t chunk_passes; // n
	int32_t mode;          // rt_robust_mode
	uint32_t trim;
	float gini_gain;
	const float *sums;     // 3 * split * n_work
	const float *albedo;   // 3 * w * h or null
	float *out;            // 3 * w * h
	float *mean;           // 3 * w * h or null: the plain combine
	float *gini;           // w * h or null
	uint8_t *trimmed, *dropped; // w * h each or null
};

hipError_t launch_robust_chunks(hipStream_t stream, const DevRobustParams &P);

} // namespace rt
