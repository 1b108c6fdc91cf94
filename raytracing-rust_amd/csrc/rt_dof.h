// rt_dof.h -- launch interface of the depth-of-field stage kernels (rt_dof.hip), shared with rt_api_post.cpp.
#pragma once

#include <stdint.h>
#include <hip/hip_runtime.h>

#include "../../include/rt_hip.h"

namespace rt {

constexpr uint32_t kDofMaxRadius = 16;            // the largest max_radius: the gather's LDS is sized for it
constexpr uint32_t kDofTileW = 32, kDofTileH = 8; // the output tile of one gather workgroup (one pixel per lane)
constexpr uint32_t kDofMaxTiles = 2048;           // the gather grid: at most this many workgroups, grid-stride beyond
constexpr uint32_t kDofMaxBlocks = 1024;          // the circle-of-confusion grid (256 pixels per workgroup and trip)
// the footprint of one tile at the largest radius: 64 x 40 pixels of (r, g, b, radius, depth key), 20 bytes each: 51 200 bytes
constexpr uint32_t kDofFootPixels = (kDofTileW + 2u * kDofMaxRadius) * (kDofTileH + 2u * kDofMaxRadius);
constexpr uint32_t kDofWorkspaceBytesPerPixel = 8; // (radius, depth key), both f32

// the workspace of a W x H frame: one (radius, depth key) pair per pixel, the size rounded up to 16 bytes
inline uint64_t dof_workspace_bytes(uint64_t n_pixels) { return (kDofWorkspaceBytesPerPixel * n_pixels + 15u) / 16u * 16u; }

struct DevDofParams {
	uint32_t width, height;
	float focus_distance, blur_scale;
	uint32_t max_radius;
	uint32_t planar; // z = t * cosine of the pixel-centre ray to the camera's forward axis (cam holds the camera); 0: z = t
	float cam[12];   // origin, lower_left, horizontal, vertical
	const float *rgb;
	const float *depth;
	float2 *ws;
	float *out;
	float *coc; // NULL: not wanted
};

// both kernels on `stream`: no allocation, no synchronisation
hipError_t launch_dof(hipStream_t stream, const DevDofParams &P);

} // namespace rt
