// rt_bloom.h -- launch interface of the bloom stage kernels (rt_bloom.hip), shared with rt_api_post.cpp.
#pragma once

#include <stdint.h>
#include <hip/hip_runtime.h>

#include "../../include/rt_hip.h"

namespace rt {

constexpr uint32_t kBloomMaxLevels = 12;
constexpr uint32_t kBloomTileW = 32, kBloomTileH = 8; // the output tile of one reduce workgroup (one pixel per lane)
constexpr uint32_t kBloomMaxTiles = 1024;             // the reduce grid: at most this many workgroups, grid-stride beyond
constexpr uint32_t kBloomMaxBlocks = 1024;            // the expand and composite grids (256 pixels per workgroup and trip)
// the fused tail keeps every level it owns in LDS, 12 bytes per pixel: 48 KB, what a launch gets without asking for more
constexpr uint32_t kBloomTailPixels = 4096;

// The pyramid of a W x H frame: level i is ceil(w/2) x ceil(h/2) of level i - 1 (of the frame for i = 0), n = min(levels, the
// levels up to and including the first of 1 x 1).  Each level is one RGB f32 image (12 bytes per pixel) in the workspace, its
// size rounded up to 16 bytes.
struct BloomLevels {
	uint32_t n;
	uint32_t w[kBloomMaxLevels], h[kBloomMaxLevels];
	uint64_t offset[kBloomMaxLevels]; // bytes into the workspace
	uint64_t bytes;                   // the workspace
	// the first level of the fused tail: the smallest t >= 1 whose levels t .. n-1 together hold at most kBloomTailPixels
	// pixels; n when there is none (n == 1)
	uint32_t tail_from;
};

inline BloomLevels bloom_levels(uint32_t W, uint32_t H, uint32_t levels)
{
	BloomLevels L{};
	uint32_t w = W, h = H;
	while (L.n < levels && L.n < kBloomMaxLevels) {
		w = (w + 1u) / 2u;
		h = (h + 1u) / 2u;
		L.w[L.n] = w;
		L.h[L.n] = h;
		L.offset[L.n] = L.bytes;
		L.bytes += (12ull * w * h + 15u) / 16u * 16u;
		++L.n;
		if (w == 1u && h == 1u)
			break;
	}
	L.tail_from = L.n;
	uint64_t px = 0;
	for (uint32_t i = L.n; i-- > 1u;) {
		px += (uint64_t)L.w[i] * L.h[i];
		if (px > kBloomTailPixels)
			break;
		L.tail_from = i;
	}
	return L;
}

struct DevBloomParams {
	uint32_t width, height;
	float threshold, knee, intensity, scatter, exposure_ev, clamp_max;
	uint32_t fuse_tail;
	const float *rgb;
	const rt_display_state *state; // NULL: ev = exposure_ev
	char *ws;
	float *out;
};

// the whole chain on `stream`: no allocation, no synchronisation
hipError_t launch_bloom(hipStream_t stream, const DevBloomParams &P, const BloomLevels &L);

} // namespace rt
