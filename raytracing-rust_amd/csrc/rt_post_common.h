// rt_post_common.h -- the few device helpers the post-processing kernels share (denoiser, temporal accumulation, display, bloom,
// upscaler, noise estimates, robust frames): one copy each, with internal linkage like the private copies they replace.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace rt {

namespace {

constexpr uint32_t kMaxBlocks = 65536; // grid-stride beyond this (tall one-column frames)

// Rec. 709 luminance, as written: (0.2126 r + 0.7152 g) + 0.0722 b, no fma (host too: rt_chunk_stats.h is checked there)
__host__ __device__ inline float lum(float r, float g, float b) { return 0.2126f * r + 0.7152f * g + 0.0722f * b; }

__device__ inline bool finite3(float a, float b, float c) { return __builtin_isfinite(a) && __builtin_isfinite(b) && __builtin_isfinite(c); }

// pixel of this lane in 16 x 16 tile `tile`: wave w takes the 8 x 8 quadrant (w & 1, w >> 1), lane l the pixel (l & 7, l >> 3)
__device__ inline void tile_pixel(uint32_t tile, uint32_t tiles_x, uint32_t &x, uint32_t &y)
{
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	x = (tile % tiles_x) * 16u + (wave & 1u) * 8u + (lane & 7u);
	y = (tile / tiles_x) * 16u + (wave >> 1) * 8u + (lane >> 3);
}

} // namespace

} // namespace rt
