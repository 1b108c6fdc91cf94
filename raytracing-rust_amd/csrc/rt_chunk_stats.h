// rt_chunk_stats.h -- what every stage that reads the per-chunk sums of a render at sample_split = S does with them (noise
// estimates, rt_noise.hip; the fold of a masked batch, rt_adaptive.hip; robust frames, rt_robust.hip): one copy each, host and
// device, with internal linkage like rt_post_common.h.  The definitions are include/rt_hip.h's (rt_noise_opts); tests/noise_checker.py
// and tests/adaptive_checker.py restate them in numpy f32, and tests/cpp/chunk_stats_check.cpp runs THESE functions on the host
// against that Python, bit for bit.  A further consumer of chunk sums calls these; it does not restate them.
#pragma once
#include "rt_post_common.h"

namespace rt {
namespace {

// Work item `wp` of a whole-frame render (RT_LAYOUT_FRAME, shard 0 of 1) -> pixel index y * width + x: the render kernel's
// work_to_pixel (rt_render.hip) for that case -- tile k = wp / (tile_w * tile_h), tiles row-major, pixels row-major inside the
// tile.  false: padding of an edge tile.
__host__ __device__ __forceinline__ bool frame_work_pixel(uint32_t wp, uint32_t tile_w, uint32_t tile_h, uint32_t tiles_x, uint32_t width, uint32_t height,
                                                 size_t &p)
{
	const uint32_t tile_pixels = tile_w * tile_h;
	const uint32_t tile = wp / tile_pixels, in = wp - tile * tile_pixels;
	const uint32_t ty = tile / tiles_x, tx = tile - ty * tiles_x;
	const uint32_t x = tx * tile_w + in % tile_w, y = ty * tile_h + in / tile_w;
	if (x >= width || y >= height)
		return false;
	p = (size_t)y * width + x;
	return true;
}

// Place 0..63 of tile `tile` in the 8 x 8 tile grid of the frame (rt_noise_tiles' grid, tiles_x across; places row-major) -> (x, y).
// false: a place outside the frame, in an edge tile.  (Not the 16 x 16 tile_pixel of rt_post_common.h.)
__host__ __device__ __forceinline__ bool grid8_pixel(uint32_t tile, uint32_t place, uint32_t tiles_x, uint32_t width, uint32_t height, uint32_t &x, uint32_t &y)
{
	const uint32_t ty = tile / tiles_x, tx = tile - ty * tiles_x;
	x = 8u * tx + (place & 7u);
	y = 8u * ty + (place >> 3);
	return x < width && y < height;
}

// what a pixel's estimates are divided by, per component: its albedo clamped below at 1e-3 (a NaN albedo gives the clamp), or 1
// where there is no albedo plane.  p3 = 3 * pixel.
struct Demod { float d0, d1, d2; };
__host__ __device__ __forceinline__ Demod demod_divisors(const float *albedo, size_t p3)
{
	float d0 = 1.0f, d1 = 1.0f, d2 = 1.0f;
	if (albedo) {
		d0 = fmaxf(albedo[p3], 1e-3f);
		d1 = fmaxf(albedo[p3 + 1u], 1e-3f);
		d2 = fmaxf(albedo[p3 + 2u], 1e-3f);
	}
	return Demod{d0, d1, d2};
}

// l_c: the demodulated luminance of the estimate one chunk gives, from its sum m[3] over n passes
__host__ __device__ __forceinline__ float chunk_lum(const float *m, float n, const Demod &d) { return lum(m[0] / n / d.d0, m[1] / n / d.d1, m[2] / n / d.d2); }

// lbar = (sum of the l_c) / S and var = (sum of (l_c - lbar)^2) / (S (S - 1)) of the S sums first[c * stride], n passes each; both
// sums run in chunk order from +0.  The sums are read twice -- once for lbar, once for the squared deviations: no array is kept,
// so nothing is indexed dynamically (a private array indexed by the chunk would live in scratch).
struct ChunkStats { float lbar, var; };
__host__ __device__ __forceinline__ ChunkStats chunk_stats(const float *first, size_t stride, uint32_t split, float n, const Demod &d)
{
	const float s = (float)split;
	float lsum = 0.0f;
	for (uint32_t c = 0; c < split; ++c)
		lsum = lsum + chunk_lum(first + c * stride, n, d);
	const float lbar = lsum / s;
	float sq = 0.0f;
	for (uint32_t c = 0; c < split; ++c) {
		const float dl = chunk_lum(first + c * stride, n, d) - lbar;
		sq = sq + dl * dl;
	}
	return ChunkStats{lbar, sq / (float)(split * (split - 1u))};
}

// One batch (its mean at mean_in, its lbar and var) into pixel p of the state (M, L, V): added, or stored when the sequence is
// `fresh`; then the planes M / nb, L / nb, V / (nb * nb), nb the batches the pixel holds with this one.  OPTIONAL: the state (all
// three planes or none: one batch, nothing kept) and each output may be null; else none of them is tested.
template <bool OPTIONAL>
__host__ __device__ __forceinline__ void chunk_state_step(size_t p, const float *mean_in, ChunkStats b, float *state_m, float *state_l, float *state_v, bool fresh,
                                                 float nb, float *out_mean, float *out_lum, float *out_var)
{
	const size_t p3 = 3u * p;
	float m0 = mean_in[p3], m1 = mean_in[p3 + 1u], m2 = mean_in[p3 + 2u], l = b.lbar, v = b.var;
	if (!OPTIONAL || state_m) {
		if (!fresh) {
			m0 = state_m[p3] + m0;
			m1 = state_m[p3 + 1u] + m1;
			m2 = state_m[p3 + 2u] + m2;
			l = state_l[p] + l;
			v = state_v[p] + v;
		}
		state_m[p3] = m0;
		state_m[p3 + 1u] = m1;
		state_m[p3 + 2u] = m2;
		state_l[p] = l;
		state_v[p] = v;
	}
	if (!OPTIONAL || out_mean) {
		out_mean[p3] = m0 / nb;
		out_mean[p3 + 1u] = m1 / nb;
		out_mean[p3 + 2u] = m2 / nb;
	}
	if (!OPTIONAL || out_lum)
		out_lum[p] = l / nb;
	if (!OPTIONAL || out_var)
		out_var[p] = v / (nb * nb);
}

} // namespace
} // namespace rt
