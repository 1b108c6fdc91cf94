// rt_denoise.hip -- AOV-guided edge-aware A-Trous denoiser (rt_denoise, include/rt_hip.h): the spatial part of SVGF on
// albedo-demodulated radiance.  The filter is defined in the header; tests/denoise_checker.py restates it in float64.
//
// Workspace: three float4 planes of w*h.  plane0 / plane1 hold (e.rgb, Var) and ping-pong between iterations; guide holds
// (n^.xyz, z).  Each filter tap is two 16-byte loads.  An invalid pixel is stored as (0, 0, 0, NaN): a NaN variance is the mark
// every tap tests (a valid pixel's variance is finite for finite inputs).
//
// Kernels (stable names for rocprofv3):
//   denoise_prepass_kernel<MODE>   one lane per pixel: demodulate, normalise the normal, the initial variance (MODE 0: given;
//                                  MODE 1: lum(e0) into plane1 for the 5 x 5 estimate; MODE 2: the two halves of
//                                  rt_render_denoised, which also writes the noisy mean)
//   denoise_variance_kernel        MODE 1 only: the 5 x 5 two-pass estimate, plane1 -> plane0
//   denoise_iteration_kernel<LAST> one launch per iteration: 3 x 3 prefiltered variance, 25 taps at step 2^i; the last one
//                                  remodulates and writes 3 floats per pixel
// The tiled kernels give each 256-thread workgroup a 16 x 16 block and each wave an 8 x 8 block of it (one lane per pixel), so a
// wave's taps fall on few cache lines.  Taps are gathered through L1 / L2: the working set (48 B per pixel) stays in the
// Infinity Cache at 1080p.
#include "rt_denoise.h"
#include "rt_post_common.h"

namespace rt {

template <int MODE>
__global__ __launch_bounds__(256) void denoise_prepass_kernel(const DevDenoiseParams P)
{
	const uint32_t n = P.width * P.height;
	for (uint32_t p = blockIdx.x * 256u + threadIdx.x; p < n; p += gridDim.x * 256u) {
		const size_t p3 = 3ull * p;
		float c[3], d[3] = {1.0f, 1.0f, 1.0f}, e[3];
		float var;
		if (P.albedo)
			for (int i = 0; i < 3; ++i)
				d[i] = fmaxf(P.albedo[p3 + i], 1e-3f);
		if (MODE == 2) {
			float a[3], b[3];
			for (int i = 0; i < 3; ++i) {
				a[i] = P.half_a[p3 + i];
				b[i] = P.half_b[p3 + i];
				c[i] = (a[i] + b[i]) * 0.5f;
				P.noisy[p3 + i] = c[i];
			}
			const float la = lum(a[0] / d[0], a[1] / d[1], a[2] / d[2]);
			const float lb = lum(b[0] / d[0], b[1] / d[1], b[2] / d[2]);
			var = (la - lb) * (la - lb) * 0.25f;
		} else {
			for (int i = 0; i < 3; ++i)
				c[i] = P.color[p3 + i];
		}
		for (int i = 0; i < 3; ++i)
			e[i] = c[i] / d[i];
		if (MODE == 0)
			var = P.variance[p];
		else if (MODE == 1)
			var = lum(e[0], e[1], e[2]);
		const bool valid = finite3(c[0], c[1], c[2]) && __builtin_isfinite(var);
		const float4 v = valid ? make_float4(e[0], e[1], e[2], var) : make_float4(0.0f, 0.0f, 0.0f, __builtin_nanf(""));
		(MODE == 1 ? P.plane1 : P.plane0)[p] = v;

		float4 g = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
		if (P.normal) {
			const float nx = P.normal[p3], ny = P.normal[p3 + 1], nz = P.normal[p3 + 2];
			const float len = sqrtf(nx * nx + ny * ny + nz * nz);
			if (len != 0.0f) {
				g.x = nx / len;
				g.y = ny / len;
				g.z = nz / len;
			}
		}
		if (P.depth)
			g.w = P.depth[p];
		P.guide[p] = g;
	}
}

// Var0 when no variance is given: over the in-frame valid q of the 5 x 5 box, m = sum l / count, Var0 = sum (l - m)^2 / count
__global__ __launch_bounds__(256) void denoise_variance_kernel(const DevDenoiseParams P, uint32_t tiles_x, uint32_t n_tiles)
{
	const uint32_t W = P.width, H = P.height;
	for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
		uint32_t x, y;
		tile_pixel(tile, tiles_x, x, y);
		if (x >= W || y >= H)
			continue;
		const uint32_t p = y * W + x;
		float4 c = P.plane1[p];
		if (!__builtin_isnan(c.w)) {
			float sum = 0.0f, count = 0.0f;
#pragma unroll
			for (int dy = -2; dy <= 2; ++dy)
#pragma unroll
				for (int dx = -2; dx <= 2; ++dx) {
					const uint32_t qx = x + (uint32_t)dx, qy = y + (uint32_t)dy; // wraps to >= W / H when off the low edge
					if (qx < W && qy < H) {
						const float l = P.plane1[qy * W + qx].w;
						if (!__builtin_isnan(l)) {
							sum += l;
							count += 1.0f;
						}
					}
				}
			const float m = sum / count;
			float sq = 0.0f;
#pragma unroll
			for (int dy = -2; dy <= 2; ++dy)
#pragma unroll
				for (int dx = -2; dx <= 2; ++dx) {
					const uint32_t qx = x + (uint32_t)dx, qy = y + (uint32_t)dy;
					if (qx < W && qy < H) {
						const float l = P.plane1[qy * W + qx].w;
						if (!__builtin_isnan(l))
							sq += (l - m) * (l - m);
					}
				}
			c.w = sq / count;
		}
		P.plane0[p] = c;
	}
}

template <bool LAST>
__global__ __launch_bounds__(256) void denoise_iteration_kernel(const DevDenoiseParams P, const float4 *__restrict__ src,
                                                               float4 *__restrict__ dst, uint32_t step, uint32_t tiles_x,
                                                               uint32_t n_tiles)
{
	const float h5[5] = {1.0f / 16.0f, 1.0f / 4.0f, 3.0f / 8.0f, 1.0f / 4.0f, 1.0f / 16.0f};
	const float g3[3] = {0.25f, 0.5f, 0.25f};
	const uint32_t W = P.width, H = P.height;
	const bool use_n = P.normal != nullptr, use_z = P.depth != nullptr; // (wave-uniform)
	const float4 *__restrict__ guide = P.guide;
	for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
		uint32_t x, y;
		tile_pixel(tile, tiles_x, x, y);
		if (x >= W || y >= H)
			continue;
		const uint32_t p = y * W + x;
		const float4 cp = src[p];
		if (__builtin_isnan(cp.w)) { // invalid: passes through
			if (LAST) {
				const size_t p3 = 3ull * p;
				for (int i = 0; i < 3; ++i)
					P.out[p3 + i] = P.color[p3 + i];
			} else {
				dst[p] = cp;
			}
			continue;
		}
		// g(p): 3 x 3 binomial prefilter of the variance over the in-frame valid neighbours
		float gs = 0.0f, gw = 0.0f;
#pragma unroll
		for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
			for (int dx = -1; dx <= 1; ++dx) {
				const uint32_t qx = x + (uint32_t)dx, qy = y + (uint32_t)dy;
				if (qx < W && qy < H) {
					const float v = src[qy * W + qx].w;
					if (!__builtin_isnan(v)) {
						const float wg = g3[dx + 1] * g3[dy + 1];
						gs += wg * v;
						gw += wg;
					}
				}
			}
		const float denom = P.sigma_l * sqrtf(gs / gw) + 1e-6f;
		const float lp = lum(cp.x, cp.y, cp.z);
		const float4 gp = (use_n || use_z) ? guide[p] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
		const bool np0 = gp.x == 0.0f && gp.y == 0.0f && gp.z == 0.0f;
		const float zscale = P.sigma_z * gp.w * (float)step;
		float sr = 0.0f, sg = 0.0f, sb = 0.0f, sw = 0.0f, sv = 0.0f;
#pragma unroll
		for (int dy = -2; dy <= 2; ++dy)
#pragma unroll
			for (int dx = -2; dx <= 2; ++dx) {
				const uint32_t qx = x + (uint32_t)(dx * (int)step), qy = y + (uint32_t)(dy * (int)step);
				if (qx >= W || qy >= H)
					continue;
				const uint32_t q = qy * W + qx;
				const float4 cq = src[q];
				if (__builtin_isnan(cq.w))
					continue;
				float w;
				if (dx == 0 && dy == 0) {
					w = 9.0f / 64.0f;
				} else {
					const float wl = expf(-fabsf(lp - lum(cq.x, cq.y, cq.z)) / denom);
					float wn = 1.0f, wz = 1.0f;
					if (use_n || use_z) {
						const float4 gq = guide[q];
						if (use_n) {
							const bool nq0 = gq.x == 0.0f && gq.y == 0.0f && gq.z == 0.0f;
							if (!(np0 && nq0))
								wn = powf(fmaxf(0.0f, gp.x * gq.x + gp.y * gq.y + gp.z * gq.z), P.sigma_n);
						}
						if (use_z) {
							if (gp.w == 0.0f || gq.w == 0.0f)
								wz = (gp.w == 0.0f && gq.w == 0.0f) ? 1.0f : 0.0f;
							else
								wz = expf(-fabsf(gp.w - gq.w) / zscale);
						}
					}
					w = h5[dx + 2] * h5[dy + 2] * wl * wn * wz;
				}
				sr += w * cq.x;
				sg += w * cq.y;
				sb += w * cq.z;
				sw += w;
				sv += w * w * cq.w;
			}
		if (LAST) {
			const size_t p3 = 3ull * p;
			float d[3] = {1.0f, 1.0f, 1.0f};
			if (P.albedo)
				for (int i = 0; i < 3; ++i)
					d[i] = fmaxf(P.albedo[p3 + i], 1e-3f);
			P.out[p3] = sr / sw * d[0];
			P.out[p3 + 1] = sg / sw * d[1];
			P.out[p3 + 2] = sb / sw * d[2];
		} else {
			dst[p] = make_float4(sr / sw, sg / sw, sb / sw, sv / (sw * sw));
		}
	}
}

static void tile_grid(const DevDenoiseParams &P, uint32_t &tiles_x, uint32_t &n_tiles, dim3 &blocks)
{
	tiles_x = (P.width + 15u) / 16u;
	n_tiles = tiles_x * ((P.height + 15u) / 16u);
	blocks = dim3(std::min(n_tiles, kMaxBlocks));
}

void launch_denoise_variance(hipStream_t stream, const DevDenoiseParams &P)
{
	uint32_t tiles_x, n_tiles;
	dim3 tile_blocks;
	tile_grid(P, tiles_x, n_tiles, tile_blocks);
	hipLaunchKernelGGL(denoise_variance_kernel, tile_blocks, dim3(256), 0, stream, P, tiles_x, n_tiles);
}

void launch_denoise_iteration(hipStream_t stream, const DevDenoiseParams &P, uint32_t i, const float4 *src, float4 *dst)
{
	uint32_t tiles_x, n_tiles;
	dim3 tile_blocks;
	tile_grid(P, tiles_x, n_tiles, tile_blocks);
	const uint32_t step = 1u << i;
	if (i + 1u == P.iterations)
		hipLaunchKernelGGL(denoise_iteration_kernel<true>, tile_blocks, dim3(256), 0, stream, P, src, nullptr, step, tiles_x, n_tiles);
	else
		hipLaunchKernelGGL(denoise_iteration_kernel<false>, tile_blocks, dim3(256), 0, stream, P, src, dst, step, tiles_x, n_tiles);
}

hipError_t launch_denoise(hipStream_t stream, const DevDenoiseParams &P)
{
	const uint32_t n = P.width * P.height;
	const dim3 pre_blocks(std::min<uint32_t>((n + 255u) / 256u, kMaxBlocks));
	if (P.half_a)
		hipLaunchKernelGGL(denoise_prepass_kernel<2>, pre_blocks, dim3(256), 0, stream, P);
	else if (P.variance)
		hipLaunchKernelGGL(denoise_prepass_kernel<0>, pre_blocks, dim3(256), 0, stream, P);
	else {
		hipLaunchKernelGGL(denoise_prepass_kernel<1>, pre_blocks, dim3(256), 0, stream, P);
		launch_denoise_variance(stream, P);
	}
	float4 *src = P.plane0, *dst = P.plane1;
	for (uint32_t i = 0; i < P.iterations; ++i) {
		launch_denoise_iteration(stream, P, i, src, dst);
		std::swap(src, dst);
	}
	return hipGetLastError();
}

} // namespace rt
