// rt_noise.hip -- per-pixel noise estimates from the chunk sums of one render (rt_render_noise, include/rt_hip.h): the S
// independent estimates of a pixel that a render at sample_split = S leaves in the scene's partial buffer give a variance of the
// mean at no extra ray.  The definition is in the header; tests/noise_checker.py restates it in numpy f32, bit for bit.  The
// arithmetic of a pixel and both maps to a pixel are rt_chunk_stats.h's, shared with the other readers of chunk sums.
//
// Kernels (stable names for rocprofv3):
//   noise_chunk_kernel   one lane per work item of a chunk (= per pixel, in the render's tile order): (lbar, var) of its S chunk
//                        sums (chunk_stats), then (mean, lbar, var) added to the batch state and the state divided out
//                        (chunk_state_step).  A wave reads 64 consecutive work items of one chunk: 768 contiguous bytes per load
//                        instruction triple.
//   noise_tile_kernel    one wave per 8 x 8 tile, one lane per pixel: the relative error of the pixel, a butterfly sum over the
//                        64 lanes by __shfl_xor (every lane adds the same two values in either order, so all 64 hold the same
//                        bits and the result is the tree the header states), lane 0 writes the tile and does the two atomics.
//                        -DRT_NOISE_TILE_LDS builds the same tree through LDS instead (a measurement variant).
#include "rt_noise.h"
#include "rt_chunk_stats.h"

namespace rt {

__global__ __launch_bounds__(256) void noise_chunk_kernel(const DevNoiseChunkParams P)
{
	const uint32_t wp = blockIdx.x * 256u + threadIdx.x;
	if (wp >= P.n_work)
		return;
	size_t p;
	if (!frame_work_pixel(wp, P.tile_w, P.tile_h, P.tiles_x, P.width, P.height, p))
		return; // edge-tile padding
	const Demod d = demod_divisors(P.albedo, 3u * p);
	const ChunkStats b = chunk_stats(P.partial + 3u * (size_t)wp, 3u * (size_t)P.n_work, P.split, (float)P.chunk_passes, d);
	chunk_state_step<true>(p, P.mean_in, b, P.state_m, P.state_l, P.state_v, P.fresh != 0u, P.batches, P.out_mean, P.out_lum, P.out_var);
}

__global__ __launch_bounds__(256) void noise_tile_kernel(const DevNoiseTileParams P)
{
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
#ifdef RT_NOISE_TILE_LDS
	__shared__ float slots[4][64];
#endif
	// (a wave's trip count is its own: nothing below synchronises the workgroup)
	for (uint32_t tile = blockIdx.x * 4u + wave; tile < P.n_tiles; tile += gridDim.x * 4u) {
		uint32_t x, y;
		float v = 0.0f; // a slot outside the frame
		if (grid8_pixel(tile, lane, P.tiles_x, P.width, P.height, x, y)) {
			const size_t p = (size_t)y * P.width + x;
			v = sqrtf(P.variance[p]) / (fabsf(P.lum_mean[p]) + P.luminance_floor);
			if (!__builtin_isfinite(v))
				v = __builtin_inff();
		}
#ifdef RT_NOISE_TILE_LDS
		volatile float *const mine = slots[wave];
		for (uint32_t k = 0; k < 6u; ++k) {
			mine[lane] = v;
			__builtin_amdgcn_wave_barrier();
			v = v + mine[lane ^ (1u << k)];
			__builtin_amdgcn_wave_barrier();
		}
#else
		for (int k = 0; k < 6; ++k)
			v = v + __shfl_xor(v, 1 << k);
#endif
		if (lane == 0u) {
			const uint32_t ty = tile / P.tiles_x, tx = tile - ty * P.tiles_x;
			const uint32_t w_in = P.width - 8u * tx < 8u ? P.width - 8u * tx : 8u, h_in = P.height - 8u * ty < 8u ? P.height - 8u * ty : 8u;
			const float e = v / (float)(w_in * h_in);
			if (P.tile_error)
				P.tile_error[tile] = e;
			if (P.summary) {
				atomicMax(P.summary, __float_as_uint(e + 0.0f)); // >= +0 or +inf (a -0 folded to +0): the bit patterns order as the values
				if (e > P.threshold)
					atomicAdd(P.summary + 1, 1u);
				if (tile == 0u)
					P.summary[2] = P.n_tiles;
			}
		}
	}
}

hipError_t launch_noise_chunks(hipStream_t stream, const DevNoiseChunkParams &P)
{
	hipLaunchKernelGGL(noise_chunk_kernel, dim3((P.n_work + 255u) / 256u), dim3(256), 0, stream, P);
	return hipGetLastError();
}

hipError_t launch_noise_tiles(hipStream_t stream, const DevNoiseTileParams &P)
{
	uint32_t blocks = (P.n_tiles + 3u) / 4u;
	if (blocks > kNoiseTileGridBlocks)
		blocks = kNoiseTileGridBlocks;
	hipLaunchKernelGGL(noise_tile_kernel, dim3(blocks), dim3(256), 0, stream, P);
	return hipGetLastError();
}

} // namespace rt
