// rt_adaptive.hip -- the render on a LIST of 8 x 8 tiles (rt_render_tiles, include/rt_hip.h) and the selection of the tiles
// whose error is above a threshold (rt_noise_select_tiles): what per-tile refinement and a region render need of the device.
//
// tiles_kernel is radiance_kernel (rt_radiance.hip) with another START and another FINISH around the same
// per-lane integrator, rt_path_lane.h (its header describes the phases, the quorum and the hand-out).  This file holds:
//   START   the render's own camera ray (rt_render.hip do_gen, rt_aov_common.h aov_camera_ray): the first two draws of the stream
//           (seed, pixel, sample_begin + pass) jitter the pixel, SimpleCamera::get_ray draws its unused time, and the path goes on
//           ON THAT STREAM
//   FINISH  the NaN filter, then the fold rt_render_opts states: split 1 the running mean `mean += (pass - mean) / i`, else the
//           chunk's sum in pass order from +0.  A chunk's end stores the sum (chunk_sums given) or adds it to the pixel's total in
//           chunk order, which the last chunk divides by spp once -- the bytes combine_chunks_kernel (rt_render.hip) produces
// Work items: item i is tile slot i / (split / item_chunks) of the list and `item_chunks` chunks of it from chunk
// (i % (split / item_chunks)) * item_chunks on; its 64 lane slots are the 64 pixels of the tile, row-major.  With a chunk buffer an
// item is ONE chunk, so that ten tiles at split 16 are 10 240 lanes of work and not 640; without one it is the whole pixel and the
// launch needs no memory besides the frame.  The hand-out's blocks of 64 slots are the items (WaveBlocks, rt_path_lane.h).  A lane
// whose slot is padding of an edge tile writes +0 sums and claims again; a tile index past the grid is skipped whole.
//
// Ray counters: SamplerProgress.rays_shot as rt_render.hip counts it -- naive: one per walk of a path ray (do_shade), MIS: one per
// sample_lights call (do_light, mis.rs:38) -- summed per lane, reduced per wave, one atomic per wave.
//
// select_tiles_kernel: ONE workgroup walks the tile-error plane 256 tiles at a time; ballots and prefix counts place the indices
// above the threshold in ascending order, so the list is a pure function of the plane.
#include <algorithm>

#include "rt_path_lane.h"
#include "rt_adaptive.h"
#include "rt_chunk_stats.h"

namespace rt {

struct TilesArgs {
	DevScene S;
	DevTilesParams P;
};

// lanes of the wave that must wait for a closest-hit walk before it runs while shadow rays are pending elsewhere (as
// kRadianceQuorum)
#ifndef RT_TILES_QUORUM
#define RT_TILES_QUORUM 32
#endif
constexpr uint32_t kTilesQuorum = RT_TILES_QUORUM;

template <int METHOD, bool PRUNE>
__global__ __launch_bounds__(256, kTilesWaves) void tiles_kernel(const TilesArgs args_by_value)
{
	using F = FeatFull; // every primitive, material and texture type compiled in (as radiance_kernel)
	extern __shared__ __align__(16) uint32_t lds[];
	const DevScene &S = args_by_value.S;
	const WaveStack W = wave_stack(S, lds);
	// Behind the stacks: the lane's FOLD RECORD, kTilesRecordWords words (word w of thread t at rec[256 w]).  What a pixel's fold
	// carries from pass to pass is needed in FINISH, CLAIM and START only, so it waits in LDS while the walks and the shading have
	// the registers: kept there, the MIS kernels spilled 14 to 19 VGPRs to scratch.
	uint32_t *const rec = lds + kFourWaves * (S.stack_depth * kStackStride) + threadIdx.x;
	enum : uint32_t {
		R_TOTAL = 0u * 256u,     // [3] whole-pixel item: the total of its chunk sums so far, in chunk order
		R_SUM = 3u * 256u,       // [3] the chunk's passes so far, in pass order (split 1: the running mean)
		R_ID = 6u * 256u,        // 64 * item + the pixel's place in its tile
		R_PIXEL = 7u * 256u,     // y * width + x
		R_PASS = 8u * 256u,      // the pass in flight, counted from the pixel's first
		R_CHUNK_END = 9u * 256u, // where its chunk ends
		R_RAYS = 10u * 256u,     // the lane's ray counter (flushed in FINISH long before it could wrap)
	};
	rec[R_RAYS] = 0u;
	const auto count_ray = [rec] { rec[R_RAYS] += 1u; };
	WaveBlocks blocks; // of 64 lane slots: a work item each
	PathLane L;        // the path, in registers

#pragma unroll 1
	for (;;) {
		// ---- FINISH: the sample's value, then the fold of rt_render_opts.sample_split ----
		if (L.ph >= PH_FINISH) {
			const V3 v = L.sample_value();
			const KArgPtr<TilesArgs> ka = aov_kargs(args_by_value);
			const uint32_t split = ka->P.split;
			const uint32_t k = rec[R_PASS] + 1u; // passes of the pixel folded once this one is
			V3 sum = v3(__uint_as_float(rec[R_SUM]), __uint_as_float(rec[R_SUM + 256u]), __uint_as_float(rec[R_SUM + 512u]));
			if (split > 1u) { // (wave-uniform)
				sum.x += v.x;
				sum.y += v.y;
				sum.z += v.z;
			} else {
				const float i_f = (float)k;
				sum.x += (v.x - sum.x) / i_f; // src/main.rs:179-185
				sum.y += (v.y - sum.y) / i_f;
				sum.z += (v.z - sum.z) / i_f;
			}
			{ // (a pass shoots fewer than 2^31 rays, as rt_render.hip's per-sample counter assumes: the lane's counter cannot wrap)
				uint32_t lane_rays = rec[R_RAYS];
				if (lane_rays >= 0x80000000u) {
					unsigned long long *const rays_shot = ka->P.rays_shot;
					if (rays_shot != nullptr)
						atomicAdd(rays_shot, (unsigned long long)lane_rays);
					lane_rays = 0u;
				}
				rec[R_RAYS] = lane_rays;
			}
			rec[R_PASS] = k;
			L.ph = PH_START;
			if (k == rec[R_CHUNK_END]) {
				const uint32_t spp = ka->P.spp;
				float *const sums = ka->P.chunk_sums;
				if (split == 1u) {
					float *const o = ka->P.out + 3u * (size_t)rec[R_PIXEL];
					o[0] = sum.x;
					o[1] = sum.y;
					o[2] = sum.z;
					L.ph = PH_CLAIM;
				} else if (sums != nullptr) { // the item was this chunk: [chunk][64 * slot + place][3]
					const uint32_t id = rec[R_ID];
					const uint32_t item = id >> 6, slot = item / split, c = item - slot * split;
					float *const o = sums + 3u * ((size_t)c * 64u * ka->P.n_tiles + (64u * slot + (id & 63u)));
					o[0] = sum.x;
					o[1] = sum.y;
					o[2] = sum.z;
					L.ph = PH_CLAIM;
				} else {
					// the item is the pixel: its chunk sums added in chunk order from +0, divided by spp once.
					// j = the chunk that starts at pass k: floor(j * spp / split) == k
					const uint32_t j = (uint32_t)(((uint64_t)k * split + (spp - 1u)) / spp);
					V3 t = v3s(0.0f);
					if (j != 1u)
						t = v3(__uint_as_float(rec[R_TOTAL]), __uint_as_float(rec[R_TOTAL + 256u]), __uint_as_float(rec[R_TOTAL + 512u]));
					t.x = t.x + sum.x;
					t.y = t.y + sum.y;
					t.z = t.z + sum.z;
					if (k == spp) {
						float *const o = ka->P.out + 3u * (size_t)rec[R_PIXEL];
						o[0] = t.x / (float)spp;
						o[1] = t.y / (float)spp;
						o[2] = t.z / (float)spp;
						L.ph = PH_CLAIM;
					} else {
						rec[R_TOTAL] = __float_as_uint(t.x);
						rec[R_TOTAL + 256u] = __float_as_uint(t.y);
						rec[R_TOTAL + 512u] = __float_as_uint(t.z);
						rec[R_CHUNK_END] = (uint32_t)(((uint64_t)(j + 1u) * spp) / split);
						sum = v3s(0.0f);
					}
				}
			}
			rec[R_SUM] = __float_as_uint(sum.x);
			rec[R_SUM + 256u] = __float_as_uint(sum.y);
			rec[R_SUM + 512u] = __float_as_uint(sum.z);
		}
		// ---- CLAIM: the next lane slot of the wave's item -> tile, chunk and pixel ----
		const uint64_t need = __ballot(L.ph == PH_CLAIM);
		if (need != 0ull) { // (wave-uniform)
			const KArgPtr<TilesArgs> ka = aov_kargs(args_by_value);
			const uint32_t n = ka->P.n_lanes;
			if (L.ph == PH_CLAIM) {
				const uint32_t id = blocks.claimed(need);
				if (id >= n) {
					L.ph = PH_DONE;
				} else {
					const uint32_t split = ka->P.split, item_chunks = ka->P.item_chunks, spp = ka->P.spp;
					const uint32_t per_tile = item_chunks == 1u ? split : 1u; // items a tile is
					const uint32_t item = id >> 6, place = id & 63u;
					const uint32_t slot = item / per_tile, c0 = (item - slot * per_tile) * item_chunks;
					const uint32_t tile = ka->P.tiles[slot]; // (slot < n_tiles: id < n_lanes)
					const uint32_t width = ka->P.width;
					uint32_t x, y;
					const bool inside = grid8_pixel(tile, place, ka->P.tiles_x, width, ka->P.height, x, y);
					if (tile >= ka->P.tile_count) {
						// not a tile of this frame: skipped whole (ph stays CLAIM: the lane takes another slot next iteration)
					} else if (!inside) { // padding of an edge tile
						float *const sums = ka->P.chunk_sums;
						if (split > 1u && sums != nullptr) {
							float *const o = sums + 3u * ((size_t)c0 * 64u * ka->P.n_tiles + (64u * slot + place));
							o[0] = o[1] = o[2] = 0.0f;
						}
					} else {
						rec[R_ID] = id;
						rec[R_PIXEL] = y * width + x;
						rec[R_PASS] = (uint32_t)(((uint64_t)c0 * spp) / split);
						rec[R_CHUNK_END] = (uint32_t)(((uint64_t)(c0 + 1u) * spp) / split);
						rec[R_SUM] = rec[R_SUM + 256u] = rec[R_SUM + 512u] = 0u; // +0
						L.ph = PH_START;
					}
				}
			}
			blocks.advance(need, n);
		}
		// ---- START: the next pass of the pixel.  random_sampler.rs:50-61 as rt_render.hip do_gen ----
		if (L.ph == PH_START) {
			const KArgPtr<TilesArgs> ka = aov_kargs(args_by_value);
			const uint64_t seed = ((uint64_t)ka->P.seed_hi << 32) | ka->P.seed_lo;
			const uint64_t sample_begin = ((uint64_t)ka->P.sample_begin_hi << 32) | ka->P.sample_begin_lo;
			const V3 cam_o = v3(ka->P.cam.origin[0], ka->P.cam.origin[1], ka->P.cam.origin[2]);
			const V3 cam_ll = v3(ka->P.cam.lower_left[0], ka->P.cam.lower_left[1], ka->P.cam.lower_left[2]);
			const V3 cam_h = v3(ka->P.cam.horizontal[0], ka->P.cam.horizontal[1], ka->P.cam.horizontal[2]);
			const V3 cam_v = v3(ka->P.cam.vertical[0], ka->P.cam.vertical[1], ka->P.cam.vertical[2]);
			const uint32_t width = ka->P.width, height = ka->P.height;
			const uint32_t pixel = rec[R_PIXEL], k = rec[R_PASS];
			const uint32_t py = pixel / width, px = pixel - py * width;
			rt_rng_seed(&L.rng, seed, (uint64_t)pixel, sample_begin + k);
			const float jx = rt_rng_range_f32(&L.rng, 0.0f, 1.0f) + (float)px, jy = rt_rng_range_f32(&L.rng, 0.0f, 1.0f) + (float)py;
			const float u = jx / (float)(width - 1u);
			const float v = 1.0f - jy / (float)(height - 1u);
			L.ray = ray_new<F>(cam_o, cam_ll + cam_h * u + cam_v * v - cam_o); // SimpleCamera::get_ray  camera.rs:57-63
			(void)rt_rng_f32(&L.rng);                                         // (its unused `time`)
			L.start();
		}

		const uint64_t m_closest = __ballot(L.ph == PH_CLOSEST), m_shadow = __ballot(L.ph == PH_SHADOW);
		// no walk is waiting: every lane is DONE, or some claim again (their slot was padding or no tile)
		if ((m_closest | m_shadow) == 0ull && __ballot(L.ph == PH_CLAIM) == 0ull)
			break;
		// (the walk falls through when only claims wait: a `continue` would be the loop's second back edge)
		path_lane_walk<METHOD, PRUNE, kTilesQuorum, F>(L, args_by_value, W, m_closest, m_shadow, count_ray);
	}

	// ---- SamplerProgress.rays_shot: wave reduction, one atomic per wave (as rt_render.hip) ----
	unsigned long long *const rays_shot = aov_kargs(args_by_value)->P.rays_shot;
	if (rays_shot != nullptr) {
		unsigned long long total = rec[R_RAYS];
		for (int off = 32; off > 0; off >>= 1)
			total += __shfl_down(total, off);
		if ((threadIdx.x & 63u) == 0u)
			atomicAdd(rays_shot, total);
	}
}

// the counter of a launch zeroed by a kernel, not a memset node (rt_render.hip reset_kernel says why)
__global__ void tiles_zero_kernel(unsigned long long *rays_shot) { *rays_shot = 0ull; }

// chunk_sums -> the listed pixels: the S sums added in chunk order from +0, divided by spp once (combine_chunks_kernel's arithmetic)
__global__ __launch_bounds__(256) void tiles_combine_kernel(const DevTilesParams P)
{
	const uint32_t i = blockIdx.x * 256u + threadIdx.x; // 64 * slot + place
	if (i >= 64u * P.n_tiles)
		return;
	const uint32_t tile = P.tiles[i >> 6], place = i & 63u;
	if (tile >= P.tile_count)
		return;
	uint32_t x, y;
	if (!grid8_pixel(tile, place, P.tiles_x, P.width, P.height, x, y))
		return;
	const size_t stride = 3u * (size_t)64u * P.n_tiles;
	const float *m = P.chunk_sums + 3u * (size_t)i;
	float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f;
	for (uint32_t c = 0; c < P.split; ++c, m += stride) {
		a0 = a0 + m[0];
		a1 = a1 + m[1];
		a2 = a2 + m[2];
	}
	float *const o = P.out + 3u * ((size_t)y * P.width + x);
	o[0] = a0 / (float)P.spp;
	o[1] = a1 / (float)P.spp;
	o[2] = a2 / (float)P.spp;
}

// One workgroup.  Round r looks at tiles [256 r, 256 r + 256): a wave's ballot gives each lane its rank among the wave's tiles
// above the threshold, the four wave counts (LDS) the wave's offset in the round, `total` (kept by every thread alike) the
// round's offset in the list -- so the list is ascending.  `e > threshold` is false for NaN, as tiles_above counts.
__global__ __launch_bounds__(256) void select_tiles_kernel(const DevSelectParams P)
{
	__shared__ uint32_t wave_count[4];
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	uint32_t total = 0u;
	for (uint32_t base = 0u; base < P.n_tiles; base += 256u) { // (uniform trip count: the barriers below are reached by all)
		const uint32_t tile = base + threadIdx.x;
		const bool above = tile < P.n_tiles && P.tile_error[tile] > P.threshold;
		const uint64_t m = __ballot(above);
		if (lane == 0u)
			wave_count[wave] = (uint32_t)__popcll(m);
		__syncthreads();
		uint32_t before = 0u, round = 0u;
		for (uint32_t w = 0u; w < 4u; ++w) {
			const uint32_t n = wave_count[w];
			before += w < wave ? n : 0u;
			round += n;
		}
		if (above)
			P.tiles[total + before + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = tile;
		total += round;
		__syncthreads(); // (wave_count is rewritten next round)
	}
	if (threadIdx.x == 0u)
		*P.count = total;
}

hipError_t launch_tiles(int method, bool prune, hipStream_t stream, const DevScene &S, const DevTilesParams &P, uint32_t groups)
{
	if (P.rays_shot != nullptr) {
		hipLaunchKernelGGL(tiles_zero_kernel, dim3(1), dim3(1), 0, stream, P.rays_shot);
		const hipError_t e = hipGetLastError();
		if (e != hipSuccess)
			return e;
	}
	if (P.n_tiles == 0u)
		return hipSuccess;
	TilesArgs A;
	A.S = S;
	A.P = P;
	void (*const fn)(const TilesArgs) = method == 0 ? (prune ? tiles_kernel<0, true> : tiles_kernel<0, false>)
	                                                : (prune ? tiles_kernel<1, true> : tiles_kernel<1, false>);
	const hipError_t e = launch_path_lanes(fn, groups, four_wave_stack_lds_bytes(S) + kTilesRecordLdsBytes, stream, A);
	if (e != hipSuccess || P.split == 1u || P.item_chunks != 1u)
		return e;
	hipLaunchKernelGGL(tiles_combine_kernel, dim3((64u * P.n_tiles + 255u) / 256u), dim3(256), 0, stream, P);
	return hipGetLastError();
}

// (mean_b, lbar_b, var_b) of a listed pixel's chunk sums into its state, by the routines of the whole-frame batch (rt_chunk_stats.h)
__global__ __launch_bounds__(256) void adaptive_fold_kernel(const DevFoldParams P)
{
	const uint32_t lane = threadIdx.x & 63u, slot = blockIdx.x * 4u + (threadIdx.x >> 6);
	if (slot >= P.n_tiles)
		return;
	const uint32_t tile = P.tiles[slot];
	if (tile >= P.tile_count)
		return;
	uint32_t x, y;
	if (!grid8_pixel(tile, lane, P.tiles_x, P.width, P.height, x, y))
		return;
	const size_t p = (size_t)y * P.width + x;
	const Demod d = demod_divisors(P.albedo, 3u * p);
	const ChunkStats b = chunk_stats(P.sums + 3u * ((size_t)64u * slot + lane), 3u * (size_t)64u * P.n_tiles, P.split, (float)P.chunk_passes, d);
	const uint32_t count = P.nb[p] + 1u; // the pixel's own batch count
	chunk_state_step<false>(p, P.mean_in, b, P.state_m, P.state_l, P.state_v, false, (float)count, P.out_mean, P.out_lum, P.out_var);
	P.nb[p] = count;
}

__global__ __launch_bounds__(256) void adaptive_fill_kernel(uint32_t *p, uint64_t n, uint32_t value)
{
	for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256u)
		p[i] = value;
}

hipError_t launch_adaptive_fold(hipStream_t stream, const DevFoldParams &P)
{
	hipLaunchKernelGGL(adaptive_fold_kernel, dim3((P.n_tiles + 3u) / 4u), dim3(256), 0, stream, P);
	return hipGetLastError();
}

hipError_t launch_fill_u32(hipStream_t stream, uint32_t *p, uint64_t n, uint32_t value)
{
	const uint64_t blocks = std::min<uint64_t>(std::max<uint64_t>((n + 255u) / 256u, 1u), 4096u);
	hipLaunchKernelGGL(adaptive_fill_kernel, dim3((uint32_t)blocks), dim3(256), 0, stream, p, n, value);
	return hipGetLastError();
}

hipError_t launch_select_tiles(hipStream_t stream, const DevSelectParams &P)
{
	hipLaunchKernelGGL(select_tiles_kernel, dim3(1), dim3(256), 0, stream, P);
	return hipGetLastError();
}

} // namespace rt
