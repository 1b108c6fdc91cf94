// rt_lens.hip -- whole frames through a camera MODEL (rt_render_lens, include/rt_hip.h): the thin lens the reference's SimpleCamera
// stores and never uses, and the orthographic, equidistant-fisheye and equirectangular projections.  The ray of a sample is made ON
// THE DEVICE, per sample, so a frame costs no ray upload (rt_radiance would need one rt_ray_desc per sample).
//
// lens_kernel is tiles_kernel (rt_adaptive.hip) with another START around the same per-lane integrator,
// rt_path_lane.h (its header describes the phases, the quorum and the hand-out).  This file holds:
//   START   the camera stream (seed, 2^63 + pixel, sample_begin + pass): the jitter and, for a lens, the lens point; the ray of the
//           projection -- a WAVE-UNIFORM switch on a launch constant, each arm straight-line code; then the path's own stream
//           (seed, pixel, sample_begin + pass) FROM ITS FIRST DRAW: sample n of rt_radiance with streams[i] = pixel.  A fisheye sample
//           outside the image circle is +0: the lane goes START -> FINISH and enters no walk
//   FINISH  tiles_kernel's, restated: the NaN filter, then the fold rt_render_opts states
//   CLAIM   tiles_kernel's without a list: item i is tile i / (split / item_chunks)
// The loop keeps ONE back edge.  A lane whose sample is black waits in FINISH through the walk of its wave (which does nothing for
// it) and folds at the top of the next trip, so every trip advances its pass counter by one: tests/test_lens.py restates the walk.
// The camera is read from the kernel arguments where START uses it (aov_kargs) and held nowhere else.
//
// Ray counters: tiles_kernel's (the functor handed to path_lane_walk); a black sample shoots none.
#include "rt_path_lane.h"
#include "rt_lens.h"
#include "rt_chunk_stats.h"

namespace rt {

struct LensArgs {
	DevScene S;
	DevLensParams P;
};

// lanes of the wave that must wait for a closest-hit walk before it runs while shadow rays are pending elsewhere (as kTilesQuorum)
#ifndef RT_LENS_QUORUM
#define RT_LENS_QUORUM 32
#endif
constexpr uint32_t kLensQuorum = RT_LENS_QUORUM;

// three floats of the kernel arguments as a vector, loaded where they are used
#define RT_LENS_V3(field) v3(ka->P.field[0], ka->P.field[1], ka->P.field[2])

template <int METHOD, bool PRUNE>
__global__ __launch_bounds__(256, kLensWaves) void lens_kernel(const LensArgs args_by_value)
{
	using F = FeatFull; // every primitive, material and texture type compiled in (as tiles_kernel)
	extern __shared__ __align__(16) uint32_t lds[];
	const DevScene &S = args_by_value.S;
	const WaveStack W = wave_stack(S, lds);
	// behind the stacks: the lane's FOLD RECORD (tiles_kernel's: word w of thread t at rec[256 w])
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
		// ---- FINISH: the sample's value, then the fold of rt_render_opts.sample_split (tiles_kernel's) ----
		if (L.ph >= PH_FINISH) {
			const V3 v = L.sample_value();
			const KArgPtr<LensArgs> ka = aov_kargs(args_by_value);
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
			{ // (a pass shoots fewer than 2^31 rays: the lane's counter cannot wrap)
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
				} else if (sums != nullptr) { // the item was this chunk: [chunk][64 * tile + place][3]
					const uint32_t id = rec[R_ID];
					const uint32_t item = id >> 6, tile = item / split, c = item - tile * split;
					float *const o = sums + 3u * ((size_t)c * 64u * ka->P.n_tiles + (64u * tile + (id & 63u)));
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
		// ---- CLAIM: the next lane slot of the wave's item -> tile, chunk and pixel (no list: the tile is the item's) ----
		const uint64_t need = __ballot(L.ph == PH_CLAIM);
		if (need != 0ull) { // (wave-uniform)
			const KArgPtr<LensArgs> ka = aov_kargs(args_by_value);
			const uint32_t n = ka->P.n_lanes;
			if (L.ph == PH_CLAIM) {
				const uint32_t id = blocks.claimed(need);
				if (id >= n) {
					L.ph = PH_DONE;
				} else {
					const uint32_t split = ka->P.split, item_chunks = ka->P.item_chunks, spp = ka->P.spp;
					const uint32_t per_tile = item_chunks == 1u ? split : 1u; // items a tile is
					const uint32_t item = id >> 6, place = id & 63u;
					const uint32_t tile = item / per_tile, c0 = (item - tile * per_tile) * item_chunks; // (tile < n_tiles: id < n_lanes)
					const uint32_t width = ka->P.width;
					uint32_t x, y;
					if (!grid8_pixel(tile, place, ka->P.tiles_x, width, ka->P.height, x, y)) {
						// padding of an edge tile (ph stays CLAIM: the lane takes another slot next iteration)
						float *const sums = ka->P.chunk_sums;
						if (split > 1u && sums != nullptr) {
							float *const o = sums + 3u * ((size_t)c0 * 64u * ka->P.n_tiles + (64u * tile + place));
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
		// ---- START: the next pass of the pixel through the camera model (rt_hip.h states every expression; all of it f32, in
		// the written order) ----
		if (L.ph == PH_START) {
			const KArgPtr<LensArgs> ka = aov_kargs(args_by_value);
			const uint64_t seed = ((uint64_t)ka->P.seed_hi << 32) | ka->P.seed_lo;
			const uint64_t sample_begin = ((uint64_t)ka->P.sample_begin_hi << 32) | ka->P.sample_begin_lo;
			const uint32_t width = ka->P.width, height = ka->P.height;
			const uint32_t pixel = rec[R_PIXEL], k = rec[R_PASS];
			const uint32_t py = pixel / width, px = pixel - py * width;
			const int32_t projection = ka->P.projection;
			rt_rng cam; // the camera stream: no pixel's path stream (pixels are below 2^31)
			rt_rng_seed(&cam, seed, 0x8000000000000000ull + (uint64_t)pixel, sample_begin + k);
			const float jx = rt_rng_range_f32(&cam, 0.0f, 1.0f) + (float)px, jy = rt_rng_range_f32(&cam, 0.0f, 1.0f) + (float)py;
			const float s = jx / (float)(width - 1u);
			const float t = 1.0f - jy / (float)(height - 1u);
			V3 o, d;
			bool black = false;
			if (projection == kProjPerspective) { // (wave-uniform, as every arm below)
				const float lens_radius = ka->P.lens_radius;
				o = RT_LENS_V3(cam.origin);
				d = RT_LENS_V3(cam.lower_left) + RT_LENS_V3(cam.horizontal) * s + RT_LENS_V3(cam.vertical) * t - o; // get_ray  camera.rs:57-63
				if (lens_radius != 0.0f) { // the thin lens focused on the plane focus_dist scales the viewport to
					const float xi1 = rt_rng_f32(&cam), xi2 = rt_rng_f32(&cam);
					const float r = lens_radius * sqrtf(xi1);
					const float phi = RT_TAU * xi2;
					const V3 off = RT_LENS_V3(right) * (r * rt_cosf(phi)) + RT_LENS_V3(up) * (r * rt_sinf(phi));
					o = o + off;
					d = d - off;
				}
			} else if (projection == kProjOrthographic) {
				o = RT_LENS_V3(cam.lower_left) + RT_LENS_V3(cam.horizontal) * s + RT_LENS_V3(cam.vertical) * t;
				d = RT_LENS_V3(forward);
			} else if (projection == kProjFisheye) { // equidistant: the angle from the axis grows with the radius in the image circle
				const float a = 2.0f * s - 1.0f;
				const float b = (2.0f * t - 1.0f) * ((float)(height - 1u) / (float)(width - 1u));
				const float rho = sqrtf(a * a + b * b);
				black = !(rho <= 1.0f); // outside the circle, or NaN
				const float theta = rho * ka->P.fisheye_half_angle;
				const float sin_t = rt_sinf(theta);
				const V3 fwd = RT_LENS_V3(forward);
				o = RT_LENS_V3(cam.origin);
				d = RT_LENS_V3(right) * (sin_t * (a / rho)) + RT_LENS_V3(up) * (sin_t * (b / rho)) + fwd * rt_cosf(theta);
				if (rho == 0.0f)
					d = fwd;
			} else { // kProjEquirect
				const float lon = (2.0f * s - 1.0f) * RT_PI;
				const float lat = (2.0f * t - 1.0f) * RT_FRAC_PI_2;
				const float cos_lat = rt_cosf(lat);
				o = RT_LENS_V3(cam.origin);
				d = RT_LENS_V3(right) * (cos_lat * rt_sinf(lon)) + RT_LENS_V3(up) * rt_sinf(lat) + RT_LENS_V3(forward) * (cos_lat * rt_cosf(lon));
			}
			if (black) { // +0 in all channels: no path, no integrator draw, no ray counted
				L.outp = v3s(0.0f);
				L.ph = PH_FINISH;
			} else {
				rt_rng_seed(&L.rng, seed, (uint64_t)pixel, sample_begin + k); // the path's stream from its first draw
				L.ray = ray_new<F>(o, d);
				L.start();
			}
		}

		const uint64_t m_closest = __ballot(L.ph == PH_CLOSEST), m_shadow = __ballot(L.ph == PH_SHADOW);
		// no walk is waiting and every lane is DONE (a lane may wait in CLAIM: its slot was padding; or in FINISH: its sample was black)
		if ((m_closest | m_shadow) == 0ull && __ballot(L.ph != PH_DONE) == 0ull)
			break;
		// (the walk falls through when no lane waits for one: a `continue` would be the loop's second back edge)
		path_lane_walk<METHOD, PRUNE, kLensQuorum, F>(L, args_by_value, W, m_closest, m_shadow, count_ray);
	}

	// ---- SamplerProgress.rays_shot: wave reduction, one atomic per wave (as tiles_kernel) ----
	unsigned long long *const rays_shot = aov_kargs(args_by_value)->P.rays_shot;
	if (rays_shot != nullptr) {
		unsigned long long total = rec[R_RAYS];
		for (int off = 32; off > 0; off >>= 1)
			total += __shfl_down(total, off);
		if ((threadIdx.x & 63u) == 0u)
			atomicAdd(rays_shot, total);
	}
}
#undef RT_LENS_V3

// the counter of a launch zeroed by a kernel, not a memset node (rt_render.hip reset_kernel says why)
__global__ void lens_zero_kernel(unsigned long long *rays_shot) { *rays_shot = 0ull; }

// chunk_sums -> the frame: the S sums added in chunk order from +0, divided by spp once (combine_chunks_kernel's arithmetic)
__global__ __launch_bounds__(256) void lens_combine_kernel(const DevLensParams P)
{
	const uint32_t i = blockIdx.x * 256u + threadIdx.x; // 64 * tile + place
	if (i >= 64u * P.n_tiles)
		return;
	uint32_t x, y;
	if (!grid8_pixel(i >> 6, i & 63u, P.tiles_x, P.width, P.height, x, y))
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

hipError_t launch_lens(int method, bool prune, hipStream_t stream, const DevScene &S, const DevLensParams &P, uint32_t groups)
{
	if (P.rays_shot != nullptr) {
		hipLaunchKernelGGL(lens_zero_kernel, dim3(1), dim3(1), 0, stream, P.rays_shot);
		const hipError_t e = hipGetLastError();
		if (e != hipSuccess)
			return e;
	}
	LensArgs A;
	A.S = S;
	A.P = P;
	void (*const fn)(const LensArgs) = method == 0 ? (prune ? lens_kernel<0, true> : lens_kernel<0, false>)
	                                               : (prune ? lens_kernel<1, true> : lens_kernel<1, false>);
	const hipError_t e = launch_path_lanes(fn, groups, four_wave_stack_lds_bytes(S) + kLensRecordLdsBytes, stream, A);
	if (e != hipSuccess || P.split == 1u || P.item_chunks != 1u)
		return e;
	hipLaunchKernelGGL(lens_combine_kernel, dim3((64u * P.n_tiles + 255u) / 256u), dim3(256), 0, stream, P);
	return hipGetLastError();
}

} // namespace rt
