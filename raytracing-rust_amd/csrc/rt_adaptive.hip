// rt_adaptive.hip -- the render on a LIST of 8 x 8 tiles (rt_render_tiles, include/rt_hip.h) and the selection of the tiles
// whose error is above a threshold (rt_noise_select_tiles): what per-tile refinement and a region render need of the device.
//
// tiles_kernel is radiance_kernel (rt_radiance.hip) with another START and another FINISH: every lane is
// the state machine FINISH / CLAIM / START / CLOSEST / SHADOW over the device functions of rt_shade.h / rt_intersect.h, the wave
// decides by ballot which of the two walks an iteration runs, and the integrator arms are restated here once more -- shared
// through a header they would have to be proven not to move radiance_kernel's register rows, which nothing here needs.
//   START   the render's own camera ray (rt_render.hip do_gen, rt_aov_common.h aov_camera_ray): the first two draws of the stream
//           (seed, pixel, sample_begin + pass) jitter the pixel, SimpleCamera::get_ray draws its unused time, and the path goes on
//           ON THAT STREAM
//   FINISH  the NaN filter, then the fold rt_render_opts states: split 1 the running mean `mean += (pass - mean) / i`, else the
//           chunk's sum in pass order from +0.  A chunk's end stores the sum (chunk_sums given) or adds it to the pixel's total in
//           chunk order, which the last chunk divides by spp once -- the bytes combine_chunks_kernel (rt_render.hip) produces
// Work items: item i is tile slot i / (split / item_chunks) of the list and `item_chunks` chunks of it from chunk
// (i % (split / item_chunks)) * item_chunks on; its 64 lane slots are the 64 pixels of the tile, row-major.  With a chunk buffer an
// item is ONE chunk, so that ten tiles at split 16 are 10 240 lanes of work and not 640; without one it is the whole pixel and the
// launch needs no memory besides the frame.  Hand-out as radiance_kernel's: wave w of W takes items w, w + W, ... and its lanes
// refill in place from the wave's current item -- a cursor in registers, no counter in memory, nothing two launches share.  A lane
// whose slot is padding of an edge tile writes +0 sums and claims again; a tile index past the grid is skipped whole.
//
// Ray counters: SamplerProgress.rays_shot as rt_render.hip counts it -- naive: one per walk of a path ray (do_shade), MIS: one per
// sample_lights call (do_light, mis.rs:38) -- summed per lane, reduced per wave, one atomic per wave.
//
// select_tiles_kernel: ONE workgroup walks the tile-error plane 256 tiles at a time; ballots and prefix counts place the indices
// above the threshold in ascending order, so the list is a pure function of the plane.
#include <algorithm>

#include "rt_aov_common.h"
#include "rt_adaptive.h"

namespace rt {

struct TilesArgs {
	DevScene S;
	DevTilesParams P;
};

namespace {

// lanes of the wave that must wait for a closest-hit walk before it runs while shadow rays are pending elsewhere (as
// kRadianceQuorum)
#ifndef RT_TILES_QUORUM
#define RT_TILES_QUORUM 32
#endif
constexpr uint32_t kTilesQuorum = RT_TILES_QUORUM;

enum : int { PH_CLAIM = 0, PH_START = 1, PH_CLOSEST = 2, PH_SHADOW = 3, PH_DONE = 4, PH_FINISH = 5, PH_FINISH_UNFILTERED = 6 };

__device__ __forceinline__ float power_heuristic(float pdf_a, float pdf_b) // rt_core/src/lib.rs:36-40
{
	const float a_sq = pdf_a * pdf_a;
	return a_sq / (a_sq + pdf_b * pdf_b);
}

// the sky's tables where they lie (global memory)
__device__ __forceinline__ SkyTables sky_tables(const DevScene &S, KWords inv_res)
{
	SkyTables T;
	T.row_cdf = S.sky.row_cdf;
	T.marginal_cdf = S.sky.marginal_cdf;
	T.guide = S.sky.guide;
	T.guide_k = S.sky.guide_k;
	T.inv_res = inv_res;
	return T;
}

// bvh.get_samplable().contains(&index) (acceleration/mod.rs:84-88): the material of the primitive that was hit answers it
__device__ __forceinline__ bool prim_in_light_list(const DevScene &S, uint32_t prim, uint32_t prim_mat)
{
	return prim != kNoPrim && mat_is_light(S, prim_mat);
}

// how many things sample_lights chooses among (mis.rs:135-157)
__device__ __forceinline__ uint32_t light_choices(const DevScene &S) { return sky_can_sample(S) ? S.n_lights + 1u : S.n_lights; }

// Bvh::get_pdf_from_index  acceleration/mod.rs:299-318
template <class F>
__device__ __forceinline__ float pdf_from_index(const DevScene &S, const SkyTables &T, const Hit &last, const Hit &now, V3 wi, uint32_t prim)
{
	if (prim == kNoPrim)
		return div_by_count(sky_pdf(S, T, wi), light_choices(S));
	const PrimGeom g = load_prim<F>(S, prim);
	return div_by_count(prim_scattering_pdf<F>(g, last.point, wi, now), light_choices(S));
}

} // namespace

template <int METHOD, bool PRUNE>
__global__ __launch_bounds__(256, kTilesWaves) void tiles_kernel(const TilesArgs args_by_value)
{
	using F = FeatFull; // every primitive, material and texture type compiled in (as radiance_kernel)
	extern __shared__ __align__(16) uint32_t lds[];
	const DevScene &S = args_by_value.S;
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	uint32_t *stk = lds + wave * (S.stack_depth * kStackStride) + lane;
	// the whole worst case in LDS: the overflow branch is never taken (its base only has to be some global pointer, rt_query.hip)
	const StackMem SM = {S.stack_depth, 0u, const_cast<uint32_t *>(S.prim_rank), lds};
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

	// the wave's hand-out: lane slots [wq_next, wq_end) of its current item; `block` the next item it takes
	const uint32_t n_waves = gridDim.x * kFourWaves;
	uint32_t wq_next = 0u, wq_end = 0u, block = blockIdx.x * kFourWaves + wave;

	// ---- per-lane state in registers: the path ----
	int ph = PH_CLAIM;
	rt_rng rng = {0u, 0u, 0u, 0u};
	Ray ray; // the path ray (CLOSEST) or the shadow ray (SHADOW)
	ray.o = ray.d = ray.inv = ray.shear = v3s(0.0f);
	V3 thr = v3s(1.0f), outp = v3s(0.0f), wo = v3s(0.0f);
	Hit hit; // MIS: the vertex the path stands on
	hit.t = 0.0f;
	hit.point = hit.error = hit.normal = v3s(0.0f);
	hit.err_dot = 0.0f;
	hit.uvx = hit.uvy = 0.0f;
	hit.has_uv = hit.out = false;
	uint32_t mat = 0u, depth = 0u;
	bool primary = true;
	// the light sample in flight (MIS): its direction as sampled, the shadow ray's limit (NaN: the sky, no limit) and the light's slot
	V3 l_wi = v3s(0.0f);
	float t_limit = 0.0f;
	uint32_t skip = kNoPrim;
	bool have_shadow = false; // false: sample_lights produced no shadow ray (the SHADOW step only scatters)

#pragma unroll 1
	for (;;) {
		// ---- FINISH: integrators/mod.rs:74-76, mis.rs:88-90, then the fold of rt_render_opts.sample_split ----
		if (ph >= PH_FINISH) {
			V3 v = outp;
			if (ph == PH_FINISH && (contains_nan(v) || !is_finite_any(v)))
				v = v3s(0.0f);
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
			ph = PH_START;
			if (k == rec[R_CHUNK_END]) {
				const uint32_t spp = ka->P.spp;
				float *const sums = ka->P.chunk_sums;
				if (split == 1u) {
					float *const o = ka->P.out + 3u * (size_t)rec[R_PIXEL];
					o[0] = sum.x;
					o[1] = sum.y;
					o[2] = sum.z;
					ph = PH_CLAIM;
				} else if (sums != nullptr) { // the item was this chunk: [chunk][64 * slot + place][3]
					const uint32_t id = rec[R_ID];
					const uint32_t item = id >> 6, slot = item / split, c = item - slot * split;
					float *const o = sums + 3u * ((size_t)c * 64u * ka->P.n_tiles + (64u * slot + (id & 63u)));
					o[0] = sum.x;
					o[1] = sum.y;
					o[2] = sum.z;
					ph = PH_CLAIM;
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
						ph = PH_CLAIM;
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
		// ---- CLAIM: refill in place from the wave's item (as radiance_kernel), then the lane slot -> tile, chunk and pixel ----
		const uint64_t need = __ballot(ph == PH_CLAIM);
		if (need != 0ull) { // (wave-uniform)
			const KArgPtr<TilesArgs> ka = aov_kargs(args_by_value);
			const uint32_t n = ka->P.n_lanes;
			const uint32_t cnt = (uint32_t)__popcll(need), avail = wq_end - wq_next;
			const uint32_t base = block * 64u;
			if (ph == PH_CLAIM) {
				const uint32_t r = (uint32_t)__popcll(need & ((1ull << lane) - 1ull));
				const uint32_t id = r < avail ? wq_next + r : base + (r - avail);
				if (id >= n) {
					ph = PH_DONE;
				} else {
					const uint32_t split = ka->P.split, item_chunks = ka->P.item_chunks, spp = ka->P.spp;
					const uint32_t per_tile = item_chunks == 1u ? split : 1u; // items a tile is
					const uint32_t item = id >> 6, place = id & 63u;
					const uint32_t slot = item / per_tile, c0 = (item - slot * per_tile) * item_chunks;
					const uint32_t tile = ka->P.tiles[slot]; // (slot < n_tiles: id < n_lanes)
					const uint32_t tiles_x = ka->P.tiles_x, width = ka->P.width;
					const uint32_t ty = tile / tiles_x, tx = tile - ty * tiles_x;
					const uint32_t x = 8u * tx + (place & 7u), y = 8u * ty + (place >> 3);
					if (tile >= ka->P.tile_count) {
						// not a tile of this frame: skipped whole (ph stays CLAIM: the lane takes another slot next iteration)
					} else if (x >= width || y >= ka->P.height) { // padding of an edge tile
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
						ph = PH_START;
					}
				}
			}
			if (avail < cnt) {
				wq_next = base + (cnt - avail);
				wq_end = base + 64u;
				if (base < n) // (past the list every claim ends its lane: the cursor stays, so it cannot wrap)
					block += n_waves;
			} else {
				wq_next += cnt;
			}
		}
		// ---- START: the next pass of the pixel.  random_sampler.rs:50-61 as rt_render.hip do_gen ----
		if (ph == PH_START) {
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
			rt_rng_seed(&rng, seed, (uint64_t)pixel, sample_begin + k);
			const float jx = rt_rng_range_f32(&rng, 0.0f, 1.0f) + (float)px, jy = rt_rng_range_f32(&rng, 0.0f, 1.0f) + (float)py;
			const float u = jx / (float)(width - 1u);
			const float v = 1.0f - jy / (float)(height - 1u);
			ray = ray_new<F>(cam_o, cam_ll + cam_h * u + cam_v * v - cam_o); // SimpleCamera::get_ray  camera.rs:57-63
			(void)rt_rng_f32(&rng);                                         // (its unused `time`)
			thr = v3s(1.0f);
			outp = v3s(0.0f);
			depth = 0u;
			primary = true;
			ph = PH_CLOSEST;
		}

		const uint64_t m_closest = __ballot(ph == PH_CLOSEST), m_shadow = __ballot(ph == PH_SHADOW);
		// no walk is waiting: every lane is DONE, or some claim again (their slot was padding or no tile)
		if ((m_closest | m_shadow) == 0ull && __ballot(ph == PH_CLAIM) == 0ull)
			break;

		if (METHOD == 0 || m_shadow == 0ull || (uint32_t)__popcll(m_closest) >= kTilesQuorum) { // (wave-uniform)
			// ---- CLOSEST: the walk of a path ray and the shading of what it reached ----
			if (ph == PH_CLOSEST) {
				float best_t;
				uint32_t prim;
				trace_closest<F, PRUNE>(S, S, SM, ray, stk, best_t, prim);
				Hit nh;
				uint32_t nmat;
				if (prim != kNoPrim)
					make_hit<F>(S, prim, ray, best_t, nh, nmat);
				else
					make_sky_hit(S, nh, nmat);
				bool finish = false, filter = true;
				if (METHOD == 0) {
					// ---- NaiveIntegrator::get_colour loop body  integrators/mod.rs:31-72 ----
					rec[R_RAYS] += 1u;
					const V3 wo_n = ray.d;
					const V3 emission = mat_get_emission<F>(S, nmat, nh, wo_n);
					const bool exit = mat_scatter_ray<F>(S, nmat, ray, nh, rng);
					if (depth == 0u) {
						outp = outp + emission;
						if (exit)
							finish = true;
					}
					if (!finish && exit) {
						outp = outp + thr * emission;
						finish = true;
					}
					if (!finish) {
						if (!mat_is_delta<F>(S, nmat))
							thr = thr * mat_eval_over_pdf<F>(S, nmat, nh, wo_n, ray.d);
						else
							thr = thr * mat_eval<F>(S, nmat, nh, wo_n, ray.d);
						const KArgPtr<TilesArgs> ka = aov_kargs(args_by_value);
						if (depth > ka->P.rr_threshold) {
							const float p = component_max(thr);
							if (rt_rng_f32(&rng) > p)
								finish = true;
							else
								thr = thr / p;
						}
						if (!finish) {
							depth += 1u;
							if (!(depth < ka->P.max_depth))
								finish = true;
						}
					}
					// (the path continues: `ray` already is the scattered ray, ph stays CLOSEST)
				} else if (primary) {
					// ---- MisIntegrator::get_colour prologue  mis.rs:17-33 ----
					wo = ray.d;
					hit = nh;
					mat = nmat;
					const V3 emission = mat_get_emission<F>(S, mat, hit, wo);
					Ray clone = ray; // scatter on a clone: the draws are consumed, the ray is discarded (mis.rs:25)
					const bool exit = mat_scatter_ray<F>(S, mat, clone, hit, rng);
					outp = outp + emission;
					if (exit) {
						finish = true;
						filter = false; // mis.rs:29-31 returns before the filter
					} else {
						depth = 1u;
						primary = false;
						if (!(depth < aov_kargs(args_by_value)->P.max_depth))
							finish = true;
					}
				} else {
					// ---- material-sampling half of the MIS loop  mis.rs:50-86 ----
					const V3 m_wi = ray.d;
					const float m_pdf = mat_scattering_pdf<F>(S, mat, hit, wo, m_wi);
					const V3 le = mat_get_emission<F>(S, nmat, hit /* the OLD hit, mis.rs:55 */, m_wi);
					thr = thr * mat_eval_over_pdf<F>(S, mat, hit, wo, m_wi);
					if (!is_zero(le)) {
						if ((prim_in_light_list(S, prim, nmat) && !mat_is_delta<F>(S, mat)) || (prim == kNoPrim && sky_can_sample(S))) {
							const KArgPtr<TilesArgs> ka = aov_kargs(args_by_value);
							const SkyTables T = sky_tables(S, reinterpret_cast<KWords>(&ka->S.sky.inv_res_ok));
							const float l_pdf = pdf_from_index<F>(S, T, hit, nh, m_wi, prim);
							const float mis_weight = power_heuristic(m_pdf, l_pdf);
							outp = outp + thr * le * mis_weight;
						} else {
							outp = outp + thr * le;
						}
					}
					if (mat_is_light(S, nmat)) {
						finish = true;
					} else {
						const KArgPtr<TilesArgs> ka = aov_kargs(args_by_value);
						if (depth > ka->P.rr_threshold) {
							const float p = component_max(thr);
							if (rt_rng_f32(&rng) > p)
								finish = true;
							else
								thr = thr / p;
						}
						if (!finish) {
							wo = m_wi;
							hit = nh;
							mat = nmat;
							depth += 1u;
							if (!(depth < ka->P.max_depth))
								finish = true;
						}
					}
				}
				if (finish) {
					ph = filter ? PH_FINISH : PH_FINISH_UNFILTERED;
				} else if (METHOD == 1) {
					// ---- sample_lights up to the shadow ray  mis.rs:95-157 ----
					rec[R_RAYS] += 1u; // mis.rs:38
					have_shadow = false;
					skip = kNoPrim;
					const uint32_t samplable_len = S.n_lights;
					const bool sky_samplable = sky_can_sample(S);
					bool pick_sky = false, pick_light = false;
					uint32_t light_slot = 0u;
					if (samplable_len == 0u) {
						pick_sky = sky_samplable; // (0, true) => sample_sky(1.0); (0, false) => None
					} else if (!sky_samplable) {
						light_slot = rt_rng_below(&rng, samplable_len); // gen_range(0..len)
						pick_light = true;
					} else {
						light_slot = rt_rng_below(&rng, samplable_len + 1u); // gen_range(0..=len)
						if (light_slot == samplable_len)
							pick_sky = true;
						else
							pick_light = true;
					}
					PrimGeom g;
					g.type = g.material = 0u;
					g.p0 = g.p1 = g.p2 = v3s(0.0f);
					if (pick_sky) {
						const KArgPtr<TilesArgs> ka = aov_kargs(args_by_value);
						const SkyTables T = sky_tables(S, reinterpret_cast<KWords>(&ka->S.sky.inv_res_ok));
						l_wi = sky_sample(S, T, rng);
						t_limit = __uint_as_float(0x7FC00000u); // NaN: any t > 0 occludes
						have_shadow = true;
					} else if (pick_light) {
						skip = S.lights[light_slot];
						g = load_prim<F>(S, skip);
						l_wi = prim_sample_visible_from_point<F>(g, hit.point, rng);
					}
					if (pick_sky || pick_light)
						ray = ray_new<F>(hit.point + 0.0001f * hit.normal, l_wi);
					if (pick_light) {
						float lt;
						if (prim_t<F>(g, ray, lt) && lt > 0.0f) { // Bvh::check_hit_index  mod.rs:231-242
							t_limit = lt;
							have_shadow = true;
						}
					}
					ph = PH_SHADOW;
				}
			}
		} else if (METHOD == 1) {
			// ---- SHADOW: the shadow walk, the light's contribution (mis.rs:39-43) and material sampling (mis.rs:46-49) ----
			if (ph == PH_SHADOW) {
				if (have_shadow && !trace_any<F, PRUNE>(S, S, SM, ray, stk, t_limit, skip)) {
					const bool is_sky = t_limit != t_limit;
					const uint32_t n_l = S.n_lights;
					// sample_lights' pdf_multiplier: 1 when the sky is all there is to choose
					const float pdf_multiplier = n_l == 0u ? 1.0f : 1.0f / (float)light_choices(S);
					bool valid = false;
					V3 le = v3s(0.0f);
					float l_pdf = 0.0f;
					if (is_sky) { // sample_sky  mis.rs:104-115
						const KArgPtr<TilesArgs> ka = aov_kargs(args_by_value);
						const SkyTables T = sky_tables(S, reinterpret_cast<KWords>(&ka->S.sky.inv_res_ok));
						le = mat_get_emission<F>(S, S.sky.material, hit, l_wi);
						l_pdf = sky_pdf(S, T, l_wi) * pdf_multiplier;
						valid = true;
					} else { // sample_light  mis.rs:117-133 (`ray` still is the shadow ray)
						Hit lh;
						uint32_t lm;
						make_hit<F>(S, skip, ray, t_limit, lh, lm);
						const PrimGeom g = load_prim<F>(S, skip);
						const float p = prim_scattering_pdf<F>(g, hit.point, l_wi, lh);
						if (p > 0.0f) {
							le = mat_get_emission<F>(S, lm, lh, l_wi);
							l_pdf = p * pdf_multiplier;
							valid = true;
						}
					}
					if (valid) { // mis.rs:39-43
						const float m_pdf = mat_scattering_pdf<F>(S, mat, hit, wo, l_wi);
						const float mis_weight = power_heuristic(l_pdf, m_pdf);
						outp = outp + thr * mat_eval<F>(S, mat, hit, wo, l_wi) * mis_weight * le / l_pdf;
					}
				}
				// scatter_ray reads only the incoming direction of the ray that produced `hit`, which is `wo` (mis.rs:21,82)
				ray.d = wo;
				if (mat_scatter_ray<F>(S, mat, ray, hit, rng))
					ph = PH_FINISH;
				else
					ph = PH_CLOSEST;
			}
		}
	}

	// ---- SamplerProgress.rays_shot: wave reduction, one atomic per wave (as rt_render.hip) ----
	unsigned long long *const rays_shot = aov_kargs(args_by_value)->P.rays_shot;
	if (rays_shot != nullptr) {
		unsigned long long total = rec[R_RAYS];
		for (int off = 32; off > 0; off >>= 1)
			total += __shfl_down(total, off);
		if (lane == 0u)
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
	const uint32_t ty = tile / P.tiles_x, tx = tile - ty * P.tiles_x;
	const uint32_t x = 8u * tx + (place & 7u), y = 8u * ty + (place >> 3);
	if (x >= P.width || y >= P.height)
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
	const size_t lds_bytes = four_wave_stack_lds_bytes(S) + kTilesRecordLdsBytes;
	// deep trees: more than the default 64 KB of dynamic LDS per workgroup
	hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
	if (e != hipSuccess)
		return e;
	hipLaunchKernelGGL(fn, dim3(groups), dim3(256), lds_bytes, stream, A);
	e = hipGetLastError();
	if (e != hipSuccess || P.split == 1u || P.item_chunks != 1u)
		return e;
	hipLaunchKernelGGL(tiles_combine_kernel, dim3((64u * P.n_tiles + 255u) / 256u), dim3(256), 0, stream, P);
	return hipGetLastError();
}

// the denoiser's lum, left to right (rt_post_common.h lum; restated: this file does not include the post-processing header)
__device__ __forceinline__ float fold_lum(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }

__global__ __launch_bounds__(256) void adaptive_fold_kernel(const DevFoldParams P)
{
	const uint32_t lane = threadIdx.x & 63u, slot = blockIdx.x * 4u + (threadIdx.x >> 6);
	if (slot >= P.n_tiles)
		return;
	const uint32_t tile = P.tiles[slot];
	if (tile >= P.tile_count)
		return;
	const uint32_t ty = tile / P.tiles_x, tx = tile - ty * P.tiles_x;
	const uint32_t x = 8u * tx + (lane & 7u), y = 8u * ty + (lane >> 3);
	if (x >= P.width || y >= P.height)
		return;
	const size_t p = (size_t)y * P.width + x, p3 = 3u * p;
	float d0 = 1.0f, d1 = 1.0f, d2 = 1.0f;
	if (P.albedo) {
		d0 = fmaxf(P.albedo[p3], 1e-3f);
		d1 = fmaxf(P.albedo[p3 + 1u], 1e-3f);
		d2 = fmaxf(P.albedo[p3 + 2u], 1e-3f);
	}
	const float n = (float)P.chunk_passes, s = (float)P.split;
	const float *const first = P.sums + 3u * ((size_t)64u * slot + lane);
	const size_t stride = 3u * (size_t)64u * P.n_tiles;
	float lsum = 0.0f;
	for (uint32_t c = 0; c < P.split; ++c) { // (the sums are read twice: no array, nothing indexed by the loop)
		const float *m = first + c * stride;
		lsum = lsum + fold_lum(m[0] / n / d0, m[1] / n / d1, m[2] / n / d2);
	}
	const float lbar = lsum / s;
	float sq = 0.0f;
	for (uint32_t c = 0; c < P.split; ++c) {
		const float *m = first + c * stride;
		const float dl = fold_lum(m[0] / n / d0, m[1] / n / d1, m[2] / n / d2) - lbar;
		sq = sq + dl * dl;
	}
	const float var = sq / (float)(P.split * (P.split - 1u));
	const float m0 = P.state_m[p3] + P.mean_in[p3], m1 = P.state_m[p3 + 1u] + P.mean_in[p3 + 1u], m2 = P.state_m[p3 + 2u] + P.mean_in[p3 + 2u];
	const float l = P.state_l[p] + lbar, v = P.state_v[p] + var;
	const uint32_t count = P.nb[p] + 1u;
	P.state_m[p3] = m0;
	P.state_m[p3 + 1u] = m1;
	P.state_m[p3 + 2u] = m2;
	P.state_l[p] = l;
	P.state_v[p] = v;
	P.nb[p] = count;
	const float nb = (float)count;
	P.out_mean[p3] = m0 / nb;
	P.out_mean[p3 + 1u] = m1 / nb;
	P.out_mean[p3 + 2u] = m2 / nb;
	P.out_lum[p] = l / nb;
	P.out_var[p] = v / (nb * nb);
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
