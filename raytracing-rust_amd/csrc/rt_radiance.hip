// rt_radiance.hip -- radiance queries (rt_radiance, include/rt_hip.h): NaiveIntegrator / MisIntegrator::get_colour on rays the
// caller supplies, K samples a ray, on the stream (seed, stream_i, sample_begin + k) with NO draw ahead of the integrator.  The
// integrator is the one of rt_render.hip's SHADE / LIGHT / SCATTER arms, written once more as a per-lane loop over the device
// functions of rt_shade.h / rt_intersect.h; the CPU checker's fixed-ray integrator is its counterpart, bit for bit.
//
// The shape of ao_kernel (rt_ao.hip) taken one step further.  Paths end after 1 to 49 bounces and under MIS every bounce is two
// walks (the shadow ray, the scattered ray), so every lane is a state machine and the WAVE decides by ballot what an iteration
// runs:
//   FINISH  a sample ended: the NaN filter, the ray's sum; the next sample of the ray (START) or the output and CLAIM
//   CLAIM   the next ray of the wave's block of 64 (refill in place); none left: DONE
//   START   ray and stream of sample k: Ray::new, rt_rng_seed
//   CLOSEST trace_closest on `ray` (primary and scattered rays alike), then the shading of what it reached -- naive: the whole
//           loop body; MIS: the prologue or the material-sampling half, then sample_lights up to the shadow ray (-> SHADOW)
//   SHADOW  trace_any on the shadow ray (sky: no limit; emissive primitive: its own t the limit, its slot skipped), the light's
//           contribution, scatter_ray (-> CLOSEST)
// FINISH, CLAIM and START run whenever a lane waits in them (they are short); of the two walks an iteration runs ONE: the
// closest-hit step when no shadow ray is pending or at least kRadianceQuorum lanes wait for it, else the shadow step.  Each walk
// is compiled in once.  A lane works through its rays, their samples and each path strictly in order and no value crosses lanes,
// so neither the quorum nor the hand-out can change a bit of the result.
//
// Hand-out: wave w of W takes the blocks of 64 rays w, w + W, w + 2 W, ... -- a cursor in the wave's own registers.  There is no
// counter in memory: nothing to reset ahead of a launch, nothing two launches in flight could share.
//
// Carried across the walks: the ray (the shadow ray and the path ray take turns: scatter_ray needs only `wo` of the latter), the
// whole Hit (the emission of what a scattered ray reaches is evaluated against the PREVIOUS hit, mis.rs:55), its material handle,
// wo, throughput, the sample's output, the ray's sum, depth, the stream, the pending light sample (l_wi, t_limit, skip), id and k.
// Launch parameters are read through the opaque kernarg pointer where they are used.  No array is indexed dynamically.
#include "rt_aov_common.h"
#include "rt_radiance.h"

namespace rt {

struct RadianceArgs {
	DevScene S;
	DevRadianceParams P;
};

namespace {

// lanes of the wave that must wait for a closest-hit walk before it runs while shadow rays are pending elsewhere
// 
#ifndef RT_RADIANCE_QUORUM
#define RT_RADIANCE_QUORUM 32
#endif
constexpr uint32_t kRadianceQuorum = RT_RADIANCE_QUORUM;

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

// bvh.get_samplable().contains(&index): Bvh.lights is exactly the primitives whose material is_light() (acceleration/mod.rs:84-88),
// so the material of the primitive that was hit answers it (`prim_mat`: its handle, as make_hit returns it)
__device__ __forceinline__ bool prim_in_light_list(const DevScene &S, uint32_t prim, uint32_t prim_mat)
{
	return prim != kNoPrim && mat_is_light(S, prim_mat);
}

// how many things sample_lights chooses among (mis.rs:135-157): the emissive primitives, and the sky when it can be sampled
__device__ __forceinline__ uint32_t light_choices(const DevScene &S) { return sky_can_sample(S) ? S.n_lights + 1u : S.n_lights; }

// Bvh::get_pdf_from_index  acceleration/mod.rs:299-318: the pdf with which sample_lights would have produced `wi` from `last`,
// given that `wi` reached primitive `prim` at `now` (kNoPrim: the sky)
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
__global__ __launch_bounds__(256, kRadianceWaves) void radiance_kernel(const RadianceArgs args_by_value)
{
	using F = FeatFull; // every primitive, material and texture type compiled in (as the batch queries and the AOV passes)
	extern __shared__ __align__(16) uint32_t lds[];
	const DevScene &S = args_by_value.S;
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	uint32_t *stk = lds + wave * (S.stack_depth * kStackStride) + lane;
	// the whole worst case in LDS: the overflow branch is never taken (its base only has to be some global pointer, rt_query.hip)
	const StackMem SM = {S.stack_depth, 0u, const_cast<uint32_t *>(S.prim_rank), lds};

	// the wave's hand-out: rays [wq_next, wq_end) of its current block; `block` the next one it takes
	const uint32_t n_waves = gridDim.x * kFourWaves;
	uint32_t wq_next = 0u, wq_end = 0u, block = blockIdx.x * kFourWaves + wave;

	// ---- per-lane state ----
	int ph = PH_CLAIM;
	uint32_t id = 0u, k = 0u; // the ray, and the sample of it in flight
	V3 sum = v3s(0.0f);       // of the ray's samples so far, in order
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
		// ---- FINISH: integrators/mod.rs:74-76, mis.rs:88-90, then the output rule of rt_radiance ----
		if (ph >= PH_FINISH) {
			V3 c = outp;
			if (ph == PH_FINISH && (contains_nan(c) || !is_finite_any(c)))
				c = v3s(0.0f);
			sum.x += c.x;
			sum.y += c.y;
			sum.z += c.z;
			k += 1u;
			const KArgPtr<RadianceArgs> ka = aov_kargs(args_by_value);
			const uint32_t samples = ka->P.samples;
			if (k < samples) {
				ph = PH_START;
			} else {
				float *const o = ka->P.out + 3u * (size_t)id;
				const float n = (float)samples;
				o[0] = sum.x / n;
				o[1] = sum.y / n;
				o[2] = sum.z / n;
				ph = PH_CLAIM;
			}
		}
		// ---- CLAIM: refill in place from the wave's block (as trace_queue_kernel, rt_query.hip, without its counter) ----
		const uint64_t need = __ballot(ph == PH_CLAIM);
		if (need != 0ull) { // (wave-uniform)
			const uint32_t n = aov_kargs(args_by_value)->P.n_rays;
			const uint32_t cnt = (uint32_t)__popcll(need), avail = wq_end - wq_next;
			const uint32_t base = block * 64u;
			if (ph == PH_CLAIM) {
				const uint32_t r = (uint32_t)__popcll(need & ((1ull << lane) - 1ull));
				id = r < avail ? wq_next + r : base + (r - avail);
				if (id >= n) {
					ph = PH_DONE;
				} else {
					k = 0u;
					sum = v3s(0.0f);
					ph = PH_START;
				}
			}
			if (avail < cnt) {
				wq_next = base + (cnt - avail);
				wq_end = base + 64u;
				if (base < n) // (past the batch every claim ends its lane: the cursor stays, so it cannot wrap)
					block += n_waves;
			} else {
				wq_next += cnt;
			}
		}
		// ---- START: sample k of ray id.  No draw before the integrator: no jitter, no camera time ----
		if (ph == PH_START) {
			const KArgPtr<RadianceArgs> ka = aov_kargs(args_by_value);
			const float *const rp = ka->P.rays + 6u * (size_t)id;
			const uint64_t *const streams = ka->P.streams;
			const uint64_t stream = streams != nullptr ? streams[id] : (uint64_t)id;
			const uint64_t seed = ((uint64_t)ka->P.seed_hi << 32) | ka->P.seed_lo;
			const uint64_t sample_begin = ((uint64_t)ka->P.sample_begin_hi << 32) | ka->P.sample_begin_lo;
			rt_rng_seed(&rng, seed, stream, sample_begin + k);
			ray = ray_new<F>(v3(rp[0], rp[1], rp[2]), v3(rp[3], rp[4], rp[5]));
			thr = v3s(1.0f);
			outp = v3s(0.0f);
			depth = 0u;
			primary = true;
			ph = PH_CLOSEST;
		}

		const uint64_t m_closest = __ballot(ph == PH_CLOSEST), m_shadow = __ballot(ph == PH_SHADOW);
		if ((m_closest | m_shadow) == 0ull)
			break; // every lane is DONE (FINISH, CLAIM and START were emptied above)

		if (METHOD == 0 || m_shadow == 0ull || (uint32_t)__popcll(m_closest) >= kRadianceQuorum) { // (wave-uniform)
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
						const KArgPtr<RadianceArgs> ka = aov_kargs(args_by_value);
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
							const KArgPtr<RadianceArgs> ka = aov_kargs(args_by_value);
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
						const KArgPtr<RadianceArgs> ka = aov_kargs(args_by_value);
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
						const KArgPtr<RadianceArgs> ka = aov_kargs(args_by_value);
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
						const KArgPtr<RadianceArgs> ka = aov_kargs(args_by_value);
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
}

hipError_t launch_radiance(int method, bool prune, hipStream_t stream, const DevScene &S, const DevRadianceParams &P, uint32_t groups)
{
	RadianceArgs A;
	A.S = S;
	A.P = P;
	void (*const fn)(const RadianceArgs) = method == 0 ? (prune ? radiance_kernel<0, true> : radiance_kernel<0, false>)
	                                                   : (prune ? radiance_kernel<1, true> : radiance_kernel<1, false>);
	const size_t lds_bytes = four_wave_stack_lds_bytes(S);
	// deep trees: more than the default 64 KB of dynamic LDS per workgroup
	const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
	if (e != hipSuccess)
		return e;
	hipLaunchKernelGGL(fn, dim3(groups), dim3(256), lds_bytes, stream, A);
	return hipGetLastError();
}

} // namespace rt
