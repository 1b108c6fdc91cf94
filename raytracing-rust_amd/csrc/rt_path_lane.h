// rt_path_lane.h -- the per-lane path integrator radiance_kernel (rt_radiance.hip) and tiles_kernel
// (rt_adaptive.hip, section 22) share, written ONCE: NaiveIntegrator / MisIntegrator::get_colour as a state machine over the device
// functions of rt_shade.h / rt_intersect.h (the code of rt_render.hip's SHADE / LIGHT / SCATTER arms in their general forms).
//
// Paths end after 1 to 49 bounces and under MIS every bounce is two walks (the shadow ray, the scattered ray), so every lane is a
// state machine and the WAVE decides by ballot what an iteration of the kernel's loop runs:
//   FINISH  a sample ended: the kernel folds PathLane::sample_value() its own way; the next sample (START) or CLAIM
//   CLAIM   the next slot of the wave's block of 64 (WaveBlocks: refill in place); none left: DONE.  What a slot is, is the kernel's
//   START   the kernel's ray and stream of the sample, then PathLane::start()
//   CLOSEST trace_closest on `ray` (primary and scattered rays alike), then the shading of what it reached -- naive: the whole
//           loop body; MIS: the prologue or the material-sampling half, then sample_lights up to the shadow ray (-> SHADOW)
//   SHADOW  trace_any on the shadow ray (sky: no limit; emissive primitive: its own t the limit, its slot skipped), the light's
//           contribution, scatter_ray (-> CLOSEST)
// FINISH, CLAIM and START are the kernels' and run whenever a lane waits in them (they are short); of the two walks an iteration
// runs ONE (path_lane_walk): the closest-hit step when no shadow ray is pending or at least QUORUM lanes wait for it, else the
// shadow step.  Each walk is compiled in once.  A lane works through its slots, their samples and each path strictly in order and
// no value crosses lanes, so neither the quorum nor the hand-out can change a bit of the result.
//
// What the kernels' loops must keep (section 22 records the cost of each): ONE back edge (no `continue`), `#pragma unroll 1`, no
// dynamically indexed array, launch parameters read through the opaque kernarg pointer (aov_kargs) where they are used.
//
// For rt_radiance.hip and rt_adaptive.hip ONLY.  The enum and the helpers below are plain names of namespace rt (every function
// __forceinline__, the units built without relocatable device code): rt_render.hip keeps a power_heuristic of its own for its
// specialised arms, so a unit that includes both would see an ambiguous overload -- a third user moves them into a namespace first.
#pragma once
#include "rt_aov_common.h"

namespace rt {

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

// the lane's stack column and the workgroup's stacks: the whole worst case in LDS, so the overflow branch is never taken (its base
// only has to be some global pointer, rt_query.hip)
struct WaveStack {
	uint32_t *stk;
	StackMem SM;
};
__device__ __forceinline__ WaveStack wave_stack(const DevScene &S, uint32_t *lds)
{
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	return {lds + wave * (S.stack_depth * kStackStride) + lane, {S.stack_depth, 0u, const_cast<uint32_t *>(S.prim_rank), lds}};
}

// The wave's hand-out: wave w of W takes the blocks of 64 slots w, w + W, w + 2 W, ... -- a cursor in the wave's own registers
// (the ballot / prefix-count refill of trace_queue_kernel, rt_query.hip, without its counter).  There is no counter in memory:
// nothing to reset ahead of a launch, nothing two launches in flight could share.
struct WaveBlocks {
	uint32_t wq_next = 0u, wq_end = 0u; // slots [wq_next, wq_end) of the current block are still to be handed out
	uint32_t block;                     // the next block the wave takes
	const uint32_t n_waves;             // W (kept, not read from the grid at each advance: that form moved the MIS kernels' SGPR spills)

	__device__ __forceinline__ WaveBlocks() : block(blockIdx.x * kFourWaves + (threadIdx.x >> 6)), n_waves(gridDim.x * kFourWaves) {}

	// the slot of a lane of `need` (the ballot of the lanes that claim): its rank among them, from the cursor on
	__device__ __forceinline__ uint32_t claimed(uint64_t need) const
	{
		const uint32_t lane = threadIdx.x & 63u, avail = wq_end - wq_next;
		const uint32_t r = (uint32_t)__popcll(need & ((1ull << lane) - 1ull));
		return r < avail ? wq_next + r : block * 64u + (r - avail);
	}
	// the cursor past the slots `need` took, of `n` in all (wave-uniform)
	__device__ __forceinline__ void advance(uint64_t need, uint32_t n)
	{
		const uint32_t cnt = (uint32_t)__popcll(need), avail = wq_end - wq_next;
		const uint32_t base = block * 64u;
		if (avail < cnt) {
			wq_next = base + (cnt - avail);
			wq_end = base + 64u;
			if (base < n) // (past the end every claim ends its lane: the cursor stays, so it cannot wrap)
				block += n_waves;
		} else {
			wq_next += cnt;
		}
	}
};

// Carried across the walks: the ray (the shadow ray and the path ray take turns: scatter_ray needs only `wo` of the latter), the
// whole Hit (the emission of what a scattered ray reaches is evaluated against the PREVIOUS hit, mis.rs:55), its material handle,
// wo, throughput, the sample's output, depth, the stream and the pending light sample.
struct PathLane {
	int ph = PH_CLAIM;
	rt_rng rng = {0u, 0u, 0u, 0u};
	Ray ray; // the path ray (CLOSEST) or the shadow ray (SHADOW)
	V3 thr = v3s(1.0f), outp = v3s(0.0f), wo = v3s(0.0f);
	Hit hit; // MIS: the vertex the path stands on
	uint32_t mat = 0u, depth = 0u;
	bool primary = true;
	// the light sample in flight (MIS): its direction as sampled, the shadow ray's limit (NaN: the sky, no limit) and the light's slot
	V3 l_wi = v3s(0.0f);
	float t_limit = 0.0f;
	uint32_t skip = kNoPrim;
	bool have_shadow = false; // false: sample_lights produced no shadow ray (the SHADOW step only scatters)

	__device__ __forceinline__ PathLane()
	{
		ray.o = ray.d = ray.inv = ray.shear = v3s(0.0f);
		hit.t = 0.0f;
		hit.point = hit.error = hit.normal = v3s(0.0f);
		hit.err_dot = 0.0f;
		hit.uvx = hit.uvy = 0.0f;
		hit.has_uv = hit.out = false;
	}
	// the tail of START: `ray` and `rng` are the sample's
	__device__ __forceinline__ void start()
	{
		thr = v3s(1.0f);
		outp = v3s(0.0f);
		depth = 0u;
		primary = true;
		ph = PH_CLOSEST;
	}
	// FINISH: the sample's value  integrators/mod.rs:74-76, mis.rs:88-90
	__device__ __forceinline__ V3 sample_value() const
	{
		V3 c = outp;
		if (ph == PH_FINISH && (contains_nan(c) || !is_finite_any(c)))
			c = v3s(0.0f);
		return c;
	}
};

// One walk for the wave: m_closest / m_shadow are the ballots of the lanes waiting in CLOSEST / SHADOW (not both empty, or the
// call does nothing).  Args is the kernel's one argument {DevScene S; P with max_depth, rr_threshold}; count_ray() is called where
// SamplerProgress.rays_shot counts as rt_render.hip does -- naive: one per walk of a path ray (do_shade), MIS: one per sample_lights
// call (do_light, mis.rs:38).
template <int METHOD, bool PRUNE, uint32_t QUORUM, class F, class Args, class Count>
__device__ __forceinline__ void path_lane_walk(PathLane &L, const Args &args_by_value, const WaveStack &W, uint64_t m_closest, uint64_t m_shadow,
                                               Count count_ray)
{
	const DevScene &S = args_by_value.S;
	if (METHOD == 0 || m_shadow == 0ull || (uint32_t)__popcll(m_closest) >= QUORUM) { // (wave-uniform)
		// ---- CLOSEST: the walk of a path ray and the shading of what it reached ----
		if (L.ph == PH_CLOSEST) {
			float best_t;
			uint32_t prim;
			trace_closest<F, PRUNE>(S, S, W.SM, L.ray, W.stk, best_t, prim);
			Hit nh;
			uint32_t nmat;
			if (prim != kNoPrim)
				make_hit<F>(S, prim, L.ray, best_t, nh, nmat);
			else
				make_sky_hit(S, nh, nmat);
			bool finish = false, filter = true;
			if (METHOD == 0) {
				// ---- NaiveIntegrator::get_colour loop body  integrators/mod.rs:31-72 ----
				count_ray();
				const V3 wo_n = L.ray.d;
				const V3 emission = mat_get_emission<F>(S, nmat, nh, wo_n);
				const bool exit = mat_scatter_ray<F>(S, nmat, L.ray, nh, L.rng);
				if (L.depth == 0u) {
					L.outp = L.outp + emission;
					if (exit)
						finish = true;
				}
				if (!finish && exit) {
					L.outp = L.outp + L.thr * emission;
					finish = true;
				}
				if (!finish) {
					if (!mat_is_delta<F>(S, nmat))
						L.thr = L.thr * mat_eval_over_pdf<F>(S, nmat, nh, wo_n, L.ray.d);
					else
						L.thr = L.thr * mat_eval<F>(S, nmat, nh, wo_n, L.ray.d);
					const KArgPtr<Args> ka = aov_kargs(args_by_value);
					if (L.depth > ka->P.rr_threshold) {
						const float p = component_max(L.thr);
						if (rt_rng_f32(&L.rng) > p)
							finish = true;
						else
							L.thr = L.thr / p;
					}
					if (!finish) {
						L.depth += 1u;
						if (!(L.depth < ka->P.max_depth))
							finish = true;
					}
				}
				// (the path continues: `ray` already is the scattered ray, ph stays CLOSEST)
			} else if (L.primary) {
				// ---- MisIntegrator::get_colour prologue  mis.rs:17-33 ----
				L.wo = L.ray.d;
				L.hit = nh;
				L.mat = nmat;
				const V3 emission = mat_get_emission<F>(S, L.mat, L.hit, L.wo);
				Ray clone = L.ray; // scatter on a clone: the draws are consumed, the ray is discarded (mis.rs:25)
				const bool exit = mat_scatter_ray<F>(S, L.mat, clone, L.hit, L.rng);
				L.outp = L.outp + emission;
				if (exit) {
					finish = true;
					filter = false; // mis.rs:29-31 returns before the filter
				} else {
					L.depth = 1u;
					L.primary = false;
					if (!(L.depth < aov_kargs(args_by_value)->P.max_depth))
						finish = true;
				}
			} else {
				// ---- material-sampling half of the MIS loop  mis.rs:50-86 ----
				const V3 m_wi = L.ray.d;
				const float m_pdf = mat_scattering_pdf<F>(S, L.mat, L.hit, L.wo, m_wi);
				const V3 le = mat_get_emission<F>(S, nmat, L.hit /* the OLD hit, mis.rs:55 */, m_wi);
				L.thr = L.thr * mat_eval_over_pdf<F>(S, L.mat, L.hit, L.wo, m_wi);
				if (!is_zero(le)) {
					if ((prim_in_light_list(S, prim, nmat) && !mat_is_delta<F>(S, L.mat)) || (prim == kNoPrim && sky_can_sample(S))) {
						const KArgPtr<Args> ka = aov_kargs(args_by_value);
						const SkyTables T = sky_tables(S, reinterpret_cast<KWords>(&ka->S.sky.inv_res_ok));
						const float l_pdf = pdf_from_index<F>(S, T, L.hit, nh, m_wi, prim);
						const float mis_weight = power_heuristic(m_pdf, l_pdf);
						L.outp = L.outp + L.thr * le * mis_weight;
					} else {
						L.outp = L.outp + L.thr * le;
					}
				}
				if (mat_is_light(S, nmat)) {
					finish = true;
				} else {
					const KArgPtr<Args> ka = aov_kargs(args_by_value);
					if (L.depth > ka->P.rr_threshold) {
						const float p = component_max(L.thr);
						if (rt_rng_f32(&L.rng) > p)
							finish = true;
						else
							L.thr = L.thr / p;
					}
					if (!finish) {
						L.wo = m_wi;
						L.hit = nh;
						L.mat = nmat;
						L.depth += 1u;
						if (!(L.depth < ka->P.max_depth))
							finish = true;
					}
				}
			}
			if (finish) {
				L.ph = filter ? PH_FINISH : PH_FINISH_UNFILTERED;
			} else if (METHOD == 1) {
				// ---- sample_lights up to the shadow ray  mis.rs:95-157 ----
				count_ray();
				L.have_shadow = false;
				L.skip = kNoPrim;
				const uint32_t samplable_len = S.n_lights;
				const bool sky_samplable = sky_can_sample(S);
				bool pick_sky = false, pick_light = false;
				uint32_t light_slot = 0u;
				if (samplable_len == 0u) {
					pick_sky = sky_samplable; // (0, true) => sample_sky(1.0); (0, false) => None
				} else if (!sky_samplable) {
					light_slot = rt_rng_below(&L.rng, samplable_len); // gen_range(0..len)
					pick_light = true;
				} else {
					light_slot = rt_rng_below(&L.rng, samplable_len + 1u); // gen_range(0..=len)
					if (light_slot == samplable_len)
						pick_sky = true;
					else
						pick_light = true;
				}
				PrimGeom g;
				g.type = g.material = 0u;
				g.p0 = g.p1 = g.p2 = v3s(0.0f);
				if (pick_sky) {
					const KArgPtr<Args> ka = aov_kargs(args_by_value);
					const SkyTables T = sky_tables(S, reinterpret_cast<KWords>(&ka->S.sky.inv_res_ok));
					L.l_wi = sky_sample(S, T, L.rng);
					L.t_limit = __uint_as_float(0x7FC00000u); // NaN: any t > 0 occludes
					L.have_shadow = true;
				} else if (pick_light) {
					L.skip = S.lights[light_slot];
					g = load_prim<F>(S, L.skip);
					L.l_wi = prim_sample_visible_from_point<F>(g, L.hit.point, L.rng);
				}
				if (pick_sky || pick_light)
					L.ray = ray_new<F>(L.hit.point + 0.0001f * L.hit.normal, L.l_wi);
				if (pick_light) {
					float lt;
					if (prim_t<F>(g, L.ray, lt) && lt > 0.0f) { // Bvh::check_hit_index  mod.rs:231-242
						L.t_limit = lt;
						L.have_shadow = true;
					}
				}
				L.ph = PH_SHADOW;
			}
		}
	} else if (METHOD == 1) {
		// ---- SHADOW: the shadow walk, the light's contribution (mis.rs:39-43) and material sampling (mis.rs:46-49) ----
		if (L.ph == PH_SHADOW) {
			if (L.have_shadow && !trace_any<F, PRUNE>(S, S, W.SM, L.ray, W.stk, L.t_limit, L.skip)) {
				const bool is_sky = L.t_limit != L.t_limit;
				const uint32_t n_l = S.n_lights;
				// sample_lights' pdf_multiplier: 1 when the sky is all there is to choose
				const float pdf_multiplier = n_l == 0u ? 1.0f : 1.0f / (float)light_choices(S);
				bool valid = false;
				V3 le = v3s(0.0f);
				float l_pdf = 0.0f;
				if (is_sky) { // sample_sky  mis.rs:104-115
					const KArgPtr<Args> ka = aov_kargs(args_by_value);
					const SkyTables T = sky_tables(S, reinterpret_cast<KWords>(&ka->S.sky.inv_res_ok));
					le = mat_get_emission<F>(S, S.sky.material, L.hit, L.l_wi);
					l_pdf = sky_pdf(S, T, L.l_wi) * pdf_multiplier;
					valid = true;
				} else { // sample_light  mis.rs:117-133 (`ray` still is the shadow ray)
					Hit lh;
					uint32_t lm;
					make_hit<F>(S, L.skip, L.ray, L.t_limit, lh, lm);
					const PrimGeom g = load_prim<F>(S, L.skip);
					const float p = prim_scattering_pdf<F>(g, L.hit.point, L.l_wi, lh);
					if (p > 0.0f) {
						le = mat_get_emission<F>(S, lm, lh, L.l_wi);
						l_pdf = p * pdf_multiplier;
						valid = true;
					}
				}
				if (valid) { // mis.rs:39-43
					const float m_pdf = mat_scattering_pdf<F>(S, L.mat, L.hit, L.wo, L.l_wi);
					const float mis_weight = power_heuristic(l_pdf, m_pdf);
					L.outp = L.outp + L.thr * mat_eval<F>(S, L.mat, L.hit, L.wo, L.l_wi) * mis_weight * le / l_pdf;
				}
			}
			// scatter_ray reads only the incoming direction of the ray that produced `hit`, which is `wo` (mis.rs:21,82)
			L.ray.d = L.wo;
			if (mat_scatter_ray<F>(S, L.mat, L.ray, L.hit, L.rng))
				L.ph = PH_FINISH;
			else
				L.ph = PH_CLOSEST;
		}
	}
}

// `groups` 256-thread workgroups of fn with lds_bytes of dynamic LDS (deep trees: more than the default 64 KB per workgroup)
template <class Args> hipError_t launch_path_lanes(void (*fn)(const Args), uint32_t groups, size_t lds_bytes, hipStream_t stream, const Args &A)
{
	const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
	if (e != hipSuccess)
		return e;
	hipLaunchKernelGGL(fn, dim3(groups), dim3(256), lds_bytes, stream, A);
	return hipGetLastError();
}

} // namespace rt
