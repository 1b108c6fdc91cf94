// rt_aov.hip -- first-hit auxiliary buffers (rt_render_aov, include/rt_hip.h): albedo, normal, depth, coverage and the
// primitive / material IDs of the primary hit, over the SAME camera rays the render traces.
//
// One wave per 8 x 8 tile, one lane per pixel, each lane loops over the passes: adjacent lanes walk coherent primary rays (one
// walk and one texture read per pass, no bounces), the sums stay in registers and every requested channel is stored once per
// pixel.  Everything computed here is what the render kernels compute for the same ray (rt_render.hip GEN: stream seed, jitter,
// SimpleCamera::get_ray; rt_intersect.h trace_closest / make_hit / make_sky_hit; rt_shade.h texture colours), so the result is
// reproducible bit for bit from the checker's pieces (tests/aov_checker.py).
#include "rt_shade.h"
#include "rt_aov.h"

namespace rt {

constexpr uint32_t kAovWaves = 4; // 256-thread workgroups: four tiles

struct AovArgs {
	DevScene S;
	DevAovParams P;
};
// The camera, the seed and the sample window are needed once per pass: read through a pointer the optimiser cannot see through,
// they are loaded where they are used instead of living in SGPRs (and spilling from there) across the walk (as rt_render.hip's
// kargs()).
#if defined(__HIP_DEVICE_COMPILE__)
typedef const __attribute__((address_space(4))) AovArgs *AovKArgs; // the kernarg segment is constant memory: s_load
#else
typedef const AovArgs *AovKArgs;
#endif

template <bool PRUNE>
__global__ __launch_bounds__(256, 4) void aov_kernel(const AovArgs args_by_value)
{
	using F = FeatFull; // every primitive, material and texture type compiled in (as the batch hit queries)
	extern __shared__ __align__(16) uint32_t lds[];
#if defined(__HIP_DEVICE_COMPILE__)
	const AovKArgs K = (AovKArgs)__builtin_amdgcn_kernarg_segment_ptr();
	auto kargs = [&]() -> AovKArgs {
		AovKArgs k = K;
		asm volatile("" : "+s"(k));
		return k;
	};
#else
	const AovKArgs K = &args_by_value;
	auto kargs = [&]() -> AovKArgs { return K; };
#endif
	const DevScene &S = args_by_value.S;
	const DevAovParams &P = args_by_value.P;
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	uint32_t *stk = lds + wave * (S.stack_depth * kStackStride) + lane;
	// the whole worst case in LDS: the overflow branch is never taken (its base only has to be some global pointer, see
	// rt_render.hip check_hit_kernel)
	const StackMem SM = {S.stack_depth, 0u, const_cast<uint32_t *>(P.prim_desc), lds};
	const uint32_t tile = blockIdx.x * kAovWaves + wave;
	if (tile >= P.n_tiles)
		return;
	const uint32_t px = (tile % P.tiles_x) * 8u + (lane & 7u), py = (tile / P.tiles_x) * 8u + (lane >> 3);
	if (px >= P.width || py >= P.height)
		return;
	const uint64_t pixel = (uint64_t)py * P.width + px;
	const bool want_albedo = (P.mask & kAovAlbedo) != 0u; // (wave-uniform)

	V3 albedo = v3s(0.0f), normal = v3s(0.0f);
	float t_sum = 0.0f;
	uint32_t hits = 0, first_prim = 0xFFFFFFFFu, first_mat = 0xFFFFFFFFu;
#pragma unroll 1
	for (uint32_t p = 0; p < P.spp; ++p) {
		// random_sampler.rs:50-61 as rt_render.hip do_gen: the first two draws of (seed, pixel, pass) jitter the pixel
		const AovKArgs k = kargs();
		const uint64_t seed = ((uint64_t)k->P.seed_hi << 32) | k->P.seed_lo;
		const uint64_t sample_begin = ((uint64_t)k->P.sample_begin_hi << 32) | k->P.sample_begin_lo;
		const V3 cam_o = v3(k->P.cam.origin[0], k->P.cam.origin[1], k->P.cam.origin[2]);
		const V3 cam_ll = v3(k->P.cam.lower_left[0], k->P.cam.lower_left[1], k->P.cam.lower_left[2]);
		const V3 cam_h = v3(k->P.cam.horizontal[0], k->P.cam.horizontal[1], k->P.cam.horizontal[2]);
		const V3 cam_v = v3(k->P.cam.vertical[0], k->P.cam.vertical[1], k->P.cam.vertical[2]);
		rt_rng rng;
		rt_rng_seed(&rng, seed, pixel, sample_begin + p);
		const float jx = rt_rng_range_f32(&rng, 0.0f, 1.0f) + (float)px, jy = rt_rng_range_f32(&rng, 0.0f, 1.0f) + (float)py;
		const float u = jx / (float)(k->P.width - 1u);
		const float v = 1.0f - jy / (float)(k->P.height - 1u);
		const Ray ray = ray_new<F>(cam_o, cam_ll + cam_h * u + cam_v * v - cam_o); // SimpleCamera::get_ray  camera.rs:57-63
		float best_t;
		uint32_t prim;
		trace_closest<F, PRUNE>(S, S, SM, ray, stk, best_t, prim);
		const bool hit = prim != kNoPrim;
		Hit h;
		uint32_t mat;
		if (hit)
			make_hit<F>(S, prim, ray, best_t, h, mat);
		else
			make_sky_hit(S, h, mat);
		if (want_albedo) {
			// colour_value(wo, point) of the material's texture; a Lambertian scales it by its albedo (lambertian.rs:47-49, as
			// rt_shade.h mat_eval_over_pdf); the sky contributes its texture colour alone
			const DevMaterial &m = mat_record(S, mat);
			V3 c = material_texture_colour<F>(S, m, mat, ray.d, h.point);
			if (hit && mat_handle_type(mat) == 1) // RT_MAT_LAMBERTIAN
				c = c * m.param;
			albedo = albedo + c;
		}
		if (hit) {
			normal = normal + h.normal;
			t_sum += h.t;
			hits += 1u;
		}
		if (p == 0u && hit) {
			const uint32_t *prim_desc = k->P.prim_desc;
			first_prim = prim_desc != nullptr ? prim_desc[prim] : prim;
			first_mat = mat_handle_index(mat); // the caller's index, not the handle
		}
	}

	// (the channel pointers, like the camera, come through kargs(): one round of scalar loads here)
	const AovKArgs k = kargs();
	const uint32_t mask = k->P.mask;
	const float n = (float)k->P.spp;
	if (mask & kAovAlbedo) {
		float *const o = k->P.albedo;
		o[3u * pixel + 0u] = albedo.x / n;
		o[3u * pixel + 1u] = albedo.y / n;
		o[3u * pixel + 2u] = albedo.z / n;
	}
	if (mask & kAovNormal) {
		float *const o = k->P.normal;
		o[3u * pixel + 0u] = normal.x / n;
		o[3u * pixel + 1u] = normal.y / n;
		o[3u * pixel + 2u] = normal.z / n;
	}
	if (mask & kAovDepth)
		k->P.depth[pixel] = hits != 0u ? t_sum / (float)hits : 0.0f;
	if (mask & kAovCoverage)
		k->P.coverage[pixel] = (float)hits / n;
	if (mask & kAovPrimitive)
		k->P.primitive[pixel] = first_prim;
	if (mask & kAovMaterial)
		k->P.material[pixel] = first_mat;
}

size_t aov_lds_bytes(const DevScene &S) { return (size_t)kAovWaves * S.stack_depth * kStackStride * sizeof(uint32_t); }

hipError_t launch_aov(bool prune, hipStream_t stream, const DevScene &S, const DevAovParams &P)
{
	const size_t lds_bytes = aov_lds_bytes(S);
	const uint32_t blocks = (P.n_tiles + kAovWaves - 1u) / kAovWaves;
	const void *fn = prune ? reinterpret_cast<const void *>(aov_kernel<true>) : reinterpret_cast<const void *>(aov_kernel<false>);
	hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
	if (e != hipSuccess)
		return e;
	AovArgs A;
	A.S = S;
	A.P = P;
	if (prune)
		hipLaunchKernelGGL(aov_kernel<true>, dim3(blocks), dim3(256), lds_bytes, stream, A);
	else
		hipLaunchKernelGGL(aov_kernel<false>, dim3(blocks), dim3(256), lds_bytes, stream, A);
	return hipGetLastError();
}

} // namespace rt
