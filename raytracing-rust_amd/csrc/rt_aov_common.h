// rt_aov_common.h -- device code the two AOV kernels share (rt_aov.hip: the first hit; rt_aov_chain.hip: the first hit behind
// followed mirrors and glass), and their launcher.  They differ in the loop between the camera ray and the terminal hit only.
#pragma once
#include "rt_shade.h"
#include "rt_aov.h"

namespace rt {

// The camera, the seed, the sample window and the channel pointers are needed once per pass or once per pixel: read through a
// pointer the optimiser cannot see through (aov_kargs: the kernel's one argument, made opaque anew at every call), they are loaded
// where they are used instead of living in SGPRs (and spilling from there) across the walk (as rt_render.hip's kargs()).
#if defined(__HIP_DEVICE_COMPILE__)
template <class T> using KArgPtr = const __attribute__((address_space(4))) T *; // the kernarg segment is constant memory: s_load
#else
template <class T> using KArgPtr = const T *;
#endif
template <class Args> __device__ __forceinline__ KArgPtr<Args> aov_kargs(const Args &args_by_value)
{
#if defined(__HIP_DEVICE_COMPILE__)
	KArgPtr<Args> k = (KArgPtr<Args>)__builtin_amdgcn_kernarg_segment_ptr();
	asm volatile("" : "+s"(k));
	return k;
#else
	return &args_by_value;
#endif
}

// wave -> tile, lane -> pixel, and the lane's stack column.  The whole worst case is in LDS: the overflow branch is never taken
// (its base only has to be some global pointer, see rt_query.hip check_hit_kernel).
struct AovLane {
	uint32_t px, py;
	uint64_t pixel;
	uint32_t *stk;
	StackMem SM;
};
// false: this lane has no pixel (a tile past the frame, or the padding of an edge tile)
__device__ __forceinline__ bool aov_lane(const DevScene &S, const DevAovParams &P, uint32_t *lds, AovLane &L)
{
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	L.stk = lds + wave * (S.stack_depth * kStackStride) + lane;
	L.SM = {S.stack_depth, 0u, const_cast<uint32_t *>(P.prim_desc), lds};
	const uint32_t tile = blockIdx.x * kFourWaves + wave;
	if (tile >= P.n_tiles)
		return false;
	L.px = (tile % P.tiles_x) * 8u + (lane & 7u);
	L.py = (tile / P.tiles_x) * 8u + (lane >> 3);
	if (L.px >= P.width || L.py >= P.height)
		return false;
	L.pixel = (uint64_t)L.py * P.width + L.px;
	return true;
}

// random_sampler.rs:50-61 as rt_render.hip do_gen: the first two draws of (seed, pixel, pass) jitter the pixel
template <class F> __device__ __forceinline__ Ray aov_camera_ray(KArgPtr<DevAovParams> k, const AovLane &L, uint32_t pass)
{
	const uint64_t seed = ((uint64_t)k->seed_hi << 32) | k->seed_lo;
	const uint64_t sample_begin = ((uint64_t)k->sample_begin_hi << 32) | k->sample_begin_lo;
	const V3 cam_o = v3(k->cam.origin[0], k->cam.origin[1], k->cam.origin[2]);
	const V3 cam_ll = v3(k->cam.lower_left[0], k->cam.lower_left[1], k->cam.lower_left[2]);
	const V3 cam_h = v3(k->cam.horizontal[0], k->cam.horizontal[1], k->cam.horizontal[2]);
	const V3 cam_v = v3(k->cam.vertical[0], k->cam.vertical[1], k->cam.vertical[2]);
	rt_rng rng;
	rt_rng_seed(&rng, seed, L.pixel, sample_begin + pass);
	const float jx = rt_rng_range_f32(&rng, 0.0f, 1.0f) + (float)L.px, jy = rt_rng_range_f32(&rng, 0.0f, 1.0f) + (float)L.py;
	const float u = jx / (float)(k->width - 1u);
	const float v = 1.0f - jy / (float)(k->height - 1u);
	return ray_new<F>(cam_o, cam_ll + cam_h * u + cam_v * v - cam_o); // SimpleCamera::get_ray  camera.rs:57-63
}

// the sums of one pixel over its passes
struct AovSums {
	V3 albedo = v3s(0.0f), normal = v3s(0.0f);
	float t_sum = 0.0f;
	uint32_t hits = 0, first_prim = 0xFFFFFFFFu, first_mat = 0xFFFFFFFFu;

	// The terminal vertex of pass `pass`, reached under throughput T after a path of length D.  The first hit itself is T = 1, D = 0,
	// and gives the bits of the sums without them: 1 * c is c for every c, finite or not, and 0 + t could differ from t only in the
	// sign of a zero, which a hit distance (t > 0) is not.  `c` is the texture colour at the vertex, colour_value(wo, point) (read
	// only when the albedo is wanted); a Lambertian scales it by its albedo (lambertian.rs:47-49, as rt_shade.h mat_eval_over_pdf),
	// the sky contributes it alone.  (The material record is looked up HERE: handed in it costs aov_kernel<false> a register.)
	__device__ __forceinline__ void terminal(KArgPtr<DevAovParams> k, const DevScene &S, bool want_albedo, uint32_t pass, bool hit, uint32_t prim,
	                                         uint32_t mat, const Hit &h, V3 c, V3 T, float D)
	{
		if (want_albedo) {
			if (hit && mat_handle_type(mat) == 1) // RT_MAT_LAMBERTIAN
				c = c * mat_record(S, mat).param;
			albedo = albedo + T * c;
		}
		if (hit) {
			normal = normal + h.normal;
			t_sum += D + h.t;
			hits += 1u;
		}
		if (pass == 0u && hit) {
			const uint32_t *prim_desc = k->prim_desc;
			first_prim = prim_desc != nullptr ? prim_desc[prim] : prim;
			first_mat = mat_handle_index(mat); // the caller's index, not the handle
		}
	}

	// (the channel pointers, like the camera, come through the opaque pointer: one round of scalar loads here)
	__device__ __forceinline__ void store(KArgPtr<DevAovParams> k, uint64_t pixel) const
	{
		const uint32_t mask = k->mask;
		const float n = (float)k->spp;
		if (mask & kAovAlbedo) {
			float *const o = k->albedo;
			o[3u * pixel + 0u] = albedo.x / n;
			o[3u * pixel + 1u] = albedo.y / n;
			o[3u * pixel + 2u] = albedo.z / n;
		}
		if (mask & kAovNormal) {
			float *const o = k->normal;
			o[3u * pixel + 0u] = normal.x / n;
			o[3u * pixel + 1u] = normal.y / n;
			o[3u * pixel + 2u] = normal.z / n;
		}
		if (mask & kAovDepth)
			k->depth[pixel] = hits != 0u ? t_sum / (float)hits : 0.0f;
		if (mask & kAovCoverage)
			k->coverage[pixel] = (float)hits / n;
		if (mask & kAovPrimitive)
			k->primitive[pixel] = first_prim;
		if (mask & kAovMaterial)
			k->material[pixel] = first_mat;
	}
};

// 256-thread workgroups: one wave per tile (kFourWaves, rt_types.h), four_wave_stack_lds_bytes of dynamic LDS (deep trees: more than the default 64 KB per workgroup)
template <class Args> hipError_t launch_aov_tiles(void (*pruned)(const Args), void (*exhaustive)(const Args), bool prune, hipStream_t stream, uint32_t n_tiles, const Args &A)
{
	void (*const fn)(const Args) = prune ? pruned : exhaustive;
	const size_t lds_bytes = four_wave_stack_lds_bytes(A.S);
	const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
	if (e != hipSuccess)
		return e;
	hipLaunchKernelGGL(fn, dim3((n_tiles + kFourWaves - 1u) / kFourWaves), dim3(256), lds_bytes, stream, A);
	return hipGetLastError();
}

} // namespace rt
