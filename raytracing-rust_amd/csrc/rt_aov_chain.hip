// rt_aov_chain.hip -- specular-chain auxiliary buffers (rt_render_aov_chain, include/rt_hip.h): the channels of rt_render_aov taken
// at the first vertex of each camera path that is NOT a followed mirror or glass surface, with the texture colours of the followed
// surfaces multiplied into the albedo and their segment lengths added to the depth.  No random draw beyond the jitter: a Reflect
// continues without its fuzz term, a Refract takes the branch the reference takes with certainty or with the larger weight.
//
// The shape of aov_kernel (rt_aov.hip): one wave per 8 x 8 tile, one lane per pixel, the traversal stack in LDS, sums in registers,
// every requested channel stored once.  (pass, segment) is flattened into ONE loop around ONE walk: a lane whose chain has ended
// generates the camera ray of its next pass in the same iteration in which its neighbour follows a bounce ("refill in place", as
// the render kernels), so lanes do not wait for each other's chains and the walk is compiled in once.
#include "rt_shade.h"
#include "rt_aov_chain.h"

namespace rt {

constexpr uint32_t kAovChainWaves = 4; // 256-thread workgroups: four tiles

struct AovChainArgs {
	DevScene S;
	DevAovChainParams P;
};
// as rt_aov.hip: what is needed once per pass or once per bounce is read through a pointer the optimiser cannot see through
#if defined(__HIP_DEVICE_COMPILE__)
typedef const __attribute__((address_space(4))) AovChainArgs *AovChainKArgs; // the kernarg segment is constant memory: s_load
#else
typedef const AovChainArgs *AovChainKArgs;
#endif

template <bool PRUNE>
__global__ __launch_bounds__(256, 4) void aov_chain_kernel(const AovChainArgs args_by_value)
{
	using F = FeatFull;
	extern __shared__ __align__(16) uint32_t lds[];
#if defined(__HIP_DEVICE_COMPILE__)
	const AovChainKArgs K = (AovChainKArgs)__builtin_amdgcn_kernarg_segment_ptr();
	auto kargs = [&]() -> AovChainKArgs {
		AovChainKArgs k = K;
		asm volatile("" : "+s"(k));
		return k;
	};
#else
	const AovChainKArgs K = &args_by_value;
	auto kargs = [&]() -> AovChainKArgs { return K; };
#endif
	const DevScene &S = args_by_value.S;
	const DevAovParams &P = args_by_value.P.A;
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	uint32_t *stk = lds + wave * (S.stack_depth * kStackStride) + lane;
	// the whole worst case in LDS: the overflow branch is never taken (as rt_aov.hip)
	const StackMem SM = {S.stack_depth, 0u, const_cast<uint32_t *>(P.prim_desc), lds};
	const uint32_t tile = blockIdx.x * kAovChainWaves + wave;
	if (tile >= P.n_tiles)
		return;
	const uint32_t px = (tile % P.tiles_x) * 8u + (lane & 7u), py = (tile / P.tiles_x) * 8u + (lane >> 3);
	if (px >= P.width || py >= P.height)
		return;
	const uint64_t pixel = (uint64_t)py * P.width + px;
	const bool want_albedo = (P.mask & kAovAlbedo) != 0u; // (wave-uniform)

	V3 albedo = v3s(0.0f), normal = v3s(0.0f);
	float t_sum = 0.0f, b_sum = 0.0f;
	uint32_t hits = 0, first_prim = 0xFFFFFFFFu, first_mat = 0xFFFFFFFFu;
	// the chain of the pass in flight: throughput T, length D, followed hits b
	V3 T = v3s(1.0f);
	float D = 0.0f;
	uint32_t b = 0, p = 0;
	bool fresh = true; // the next segment is the camera ray of pass p
	Ray ray;
#pragma unroll 1
	for (;;) {
		if (fresh) {
			if (p >= P.spp)
				break;
			// random_sampler.rs:50-61 as rt_aov.hip: the first two draws of (seed, pixel, pass) jitter the pixel -- the only draws
			const AovChainKArgs k = kargs();
			const uint64_t seed = ((uint64_t)k->P.A.seed_hi << 32) | k->P.A.seed_lo;
			const uint64_t sample_begin = ((uint64_t)k->P.A.sample_begin_hi << 32) | k->P.A.sample_begin_lo;
			const V3 cam_o = v3(k->P.A.cam.origin[0], k->P.A.cam.origin[1], k->P.A.cam.origin[2]);
			const V3 cam_ll = v3(k->P.A.cam.lower_left[0], k->P.A.cam.lower_left[1], k->P.A.cam.lower_left[2]);
			const V3 cam_h = v3(k->P.A.cam.horizontal[0], k->P.A.cam.horizontal[1], k->P.A.cam.horizontal[2]);
			const V3 cam_v = v3(k->P.A.cam.vertical[0], k->P.A.cam.vertical[1], k->P.A.cam.vertical[2]);
			rt_rng rng;
			rt_rng_seed(&rng, seed, pixel, sample_begin + p);
			const float jx = rt_rng_range_f32(&rng, 0.0f, 1.0f) + (float)px, jy = rt_rng_range_f32(&rng, 0.0f, 1.0f) + (float)py;
			const float u = jx / (float)(k->P.A.width - 1u);
			const float v = 1.0f - jy / (float)(k->P.A.height - 1u);
			ray = ray_new<F>(cam_o, cam_ll + cam_h * u + cam_v * v - cam_o); // SimpleCamera::get_ray  camera.rs:57-63
			T = v3s(1.0f);
			D = 0.0f;
			b = 0u;
		}
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
		const DevMaterial &m = mat_record(S, mat);
		const int type = mat_handle_type(mat);
		const AovChainKArgs k = kargs();
		// followed: glass always, a mirror whose fuzz is within the limit -- while the chain may still grow
		const bool followed = hit && b < k->P.max_chain && (type == 4 || (type == 3 && m.param <= k->P.fuzz_limit));
		V3 c = v3s(0.0f);
		if (want_albedo) // colour_value(wo, point) of the material's texture (as rt_aov.hip)
			c = material_texture_colour<F>(S, m, mat, ray.d, h.point);
		if (followed) {
			T = T * c;
			D = D + h.t;
			b += 1u;
			bool mirror = type == 3;
			float eta_fraction = 0.0f, cos_theta = 0.0f;
			if (!mirror) { // refract.rs:28-36
				const float eta = m.param;
				eta_fraction = 1.0f / eta;
				if (!h.out)
					eta_fraction = eta;
				cos_theta = fmin_(dot(-ray.d, h.normal), 1.0f);
				const float sin_theta = sqrtf(1.0f - cos_theta * cos_theta);
				mirror = eta_fraction * sin_theta > 1.0f; // cannot refract: the reflect branch; the Fresnel draw is not made
			}
			if (mirror) { // reflect.rs:27-31 with the fuzz term left out (not multiplied by zero)
				const V3 direction = reflected(-ray.d, h.normal);
				const V3 point = offset_ray(h.point, h.normal, h.err_dot, true);
				ray = ray_new<F>(point, direction);
			} else { // refract.rs:44-48
				const V3 perp = eta_fraction * (ray.d + cos_theta * h.normal);
				const V3 para = (-1.0f * sqrtf(fabsf(1.0f - mag_sq(perp)))) * h.normal;
				const V3 point = offset_ray(h.point, h.normal, h.err_dot, false);
				ray = ray_new<F>(point, perp + para);
			}
			fresh = false;
		} else { // the terminal of pass p: the first-hit rule of rt_aov.hip under the chain's throughput and length
			if (want_albedo) {
				if (hit && type == 1) // RT_MAT_LAMBERTIAN (lambertian.rs:47-49)
					c = c * m.param;
				albedo = albedo + T * c;
			}
			if (hit) {
				normal = normal + h.normal;
				t_sum += D + h.t;
				hits += 1u;
			}
			b_sum += (float)b;
			if (p == 0u && hit) {
				const uint32_t *prim_desc = k->P.A.prim_desc;
				first_prim = prim_desc != nullptr ? prim_desc[prim] : prim;
				first_mat = mat_handle_index(mat); // the caller's index, not the handle
			}
			p += 1u;
			fresh = true;
		}
	}

	const AovChainKArgs k = kargs();
	const uint32_t mask = k->P.A.mask;
	const float n = (float)k->P.A.spp;
	if (mask & kAovAlbedo) {
		float *const o = k->P.A.albedo;
		o[3u * pixel + 0u] = albedo.x / n;
		o[3u * pixel + 1u] = albedo.y / n;
		o[3u * pixel + 2u] = albedo.z / n;
	}
	if (mask & kAovNormal) {
		float *const o = k->P.A.normal;
		o[3u * pixel + 0u] = normal.x / n;
		o[3u * pixel + 1u] = normal.y / n;
		o[3u * pixel + 2u] = normal.z / n;
	}
	if (mask & kAovDepth)
		k->P.A.depth[pixel] = hits != 0u ? t_sum / (float)hits : 0.0f;
	if (mask & kAovCoverage)
		k->P.A.coverage[pixel] = (float)hits / n;
	if (mask & kAovPrimitive)
		k->P.A.primitive[pixel] = first_prim;
	if (mask & kAovMaterial)
		k->P.A.material[pixel] = first_mat;
	if (mask & kAovBounces)
		k->P.bounces[pixel] = b_sum / n;
}

size_t aov_chain_lds_bytes(const DevScene &S) { return (size_t)kAovChainWaves * S.stack_depth * kStackStride * sizeof(uint32_t); }

hipError_t launch_aov_chain(bool prune, hipStream_t stream, const DevScene &S, const DevAovChainParams &P)
{
	const size_t lds_bytes = aov_chain_lds_bytes(S);
	const uint32_t blocks = (P.A.n_tiles + kAovChainWaves - 1u) / kAovChainWaves;
	const void *fn = prune ? reinterpret_cast<const void *>(aov_chain_kernel<true>) : reinterpret_cast<const void *>(aov_chain_kernel<false>);
	hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
	if (e != hipSuccess)
		return e;
	AovChainArgs A;
	A.S = S;
	A.P = P;
	if (prune)
		hipLaunchKernelGGL(aov_chain_kernel<true>, dim3(blocks), dim3(256), lds_bytes, stream, A);
	else
		hipLaunchKernelGGL(aov_chain_kernel<false>, dim3(blocks), dim3(256), lds_bytes, stream, A);
	return hipGetLastError();
}

} // namespace rt
