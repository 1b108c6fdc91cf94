// rt_aov_chain.hip -- specular-chain auxiliary buffers (rt_render_aov_chain, include/rt_hip.h): the channels of rt_render_aov taken
// at the first vertex of each camera path that is NOT a followed mirror or glass surface, with the texture colours of the followed
// surfaces multiplied into the albedo and their segment lengths added to the depth.  No random draw beyond the jitter: a Reflect
// continues without its fuzz term, a Refract takes the branch the reference takes with certainty or with the larger weight.
//
// The shape of aov_kernel (rt_aov.hip): one wave per 8 x 8 tile, one lane per pixel, the traversal stack in LDS, sums in registers,
// every requested channel stored once.  (pass, segment) is flattened into ONE loop around ONE walk: a lane whose chain has ended
// generates the camera ray of its next pass in the same iteration in which its neighbour follows a bounce ("refill in place", as
// the render kernels), so lanes do not wait for each other's chains and the walk is compiled in once.
#include "rt_aov_common.h"
#include "rt_aov_chain.h"

namespace rt {

struct AovChainArgs {
	DevScene S;
	DevAovChainParams P;
};

template <bool PRUNE>
__global__ __launch_bounds__(256, 4) void aov_chain_kernel(const AovChainArgs args_by_value)
{
	using F = FeatFull;
	extern __shared__ __align__(16) uint32_t lds[];
	const DevScene &S = args_by_value.S;
	const DevAovParams &P = args_by_value.P.A;
	AovLane L;
	if (!aov_lane(S, P, lds, L))
		return;
	const bool want_albedo = (P.mask & kAovAlbedo) != 0u; // (wave-uniform)

	AovSums sums;
	float b_sum = 0.0f;
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
			ray = aov_camera_ray<F>(&aov_kargs(args_by_value)->P.A, L, p); // the only random draws: the jitter
			T = v3s(1.0f);
			D = 0.0f;
			b = 0u;
		}
		float best_t;
		uint32_t prim;
		trace_closest<F, PRUNE>(S, S, L.SM, ray, L.stk, best_t, prim);
		const bool hit = prim != kNoPrim;
		Hit h;
		uint32_t mat;
		if (hit)
			make_hit<F>(S, prim, ray, best_t, h, mat);
		else
			make_sky_hit(S, h, mat);
		const DevMaterial &m = mat_record(S, mat);
		const int type = mat_handle_type(mat);
		const KArgPtr<AovChainArgs> k = aov_kargs(args_by_value);
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
		} else { // the terminal of pass p: the first-hit rule under the chain's throughput and length
			sums.terminal(&k->P.A, S, want_albedo, p, hit, prim, mat, h, c, T, D);
			b_sum += (float)b;
			p += 1u;
			fresh = true;
		}
	}

	const KArgPtr<AovChainArgs> k = aov_kargs(args_by_value);
	sums.store(&k->P.A, L.pixel);
	if (k->P.A.mask & kAovBounces)
		k->P.bounces[L.pixel] = b_sum / (float)k->P.A.spp;
}

hipError_t launch_aov_chain(bool prune, hipStream_t stream, const DevScene &S, const DevAovChainParams &P)
{
	AovChainArgs A;
	A.S = S;
	A.P = P;
	return launch_aov_tiles<AovChainArgs>(aov_chain_kernel<true>, aov_chain_kernel<false>, prune, stream, P.A.n_tiles, A);
}

} // namespace rt
