// rt_ao.hip -- the ambient-occlusion pass (rt_render_ao, include/rt_hip.h): per pixel the share of short cosine-weighted rays from
// the first hit that reach nothing (visibility), and the mean of those rays' directions (the bent normal).  Pass s of a pixel is
// the camera ray of rt_render_aov, its closest hit, and K any-hit rays drawn on the same stream behind the jitter:
// lambertian_sample about Hit.normal from the origin a Lambertian scatter uses.  tests/ao_checker.py restates it in numpy.
//
// The shape of aov_chain_kernel (rt_aov_chain.hip): one wave per 8 x 8 tile, one lane per pixel, the traversal stack in LDS.  A
// pass is ONE closest-hit walk and then, on the lanes that hit, K any-hit walks; in lockstep the sky lanes would idle for K walks.
// So every lane is a small state machine -- `pending` AO rays left of the pass in flight, `p` passes started -- and the WAVE
// decides by ballot which of the two walks an iteration runs: the primary step (camera ray, trace_closest, make_hit; a lane that
// hits loads its K rays, a lane that misses is ready for its next pass at once) when no lane has an AO ray pending or when at
// least kAoPrimaryQuorum lanes wait for a camera ray, else the occlusion step (one sampled ray, trace_any) on the lanes that
// have one pending.  Each walk is compiled in once.  A lane works through its own passes and rays strictly in order and no value
// crosses lanes, so the schedule (the quorum, the shape of the tile) cannot change a bit of the result.
//
// Carried across a pass: the normal, the offset origin, the stream (4 words), p and pending; across the pixel: two counts and the
// bent sum.  No array is indexed dynamically.
#include "rt_aov_common.h"
#include "rt_ao.h"

namespace rt {

struct AoArgs {
	DevScene S;
	DevAoParams P;
};

namespace {

// lanes of the wave that must wait for a camera ray before the primary step runs while AO rays are pending elsewhere
// (what was tried)
#ifndef RT_AO_QUORUM
#define RT_AO_QUORUM 48
#endif
constexpr uint32_t kAoPrimaryQuorum = RT_AO_QUORUM;

} // namespace

template <bool PRUNE>
__global__ __launch_bounds__(256, 4) void ao_kernel(const AoArgs args_by_value)
{
	using F = FeatFull; // every primitive type compiled in (as the AOV passes)
	extern __shared__ __align__(16) uint32_t lds[];
	const DevScene &S = args_by_value.S;
	const DevAovParams &P = args_by_value.P.A;
	AovLane L;
	if (!aov_lane(S, P, lds, L))
		return;

	uint32_t n = 0, u = 0; // AO rays shot (hits * K), and those of them that reached nothing
	V3 bent = v3s(0.0f);   // the sum of the directions of the latter
	// the pass in flight
	V3 normal = v3s(0.0f), origin = v3s(0.0f);
	rt_rng rng = {0u, 0u, 0u, 0u};
	uint32_t p = 0, pending = 0; // passes started; AO rays the pass in flight has left
#pragma unroll 1
	for (;;) {
		const bool waits = pending == 0u && p < P.spp; // for the camera ray of pass p
		const uint64_t m_pending = __ballot(pending != 0u), m_waits = __ballot(waits);
		if ((m_pending | m_waits) == 0ull)
			break;
		if (m_pending == 0ull || (uint32_t)__popcll(m_waits) >= kAoPrimaryQuorum) { // (wave-uniform) the primary step
			if (waits) {
				const KArgPtr<AoArgs> k = aov_kargs(args_by_value);
				const Ray ray = aov_camera_ray<F>(&k->P.A, L, p);
				float best_t;
				uint32_t prim;
				trace_closest<F, PRUNE>(S, S, L.SM, ray, L.stk, best_t, prim);
				if (prim != kNoPrim) {
					Hit h;
					uint32_t mat;
					make_hit<F>(S, prim, ray, best_t, h, mat);
					normal = h.normal;
					origin = offset_ray(h.point, h.normal, h.err_dot, true); // the origin a Lambertian scatter uses
					// the AO rays continue the stream of the pass behind the two jitter draws
					const KArgPtr<AoArgs> ks = aov_kargs(args_by_value);
					const uint64_t seed = ((uint64_t)ks->P.A.seed_hi << 32) | ks->P.A.seed_lo;
					const uint64_t sample_begin = ((uint64_t)ks->P.A.sample_begin_hi << 32) | ks->P.A.sample_begin_lo;
					rt_rng_seed(&rng, seed, L.pixel, sample_begin + p);
					(void)rt_rng_u32(&rng);
					(void)rt_rng_u32(&rng);
					pending = ks->P.rays_per_pass;
					n += pending;
				}
				p += 1u;
			}
		} else { // the occlusion step: the next AO ray of every lane that has one
			if (pending != 0u) {
				const V3 d = lambertian_sample(normal, rng);
				const Ray ray = ray_new<F>(origin, d);
				const float t_limit = aov_kargs(args_by_value)->P.t_limit;
				if (!trace_any<F, PRUNE>(S, S, L.SM, ray, L.stk, t_limit, kNoPrim)) {
					u += 1u;
					bent = bent + d; // as sampled, not the ray's normalised direction
				}
				pending -= 1u;
			}
		}
	}

	const KArgPtr<AoArgs> k = aov_kargs(args_by_value);
	const float nf = (float)n;
	float *const visibility = k->P.visibility;
	if (visibility != nullptr)
		visibility[L.pixel] = n != 0u ? (float)u / nf : 1.0f;
	float *const bent_normal = k->P.bent_normal;
	if (bent_normal != nullptr) {
		bent_normal[3u * L.pixel + 0u] = n != 0u ? bent.x / nf : 0.0f;
		bent_normal[3u * L.pixel + 1u] = n != 0u ? bent.y / nf : 0.0f;
		bent_normal[3u * L.pixel + 2u] = n != 0u ? bent.z / nf : 0.0f;
	}
}

hipError_t launch_ao(bool prune, hipStream_t stream, const DevScene &S, const DevAoParams &P)
{
	AoArgs A;
	A.S = S;
	A.P = P;
	return launch_aov_tiles<AoArgs>(ao_kernel<true>, ao_kernel<false>, prune, stream, P.A.n_tiles, A);
}

} // namespace rt
