// rt_radiance.hip -- radiance queries (rt_radiance, include/rt_hip.h): NaiveIntegrator / MisIntegrator::get_colour on rays the
// caller supplies, K samples a ray, on the stream (seed, stream_i, sample_begin + k) with NO draw ahead of the integrator.  The
// integrator is the per-lane state machine of rt_path_lane.h (its header describes the phases, the quorum and the hand-out), shared
// with tiles_kernel (rt_adaptive.hip); the CPU checker's fixed-ray integrator is its counterpart, bit for bit.  This file holds
// what a radiance query adds:
//   FINISH  the sample's value added to the ray's sum; the next sample of the ray (START) or the output and CLAIM
//   CLAIM   a slot of the hand-out is a ray of the batch
//   START   ray and stream of sample k: Ray::new, rt_rng_seed
// Carried across the walks besides the PathLane: the ray's index, the sample's, and the ray's sum.
#include "rt_path_lane.h"
#include "rt_radiance.h"

namespace rt {

struct RadianceArgs {
	DevScene S;
	DevRadianceParams P;
};

// lanes of the wave that must wait for a closest-hit walk before it runs while shadow rays are pending elsewhere
// 
#ifndef RT_RADIANCE_QUORUM
#define RT_RADIANCE_QUORUM 32
#endif
constexpr uint32_t kRadianceQuorum = RT_RADIANCE_QUORUM;

template <int METHOD, bool PRUNE>
__global__ __launch_bounds__(256, kRadianceWaves) void radiance_kernel(const RadianceArgs args_by_value)
{
	using F = FeatFull; // every primitive, material and texture type compiled in (as the batch queries and the AOV passes)
	extern __shared__ __align__(16) uint32_t lds[];
	const WaveStack W = wave_stack(args_by_value.S, lds);
	WaveBlocks blocks; // of 64 rays
	PathLane L;
	uint32_t id = 0u, k = 0u; // the ray, and the sample of it in flight
	V3 sum = v3s(0.0f);       // of the ray's samples so far, in order

#pragma unroll 1
	for (;;) {
		// ---- FINISH: the sample's value, then the output rule of rt_radiance ----
		if (L.ph >= PH_FINISH) {
			const V3 c = L.sample_value();
			sum.x += c.x;
			sum.y += c.y;
			sum.z += c.z;
			k += 1u;
			const KArgPtr<RadianceArgs> ka = aov_kargs(args_by_value);
			const uint32_t samples = ka->P.samples;
			if (k < samples) {
				L.ph = PH_START;
			} else {
				float *const o = ka->P.out + 3u * (size_t)id;
				const float n = (float)samples;
				o[0] = sum.x / n;
				o[1] = sum.y / n;
				o[2] = sum.z / n;
				L.ph = PH_CLAIM;
			}
		}
		// ---- CLAIM: the next ray of the wave's block ----
		const uint64_t need = __ballot(L.ph == PH_CLAIM);
		if (need != 0ull) { // (wave-uniform)
			const uint32_t n = aov_kargs(args_by_value)->P.n_rays;
			if (L.ph == PH_CLAIM) {
				id = blocks.claimed(need);
				if (id >= n) {
					L.ph = PH_DONE;
				} else {
					k = 0u;
					sum = v3s(0.0f);
					L.ph = PH_START;
				}
			}
			blocks.advance(need, n);
		}
		// ---- START: sample k of ray id.  No draw before the integrator: no jitter, no camera time ----
		if (L.ph == PH_START) {
			const KArgPtr<RadianceArgs> ka = aov_kargs(args_by_value);
			const float *const rp = ka->P.rays + 6u * (size_t)id;
			const uint64_t *const streams = ka->P.streams;
			const uint64_t stream = streams != nullptr ? streams[id] : (uint64_t)id;
			const uint64_t seed = ((uint64_t)ka->P.seed_hi << 32) | ka->P.seed_lo;
			const uint64_t sample_begin = ((uint64_t)ka->P.sample_begin_hi << 32) | ka->P.sample_begin_lo;
			rt_rng_seed(&L.rng, seed, stream, sample_begin + k);
			L.ray = ray_new<F>(v3(rp[0], rp[1], rp[2]), v3(rp[3], rp[4], rp[5]));
			L.start();
		}

		const uint64_t m_closest = __ballot(L.ph == PH_CLOSEST), m_shadow = __ballot(L.ph == PH_SHADOW);
		if ((m_closest | m_shadow) == 0ull)
			break; // every lane is DONE (FINISH, CLAIM and START were emptied above)
		path_lane_walk<METHOD, PRUNE, kRadianceQuorum, F>(L, args_by_value, W, m_closest, m_shadow, [] {});
	}
}

hipError_t launch_radiance(int method, bool prune, hipStream_t stream, const DevScene &S, const DevRadianceParams &P, uint32_t groups)
{
	RadianceArgs A;
	A.S = S;
	A.P = P;
	void (*const fn)(const RadianceArgs) = method == 0 ? (prune ? radiance_kernel<0, true> : radiance_kernel<0, false>)
	                                                   : (prune ? radiance_kernel<1, true> : radiance_kernel<1, false>);
	return launch_path_lanes(fn, groups, four_wave_stack_lds_bytes(S), stream, A);
}

} // namespace rt
