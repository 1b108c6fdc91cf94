// rt_aov.hip -- first-hit auxiliary buffers (rt_render_aov, include/rt_hip.h): albedo, normal, depth, coverage and the
// primitive / material IDs of the primary hit, over the SAME camera rays the render traces.
//
// One wave per 8 x 8 tile, one lane per pixel, each lane loops over the passes: adjacent lanes walk coherent primary rays (one
// walk and one texture read per pass, no bounces), the sums stay in registers and every requested channel is stored once per
// pixel.  Everything computed here is what the render kernels compute for the same ray (rt_render.hip GEN: stream seed, jitter,
// SimpleCamera::get_ray; rt_intersect.h trace_closest / make_hit / make_sky_hit; rt_shade.h texture colours), so the result is
// reproducible bit for bit from the checker's pieces (tests/aov_checker.py).
#include "rt_aov_common.h"

namespace rt {

struct AovArgs {
	DevScene S;
	DevAovParams P;
};

template <bool PRUNE>
__global__ __launch_bounds__(256, 4) void aov_kernel(const AovArgs args_by_value)
{
	using F = FeatFull; // every primitive, material and texture type compiled in (as the batch hit queries)
	extern __shared__ __align__(16) uint32_t lds[];
	const DevScene &S = args_by_value.S;
	const DevAovParams &P = args_by_value.P;
	AovLane L;
	if (!aov_lane(S, P, lds, L))
		return;
	const bool want_albedo = (P.mask & kAovAlbedo) != 0u; // (wave-uniform)

	AovSums sums;
#pragma unroll 1
	for (uint32_t p = 0; p < P.spp; ++p) {
		const KArgPtr<DevAovParams> k = &aov_kargs(args_by_value)->P;
		const Ray ray = aov_camera_ray<F>(k, L, p);
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
		V3 c = v3s(0.0f);
		if (want_albedo)
			c = material_texture_colour<F>(S, mat_record(S, mat), mat, ray.d, h.point);
		sums.terminal(k, S, want_albedo, p, hit, prim, mat, h, c, v3s(1.0f), 0.0f);
	}
	sums.store(&aov_kargs(args_by_value)->P, L.pixel);
}

hipError_t launch_aov(bool prune, hipStream_t stream, const DevScene &S, const DevAovParams &P)
{
	AovArgs A;
	A.S = S;
	A.P = P;
	return launch_aov_tiles<AovArgs>(aov_kernel<true>, aov_kernel<false>, prune, stream, P.n_tiles, A);
}

} // namespace rt
