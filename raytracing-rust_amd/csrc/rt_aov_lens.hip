// rt_aov_lens.hip -- the auxiliary buffers of rt_render_aov_chain through a camera MODEL (rt_render_lens_aov, include/rt_hip.h): segment
// 0 of every pass is the ray rt_render_lens makes for that sample, on the same camera stream (seed, 2^63 + pixel, sample_begin +
// pass) and with the same draws in the same order, so the guides see the sub-pixel positions and lens points the frame's paths start
// from.  From there on the chain, the terminal and the folds are rt_aov_chain.hip's; max_chain = 0 is the first-hit pass.
//
// aov_lens_guide_kernel is aov_chain_kernel (rt_aov_chain.hip) with another `fresh` arm: one wave per 8 x 8 tile, one lane per
// pixel, the four waves' stacks in dynamic LDS, (pass, segment) flattened into ONE loop around ONE walk.  The projection is a
// WAVE-UNIFORM switch on a launch constant, each arm straight-line code (rt_lens.hip START, restated: rt_hip.h states every
// expression); the camera's vectors are read from the kernel arguments where an arm uses them (aov_kargs) and held nowhere else.
// A fisheye sample outside the image circle is skipped: it advances the pass counter, adds no term to any sum, and the lane
// stays `fresh` through the walk of its wave (which does nothing for it), so a lane whose remaining passes are all black leaves
// the loop after one trip a pass without ever walking.
#include "rt_aov_common.h"
#include "rt_aov_lens.h"

namespace rt {

struct AovLensArgs {
	DevScene S;
	DevAovLensParams P;
};

// three floats of the kernel arguments as a vector, loaded where they are used
#define RT_AOV_LENS_V3(field) v3(ka->P.field[0], ka->P.field[1], ka->P.field[2])

// The ray of pass `pass` of the lane's pixel (all of it f32, in the written order); false: the sample is black and `ray` is not
// to be used.  The only random draws of the pass: the jitter and, for a lens, the lens point.
template <class F> __device__ __forceinline__ bool aov_lens_ray(KArgPtr<AovLensArgs> ka, const AovLane &L, uint32_t pass, Ray &ray)
{
	const uint64_t seed = ((uint64_t)ka->P.C.A.seed_hi << 32) | ka->P.C.A.seed_lo;
	const uint64_t sample_begin = ((uint64_t)ka->P.C.A.sample_begin_hi << 32) | ka->P.C.A.sample_begin_lo;
	const uint32_t width = ka->P.C.A.width, height = ka->P.C.A.height;
	const int32_t projection = ka->P.projection;
	rt_rng cam; // the camera stream: no pixel's path stream (pixels are below 2^31)
	rt_rng_seed(&cam, seed, 0x8000000000000000ull + L.pixel, sample_begin + pass);
	const float jx = rt_rng_range_f32(&cam, 0.0f, 1.0f) + (float)L.px, jy = rt_rng_range_f32(&cam, 0.0f, 1.0f) + (float)L.py;
	const float s = jx / (float)(width - 1u);
	const float t = 1.0f - jy / (float)(height - 1u);
	V3 o, d;
	if (projection == kProjPerspective) { // (wave-uniform, as every arm below)
		const float lens_radius = ka->P.lens_radius;
		o = RT_AOV_LENS_V3(C.A.cam.origin);
		d = RT_AOV_LENS_V3(C.A.cam.lower_left) + RT_AOV_LENS_V3(C.A.cam.horizontal) * s + RT_AOV_LENS_V3(C.A.cam.vertical) * t - o; // get_ray  camera.rs:57-63
		if (lens_radius != 0.0f) {
			const float xi1 = rt_rng_f32(&cam), xi2 = rt_rng_f32(&cam);
			const float r = lens_radius * sqrtf(xi1);
			const float phi = RT_TAU * xi2;
			const V3 off = RT_AOV_LENS_V3(right) * (r * rt_cosf(phi)) + RT_AOV_LENS_V3(up) * (r * rt_sinf(phi));
			o = o + off;
			d = d - off;
		}
	} else if (projection == kProjOrthographic) {
		o = RT_AOV_LENS_V3(C.A.cam.lower_left) + RT_AOV_LENS_V3(C.A.cam.horizontal) * s + RT_AOV_LENS_V3(C.A.cam.vertical) * t;
		d = RT_AOV_LENS_V3(forward);
	} else if (projection == kProjFisheye) { // equidistant: the angle from the axis grows with the radius in the image circle
		const float a = 2.0f * s - 1.0f;
		const float b = (2.0f * t - 1.0f) * ((float)(height - 1u) / (float)(width - 1u));
		const float rho = sqrtf(a * a + b * b);
		if (!(rho <= 1.0f)) // outside the circle, or NaN
			return false;
		const float theta = rho * ka->P.fisheye_half_angle;
		const float sin_t = rt_sinf(theta);
		const V3 fwd = RT_AOV_LENS_V3(forward);
		o = RT_AOV_LENS_V3(C.A.cam.origin);
		d = RT_AOV_LENS_V3(right) * (sin_t * (a / rho)) + RT_AOV_LENS_V3(up) * (sin_t * (b / rho)) + fwd * rt_cosf(theta);
		if (rho == 0.0f)
			d = fwd;
	} else { // kProjEquirect
		const float lon = (2.0f * s - 1.0f) * RT_PI;
		const float lat = (2.0f * t - 1.0f) * RT_FRAC_PI_2;
		const float cos_lat = rt_cosf(lat);
		o = RT_AOV_LENS_V3(C.A.cam.origin);
		d = RT_AOV_LENS_V3(right) * (cos_lat * rt_sinf(lon)) + RT_AOV_LENS_V3(up) * rt_sinf(lat) + RT_AOV_LENS_V3(forward) * (cos_lat * rt_cosf(lon));
	}
	ray = ray_new<F>(o, d);
	return true;
}
#undef RT_AOV_LENS_V3

template <bool PRUNE>
__global__ __launch_bounds__(256, 4) void aov_lens_guide_kernel(const AovLensArgs args_by_value)
{
	using F = FeatFull;
	extern __shared__ __align__(16) uint32_t lds[];
	const DevScene &S = args_by_value.S;
	const DevAovParams &P = args_by_value.P.C.A;
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
		bool walk = true; // false: pass p was black -- the lane sits out this trip's walk and stays fresh
		if (fresh) {
			if (p >= P.spp)
				break;
			walk = aov_lens_ray<F>(aov_kargs(args_by_value), L, p, ray);
			T = v3s(1.0f);
			D = 0.0f;
			b = 0u;
			if (!walk)
				p += 1u; // counted toward no sum; the divisors stay spp
		}
		if (walk) { // (the body of aov_chain_kernel's loop from here on)
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
			const KArgPtr<AovLensArgs> k = aov_kargs(args_by_value);
			// followed: glass always, a mirror whose fuzz is within the limit -- while the chain may still grow
			const bool followed = hit && b < k->P.C.max_chain && (type == 4 || (type == 3 && m.param <= k->P.C.fuzz_limit));
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
				sums.terminal(&k->P.C.A, S, want_albedo, p, hit, prim, mat, h, c, T, D);
				b_sum += (float)b;
				p += 1u;
				fresh = true;
			}
		}
	}

	const KArgPtr<AovLensArgs> k = aov_kargs(args_by_value);
	sums.store(&k->P.C.A, L.pixel);
	if (k->P.C.A.mask & kAovBounces)
		k->P.C.bounces[L.pixel] = b_sum / (float)k->P.C.A.spp;
}

hipError_t launch_aov_lens(bool prune, hipStream_t stream, const DevScene &S, const DevAovLensParams &P)
{
	AovLensArgs A;
	A.S = S;
	A.P = P;
	return launch_aov_tiles<AovLensArgs>(aov_lens_guide_kernel<true>, aov_lens_guide_kernel<false>, prune, stream, P.C.A.n_tiles, A);
}

} // namespace rt
