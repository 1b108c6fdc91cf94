// rt_probe.hip -- light probes (rt_probe_sh, include/rt_hip.h): K radiance samples in uniformly drawn directions from a POSITION,
// projected onto the nine real spherical harmonics of bands 0 to 2 ON THE DEVICE.  A probe costs 12 bytes up and 108 down; the
// same samples through rt_radiance would cost one rt_ray_desc up and one RGB down per sample.
//
// probe_kernel is lens_kernel (rt_lens.hip) with another START and another FINISH around the same per-lane
// integrator, rt_path_lane.h (its header describes the phases, the quorum and the hand-out).  This file holds:
//   START   the probe's stream (seed, 2^63 + probe, sample_begin + pass): two draws, the uniform direction; then the path's own stream
//           (seed, probe, sample_begin + pass) FROM ITS FIRST DRAW: sample n of rt_radiance with streams[i] = probe
//   FINISH  the NaN filter, then value x basis added into the slot's 27 sums
//   CLAIM   a slot of the hand-out is (probe, chunk): slot = probe * split + chunk
// WHERE THE 27 SUMS LIVE: in the slot's own record of the caller's workspace, [term][slot].  CLAIM zeroes
// it, FINISH reads, adds and writes it, probe_combine_kernel adds the records of a probe in chunk order.  The direction survives the
// path in three words of the lane's LDS record; the basis is evaluated in FINISH.  No sum lives in a register across the walk.
// The loop keeps ONE back edge, no dynamically indexed array, and reads launch constants through aov_kargs where it uses them.
//
// Ray counters: lens_kernel's (the functor handed to path_lane_walk).
#include "rt_path_lane.h"
#include "rt_probe.h"

namespace rt {

struct ProbeArgs {
	DevScene S;
	DevProbeParams P;
};

// lanes of the wave that must wait for a closest-hit walk before it runs while shadow rays are pending elsewhere (as kLensQuorum)
#ifndef RT_PROBE_QUORUM
#define RT_PROBE_QUORUM 32
#endif
constexpr uint32_t kProbeQuorum = RT_PROBE_QUORUM;

// the basis of rt_hip.h on a direction AS GIVEN (not renormalised), every product in the written order
struct ProbeBasis {
	float y0, y1, y2, y3, y4, y5, y6, y7, y8;
};
__device__ __forceinline__ ProbeBasis probe_basis(float x, float y, float z)
{
	ProbeBasis B;
	B.y0 = 0.282094792f;
	B.y1 = 0.488602512f * y;
	B.y2 = 0.488602512f * z;
	B.y3 = 0.488602512f * x;
	B.y4 = 1.092548431f * (x * y);
	B.y5 = 1.092548431f * (y * z);
	B.y6 = 0.315391565f * (3.0f * (z * z) - 1.0f);
	B.y7 = 1.092548431f * (x * z);
	B.y8 = 0.546274215f * (x * x - y * y);
	return B;
}

template <int METHOD, bool PRUNE>
__global__ __launch_bounds__(256, kProbeWaves) void probe_kernel(const ProbeArgs args_by_value)
{
	using F = FeatFull; // every primitive, material and texture type compiled in (as lens_kernel)
	extern __shared__ __align__(16) uint32_t lds[];
	const DevScene &S = args_by_value.S;
	const WaveStack W = wave_stack(S, lds);
	// behind the stacks: the lane's record (word w of thread t at rec[256 w])
	uint32_t *const rec = lds + kFourWaves * (S.stack_depth * kStackStride) + threadIdx.x;
	enum : uint32_t {
		R_DIR = 0u * 256u,       // [3] the direction of the sample in flight
		R_SLOT = 3u * 256u,      // probe * split + chunk
		R_PROBE = 4u * 256u,     // the probe
		R_PASS = 5u * 256u,      // the pass in flight, counted from the probe's first
		R_CHUNK_END = 6u * 256u, // where its chunk ends
		R_RAYS = 7u * 256u,      // the lane's ray counter (flushed in FINISH long before it could wrap)
	};
	rec[R_RAYS] = 0u;
	const auto count_ray = [rec] { rec[R_RAYS] += 1u; };
	WaveBlocks blocks; // of 64 slots
	PathLane L;        // the path, in registers

#pragma unroll 1
	for (;;) {
		// ---- FINISH: the sample's value times the basis of its direction, added into the slot's record ----
		if (L.ph >= PH_FINISH) {
			const V3 v = L.sample_value();
			const KArgPtr<ProbeArgs> ka = aov_kargs(args_by_value);
			const size_t stride = ka->P.n_slots;
			float *const r = ka->P.records + rec[R_SLOT];
			const ProbeBasis B = probe_basis(__uint_as_float(rec[R_DIR]), __uint_as_float(rec[R_DIR + 256u]), __uint_as_float(rec[R_DIR + 512u]));
			// three bands of the record at a time: nine loads in flight, then nine adds and stores (one statement per term would
			// wait for each load behind the store before it, 27 round trips to memory in a row)
#define RT_PROBE_ADD3(j, Ya, Yb, Yc)                                                                                                     \
	{                                                                                                                                \
		float *const q = r + (3u * (j)) * stride;                                                                                    \
		const float a0 = q[0], a1 = q[stride], a2 = q[2u * stride], b0 = q[3u * stride], b1 = q[4u * stride], b2 = q[5u * stride], \
		            c0 = q[6u * stride], c1 = q[7u * stride], c2 = q[8u * stride];                                                   \
		q[0] = a0 + v.x * (Ya);                                                                                                      \
		q[stride] = a1 + v.y * (Ya);                                                                                                 \
		q[2u * stride] = a2 + v.z * (Ya);                                                                                            \
		q[3u * stride] = b0 + v.x * (Yb);                                                                                            \
		q[4u * stride] = b1 + v.y * (Yb);                                                                                            \
		q[5u * stride] = b2 + v.z * (Yb);                                                                                            \
		q[6u * stride] = c0 + v.x * (Yc);                                                                                            \
		q[7u * stride] = c1 + v.y * (Yc);                                                                                            \
		q[8u * stride] = c2 + v.z * (Yc);                                                                                            \
	}
			RT_PROBE_ADD3(0u, B.y0, B.y1, B.y2)
			RT_PROBE_ADD3(3u, B.y3, B.y4, B.y5)
			RT_PROBE_ADD3(6u, B.y6, B.y7, B.y8)
#undef RT_PROBE_ADD3
			{ // (a pass shoots fewer than 2^31 rays: the lane's counter cannot wrap)
				uint32_t lane_rays = rec[R_RAYS];
				if (lane_rays >= 0x80000000u) {
					unsigned long long *const rays_shot = ka->P.rays_shot;
					if (rays_shot != nullptr)
						atomicAdd(rays_shot, (unsigned long long)lane_rays);
					lane_rays = 0u;
				}
				rec[R_RAYS] = lane_rays;
			}
			const uint32_t k = rec[R_PASS] + 1u;
			rec[R_PASS] = k;
			L.ph = k == rec[R_CHUNK_END] ? PH_CLAIM : PH_START;
		}
		// ---- CLAIM: the next slot of the wave's block -> probe, chunk and its passes; the record from +0 ----
		const uint64_t need = __ballot(L.ph == PH_CLAIM);
		if (need != 0ull) { // (wave-uniform)
			const KArgPtr<ProbeArgs> ka = aov_kargs(args_by_value);
			const uint32_t n = ka->P.n_slots;
			if (L.ph == PH_CLAIM) {
				const uint32_t id = blocks.claimed(need);
				if (id >= n) {
					L.ph = PH_DONE;
				} else {
					const uint32_t split = ka->P.split, samples = ka->P.samples;
					const uint32_t probe = id / split, c = id - probe * split;
					rec[R_SLOT] = id;
					rec[R_PROBE] = probe;
					rec[R_PASS] = (uint32_t)(((uint64_t)c * samples) / split);
					rec[R_CHUNK_END] = (uint32_t)(((uint64_t)(c + 1u) * samples) / split);
					float *r = ka->P.records + id; // (id < n_slots: every term of the slot is inside the workspace)
#pragma unroll
					for (uint32_t t = 0u; t < kProbeTerms; ++t, r += n) // (unrolled: 27 stores, no back edge)
						*r = 0.0f;
					L.ph = PH_START;
				}
			}
			blocks.advance(need, n);
		}
		// ---- START: the next pass of the probe (rt_hip.h states every expression; all of it f32, in the written order) ----
		if (L.ph == PH_START) {
			const KArgPtr<ProbeArgs> ka = aov_kargs(args_by_value);
			const uint64_t seed = ((uint64_t)ka->P.seed_hi << 32) | ka->P.seed_lo;
			const uint64_t sample_begin = ((uint64_t)ka->P.sample_begin_hi << 32) | ka->P.sample_begin_lo;
			const uint32_t probe = rec[R_PROBE], k = rec[R_PASS];
			rt_rng dir; // the probe's stream: no probe's path stream (probes are below 2^31)
			rt_rng_seed(&dir, seed, 0x8000000000000000ull + (uint64_t)probe, sample_begin + k);
			const float xi1 = rt_rng_f32(&dir), xi2 = rt_rng_f32(&dir);
			const float z = 1.0f - 2.0f * xi1;
			const float s = sqrtf(1.0f - z * z);
			const float phi = RT_TAU * xi2;
			const V3 d = v3(s * rt_cosf(phi), s * rt_sinf(phi), z);
			rec[R_DIR] = __float_as_uint(d.x);
			rec[R_DIR + 256u] = __float_as_uint(d.y);
			rec[R_DIR + 512u] = __float_as_uint(d.z);
			const float *const p = ka->P.positions + 3u * (size_t)probe;
			rt_rng_seed(&L.rng, seed, (uint64_t)probe, sample_begin + k); // the path's stream from its first draw
			L.ray = ray_new<F>(v3(p[0], p[1], p[2]), d);
			L.start();
		}

		const uint64_t m_closest = __ballot(L.ph == PH_CLOSEST), m_shadow = __ballot(L.ph == PH_SHADOW);
		if ((m_closest | m_shadow) == 0ull)
			break; // every lane is DONE (FINISH, CLAIM and START were emptied above)
		path_lane_walk<METHOD, PRUNE, kProbeQuorum, F>(L, args_by_value, W, m_closest, m_shadow, count_ray);
	}

	// ---- SamplerProgress.rays_shot: wave reduction, one atomic per wave (as lens_kernel) ----
	unsigned long long *const rays_shot = aov_kargs(args_by_value)->P.rays_shot;
	if (rays_shot != nullptr) {
		unsigned long long total = rec[R_RAYS];
		for (int off = 32; off > 0; off >>= 1)
			total += __shfl_down(total, off);
		if ((threadIdx.x & 63u) == 0u)
			atomicAdd(rays_shot, total);
	}
}

// the counter of a launch zeroed by a kernel, not a memset node (rt_render.hip reset_kernel says why)
__global__ void probe_zero_kernel(unsigned long long *rays_shot) { *rays_shot = 0ull; }

// records -> coefficients: the S records of a probe added in chunk order from +0, scaled by 4 pi / K, then the band factors
__global__ __launch_bounds__(256) void probe_combine_kernel(const DevProbeParams P)
{
	const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; // 27 * probe + term
	if (i >= (uint64_t)kProbeTerms * P.n_probes)
		return;
	const uint32_t probe = (uint32_t)(i / kProbeTerms), term = (uint32_t)(i - (uint64_t)probe * kProbeTerms);
	const float *m = P.records + ((size_t)term * P.n_slots + (size_t)probe * P.split);
	float a = 0.0f;
	for (uint32_t c = 0; c < P.split; ++c)
		a = a + m[c];
	float coeff = a * (12.5663706f / (float)P.samples);
	if (P.convolve != 0u) {
		const uint32_t j = term / 3u;
		coeff = coeff * (j == 0u ? RT_PI : j < 4u ? 2.09439510f : 0.785398163f);
	}
	P.out[i] = coeff;
}

// coefficients and normals -> colours: the nine terms from +0 in order; an index past the probes gives the quiet NaN
__global__ __launch_bounds__(256) void probe_eval_kernel(const DevProbeEvalParams P)
{
	const uint64_t step = (uint64_t)gridDim.x * 256u;
	for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < P.m; i += step) {
		const uint64_t p = P.probe_index != nullptr ? (uint64_t)P.probe_index[i] : i;
		float *const o = P.out + 3u * i;
		if (p >= P.n_probes) {
			o[0] = o[1] = o[2] = __uint_as_float(0x7FC00000u);
		} else {
			const float *const n = P.normals + 3u * i;
			const float *const c = P.coeffs + (size_t)kProbeTerms * p;
			const ProbeBasis B = probe_basis(n[0], n[1], n[2]);
			float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f;
#define RT_PROBE_TERM(j, Y)            \
	a0 = a0 + c[3 * j + 0] * (Y); \
	a1 = a1 + c[3 * j + 1] * (Y); \
	a2 = a2 + c[3 * j + 2] * (Y);
			RT_PROBE_TERM(0, B.y0)
			RT_PROBE_TERM(1, B.y1)
			RT_PROBE_TERM(2, B.y2)
			RT_PROBE_TERM(3, B.y3)
			RT_PROBE_TERM(4, B.y4)
			RT_PROBE_TERM(5, B.y5)
			RT_PROBE_TERM(6, B.y6)
			RT_PROBE_TERM(7, B.y7)
			RT_PROBE_TERM(8, B.y8)
#undef RT_PROBE_TERM
			o[0] = a0;
			o[1] = a1;
			o[2] = a2;
		}
	}
}

hipError_t launch_probe(int method, bool prune, hipStream_t stream, const DevScene &S, const DevProbeParams &P, uint32_t groups)
{
	if (P.rays_shot != nullptr) {
		hipLaunchKernelGGL(probe_zero_kernel, dim3(1), dim3(1), 0, stream, P.rays_shot);
		const hipError_t e = hipGetLastError();
		if (e != hipSuccess)
			return e;
	}
	ProbeArgs A;
	A.S = S;
	A.P = P;
	void (*const fn)(const ProbeArgs) = method == 0 ? (prune ? probe_kernel<0, true> : probe_kernel<0, false>)
	                                                : (prune ? probe_kernel<1, true> : probe_kernel<1, false>);
	const hipError_t e = launch_path_lanes(fn, groups, four_wave_stack_lds_bytes(S) + kProbeRecordLdsBytes, stream, A);
	if (e != hipSuccess)
		return e;
	const uint64_t n_out = (uint64_t)kProbeTerms * P.n_probes; // below 27 * 2^31: the grid is below 2^28 workgroups
	hipLaunchKernelGGL(probe_combine_kernel, dim3((uint32_t)((n_out + 255u) / 256u)), dim3(256), 0, stream, P);
	return hipGetLastError();
}

hipError_t launch_probe_eval(hipStream_t stream, const DevProbeEvalParams &P)
{
	const uint64_t blocks = (P.m + 255u) / 256u; // beyond 2^20 workgroups the threads stride
	hipLaunchKernelGGL(probe_eval_kernel, dim3((uint32_t)(blocks < (1ull << 20) ? blocks : (1ull << 20))), dim3(256), 0, stream, P);
	return hipGetLastError();
}

} // namespace rt
