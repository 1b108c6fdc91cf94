// rt_selftest.hip -- the device self-tests (include/rt_hip.h): the kernels' own arithmetic and sky code, callable directly.
//   rt_selftest_lean          the short arithmetic forms of rt_lean.h against the plain operators
//   rt_selftest_pair_primary  the host's DevPairPrimary against the same terms formed on the device
//   rt_selftest_sky           sky_sample / sky_pdf of rt_shade.h on the caller's streams and directions
// No render launches any of these, so they share no translation unit with the render kernels (rt_render.hip).
#include <algorithm>

#include "rt_shade.h"
#include "rt_selftest.h"
#include "rt_selftest_dev.h"

namespace rt {

// ---- rt_selftest_lean: the short arithmetic forms of rt_lean.h against the plain operators / rt_detmath.h, on the device.
// Operand classes: 0 lean_div, 1 lean_div_fix (numerator may be zero / inf / NaN), 2 lean_inv, 3 lean_div3 (shared reciprocal),
// 4 lean_sqrt, 5 lean_sincos, 6 lean_acos_dev, 7 lean_atan2, 8 ray_new (fast path and fallback against the plain operators).
// mismatches[k] counts results whose BITS differ (two NaNs count as equal). ----
__device__ __forceinline__ float tame_from_bits(uint32_t u, int lo_exp, int hi_exp) // random sign and mantissa, exponent in [lo_exp, hi_exp]
{
	const uint32_t span = (uint32_t)(hi_exp - lo_exp + 1);
	const uint32_t e = (uint32_t)(127 + lo_exp) + ((u >> 23) & 0xFFu) % span;
	return __uint_as_float((u & 0x807FFFFFu) | (e << 23));
}
__global__ __launch_bounds__(256) void selftest_lean_kernel(uint64_t n_per_thread, uint64_t seed, unsigned long long *__restrict__ mismatches)
{
	const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	rt_rng rng;
	rt_rng_seed(&rng, seed, tid, 0x5E1F7E57ull);
	unsigned long long bad[9] = {};
	for (uint64_t it = 0; it < n_per_thread; ++it) {
		const uint32_t u0 = rt_rng_u32(&rng), u1 = rt_rng_u32(&rng), u2 = rt_rng_u32(&rng), u3 = rt_rng_u32(&rng);
		// tame operands at the EDGES of what the call sites guarantee as well as in the middle
		const float d = tame_from_bits(u0, -81, 41), n = tame_from_bits(u1, -81, 41);
		if (fabsf(n) <= fabsf(d) * 0x1p95f && fabsf(d) <= fabsf(n) * 0x1p120f) {
			bad[0] += !same_f32(lean_div(n, d), n / d);
			bad[1] += !same_f32(lean_div_fix(n, d), n / d);
		}
		const uint32_t pick = u2 & 7u; // special numerators for the fix-up form
		const float ns = pick == 0u ? 0.0f : (pick == 1u ? -0.0f : (pick == 2u ? INFINITY : (pick == 3u ? -INFINITY : (pick == 4u ? __uint_as_float(0x7FC00000u) : n))));
		if (pick < 5u)
			bad[1] += !same_f32(lean_div_fix(ns, d), ns / d);
		bad[2] += !same_f32(lean_inv(d), 1.0f / d);
		{
			const V3 v = v3(tame_from_bits(u1, -60, 20), tame_from_bits(u2, -60, 20), tame_from_bits(u3, -60, 20));
			const float dd = tame_from_bits(u0, -20, 20);
			const V3 a = lean_div3(v, dd), b = v / dd;
			bad[3] += !(same_f32(a.x, b.x) && same_f32(a.y, b.y) && same_f32(a.z, b.z));
			const V3 vz = v3((u3 & 1u) ? 0.0f : v.x, (u3 & 2u) ? -0.0f : v.y, v.z);
			const V3 af = lean_div3_fix(vz, dd), bf = vz / dd;
			bad[3] += !(same_f32(af.x, bf.x) && same_f32(af.y, bf.y) && same_f32(af.z, bf.z));
		}
		{
			// square roots: the whole stated domain -- zero, [2^-96, inf], NaN, negatives -- and squares near exact roots
			const uint32_t k = u3 & 15u;
			float x = fabsf(tame_from_bits(u0, -96, 127));
			if (k == 0u) x = 0.0f; else if (k == 1u) x = -0.0f; else if (k == 2u) x = INFINITY; else if (k == 3u) x = -fabsf(n);
			else if (k == 4u) { const float r = fabsf(tame_from_bits(u1, -40, 40)); x = r * r; }
			else if (k == 5u) x = 1.0f - (float)(u1 >> 8) * 5.9604644775390625e-08f; // 1 - r, the Lambert sampler's argument
			else if (k == 6u) x = __uint_as_float(0x0F800000u + (u1 & 0xFFu));          // just above 2^-96
			bad[4] += !same_f32(lean_sqrt(x), sqrtf(x));
		}
		{
			const float r = (float)(u0 >> 8) * 5.9604644775390625e-08f;
			const float ang = (u1 & 1u) ? 2.0f * kPi * r : ((u1 & 2u) ? kPi * r * (1.0f + 0x1p-20f) : (float)(int32_t)(u2 >> 9) * r - 4194304.0f * r);
			float s_, c_;
			lean_sincos(ang, s_, c_);
			bad[5] += !(same_f32(s_, rt_sinf(ang)) && same_f32(c_, rt_cosf(ang)));
		}
		{
			const uint32_t k = u3 & 7u;
			float x = 2.0f * ((float)(u0 >> 8) * 5.9604644775390625e-08f) - 1.0f;
			if (k == 0u) x = tame_from_bits(u0, -30, 1); else if (k == 1u) x = (u1 & 1u) ? 1.0f : -1.0f; else if (k == 2u) x = __uint_as_float(0x3F000000u + (u1 & 3u) - 1u);
			else if (k == 3u) x = __uint_as_float(0x7FC00000u);
			bad[6] += !same_f32(lean_acos_dev(x), rt_acosf(x));
		}
		{
			const uint32_t k = u3 >> 28;
			float y = tame_from_bits(u0, -30, 30), x = tame_from_bits(u1, -30, 30);
			if (k == 0u) y = 0.0f; else if (k == 1u) x = -0.0f; else if (k == 2u) { x = 0.0f; y = -0.0f; } else if (k == 3u) y = (u2 & 1u) ? x : -x;
			else if (k == 4u) x = INFINITY; else if (k == 5u) { x = -INFINITY; y = INFINITY; } else if (k == 6u) y = __uint_as_float(0x7FC00000u);
			else if (k == 7u) { x = __uint_as_float(u0); y = __uint_as_float(u1); }
			bad[7] += !same_f32(lean_atan2(y, x), rt_atan2f(y, x));
		}
		{
			const uint32_t k = u3 & 15u;
			V3 dir = v3(tame_from_bits(u0, -8, 8), tame_from_bits(u1, -8, 8), tame_from_bits(u2, -8, 8));
			if (k == 0u) dir.x = 0.0f; else if (k == 1u) dir = v3(tame_from_bits(u0, -62, -58), tame_from_bits(u1, -8, 8), tame_from_bits(u2, -22, 21));
			else if (k == 2u) dir = v3(tame_from_bits(u0, -70, 70), tame_from_bits(u1, -70, 70), tame_from_bits(u2, -70, 70));
			else if (k == 3u) dir.y = -0.0f;
			const Ray a = ray_new<FeatFull>(v3s(0.0f), dir), b = ray_new_plain(v3s(0.0f), dir);
			bad[8] += !(same_f32(a.d.x, b.d.x) && same_f32(a.d.y, b.d.y) && same_f32(a.d.z, b.d.z) && same_f32(a.inv.x, b.inv.x) && same_f32(a.inv.y, b.inv.y) &&
			            same_f32(a.inv.z, b.inv.z) && same_f32(a.shear.x, b.shear.x) && same_f32(a.shear.y, b.shear.y) && same_f32(a.shear.z, b.shear.z));
		}
	}
	for (int k = 0; k < 9; ++k)
		if (bad[k])
			atomicAdd(&mismatches[k], bad[k]);
}
hipError_t launch_selftest_lean(hipStream_t stream, uint32_t blocks, uint64_t n_per_thread, uint64_t seed, unsigned long long *mismatches)
{
	hipLaunchKernelGGL(selftest_lean_kernel, dim3(blocks), dim3(256), 0, stream, n_per_thread, seed, mismatches);
	return hipGetLastError();
}

// ---- rt_selftest_pair_primary: the host's DevPairPrimary against the same terms formed on the device (one lane), word by word ----
struct PairPrimaryCheck {
	DevPairScene pair;
	DevPairPrimary host;
	float root_min[3], root_max[3], origin[3];
};
__global__ __launch_bounds__(64) void selftest_pair_primary_kernel(const PairPrimaryCheck c, unsigned long long *__restrict__ mismatches)
{
	if (threadIdx.x != 0u || blockIdx.x != 0u)
		return;
	DevPairPrimary d;
	pair_primary_terms(c.pair, c.root_min, c.root_max, v3(c.origin[0], c.origin[1], c.origin[2]), d);
	auto differ = [](float a, float b) { return __float_as_uint(a) != __float_as_uint(b) && !(a != a && b != b); }; // (NaN == NaN)
	unsigned long long bad = d.valid != c.host.valid ? 1ull : 0ull;
	for (int ch = 0; ch < 2; ++ch) {
		for (int k = 0; k < 3; ++k) {
			bad += differ(d.box[ch][0][k], c.host.box[ch][0][k]);
			bad += differ(d.box[ch][1][k], c.host.box[ch][1][k]);
			bad += differ(d.root[ch][k], c.host.root[ch][k]);
		}
		for (int k = 0; k < 4; ++k)
			bad += differ(d.sphere[ch][k], c.host.sphere[ch][k]);
		bad += differ(d.deltapdot[ch], c.host.deltapdot[ch]);
	}
	*mismatches = bad;
}
hipError_t launch_selftest_pair_primary(hipStream_t stream, const DevPairScene &pair, const float root_min[3], const float root_max[3], const float origin[3],
                                        const DevPairPrimary &host_block, unsigned long long *mismatches)
{
	PairPrimaryCheck c;
	c.pair = pair;
	c.host = host_block;
	for (int k = 0; k < 3; ++k) {
		c.root_min[k] = root_min[k];
		c.root_max[k] = root_max[k];
		c.origin[k] = origin[k];
	}
	hipLaunchKernelGGL(selftest_pair_primary_kernel, dim3(1), dim3(64), 0, stream, c, mismatches);
	return hipGetLastError();
}

// ---- rt_selftest_sky: the render kernels' own sky code, callable directly.  One thread per
// item: item i < n seeds a stream with rt_rng_seed(seed, 0, i), runs sky_sample on it and sky_pdf at the direction it got; item
// n + j runs sky_pdf at the caller's direction j.  The inline functions are rt_shade.h's, untouched; the tables are read where a
// render reads them: from global memory, or staged into LDS in the layout of render_kernel's prologue (rt_render.hip: rows and
// marginal, padding to 16 bytes, guides), with the verified reciprocals read through the kernel arguments as there. ----
struct SkySelftestArgs {
	DevScene S;
	DevSkySelftest P;
};

template <bool SKY_LDS>
__global__ __launch_bounds__(256) void sky_selftest_kernel(const SkySelftestArgs args_by_value)
{
	extern __shared__ __align__(16) uint32_t lds[];
#if defined(__HIP_DEVICE_COMPILE__)
	typedef const __attribute__((address_space(4))) SkySelftestArgs *KArgs;
	const KArgs K = (KArgs)__builtin_amdgcn_kernarg_segment_ptr();
#else
	const SkySelftestArgs *K = &args_by_value;
#endif
	(void)args_by_value;
	const DevScene S = K->S;
	const DevSkySelftest P = K->P;

	SkyTables T;
	if (SKY_LDS) {
		const uint32_t n_rows = S.sky.res_y * (S.sky.res_x + 1u);
		const uint32_t n_all = n_rows + S.sky.res_y + 1u;
		float *lds_sky = reinterpret_cast<float *>(lds);
		for (uint32_t i = threadIdx.x; i < n_all; i += blockDim.x)
			lds_sky[i] = S.sky.row_cdf[i]; // marginal follows the rows in the same allocation
		const uint32_t sky_words = (n_all + 3u) & ~3u;
		const uint32_t guide_words = (S.sky.res_y + 1u) * S.sky.guide_k / 4u;
		uint32_t *lds_guide = lds + sky_words;
		const uint32_t *src_guide = reinterpret_cast<const uint32_t *>(S.sky.guide);
		for (uint32_t i = threadIdx.x; i < guide_words; i += blockDim.x)
			lds_guide[i] = src_guide[i];
		__syncthreads();
		T.row_cdf = lds_sky;
		T.marginal_cdf = lds_sky + n_rows;
		T.guide = reinterpret_cast<const uint8_t *>(lds_guide);
	} else {
		T.row_cdf = S.sky.row_cdf;
		T.marginal_cdf = S.sky.marginal_cdf;
		T.guide = S.sky.guide;
	}
	T.guide_k = S.sky.guide_k;
	T.inv_res = reinterpret_cast<KWords>(&K->S.sky.inv_res_ok);

	const uint64_t total = P.n + P.m;
	for (uint64_t item = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; item < total; item += (uint64_t)gridDim.x * blockDim.x) {
		if (item < P.n) {
			rt_rng rng;
			rt_rng_seed(&rng, P.seed, 0, item);
			const V3 d = sky_sample(S, T, rng);
			P.out_dirs[3 * item] = d.x;
			P.out_dirs[3 * item + 1] = d.y;
			P.out_dirs[3 * item + 2] = d.z;
			P.out_pdf_s[item] = sky_pdf(S, T, d);
		} else {
			const uint64_t j = item - P.n;
			P.out_pdf[j] = sky_pdf(S, T, v3(P.dirs[3 * j], P.dirs[3 * j + 1], P.dirs[3 * j + 2]));
		}
	}
}

size_t sky_selftest_lds_bytes(const DevScene &S)
{
	const uint32_t n_all = S.sky.res_y * (S.sky.res_x + 1u) + S.sky.res_y + 1u;
	return ((size_t)((n_all + 3u) & ~3u) + (size_t)(S.sky.res_y + 1u) * S.sky.guide_k / 4u) * sizeof(uint32_t);
}

hipError_t launch_sky_selftest(bool tables_in_lds, hipStream_t stream, const DevScene &S, const DevSkySelftest &P)
{
	SkySelftestArgs A;
	A.S = S;
	A.P = P;
	const uint64_t total = P.n + P.m;
	const uint32_t blocks = (uint32_t)std::min<uint64_t>((total + 255) / 256, 2048); // (a staged table is copied once per workgroup)
	if (tables_in_lds) {
		const size_t lds_bytes = sky_selftest_lds_bytes(S);
		hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(sky_selftest_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
		if (e != hipSuccess)
			return e;
		hipLaunchKernelGGL(sky_selftest_kernel<true>, dim3(blocks), dim3(256), lds_bytes, stream, A);
	} else {
		hipLaunchKernelGGL(sky_selftest_kernel<false>, dim3(blocks), dim3(256), 0, stream, A);
	}
	return hipGetLastError();
}

} // namespace rt
