// rt_sky_selftest.hip -- rt_selftest_sky (include/rt_hip.h): the render kernels' own sky code, callable directly.  One thread per
// item: item i < n seeds a stream with rt_rng_seed(seed, 0, i), runs sky_sample on it and sky_pdf at the direction it got; item
// n + j runs sky_pdf at the caller's direction j.  The inline functions are rt_shade.h's, untouched; the tables are read where a
// render reads them: from global memory, or staged into LDS in the layout of render_kernel's prologue (rt_render.hip: rows and
// marginal, padding to 16 bytes, guides), with the verified reciprocals read through the kernel arguments as there.
#include <algorithm>

#include "rt_shade.h"
#include "rt_sky_selftest.h"

namespace rt {

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
