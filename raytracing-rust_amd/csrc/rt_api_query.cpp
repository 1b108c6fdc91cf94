// rt_api_query.cpp -- the entry points of librt_hip.so that ask a scene or the device a question without rendering: the batch
// hit queries (rt_check_hit / rt_check_hit_index), the radiance queries (rt_radiance), the self-tests (rt_selftest_*) and, in the
// diagnostic build, rt_debug_trace_queue.  Their kernels are rt_query.hip, rt_radiance.hip and rt_selftest.hip; the scene handle,
// the error convention and the traversal policy are rt_api_internal.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "../../include/rt_hip.h"
#include "rt_api_internal.h"
#include "rt_query.h"
#include "rt_radiance.h"
#include "rt_selftest.h"
#include "rt_gen_keys.h"

using namespace rt;

#ifdef RT_STATS
// diagnostic build only (tests/probes/gpu_trace_queue.py): n rays through the traversal-only persistent kernel at `waves`
// waves/SIMD with `cap` stack entries per lane in LDS; returns (t, primitive) per ray, the kernel time and the node steps
extern "C" int rt_debug_trace_queue(rt_scene *s, const rt_ray_desc *rays, uint64_t n, int waves, uint32_t cap, float *out_t, uint32_t *out_prim,
                                    float *ms, unsigned long long *node_steps)
{
	if (!s || !rays || !out_t || !out_prim || n == 0 || n >= (1ull << 31) || s->device == RT_DEVICE_NONE || s->dev.nodes4 == nullptr)
		return fail(RT_ERR_INVALID_ARGUMENT, "bad arguments (or no wide tree)");
	HIP_TRY(hipSetDevice(s->device));
	cap = std::min(std::max(cap, 1u), s->dev.stack_depth);
	const uint32_t ovf_depth = s->dev.stack_depth - cap;
	const uint32_t n_blocks = (uint32_t)s->n_cus * (uint32_t)waves;
	const size_t lds_bytes = (size_t)4 * cap * 64 * 4;
	void *d_rays = nullptr, *d_out = nullptr, *d_misc = nullptr, *d_ovf = nullptr;
	HIP_TRY(hipMalloc(&d_rays, n * sizeof(rt_ray_desc)));
	HIP_TRY(hipMalloc(&d_out, n * 8));
	HIP_TRY(hipMalloc(&d_misc, 16));
	HIP_TRY(hipMalloc(&d_ovf, std::max<size_t>(16, (size_t)n_blocks * 256 * ovf_depth * 4)));
	HIP_TRY(hipMemcpy(d_rays, rays, n * sizeof(rt_ray_desc), hipMemcpyHostToDevice));
	float best = 1e30f;
	for (int rep = 0; rep < 3; ++rep) {
		HIP_TRY(hipMemset(d_misc, 0, 16));
		HIP_TRY(hipEventRecord(s->ev_start, s->stream));
		HIP_TRY(launch_trace_queue(waves, n_blocks, lds_bytes, s->stream, s->dev, d_rays, (uint32_t)n, d_out, static_cast<uint32_t *>(d_misc),
		                           reinterpret_cast<unsigned long long *>(static_cast<char *>(d_misc) + 8), cap, ovf_depth, static_cast<uint32_t *>(d_ovf)));
		HIP_TRY(hipEventRecord(s->ev_stop, s->stream));
		HIP_TRY(hipEventSynchronize(s->ev_stop));
		float t = 0.0f;
		HIP_TRY(hipEventElapsedTime(&t, s->ev_start, s->ev_stop));
		best = std::min(best, t);
	}
	std::vector<float> tmp(2 * n);
	HIP_TRY(hipMemcpy(tmp.data(), d_out, n * 8, hipMemcpyDeviceToHost));
	for (uint64_t i = 0; i < n; ++i) {
		out_t[i] = tmp[2 * i];
		std::memcpy(&out_prim[i], &tmp[2 * i + 1], 4);
	}
	if (node_steps)
		HIP_TRY(hipMemcpy(node_steps, static_cast<char *>(d_misc) + 8, 8, hipMemcpyDeviceToHost));
	if (ms)
		*ms = best;
	(void)hipFree(d_rays); (void)hipFree(d_out); (void)hipFree(d_misc); (void)hipFree(d_ovf);
	return RT_OK;
}
#endif

extern "C" {

// ---- batch hit queries ----
static int check_common(rt_scene *s, const rt_ray_desc *rays, const uint64_t *object_index, uint64_t n, rt_hit_record *out)
{
	if (!s || !rays || !out)
		return fail(RT_ERR_INVALID_ARGUMENT, "null argument");
	if (int rc = need_device(s); rc != RT_OK)
		return rc;
	if (n == 0)
		return RT_OK;
	if (object_index)
		for (uint64_t i = 0; i < n; ++i)
			if (object_index[i] >= s->dev.n_prims)
				return fail(RT_ERR_INVALID_ARGUMENT, "object index out of range");
	bool prune = false;
	DevScene dev;
	if (int rc = four_wave_traversal(s, &prune, &dev); rc != RT_OK) // (rt_api_internal.h)
		return rc;
	HIP_TRY(hipSetDevice(s->device));
	void *d_rays = nullptr, *d_out = nullptr, *d_idx = nullptr;
	HIP_TRY(hipMalloc(&d_rays, n * sizeof(rt_ray_desc)));
	hipError_t e = hipMalloc(&d_out, n * sizeof(rt_hit_record));
	if (e == hipSuccess && object_index)
		e = hipMalloc(&d_idx, n * sizeof(uint64_t));
	if (e == hipSuccess)
		e = hipMemcpyAsync(d_rays, rays, n * sizeof(rt_ray_desc), hipMemcpyHostToDevice, s->stream);
	if (e == hipSuccess && object_index)
		e = hipMemcpyAsync(d_idx, object_index, n * sizeof(uint64_t), hipMemcpyHostToDevice, s->stream);
	if (e == hipSuccess)
		e = object_index ? launch_check_hit_index(prune, s->stream, dev, d_rays, d_idx, n, d_out)
		                 : launch_check_hit(prune, s->stream, dev, d_rays, n, d_out);
	if (e == hipSuccess)
		e = hipMemcpyAsync(out, d_out, n * sizeof(rt_hit_record), hipMemcpyDeviceToHost, s->stream);
	if (e == hipSuccess)
		e = hipStreamSynchronize(s->stream);
	(void)hipFree(d_rays);
	(void)hipFree(d_out);
	(void)hipFree(d_idx);
	if (e != hipSuccess)
		return hip_fail(e, "check_hit");
	return RT_OK;
}

int rt_check_hit(rt_scene *s, const rt_ray_desc *rays, uint64_t n_rays, rt_hit_record *out)
{
	return check_common(s, rays, nullptr, n_rays, out);
}
int rt_check_hit_index(rt_scene *s, const rt_ray_desc *rays, const uint64_t *object_index, uint64_t n_rays, rt_hit_record *out)
{
	if (!object_index)
		return fail(RT_ERR_INVALID_ARGUMENT, "null argument");
	return check_common(s, rays, object_index, n_rays, out);
}

// ---- radiance queries (rt_radiance.hip) ----
int rt_radiance_opts_default(rt_radiance_opts *out)
{
	if (!out)
		return fail(RT_ERR_INVALID_ARGUMENT, "null argument");
	std::memset(out, 0, sizeof *out);
	out->samples_per_ray = 1;
	out->render_method = RT_METHOD_MIS;
	out->max_depth = 50;
	out->rr_threshold = 3;
	return RT_OK;
}

// argument checks of both entry points, the device last (so that a host-only scene reports bad arguments as such)
static int radiance_check(const rt_scene *s, const rt_ray_desc *rays, uint64_t n, const rt_radiance_opts *o, const float *out)
{
	if (!s || !rays || !o || !out)
		return fail(RT_ERR_INVALID_ARGUMENT, "null argument");
	if (o->samples_per_ray == 0)
		return fail(RT_ERR_INVALID_ARGUMENT, "radiance: samples_per_ray must be >= 1");
	if (o->render_method != RT_METHOD_NAIVE && o->render_method != RT_METHOD_MIS)
		return fail(RT_ERR_INVALID_ARGUMENT, "radiance: unknown render_method");
	for (uint32_t r : o->reserved)
		if (r != 0u)
			return fail(RT_ERR_INVALID_ARGUMENT, "radiance: reserved must be zero");
	if (n >= (1ull << 31))
		return fail(RT_ERR_UNSUPPORTED, "radiance: 2^31 rays or more in one call");
	return need_device(s);
}

int rt_radiance_device(rt_scene *s, const rt_ray_desc *d_rays, const uint64_t *d_streams, uint64_t n_rays, const rt_radiance_opts *o,
                       float *d_out_rgb, void *hip_stream)
{
	if (int rc = radiance_check(s, d_rays, n_rays, o, d_out_rgb); rc != RT_OK)
		return rc;
	if (n_rays == 0)
		return RT_OK;
	// a multi-device head is an ordinary scene on devices[0]: the query runs there alone
	HIP_TRY(hipSetDevice(s->device));
	bool prune = false;
	DevScene dev;
	if (int rc = four_wave_traversal(s, &prune, &dev); rc != RT_OK) // (rt_api_internal.h)
		return rc;
	DevRadianceParams P;
	std::memset(&P, 0, sizeof P);
	P.rays = reinterpret_cast<const float *>(d_rays);
	P.streams = d_streams;
	P.out = d_out_rgb;
	P.n_rays = (uint32_t)n_rays;
	P.samples = o->samples_per_ray;
	P.seed_lo = (uint32_t)o->seed;
	P.seed_hi = (uint32_t)(o->seed >> 32);
	P.sample_begin_lo = (uint32_t)o->sample_begin;
	P.sample_begin_hi = (uint32_t)(o->sample_begin >> 32);
	P.max_depth = o->max_depth;
	P.rr_threshold = o->rr_threshold;
	// one lane per ray (n_rays >= 1 here, so the planner's floor of one workgroup changes nothing)
	HIP_TRY(launch_radiance(o->render_method == RT_METHOD_NAIVE ? 0 : 1, prune, static_cast<hipStream_t>(hip_stream), dev, P,
	                        path_lane_groups(s, four_wave_stack_lds_bytes(dev), kRadianceWaves, (n_rays + 255) / 256)));
	return RT_OK;
}

int rt_radiance(rt_scene *s, const rt_ray_desc *rays, const uint64_t *streams, uint64_t n_rays, const rt_radiance_opts *o, float *out_rgb)
{
	if (int rc = radiance_check(s, rays, n_rays, o, out_rgb); rc != RT_OK)
		return rc;
	if (n_rays == 0)
		return RT_OK;
	HIP_TRY(hipSetDevice(s->device));
	// the rays, the streams if given, the output
	Layout L;
	const auto p_rays = L.add<rt_ray_desc>(n_rays);
	const auto p_streams = L.optional<uint64_t>(streams, n_rays);
	const auto p_out = L.add<float>(3 * n_rays);
	RT_TRY(grow_device_buffer(s->d_denoise, s->d_denoise_bytes, L)); // shared with rt_denoise / rt_render_ao
	Staging st{s};
	st.put(L, p_rays, rays);
	st.put(L, p_streams, streams);
	if (st.ok())
		st.rc = rt_radiance_device(s, L.at(p_rays), L.at(p_streams), n_rays, o, L.at(p_out), s->stream);
	st.get(out_rgb, L, p_out);
	return st.finish("radiance");
}

int rt_selftest_division(float divisor, float *reciprocal, int *exact)
{
	if (!reciprocal || !exact)
		return fail(RT_ERR_INVALID_ARGUMENT, "null argument");
	*exact = verified_reciprocal(divisor, reciprocal) ? 1 : 0;
	return RT_OK;
}

int rt_selftest_sky(rt_scene *s, int tables_in_lds, uint64_t seed, uint64_t n, float *out_dirs, float *out_pdf_of_sample, const float *dirs, uint64_t m,
                    float *out_pdf)
{
	if (!s || (tables_in_lds != 0 && tables_in_lds != 1) || (n && (!out_dirs || !out_pdf_of_sample)) || (m && (!dirs || !out_pdf)))
		return fail(RT_ERR_INVALID_ARGUMENT, "bad arguments");
	if (n > (1ull << 28) || m > (1ull << 28))
		return fail(RT_ERR_INVALID_ARGUMENT, "at most 2^28 samples and 2^28 directions");
	if ((s->host.sky.sampler_res_x | s->host.sky.sampler_res_y) == 0u)
		return fail(RT_ERR_INVALID_ARGUMENT, "the sky is not samplable (sampler_res 0 x 0)");
	if (int rc = need_device(s); rc != RT_OK)
		return rc;
	if (tables_in_lds && (sky_table_bytes(s->dev.sky.res_x, s->dev.sky.res_y, s->dev.sky.guide_k) > kSkyLdsLimit || sky_selftest_lds_bytes(s->dev) > s->max_lds))
		return fail(RT_ERR_UNSUPPORTED, "the sky tables exceed what a launch stages into LDS");
	if (n + m == 0)
		return RT_OK;
	HIP_TRY(hipSetDevice(s->device));
	// one allocation: directions and pdfs of the samples, then the caller's directions and their pdfs
	float *d = nullptr;
	HIP_TRY(hipMalloc(reinterpret_cast<void **>(&d), (4 * n + 4 * m) * sizeof(float)));
	DevSkySelftest P;
	P.seed = seed;
	P.n = n;
	P.m = m;
	P.out_dirs = d;
	P.out_pdf_s = d + 3 * n;
	float *d_dirs = d + 4 * n;
	P.dirs = d_dirs;
	P.out_pdf = d_dirs + 3 * m;
	hipError_t e = hipSuccess;
	if (m)
		e = hipMemcpyAsync(d_dirs, dirs, 3 * m * sizeof(float), hipMemcpyHostToDevice, s->stream);
	if (e == hipSuccess)
		e = launch_sky_selftest(tables_in_lds != 0, s->stream, s->dev, P);
	if (e == hipSuccess && n)
		e = hipMemcpyAsync(out_dirs, P.out_dirs, 3 * n * sizeof(float), hipMemcpyDeviceToHost, s->stream);
	if (e == hipSuccess && n)
		e = hipMemcpyAsync(out_pdf_of_sample, P.out_pdf_s, n * sizeof(float), hipMemcpyDeviceToHost, s->stream);
	if (e == hipSuccess && m)
		e = hipMemcpyAsync(out_pdf, P.out_pdf, m * sizeof(float), hipMemcpyDeviceToHost, s->stream);
	const hipError_t e_sync = hipStreamSynchronize(s->stream);
	if (e == hipSuccess)
		e = e_sync;
	(void)hipFree(d);
	if (e != hipSuccess)
		return hip_fail(e, "selftest_sky");
	return RT_OK;
}

int rt_selftest_lean(int device, uint64_t n_per_thread, uint64_t seed, uint64_t mismatches[RT_SELFTEST_LEAN_CLASSES])
{
	if (!mismatches || n_per_thread == 0 || n_per_thread > (1ull << 20))
		return fail(RT_ERR_INVALID_ARGUMENT, "bad arguments (n_per_thread in [1, 2^20])");
	int n_dev = 0;
	if (hipGetDeviceCount(&n_dev) != hipSuccess || device < 0 || device >= n_dev)
		return fail(RT_ERR_NO_DEVICE, "no such HIP device");
	HIP_TRY(hipSetDevice(device));
	unsigned long long *d = nullptr;
	HIP_TRY(hipMalloc(reinterpret_cast<void **>(&d), RT_SELFTEST_LEAN_CLASSES * sizeof(unsigned long long)));
	hipError_t e = hipMemset(d, 0, RT_SELFTEST_LEAN_CLASSES * sizeof(unsigned long long));
	if (e == hipSuccess)
		e = launch_selftest_lean(nullptr, 1024u, n_per_thread, seed, d);
	if (e == hipSuccess)
		e = hipMemcpy(mismatches, d, RT_SELFTEST_LEAN_CLASSES * sizeof(unsigned long long), hipMemcpyDeviceToHost);
	(void)hipFree(d);
	if (e != hipSuccess)
		return hip_fail(e, "selftest");
	return RT_OK;
}

int rt_selftest_short_forms(int device, const float *operands, uint64_t n_operands, rt_short_forms_result *out)
{
	if (!out || (operands && (n_operands == 0 || n_operands > (1ull << 20))) || (!operands && n_operands != 0))
		return fail(RT_ERR_INVALID_ARGUMENT, "bad arguments (operands NULL with n_operands 0, or 1 to 2^20 operands)");
	int n_dev = 0;
	if (hipGetDeviceCount(&n_dev) != hipSuccess || device < 0 || device >= n_dev)
		return fail(RT_ERR_NO_DEVICE, "no such HIP device");
	HIP_TRY(hipSetDevice(device));
	// one allocation: the counters in the order of DevShortForms, then the operands
	constexpr size_t kWords = 2 + RT_SHORT_FORMS + RT_SHORT_FORMS + 4 + 1 + RT_SHORT_SITES;
	unsigned long long host[kWords] = {};
	unsigned long long *d = nullptr;
	HIP_TRY(hipMalloc(reinterpret_cast<void **>(&d), kWords * sizeof *d + (size_t)n_operands * sizeof(float)));
	DevShortForms D;
	D.tested = d;
	D.mismatches = D.tested + 2;
	D.first_index = D.mismatches + RT_SHORT_FORMS;
	D.sqrt_raw = D.first_index + RT_SHORT_FORMS;
	D.site_tested = D.sqrt_raw + 4;
	D.site_mismatches = D.site_tested + 1;
	for (int k = 0; k < RT_SHORT_FORMS; ++k)
		host[2 + RT_SHORT_FORMS + k] = ~0ull;
	float *d_operands = reinterpret_cast<float *>(d + kWords);
	hipError_t e = hipMemcpy(d, host, sizeof host, hipMemcpyHostToDevice);
	if (e == hipSuccess && operands)
		e = hipMemcpy(d_operands, operands, (size_t)n_operands * sizeof(float), hipMemcpyHostToDevice);
	if (e == hipSuccess)
		e = launch_short_forms(nullptr, D, operands ? d_operands : nullptr, n_operands);
	if (e == hipSuccess)
		e = hipMemcpy(host, d, sizeof host, hipMemcpyDeviceToHost);
	(void)hipFree(d);
	if (e != hipSuccess)
		return hip_fail(e, "selftest_short_forms");
	std::memset(out, 0, sizeof *out);
	for (int k = 0; k < RT_SHORT_FORMS; ++k) {
		out->form[k].tested = host[k <= RT_SHORT_FORM_INV_TWO_PAIRS ? 0 : 1];
		out->form[k].mismatches = host[2 + k];
		if (out->form[k].mismatches)
			out->form[k].first_mismatch = short_forms_input_bits(k, host[2 + RT_SHORT_FORMS + k]);
	}
	const unsigned long long *raw = host + 2 + 2 * RT_SHORT_FORMS;
	out->sqrt_raw_exact = raw[0];
	out->sqrt_raw_high = raw[1];
	out->sqrt_raw_low = raw[2];
	out->sqrt_raw_other = raw[3];
	out->site_tested = raw[4];
	for (int k = 0; k < RT_SHORT_SITES; ++k)
		out->site_mismatches[k] = raw[5 + k];
	out->in_use = short_forms_in_use();
	return RT_OK;
}

int rt_selftest_div_forms(int device, const rt_div_forms_slice *slice, const float *operands, uint64_t n_operand_pairs, rt_div_forms_result *out)
{
	if (!out || (slice != nullptr) == (operands != nullptr))
		return fail(RT_ERR_INVALID_ARGUMENT, "bad arguments (a slice or operands, not both)");
	if (operands && (n_operand_pairs == 0 || n_operand_pairs > (1ull << 20)))
		return fail(RT_ERR_INVALID_ARGUMENT, "bad arguments (1 to 2^20 operand pairs)");
	if (slice) {
		if (!slice->exponents || slice->n_denominators == 0 || slice->n_exponent_pairs == 0 || slice->n_denominators > (1ull << 17) ||
		    slice->n_exponent_pairs > (1ull << 17) || slice->n_denominators * slice->n_exponent_pairs > (1ull << 17))
			return fail(RT_ERR_INVALID_ARGUMENT, "bad slice (n_denominators * n_exponent_pairs in [1, 2^17])");
		if (!slice->denominators && (uint64_t)slice->first_denominator + slice->n_denominators > (1ull << 23))
			return fail(RT_ERR_INVALID_ARGUMENT, "bad slice (the range leaves the 2^23 significands)");
		for (uint64_t k = 0; k < 2 * slice->n_exponent_pairs; ++k)
			if (slice->exponents[k] < -126 || slice->exponents[k] > 127)
				return fail(RT_ERR_INVALID_ARGUMENT, "bad slice (binary exponents in [-126, 127])");
	}
	int n_dev = 0;
	if (hipGetDeviceCount(&n_dev) != hipSuccess || device < 0 || device >= n_dev)
		return fail(RT_ERR_NO_DEVICE, "no such HIP device");
	HIP_TRY(hipSetDevice(device));
	// one allocation: the counters, then the operands, or the exponents and the denominator list
	const uint64_t n_den = slice && slice->denominators ? slice->n_denominators : 0, n_exp = slice ? 2 * slice->n_exponent_pairs : 0;
	const size_t tail_bytes = operands ? (size_t)n_operand_pairs * 2 * sizeof(float) : (size_t)(n_exp + n_den) * sizeof(uint32_t);
	unsigned long long host[kDivCounts] = {};
	for (int k = 0; k < RT_DIV_FORMS; ++k)
		host[kDivCountFirst + k] = ~0ull;
	unsigned long long *d = nullptr;
	HIP_TRY(hipMalloc(reinterpret_cast<void **>(&d), sizeof host + tail_bytes));
	hipError_t e = hipMemcpy(d, host, sizeof host, hipMemcpyHostToDevice);
	if (operands) {
		float *d_pairs = reinterpret_cast<float *>(d + kDivCounts);
		if (e == hipSuccess)
			e = hipMemcpy(d_pairs, operands, tail_bytes, hipMemcpyHostToDevice);
		if (e == hipSuccess)
			e = launch_div_sites(nullptr, d_pairs, n_operand_pairs, d);
	} else {
		int32_t *d_exp = reinterpret_cast<int32_t *>(d + kDivCounts);
		uint32_t *d_den = reinterpret_cast<uint32_t *>(d_exp + n_exp);
		if (e == hipSuccess)
			e = hipMemcpy(d_exp, slice->exponents, n_exp * sizeof(int32_t), hipMemcpyHostToDevice);
		if (e == hipSuccess && n_den)
			e = hipMemcpy(d_den, slice->denominators, n_den * sizeof(uint32_t), hipMemcpyHostToDevice);
		DevDivForms D;
		D.denominators = n_den ? d_den : nullptr;
		D.n_denominators = (uint32_t)slice->n_denominators;
		D.first_denominator = slice->first_denominator;
		D.exponents = d_exp;
		D.n_exponent_pairs = (uint32_t)slice->n_exponent_pairs;
		D.counts = d;
		if (e == hipSuccess)
			e = launch_div_forms(nullptr, D);
	}
	if (e == hipSuccess)
		e = hipMemcpy(host, d, sizeof host, hipMemcpyDeviceToHost);
	(void)hipFree(d);
	if (e != hipSuccess)
		return hip_fail(e, "selftest_div_forms");
	std::memset(out, 0, sizeof *out);
	out->tested = host[kDivCountTested];
	for (int k = 0; k < RT_DIV_FORMS; ++k) {
		out->mismatches[k] = host[kDivCountBad + k];
		if (slice && out->mismatches[k]) { // the first index back to its operands
			const unsigned long long index = host[kDivCountFirst + k];
			const uint64_t pair_index = index >> 23, ep = pair_index / slice->n_denominators, j = pair_index - ep * slice->n_denominators;
			const uint32_t d_sig = (slice->denominators ? slice->denominators[j] : slice->first_denominator + (uint32_t)j) & 0x007FFFFFu;
			out->first_numerator[k] = (uint32_t)(127 + slice->exponents[2 * ep]) << 23 | ((uint32_t)index & 0x007FFFFFu);
			out->first_denominator[k] = (uint32_t)(127 + slice->exponents[2 * ep + 1]) << 23 | d_sig;
		}
	}
	out->site_tested = host[kDivCountSiteTested];
	out->site_in_domain = host[kDivCountSiteInDomain];
	for (int k = 0; k < RT_DIV_SITES; ++k)
		out->site_mismatches[k] = host[kDivCountSiteBad + k];
	out->in_use = div_forms_in_use();
	return RT_OK;
}

int rt_selftest_sky_pdf_forms(rt_scene *s, const float *dirs, uint64_t m, float *out_pdf_pair, float *out_pdf_default)
{
	if (!s || !dirs || !out_pdf_pair || !out_pdf_default || m == 0 || m > (1ull << 24))
		return fail(RT_ERR_INVALID_ARGUMENT, "bad arguments (1 to 2^24 directions)");
	if ((s->host.sky.sampler_res_x | s->host.sky.sampler_res_y) == 0u)
		return fail(RT_ERR_INVALID_ARGUMENT, "the sky is not samplable (sampler_res 0 x 0)");
	if (int rc = need_device(s); rc != RT_OK)
		return rc;
	HIP_TRY(hipSetDevice(s->device));
	float *d = nullptr; // directions, then both results
	HIP_TRY(hipMalloc(reinterpret_cast<void **>(&d), 5 * m * sizeof(float)));
	hipError_t e = hipMemcpyAsync(d, dirs, 3 * m * sizeof(float), hipMemcpyHostToDevice, s->stream);
	if (e == hipSuccess)
		e = launch_sky_pdf_forms(s->stream, s->dev, d, m, d + 3 * m, d + 4 * m);
	if (e == hipSuccess)
		e = hipMemcpyAsync(out_pdf_pair, d + 3 * m, m * sizeof(float), hipMemcpyDeviceToHost, s->stream);
	if (e == hipSuccess)
		e = hipMemcpyAsync(out_pdf_default, d + 4 * m, m * sizeof(float), hipMemcpyDeviceToHost, s->stream);
	const hipError_t e_sync = hipStreamSynchronize(s->stream);
	if (e == hipSuccess)
		e = e_sync;
	(void)hipFree(d);
	if (e != hipSuccess)
		return hip_fail(e, "selftest_sky_pdf_forms");
	return RT_OK;
}

// rt_selftest_pair_shadow / _walk: the caller's cases up, one launch, the counters down
static int run_pair_shadow_cases(int device, const float *cases, uint64_t n_cases, size_t case_floats, uint64_t *counts, int n_counts,
                                 hipError_t (*launch)(hipStream_t, const float *, uint64_t, unsigned long long *), const char *what)
{
	if (!cases || !counts || n_cases == 0 || n_cases > (1ull << 22))
		return fail(RT_ERR_INVALID_ARGUMENT, "bad arguments (1 to 2^22 cases)");
	int n_dev = 0;
	if (hipGetDeviceCount(&n_dev) != hipSuccess || device < 0 || device >= n_dev)
		return fail(RT_ERR_NO_DEVICE, "no such HIP device");
	HIP_TRY(hipSetDevice(device));
	// one allocation: the counters, then the cases
	constexpr int kMaxCounts = 8;
	static_assert(RT_PAIR_SHADOW_COUNTS <= kMaxCounts && RT_PAIR_SHADOW_WALK_COUNTS <= kMaxCounts && RT_FRAME_FORMS_COUNTS <= kMaxCounts, "counters");
	unsigned long long host[kMaxCounts] = {};
	const size_t case_bytes = (size_t)n_cases * case_floats * sizeof(float);
	unsigned long long *d = nullptr;
	HIP_TRY(hipMalloc(reinterpret_cast<void **>(&d), sizeof host + case_bytes));
	float *d_cases = reinterpret_cast<float *>(d + kMaxCounts);
	hipError_t e = hipMemcpy(d, host, sizeof host, hipMemcpyHostToDevice);
	if (e == hipSuccess)
		e = hipMemcpy(d_cases, cases, case_bytes, hipMemcpyHostToDevice);
	if (e == hipSuccess)
		e = launch(nullptr, d_cases, n_cases, d);
	if (e == hipSuccess)
		e = hipMemcpy(host, d, sizeof host, hipMemcpyDeviceToHost);
	(void)hipFree(d);
	if (e != hipSuccess)
		return hip_fail(e, what);
	for (int k = 0; k < n_counts; ++k)
		counts[k] = host[k];
	return RT_OK;
}
int rt_selftest_pair_shadow(int device, const float *cases, uint64_t n_cases, uint64_t counts[RT_PAIR_SHADOW_COUNTS])
{
	return run_pair_shadow_cases(device, cases, n_cases, RT_PAIR_SHADOW_CASE_FLOATS, counts, RT_PAIR_SHADOW_COUNTS, launch_pair_shadow, "selftest_pair_shadow");
}
int rt_selftest_pair_shadow_walk(int device, const float *cases, uint64_t n_cases, uint64_t counts[RT_PAIR_SHADOW_WALK_COUNTS])
{
	return run_pair_shadow_cases(device, cases, n_cases, RT_PAIR_SHADOW_WALK_CASE_FLOATS, counts, RT_PAIR_SHADOW_WALK_COUNTS, launch_pair_shadow_walk,
	                             "selftest_pair_shadow_walk");
}
// rt_selftest_frame_forms: the same plumbing, three floats a vector; the switches' report is the host's to fill
int rt_selftest_frame_forms(int device, const float *vectors, uint64_t n_vectors, uint64_t counts[RT_FRAME_FORMS_COUNTS])
{
	const int rc = run_pair_shadow_cases(device, vectors, n_vectors, 3, counts, RT_FRAME_FORMS_COUNTS, launch_frame_forms, "selftest_frame_forms");
	if (rc == RT_OK)
		counts[RT_FRAME_FORMS_IN_USE] = frame_forms_in_use();
	return rc;
}

// rt_selftest_gen_keys: the cases up, one launch on the key table of `seed`, the counters down
int rt_selftest_gen_keys(int device, uint64_t seed, const uint32_t *cases, uint64_t n_cases, uint64_t counts[RT_GEN_KEYS_COUNTS])
{
	if (!cases || !counts || n_cases == 0 || n_cases > (1ull << 22))
		return fail(RT_ERR_INVALID_ARGUMENT, "bad arguments (1 to 2^22 cases)");
	int n_dev = 0;
	if (hipGetDeviceCount(&n_dev) != hipSuccess || device < 0 || device >= n_dev)
		return fail(RT_ERR_NO_DEVICE, "no such HIP device");
	HIP_TRY(hipSetDevice(device));
	// one allocation: the counters, then the cases
	unsigned long long host[RT_GEN_KEYS_COUNTS] = {};
	const size_t case_bytes = (size_t)n_cases * RT_GEN_KEYS_CASE_WORDS * sizeof(uint32_t);
	unsigned long long *d = nullptr;
	HIP_TRY(hipMalloc(reinterpret_cast<void **>(&d), sizeof host + case_bytes));
	uint32_t *d_cases = reinterpret_cast<uint32_t *>(d + RT_GEN_KEYS_COUNTS);
	hipError_t e = hipMemcpy(d, host, sizeof host, hipMemcpyHostToDevice);
	if (e == hipSuccess)
		e = hipMemcpy(d_cases, cases, case_bytes, hipMemcpyHostToDevice);
	if (e == hipSuccess)
		e = launch_gen_keys(nullptr, seed, d_cases, n_cases, d);
	if (e == hipSuccess)
		e = hipMemcpy(host, d, sizeof host, hipMemcpyDeviceToHost);
	(void)hipFree(d);
	if (e != hipSuccess)
		return hip_fail(e, "selftest_gen_keys");
	for (int k = 0; k < RT_GEN_KEYS_COUNTS; ++k)
		counts[k] = host[k];
	counts[RT_GEN_KEYS_IN_USE] = gen_keys_in_use();
	return RT_OK;
}

void rt_philox_round_keys(uint64_t seed, uint32_t keys[20])
{
	if (!keys)
		return;
	DevGenKeys K;
	philox_round_keys(seed, K);
	for (int r = 0; r < 10; ++r) {
		keys[2 * r] = K.key[r][0];
		keys[2 * r + 1] = K.key[r][1];
	}
}

int rt_selftest_pair_primary(rt_scene *s, const float origin[3], uint32_t *valid, uint64_t *mismatches)
{
	if (!s || !origin || !valid || !mismatches)
		return fail(RT_ERR_INVALID_ARGUMENT, "null argument");
	if (int rc = need_device(s); rc != RT_OK)
		return rc;
	if (!s->pair_tree)
		return fail(RT_ERR_UNSUPPORTED, "not a scene the two-sphere kernels take");
	HIP_TRY(hipSetDevice(s->device));
	DevPairPrimary host{};
	pair_primary_terms(s->pair, s->dev.root_min, s->dev.root_max, v3(origin[0], origin[1], origin[2]), host);
	unsigned long long *d = nullptr, bad = 0;
	HIP_TRY(hipMalloc(reinterpret_cast<void **>(&d), sizeof *d));
	hipError_t e = launch_selftest_pair_primary(nullptr, s->pair, s->dev.root_min, s->dev.root_max, origin, host, d);
	if (e == hipSuccess)
		e = hipMemcpy(&bad, d, sizeof bad, hipMemcpyDeviceToHost);
	(void)hipFree(d);
	if (e != hipSuccess)
		return hip_fail(e, "selftest_pair_primary");
	*valid = host.valid;
	*mismatches = bad;
	return RT_OK;
}

} // extern "C"
