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

// ---- what the self-tests share: cases up, one launch, counters down ----
// On `device`: ONE allocation of the n_words counters -- they start as `counts` holds them: zeros, all ones in a first-index slot --
// with the case_bytes of `cases` behind them (none: nothing goes up); launch(d_counts, d_cases) on the null stream; the counters
// back into `counts`.  The caller has checked its arguments: the device is looked at here, last.
template <class Launch>
static int run_cases(int device, const void *cases, size_t case_bytes, unsigned long long *counts, size_t n_words, const char *what, Launch launch)
{
	int n_dev = 0;
	if (hipGetDeviceCount(&n_dev) != hipSuccess || device < 0 || device >= n_dev)
		return fail(RT_ERR_NO_DEVICE, "no such HIP device");
	HIP_TRY(hipSetDevice(device));
	unsigned long long *d = nullptr;
	HIP_TRY(hipMalloc(reinterpret_cast<void **>(&d), n_words * sizeof *d + case_bytes));
	void *d_cases = d + n_words;
	hipError_t e = hipMemcpy(d, counts, n_words * sizeof *d, hipMemcpyHostToDevice);
	if (e == hipSuccess && case_bytes)
		e = hipMemcpy(d_cases, cases, case_bytes, hipMemcpyHostToDevice);
	if (e == hipSuccess)
		e = launch(d, d_cases);
	if (e == hipSuccess)
		e = hipMemcpy(counts, d, n_words * sizeof *d, hipMemcpyDeviceToHost);
	(void)hipFree(d);
	if (e != hipSuccess)
		return hip_fail(e, what);
	return RT_OK;
}

// the self-tests that take a table of 1 to 2^22 cases of `case_size` bytes and answer N counters, all from zero
template <int N, class Case, class Launch>
static int run_case_table(int device, const Case *cases, uint64_t n_cases, size_t case_size, uint64_t *counts, const char *what, Launch launch)
{
	if (!cases || !counts || n_cases == 0 || n_cases > (1ull << 22))
		return fail(RT_ERR_INVALID_ARGUMENT, "bad arguments (1 to 2^22 cases)");
	unsigned long long host[N] = {};
	RT_TRY(run_cases(device, cases, (size_t)n_cases * case_size, host, N, what, [&](unsigned long long *d_counts, void *d_cases) {
		return launch(nullptr, static_cast<const Case *>(d_cases), n_cases, d_counts);
	}));
	std::copy(host, host + N, counts);
	return RT_OK;
}

// the two self-tests on a scene's stream: a device buffer of their own carved by `L` (freed by sky_finish), copies through Staging
static int sky_buffer(rt_scene *s, Layout &L)
{
	HIP_TRY(hipSetDevice(s->device));
	HIP_TRY(hipMalloc(reinterpret_cast<void **>(&L.base), L.total()));
	return RT_OK;
}
static int sky_finish(Staging &st, Layout &L, const char *what)
{
	const int rc = st.finish(what);
	(void)hipFree(L.base);
	return rc;
}

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
	// directions and pdfs of the samples, then the caller's directions and their pdfs (a part of no elements is absent: NULL)
	Layout L;
	const auto p_out_dirs = L.add<float>(3 * n), p_out_pdf_s = L.add<float>(n), p_dirs = L.add<float>(3 * m), p_out_pdf = L.add<float>(m);
	RT_TRY(sky_buffer(s, L));
	DevSkySelftest P;
	P.seed = seed;
	P.n = n;
	P.m = m;
	P.out_dirs = L.at(p_out_dirs);
	P.out_pdf_s = L.at(p_out_pdf_s);
	P.dirs = L.at(p_dirs);
	P.out_pdf = L.at(p_out_pdf);
	Staging st{s};
	st.put(L, p_dirs, dirs);
	if (st.ok())
		st.e = launch_sky_selftest(tables_in_lds != 0, s->stream, s->dev, P);
	st.get(out_dirs, L, p_out_dirs);
	st.get(out_pdf_of_sample, L, p_out_pdf_s);
	st.get(out_pdf, L, p_out_pdf);
	return sky_finish(st, L, "selftest_sky");
}

int rt_selftest_lean(int device, uint64_t n_per_thread, uint64_t seed, uint64_t mismatches[RT_SELFTEST_LEAN_CLASSES])
{
	if (!mismatches || n_per_thread == 0 || n_per_thread > (1ull << 20))
		return fail(RT_ERR_INVALID_ARGUMENT, "bad arguments (n_per_thread in [1, 2^20])");
	unsigned long long host[RT_SELFTEST_LEAN_CLASSES] = {};
	RT_TRY(run_cases(device, nullptr, 0, host, RT_SELFTEST_LEAN_CLASSES, "selftest",
	                 [&](unsigned long long *d, void *) { return launch_selftest_lean(nullptr, 1024u, n_per_thread, seed, d); }));
	std::copy(host, host + RT_SELFTEST_LEAN_CLASSES, mismatches);
	return RT_OK;
}

int rt_selftest_short_forms(int device, const float *operands, uint64_t n_operands, rt_short_forms_result *out)
{
	if (!out || (operands && (n_operands == 0 || n_operands > (1ull << 20))) || (!operands && n_operands != 0))
		return fail(RT_ERR_INVALID_ARGUMENT, "bad arguments (operands NULL with n_operands 0, or 1 to 2^20 operands)");
	// the counters in the order of DevShortForms, the first indices all ones
	constexpr size_t kWords = 2 + RT_SHORT_FORMS + RT_SHORT_FORMS + 4 + 1 + RT_SHORT_SITES;
	unsigned long long host[kWords] = {};
	for (int k = 0; k < RT_SHORT_FORMS; ++k)
		host[2 + RT_SHORT_FORMS + k] = ~0ull;
	RT_TRY(run_cases(device, operands, (size_t)n_operands * sizeof(float), host, kWords, "selftest_short_forms", [&](unsigned long long *d, void *d_operands) {
		DevShortForms D;
		D.tested = d;
		D.mismatches = D.tested + 2;
		D.first_index = D.mismatches + RT_SHORT_FORMS;
		D.sqrt_raw = D.first_index + RT_SHORT_FORMS;
		D.site_tested = D.sqrt_raw + 4;
		D.site_mismatches = D.site_tested + 1;
		return launch_short_forms(nullptr, D, operands ? static_cast<const float *>(d_operands) : nullptr, n_operands);
	}));
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
	unsigned long long host[kDivCounts] = {};
	for (int k = 0; k < RT_DIV_FORMS; ++k)
		host[kDivCountFirst + k] = ~0ull;
	if (operands) {
		RT_TRY(run_cases(device, operands, (size_t)n_operand_pairs * 2 * sizeof(float), host, kDivCounts, "selftest_div_forms",
		                 [&](unsigned long long *d, void *d_pairs) { return launch_div_sites(nullptr, static_cast<const float *>(d_pairs), n_operand_pairs, d); }));
	} else {
		// behind the counters: the exponents, then the denominator list if there is one
		const uint64_t n_den = slice->denominators ? slice->n_denominators : 0, n_exp = 2 * slice->n_exponent_pairs;
		std::vector<uint32_t> tail(n_exp + n_den);
		std::memcpy(tail.data(), slice->exponents, n_exp * sizeof(int32_t));
		if (n_den)
			std::memcpy(tail.data() + n_exp, slice->denominators, n_den * sizeof(uint32_t));
		RT_TRY(run_cases(device, tail.data(), tail.size() * sizeof(uint32_t), host, kDivCounts, "selftest_div_forms", [&](unsigned long long *d, void *d_tail) {
			DevDivForms D;
			D.exponents = static_cast<const int32_t *>(d_tail);
			D.n_exponent_pairs = (uint32_t)slice->n_exponent_pairs;
			D.denominators = n_den ? static_cast<const uint32_t *>(d_tail) + n_exp : nullptr;
			D.n_denominators = (uint32_t)slice->n_denominators;
			D.first_denominator = slice->first_denominator;
			D.counts = d;
			return launch_div_forms(nullptr, D);
		}));
	}
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
	Layout L; // directions, then both results
	const auto p_dirs = L.add<float>(3 * m), p_pair = L.add<float>(m), p_default = L.add<float>(m);
	RT_TRY(sky_buffer(s, L));
	Staging st{s};
	st.put(L, p_dirs, dirs);
	if (st.ok())
		st.e = launch_sky_pdf_forms(s->stream, s->dev, L.at(p_dirs), m, L.at(p_pair), L.at(p_default));
	st.get(out_pdf_pair, L, p_pair);
	st.get(out_pdf_default, L, p_default);
	return sky_finish(st, L, "selftest_sky_pdf_forms");
}

int rt_selftest_sky_cell(rt_scene *s, const uint32_t *cases, uint64_t n, uint32_t axis, uint32_t su, uint32_t sv, uint32_t *out, uint64_t counts[RT_SKY_CELL_COUNTS],
                         uint32_t guard[RT_SKY_CELL_GUARD_WORDS])
{
	if (!s || !guard || (cases && (!out || n == 0 || n > (1ull << 20))))
		return fail(RT_ERR_INVALID_ARGUMENT, "bad arguments (1 to 2^20 cases with their output, or no cases)");
	const uint32_t rx = s->host.sky.sampler_res_x, ry = s->host.sky.sampler_res_y;
	{ // the guard first: it is answered for every scene, a sky without sampler included, and alone when counts is null
		const SkyCellGuard g = sky_cell_guard(rx, ry, s->dev.sky.inv_res_ok != 0u);
		const float du = (float)g.delta_u, dv = (float)g.delta_v;
		std::memset(guard, 0, RT_SKY_CELL_GUARD_WORDS * sizeof(uint32_t));
		guard[RT_SKY_CELL_GUARD_PROVEN] = g.ok;
		guard[RT_SKY_CELL_GUARD_ENABLED] = s->sky_cell.ok;
		std::memcpy(&guard[RT_SKY_CELL_GUARD_DELTA_U], &du, 4);
		std::memcpy(&guard[RT_SKY_CELL_GUARD_DELTA_V], &dv, 4);
		guard[RT_SKY_CELL_GUARD_ROW_LO] = g.row_lo;
		guard[RT_SKY_CELL_GUARD_ROW_HI] = g.row_lo + g.row_span;
		guard[RT_SKY_CELL_GUARD_IN_USE] = sky_cell_in_use() ? 1u : 0u;
	}
	if (!counts)
		return cases ? fail(RT_ERR_INVALID_ARGUMENT, "bad arguments (cases need counts)") : RT_OK;
	if ((rx | ry) == 0u)
		return fail(RT_ERR_INVALID_ARGUMENT, "the sky is not samplable (sampler_res 0 x 0)");
	if (!cases && (axis > 1u || su >= rx || sv >= ry))
		return fail(RT_ERR_INVALID_ARGUMENT, "bad enumeration (axis 0 or 1, a cell of the table)");
	if (rx >= kSkyCellMaxRes || ry >= kSkyCellMaxRes)
		return fail(RT_ERR_UNSUPPORTED, "the cell word holds resolutions below 2^15");
	for (uint64_t i = 0; cases && i < n; ++i) {
		float r[2];
		std::memcpy(r, cases + 4 * i + 2, sizeof r);
		if (cases[4 * i] >= rx || cases[4 * i + 1] >= ry || !(r[0] >= 0.0f && r[0] < 1.0f && r[1] >= 0.0f && r[1] < 1.0f))
			return fail(RT_ERR_INVALID_ARGUMENT, "bad case (a cell of the table, jitters in [0, 1))");
	}
	if (int rc = need_device(s); rc != RT_OK)
		return rc;
	const uint64_t n_run = cases ? n : 1ull << 24;
	Layout L; // counters, then the cases and their results
	const auto p_counts = L.add<unsigned long long>(RT_SKY_CELL_COUNTS);
	const auto p_cases = L.add<uint32_t>(cases ? 4 * n : 4), p_out = L.add<uint32_t>(cases ? RT_SKY_CELL_OUT_WORDS * n : 4);
	RT_TRY(sky_buffer(s, L));
	Staging st{s};
	const unsigned long long zero[RT_SKY_CELL_COUNTS] = {};
	unsigned long long host[RT_SKY_CELL_COUNTS] = {};
	st.put(L, p_counts, zero);
	if (cases)
		st.put(L, p_cases, cases);
	if (st.ok())
		st.e = launch_sky_cell(s->stream, s->dev, s->sky_cell, cases ? L.at(p_cases) : nullptr, n_run, L.at(p_out), L.at(p_counts), axis, su, sv);
	st.get(host, L, p_counts);
	if (cases)
		st.get(out, L, p_out);
	const int rc = sky_finish(st, L, "selftest_sky_cell");
	for (int k = 0; k < RT_SKY_CELL_COUNTS; ++k)
		counts[k] = host[k];
	return rc;
}

int rt_selftest_pair_shadow(int device, const float *cases, uint64_t n_cases, uint64_t counts[RT_PAIR_SHADOW_COUNTS])
{
	return run_case_table<RT_PAIR_SHADOW_COUNTS>(device, cases, n_cases, RT_PAIR_SHADOW_CASE_FLOATS * sizeof(float), counts, "selftest_pair_shadow",
	                                             launch_pair_shadow);
}
int rt_selftest_pair_shadow_walk(int device, const float *cases, uint64_t n_cases, uint64_t counts[RT_PAIR_SHADOW_WALK_COUNTS])
{
	return run_case_table<RT_PAIR_SHADOW_WALK_COUNTS>(device, cases, n_cases, RT_PAIR_SHADOW_WALK_CASE_FLOATS * sizeof(float), counts,
	                                                  "selftest_pair_shadow_walk", launch_pair_shadow_walk);
}
// ... three floats a vector; what the switches select is the host's to fill in, here and below
int rt_selftest_frame_forms(int device, const float *vectors, uint64_t n_vectors, uint64_t counts[RT_FRAME_FORMS_COUNTS])
{
	RT_TRY(run_case_table<RT_FRAME_FORMS_COUNTS>(device, vectors, n_vectors, 3 * sizeof(float), counts, "selftest_frame_forms", launch_frame_forms));
	counts[RT_FRAME_FORMS_IN_USE] = frame_forms_in_use();
	return RT_OK;
}
// ... one launch on the key table of `seed`
int rt_selftest_gen_keys(int device, uint64_t seed, const uint32_t *cases, uint64_t n_cases, uint64_t counts[RT_GEN_KEYS_COUNTS])
{
	RT_TRY(run_case_table<RT_GEN_KEYS_COUNTS>(device, cases, n_cases, RT_GEN_KEYS_CASE_WORDS * sizeof(uint32_t), counts, "selftest_gen_keys",
	                                          [seed](hipStream_t stream, const uint32_t *d_cases, uint64_t n, unsigned long long *d_counts) {
		                                          return launch_gen_keys(stream, seed, d_cases, n, d_counts);
	                                          }));
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
	DevPairPrimary host{};
	pair_primary_terms(s->pair, s->dev.root_min, s->dev.root_max, v3(origin[0], origin[1], origin[2]), host);
	unsigned long long bad = 0; // (the kernel's one word; the scene's device, no cases)
	RT_TRY(run_cases(s->device, nullptr, 0, &bad, 1, "selftest_pair_primary", [&](unsigned long long *d, void *) {
		return launch_selftest_pair_primary(nullptr, s->pair, s->dev.root_min, s->dev.root_max, origin, host, d);
	}));
	*valid = host.valid;
	*mismatches = bad;
	return RT_OK;
}

int rt_selftest_sky_tiles(rt_scene *s, const rt_camera *camera, const rt_render_opts *o, uint8_t *out_flags, uint64_t n_tiles)
{
	if (!s || !camera || !o || !out_flags)
		return fail(RT_ERR_INVALID_ARGUMENT, "null argument");
	if (int rc = need_device(s); rc != RT_OK)
		return rc;
	if (o->width < 2 || o->height < 2 || o->width >= 65536 || o->height >= 65536)
		return fail(RT_ERR_INVALID_ARGUMENT, "width and height must be in [2, 65536)");
	const FrameTiling t = frame_tiling(o);
	if (n_tiles != (uint64_t)t.tiles_x * t.tiles_y)
		return fail(RT_ERR_INVALID_ARGUMENT, "n_tiles must be the tiles of the frame the options describe");
	std::memset(out_flags, 0, (size_t)n_tiles);
	uint32_t log2_w = 0;
	while (log2_w < 7u && (1u << log2_w) != t.tile_w)
		++log2_w;
	if (!s->pair_tree || t.tile_w * t.tile_h != 64u || log2_w >= 7u)
		return RT_OK; // not a scene, or not a tiling, whose claims are ever flagged: all zeros
	// the block as a render of this camera and size forms it (rt_api.cpp)
	const DevCamera cam = dev_camera(camera);
	DevPairPrimary primary{};
	pair_primary_terms(s->pair, s->dev.root_min, s->dev.root_max, v3(cam.origin[0], cam.origin[1], cam.origin[2]), primary);
	const DevSkyTiles block = sky_tiles_block(s, primary, cam, (uint32_t)o->width, (uint32_t)o->height, true);
	// The case runner moves 64-bit words: zeros up, the kernel's results down.  The flags are bytes, so they travel as ceil(n / 8)
	// zeroed words that the kernel fills through a byte pointer (every tile's byte is written; the padding stays zero) and that
	// are copied out as bytes below -- no byte order is involved, both sides address the same buffer by bytes.
	std::vector<unsigned long long> words((size_t)((n_tiles + 7u) / 8u), 0ull);
	RT_TRY(run_cases(s->device, nullptr, 0, words.data(), words.size(), "selftest_sky_tiles", [&](unsigned long long *d, void *) {
		return launch_sky_tiles(nullptr, block, (uint32_t)o->width, (uint32_t)o->height, log2_w, t.tiles_x, n_tiles, reinterpret_cast<uint8_t *>(d));
	}));
	std::memcpy(out_flags, words.data(), (size_t)n_tiles);
	return RT_OK;
}

} // extern "C"
