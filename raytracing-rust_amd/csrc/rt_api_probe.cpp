// rt_api_probe.cpp -- the host side of the light probes (include/rt_hip.h: rt_probe_sh[_device], rt_probe_sh_eval[_device],
// rt_probe_workspace_bytes); their kernels are rt_probe.hip.  The argument checks come in rt_render_lens' order (rt_api_lens.cpp):
// bad arguments, then what is unsupported, the device last (so that a host-only scene reports bad arguments as such); the blocking
// entries stage through the scene's d_noise buffer, as rt_render_lens does.
#include <hip/hip_runtime.h>

#include <cstring>

#include "rt_api_internal.h"
#include "rt_probe.h"

using namespace rt;

static_assert(sizeof(rt_probe_opts) == 48, "rt_probe_opts layout");

// the options alone (rt_probe_workspace_bytes checks nothing else)
static int probe_opts_check(const rt_probe_opts *o)
{
	if (o->samples_per_probe == 0)
		return fail(RT_ERR_INVALID_ARGUMENT, "probe_sh: samples_per_probe must be >= 1");
	if (o->sample_split == 0 || o->sample_split > o->samples_per_probe)
		return fail(RT_ERR_INVALID_ARGUMENT, "probe_sh: sample_split must be in [1, samples_per_probe]");
	if (o->render_method != RT_METHOD_NAIVE && o->render_method != RT_METHOD_MIS)
		return fail(RT_ERR_INVALID_ARGUMENT, "probe_sh: unknown render_method");
	if (o->convolve > 1u)
		return fail(RT_ERR_INVALID_ARGUMENT, "probe_sh: convolve must be 0 or 1");
	for (uint32_t r : o->reserved)
		if (r != 0u)
			return fail(RT_ERR_INVALID_ARGUMENT, "probe_sh: reserved must be zero");
	return RT_OK;
}

static int probe_slots_check(uint64_t n, const rt_probe_opts *o)
{
	if (n >= (1ull << 31) || n * o->sample_split >= (1ull << 31))
		return fail(RT_ERR_UNSUPPORTED, "probe_sh: probes x sample_split reaches 2^31 slots");
	return RT_OK;
}

// `workspace`: the device form's (the host form passes its own non-NULL marker)
static int probe_check(const rt_scene *s, const float *positions, uint64_t n, const rt_probe_opts *o, const float *out, const void *workspace)
{
	if (!s || !positions || !o || !out || !workspace)
		return fail(RT_ERR_INVALID_ARGUMENT, "null argument");
	RT_TRY(probe_opts_check(o));
	RT_TRY(probe_slots_check(n, o));
	if (!s->peers.empty())
		return fail(RT_ERR_UNSUPPORTED, "probe_sh: a multi-device scene is not served");
	return need_device(s);
}

// p = probe_index ? probe_index[i] : i must be below n_probes: the host form looks (check_range), the device form cannot
static int probe_eval_check(const rt_scene *s, const float *coeffs, uint64_t n, const uint32_t *index, const float *normals, uint64_t m,
                            const float *out, bool check_range)
{
	if (!s || !coeffs || !normals || !out)
		return fail(RT_ERR_INVALID_ARGUMENT, "null argument");
	if (check_range) {
		if (!index && m > n)
			return fail(RT_ERR_INVALID_ARGUMENT, "probe_sh_eval: more normals than probes and no probe_index");
		for (uint64_t i = 0; index && i < m; ++i)
			if (index[i] >= n)
				return fail(RT_ERR_INVALID_ARGUMENT, "probe_sh_eval: probe_index out of range");
	}
	if (n >= (1ull << 58) || m >= (1ull << 58)) // (the byte counts of the buffers must not wrap)
		return fail(RT_ERR_UNSUPPORTED, "probe_sh_eval: 2^58 probes or normals, or more");
	if (!s->peers.empty())
		return fail(RT_ERR_UNSUPPORTED, "probe_sh_eval: a multi-device scene is not served");
	return need_device(s);
}

extern "C" {

int rt_probe_opts_default(rt_probe_opts *out)
{
	if (!out)
		return fail(RT_ERR_INVALID_ARGUMENT, "null argument");
	std::memset(out, 0, sizeof *out);
	out->samples_per_probe = 1024;
	out->sample_split = 64;
	out->render_method = RT_METHOD_MIS;
	out->max_depth = 50;
	out->rr_threshold = 3;
	return RT_OK;
}

int rt_probe_workspace_bytes(uint64_t n_probes, const rt_probe_opts *o, uint64_t *bytes)
{
	if (!o || !bytes)
		return fail(RT_ERR_INVALID_ARGUMENT, "null argument");
	RT_TRY(probe_opts_check(o));
	RT_TRY(probe_slots_check(n_probes, o));
	*bytes = probe_workspace_bytes(n_probes, o->sample_split);
	return RT_OK;
}

int rt_probe_sh_device(rt_scene *s, const float *d_positions, uint64_t n_probes, const rt_probe_opts *o, float *d_out_coeffs, void *d_workspace,
                       uint64_t *d_rays_shot, void *hip_stream)
{
	int rc = probe_check(s, d_positions, n_probes, o, d_out_coeffs, d_workspace);
	if (rc != RT_OK)
		return rc;
	if (n_probes == 0)
		return RT_OK;
	HIP_TRY(hipSetDevice(s->device));
	bool prune = false;
	DevScene dev;
	rc = four_wave_traversal(s, &prune, &dev); // (rt_api_internal.h)
	if (rc != RT_OK)
		return rc;
	const size_t lds_bytes = four_wave_stack_lds_bytes(dev) + kProbeRecordLdsBytes;
	if (lds_bytes > s->max_lds)
		return fail(RT_ERR_UNSUPPORTED, "traversal stacks exceed the LDS of one CU");
	DevProbeParams P;
	std::memset(&P, 0, sizeof P);
	P.positions = d_positions;
	P.records = static_cast<float *>(d_workspace);
	P.out = d_out_coeffs;
	P.rays_shot = reinterpret_cast<unsigned long long *>(d_rays_shot);
	P.n_probes = (uint32_t)n_probes;
	P.samples = o->samples_per_probe;
	P.split = o->sample_split;
	const uint64_t slots = n_probes * o->sample_split;
	P.n_slots = (uint32_t)slots;
	P.seed_lo = (uint32_t)o->seed;
	P.seed_hi = (uint32_t)(o->seed >> 32);
	P.sample_begin_lo = (uint32_t)o->sample_begin;
	P.sample_begin_hi = (uint32_t)(o->sample_begin >> 32);
	P.max_depth = o->max_depth;
	P.rr_threshold = o->rr_threshold;
	P.convolve = o->convolve;
	// one lane per slot at a time
	HIP_TRY(launch_probe(o->render_method == RT_METHOD_NAIVE ? 0 : 1, prune, static_cast<hipStream_t>(hip_stream), dev, P,
	                     path_lane_groups(s, lds_bytes, kProbeWaves, (slots + 255u) / 256u)));
	return RT_OK;
}

int rt_probe_sh(rt_scene *s, const float *positions, uint64_t n_probes, const rt_probe_opts *o, float *out_coeffs, uint64_t *rays_shot)
{
	const int rc = probe_check(s, positions, n_probes, o, out_coeffs, /* no workspace of the caller's */ out_coeffs);
	if (rc != RT_OK)
		return rc;
	if (n_probes == 0)
		return RT_OK;
	HIP_TRY(hipSetDevice(s->device));
	Layout L;
	const auto p_pos = L.add<float>(3 * n_probes), p_out = L.add<float>(kProbeTerms * n_probes);
	const auto p_work = L.bytes(probe_workspace_bytes(n_probes, o->sample_split));
	RT_TRY(grow_device_buffer(s->d_noise, s->d_noise_bytes, L));
	Staging st{s};
	st.put(L, p_pos, positions);
	if (st.ok())
		st.rc = rt_probe_sh_device(s, L.at(p_pos), n_probes, o, L.at(p_out), L.at(p_work), reinterpret_cast<uint64_t *>(s->d_rays), s->stream);
	st.get(out_coeffs, L, p_out);
	st.download(rays_shot, s->d_rays, sizeof(uint64_t));
	return st.finish("probe_sh");
}

int rt_probe_sh_eval_device(rt_scene *s, const float *d_coeffs, uint64_t n_probes, const uint32_t *d_probe_index, const float *d_normals, uint64_t m,
                            float *d_out_rgb, void *hip_stream)
{
	const int rc = probe_eval_check(s, d_coeffs, n_probes, d_probe_index, d_normals, m, d_out_rgb, false);
	if (rc != RT_OK)
		return rc;
	if (m == 0)
		return RT_OK;
	HIP_TRY(hipSetDevice(s->device));
	DevProbeEvalParams P;
	P.coeffs = d_coeffs;
	P.probe_index = d_probe_index;
	P.normals = d_normals;
	P.out = d_out_rgb;
	P.n_probes = n_probes;
	P.m = m;
	HIP_TRY(launch_probe_eval(static_cast<hipStream_t>(hip_stream), P));
	return RT_OK;
}

int rt_probe_sh_eval(rt_scene *s, const float *coeffs, uint64_t n_probes, const uint32_t *probe_index, const float *normals, uint64_t m, float *out_rgb)
{
	const int rc = probe_eval_check(s, coeffs, n_probes, probe_index, normals, m, out_rgb, true);
	if (rc != RT_OK)
		return rc;
	if (m == 0)
		return RT_OK;
	HIP_TRY(hipSetDevice(s->device));
	Layout L;
	const auto p_coeffs = L.add<float>(kProbeTerms * n_probes);
	const auto p_index = L.optional<uint32_t>(probe_index, m);
	const auto p_normals = L.add<float>(3 * m), p_out = L.add<float>(3 * m);
	RT_TRY(grow_device_buffer(s->d_noise, s->d_noise_bytes, L));
	Staging st{s};
	st.put(L, p_coeffs, coeffs);
	st.put(L, p_index, probe_index);
	st.put(L, p_normals, normals);
	if (st.ok())
		st.rc = rt_probe_sh_eval_device(s, L.at(p_coeffs), n_probes, L.at(p_index), L.at(p_normals), m, L.at(p_out), s->stream);
	st.get(out_rgb, L, p_out);
	return st.finish("probe_sh_eval");
}

} // extern "C"
