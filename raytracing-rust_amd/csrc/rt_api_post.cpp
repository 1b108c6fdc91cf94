// rt_api_post.cpp -- the host side of the post-processing stages of librt_hip.so (include/rt_hip.h): first-hit and specular-chain
// AOV buffers, ID mattes, ambient occlusion, the A-Trous denoiser, noise estimates, firefly-robust frames, temporal accumulation, the depth-of-field, bloom and display stages and AOV-guided upscaling.  Each stage has its kernels in a file of
// its own (rt_aov.hip, rt_aov_chain.hip, rt_matte.hip, rt_ao.hip, rt_denoise.hip, rt_noise.hip, rt_robust.hip, rt_temporal.hip, rt_dof.hip, rt_bloom.hip, rt_display.hip, rt_upscale.hip); here are their argument checks, their _device entry points
// and the blocking wrappers that stage host buffers through scene-owned device memory: each buffer is carved by a Layout (rt_layout.h),
// so its size and every pointer into it come from one description; Staging (rt_api_internal.h) carries the copies and the status.
// The steps the one-call composites share: enqueue_guides, enqueue_denoise, render_denoised_guided; render_denoised_staged and
// render_aov_staged serve the lens cameras too (rt_api_lens.cpp; declared in rt_api_internal.h).
// Every check function ends with the device (need_device), so that a host-only scene reports bad arguments as such.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "rt_api_internal.h"
#include "rt_aov.h"
#include "rt_aov_chain.h"
#include "rt_matte.h"
#include "rt_ao.h"
#include "rt_denoise.h"
#include "rt_noise.h"
#include "rt_adaptive.h"
#include "rt_render.h"
#include "rt_robust.h"
#include "rt_temporal.h"
#include "rt_bloom.h"
#include "rt_dof.h"
#include "rt_display.h"
#include "rt_upscale.h"

using namespace rt;

// ---- first-hit AOV buffers (rt_aov.hip) ----
// what every pass over the camera rays asks of its render options (both AOV passes and the ID-matte layers)
static int aov_opts_check(const rt_render_opts *o)
{
	if (int rc = frame_sides("", o->width, o->height, 2); rc != RT_OK)
		return rc;
	if (o->width * o->height >= (1ull << 31)) // (this pass alone refuses exactly 2^31 pixels too)
		return fail(RT_ERR_UNSUPPORTED, "image larger than 2^31 pixels");
	if (o->samples_per_pixel == 0 || o->samples_per_pixel >= (1ull << 32))
		return fail(RT_ERR_INVALID_ARGUMENT, "samples_per_pixel must be in [1, 2^32)");
	if (o->output_layout != RT_LAYOUT_FRAME)
		return fail(RT_ERR_UNSUPPORTED, "AOV buffers are produced in RT_LAYOUT_FRAME only");
	if (o->shard_count != 1)
		return fail(RT_ERR_UNSUPPORTED, "AOV buffers are produced for the whole frame only (shard_count 1)");
	return RT_OK;
}

// argument checks of both entry points, the device last (so that a host-only scene reports bad arguments as such)
static int aov_check(const rt_scene *s, const rt_camera *camera, const rt_render_opts *o, const rt_aov_buffers *b, uint32_t *mask)
{
	if (!s || !camera || !o || !b)
		return fail(RT_ERR_INVALID_ARGUMENT, "null argument");
	*mask = (b->albedo ? kAovAlbedo : 0u) | (b->normal ? kAovNormal : 0u) | (b->depth ? kAovDepth : 0u) |
	        (b->coverage ? kAovCoverage : 0u) | (b->primitive ? kAovPrimitive : 0u) | (b->material ? kAovMaterial : 0u);
	if (*mask == 0u)
		return fail(RT_ERR_INVALID_ARGUMENT, "rt_aov_buffers: every channel is NULL");
	if (int rc = aov_opts_check(o); rc != RT_OK)
		return rc;
	return need_device(s);
}

// the launch parameters the AOV kernels share (rt_api_lens.cpp: the lens pass takes them too)
DevAovParams aov_params(const rt_scene *s, const rt_camera *camera, const rt_render_opts *o, const rt_aov_buffers *d_out, uint32_t mask)
{
	DevAovParams P;
	std::memset(&P, 0, sizeof P);
	P.cam = dev_camera(camera);
	P.width = (uint32_t)o->width;
	P.height = (uint32_t)o->height;
	P.tiles_x = tile_grid(o->width, o->height).tiles_x;
	P.n_tiles = (uint32_t)tile_grid(o->width, o->height).count;
	P.spp = (uint32_t)o->samples_per_pixel;
	P.mask = mask;
	P.seed_lo = (uint32_t)o->seed;
	P.seed_hi = (uint32_t)(o->seed >> 32);
	P.sample_begin_lo = (uint32_t)o->sample_begin;
	P.sample_begin_hi = (uint32_t)(o->sample_begin >> 32);
	P.prim_desc = s->d_prim_desc;
	P.albedo = d_out->albedo;
	P.normal = d_out->normal;
	P.depth = d_out->depth;
	P.coverage = d_out->coverage;
	P.primitive = d_out->primitive;
	P.material = d_out->material;
	return P;
}

extern "C" {

int rt_render_aov_device(rt_scene *s, const rt_camera *camera, const rt_render_opts *o, const rt_aov_buffers *d_out, void *hip_stream)
{
	uint32_t mask = 0;
	int rc = aov_check(s, camera, o, d_out, &mask);
	if (rc != RT_OK)
		return rc;
	// a multi-device head is an ordinary scene on devices[0]: the AOV pass runs there alone
	HIP_TRY(hipSetDevice(s->device));
	if ((mask & kAovPrimitive) && !s->d_prim_desc) // (upload_scene, rt_api.cpp, makes the table for fewer primitives)
		return fail(RT_ERR_UNSUPPORTED, "primitive IDs need fewer than 2^32 - 1 primitives");
	bool prune = false;
	DevScene dev;
	rc = four_wave_traversal(s, &prune, &dev); // (rt_api_internal.h)
	if (rc != RT_OK)
		return rc;
	const DevAovParams P = aov_params(s, camera, o, d_out, mask);
	HIP_TRY(launch_aov(prune, static_cast<hipStream_t>(hip_stream), dev, P));
	return RT_OK;
}

} // extern "C"

// The blocking AOV entry points once their arguments are checked: one device allocation per call for the requested channels, in
// rt_aov_chain_buffers order (4-byte elements throughout); `enqueue` is the entry point's _device form on s->stream
int render_aov_staged(rt_scene *s, const rt_render_opts *o, const rt_aov_buffers &a, float *bounces, const char *what,
                      const std::function<int(const rt_aov_chain_buffers &)> &enqueue)
{
	HIP_TRY(hipSetDevice(s->device));
	const uint64_t n_px = o->width * o->height;
	void *host[7] = {a.albedo, a.normal, a.depth, a.coverage, a.primitive, a.material, bounces};
	Layout L;
	Layout::Part<float> ch[7];
	for (int k = 0; k < 7; ++k)
		ch[k] = L.optional<float>(host[k], (k < 2 ? 3 : 1) * n_px);
	char *d = nullptr;
	HIP_TRY(hipMalloc(reinterpret_cast<void **>(&d), L.total()));
	L.base = d;
	auto ids = [&](int k) { return reinterpret_cast<uint32_t *>(L.at(ch[k])); };
	const rt_aov_chain_buffers dev_out = {{L.at(ch[0]), L.at(ch[1]), L.at(ch[2]), L.at(ch[3]), ids(4), ids(5)}, L.at(ch[6])};
	Staging st{s};
	st.rc = enqueue(dev_out);
	for (int k = 0; k < 7; ++k)
		st.get(host[k], L, ch[k]);
	const int rc = st.finish(what);
	(void)hipFree(d);
	return rc;
}

// the option ranges of a chain (rt_api_lens.cpp: the lens pass checks them too)
int aov_chain_opts_check(const rt_aov_chain_opts *c)
{
	if (c->max_chain > kAovChainMaxChain)
		return fail(RT_ERR_INVALID_ARGUMENT, "aov_chain: max_chain must be in 0..64");
	if (!std::isfinite(c->fuzz_limit) || !(c->fuzz_limit >= 0.0f))
		return fail(RT_ERR_INVALID_ARGUMENT, "aov_chain: fuzz_limit must be finite and >= 0");
	return RT_OK;
}

extern "C" {

int rt_render_aov(rt_scene *s, const rt_camera *camera, const rt_render_opts *o, const rt_aov_buffers *out)
{
	uint32_t mask = 0;
	const int rc = aov_check(s, camera, o, out, &mask);
	if (rc != RT_OK)
		return rc;
	return render_aov_staged(s, o, *out, nullptr, "render_aov",
	                         [&](const rt_aov_chain_buffers &d) { return rt_render_aov_device(s, camera, o, &d.aov, s->stream); });
}

// ---- specular-chain AOV buffers (rt_aov_chain.hip) ----
int rt_aov_chain_opts_default(rt_aov_chain_opts *out)
{
	if (!out)
		return fail(RT_ERR_INVALID_ARGUMENT, "null argument");
	std::memset(out, 0, sizeof *out);
	out->max_chain = 8;
	out->fuzz_limit = 0.0f;
	return RT_OK;
}

// argument checks of both chain entry points: the chain's own, then those of the first-hit pass (the device last)
static int aov_chain_check(const rt_scene *s, const rt_camera *camera, const rt_render_opts *o, const rt_aov_chain_opts *c,
                           const rt_aov_chain_buffers *b, uint32_t *mask)
{
	if (!s || !camera || !o || !c || !b)
		return fail(RT_ERR_INVALID_ARGUMENT, "null argument");
	if (int rc = aov_chain_opts_check(c); rc != RT_OK)
		return rc;
	// (a `bounces` pointer stands in for "some channel is given" in the first-hit check)
	rt_aov_buffers any = b->aov;
	if (b->bounces && !any.albedo)
		any.albedo = b->bounces;
	const int rc = aov_check(s, camera, o, &any, mask);
	*mask = (*mask & ~(b->aov.albedo ? 0u : kAovAlbedo)) | (b->bounces ? kAovBounces : 0u);
	return rc;
}

int rt_render_aov_chain_device(rt_scene *s, const rt_camera *camera, const rt_render_opts *o, const rt_aov_chain_opts *c,
                               const rt_aov_chain_buffers *d_out, void *hip_stream)
{
	uint32_t mask = 0;
	int rc = aov_chain_check(s, camera, o, c, d_out, &mask);
	if (rc != RT_OK)
		return rc;
	// a multi-device head is an ordinary scene on devices[0]: the pass runs there alone
	HIP_TRY(hipSetDevice(s->device));
	if ((mask & kAovPrimitive) && !s->d_prim_desc)
		return fail(RT_ERR_UNSUPPORTED, "primitive IDs need fewer than 2^32 - 1 primitives");
	bool prune = false;
	DevScene dev;
	rc = four_wave_traversal(s, &prune, &dev); // (rt_api_internal.h)
	if (rc != RT_OK)
		return rc;
	DevAovChainParams P;
	std::memset(&P, 0, sizeof P);
	P.A = aov_params(s, camera, o, &d_out->aov, mask);
	P.max_chain = c->max_chain;
	P.fuzz_limit = c->fuzz_limit;
	P.bounces = d_out->bounces;
	HIP_TRY(launch_aov_chain(prune, static_cast<hipStream_t>(hip_stream), dev, P));
	return RT_OK;
}

int rt_render_aov_chain(rt_scene *s, const rt_camera *camera, const rt_render_opts *o, const rt_aov_chain_opts *c,
                        const rt_aov_chain_buffers *out)
{
	uint32_t mask = 0;
	const int rc = aov_chain_check(s, camera, o, c, out, &mask);
	if (rc != RT_OK)
		return rc;
	return render_aov_staged(s, o, out->aov, out->bounces, "render_aov_chain",
	                         [&](const rt_aov_chain_buffers &d) { return rt_render_aov_chain_device(s, camera, o, c, &d, s->stream); });
}

} // extern "C"

// ---- anti-aliased ID mattes (rt_matte.hip) ----
// argument checks of rt_render_matte(_device): the matte's own, then those of the first-hit pass, the device last
static int matte_check(const rt_scene *s, const rt_camera *camera, const rt_render_opts *o, const rt_matte_opts *m, const rt_matte_buffers *b)
{
	if (!s || !camera || !o || !m || !b)
		return fail(RT_ERR_INVALID_ARGUMENT, "null argument");
	if (!b->ids || !b->coverage)
		return fail(RT_ERR_INVALID_ARGUMENT, "matte: ids and coverage must not be NULL");
	if (m->layers < 1 || m->layers > kMatteSlots)
		return fail(RT_ERR_INVALID_ARGUMENT, "matte: layers must be in 1..8");
	if (m->id_kind != RT_MATTE_ID_PRIMITIVE && m->id_kind != RT_MATTE_ID_MATERIAL)
		return fail(RT_ERR_INVALID_ARGUMENT, "matte: unknown id_kind");
	for (uint32_t r : m->reserved)
		if (r != 0u)
			return fail(RT_ERR_INVALID_ARGUMENT, "matte: reserved must be zero");
	int rc = aov_opts_check(o);
	if (rc != RT_OK)
		return rc;
	const uint64_t n = o->width * o->height;
	const void *buf[3] = {b->ids, b->coverage, b->residual};
	const uint64_t bytes[3] = {4 * m->layers * n, 4 * m->layers * n, 4 * n};
	rc = check_disjoint("matte: two output buffers overlap", buf, bytes, 3, 3);
	return rc == RT_OK ? need_device(s) : rc;
}

// argument checks of rt_matte_extract(_device), the device last
static int matte_extract_check(const rt_scene *s, const rt_matte_buffers *b, uint64_t w, uint64_t h, uint32_t layers, const uint32_t *ids,
                               uint64_t n_ids, const float *out)
{
	if (!s || !b)
		return fail(RT_ERR_INVALID_ARGUMENT, "null argument");
	if (!b->ids || !b->coverage || !out)
		return fail(RT_ERR_INVALID_ARGUMENT, "matte_extract: ids, coverage and out must not be NULL");
	if (n_ids != 0 && !ids)
		return fail(RT_ERR_INVALID_ARGUMENT, "matte_extract: a NULL selection with n_ids > 0");
	if (int rc = frame_sides("matte_extract: ", w, h, 1); rc != RT_OK)
		return rc;
	if (layers < 1 || layers > kMatteSlots)
		return fail(RT_ERR_INVALID_ARGUMENT, "matte_extract: layers must be in 1..8");
	if (n_ids > kMatteMaxIds)
		return fail(RT_ERR_UNSUPPORTED, "matte_extract: more than 2^20 selected IDs");
	uint64_t n = 0;
	int rc = frame_pixels("matte_extract: ", w, h, 1, &n);
	if (rc != RT_OK)
		return rc;
	const void *buf[4] = {out, b->ids, b->coverage, ids};
	const uint64_t bytes[4] = {4 * n, 4 * layers * n, 4 * layers * n, 4 * n_ids};
	rc = check_disjoint("matte_extract: out overlaps the layers or the selection", buf, bytes, 1, 4);
	return rc == RT_OK ? need_device(s) : rc;
}

extern "C" {

int rt_matte_opts_default(rt_matte_opts *out)
{
	if (!out)
		return fail(RT_ERR_INVALID_ARGUMENT, "null argument");
	std::memset(out, 0, sizeof *out);
	out->id_kind = RT_MATTE_ID_MATERIAL;
	out->layers = 4;
	return RT_OK;
}

int rt_render_matte_device(rt_scene *s, const rt_camera *camera, const rt_render_opts *o, const rt_matte_opts *m,
                           const rt_matte_buffers *d_out, void *hip_stream)
{
	int rc = matte_check(s, camera, o, m, d_out);
	if (rc != RT_OK)
		return rc;
	// a multi-device head is an ordinary scene on devices[0]: the pass runs there alone
	HIP_TRY(hipSetDevice(s->device));
	if (m->id_kind == RT_MATTE_ID_PRIMITIVE && !s->d_prim_desc) // (upload_scene, rt_api.cpp, makes the table for fewer primitives)
		return fail(RT_ERR_UNSUPPORTED, "primitive IDs need fewer than 2^32 - 1 primitives");
	bool prune = false;
	DevScene dev;
	rc = four_wave_traversal(s, &prune, &dev); // (rt_api_internal.h)
	if (rc != RT_OK)
		return rc;
	const rt_aov_buffers no_channels = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
	DevMatteParams P;
	std::memset(&P, 0, sizeof P);
	P.A = aov_params(s, camera, o, &no_channels, 0u);
	P.id_kind = (uint32_t)m->id_kind;
	P.layers = m->layers;
	P.ids = d_out->ids;
	P.coverage = d_out->coverage;
	P.residual = d_out->residual;
	HIP_TRY(launch_matte(prune, static_cast<hipStream_t>(hip_stream), dev, P));
	return RT_OK;
}

int rt_render_matte(rt_scene *s, const rt_camera *camera, const rt_render_opts *o, const rt_matte_opts *m, const rt_matte_buffers *out)
{
	int rc = matte_check(s, camera, o, m, out);
	if (rc != RT_OK)
		return rc;
	HIP_TRY(hipSetDevice(s->device));
	// ids, coverage, then the residual if asked for; 4-byte elements throughout
	const uint64_t n = o->width * o->height;
	Layout L;
	const auto p_ids = L.add<uint32_t>(m->layers * n);
	const auto p_coverage = L.add<float>(m->layers * n), p_residual = L.optional<float>(out->residual, n);
	RT_TRY(grow_device_buffer(s->d_denoise, s->d_denoise_bytes, L)); // shared with rt_denoise / rt_render_denoised
	const rt_matte_buffers d_out = {L.at(p_ids), L.at(p_coverage), L.at(p_residual)};
	Staging st{s};
	st.rc = rt_render_matte_device(s, camera, o, m, &d_out, s->stream);
	st.get(out->ids, L, p_ids);
	st.get(out->coverage, L, p_coverage);
	st.get(out->residual, L, p_residual);
	return st.finish("render_matte");
}

int rt_matte_extract_device(rt_scene *s, const rt_matte_buffers *d_layers, uint32_t width, uint32_t height, uint32_t layers,
                            const uint32_t *d_sorted_ids, uint64_t n_ids, float *d_out, void *hip_stream)
{
	int rc = matte_extract_check(s, d_layers, width, height, layers, d_sorted_ids, n_ids, d_out);
	if (rc != RT_OK)
		return rc;
	HIP_TRY(hipSetDevice(s->device)); // a multi-device head runs on devices[0]
	DevMatteExtractParams P;
	std::memset(&P, 0, sizeof P);
	P.ids = d_layers->ids;
	P.coverage = d_layers->coverage;
	P.sel = d_sorted_ids;
	P.n_sel = (uint32_t)n_ids;
	P.layers = layers;
	P.n_px = (uint32_t)((uint64_t)width * height);
	P.out = d_out;
	HIP_TRY(launch_matte_extract(static_cast<hipStream_t>(hip_stream), P));
	return RT_OK;
}

int rt_matte_extract(rt_scene *s, const rt_matte_buffers *layers_in, uint32_t width, uint32_t height, uint32_t layers, const uint32_t *ids,
                     uint64_t n_ids, float *out)
{
	int rc = matte_extract_check(s, layers_in, width, height, layers, ids, n_ids, out);
	if (rc != RT_OK)
		return rc;
	HIP_TRY(hipSetDevice(s->device));
	std::vector<uint32_t> sorted(ids, ids + n_ids); // the caller's selection in any order, duplicates and all
	std::sort(sorted.begin(), sorted.end());
	const uint64_t n = (uint64_t)width * height;
	// out first, then the layers and the sorted selection
	Layout L;
	const auto p_out = L.add<float>(n), p_coverage = L.add<float>(layers * n);
	const auto p_ids = L.add<uint32_t>(layers * n), p_sel = L.add<uint32_t>(sorted.size());
	RT_TRY(grow_device_buffer(s->d_denoise, s->d_denoise_bytes, L)); // shared with rt_denoise / rt_render_denoised
	Staging st{s};
	st.put(L, p_ids, layers_in->ids);
	st.put(L, p_coverage, layers_in->coverage);
	st.put(L, p_sel, sorted.data());
	if (!st.ok())
		return st.finish("matte_extract upload");
	const rt_matte_buffers d_layers = {L.at(p_ids), L.at(p_coverage), nullptr};
	st.rc = rt_matte_extract_device(s, &d_layers, width, height, layers, L.at(p_sel), n_ids, L.at(p_out), s->stream);
	st.get(out, L, p_out);
	return st.finish("matte_extract");
}

} // extern "C"

// ---- ambient occlusion (rt_ao.hip) ----
// argument checks of rt_render_ao(_device): the pass's own, then those of the first-hit pass, the device last
static int ao_check(const rt_scene *s, const rt_camera *camera, const rt_render_opts *o, const rt_ao_opts *a, const rt_ao_buffers *b)
{
	if (!s || !camera || !o || !a || !b)
		return fail(RT_ERR_INVALID_ARGUMENT, "null argument");
	if (!b->visibility && !b->bent_normal)
		return fail(RT_ERR_INVALID_ARGUMENT, "rt_ao_buffers: every channel is NULL");
	if (a->rays_per_pass < 1 || a->rays_per_pass > kAoMaxRays)
		return fail(RT_ERR_INVALID_ARGUMENT, "ao: rays_per_pass must be in 1..64");
	if (!(a->radius >= 0.0f)) // (a NaN too)
		return fail(RT_ERR_INVALID_ARGUMENT, "ao: radius must be >= 0 (0: no limit)");
	for (uint32_t r : a->reserved)
		if (r != 0u)
			return fail(RT_ERR_INVALID_ARGUMENT, "ao: reserved must be zero");
	int rc = aov_opts_check(o);
	if (rc != RT_OK)
		return rc;
	if (o->samples_per_pixel * a->rays_per_pass >= (1ull << 32)) // (the ray counts of a pixel are 32-bit)
		return fail(RT_ERR_INVALID_ARGUMENT, "ao: samples_per_pixel * rays_per_pass must be below 2^32");
	uint64_t n = 0;
	rc = frame_pixels("", o->width, o->height, 2, &n);
	if (rc != RT_OK)
		return rc;
	const void *buf[2] = {b->visibility, b->bent_normal};
	const uint64_t bytes[2] = {4 * n, 12 * n};
	rc = check_disjoint("ao: the two output buffers overlap", buf, bytes, 2, 2);
	return rc == RT_OK ? need_device(s) : rc;
}

extern "C" {

int rt_ao_opts_default(rt_ao_opts *out)
{
	if (!out)
		return fail(RT_ERR_INVALID_ARGUMENT, "null argument");
	std::memset(out, 0, sizeof *out);
	out->rays_per_pass = 4;
	out->radius = 0.0f;
	return RT_OK;
}

int rt_render_ao_device(rt_scene *s, const rt_camera *camera, const rt_render_opts *o, const rt_ao_opts *a, const rt_ao_buffers *d_out,
                        void *hip_stream)
{
	int rc = ao_check(s, camera, o, a, d_out);
	if (rc != RT_OK)
		return rc;
	// a multi-device head is an ordinary scene on devices[0]: the pass runs there alone
	HIP_TRY(hipSetDevice(s->device));
	bool prune = false;
	DevScene dev;
	rc = four_wave_traversal(s, &prune, &dev); // (rt_api_internal.h)
	if (rc != RT_OK)
		return rc;
	const rt_aov_buffers no_channels = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
	DevAoParams P;
	std::memset(&P, 0, sizeof P);
	P.A = aov_params(s, camera, o, &no_channels, 0u);
	P.rays_per_pass = a->rays_per_pass;
	P.t_limit = a->radius > 0.0f ? a->radius : std::nanf(""); // radius 0: no limit, as the sky shadow ray (rt_intersect.h trace_any)
	P.visibility = d_out->visibility;
	P.bent_normal = d_out->bent_normal;
	HIP_TRY(launch_ao(prune, static_cast<hipStream_t>(hip_stream), dev, P));
	return RT_OK;
}

int rt_render_ao(rt_scene *s, const rt_camera *camera, const rt_render_opts *o, const rt_ao_opts *a, const rt_ao_buffers *out)
{
	int rc = ao_check(s, camera, o, a, out);
	if (rc != RT_OK)
		return rc;
	HIP_TRY(hipSetDevice(s->device));
	// the visibility, then the bent normal, each if asked for; 4-byte elements throughout
	const uint64_t n = o->width * o->height;
	Layout L;
	const auto p_visibility = L.optional<float>(out->visibility, n), p_bent = L.optional<float>(out->bent_normal, 3 * n);
	RT_TRY(grow_device_buffer(s->d_denoise, s->d_denoise_bytes, L)); // shared with rt_denoise / rt_render_denoised
	const rt_ao_buffers d_out = {L.at(p_visibility), L.at(p_bent)};
	Staging st{s};
	st.rc = rt_render_ao_device(s, camera, o, a, &d_out, s->stream);
	st.get(out->visibility, L, p_visibility);
	st.get(out->bent_normal, L, p_bent);
	return st.finish("render_ao");
}

} // extern "C"

// ---- AOV-guided A-Trous denoiser (rt_denoise.hip) ----
// the frame size and the filter options (width and height are passed separately: rt_render_denoised takes them from the render)
static int denoise_opts_check(const rt_denoise_opts *d, uint64_t w, uint64_t h)
{
	if (int rc = frame_sides("denoise: ", w, h, 1); rc != RT_OK)
		return rc;
	if (d->iterations < 1 || d->iterations > 10)
		return fail(RT_ERR_INVALID_ARGUMENT, "denoise: iterations must be in 1..10");
	const float sig[3] = {d->sigma_luminance, d->sigma_normal, d->sigma_depth};
	for (float x : sig)
		if (!std::isfinite(x) || !(x > 0.0f))
			return fail(RT_ERR_INVALID_ARGUMENT, "denoise: sigma_luminance, sigma_normal and sigma_depth must be finite and > 0");
	uint64_t n = 0;
	return frame_pixels("denoise: ", w, h, 1, &n);
}

// argument checks of rt_denoise / rt_denoise_device, the device last (so that a host-only scene reports bad arguments as such);
// `ws` is checked for the device call only
static int denoise_check(const rt_scene *s, const rt_denoise_inputs *in, const rt_denoise_opts *o, const float *out, bool device,
                         const void *ws)
{
	if (!s || !in || !o)
		return fail(RT_ERR_INVALID_ARGUMENT, "null argument");
	if (!in->color || !out)
		return fail(RT_ERR_INVALID_ARGUMENT, "denoise: color and out must not be NULL");
	int rc = denoise_opts_check(o, o->width, o->height);
	if (rc != RT_OK)
		return rc;
	const uint64_t n = (uint64_t)o->width * o->height;
	// the workspace, then out, against what follows them (the inputs may share memory with one another)
	const void *buf[7] = {ws, out, in->color, in->albedo, in->normal, in->depth, in->variance};
	const uint64_t bytes[7] = {kDenoiseWorkspaceBytesPerPixel * n, 12 * n, 12 * n, 12 * n, 12 * n, 4 * n, 4 * n};
	rc = check_disjoint("denoise: out overlaps an input", buf + 1, bytes + 1, 1, 6);
	if (rc != RT_OK)
		return rc;
	if (device) {
		if (!ws || reinterpret_cast<uintptr_t>(ws) % 16u != 0u)
			return fail(RT_ERR_INVALID_ARGUMENT, "denoise: the workspace must be non-NULL and 16-byte aligned");
		rc = check_disjoint("denoise: the workspace overlaps an input or out", buf, bytes, 1, 7);
		if (rc != RT_OK)
			return rc;
	}
	return need_device(s);
}

static DevDenoiseParams denoise_params(const rt_denoise_opts *o, uint64_t w, uint64_t h, const rt_denoise_inputs &in, void *ws,
                                       float *out)
{
	DevDenoiseParams P;
	std::memset(&P, 0, sizeof P);
	P.width = (uint32_t)w;
	P.height = (uint32_t)h;
	P.iterations = o->iterations;
	P.sigma_l = o->sigma_luminance;
	P.sigma_n = o->sigma_normal;
	P.sigma_z = o->sigma_depth;
	P.color = in.color;
	P.albedo = in.albedo;
	P.normal = in.normal;
	P.depth = in.depth;
	P.variance = in.variance;
	const size_t n = (size_t)(w * h);
	P.plane0 = static_cast<float4 *>(ws);
	P.plane1 = P.plane0 + n;
	P.guide = P.plane1 + n;
	P.out = out;
	return P;
}

// what rt_render_denoised, rt_render_upscaled and rt_render_lens_denoised (rt_api_lens.cpp) ask of their render options, for a render of w x h
int render_denoised_opts_check(const char *who, const rt_render_opts *o, const rt_denoise_opts *dopts, uint64_t w, uint64_t h)
{
	int rc = denoise_opts_check(dopts, w, h);
	if (rc != RT_OK)
		return rc;
	rc = frame_sides("", w, h, 2);
	if (rc != RT_OK)
		return rc;
	if (o->samples_per_pixel < 2 || o->samples_per_pixel % 2 != 0 || o->samples_per_pixel >= (1ull << 32))
		return fail(RT_ERR_INVALID_ARGUMENT, std::string(who) + ": samples_per_pixel must be even, >= 2 and < 2^32");
	if (o->render_method != RT_METHOD_NAIVE && o->render_method != RT_METHOD_MIS)
		return fail(RT_ERR_INVALID_ARGUMENT, "unknown render method");
	if (o->output_layout != RT_LAYOUT_FRAME)
		return fail(RT_ERR_UNSUPPORTED, std::string(who) + ": RT_LAYOUT_FRAME only");
	if (o->shard_count != 1)
		return fail(RT_ERR_UNSUPPORTED, std::string(who) + ": the whole frame only (shard_count 1)");
	return RT_OK;
}

// ---- the steps the one-call composites share, on s->stream; the status goes to `st` (nothing is enqueued once it is not ok) ----
// the guide AOVs of all passes of the render `o` into device planes, any of them NULL
static void enqueue_guides(rt_scene *s, const rt_camera *camera, const rt_render_opts *o, float *d_albedo, float *d_normal, float *d_depth,
                           Staging &st)
{
	if (!st.ok())
		return;
	const rt_aov_buffers aov = {d_albedo, d_normal, d_depth, nullptr, nullptr, nullptr};
	st.rc = rt_render_aov_device(s, camera, o, &aov, s->stream);
}

// rt_denoise_device at the render's size with the caller's options
static void enqueue_denoise(rt_scene *s, const rt_render_opts *o, const rt_denoise_opts *dopts, const rt_denoise_inputs &in, void *ws,
                            float *d_clean, Staging &st)
{
	if (!st.ok())
		return;
	rt_denoise_opts d = *dopts;
	d.width = (uint32_t)o->width;
	d.height = (uint32_t)o->height;
	st.rc = rt_denoise_device(s, &in, &d, ws, d_clean, s->stream);
}

// The device side of rt_render_denoised for a render of n pixels: two ray counters, the workspace, then the frames A, B, albedo,
// normal, depth, noisy, clean.  rt_render_upscaled describes its destination-size frames behind them.
struct DenoisedParts {
	Layout::Part<unsigned long long> rays;
	Layout::Part<char> ws;
	Layout::Part<float> a, b, albedo, normal, depth, noisy, clean;
};
static DenoisedParts denoised_parts(Layout &L, uint64_t n)
{
	return DenoisedParts{L.add<unsigned long long>(2), L.bytes(kDenoiseWorkspaceBytesPerPixel * n), L.add<float>(3 * n), L.add<float>(3 * n),
	                     L.add<float>(3 * n), L.add<float>(3 * n), L.add<float>(n), L.add<float>(3 * n), L.add<float>(3 * n)}; // (in this order)
}

// rt_render_denoised's camera: the pinhole entry points on s->stream
static DenoisedSource pinhole_source(rt_scene *s, const rt_camera *camera)
{
	return DenoisedSource{
	    [=](const rt_render_opts *oh, float *d_rgb, uint64_t *d_rays) { return rt_render_device(s, camera, oh, d_rgb, d_rays, s->stream); },
	    [=](const rt_render_opts *o, const rt_aov_buffers &d_guides) { return rt_render_aov_device(s, camera, o, &d_guides, s->stream); }};
}

// two half renders, the AOVs of all passes, the variance and the filter, in the parts `P` of the grown buffer
static void enqueue_render_denoised(rt_scene *s, const DenoisedSource &src, const rt_render_opts *o, const rt_denoise_opts *dopts,
                                    const Layout &L, const DenoisedParts &P, Staging &st)
{
	uint64_t *d_rays = reinterpret_cast<uint64_t *>(L.at(P.rays));
	float *d_a = L.at(P.a), *d_b = L.at(P.b), *d_albedo = L.at(P.albedo), *d_normal = L.at(P.normal),
	      *d_depth = L.at(P.depth), *d_noisy = L.at(P.noisy);
	const uint64_t half = o->samples_per_pixel / 2;
	rt_render_opts oh = *o;
	oh.samples_per_pixel = half;
	if (st.ok())
		st.rc = src.half(&oh, d_a, d_rays);
	if (st.ok()) {
		oh.sample_begin = o->sample_begin + half;
		st.rc = src.half(&oh, d_b, d_rays + 1);
	}
	if (st.ok())
		st.e = hipSetDevice(s->device);
	if (st.ok())
		st.rc = src.guides(o, rt_aov_buffers{d_albedo, d_normal, d_depth, nullptr, nullptr, nullptr});
	if (st.ok()) {
		const rt_denoise_inputs in = {d_noisy, d_albedo, d_normal, d_depth, nullptr};
		DevDenoiseParams D = denoise_params(dopts, o->width, o->height, in, L.at(P.ws), L.at(P.clean));
		D.half_a = d_a;
		D.half_b = d_b;
		D.noisy = d_noisy;
		st.e = launch_denoise(s->stream, D);
	}
}

// What rt_render_denoised_split and rt_render_denoised_robust share once their own arguments are checked.  In the denoiser's buffer:
// the ray counter, the workspace, albedo, normal, depth, the frame the filter reads, `extra_floats` for the middle call, clean.
// Enqueued: the guides, middle(d_albedo, d_frame, d_extra, d_rays) -- the render into d_frame --, the filter (d_extra its variance
// plane if extra_is_variance), the downloads and the ray count.
template <class Middle>
static int render_denoised_guided(rt_scene *s, const rt_camera *camera, const rt_render_opts *o, const rt_denoise_opts *dopts, uint64_t px,
                                  uint64_t extra_floats, bool extra_is_variance, Middle middle, const char *what, float *out_clean,
                                  float *out_frame, float *out_extra, uint64_t *rays_shot)
{
	int rc = need_device(s);
	if (rc != RT_OK)
		return rc;
	HIP_TRY(hipSetDevice(s->device));
	Layout L;
	const auto p_rays = L.add<uint64_t>(1);
	const auto p_ws = L.bytes(kDenoiseWorkspaceBytesPerPixel * px);
	const auto p_albedo = L.add<float>(3 * px), p_normal = L.add<float>(3 * px), p_depth = L.add<float>(px), p_frame = L.add<float>(3 * px),
	           p_extra = L.add<float>(extra_floats), p_clean = L.add<float>(3 * px);
	RT_TRY(grow_device_buffer(s->d_denoise, s->d_denoise_bytes, L));
	float *d_albedo = L.at(p_albedo), *d_normal = L.at(p_normal), *d_depth = L.at(p_depth), *d_frame = L.at(p_frame),
	      *d_extra = L.at(p_extra);
	Staging st{s};
	enqueue_guides(s, camera, o, d_albedo, d_normal, d_depth, st);
	if (st.ok())
		st.rc = middle(d_albedo, d_frame, d_extra, L.at(p_rays));
	enqueue_denoise(s, o, dopts, {d_frame, d_albedo, d_normal, d_depth, extra_is_variance ? d_extra : nullptr}, L.at(p_ws),
	                L.at(p_clean), st);
	uint64_t rays = 0;
	st.get(out_clean, L, p_clean);
	st.get(out_frame, L, p_frame);
	st.get(out_extra, L, p_extra);
	st.get(&rays, L, p_rays);
	rc = st.finish(what);
	if (rc == RT_OK && rays_shot)
		*rays_shot = rays;
	return rc;
}

extern "C" {

int rt_denoise_opts_default(rt_denoise_opts *out)
{
	if (!out)
		return fail(RT_ERR_INVALID_ARGUMENT, "null argument");
	std::memset(out, 0, sizeof *out);
	out->iterations = 5;
	out->sigma_luminance = 4.0f;
	out->sigma_normal = 128.0f;
	out->sigma_depth = 0.1f;
	return RT_OK;
}

int rt_denoise_workspace_bytes(const rt_denoise_opts *o, uint64_t *bytes)
{
	if (!o || !bytes)
		return fail(RT_ERR_INVALID_ARGUMENT, "null argument");
	uint64_t n = 0;
	const int rc = frame_pixels("denoise: ", o->width, o->height, 1, &n);
	if (rc == RT_OK)
		*bytes = kDenoiseWorkspaceBytesPerPixel * n;
	return rc;
}

int rt_denoise_device(rt_scene *s, const rt_denoise_inputs *d_in, const rt_denoise_opts *o, void *d_workspace, float *d_out,
                      void *hip_stream)
{
	int rc = denoise_check(s, d_in, o, d_out, true, d_workspace);
	if (rc != RT_OK)
		return rc;
	// a multi-device head is an ordinary scene on devices[0]: the filter runs there alone
	HIP_TRY(hipSetDevice(s->device));
	HIP_TRY(launch_denoise(static_cast<hipStream_t>(hip_stream), denoise_params(o, o->width, o->height, *d_in, d_workspace, d_out)));
	return RT_OK;
}

int rt_denoise(rt_scene *s, const rt_denoise_inputs *in, const rt_denoise_opts *o, float *out)
{
	int rc = denoise_check(s, in, o, out, false, nullptr);
	if (rc != RT_OK)
		return rc;
	HIP_TRY(hipSetDevice(s->device));
	const uint64_t n = (uint64_t)o->width * o->height;
	// the workspace, out, then the inputs given, in rt_denoise_inputs order
	Layout L;
	const auto p_ws = L.bytes(kDenoiseWorkspaceBytesPerPixel * n);
	const auto p_out = L.add<float>(3 * n), p_color = L.add<float>(3 * n), p_albedo = L.optional<float>(in->albedo, 3 * n),
	           p_normal = L.optional<float>(in->normal, 3 * n), p_depth = L.optional<float>(in->depth, n),
	           p_variance = L.optional<float>(in->variance, n);
	RT_TRY(grow_device_buffer(s->d_denoise, s->d_denoise_bytes, L)); // grown on first use / larger frames only
	Staging st{s};
	st.put(L, p_color, in->color);
	st.put(L, p_albedo, in->albedo);
	st.put(L, p_normal, in->normal);
	st.put(L, p_depth, in->depth);
	st.put(L, p_variance, in->variance);
	if (!st.ok())
		return st.finish("denoise upload");
	const rt_denoise_inputs d_in = {L.at(p_color), L.at(p_albedo), L.at(p_normal), L.at(p_depth), L.at(p_variance)};
	st.rc = rt_denoise_device(s, &d_in, o, L.at(p_ws), L.at(p_out), s->stream);
	st.get(out, L, p_out);
	return st.finish("denoise");
}

int rt_render_denoised(rt_scene *s, const rt_camera *camera, const rt_render_opts *o, const rt_denoise_opts *dopts, float *out_clean,
                       float *out_noisy, uint64_t *rays_shot)
{
	if (!s || !camera || !o || !dopts || !out_clean)
		return fail(RT_ERR_INVALID_ARGUMENT, "null argument");
	int rc = render_denoised_opts_check("rt_render_denoised", o, dopts, o->width, o->height);
	if (rc != RT_OK)
		return rc;
	const uint64_t n = o->width * o->height;
	if (ranges_overlap(out_clean, 12 * n, out_noisy, 12 * n))
		return fail(RT_ERR_INVALID_ARGUMENT, "rt_render_denoised: out_clean overlaps out_noisy");
	rc = need_device(s);
	if (rc != RT_OK)
		return rc;
	return render_denoised_staged(s, pinhole_source(s, camera), o, dopts, "render_denoised", out_clean, out_noisy, rays_shot);
}

} // extern "C"

// rt_render_denoised once its arguments are checked (rt_api_lens.cpp: rt_render_lens_denoised too): the frames in the denoiser's
// buffer on the scene, the steps enqueued, the downloads and the ray count
int render_denoised_staged(rt_scene *s, const DenoisedSource &src, const rt_render_opts *o, const rt_denoise_opts *dopts, const char *what,
                           float *out_clean, float *out_noisy, uint64_t *rays_shot)
{
	HIP_TRY(hipSetDevice(s->device));
	Layout L;
	const DenoisedParts P = denoised_parts(L, o->width * o->height);
	RT_TRY(grow_device_buffer(s->d_denoise, s->d_denoise_bytes, L));
	Staging st{s};
	enqueue_render_denoised(s, src, o, dopts, L, P, st);
	unsigned long long rays[2] = {0, 0};
	st.get(out_clean, L, P.clean);
	st.get(out_noisy, L, P.noisy);
	st.get(rays, L, P.rays);
	const int rc = st.finish(what);
	if (rc == RT_OK && rays_shot)
		*rays_shot = rays[0] + rays[1];
	return rc;
}

// ---- per-pixel noise estimates and render-until-converged (rt_noise.hip) ----
static int noise_opts_check(const rt_noise_opts *n)
{
	if (!std::isfinite(n->luminance_floor) || !(n->luminance_floor > 0.0f))
		return fail(RT_ERR_INVALID_ARGUMENT, "noise: luminance_floor must be finite and > 0");
	if (!std::isfinite(n->threshold) || !(n->threshold >= 0.0f))
		return fail(RT_ERR_INVALID_ARGUMENT, "noise: threshold must be finite and >= 0");
	for (uint32_t r : n->reserved)
		if (r != 0u)
			return fail(RT_ERR_INVALID_ARGUMENT, "noise: reserved must be zero");
	return RT_OK;
}

// The split rule of rt_hip.h for `spp` passes: an explicit split in 2..64 that divides them, or the automatic one halved until it
// does.  A host-only scene has no device to size the automatic split by: 256 CUs stand in (the rule's refusals do not depend on it).
static int noise_split(const rt_scene *s, const rt_render_opts *o, uint64_t spp, uint32_t *split)
{
	if (spp == 0 || spp >= (1ull << 32))
		return fail(RT_ERR_INVALID_ARGUMENT, "noise: the passes of one render must be in [1, 2^32)");
	uint32_t S = o->sample_split;
	if (S == 0u) {
		S = auto_sample_split(s->n_cus, o->width * o->height, spp, 1u);
		while (S > 1u && spp % S != 0u)
			S /= 2u;
		if (S < 2u)
			return fail(RT_ERR_INVALID_ARGUMENT, "noise: no automatic sample_split >= 2 divides the passes (an odd number of passes)");
	} else if (S < 2u || S > kNoiseMaxSplit || spp % S != 0u) {
		return fail(RT_ERR_INVALID_ARGUMENT, "noise: sample_split must be in 2..64 and divide the passes of one render (0: automatic)");
	}
	*split = S;
	return RT_OK;
}

// what every rendering entry point of this stage asks of the scene and the render options, for renders of `spp` passes; the
// caller checks its buffers next and the device last
static int noise_render_check(const rt_scene *s, const rt_render_opts *o, const rt_noise_opts *n, uint64_t spp, uint32_t *split, uint64_t *px)
{
	int rc = noise_opts_check(n);
	if (rc != RT_OK)
		return rc;
	rc = frame_sides("", o->width, o->height, 2);
	if (rc != RT_OK)
		return rc;
	if (o->render_method != RT_METHOD_NAIVE && o->render_method != RT_METHOD_MIS)
		return fail(RT_ERR_INVALID_ARGUMENT, "unknown render method");
	rc = noise_split(s, o, spp, split);
	if (rc != RT_OK)
		return rc;
	if (o->output_layout != RT_LAYOUT_FRAME)
		return fail(RT_ERR_UNSUPPORTED, "noise: RT_LAYOUT_FRAME only");
	if (o->shard_count != 1)
		return fail(RT_ERR_UNSUPPORTED, "noise: the whole frame only (shard_count 1)");
	if (!s->peers.empty())
		return fail(RT_ERR_UNSUPPORTED, "noise: a multi-device scene keeps its chunk sums on several devices");
	return frame_pixels("noise: ", o->width, o->height, 2, px);
}

static uint64_t noise_tile_count(uint64_t w, uint64_t h) { return tile_grid(w, h).count; }
// the render's whole-frame tiling into the parameters of a kernel that reads its chunk sums in work-item order
template <class P> static void fill_frame_tiling(P &p, const rt_render_opts *o)
{
	const FrameTiling t = frame_tiling(o);
	p.tile_w = t.tile_w, p.tile_h = t.tile_h, p.tiles_x = t.tiles_x, p.n_work = (uint32_t)t.n_work;
}
// the scene's scratch for n pixels: the summary of the blocking calls, then the state planes M, L, V; what a blocking call stages
// comes behind (described after these, so that the state is where the _device call inside it finds it)
struct NoiseState {
	Layout::Part<rt_noise_summary> summary;
	Layout::Part<float> m, l, v;
};
static NoiseState noise_state(Layout &L, uint64_t n)
{
	return NoiseState{L.add<rt_noise_summary>(1), L.add<float>(3 * n), L.add<float>(n), L.add<float>(n)}; // (in this order)
}

static int noise_buffers_check(const rt_scene *s, const float *albedo, const rt_noise_buffers *b, uint64_t n, uint64_t w, uint64_t h)
{
	if (!b->mean)
		return fail(RT_ERR_INVALID_ARGUMENT, "rt_noise_buffers: mean must not be NULL");
	const void *buf[6] = {b->mean, b->variance, b->lum_mean, b->tile_error, b->summary, albedo};
	const uint64_t bytes[6] = {12 * n, 4 * n, 4 * n, 4 * noise_tile_count(w, h), kNoiseSummaryBytes, 12 * n};
	const int rc = check_disjoint("noise: an output buffer overlaps another buffer", buf, bytes, 5, 6);
	return rc == RT_OK ? need_device(s) : rc;
}

// the tile stage on `stream`: the summary zeroed by reset_kernel (not a memset node: see its comment in rt_render.hip), its
// reserved word standing in for the counter that kernel clears
static int enqueue_noise_tiles(hipStream_t stream, const float *d_lum, const float *d_var, uint64_t w, uint64_t h, const rt_noise_opts *n,
                               float *d_tile_error, rt_noise_summary *d_summary)
{
	DevNoiseTileParams T;
	std::memset(&T, 0, sizeof T);
	T.width = (uint32_t)w;
	T.height = (uint32_t)h;
	T.tiles_x = tile_grid(w, h).tiles_x;
	T.n_tiles = (uint32_t)tile_grid(w, h).count;
	T.luminance_floor = n->luminance_floor;
	T.threshold = n->threshold;
	T.lum_mean = d_lum;
	T.variance = d_var;
	T.tile_error = d_tile_error;
	T.summary = reinterpret_cast<uint32_t *>(d_summary);
	if (d_summary)
		HIP_TRY(launch_reset(stream, T.summary + 3, nullptr, reinterpret_cast<float *>(d_summary), 3));
	HIP_TRY(launch_noise_tiles(stream, T));
	return RT_OK;
}

// One batch on `stream`: the render of rt_render_device at `split` into d_render, the chunk kernel (state == nullptr: one batch,
// nothing kept; else batch number `nb` of a sequence, 1 = fresh) and, if a tile output is asked for, the tile stage.
// out->variance / lum_mean NULL with a tile output: the state's L and V planes stand in (the parts `N` of the scene's scratch, noise_state).
static int enqueue_noise_batch(rt_scene *s, const rt_camera *camera, const rt_render_opts *o, uint32_t split, const rt_noise_opts *n,
                               const float *d_albedo, float *d_render, const Layout &L, const NoiseState &N, bool keep_state,
                               uint32_t nb, const rt_noise_buffers *out, uint64_t *d_rays, hipStream_t stream)
{
	rt_render_opts os = *o;
	os.sample_split = split;
	int rc = rt_render_device(s, camera, &os, d_render, d_rays, stream);
	if (rc != RT_OK)
		return rc;
	float *const state_m = L.at(N.m), *const state_l = L.at(N.l), *const state_v = L.at(N.v);
	const bool tiles = out->tile_error || out->summary;
	float *d_lum = out->lum_mean, *d_var = out->variance;
	if (tiles && !keep_state) { // (a sequence divides its state out into planes of its own)
		d_lum = d_lum ? d_lum : state_l;
		d_var = d_var ? d_var : state_v;
	}
	DevNoiseChunkParams C;
	std::memset(&C, 0, sizeof C);
	C.width = (uint32_t)o->width;
	C.height = (uint32_t)o->height;
	fill_frame_tiling(C, o);
	C.split = split;
	C.chunk_passes = (uint32_t)(os.samples_per_pixel / split);
	C.fresh = nb == 1u ? 1u : 0u;
	C.batches = (float)nb;
	C.partial = s->d_partial;
	C.albedo = d_albedo;
	C.mean_in = d_render;
	if (keep_state) {
		C.state_m = state_m;
		C.state_l = state_l;
		C.state_v = state_v;
	}
	C.out_mean = out->mean;
	C.out_lum = d_lum;
	C.out_var = d_var;
	HIP_TRY(launch_noise_chunks(stream, C));
	if (tiles)
		return enqueue_noise_tiles(stream, d_lum, d_var, o->width, o->height, n, out->tile_error, out->summary);
	return RT_OK;
}

static int noise_tiles_check(const rt_scene *s, const float *lum_mean, const float *variance, uint32_t w, uint32_t h, const rt_noise_opts *n,
                             const float *tile_error, const rt_noise_summary *summary)
{
	if (!s || !lum_mean || !variance || !n)
		return fail(RT_ERR_INVALID_ARGUMENT, "null argument");
	if (!tile_error && !summary)
		return fail(RT_ERR_INVALID_ARGUMENT, "noise_tiles: tile_error and summary are both NULL");
	int rc = noise_opts_check(n);
	if (rc != RT_OK)
		return rc;
	uint64_t px = 0;
	rc = frame_pixels("noise_tiles: ", w, h, 1, &px);
	if (rc != RT_OK)
		return rc;
	const void *buf[4] = {tile_error, summary, lum_mean, variance};
	const uint64_t bytes[4] = {4 * noise_tile_count(w, h), kNoiseSummaryBytes, 4 * px, 4 * px};
	rc = check_disjoint("noise_tiles: an output buffer overlaps another buffer", buf, bytes, 2, 4);
	return rc == RT_OK ? need_device(s) : rc;
}

// A sequence of batches over one state: what rt_render_converged and rt_render_adaptive share.  Batch nb = 1, 2, ... is a render of
// `batch` passes from sample_begin + (nb - 1) * batch at the resolved split, its (mean, lbar, var) go into the state, and the planes,
// the tile errors and the summary are the state's divided out.  A stage describes its own parts on L between check() and
// allocate(), and keeps its own stop rule and result.
namespace {

struct BatchSequence {
	rt_scene *s;
	const rt_camera *camera;
	const rt_render_opts *o;
	const rt_noise_opts *n;
	uint64_t batch;
	const char *stage; // starts the messages
	uint32_t split = 0;
	uint64_t px = 0, n_tiles = 0;
	Layout L;
	NoiseState N{};
	Layout::Part<float> p_render{}, p_mean{}, p_lum{}, p_variance{}, p_tiles{};
	rt_noise_buffers d_out{};

	// The checks both stages start with, in their order (the stage checks its buffers next and the device last), then the shared
	// parts: behind the state, whose summary the sequence uses, a batch's render, then mean, lum_mean, variance and the tile errors.
	int check(uint64_t max_passes, const float *out_mean, const void *result)
	{
		if (!s || !camera || !o || !n || !out_mean || !result)
			return fail(RT_ERR_INVALID_ARGUMENT, "null argument");
		if (batch == 0 || max_passes < batch)
			return fail(RT_ERR_INVALID_ARGUMENT, std::string(stage) + ": batch must be >= 1 and max_passes >= batch");
		RT_TRY(noise_render_check(s, o, n, batch, &split, &px));
		if (max_passes / batch >= (1ull << 24)) // (nb is divided by as a float)
			return fail(RT_ERR_UNSUPPORTED, std::string(stage) + ": 2^24 batches or more");
		n_tiles = noise_tile_count(o->width, o->height);
		N = noise_state(L, px);
		p_render = L.add<float>(3 * px), p_mean = L.add<float>(3 * px), p_lum = L.add<float>(px), p_variance = L.add<float>(px);
		p_tiles = L.add<float>(n_tiles);
		return RT_OK;
	}
	int allocate()
	{
		HIP_TRY(hipSetDevice(s->device));
		RT_TRY(grow_device_buffer(s->d_noise, s->d_noise_bytes, L));
		d_out = rt_noise_buffers{L.at(p_mean), L.at(p_variance), L.at(p_lum), L.at(p_tiles), L.at(N.summary)};
		return RT_OK;
	}
	rt_render_opts batch_opts(uint32_t nb) const
	{
		rt_render_opts ob = *o;
		ob.samples_per_pixel = batch, ob.sample_split = split, ob.sample_begin = o->sample_begin + (uint64_t)(nb - 1u) * batch;
		return ob;
	}
	// batch nb over the whole frame on s->stream: the render, the chunk kernel on the state, the tile stage
	int whole_frame(uint32_t nb, const float *d_albedo)
	{
		const rt_render_opts ob = batch_opts(nb);
		return enqueue_noise_batch(s, camera, &ob, split, n, d_albedo, L.at(p_render), L, N, true, nb, &d_out, reinterpret_cast<uint64_t *>(s->d_rays),
		                           s->stream);
	}
	// what the host reads after every batch, and the batch's status: the summary, and the ray counter added to *rays_shot
	int read_back(Staging &st, rt_noise_summary *summary, uint64_t *rays_shot)
	{
		unsigned long long rays = 0;
		st.get(summary, L, N.summary);
		st.download(&rays, s->d_rays, sizeof rays);
		RT_TRY(st.finish(stage));
		*rays_shot += rays;
		return RT_OK;
	}
};

} // namespace

extern "C" {

int rt_noise_opts_default(rt_noise_opts *out)
{
	if (!out)
		return fail(RT_ERR_INVALID_ARGUMENT, "null argument");
	std::memset(out, 0, sizeof *out);
	out->luminance_floor = 0.01f;
	out->threshold = 0.05f;
	return RT_OK;
}

int rt_render_noise_device(rt_scene *s, const rt_camera *camera, const rt_render_opts *o, const rt_noise_opts *n, const float *d_albedo,
                           const rt_noise_buffers *d_out, uint64_t *d_rays_shot, void *hip_stream)
{
	if (!s || !camera || !o || !n || !d_out)
		return fail(RT_ERR_INVALID_ARGUMENT, "null argument");
	uint32_t split = 0;
	uint64_t px = 0;
	int rc = noise_render_check(s, o, n, o->samples_per_pixel, &split, &px);
	if (rc == RT_OK)
		rc = noise_buffers_check(s, d_albedo, d_out, px, o->width, o->height);
	if (rc != RT_OK)
		return rc;
	HIP_TRY(hipSetDevice(s->device));
	Layout L;
	const NoiseState N = noise_state(L, px);
	RT_TRY(grow_device_buffer(s->d_noise, s->d_noise_bytes, L)); // grows on first use only (not capturable on that call)
	return enqueue_noise_batch(s, camera, o, split, n, d_albedo, d_out->mean, L, N, false, 1u, d_out, d_rays_shot,
	                           static_cast<hipStream_t>(hip_stream));
}

int rt_render_noise(rt_scene *s, const rt_camera *camera, const rt_render_opts *o, const rt_noise_opts *n, const float *albedo,
                    const rt_noise_buffers *out, uint64_t *rays_shot)
{
	if (!s || !camera || !o || !n || !out)
		return fail(RT_ERR_INVALID_ARGUMENT, "null argument");
	uint32_t split = 0;
	uint64_t px = 0;
	int rc = noise_render_check(s, o, n, o->samples_per_pixel, &split, &px);
	if (rc == RT_OK)
		rc = noise_buffers_check(s, albedo, out, px, o->width, o->height);
	if (rc != RT_OK)
		return rc;
	HIP_TRY(hipSetDevice(s->device));
	// behind the state: the mean, then the channels asked for, the summary and the albedo if given
	Layout L;
	noise_state(L, px);
	const auto p_mean = L.add<float>(3 * px), p_variance = L.optional<float>(out->variance, px), p_lum = L.optional<float>(out->lum_mean, px),
	           p_tiles = L.optional<float>(out->tile_error, noise_tile_count(o->width, o->height)), p_albedo = L.optional<float>(albedo, 3 * px);
	const auto p_summary = L.optional<rt_noise_summary>(out->summary, 1);
	RT_TRY(grow_device_buffer(s->d_noise, s->d_noise_bytes, L));
	Staging st{s};
	st.put(L, p_albedo, albedo);
	const rt_noise_buffers d_out = {L.at(p_mean), L.at(p_variance), L.at(p_lum), L.at(p_tiles), L.at(p_summary)};
	if (st.ok())
		st.rc = rt_render_noise_device(s, camera, o, n, L.at(p_albedo), &d_out, reinterpret_cast<uint64_t *>(s->d_rays), s->stream);
	st.get(out->mean, L, p_mean);
	st.get(out->variance, L, p_variance);
	st.get(out->lum_mean, L, p_lum);
	st.get(out->tile_error, L, p_tiles);
	st.get(out->summary, L, p_summary);
	st.download(rays_shot, s->d_rays, sizeof(uint64_t));
	return st.finish("render_noise");
}

int rt_noise_tiles_device(rt_scene *s, const float *d_lum_mean, const float *d_variance, uint32_t width, uint32_t height,
                          const rt_noise_opts *n, float *d_tile_error, rt_noise_summary *d_summary, void *hip_stream)
{
	int rc = noise_tiles_check(s, d_lum_mean, d_variance, width, height, n, d_tile_error, d_summary);
	if (rc != RT_OK)
		return rc;
	HIP_TRY(hipSetDevice(s->device));
	return enqueue_noise_tiles(static_cast<hipStream_t>(hip_stream), d_lum_mean, d_variance, width, height, n, d_tile_error, d_summary);
}

int rt_noise_tiles(rt_scene *s, const float *lum_mean, const float *variance, uint32_t width, uint32_t height, const rt_noise_opts *n,
                   float *tile_error, rt_noise_summary *summary)
{
	int rc = noise_tiles_check(s, lum_mean, variance, width, height, n, tile_error, summary);
	if (rc != RT_OK)
		return rc;
	HIP_TRY(hipSetDevice(s->device));
	const uint64_t px = (uint64_t)width * height;
	Layout L;
	const auto p_lum = L.add<float>(px), p_variance = L.add<float>(px), p_tiles = L.optional<float>(tile_error, noise_tile_count(width, height));
	const auto p_summary = L.optional<rt_noise_summary>(summary, 1);
	RT_TRY(grow_device_buffer(s->d_noise, s->d_noise_bytes, L));
	Staging st{s};
	st.put(L, p_lum, lum_mean);
	st.put(L, p_variance, variance);
	if (st.ok())
		st.rc = rt_noise_tiles_device(s, L.at(p_lum), L.at(p_variance), width, height, n, L.at(p_tiles), L.at(p_summary),
		                              s->stream);
	st.get(tile_error, L, p_tiles);
	st.get(summary, L, p_summary);
	return st.finish("noise_tiles");
}

int rt_render_converged(rt_scene *s, const rt_camera *camera, const rt_render_opts *o, const rt_noise_opts *n, uint64_t batch,
                        uint32_t min_batches, uint64_t max_passes, float *out_mean, float *out_variance, float *out_tile_error,
                        rt_noise_result *result)
{
	BatchSequence q{s, camera, o, n, batch, "render_converged"};
	RT_TRY(q.check(max_passes, out_mean, result));
	{
		const void *buf[3] = {out_mean, out_variance, out_tile_error};
		const uint64_t bytes[3] = {12 * q.px, 4 * q.px, 4 * q.n_tiles};
		RT_TRY(check_disjoint("render_converged: two output buffers overlap", buf, bytes, 3, 3));
		RT_TRY(need_device(s));
	}
	RT_TRY(q.allocate());
	std::memset(result, 0, sizeof *result);
	for (uint32_t nb = 1;; ++nb) {
		Staging st{s};
		st.rc = q.whole_frame(nb, nullptr);
		RT_TRY(q.read_back(st, &result->summary, &result->rays_shot));
		result->batches = nb;
		result->passes = (uint64_t)nb * batch;
		result->converged = nb >= min_batches && result->summary.max_tile_error <= n->threshold ? 1u : 0u;
		if (result->converged || result->passes + batch > max_passes)
			break;
	}
	Staging st{s};
	st.get(out_mean, q.L, q.p_mean);
	st.get(out_variance, q.L, q.p_variance);
	st.get(out_tile_error, q.L, q.p_tiles);
	return st.finish("render_converged");
}

} // extern "C"

// ---- the render on a list of tiles and the active list (rt_adaptive.hip) ----
// argument checks of both rt_render_tiles entry points in the order rt_hip.h states, the device last; *split is S resolved
static int tiles_check(const rt_scene *s, const rt_camera *camera, const rt_render_opts *o, const uint32_t *tiles, uint32_t n_tiles,
                       const float *out, const float *chunk_sums, uint32_t *split, uint64_t *px)
{
	if (!s || !camera || !o || !out || (!tiles && n_tiles != 0u))
		return fail(RT_ERR_INVALID_ARGUMENT, "null argument");
	int rc = frame_sides("", o->width, o->height, 2);
	if (rc != RT_OK)
		return rc;
	if (o->shard_count == 0 || o->shard_index >= o->shard_count)
		return fail(RT_ERR_INVALID_ARGUMENT, "shard_index must be < shard_count and shard_count >= 1");
	if (o->render_method != RT_METHOD_NAIVE && o->render_method != RT_METHOD_MIS)
		return fail(RT_ERR_INVALID_ARGUMENT, "unknown render method");
	if (o->samples_per_pixel == 0 || o->samples_per_pixel >= (1ull << 32))
		return fail(RT_ERR_INVALID_ARGUMENT, "samples_per_pixel must be in [1, 2^32)");
	if (o->output_layout != RT_LAYOUT_FRAME && o->output_layout != RT_LAYOUT_SHARD)
		return fail(RT_ERR_INVALID_ARGUMENT, "unknown output layout");
	if (o->width > (1ull << 31) || o->height > (1ull << 31) || o->width * o->height >= (1ull << 31))
		return fail(RT_ERR_UNSUPPORTED, "render_tiles: 2^31 pixels or more");
	*px = o->width * o->height;
	uint32_t S = o->sample_split;
	if (S == 0u) // as rt_render resolves it for the whole frame (a host-only scene: for 256 CUs)
		S = auto_sample_split(s->n_cus, *px, o->samples_per_pixel, 1u);
	if (S > o->samples_per_pixel)
		return fail(RT_ERR_INVALID_ARGUMENT, "sample_split larger than samples_per_pixel");
	*split = S;
	if (S > 1u && ranges_overlap(out, 12 * *px, chunk_sums, 12ull * S * 64u * n_tiles))
		return fail(RT_ERR_INVALID_ARGUMENT, "render_tiles: chunk_sums overlaps the frame");
	if (o->output_layout != RT_LAYOUT_FRAME)
		return fail(RT_ERR_UNSUPPORTED, "render_tiles: RT_LAYOUT_FRAME only");
	if (o->shard_count != 1)
		return fail(RT_ERR_UNSUPPORTED, "render_tiles: the whole frame only (shard_count 1)");
	if (!s->peers.empty())
		return fail(RT_ERR_UNSUPPORTED, "render_tiles: a multi-device scene renders its own shards");
	if (64ull * n_tiles * S >= (1ull << 31))
		return fail(RT_ERR_UNSUPPORTED, "render_tiles: 64 x tiles x sample_split exceeds 2^31 lane items");
	return need_device(s);
}

static int select_check(const rt_scene *s, const float *tile_error, uint32_t w, uint32_t h, float threshold, const uint32_t *tiles,
                        const uint32_t *count)
{
	if (!s || !tile_error || !tiles || !count)
		return fail(RT_ERR_INVALID_ARGUMENT, "null argument");
	if (threshold != threshold)
		return fail(RT_ERR_INVALID_ARGUMENT, "select_tiles: the threshold is NaN");
	uint64_t px = 0;
	int rc = frame_pixels("select_tiles: ", w, h, 1, &px);
	if (rc != RT_OK)
		return rc;
	const uint64_t n = noise_tile_count(w, h);
	const void *buf[3] = {tiles, count, tile_error};
	const uint64_t bytes[3] = {4 * n, 4, 4 * n};
	rc = check_disjoint("select_tiles: an output buffer overlaps another buffer", buf, bytes, 2, 3);
	return rc == RT_OK ? need_device(s) : rc;
}

extern "C" {

int rt_render_tiles_device(rt_scene *s, const rt_camera *camera, const rt_render_opts *o, const uint32_t *d_tiles, uint32_t n_tiles,
                           float *d_out_rgb, float *d_chunk_sums, uint64_t *d_rays_shot, void *hip_stream)
{
	uint32_t split = 0;
	uint64_t px = 0;
	int rc = tiles_check(s, camera, o, d_tiles, n_tiles, d_out_rgb, d_chunk_sums, &split, &px);
	if (rc != RT_OK)
		return rc;
	HIP_TRY(hipSetDevice(s->device));
	bool prune = false;
	DevScene dev;
	rc = four_wave_traversal(s, &prune, &dev); // (rt_api_internal.h)
	if (rc != RT_OK)
		return rc;
	const size_t lds_bytes = four_wave_stack_lds_bytes(dev) + kTilesRecordLdsBytes;
	if (lds_bytes > s->max_lds)
		return fail(RT_ERR_UNSUPPORTED, "traversal stacks exceed the LDS of one CU");
	DevTilesParams P;
	std::memset(&P, 0, sizeof P);
	P.cam = dev_camera(camera);
	P.tiles = d_tiles;
	P.out = d_out_rgb;
	P.chunk_sums = split > 1u ? d_chunk_sums : nullptr;
	P.rays_shot = reinterpret_cast<unsigned long long *>(d_rays_shot);
	P.n_tiles = n_tiles;
	P.width = (uint32_t)o->width;
	P.height = (uint32_t)o->height;
	P.tiles_x = tile_grid(o->width, o->height).tiles_x;
	P.tile_count = (uint32_t)tile_grid(o->width, o->height).count;
	P.spp = (uint32_t)o->samples_per_pixel;
	P.split = split;
	P.item_chunks = P.chunk_sums ? 1u : split;
	const uint64_t items = (uint64_t)n_tiles * (split / P.item_chunks);
	P.n_lanes = (uint32_t)(64u * items);
	P.seed_lo = (uint32_t)o->seed;
	P.seed_hi = (uint32_t)(o->seed >> 32);
	P.sample_begin_lo = (uint32_t)o->sample_begin;
	P.sample_begin_hi = (uint32_t)(o->sample_begin >> 32);
	P.max_depth = o->max_depth;
	P.rr_threshold = o->rr_threshold;
	// one wave per work item at a time (an empty list still plans one workgroup; launch_tiles then launches none)
	HIP_TRY(launch_tiles(o->render_method == RT_METHOD_NAIVE ? 0 : 1, prune, static_cast<hipStream_t>(hip_stream), dev, P,
	                     path_lane_groups(s, lds_bytes, kTilesWaves, (items + kFourWaves - 1u) / kFourWaves)));
	return RT_OK;
}

int rt_render_tiles(rt_scene *s, const rt_camera *camera, const rt_render_opts *o, const uint32_t *tiles, uint32_t n_tiles, float *out_rgb,
                    float *chunk_sums, uint64_t *rays_shot)
{
	uint32_t split = 0;
	uint64_t px = 0;
	int rc = tiles_check(s, camera, o, tiles, n_tiles, out_rgb, chunk_sums, &split, &px);
	if (rc != RT_OK && rc != RT_ERR_NO_DEVICE)
		return rc;
	{ // the list itself, ahead of the device: distinct indices below the tile count
		const uint64_t tile_count = noise_tile_count(o->width, o->height);
		if (n_tiles > tile_count) // (a longer list repeats a tile or names none)
			return fail(RT_ERR_INVALID_ARGUMENT, "render_tiles: more tiles listed than the frame has");
		std::vector<bool> seen(tile_count, false);
		for (uint32_t i = 0; i < n_tiles; ++i) {
			if (tiles[i] >= tile_count)
				return fail(RT_ERR_INVALID_ARGUMENT, "render_tiles: a tile index is not below the tile count");
			if (seen[tiles[i]])
				return fail(RT_ERR_INVALID_ARGUMENT, "render_tiles: a tile is listed twice");
			seen[tiles[i]] = true;
		}
	}
	if (rc != RT_OK)
		return need_device(s);
	HIP_TRY(hipSetDevice(s->device));
	if (split == 1u)
		chunk_sums = nullptr;
	// the frame, the list, the chunk sums if asked for
	Layout L;
	const auto p_frame = L.add<float>(3 * px), p_sums = L.optional<float>(chunk_sums, 3ull * split * 64u * n_tiles);
	const auto p_tiles = L.add<uint32_t>(n_tiles);
	RT_TRY(grow_device_buffer(s->d_noise, s->d_noise_bytes, L));
	Staging st{s};
	st.put(L, p_frame, out_rgb);
	if (n_tiles != 0u)
		st.put(L, p_tiles, tiles);
	if (st.ok())
		st.rc = rt_render_tiles_device(s, camera, o, L.at(p_tiles), n_tiles, L.at(p_frame), L.at(p_sums), reinterpret_cast<uint64_t *>(s->d_rays),
		                               s->stream);
	if (n_tiles != 0u) {
		st.get(out_rgb, L, p_frame);
		st.get(chunk_sums, L, p_sums);
	}
	st.download(rays_shot, s->d_rays, sizeof(uint64_t));
	return st.finish("render_tiles");
}

// Adaptive sampling (rt_hip.h): whole-frame batches are rt_render_converged's own (enqueue_noise_batch: the specialised render
// kernels, the same state arithmetic, so a run that never drops a tile returns its bytes); a batch whose active list is shorter
// than the tile grid goes through rt_render_tiles_device with its chunk buffer and adaptive_fold_kernel.  After either, the tile
// stage recomputes every tile's error from the planes (a stopped tile's planes have not changed, so neither has its error) and the
// selection makes the next list; the host reads the count, the summary and the ray counter.
int rt_render_adaptive(rt_scene *s, const rt_camera *camera, const rt_render_opts *o, const rt_noise_opts *n, const float *albedo,
                       uint64_t batch, uint32_t min_batches, uint64_t max_passes, float *out_mean, float *out_variance, float *out_tile_error,
                       uint32_t *out_passes, rt_adaptive_result *result)
{
	BatchSequence q{s, camera, o, n, batch, "render_adaptive"};
	RT_TRY(q.check(max_passes, out_mean, result));
	const uint64_t px = q.px, n_tiles = q.n_tiles;
	const uint32_t split = q.split;
	if (64ull * n_tiles * split >= (1ull << 31))
		return fail(RT_ERR_UNSUPPORTED, "render_adaptive: 64 x tiles x sample_split exceeds 2^31 lane items");
	{
		const void *buf[5] = {out_mean, out_variance, out_tile_error, out_passes, albedo};
		const uint64_t bytes[5] = {12 * px, 4 * px, 4 * n_tiles, 4 * px, 12 * px};
		RT_TRY(check_disjoint("render_adaptive: an output buffer overlaps another buffer", buf, bytes, 4, 5));
		RT_TRY(need_device(s));
	}
	// behind the sequence's parts: the albedo if given, the chunk sums of a masked batch (sized for the whole grid), the per-pixel
	// batch counts, the active list and its length
	Layout &L = q.L;
	const auto p_albedo = L.optional<float>(albedo, 3 * px), p_sums = L.add<float>(3ull * split * 64u * n_tiles);
	const auto p_nb = L.add<uint32_t>(px), p_list = L.add<uint32_t>(n_tiles), p_count = L.add<uint32_t>(1);
	RT_TRY(q.allocate());
	std::memset(result, 0, sizeof *result);
	uint32_t active = (uint32_t)n_tiles; // before any batch every tile is active
	bool masked = false;
	for (uint32_t nb = 1;; ++nb) {
		Staging st{s};
		if (nb == 1u)
			st.put(L, p_albedo, albedo);
		if (st.ok()) {
			// whole-frame batches come first: until one batch has been masked every pixel has nb - 1 batches behind it
			if (!masked && (nb - 1u < min_batches || active == n_tiles)) {
				st.rc = q.whole_frame(nb, L.at(p_albedo));
				if (st.rc == RT_OK)
					st.e = launch_fill_u32(s->stream, L.at(p_nb), px, nb);
			} else {
				masked = true;
				const rt_render_opts ob = q.batch_opts(nb);
				st.rc = rt_render_tiles_device(s, camera, &ob, L.at(p_list), active, L.at(q.p_render), L.at(p_sums), reinterpret_cast<uint64_t *>(s->d_rays),
				                               s->stream);
				if (st.rc == RT_OK) {
					DevFoldParams F;
					std::memset(&F, 0, sizeof F);
					F.tiles = L.at(p_list);
					F.n_tiles = active;
					F.width = (uint32_t)o->width, F.height = (uint32_t)o->height;
					F.tiles_x = tile_grid(o->width, o->height).tiles_x, F.tile_count = (uint32_t)n_tiles;
					F.split = split, F.chunk_passes = (uint32_t)(batch / split);
					F.sums = L.at(p_sums), F.albedo = L.at(p_albedo), F.mean_in = L.at(q.p_render);
					F.state_m = L.at(q.N.m), F.state_l = L.at(q.N.l), F.state_v = L.at(q.N.v), F.nb = L.at(p_nb);
					F.out_mean = q.d_out.mean, F.out_lum = q.d_out.lum_mean, F.out_var = q.d_out.variance;
					st.e = launch_adaptive_fold(s->stream, F);
				}
				if (st.ok())
					st.rc = enqueue_noise_tiles(s->stream, q.d_out.lum_mean, q.d_out.variance, o->width, o->height, n, q.d_out.tile_error, q.d_out.summary);
			}
		}
		if (st.ok())
			st.rc = rt_noise_select_tiles_device(s, q.d_out.tile_error, (uint32_t)o->width, (uint32_t)o->height, n->threshold, L.at(p_list),
			                                     L.at(p_count), s->stream);
		st.get(&active, L, p_count);
		RT_TRY(q.read_back(st, &result->summary, &result->rays_shot));
		result->batches = nb;
		result->converged = nb >= min_batches && active == 0u ? 1u : 0u;
		if (result->converged || (uint64_t)(nb + 1u) * batch > max_passes)
			break;
	}
	std::vector<uint32_t> counts(px);
	Staging st{s};
	st.get(out_mean, L, q.p_mean);
	st.get(out_variance, L, q.p_variance);
	st.get(out_tile_error, L, q.p_tiles);
	st.get(counts.data(), L, p_nb);
	RT_TRY(st.finish("render_adaptive"));
	for (uint64_t p = 0; p < px; ++p) {
		result->pixel_passes += (uint64_t)counts[p] * batch;
		if (out_passes)
			out_passes[p] = (uint32_t)((uint64_t)counts[p] * batch);
	}
	return RT_OK;
}

int rt_noise_select_tiles_device(rt_scene *s, const float *d_tile_error, uint32_t width, uint32_t height, float threshold, uint32_t *d_tiles,
                                 uint32_t *d_count, void *hip_stream)
{
	int rc = select_check(s, d_tile_error, width, height, threshold, d_tiles, d_count);
	if (rc != RT_OK)
		return rc;
	HIP_TRY(hipSetDevice(s->device));
	DevSelectParams P;
	std::memset(&P, 0, sizeof P);
	P.tile_error = d_tile_error;
	P.tiles = d_tiles;
	P.count = d_count;
	P.n_tiles = (uint32_t)noise_tile_count(width, height);
	P.threshold = threshold;
	HIP_TRY(launch_select_tiles(static_cast<hipStream_t>(hip_stream), P));
	return RT_OK;
}

int rt_noise_select_tiles(rt_scene *s, const float *tile_error, uint32_t width, uint32_t height, float threshold, uint32_t *tiles,
                          uint32_t *count)
{
	int rc = select_check(s, tile_error, width, height, threshold, tiles, count);
	if (rc != RT_OK)
		return rc;
	HIP_TRY(hipSetDevice(s->device));
	const uint64_t n = noise_tile_count(width, height);
	Layout L;
	const auto p_err = L.add<float>(n);
	const auto p_tiles = L.add<uint32_t>(n), p_count = L.add<uint32_t>(1);
	RT_TRY(grow_device_buffer(s->d_noise, s->d_noise_bytes, L));
	Staging st{s};
	st.put(L, p_err, tile_error);
	if (st.ok())
		st.rc = rt_noise_select_tiles_device(s, L.at(p_err), width, height, threshold, L.at(p_tiles), L.at(p_count), s->stream);
	uint32_t found = 0;
	st.get(&found, L, p_count);
	rc = st.finish("select_tiles");
	if (rc != RT_OK)
		return rc;
	*count = found;
	Staging st2{s};
	st2.download(tiles, L.at(p_tiles), 4ull * found); // (the rest of `tiles` stays as it was)
	return st2.finish("select_tiles");
}

int rt_render_denoised_split(rt_scene *s, const rt_camera *camera, const rt_render_opts *o, const rt_denoise_opts *dopts, float *out_clean,
                             float *out_noisy, float *out_variance, uint64_t *rays_shot)
{
	if (!s || !camera || !o || !dopts || !out_clean)
		return fail(RT_ERR_INVALID_ARGUMENT, "null argument");
	int rc = denoise_opts_check(dopts, o->width, o->height);
	if (rc != RT_OK)
		return rc;
	rt_noise_opts n;
	rt_noise_opts_default(&n);
	uint32_t split = 0;
	uint64_t px = 0;
	rc = noise_render_check(s, o, &n, o->samples_per_pixel, &split, &px);
	if (rc != RT_OK)
		return rc;
	const void *buf[3] = {out_clean, out_noisy, out_variance};
	const uint64_t bytes[3] = {12 * px, 12 * px, 4 * px};
	rc = check_disjoint("rt_render_denoised_split: two output buffers overlap", buf, bytes, 3, 3);
	if (rc != RT_OK)
		return rc;
	// the middle call: the render and its variance plane, one render at the split
	auto middle = [&](float *d_albedo, float *d_noisy, float *d_var, uint64_t *d_rays) {
		const rt_noise_buffers d_out = {d_noisy, d_var, nullptr, nullptr, nullptr};
		return rt_render_noise_device(s, camera, o, &n, d_albedo, &d_out, d_rays, s->stream);
	};
	return render_denoised_guided(s, camera, o, dopts, px, px, true, middle, "render_denoised_split", out_clean, out_noisy, out_variance, rays_shot);
}

} // extern "C"

// ---- firefly-robust frames: a rank-trimmed mean of the chunk sums (rt_robust.hip) ----
static int robust_opts_check(const rt_robust_opts *r)
{
	if (r->mode != RT_ROBUST_TRIM && r->mode != RT_ROBUST_MEDIAN && r->mode != RT_ROBUST_GINI)
		return fail(RT_ERR_INVALID_ARGUMENT, "robust: unknown mode");
	if (!std::isfinite(r->gini_gain) || !(r->gini_gain > 0.0f))
		return fail(RT_ERR_INVALID_ARGUMENT, "robust: gini_gain must be finite and > 0");
	for (uint32_t w : r->reserved)
		if (w != 0u)
			return fail(RT_ERR_INVALID_ARGUMENT, "robust: reserved must be zero");
	return RT_OK;
}

// the robust options, then what the noise stage asks of the scene and the render options (its split rule included)
static int robust_render_check(const rt_scene *s, const rt_render_opts *o, const rt_robust_opts *r, uint32_t *split, uint64_t *px)
{
	int rc = robust_opts_check(r);
	if (rc != RT_OK)
		return rc;
	rt_noise_opts n;
	rt_noise_opts_default(&n);
	return noise_render_check(s, o, &n, o->samples_per_pixel, split, px);
}

// the five outputs against each other and against what is read (`sums` of sums_bytes: the caller's planes, or NULL); the device last
static int robust_buffers_check(const rt_scene *s, const rt_robust_buffers *b, const float *albedo, const float *sums, uint64_t sums_bytes,
                                uint64_t n)
{
	if (!b->out)
		return fail(RT_ERR_INVALID_ARGUMENT, "rt_robust_buffers: out must not be NULL");
	const void *buf[7] = {b->out, b->mean, b->gini, b->trimmed, b->dropped, albedo, sums};
	const uint64_t bytes[7] = {12 * n, 12 * n, 4 * n, n, n, 12 * n, sums_bytes};
	const int rc = check_disjoint("robust: an output buffer overlaps another buffer", buf, bytes, 5, 7);
	return rc == RT_OK ? need_device(s) : rc;
}

static DevRobustParams robust_params(const rt_robust_opts *r, uint64_t w, uint64_t h, uint32_t split, uint32_t chunk_passes, const float *d_sums,
                                     const float *d_albedo, const rt_robust_buffers *d_out)
{
	DevRobustParams P;
	std::memset(&P, 0, sizeof P);
	P.width = (uint32_t)w;
	P.height = (uint32_t)h;
	P.n_work = (uint32_t)(w * h); // frame raster; the render form sets its tiles
	P.split = split;
	P.chunk_passes = chunk_passes;
	P.mode = r->mode;
	P.trim = r->trim;
	P.gini_gain = r->gini_gain;
	P.sums = d_sums;
	P.albedo = d_albedo;
	P.out = d_out->out;
	P.mean = d_out->mean;
	P.gini = d_out->gini;
	P.trimmed = d_out->trimmed;
	P.dropped = d_out->dropped;
	return P;
}

static int robust_combine_check(const rt_scene *s, const float *sums, uint32_t split, uint64_t chunk_passes, uint32_t w, uint32_t h,
                                const float *albedo, const rt_robust_opts *r, const rt_robust_buffers *b, uint64_t *px)
{
	if (!s || !sums || !r || !b)
		return fail(RT_ERR_INVALID_ARGUMENT, "null argument");
	int rc = robust_opts_check(r);
	if (rc != RT_OK)
		return rc;
	if (split < 2u || split > kRobustMaxSplit)
		return fail(RT_ERR_INVALID_ARGUMENT, "robust_combine: split must be in 2..64");
	if (chunk_passes == 0 || chunk_passes >= (1ull << 32) || split * chunk_passes >= (1ull << 32))
		return fail(RT_ERR_INVALID_ARGUMENT, "robust_combine: chunk_passes must be >= 1 and split * chunk_passes < 2^32");
	rc = frame_pixels("robust_combine: ", w, h, 1, px);
	if (rc != RT_OK)
		return rc;
	return robust_buffers_check(s, b, albedo, sums, 12 * *px * split, *px);
}

extern "C" {

int rt_robust_opts_default(rt_robust_opts *out)
{
	if (!out)
		return fail(RT_ERR_INVALID_ARGUMENT, "null argument");
	std::memset(out, 0, sizeof *out);
	out->mode = RT_ROBUST_GINI;
	out->trim = 1;
	out->gini_gain = 1.0f;
	return RT_OK;
}

int rt_render_robust_device(rt_scene *s, const rt_camera *camera, const rt_render_opts *o, const rt_robust_opts *r, const float *d_albedo,
                            const rt_robust_buffers *d_out, uint64_t *d_rays_shot, void *hip_stream)
{
	if (!s || !camera || !o || !r || !d_out)
		return fail(RT_ERR_INVALID_ARGUMENT, "null argument");
	uint32_t split = 0;
	uint64_t px = 0;
	int rc = robust_render_check(s, o, r, &split, &px);
	if (rc == RT_OK)
		rc = robust_buffers_check(s, d_out, d_albedo, nullptr, 0, px);
	if (rc != RT_OK)
		return rc;
	HIP_TRY(hipSetDevice(s->device));
	hipStream_t stream = static_cast<hipStream_t>(hip_stream);
	float *d_render = d_out->mean;
	if (!d_render) { // the render's frame goes to the noise stage's scratch: grows on first use only (not capturable on that call)
		Layout L;
		const auto p_render = L.add<float>(3 * px);
		RT_TRY(grow_device_buffer(s->d_noise, s->d_noise_bytes, L));
		d_render = L.at(p_render);
	}
	rt_render_opts os = *o;
	os.sample_split = split;
	rc = rt_render_device(s, camera, &os, d_render, d_rays_shot, stream);
	if (rc != RT_OK)
		return rc;
	rt_robust_buffers kernel_out = *d_out;
	kernel_out.mean = nullptr; // combine_chunks_kernel has written it
	DevRobustParams P = robust_params(r, o->width, o->height, split, (uint32_t)(o->samples_per_pixel / split), s->d_partial, d_albedo, &kernel_out);
	fill_frame_tiling(P, o);
	HIP_TRY(launch_robust_chunks(stream, P));
	return RT_OK;
}

int rt_render_robust(rt_scene *s, const rt_camera *camera, const rt_render_opts *o, const rt_robust_opts *r, const float *albedo,
                     const rt_robust_buffers *out, uint64_t *rays_shot)
{
	if (!s || !camera || !o || !r || !out)
		return fail(RT_ERR_INVALID_ARGUMENT, "null argument");
	uint32_t split = 0;
	uint64_t px = 0;
	int rc = robust_render_check(s, o, r, &split, &px);
	if (rc == RT_OK)
		rc = robust_buffers_check(s, out, albedo, nullptr, 0, px);
	if (rc != RT_OK)
		return rc;
	HIP_TRY(hipSetDevice(s->device));
	// the render's frame first (where the _device call would put its scratch), then out, the planes asked for and the albedo if given
	Layout L;
	const auto p_mean = L.add<float>(3 * px), p_out = L.add<float>(3 * px), p_gini = L.optional<float>(out->gini, px),
	           p_albedo = L.optional<float>(albedo, 3 * px);
	const auto p_trimmed = L.optional<uint8_t>(out->trimmed, px), p_dropped = L.optional<uint8_t>(out->dropped, px);
	RT_TRY(grow_device_buffer(s->d_noise, s->d_noise_bytes, L));
	Staging st{s};
	st.put(L, p_albedo, albedo);
	const rt_robust_buffers d_out = {L.at(p_out), L.at(p_mean), L.at(p_gini), L.at(p_trimmed), L.at(p_dropped)};
	if (st.ok())
		st.rc = rt_render_robust_device(s, camera, o, r, L.at(p_albedo), &d_out, reinterpret_cast<uint64_t *>(s->d_rays), s->stream);
	st.get(out->out, L, p_out);
	st.get(out->mean, L, p_mean);
	st.get(out->gini, L, p_gini);
	st.get(out->trimmed, L, p_trimmed);
	st.get(out->dropped, L, p_dropped);
	st.download(rays_shot, s->d_rays, sizeof(uint64_t));
	return st.finish("render_robust");
}

int rt_robust_combine_device(rt_scene *s, const float *d_sums, uint32_t split, uint64_t chunk_passes, uint32_t width, uint32_t height,
                             const float *d_albedo, const rt_robust_opts *r, const rt_robust_buffers *d_out, void *hip_stream)
{
	uint64_t px = 0;
	const int rc = robust_combine_check(s, d_sums, split, chunk_passes, width, height, d_albedo, r, d_out, &px);
	if (rc != RT_OK)
		return rc;
	HIP_TRY(hipSetDevice(s->device));
	HIP_TRY(launch_robust_chunks(static_cast<hipStream_t>(hip_stream),
	                             robust_params(r, width, height, split, (uint32_t)chunk_passes, d_sums, d_albedo, d_out)));
	return RT_OK;
}

int rt_robust_combine(rt_scene *s, const float *sums, uint32_t split, uint64_t chunk_passes, uint32_t width, uint32_t height,
                      const float *albedo, const rt_robust_opts *r, const rt_robust_buffers *out)
{
	uint64_t px = 0;
	int rc = robust_combine_check(s, sums, split, chunk_passes, width, height, albedo, r, out, &px);
	if (rc != RT_OK)
		return rc;
	HIP_TRY(hipSetDevice(s->device));
	Layout L;
	const auto p_sums = L.add<float>(3 * px * split), p_albedo = L.optional<float>(albedo, 3 * px), p_out = L.add<float>(3 * px),
	           p_mean = L.optional<float>(out->mean, 3 * px), p_gini = L.optional<float>(out->gini, px);
	const auto p_trimmed = L.optional<uint8_t>(out->trimmed, px), p_dropped = L.optional<uint8_t>(out->dropped, px);
	RT_TRY(grow_device_buffer(s->d_noise, s->d_noise_bytes, L));
	Staging st{s};
	st.put(L, p_sums, sums);
	st.put(L, p_albedo, albedo);
	const rt_robust_buffers d_out = {L.at(p_out), L.at(p_mean), L.at(p_gini), L.at(p_trimmed), L.at(p_dropped)};
	if (st.ok())
		st.rc = rt_robust_combine_device(s, L.at(p_sums), split, chunk_passes, width, height, L.at(p_albedo), r, &d_out, s->stream);
	st.get(out->out, L, p_out);
	st.get(out->mean, L, p_mean);
	st.get(out->gini, L, p_gini);
	st.get(out->trimmed, L, p_trimmed);
	st.get(out->dropped, L, p_dropped);
	return st.finish("robust_combine");
}

int rt_render_denoised_robust(rt_scene *s, const rt_camera *camera, const rt_render_opts *o, const rt_robust_opts *r,
                              const rt_denoise_opts *dopts, float *out_clean, float *out_robust, uint64_t *rays_shot)
{
	if (!s || !camera || !o || !r || !dopts || !out_clean)
		return fail(RT_ERR_INVALID_ARGUMENT, "null argument");
	int rc = denoise_opts_check(dopts, o->width, o->height);
	if (rc != RT_OK)
		return rc;
	uint32_t split = 0;
	uint64_t px = 0;
	rc = robust_render_check(s, o, r, &split, &px);
	if (rc != RT_OK)
		return rc;
	if (ranges_overlap(out_clean, 12 * px, out_robust, 12 * px))
		return fail(RT_ERR_INVALID_ARGUMENT, "rt_render_denoised_robust: out_clean overlaps out_robust");
	// the middle call: the robust frame (the one filtered) and the plain render behind it
	auto middle = [&](float *d_albedo, float *d_robust, float *d_mean, uint64_t *d_rays) {
		const rt_robust_buffers d_out = {d_robust, d_mean, nullptr, nullptr, nullptr};
		return rt_render_robust_device(s, camera, o, r, d_albedo, &d_out, d_rays, s->stream);
	};
	return render_denoised_guided(s, camera, o, dopts, px, 3 * px, false, middle, "render_denoised_robust", out_clean, out_robust, nullptr, rays_shot);
}

} // extern "C"

// ---- temporal accumulation with camera reprojection (rt_temporal.hip) ----
static int temporal_opts_check(const rt_temporal_opts *o)
{
	const uint64_t w = o->denoise.width, h = o->denoise.height;
	int rc = frame_sides("denoise_temporal: ", w, h, 2);
	if (rc == RT_OK)
		rc = denoise_opts_check(&o->denoise, w, h);
	if (rc != RT_OK)
		return rc;
	if (!(o->alpha_color > 0.0f && o->alpha_color <= 1.0f) || !(o->alpha_moments > 0.0f && o->alpha_moments <= 1.0f))
		return fail(RT_ERR_INVALID_ARGUMENT, "denoise_temporal: alpha_color and alpha_moments must be in (0, 1]");
	if (!std::isfinite(o->depth_tolerance) || !(o->depth_tolerance > 0.0f))
		return fail(RT_ERR_INVALID_ARGUMENT, "denoise_temporal: depth_tolerance must be finite and > 0");
	if (!(o->normal_tolerance >= -1.0f && o->normal_tolerance <= 1.0f))
		return fail(RT_ERR_INVALID_ARGUMENT, "denoise_temporal: normal_tolerance must be in [-1, 1]");
	if (o->max_history < 1)
		return fail(RT_ERR_INVALID_ARGUMENT, "denoise_temporal: max_history must be >= 1");
	return RT_OK;
}

// argument checks of rt_denoise_temporal(_device), the device last; hist_out and ws are checked for the device call only
static int temporal_check(const rt_scene *s, const rt_temporal_inputs *in, const rt_camera *cam, const rt_camera *prev,
                          const rt_temporal_opts *o, const void *hist_in, const void *hist_out, const void *ws, const float *out,
                          const float *motion, bool device)
{
	if (!s || !in || !cam || !o)
		return fail(RT_ERR_INVALID_ARGUMENT, "null argument");
	if (!in->color || !in->depth || !out)
		return fail(RT_ERR_INVALID_ARGUMENT, "denoise_temporal: color, depth and out must not be NULL");
	if (device && (!hist_out || !ws))
		return fail(RT_ERR_INVALID_ARGUMENT, "denoise_temporal: history_out and the workspace must not be NULL");
	if (hist_in && !prev)
		return fail(RT_ERR_INVALID_ARGUMENT, "denoise_temporal: a history needs the previous camera");
	int rc = temporal_opts_check(o);
	if (rc != RT_OK)
		return rc;
	const uint64_t n = (uint64_t)o->denoise.width * o->denoise.height;
	if (device) {
		const void *aligned[3] = {hist_in, hist_out, ws};
		for (const void *a : aligned)
			if (reinterpret_cast<uintptr_t>(a) % 16u != 0u)
				return fail(RT_ERR_INVALID_ARGUMENT, "denoise_temporal: the histories and the workspace must be 16-byte aligned");
	}
	// the four buffers written first
	const void *buf[9] = {out, motion, hist_out, ws, in->color, in->albedo, in->normal, in->depth, hist_in};
	const uint64_t bytes[9] = {12 * n, 8 * n, kTemporalHistoryBytesPerPixel * n, kTemporalWorkspaceBytesPerPixel * n,
	                           12 * n, 12 * n, 12 * n, 4 * n, kTemporalHistoryBytesPerPixel * n};
	rc = check_disjoint("denoise_temporal: a buffer written overlaps another buffer", buf, bytes, 4, 9);
	return rc == RT_OK ? need_device(s) : rc;
}

static int temporal_bytes(const rt_temporal_opts *o, uint64_t per_pixel, uint64_t *bytes)
{
	if (!o || !bytes)
		return fail(RT_ERR_INVALID_ARGUMENT, "null argument");
	uint64_t n = 0;
	const int rc = frame_pixels("denoise_temporal: ", o->denoise.width, o->denoise.height, 2, &n);
	if (rc == RT_OK)
		*bytes = per_pixel * n;
	return rc;
}

extern "C" {

int rt_temporal_opts_default(rt_temporal_opts *out)
{
	if (!out)
		return fail(RT_ERR_INVALID_ARGUMENT, "null argument");
	std::memset(out, 0, sizeof *out);
	rt_denoise_opts_default(&out->denoise);
	out->alpha_color = 0.2f;
	out->alpha_moments = 0.2f;
	out->depth_tolerance = 0.1f;
	out->normal_tolerance = 0.9f;
	out->max_history = 32;
	return RT_OK;
}

int rt_temporal_history_bytes(const rt_temporal_opts *o, uint64_t *bytes)
{
	return temporal_bytes(o, kTemporalHistoryBytesPerPixel, bytes);
}

int rt_temporal_workspace_bytes(const rt_temporal_opts *o, uint64_t *bytes)
{
	return temporal_bytes(o, kTemporalWorkspaceBytesPerPixel, bytes);
}

int rt_denoise_temporal_device(rt_scene *s, const rt_temporal_inputs *d_in, const rt_camera *cam, const rt_camera *prev_cam,
                               const void *d_history_in, void *d_history_out, const rt_temporal_opts *o, void *d_workspace,
                               float *d_out, float *d_motion, void *hip_stream)
{
	int rc = temporal_check(s, d_in, cam, prev_cam, o, d_history_in, d_history_out, d_workspace, d_out, d_motion, true);
	if (rc != RT_OK)
		return rc;
	HIP_TRY(hipSetDevice(s->device)); // a multi-device head runs on devices[0]
	const uint64_t w = o->denoise.width, h = o->denoise.height;
	const size_t n = (size_t)(w * h);
	DevTemporalParams T;
	std::memset(&T, 0, sizeof T);
	T.width = (uint32_t)w;
	T.height = (uint32_t)h;
	std::memcpy(T.cam, cam, sizeof T.cam);
	if (d_history_in)
		std::memcpy(T.prev, prev_cam, sizeof T.prev);
	T.alpha_c = o->alpha_color;
	T.alpha_m = o->alpha_moments;
	T.depth_tol = o->depth_tolerance;
	T.normal_tol = o->normal_tolerance;
	T.max_history = (float)o->max_history;
	T.color = d_in->color;
	T.albedo = d_in->albedo;
	T.normal = d_in->normal;
	T.depth = d_in->depth;
	T.hist_in = static_cast<const float4 *>(d_history_in);
	T.hist_out = static_cast<float4 *>(d_history_out);
	T.motion = d_motion;
	const rt_denoise_inputs din = {d_in->color, d_in->albedo, d_in->normal, d_in->depth, nullptr};
	DevDenoiseParams D = denoise_params(&o->denoise, w, h, din, d_workspace, d_out);
	D.guide = T.hist_out + n; // H1 of the history written is the guide plane
	HIP_TRY(launch_temporal(static_cast<hipStream_t>(hip_stream), T, D));
	return RT_OK;
}

int rt_denoise_temporal(rt_scene *s, const rt_temporal_inputs *in, const rt_camera *cam, const rt_temporal_opts *o, float *out,
                        float *motion)
{
	int rc = temporal_check(s, in, cam, nullptr, o, nullptr, nullptr, nullptr, out, motion, false);
	if (rc != RT_OK)
		return rc;
	HIP_TRY(hipSetDevice(s->device));
	const uint32_t w = o->denoise.width, h = o->denoise.height;
	const uint64_t n = (uint64_t)w * h;
	Layout H; // the two histories, alone in their buffer: the same description puts them at the same place in every call
	const Layout::Part<char> p_hist[2] = {H.bytes(kTemporalHistoryBytesPerPixel * n), H.bytes(kTemporalHistoryBytesPerPixel * n)};
	if (w != s->temporal_w || h != s->temporal_h) { // a new frame size: new histories, no history
		s->temporal_w = s->temporal_h = 0;
		s->temporal_cur = -1;
		size_t held = 0; // (always replaced: the buffer is two histories of exactly w x h)
		RT_TRY(grow_device_buffer(s->d_temporal, held, H));
		s->temporal_w = w;
		s->temporal_h = h;
	}
	// the workspace, out, motion if asked for, then the inputs given, in rt_temporal_inputs order
	Layout L;
	const auto p_ws = L.bytes(kTemporalWorkspaceBytesPerPixel * n);
	const auto p_out = L.add<float>(3 * n), p_motion = L.optional<float>(motion, 2 * n), p_color = L.add<float>(3 * n),
	           p_albedo = L.optional<float>(in->albedo, 3 * n), p_normal = L.optional<float>(in->normal, 3 * n), p_depth = L.add<float>(n);
	RT_TRY(grow_device_buffer(s->d_denoise, s->d_denoise_bytes, L)); // shared with rt_denoise / rt_render_denoised
	Staging st{s};
	st.put(L, p_color, in->color);
	st.put(L, p_albedo, in->albedo);
	st.put(L, p_normal, in->normal);
	st.put(L, p_depth, in->depth);
	if (!st.ok())
		return st.finish("denoise_temporal upload");
	const rt_temporal_inputs d_in = {L.at(p_color), L.at(p_albedo), L.at(p_normal), L.at(p_depth)};
	H.base = s->d_temporal;
	char *hist[2] = {H.at(p_hist[0]), H.at(p_hist[1])};
	const int next = s->temporal_cur == 0 ? 1 : 0;
	const void *h_in = s->temporal_cur >= 0 ? hist[s->temporal_cur] : nullptr;
	s->temporal_cur = -1; // until this call has succeeded
	st.rc = rt_denoise_temporal_device(s, &d_in, cam, &s->temporal_prev, h_in, hist[next], o, L.at(p_ws), L.at(p_out),
	                                   L.at(p_motion), s->stream);
	st.get(out, L, p_out);
	st.get(motion, L, p_motion);
	rc = st.finish("denoise_temporal");
	if (rc == RT_OK) {
		s->temporal_cur = next;
		s->temporal_prev = *cam;
	}
	return rc;
}

int rt_denoise_temporal_reset(rt_scene *s)
{
	if (!s)
		return fail(RT_ERR_INVALID_ARGUMENT, "null argument");
	s->temporal_cur = -1;
	return RT_OK;
}

} // extern "C"

// ---- display stage: histogram, auto-exposure, tone curve, transfer, quantisation (rt_display.hip) ----
static bool finite_f(float v) { return std::isfinite(v); }

static int display_opts_check(const rt_display_opts *o)
{
	if (int rc = frame_sides("display: ", o->width, o->height, 1); rc != RT_OK)
		return rc;
	if (o->exposure_mode < RT_EXPOSURE_FIXED || o->exposure_mode > RT_EXPOSURE_AUTO)
		return fail(RT_ERR_INVALID_ARGUMENT, "display: unknown exposure_mode");
	if (o->tonemap < RT_TONEMAP_CLAMP || o->tonemap > RT_TONEMAP_HABLE)
		return fail(RT_ERR_INVALID_ARGUMENT, "display: unknown tonemap");
	if (o->transfer < RT_TRANSFER_SRGB || o->transfer > RT_TRANSFER_LINEAR)
		return fail(RT_ERR_INVALID_ARGUMENT, "display: unknown transfer");
	if (o->quantiser < RT_QUANT_ROUND || o->quantiser > RT_QUANT_REFERENCE)
		return fail(RT_ERR_INVALID_ARGUMENT, "display: unknown quantiser");
	if (o->pixel_format < RT_PIXEL_RGBA8 || o->pixel_format > RT_PIXEL_RGB8)
		return fail(RT_ERR_INVALID_ARGUMENT, "display: unknown pixel_format");
	if (!finite_f(o->exposure_ev) || !finite_f(o->key_ev))
		return fail(RT_ERR_INVALID_ARGUMENT, "display: exposure_ev and key_ev must be finite");
	if (!(o->meter_low >= 0.0f && o->meter_low < o->meter_high && o->meter_high <= 1.0f))
		return fail(RT_ERR_INVALID_ARGUMENT, "display: need 0 <= meter_low < meter_high <= 1");
	if (!finite_f(o->ev_min) || !finite_f(o->ev_max) || !(o->ev_min <= o->ev_max))
		return fail(RT_ERR_INVALID_ARGUMENT, "display: ev_min and ev_max must be finite with ev_min <= ev_max");
	if (!(o->adaptation > 0.0f && o->adaptation <= 1.0f))
		return fail(RT_ERR_INVALID_ARGUMENT, "display: adaptation must be in (0, 1]");
	if (!finite_f(o->white) || !(o->white > 0.0f))
		return fail(RT_ERR_INVALID_ARGUMENT, "display: white must be finite and > 0");
	if (!finite_f(o->gamma) || !(o->gamma > 0.0f))
		return fail(RT_ERR_INVALID_ARGUMENT, "display: gamma must be finite and > 0");
	uint64_t n = 0;
	return frame_pixels("display: ", o->width, o->height, 1, &n);
}

static uint64_t display_out_bytes(const rt_display_opts *o)
{
	return (uint64_t)o->width * o->height * (o->pixel_format == RT_PIXEL_RGB8 ? 3u : 4u);
}

// argument checks of rt_display(_device), the device last; ws is checked for the device call only
static int display_check(const rt_scene *s, const float *rgb, const rt_display_opts *o, const void *state, const void *ws,
                         const void *out, const void *histogram, bool device)
{
	if (!s || !rgb || !o || !out)
		return fail(RT_ERR_INVALID_ARGUMENT, "null argument");
	int rc = display_opts_check(o);
	if (rc != RT_OK)
		return rc;
	const uint64_t n = (uint64_t)o->width * o->height;
	if (device && (!ws || reinterpret_cast<uintptr_t>(ws) % 16u != 0u))
		return fail(RT_ERR_INVALID_ARGUMENT, "display: the workspace must not be NULL and must be 16-byte aligned");
	// every buffer written (out, histogram, state, workspace) against every other buffer
	const void *buf[5] = {out, histogram, state, device ? ws : nullptr, rgb};
	const uint64_t bytes[5] = {display_out_bytes(o), 4ull * kDisplayBins, sizeof(rt_display_state), display_workspace_bytes(n), 12 * n};
	rc = check_disjoint("display: a buffer written overlaps another buffer", buf, bytes, 4, 5);
	return rc == RT_OK ? need_device(s) : rc;
}

extern "C" {

int rt_display_opts_default(rt_display_opts *out)
{
	if (!out)
		return fail(RT_ERR_INVALID_ARGUMENT, "null argument");
	std::memset(out, 0, sizeof *out);
	out->exposure_mode = RT_EXPOSURE_AUTO;
	out->tonemap = RT_TONEMAP_ACES;
	out->transfer = RT_TRANSFER_SRGB;
	out->quantiser = RT_QUANT_DITHER;
	out->pixel_format = RT_PIXEL_RGBA8;
	out->exposure_ev = 0.0f;
	out->key_ev = -2.47393119f; // log2(0.18)
	out->meter_low = 0.10f;
	out->meter_high = 0.90f;
	out->ev_min = -16.0f;
	out->ev_max = 16.0f;
	out->adaptation = 1.0f;
	out->white = 4.0f;
	out->gamma = 2.2f;
	return RT_OK;
}

int rt_display_workspace_bytes(const rt_display_opts *o, uint64_t *bytes)
{
	if (!o || !bytes)
		return fail(RT_ERR_INVALID_ARGUMENT, "null argument");
	uint64_t n = 0;
	const int rc = frame_pixels("display: ", o->width, o->height, 1, &n);
	if (rc == RT_OK)
		*bytes = display_workspace_bytes(n);
	return rc;
}

int rt_display_output_bytes(const rt_display_opts *o, uint64_t *bytes)
{
	if (!o || !bytes)
		return fail(RT_ERR_INVALID_ARGUMENT, "null argument");
	uint64_t n = 0;
	int rc = frame_sides("display: ", o->width, o->height, 1);
	if (rc == RT_OK && (o->pixel_format < RT_PIXEL_RGBA8 || o->pixel_format > RT_PIXEL_RGB8))
		rc = fail(RT_ERR_INVALID_ARGUMENT, "display: unknown pixel_format");
	if (rc == RT_OK)
		rc = frame_pixels("display: ", o->width, o->height, 1, &n);
	if (rc == RT_OK)
		*bytes = display_out_bytes(o);
	return rc;
}

int rt_display_device(rt_scene *s, const float *d_rgb, const rt_display_opts *o, rt_display_state *d_state, void *d_workspace,
                      void *d_out, uint32_t *d_histogram, void *hip_stream)
{
	int rc = display_check(s, d_rgb, o, d_state, d_workspace, d_out, d_histogram, true);
	if (rc != RT_OK)
		return rc;
	HIP_TRY(hipSetDevice(s->device)); // a multi-device head runs on devices[0]
	DevDisplayParams P;
	std::memset(&P, 0, sizeof P);
	P.n_px = o->width * o->height;
	P.width = o->width;
	P.mode = o->exposure_mode;
	P.tonemap = o->tonemap;
	P.transfer = o->transfer;
	P.quantiser = o->quantiser;
	P.format = o->pixel_format;
	P.exposure_ev = o->exposure_ev;
	P.key_ev = o->key_ev;
	P.meter_low = o->meter_low;
	P.meter_high = o->meter_high;
	P.ev_min = o->ev_min;
	P.ev_max = o->ev_max;
	P.adaptation = o->adaptation;
	P.white2 = o->white * o->white;
	P.hable_fw = display_hable(o->white);
	P.inv_gamma = 1.0f / o->gamma;
	P.seed_lo = (uint32_t)o->seed;
	P.seed_hi = (uint32_t)(o->seed >> 32);
	P.rgb = d_rgb;
	P.state = d_state;
	P.ws = static_cast<char *>(d_workspace);
	P.out = d_out;
	P.histogram = d_histogram;
	HIP_TRY(launch_display(static_cast<hipStream_t>(hip_stream), P));
	return RT_OK;
}

int rt_display(rt_scene *s, const float *host_rgb, const rt_display_opts *o, void *host_out, rt_display_state *host_state,
               uint32_t *host_histogram)
{
	int rc = display_check(s, host_rgb, o, host_state, nullptr, host_out, host_histogram, false);
	if (rc != RT_OK)
		return rc;
	HIP_TRY(hipSetDevice(s->device));
	const uint64_t n = (uint64_t)o->width * o->height;
	// the state first (so that it is found again whatever the frame size), the histogram, workspace, output, input
	Layout L;
	const auto p_state = L.add<rt_display_state>(1);
	const auto p_hist = L.add<uint32_t>(kDisplayBins);
	const auto p_ws = L.bytes(display_workspace_bytes(n)), p_out = L.bytes(display_out_bytes(o));
	const auto p_in = L.add<float>(3 * n);
	if (L.total() > s->d_display_bytes) { // grown for larger frames only; the state is kept on the host side meanwhile
		rt_display_state keep{};
		if (s->d_display && s->display_has_state)
			HIP_TRY(hipMemcpy(&keep, s->d_display, sizeof keep, hipMemcpyDeviceToHost)); // (the state is the first part)
		RT_TRY(grow_device_buffer(s->d_display, s->d_display_bytes, L));
		HIP_TRY(hipMemcpy(s->d_display, &keep, sizeof keep, hipMemcpyHostToDevice));
	}
	L.base = s->d_display;
	rt_display_state *d_state = L.at(p_state);
	const bool fresh = !s->display_has_state || o->width != s->display_w || o->height != s->display_h;
	s->display_has_state = false; // until this call has succeeded
	Staging st{s};
	if (fresh)
		st.e = hipMemsetAsync(d_state, 0, sizeof(rt_display_state), s->stream);
	st.put(L, p_in, host_rgb);
	if (!st.ok())
		return st.finish("display upload");
	st.rc = rt_display_device(s, L.at(p_in), o, d_state, L.at(p_ws), L.at(p_out), L.at(p_hist), s->stream);
	st.get(host_out, L, p_out);
	st.get(host_state, L, p_state);
	st.get(host_histogram, L, p_hist);
	rc = st.finish("display");
	if (rc == RT_OK) {
		s->display_has_state = true;
		s->display_w = o->width;
		s->display_h = o->height;
	}
	return rc;
}

int rt_display_reset(rt_scene *s)
{
	if (!s)
		return fail(RT_ERR_INVALID_ARGUMENT, "null argument");
	s->display_has_state = false;
	return RT_OK;
}

} // extern "C"

// ---- depth-of-field stage: circle of confusion from depth, occlusion-aware disc gather (rt_dof.hip) ----
// the options for a frame of w x h (rt_render_dof takes the size from the render); with_camera: one was given
static int dof_opts_check(const rt_dof_opts *o, uint64_t w, uint64_t h, bool with_camera)
{
	if (int rc = frame_sides("dof: ", w, h, 1); rc != RT_OK)
		return rc;
	if (!finite_f(o->focus_distance) || !(o->focus_distance > 0.0f))
		return fail(RT_ERR_INVALID_ARGUMENT, "dof: focus_distance must be finite and > 0");
	if (!finite_f(o->blur_scale) || !(o->blur_scale >= 0.0f))
		return fail(RT_ERR_INVALID_ARGUMENT, "dof: blur_scale must be finite and >= 0");
	if (o->max_radius < 1u || o->max_radius > kDofMaxRadius)
		return fail(RT_ERR_INVALID_ARGUMENT, "dof: max_radius must be in 1..16");
	if (o->planar_depth > 1u)
		return fail(RT_ERR_INVALID_ARGUMENT, "dof: planar_depth must be 0 or 1");
	if (o->planar_depth == 1u && !with_camera)
		return fail(RT_ERR_INVALID_ARGUMENT, "dof: planar_depth 1 needs a camera");
	if (o->planar_depth == 1u && (w < 2 || h < 2))
		return fail(RT_ERR_INVALID_ARGUMENT, "dof: planar_depth 1 needs width and height >= 2 (u and v divide by W-1 and H-1)");
	for (uint32_t r : o->reserved)
		if (r != 0u)
			return fail(RT_ERR_INVALID_ARGUMENT, "dof: reserved must be zero");
	uint64_t n = 0;
	return frame_pixels("dof: ", w, h, 1, &n);
}

// argument checks of rt_dof(_device), the device last; ws is checked for the device call only
static int dof_check(const rt_scene *s, const float *rgb, const float *depth, const rt_camera *camera, const rt_dof_opts *o, const void *ws,
                     const float *out, const float *coc, bool device)
{
	if (!s || !rgb || !depth || !o || !out)
		return fail(RT_ERR_INVALID_ARGUMENT, "null argument");
	int rc = dof_opts_check(o, o->width, o->height, camera != nullptr);
	if (rc != RT_OK)
		return rc;
	const uint64_t n = (uint64_t)o->width * o->height;
	if (device && (!ws || reinterpret_cast<uintptr_t>(ws) % 16u != 0u))
		return fail(RT_ERR_INVALID_ARGUMENT, "dof: the workspace must not be NULL and must be 16-byte aligned");
	// every pair of buffers: the gather reads the neighbours of the pixel it writes, so nothing may be shared, out == rgb included
	const void *buf[5] = {out, coc, device ? ws : nullptr, rgb, depth};
	const uint64_t bytes[5] = {12 * n, 4 * n, dof_workspace_bytes(n), 12 * n, 4 * n};
	rc = check_disjoint("dof: two buffers overlap (in place is not supported: the gather reads neighbours)", buf, bytes, 5, 5);
	return rc == RT_OK ? need_device(s) : rc;
}

static DevDofParams dof_params(const rt_dof_opts *o, uint64_t w, uint64_t h, const rt_camera *camera, const float *rgb, const float *depth,
                               void *ws, float *out, float *coc)
{
	DevDofParams P;
	std::memset(&P, 0, sizeof P);
	P.width = (uint32_t)w;
	P.height = (uint32_t)h;
	P.focus_distance = o->focus_distance;
	P.blur_scale = o->blur_scale;
	P.max_radius = o->max_radius;
	P.planar = o->planar_depth;
	if (camera)
		std::memcpy(P.cam, camera, sizeof P.cam); // origin, lower_left, horizontal, vertical
	P.rgb = rgb;
	P.depth = depth;
	P.ws = static_cast<float2 *>(ws);
	P.out = out;
	P.coc = coc;
	return P;
}

// the scene's buffer for a frame of n pixels: workspace, output, CoC plane, frame, depth
struct DofFrames {
	char *ws;
	float *out, *coc, *rgb, *depth;
};
static int dof_frames(rt_scene *s, uint64_t n, DofFrames *F)
{
	Layout L;
	const auto p_ws = L.bytes(dof_workspace_bytes(n));
	const auto p_out = L.add<float>(3 * n), p_coc = L.add<float>(n), p_rgb = L.add<float>(3 * n), p_depth = L.add<float>(n);
	RT_TRY(grow_device_buffer(s->d_dof, s->d_dof_bytes, L));
	*F = DofFrames{L.at(p_ws), L.at(p_out), L.at(p_coc), L.at(p_rgb), L.at(p_depth)};
	return RT_OK;
}

extern "C" {

int rt_dof_opts_default(rt_dof_opts *out)
{
	if (!out)
		return fail(RT_ERR_INVALID_ARGUMENT, "null argument");
	std::memset(out, 0, sizeof *out);
	out->focus_distance = 10.0f;
	out->blur_scale = 0.0f;
	out->max_radius = 8;
	out->planar_depth = 1;
	return RT_OK;
}

int rt_dof_opts_from_camera(rt_dof_opts *out, const rt_camera *camera, float aperture, float focus_dist, uint32_t width, uint32_t height)
{
	if (!out || !camera)
		return fail(RT_ERR_INVALID_ARGUMENT, "null argument");
	if (!finite_f(aperture) || !(aperture >= 0.0f))
		return fail(RT_ERR_INVALID_ARGUMENT, "dof: aperture must be finite and >= 0");
	if (!finite_f(focus_dist) || !(focus_dist > 0.0f))
		return fail(RT_ERR_INVALID_ARGUMENT, "dof: focus_dist must be finite and > 0");
	if (width < 2u || height < 2u)
		return fail(RT_ERR_INVALID_ARGUMENT, "dof: width and height must be >= 2 (u and v divide by W-1 and H-1)");
	const float *hz = camera->horizontal;
	const float len = std::sqrt((hz[0] * hz[0] + hz[1] * hz[1]) + hz[2] * hz[2]);
	const float scale = ((aperture * 0.5f) * (float)(width - 1u)) / len;
	if (!finite_f(scale))
		return fail(RT_ERR_INVALID_ARGUMENT, "dof: the camera's horizontal axis must be finite and not zero");
	rt_dof_opts_default(out);
	out->width = width;
	out->height = height;
	out->focus_distance = focus_dist;
	out->blur_scale = scale;
	out->planar_depth = 1;
	return RT_OK;
}

int rt_dof_workspace_bytes(const rt_dof_opts *o, uint64_t *bytes)
{
	if (!o || !bytes)
		return fail(RT_ERR_INVALID_ARGUMENT, "null argument");
	uint64_t n = 0;
	const int rc = frame_pixels("dof: ", o->width, o->height, 1, &n);
	if (rc == RT_OK)
		*bytes = dof_workspace_bytes(n);
	return rc;
}

int rt_dof_device(rt_scene *s, const float *d_rgb, const float *d_depth, const rt_camera *camera, const rt_dof_opts *o, void *d_workspace,
                  float *d_out, float *d_coc, void *hip_stream)
{
	int rc = dof_check(s, d_rgb, d_depth, camera, o, d_workspace, d_out, d_coc, true);
	if (rc != RT_OK)
		return rc;
	HIP_TRY(hipSetDevice(s->device)); // a multi-device head runs on devices[0]
	HIP_TRY(launch_dof(static_cast<hipStream_t>(hip_stream), dof_params(o, o->width, o->height, camera, d_rgb, d_depth, d_workspace, d_out, d_coc)));
	return RT_OK;
}

int rt_dof(rt_scene *s, const float *host_rgb, const float *host_depth, const rt_camera *camera, const rt_dof_opts *o, float *host_out,
           float *host_coc)
{
	int rc = dof_check(s, host_rgb, host_depth, camera, o, nullptr, host_out, host_coc, false);
	if (rc != RT_OK)
		return rc;
	HIP_TRY(hipSetDevice(s->device));
	const uint64_t n = (uint64_t)o->width * o->height;
	DofFrames F;
	rc = dof_frames(s, n, &F);
	if (rc != RT_OK)
		return rc;
	Staging st{s};
	st.to_device(F.rgb, host_rgb, 12 * n);
	st.to_device(F.depth, host_depth, 4 * n);
	if (!st.ok())
		return st.finish("dof upload");
	st.rc = rt_dof_device(s, F.rgb, F.depth, camera, o, F.ws, F.out, host_coc ? F.coc : nullptr, s->stream);
	st.download(host_out, F.out, 12 * n);
	st.download(host_coc, F.coc, 4 * n);
	return st.finish("dof");
}

int rt_render_dof(rt_scene *s, const rt_camera *camera, const rt_render_opts *o, const rt_dof_opts *dopts, float *out)
{
	if (!s || !camera || !o || !dopts || !out)
		return fail(RT_ERR_INVALID_ARGUMENT, "null argument");
	int rc = dof_opts_check(dopts, o->width, o->height, true);
	if (rc == RT_OK)
		rc = aov_opts_check(o);
	if (rc != RT_OK)
		return rc;
	if (o->render_method != RT_METHOD_NAIVE && o->render_method != RT_METHOD_MIS)
		return fail(RT_ERR_INVALID_ARGUMENT, "unknown render method");
	rc = need_device(s);
	if (rc != RT_OK)
		return rc;
	HIP_TRY(hipSetDevice(s->device));
	const uint64_t n = o->width * o->height;
	DofFrames F;
	rc = dof_frames(s, n, &F);
	if (rc != RT_OK)
		return rc;
	Staging st{s};
	st.rc = rt_render_device(s, camera, o, F.rgb, nullptr, s->stream);
	if (st.ok())
		st.e = hipSetDevice(s->device);
	enqueue_guides(s, camera, o, nullptr, nullptr, F.depth, st);
	if (st.ok())
		st.e = launch_dof(s->stream, dof_params(dopts, o->width, o->height, camera, F.rgb, F.depth, F.ws, F.out, nullptr));
	st.download(out, F.out, 12 * n);
	return st.finish("render_dof");
}

} // extern "C"

// ---- bloom stage: bright pass, reduce / expand pyramid, composite (rt_bloom.hip) ----
static int bloom_opts_check(const rt_bloom_opts *o)
{
	if (int rc = frame_sides("bloom: ", o->width, o->height, 1); rc != RT_OK)
		return rc;
	if (!finite_f(o->threshold) || !(o->threshold >= 0.0f))
		return fail(RT_ERR_INVALID_ARGUMENT, "bloom: threshold must be finite and >= 0");
	if (!(o->knee >= 0.0f && o->knee <= 1.0f))
		return fail(RT_ERR_INVALID_ARGUMENT, "bloom: knee must be in [0, 1]");
	if (!finite_f(o->intensity) || !(o->intensity >= 0.0f))
		return fail(RT_ERR_INVALID_ARGUMENT, "bloom: intensity must be finite and >= 0");
	if (!(o->scatter >= 0.0f && o->scatter <= 1.0f))
		return fail(RT_ERR_INVALID_ARGUMENT, "bloom: scatter must be in [0, 1]");
	if (o->levels < 1u || o->levels > kBloomMaxLevels)
		return fail(RT_ERR_INVALID_ARGUMENT, "bloom: levels must be in 1..12");
	if (!finite_f(o->exposure_ev))
		return fail(RT_ERR_INVALID_ARGUMENT, "bloom: exposure_ev must be finite");
	if (!finite_f(o->clamp_max) || !(o->clamp_max > 0.0f))
		return fail(RT_ERR_INVALID_ARGUMENT, "bloom: clamp_max must be finite and > 0");
	if (o->fuse_tail > 1u)
		return fail(RT_ERR_INVALID_ARGUMENT, "bloom: fuse_tail must be 0 or 1");
	for (uint32_t r : o->reserved)
		if (r != 0u)
			return fail(RT_ERR_INVALID_ARGUMENT, "bloom: reserved must be zero");
	uint64_t n = 0;
	return frame_pixels("bloom: ", o->width, o->height, 1, &n);
}

// argument checks of rt_bloom(_device), the device last; ws is checked for the device call only
static int bloom_check(const rt_scene *s, const float *rgb, const rt_bloom_opts *o, const void *state, const void *ws, const float *out,
                       bool device)
{
	if (!s || !rgb || !o || !out)
		return fail(RT_ERR_INVALID_ARGUMENT, "null argument");
	int rc = bloom_opts_check(o);
	if (rc != RT_OK)
		return rc;
	const uint64_t n = (uint64_t)o->width * o->height;
	if (device && (!ws || reinterpret_cast<uintptr_t>(ws) % 16u != 0u))
		return fail(RT_ERR_INVALID_ARGUMENT, "bloom: the workspace must not be NULL and must be 16-byte aligned");
	// every pair of buffers; out may BE the frame (the composite reads only its own pixel of it), nothing else may be shared
	const void *buf[4] = {out, device ? ws : nullptr, state, rgb};
	const uint64_t bytes[4] = {12 * n, bloom_levels(o->width, o->height, o->levels).bytes, sizeof(rt_display_state), 12 * n};
	for (int a = 0; a < 4; ++a)
		for (int b = a + 1; b < 4; ++b)
			if (!(a == 0 && b == 3 && out == rgb) && ranges_overlap(buf[a], bytes[a], buf[b], bytes[b]))
				return fail(RT_ERR_INVALID_ARGUMENT, "bloom: two buffers overlap (only out == rgb is allowed)");
	return need_device(s);
}

extern "C" {

int rt_bloom_opts_default(rt_bloom_opts *out)
{
	if (!out)
		return fail(RT_ERR_INVALID_ARGUMENT, "null argument");
	std::memset(out, 0, sizeof *out);
	out->threshold = 1.0f;
	out->knee = 0.5f;
	out->intensity = 0.05f;
	out->scatter = 0.7f;
	out->levels = 6;
	out->exposure_ev = 0.0f;
	out->clamp_max = 65504.0f;
	out->fuse_tail = 1;
	return RT_OK;
}

int rt_bloom_workspace_bytes(const rt_bloom_opts *o, uint64_t *bytes)
{
	if (!o || !bytes)
		return fail(RT_ERR_INVALID_ARGUMENT, "null argument");
	if (o->levels < 1u || o->levels > kBloomMaxLevels)
		return fail(RT_ERR_INVALID_ARGUMENT, "bloom: levels must be in 1..12");
	uint64_t n = 0;
	const int rc = frame_pixels("bloom: ", o->width, o->height, 1, &n);
	if (rc == RT_OK)
		*bytes = bloom_levels(o->width, o->height, o->levels).bytes;
	return rc;
}

int rt_bloom_device(rt_scene *s, const float *d_rgb, const rt_bloom_opts *o, const rt_display_state *d_state, void *d_workspace,
                    float *d_out, void *hip_stream)
{
	int rc = bloom_check(s, d_rgb, o, d_state, d_workspace, d_out, true);
	if (rc != RT_OK)
		return rc;
	HIP_TRY(hipSetDevice(s->device)); // a multi-device head runs on devices[0]
	DevBloomParams P;
	std::memset(&P, 0, sizeof P);
	P.width = o->width;
	P.height = o->height;
	P.threshold = o->threshold;
	P.knee = o->knee;
	P.intensity = o->intensity;
	P.scatter = o->scatter;
	P.exposure_ev = o->exposure_ev;
	P.clamp_max = o->clamp_max;
	P.fuse_tail = o->fuse_tail;
	P.rgb = d_rgb;
	P.state = d_state;
	P.ws = static_cast<char *>(d_workspace);
	P.out = d_out;
	HIP_TRY(launch_bloom(static_cast<hipStream_t>(hip_stream), P, bloom_levels(o->width, o->height, o->levels)));
	return RT_OK;
}

int rt_bloom(rt_scene *s, const float *host_rgb, const rt_bloom_opts *o, const rt_display_state *host_state, float *host_out)
{
	int rc = bloom_check(s, host_rgb, o, host_state, nullptr, host_out, false);
	if (rc != RT_OK)
		return rc;
	HIP_TRY(hipSetDevice(s->device));
	const uint64_t n = (uint64_t)o->width * o->height;
	// the state if given, workspace, output, input
	Layout L;
	const auto p_state = L.optional<rt_display_state>(host_state, 1);
	const auto p_ws = L.bytes(bloom_levels(o->width, o->height, o->levels).bytes);
	const auto p_out = L.add<float>(3 * n), p_in = L.add<float>(3 * n);
	RT_TRY(grow_device_buffer(s->d_bloom, s->d_bloom_bytes, L));
	Staging st{s};
	st.put(L, p_state, host_state);
	st.put(L, p_in, host_rgb);
	if (!st.ok())
		return st.finish("bloom upload");
	st.rc = rt_bloom_device(s, L.at(p_in), o, L.at(p_state), L.at(p_ws), L.at(p_out), s->stream);
	st.get(host_out, L, p_out);
	return st.finish("bloom");
}

} // extern "C"

// ---- AOV-guided upscaling (rt_upscale.hip) ----
// the two frame sizes and the options; sizes are passed separately (rt_render_upscaled takes them from the render)
static int upscale_opts_check(const rt_upscale_opts *o, uint64_t w, uint64_t h, uint64_t W, uint64_t H)
{
	int rc = frame_sides("upscale: source ", w, h, 2);
	if (rc == RT_OK)
		rc = frame_sides("upscale: destination ", W, H, 2);
	if (rc != RT_OK)
		return rc;
	if (!std::isfinite(o->sigma_normal) || !(o->sigma_normal > 0.0f) || !std::isfinite(o->depth_tolerance) || !(o->depth_tolerance > 0.0f))
		return fail(RT_ERR_INVALID_ARGUMENT, "upscale: sigma_normal and depth_tolerance must be finite and > 0");
	if (W < w || H < h)
		return fail(RT_ERR_UNSUPPORTED, "upscale: the destination is smaller than the source (this is not a downscaler)");
	uint64_t n = 0;
	return frame_pixels("upscale: ", W, H, 2, &n);
}

// argument checks of rt_upscale(_device), the device last
static int upscale_check(const rt_scene *s, const rt_upscale_inputs *in, const rt_upscale_opts *o, const float *out, const uint8_t *stage)
{
	if (!s || !in || !o)
		return fail(RT_ERR_INVALID_ARGUMENT, "null argument");
	if (!in->color || !out)
		return fail(RT_ERR_INVALID_ARGUMENT, "upscale: color and out must not be NULL");
	if (!in->src_albedo != !in->dst_albedo || !in->src_normal != !in->dst_normal || !in->src_depth != !in->dst_depth)
		return fail(RT_ERR_INVALID_ARGUMENT, "upscale: a guide must be given at both sizes or at neither");
	int rc = upscale_opts_check(o, o->src_width, o->src_height, o->dst_width, o->dst_height);
	if (rc != RT_OK)
		return rc;
	const uint64_t n = (uint64_t)o->src_width * o->src_height, N = (uint64_t)o->dst_width * o->dst_height;
	// the two buffers written against every other buffer (the inputs may share memory with one another)
	const void *buf[9] = {out, stage, in->color, in->src_albedo, in->src_normal, in->src_depth, in->dst_albedo, in->dst_normal, in->dst_depth};
	const uint64_t bytes[9] = {12 * N, N, 12 * n, 12 * n, 12 * n, 4 * n, 12 * N, 12 * N, 4 * N};
	rc = check_disjoint("upscale: out or the stage map overlaps another buffer", buf, bytes, 2, 9);
	return rc == RT_OK ? need_device(s) : rc;
}

static DevUpscaleParams upscale_params(const rt_upscale_opts *o, uint64_t w, uint64_t h, uint64_t W, uint64_t H, const rt_upscale_inputs &in,
                                       float *out, uint8_t *stage)
{
	DevUpscaleParams P;
	std::memset(&P, 0, sizeof P);
	P.w = (uint32_t)w;
	P.h = (uint32_t)h;
	P.W = (uint32_t)W;
	P.H = (uint32_t)H;
	P.sigma_n = o->sigma_normal;
	P.depth_tol = o->depth_tolerance;
	P.color = in.color;
	P.src_albedo = in.src_albedo;
	P.src_normal = in.src_normal;
	P.src_depth = in.src_depth;
	P.dst_albedo = in.dst_albedo;
	P.dst_normal = in.dst_normal;
	P.dst_depth = in.dst_depth;
	P.out = out;
	P.stage = stage;
	return P;
}

extern "C" {

int rt_upscale_opts_default(rt_upscale_opts *out)
{
	if (!out)
		return fail(RT_ERR_INVALID_ARGUMENT, "null argument");
	std::memset(out, 0, sizeof *out);
	out->sigma_normal = 32.0f;
	out->depth_tolerance = 0.1f;
	return RT_OK;
}

int rt_upscale_device(rt_scene *s, const rt_upscale_inputs *d_in, const rt_upscale_opts *o, float *d_out, uint8_t *d_stage, void *hip_stream)
{
	int rc = upscale_check(s, d_in, o, d_out, d_stage);
	if (rc != RT_OK)
		return rc;
	HIP_TRY(hipSetDevice(s->device)); // a multi-device head runs on devices[0]
	HIP_TRY(launch_upscale(static_cast<hipStream_t>(hip_stream),
	                       upscale_params(o, o->src_width, o->src_height, o->dst_width, o->dst_height, *d_in, d_out, d_stage)));
	return RT_OK;
}

int rt_upscale(rt_scene *s, const rt_upscale_inputs *in, const rt_upscale_opts *o, float *out, uint8_t *stage)
{
	int rc = upscale_check(s, in, o, out, stage);
	if (rc != RT_OK)
		return rc;
	HIP_TRY(hipSetDevice(s->device));
	const uint64_t n = (uint64_t)o->src_width * o->src_height, N = (uint64_t)o->dst_width * o->dst_height;
	// out first, then the inputs given, in rt_upscale_inputs order, then the stage map if asked for
	const void *host[7] = {in->color, in->src_albedo, in->src_normal, in->src_depth, in->dst_albedo, in->dst_normal, in->dst_depth};
	const uint64_t floats[7] = {3 * n, 3 * n, 3 * n, n, 3 * N, 3 * N, N};
	Layout L;
	const auto p_out = L.add<float>(3 * N);
	Layout::Part<float> p_in[7];
	for (int c = 0; c < 7; ++c)
		p_in[c] = L.optional<float>(host[c], floats[c]);
	const auto p_stage = L.optional<uint8_t>(stage, N);
	RT_TRY(grow_device_buffer(s->d_denoise, s->d_denoise_bytes, L)); // shared with rt_denoise / rt_render_denoised
	Staging st{s};
	for (int c = 0; c < 7; ++c)
		st.put(L, p_in[c], host[c]);
	if (!st.ok())
		return st.finish("upscale upload");
	const rt_upscale_inputs d_in = {L.at(p_in[0]), L.at(p_in[1]), L.at(p_in[2]), L.at(p_in[3]),
	                                L.at(p_in[4]), L.at(p_in[5]), L.at(p_in[6])};
	st.rc = rt_upscale_device(s, &d_in, o, L.at(p_out), L.at(p_stage), s->stream);
	st.get(out, L, p_out);
	st.get(stage, L, p_stage);
	return st.finish("upscale");
}

int rt_render_upscaled(rt_scene *s, const rt_camera *camera, const rt_render_opts *o, uint32_t src_width, uint32_t src_height,
                       const rt_denoise_opts *dopts, const rt_upscale_opts *uopts, float *out, float *out_src, uint64_t *rays_shot)
{
	if (!s || !camera || !o || !dopts || !uopts || !out)
		return fail(RT_ERR_INVALID_ARGUMENT, "null argument");
	const uint64_t w = src_width, h = src_height, W = o->width, H = o->height;
	int rc = render_denoised_opts_check("rt_render_upscaled", o, dopts, w, h);
	if (rc == RT_OK)
		rc = upscale_opts_check(uopts, w, h, W, H);
	if (rc != RT_OK)
		return rc;
	const uint64_t n = w * h, N = W * H;
	if (ranges_overlap(out, 12 * N, out_src, 12 * n))
		return fail(RT_ERR_INVALID_ARGUMENT, "rt_render_upscaled: out overlaps out_src");
	rc = need_device(s);
	if (rc != RT_OK)
		return rc;
	HIP_TRY(hipSetDevice(s->device));
	// rt_render_denoised's frames at the source size, then at the destination size: albedo, normal, depth, out
	Layout L;
	const DenoisedParts P = denoised_parts(L, n);
	const auto p_albedo = L.add<float>(3 * N), p_normal = L.add<float>(3 * N), p_depth = L.add<float>(N), p_out = L.add<float>(3 * N);
	RT_TRY(grow_device_buffer(s->d_denoise, s->d_denoise_bytes, L));
	float *d_albedo = L.at(p_albedo), *d_normal = L.at(p_normal), *d_depth = L.at(p_depth);
	rt_render_opts os = *o;
	os.width = w;
	os.height = h;
	Staging st{s};
	enqueue_render_denoised(s, pinhole_source(s, camera), &os, dopts, L, P, st);
	enqueue_guides(s, camera, o, d_albedo, d_normal, d_depth, st);
	if (st.ok()) {
		const rt_upscale_inputs in = {L.at(P.clean), L.at(P.albedo), L.at(P.normal), L.at(P.depth), d_albedo, d_normal, d_depth};
		st.e = launch_upscale(s->stream, upscale_params(uopts, w, h, W, H, in, L.at(p_out), nullptr));
	}
	unsigned long long rays[2] = {0, 0};
	st.get(out, L, p_out);
	st.get(out_src, L, P.clean);
	st.get(rays, L, P.rays);
	rc = st.finish("render_upscaled");
	if (rc == RT_OK && rays_shot)
		*rays_shot = rays[0] + rays[1];
	return rc;
}

} // extern "C"
