// rt_api_lens.cpp -- the host side of the lens cameras (include/rt_hip.h: rt_lens_camera_new, rt_render_lens[_device]); their kernels
// are rt_lens.hip.  The argument checks follow rt_render_tiles' (rt_api_post.cpp tiles_check) in order and kind, the camera's
// own behind the buffers', the device last (so that a host-only scene reports bad arguments as such); the blocking entry stages
// the frame and the chunk sums through the scene's d_noise buffer, as rt_render_tiles does.
// Also here: the auxiliary buffers through a lens camera (rt_render_lens_aov[_device]; the kernel is rt_aov_lens.hip) and the denoised
// lens frame (rt_render_lens_denoised).  Both stage and compose through the steps rt_api_post.cpp shares (rt_api_internal.h).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>

#include "rt_api_internal.h"
#include "rt_aov_lens.h"
#include "rt_lens.h"

using namespace rt;

static_assert(RT_PROJ_PERSPECTIVE == kProjPerspective && RT_PROJ_ORTHOGRAPHIC == kProjOrthographic && RT_PROJ_FISHEYE == kProjFisheye &&
                  RT_PROJ_EQUIRECT == kProjEquirect,
              "rt_projection and the kernel's constants");
static_assert(sizeof(rt_lens_camera) == sizeof(rt_camera) + 52, "rt_lens_camera layout");

// the camera's own errors (the last two whatever the projection)
static int lens_camera_check(const rt_lens_camera *camera)
{
	if (camera->projection < RT_PROJ_PERSPECTIVE || camera->projection > RT_PROJ_EQUIRECT)
		return fail(RT_ERR_INVALID_ARGUMENT, "render_lens: unknown projection");
	if (!std::isfinite(camera->lens_radius) || camera->lens_radius < 0.0f)
		return fail(RT_ERR_INVALID_ARGUMENT, "render_lens: lens_radius must be finite and >= 0");
	if (!std::isfinite(camera->fisheye_half_angle) || !(camera->fisheye_half_angle > 0.0f))
		return fail(RT_ERR_INVALID_ARGUMENT, "render_lens: fisheye_half_angle must be finite and > 0");
	return RT_OK;
}

// *split is S resolved, *px the pixels, *n_tiles the 8 x 8 tiles of the frame
static int lens_check(const rt_scene *s, const rt_lens_camera *camera, const rt_render_opts *o, const float *out, const float *chunk_sums,
                      uint32_t *split, uint64_t *px, uint64_t *n_tiles)
{
	if (!s || !camera || !o || !out)
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
		return fail(RT_ERR_UNSUPPORTED, "render_lens: 2^31 pixels or more");
	*px = o->width * o->height;
	*n_tiles = tile_grid(o->width, o->height).count;
	uint32_t S = o->sample_split;
	if (S == 0u) // as rt_render resolves it for the whole frame (a host-only scene: for 256 CUs)
		S = auto_sample_split(s->n_cus, *px, o->samples_per_pixel, 1u);
	if (S > o->samples_per_pixel)
		return fail(RT_ERR_INVALID_ARGUMENT, "sample_split larger than samples_per_pixel");
	*split = S;
	if (S > 1u && ranges_overlap(out, 12 * *px, chunk_sums, 12ull * S * 64u * *n_tiles))
		return fail(RT_ERR_INVALID_ARGUMENT, "render_lens: chunk_sums overlaps the frame");
	if (const int rc = lens_camera_check(camera); rc != RT_OK)
		return rc;
	if (o->output_layout != RT_LAYOUT_FRAME)
		return fail(RT_ERR_UNSUPPORTED, "render_lens: RT_LAYOUT_FRAME only");
	if (o->shard_count != 1)
		return fail(RT_ERR_UNSUPPORTED, "render_lens: the whole frame only (shard_count 1)");
	if (!s->peers.empty())
		return fail(RT_ERR_UNSUPPORTED, "render_lens: a multi-device scene renders its own shards");
	if (64ull * *n_tiles * S >= (1ull << 31))
		return fail(RT_ERR_UNSUPPORTED, "render_lens: 64 x tiles x sample_split exceeds 2^31 lane items");
	return need_device(s);
}

// rt_render_lens_aov[_device], in the header's order: the arguments (the options as rt_render_aov_device reads them, the camera,
// the chain), then what is unsupported, the device last.  `c` NULL: the first hit.  *mask: the kAov* bits of the channels given
static int lens_aov_check(const rt_scene *s, const rt_lens_camera *camera, const rt_render_opts *o, const rt_aov_chain_opts *c,
                          const rt_aov_chain_buffers *b, uint32_t *mask)
{
	if (!s || !camera || !o || !b)
		return fail(RT_ERR_INVALID_ARGUMENT, "null argument");
	const rt_aov_buffers &a = b->aov;
	*mask = (a.albedo ? kAovAlbedo : 0u) | (a.normal ? kAovNormal : 0u) | (a.depth ? kAovDepth : 0u) | (a.coverage ? kAovCoverage : 0u) |
	        (a.primitive ? kAovPrimitive : 0u) | (a.material ? kAovMaterial : 0u) | (b->bounces ? kAovBounces : 0u);
	if (*mask == 0u)
		return fail(RT_ERR_INVALID_ARGUMENT, "rt_aov_chain_buffers: every channel is NULL");
	int rc = frame_sides("", o->width, o->height, 2);
	if (rc != RT_OK)
		return rc;
	if (o->samples_per_pixel == 0 || o->samples_per_pixel >= (1ull << 32))
		return fail(RT_ERR_INVALID_ARGUMENT, "samples_per_pixel must be in [1, 2^32)");
	rc = lens_camera_check(camera);
	if (rc == RT_OK && c)
		rc = aov_chain_opts_check(c);
	if (rc != RT_OK)
		return rc;
	if (o->width > (1ull << 31) || o->height > (1ull << 31) || o->width * o->height >= (1ull << 31))
		return fail(RT_ERR_UNSUPPORTED, "render_lens_aov: 2^31 pixels or more");
	if (o->output_layout != RT_LAYOUT_FRAME)
		return fail(RT_ERR_UNSUPPORTED, "render_lens_aov: RT_LAYOUT_FRAME only");
	if (o->shard_count != 1)
		return fail(RT_ERR_UNSUPPORTED, "render_lens_aov: the whole frame only (shard_count 1)");
	if (!s->peers.empty())
		return fail(RT_ERR_UNSUPPORTED, "render_lens_aov: a multi-device scene is not served");
	if ((*mask & kAovPrimitive) && s->host.primitive_order.size() >= 0xFFFFFFFFull) // (upload_scene, rt_api.cpp, makes the table for fewer)
		return fail(RT_ERR_UNSUPPORTED, "primitive IDs need fewer than 2^32 - 1 primitives");
	return need_device(s);
}

// which of two statuses an entry point with several checked pieces reports: a bad argument ahead of RT_ERR_UNSUPPORTED, that ahead
// of RT_ERR_NO_DEVICE (the message follows the status)
struct WorstStatus {
	int rc = RT_OK;
	std::string message;
	static int rank(int rc) { return rc == RT_ERR_INVALID_ARGUMENT ? 3 : rc == RT_ERR_UNSUPPORTED ? 2 : rc != RT_OK ? 1 : 0; }
	void take(int r)
	{
		if (rank(r) > rank(rc)) {
			rc = r;
			message = g_error;
		}
	}
	int result() const { return rc == RT_OK ? RT_OK : fail(rc, message); }
};

extern "C" {

int rt_lens_camera_new(rt_lens_camera *out, const float origin[3], const float lookat[3], const float vup[3], float fov_degrees,
                       float aspect_ratio, float aperture, float focus_dist, int32_t projection)
{
	if (!out || !origin || !lookat || !vup)
		return fail(RT_ERR_INVALID_ARGUMENT, "null argument");
	std::memset(out, 0, sizeof *out);
	camera_new(&out->pinhole, origin, lookat, vup, fov_degrees, aspect_ratio, aperture, focus_dist);
	// SimpleCamera::new's basis (camera.rs:32-34), the expressions of camera_new (rt_build.cpp)
	const V3 w = normalised(v3(origin[0], origin[1], origin[2]) - v3(lookat[0], lookat[1], lookat[2]));
	const V3 u = normalised(cross(w, v3(vup[0], vup[1], vup[2])));
	const V3 v = cross(u, w);
	const V3 f = -w;
	const V3 all[3] = {u, v, f};
	float *dst[3] = {out->right, out->up, out->forward};
	for (int i = 0; i < 3; ++i) {
		dst[i][0] = all[i].x;
		dst[i][1] = all[i].y;
		dst[i][2] = all[i].z;
	}
	out->lens_radius = aperture / 2.0f; // camera.rs:51
	out->fisheye_half_angle = rt_to_radians(fov_degrees) / 2.0f;
	out->projection = projection;
	return RT_OK;
}

int rt_render_lens_device(rt_scene *s, const rt_lens_camera *camera, const rt_render_opts *o, float *d_out_rgb, float *d_chunk_sums,
                          uint64_t *d_rays_shot, void *hip_stream)
{
	uint32_t split = 0;
	uint64_t px = 0, n_tiles = 0;
	int rc = lens_check(s, camera, o, d_out_rgb, d_chunk_sums, &split, &px, &n_tiles);
	if (rc != RT_OK)
		return rc;
	HIP_TRY(hipSetDevice(s->device));
	bool prune = false;
	DevScene dev;
	rc = four_wave_traversal(s, &prune, &dev); // (rt_api_internal.h)
	if (rc != RT_OK)
		return rc;
	const size_t lds_bytes = four_wave_stack_lds_bytes(dev) + kLensRecordLdsBytes;
	if (lds_bytes > s->max_lds)
		return fail(RT_ERR_UNSUPPORTED, "traversal stacks exceed the LDS of one CU");
	DevLensParams P;
	std::memset(&P, 0, sizeof P);
	P.cam = dev_camera(&camera->pinhole);
	std::memcpy(P.right, camera->right, 12);
	std::memcpy(P.up, camera->up, 12);
	std::memcpy(P.forward, camera->forward, 12);
	P.lens_radius = camera->lens_radius;
	P.fisheye_half_angle = camera->fisheye_half_angle;
	P.projection = camera->projection;
	P.out = d_out_rgb;
	P.chunk_sums = split > 1u ? d_chunk_sums : nullptr;
	P.rays_shot = reinterpret_cast<unsigned long long *>(d_rays_shot);
	P.width = (uint32_t)o->width;
	P.height = (uint32_t)o->height;
	P.tiles_x = tile_grid(o->width, o->height).tiles_x;
	P.n_tiles = (uint32_t)n_tiles;
	P.spp = (uint32_t)o->samples_per_pixel;
	P.split = split;
	P.item_chunks = P.chunk_sums ? 1u : split;
	const uint64_t items = n_tiles * (split / P.item_chunks);
	P.n_lanes = (uint32_t)(64u * items);
	P.seed_lo = (uint32_t)o->seed;
	P.seed_hi = (uint32_t)(o->seed >> 32);
	P.sample_begin_lo = (uint32_t)o->sample_begin;
	P.sample_begin_hi = (uint32_t)(o->sample_begin >> 32);
	P.max_depth = o->max_depth;
	P.rr_threshold = o->rr_threshold;
	// one wave per work item at a time
	HIP_TRY(launch_lens(o->render_method == RT_METHOD_NAIVE ? 0 : 1, prune, static_cast<hipStream_t>(hip_stream), dev, P,
	                    path_lane_groups(s, lds_bytes, kLensWaves, (items + kFourWaves - 1u) / kFourWaves)));
	return RT_OK;
}

int rt_render_lens(rt_scene *s, const rt_lens_camera *camera, const rt_render_opts *o, float *out_rgb, float *chunk_sums, uint64_t *rays_shot)
{
	uint32_t split = 0;
	uint64_t px = 0, n_tiles = 0;
	int rc = lens_check(s, camera, o, out_rgb, chunk_sums, &split, &px, &n_tiles);
	if (rc != RT_OK)
		return rc;
	HIP_TRY(hipSetDevice(s->device));
	if (split == 1u)
		chunk_sums = nullptr;
	Layout L;
	const auto p_frame = L.add<float>(3 * px), p_sums = L.optional<float>(chunk_sums, 3ull * split * 64u * n_tiles);
	RT_TRY(grow_device_buffer(s->d_noise, s->d_noise_bytes, L));
	Staging st{s};
	st.rc = rt_render_lens_device(s, camera, o, L.at(p_frame), L.at(p_sums), reinterpret_cast<uint64_t *>(s->d_rays), s->stream);
	st.get(out_rgb, L, p_frame);
	st.get(chunk_sums, L, p_sums);
	st.download(rays_shot, s->d_rays, sizeof(uint64_t));
	return st.finish("render_lens");
}

// ---- the auxiliary buffers through a lens camera (rt_aov_lens.hip) ----
int rt_render_lens_aov_device(rt_scene *s, const rt_lens_camera *camera, const rt_render_opts *o, const rt_aov_chain_opts *c,
                              const rt_aov_chain_buffers *d_out, void *hip_stream)
{
	uint32_t mask = 0;
	int rc = lens_aov_check(s, camera, o, c, d_out, &mask);
	if (rc != RT_OK)
		return rc;
	HIP_TRY(hipSetDevice(s->device));
	bool prune = false;
	DevScene dev;
	rc = four_wave_traversal(s, &prune, &dev); // (rt_api_internal.h)
	if (rc != RT_OK)
		return rc;
	DevAovLensParams P;
	std::memset(&P, 0, sizeof P);
	P.C.A = aov_params(s, &camera->pinhole, o, &d_out->aov, mask);
	P.C.max_chain = c ? c->max_chain : 0u; // NULL: the first hit
	P.C.fuzz_limit = c ? c->fuzz_limit : 0.0f;
	P.C.bounces = d_out->bounces;
	std::memcpy(P.right, camera->right, 12);
	std::memcpy(P.up, camera->up, 12);
	std::memcpy(P.forward, camera->forward, 12);
	P.lens_radius = camera->lens_radius;
	P.fisheye_half_angle = camera->fisheye_half_angle;
	P.projection = camera->projection;
	HIP_TRY(launch_aov_lens(prune, static_cast<hipStream_t>(hip_stream), dev, P));
	return RT_OK;
}

int rt_render_lens_aov(rt_scene *s, const rt_lens_camera *camera, const rt_render_opts *o, const rt_aov_chain_opts *c,
                       const rt_aov_chain_buffers *out)
{
	uint32_t mask = 0;
	const int rc = lens_aov_check(s, camera, o, c, out, &mask);
	if (rc != RT_OK)
		return rc;
	return render_aov_staged(s, o, out->aov, out->bounces, "render_lens_aov",
	                         [&](const rt_aov_chain_buffers &d) { return rt_render_lens_aov_device(s, camera, o, c, &d, s->stream); });
}

// ---- a denoised lens frame: rt_render_denoised's steps (rt_api_post.cpp) with the lens entry points in place of the pinhole ones ----
int rt_render_lens_denoised(rt_scene *s, const rt_lens_camera *camera, const rt_render_opts *o, const rt_aov_chain_opts *c,
                            const rt_denoise_opts *dopts, float *out_clean, float *out_noisy, uint64_t *rays_shot)
{
	if (!s || !camera || !o || !dopts || !out_clean)
		return fail(RT_ERR_INVALID_ARGUMENT, "null argument");
	// the union of the pieces' checks: the composite's own, a half render's (on any non-NULL frame), the guides'
	WorstStatus st;
	st.take(render_denoised_opts_check("rt_render_lens_denoised", o, dopts, o->width, o->height));
	if (st.rc == RT_OK) {
		const uint64_t n = o->width * o->height;
		if (ranges_overlap(out_clean, 12 * n, out_noisy, 12 * n))
			st.take(fail(RT_ERR_INVALID_ARGUMENT, "rt_render_lens_denoised: out_clean overlaps out_noisy"));
	}
	rt_render_opts oh = *o;
	oh.samples_per_pixel = o->samples_per_pixel / 2;
	uint32_t split = 0, mask = 0;
	uint64_t px = 0, n_tiles = 0;
	st.take(lens_check(s, camera, &oh, out_clean, nullptr, &split, &px, &n_tiles));
	const rt_aov_chain_buffers guides = {{out_clean, out_clean, out_clean, nullptr, nullptr, nullptr}, nullptr};
	st.take(lens_aov_check(s, camera, o, c, &guides, &mask));
	if (st.rc != RT_OK)
		return st.result();
	const DenoisedSource src = {
	    [=](const rt_render_opts *half, float *d_rgb, uint64_t *d_rays) { return rt_render_lens_device(s, camera, half, d_rgb, nullptr, d_rays, s->stream); },
	    [=](const rt_render_opts *all, const rt_aov_buffers &d) {
		    const rt_aov_chain_buffers b = {d, nullptr};
		    return rt_render_lens_aov_device(s, camera, all, c, &b, s->stream);
	    }};
	return render_denoised_staged(s, src, o, dopts, "render_lens_denoised", out_clean, out_noisy, rays_shot);
}

} // extern "C"
