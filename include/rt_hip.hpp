// rt_hip.hpp -- header-only C++17 host side above the C ABI (rt_hip.h).
//
// The reference's host is compiled Rust; no Rust toolchain exists in this pipeline, so this header is
// the compiled-language twin of the binding in INTEGRATION.md.  It mirrors the reference's names and
// argument meaning for the one path the library replaces:
//   SceneBuilder            what crates/loader builds inside the Region arena (textures, materials, primitives, sky)
//   Bvh                     Bvh::new(primitives, sky, split_type)            acceleration/mod.rs:58-93
//   SimpleCamera            SimpleCamera::new                                camera.rs:20-54
//   RenderOptions, RenderMethod, SamplerProgress                             samplers/mod.rs:22-63
//   HipSampler::sample_image(options, camera, bvh, (data, callback))         samplers/mod.rs:7-20, random_sampler.rs:10-99
// Errors are exceptions carrying the rt_status and rt_last_error() text.
#pragma once

#include <cstdint>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "rt_hip.h"

namespace rt_hip {

struct Error : std::runtime_error {
	int code;
	Error(int c, const std::string &what) : std::runtime_error("rt_hip error " + std::to_string(c) + ": " + what), code(c) {}
};
inline void check(int rc)
{
	if (rc != RT_OK)
		throw Error(rc, rt_last_error());
}

struct Vec3 {
	float x, y, z;
};

enum class RenderMethod { Naive = RT_METHOD_NAIVE, MIS = RT_METHOD_MIS }; // samplers/mod.rs:43-47
enum class SplitType { Sah = RT_SPLIT_SAH, Middle = RT_SPLIT_MIDDLE, EqualCounts = RT_SPLIT_EQUAL_COUNTS };

struct RenderOptions { // samplers/mod.rs:22-41 (Default impl)
	uint64_t samples_per_pixel = 128;
	RenderMethod render_method = RenderMethod::MIS;
	uint64_t width = 1920;
	uint64_t height = 1080;
	float gamma = 2.2f;
};

struct SamplerProgress { // samplers/mod.rs:49-63
	uint64_t samples_completed = 0;
	uint64_t rays_shot = 0;
	std::vector<float> current_image;
	SamplerProgress(uint64_t pixel_num, uint64_t channels) : current_image(pixel_num * channels, 0.0f) {}
};
// `&SamplerProgress` as the presentation callback sees it: the image lives in the sampler's pinned buffer
struct SamplerProgressRef {
	uint64_t samples_completed = 0;
	uint64_t rays_shot = 0;
	struct Image {
		const float *ptr = nullptr;
		size_t n = 0;
		const float *data() const { return ptr; }
		size_t size() const { return n; }
		float operator[](size_t k) const { return ptr[k]; }
	} current_image;
};

class SimpleCamera { // camera.rs:6-54
  public:
	SimpleCamera(Vec3 origin, Vec3 lookat, Vec3 vup, float fov, float aspect_ratio, float aperture, float focus_dist)
	{
		const float o[3] = {origin.x, origin.y, origin.z}, l[3] = {lookat.x, lookat.y, lookat.z}, u[3] = {vup.x, vup.y, vup.z};
		check(rt_camera_new(&cam_, o, l, u, fov, aspect_ratio, aperture, focus_dist));
	}
	const rt_camera &raw() const { return cam_; }

  private:
	rt_camera cam_{};
};

// SimpleCamera with the fields get_ray never reads in use (the thin lens: aperture > 0), or another projection (rt_hip.h
// rt_lens_camera): what render_lens below takes
class LensCamera {
  public:
	LensCamera(Vec3 origin, Vec3 lookat, Vec3 vup, float fov, float aspect_ratio, float aperture, float focus_dist,
	           rt_projection projection = RT_PROJ_PERSPECTIVE)
	{
		const float o[3] = {origin.x, origin.y, origin.z}, l[3] = {lookat.x, lookat.y, lookat.z}, u[3] = {vup.x, vup.y, vup.z};
		check(rt_lens_camera_new(&cam_, o, l, u, fov, aspect_ratio, aperture, focus_dist, (int32_t)projection));
	}
	const rt_lens_camera &raw() const { return cam_; }

  private:
	rt_lens_camera cam_{};
};

// Everything Bvh::new consumes.  Handles returned by the add-functions are indices, the way the
// loader resolves names to RegionRes handles (loader/src/lib.rs:28-84).
class SceneBuilder {
  public:
	uint32_t solid(Vec3 colour) { return texture(RT_TEX_SOLID, colour, {0, 0, 0}); }                       // SolidColour::new
	uint32_t lerp(Vec3 colour_one, Vec3 colour_two) { return texture(RT_TEX_LERP, colour_one, colour_two); } // Lerp::new
	uint32_t checkered(Vec3 one, Vec3 two) { return texture(RT_TEX_CHECKERED, one, two); }                  // CheckeredTexture::new

	uint32_t emissive(uint32_t tex, float strength) { return material(RT_MAT_EMIT, tex, strength); }        // Emit::new
	uint32_t lambertian(uint32_t tex, float albedo) { return material(RT_MAT_LAMBERTIAN, tex, albedo); }    // Lambertian::new
	uint32_t reflect(uint32_t tex, float fuzz) { return material(RT_MAT_REFLECT, tex, fuzz); }              // Reflect::new
	uint32_t refract(uint32_t tex, float eta) { return material(RT_MAT_REFRACT, tex, eta); }                // Refract::new
	uint32_t trowbridge_reitz(uint32_t tex, float roughness, Vec3 ior, float metallic)                      // TrowbridgeReitz::new
	{
		const uint32_t m = material(RT_MAT_TROWBRIDGE_REITZ, tex, roughness * roughness); // alpha = roughness^2 (:17-24)
		materials_[m].ior[0] = ior.x; materials_[m].ior[1] = ior.y; materials_[m].ior[2] = ior.z;
		materials_[m].metallic = metallic;
		return m;
	}

	void sphere(Vec3 centre, float radius, uint32_t mat) // Sphere::new
	{
		rt_primitive_desc p{};
		p.type = RT_PRIM_SPHERE;
		p.material = mat;
		p.u.sphere.centre[0] = centre.x; p.u.sphere.centre[1] = centre.y; p.u.sphere.centre[2] = centre.z;
		p.u.sphere.radius = radius;
		primitives_.push_back(p);
	}
	void triangle(const Vec3 points[3], const Vec3 normals[3], uint32_t mat) // Triangle::new
	{
		rt_triangle_data t{};
		for (int k = 0; k < 3; ++k) {
			t.points[3 * k] = points[k].x; t.points[3 * k + 1] = points[k].y; t.points[3 * k + 2] = points[k].z;
			t.normals[3 * k] = normals[k].x; t.normals[3 * k + 1] = normals[k].y; t.normals[3 * k + 2] = normals[k].z;
		}
		triangles_.push_back(t);
		rt_primitive_desc p{};
		p.type = RT_PRIM_TRIANGLE;
		p.material = mat;
		p.u.triangle.data = triangles_.size() - 1;
		primitives_.push_back(p);
	}
	// Sky::new(texture, Emit(texture, 1.0), sampler_res)  sky.rs:22-39, loader/src/misc.rs:20-38
	void sky(uint32_t tex, uint32_t res_x = 100, uint32_t res_y = 100)
	{
		sky_.texture = tex;
		sky_.material = emissive(tex, 1.0f);
		sky_.sampler_res_x = res_x;
		sky_.sampler_res_y = res_y;
		has_sky_ = true;
	}

	rt_scene_desc desc(SplitType split) const
	{
		if (!has_sky_)
			throw Error(RT_ERR_INVALID_ARGUMENT, "scene has no sky");
		rt_scene_desc d{};
		d.abi_version = RT_ABI_VERSION;
		d.n_textures = (uint32_t)textures_.size();
		d.textures = textures_.data();
		d.n_materials = (uint32_t)materials_.size();
		d.materials = materials_.data();
		d.n_primitives = primitives_.size();
		d.primitives = primitives_.data();
		d.n_triangles = triangles_.size();
		d.triangles = triangles_.data();
		d.sky = sky_;
		d.split_type = (int32_t)split;
		return d;
	}

  private:
	uint32_t texture(int type, Vec3 a, Vec3 b)
	{
		rt_texture_desc t{};
		t.type = type;
		t.colour_one[0] = a.x; t.colour_one[1] = a.y; t.colour_one[2] = a.z;
		t.colour_two[0] = b.x; t.colour_two[1] = b.y; t.colour_two[2] = b.z;
		textures_.push_back(t);
		return (uint32_t)textures_.size() - 1;
	}
	uint32_t material(int type, uint32_t tex, float param)
	{
		rt_material_desc m{};
		m.type = type;
		m.texture = tex;
		m.param = param;
		m.ior[0] = m.ior[1] = m.ior[2] = 1.0f;
		materials_.push_back(m);
		return (uint32_t)materials_.size() - 1;
	}
	std::vector<rt_texture_desc> textures_;
	std::vector<rt_material_desc> materials_;
	std::vector<rt_primitive_desc> primitives_;
	std::vector<rt_triangle_data> triangles_;
	rt_sky_desc sky_{};
	bool has_sky_ = false;
};

class Bvh { // acceleration/mod.rs:44-93, resident in the HBM of `device`
  public:
	Bvh(const SceneBuilder &scene, SplitType split = SplitType::Sah, int device = 0)
	{
		const rt_scene_desc d = scene.desc(split);
		check(rt_scene_create(&d, device, &h_));
	}
	// one Bvh replicated over several GPUs of the node: every render through it shards the frame's tiles over `devices`
	// and gathers into devices[0] (rt_scene_create_multi; the partition of samplers/random_sampler.rs:45-52 across devices)
	Bvh(const SceneBuilder &scene, const std::vector<int> &devices, SplitType split = SplitType::Sah)
	{
		const rt_scene_desc d = scene.desc(split);
		check(rt_scene_create_multi(&d, devices.data(), (uint32_t)devices.size(), &h_));
	}
	uint32_t device_count() const
	{
		uint32_t n = 0;
		check(rt_scene_device_count(h_, &n));
		return n;
	}
	// how a multi-device Bvh moves its members' shards into devices[0], and why (rt_gather_mode; settled at construction)
	std::pair<int, std::string> gather_info() const
	{
		int mode = 0;
		char note[512] = {0};
		check(rt_scene_gather_info(h_, &mode, note, sizeof note));
		return {mode, std::string(note)};
	}
	// what rt_render_opts.sample_split = 0 resolves to for these options on this Bvh (the library's one rule)
	uint32_t auto_sample_split(const rt_render_opts &opts) const
	{
		uint32_t split = 1;
		check(rt_scene_auto_sample_split(h_, &opts, &split));
		return split;
	}
	~Bvh() { rt_scene_destroy(h_); }
	Bvh(const Bvh &) = delete;
	Bvh &operator=(const Bvh &) = delete;
	uint64_t number_nodes() const // Bvh::number_nodes  mod.rs:94-96
	{
		uint64_t n = 0;
		check(rt_scene_counts(h_, &n, nullptr, nullptr));
		return n;
	}
	std::vector<uint64_t> lights() const // pub lights  mod.rs:48
	{
		uint64_t n = 0;
		check(rt_scene_counts(h_, nullptr, nullptr, &n));
		std::vector<uint64_t> out(n ? n : 1);
		check(rt_scene_get_lights(h_, out.data(), out.size()));
		out.resize(n);
		return out;
	}
	rt_scene *raw() const { return h_; }

  private:
	rt_scene *h_ = nullptr;
};

// `impl Sampler` on the GPU.  The reference calls the update function after EVERY pass with that
// pass's image (random_sampler.rs:82-98); this sampler renders `batch` passes per call of the ABI and
// hands the callback the batch's mean, progress.samples_completed = passes in the batch, and the total
// number of passes so far -- with batch = 1 that is the reference's contract verbatim.  Returning true
// cancels.  `running_mean` is the TUI callback's accumulation (src/main.rs:175-191) for any batch size.
struct HipSampler {
	uint64_t batch = 0; // 0 = all passes in one launch
	uint64_t seed = 1;
	uint32_t sample_split = 1; // rt_render_opts.sample_split; 0 = automatic (>= 64 work items per resident lane on every device: 7 - 29 % faster
	                           // than whole-pixel items on the BASELINE workloads, image moves by ~1e-7); 1 = the reference's strictly sequential fold
	uint32_t max_depth = 50, rr_threshold = 3; // integrators/mod.rs:7-8

	// update(data, previous, i) -> bool, the reference's presentation_update: called once per batch with the
	// batch's mean image while the next batch renders; `true` cancels (random_sampler.rs:82-98)
	template <class T, class F>
	void sample_image(const RenderOptions &o, const SimpleCamera &camera, const Bvh &bvh, T *data, F update) const
	{
		rt_render_opts opts;
		rt_render_opts_default(&opts);
		opts.width = o.width;
		opts.height = o.height;
		opts.samples_per_pixel = o.samples_per_pixel;
		opts.seed = seed;
		opts.render_method = (int32_t)o.render_method;
		opts.max_depth = max_depth;
		opts.rr_threshold = rr_threshold;
		opts.sample_split = sample_split;
		struct Closure {
			T *data;
			F *update;
		} closure{data, &update};
		check(rt_sample_image(bvh.raw(), &camera.raw(), &opts, batch,
		                      [](void *c, const rt_sampler_progress *p, uint64_t done) -> int {
			                      auto *cl = static_cast<Closure *>(c);
			                      SamplerProgressRef ref;
			                      ref.samples_completed = p->samples_completed;
			                      ref.rays_shot = p->rays_shot;
			                      ref.current_image.ptr = p->current_image;
			                      ref.current_image.n = (size_t)p->n_floats;
			                      return (*cl->update)(cl->data, ref, done) ? 1 : 0;
		                      },
		                      &closure));
	}
};

// The output stage on the GPU (crates/output/src/lib.rs:89-97): renders and returns the 8-bit RGB image
// save_data_to_image would write, `(val.powf(1.0 / gamma) * 255.999) as u8` computed where the frame lives.
inline std::vector<uint8_t> render_rgb8(const RenderOptions &o, const SimpleCamera &camera, const Bvh &bvh, uint64_t seed = 1,
                                        uint64_t *rays_shot = nullptr)
{
	rt_render_opts opts;
	rt_render_opts_default(&opts);
	opts.width = o.width;
	opts.height = o.height;
	opts.samples_per_pixel = o.samples_per_pixel;
	opts.seed = seed;
	opts.render_method = (int32_t)o.render_method;
	std::vector<uint8_t> out((size_t)o.width * o.height * 3);
	check(rt_render_rgb8(bvh.raw(), &camera.raw(), &opts, o.gamma, out.data(), rays_shot));
	return out;
}

// First-hit auxiliary buffers of the passes [sample_begin, sample_begin + o.samples_per_pixel) -- the camera rays a render with
// the same seed traces (semantics: rt_hip.h rt_aov_buffers).  Every channel is produced; row-major, y down.
struct AovBuffers {
	std::vector<float> albedo, normal; // w*h*3
	std::vector<float> depth, coverage; // w*h
	std::vector<uint32_t> primitive, material; // w*h; UINT32_MAX where pass sample_begin missed
};
inline AovBuffers render_aov(const RenderOptions &o, const SimpleCamera &camera, const Bvh &bvh, uint64_t seed = 1,
                             uint64_t sample_begin = 0)
{
	rt_render_opts opts;
	rt_render_opts_default(&opts);
	opts.width = o.width;
	opts.height = o.height;
	opts.samples_per_pixel = o.samples_per_pixel;
	opts.sample_begin = sample_begin;
	opts.seed = seed;
	const size_t n = (size_t)o.width * o.height;
	AovBuffers a;
	a.albedo.resize(n * 3);
	a.normal.resize(n * 3);
	a.depth.resize(n);
	a.coverage.resize(n);
	a.primitive.resize(n);
	a.material.resize(n);
	const rt_aov_buffers b = {a.albedo.data(), a.normal.data(), a.depth.data(), a.coverage.data(), a.primitive.data(), a.material.data()};
	check(rt_render_aov(bvh.raw(), &camera.raw(), &opts, &b));
	return a;
}

// The same channels taken through perfect mirrors and glass, at the first vertex of each camera path that is not one (semantics:
// rt_hip.h rt_aov_chain_opts); `bounces` is the mean number of surfaces followed.  AovChainBuffers is an AovBuffers, so it goes
// wherever one is taken (denoise, upscale) -- but not to TemporalDenoiser: its depth is a path length.
struct AovChainOptions {
	uint32_t max_chain = 8;
	float fuzz_limit = 0.0f;
};
struct AovChainBuffers : AovBuffers {
	std::vector<float> bounces; // w*h
};
inline AovChainBuffers render_aov_chain(const RenderOptions &o, const SimpleCamera &camera, const Bvh &bvh,
                                        const AovChainOptions &c = AovChainOptions(), uint64_t seed = 1, uint64_t sample_begin = 0)
{
	rt_render_opts opts;
	rt_render_opts_default(&opts);
	opts.width = o.width;
	opts.height = o.height;
	opts.samples_per_pixel = o.samples_per_pixel;
	opts.sample_begin = sample_begin;
	opts.seed = seed;
	rt_aov_chain_opts copts;
	rt_aov_chain_opts_default(&copts);
	copts.max_chain = c.max_chain;
	copts.fuzz_limit = c.fuzz_limit;
	const size_t n = (size_t)o.width * o.height;
	AovChainBuffers a;
	a.albedo.resize(n * 3);
	a.normal.resize(n * 3);
	a.depth.resize(n);
	a.coverage.resize(n);
	a.primitive.resize(n);
	a.material.resize(n);
	a.bounces.resize(n);
	const rt_aov_chain_buffers b = {{a.albedo.data(), a.normal.data(), a.depth.data(), a.coverage.data(), a.primitive.data(), a.material.data()},
	                                a.bounces.data()};
	check(rt_render_aov_chain(bvh.raw(), &camera.raw(), &opts, &copts, &b));
	return a;
}

// Anti-aliased ID mattes (semantics: rt_hip.h rt_matte_opts): the `layers` most-covering primitive or material IDs of every pixel
// over ALL passes with their coverage fractions, layer-major, and what they leave out; then the matte of a selection of IDs.
struct MatteOptions {
	rt_matte_id_kind id_kind = RT_MATTE_ID_MATERIAL;
	uint32_t layers = 4; // 1..RT_MATTE_SLOTS
};
struct MatteLayers {
	uint32_t width = 0, height = 0, layers = 0;
	std::vector<uint32_t> ids;   // layers*w*h; UINT32_MAX: the sky (coverage > 0) or an empty layer (coverage 0)
	std::vector<float> coverage; // layers*w*h
	std::vector<float> residual; // w*h
};
inline MatteLayers render_matte(const RenderOptions &o, const SimpleCamera &camera, const Bvh &bvh, const MatteOptions &m = MatteOptions(),
                                uint64_t seed = 1, uint64_t sample_begin = 0)
{
	rt_render_opts opts;
	rt_render_opts_default(&opts);
	opts.width = o.width;
	opts.height = o.height;
	opts.samples_per_pixel = o.samples_per_pixel;
	opts.sample_begin = sample_begin;
	opts.seed = seed;
	rt_matte_opts mopts;
	check(rt_matte_opts_default(&mopts));
	mopts.id_kind = (int32_t)m.id_kind;
	mopts.layers = m.layers;
	const size_t n = (size_t)o.width * o.height, k = m.layers <= RT_MATTE_SLOTS ? m.layers : 0;
	MatteLayers r;
	r.width = (uint32_t)o.width;
	r.height = (uint32_t)o.height;
	r.layers = m.layers;
	r.ids.resize(k * n);
	r.coverage.resize(k * n);
	r.residual.resize(n);
	const rt_matte_buffers b = {r.ids.data(), r.coverage.data(), r.residual.data()};
	check(rt_render_matte(bvh.raw(), &camera.raw(), &opts, &mopts, &b));
	return r;
}
// the matte (w*h, in [0, 1]) of the IDs in `selection`: any order, duplicates allowed; UINT32_MAX selects the sky
inline std::vector<float> matte_extract(const Bvh &bvh, const MatteLayers &layers, const std::vector<uint32_t> &selection)
{
	std::vector<float> out((size_t)layers.width * layers.height);
	const rt_matte_buffers b = {const_cast<uint32_t *>(layers.ids.data()), const_cast<float *>(layers.coverage.data()), nullptr};
	check(rt_matte_extract(bvh.raw(), &b, layers.width, layers.height, layers.layers, selection.data(), selection.size(), out.data()));
	return out;
}

// Radiance queries (semantics: rt_hip.h rt_radiance_opts): the mean of `samples_per_ray` samples of the integrator along each of
// the caller's rays, 3 floats a ray.  Sample k of ray i runs on the stream (seed, streams[i] or i, sample_begin + k) with no draw
// ahead of the integrator: a query of a camera's rays does not reproduce a frame's bytes.  Blocking.
struct RadianceOptions {
	uint64_t seed = 0, sample_begin = 0;
	uint32_t samples_per_ray = 1;
	rt_render_method render_method = RT_METHOD_MIS;
	uint32_t max_depth = 50, rr_threshold = 3;
};
inline std::vector<float> radiance(const Bvh &bvh, const std::vector<rt_ray_desc> &rays, const RadianceOptions &r = RadianceOptions(),
                                   const std::vector<uint64_t> *streams = nullptr)
{
	rt_radiance_opts opts;
	check(rt_radiance_opts_default(&opts));
	opts.seed = r.seed;
	opts.sample_begin = r.sample_begin;
	opts.samples_per_ray = r.samples_per_ray;
	opts.render_method = r.render_method;
	opts.max_depth = r.max_depth;
	opts.rr_threshold = r.rr_threshold;
	if (streams && streams->size() != rays.size())
		throw std::invalid_argument("radiance: one stream per ray");
	std::vector<float> out(3 * rays.size());
	// (an empty batch: the library writes nothing; the vectors' data() may be null, which it would refuse)
	if (!rays.empty())
		check(rt_radiance(bvh.raw(), rays.data(), streams ? streams->data() : nullptr, rays.size(), &opts, out.data()));
	return out;
}

// Ambient occlusion (semantics: rt_hip.h rt_ao_opts): per pixel the share of `rays_per_pass` cosine-weighted rays per pass from the
// first hit that reach nothing within `radius` (0: no limit), and the mean direction of those rays (length = openness).
struct AoOptions {
	uint32_t rays_per_pass = 4; // 1..64
	float radius = 0.0f;
};
struct AoBuffers {
	std::vector<float> visibility;  // w*h, 1 where no pass hit
	std::vector<float> bent_normal; // 3*w*h, 0 where no pass hit
};
inline AoBuffers render_ao(const RenderOptions &o, const SimpleCamera &camera, const Bvh &bvh, const AoOptions &a = AoOptions(),
                           uint64_t seed = 1, uint64_t sample_begin = 0)
{
	rt_render_opts opts;
	rt_render_opts_default(&opts);
	opts.width = o.width;
	opts.height = o.height;
	opts.samples_per_pixel = o.samples_per_pixel;
	opts.sample_begin = sample_begin;
	opts.seed = seed;
	rt_ao_opts aopts;
	check(rt_ao_opts_default(&aopts));
	aopts.rays_per_pass = a.rays_per_pass;
	aopts.radius = a.radius;
	const size_t n = (size_t)o.width * o.height;
	AoBuffers r;
	r.visibility.resize(n);
	r.bent_normal.resize(3 * n);
	const rt_ao_buffers b = {r.visibility.data(), r.bent_normal.data()};
	check(rt_render_ao(bvh.raw(), &camera.raw(), &opts, &aopts, &b));
	return r;
}

// Noise estimates (semantics: rt_hip.h rt_noise_opts): from ONE render at `sample_split` (2..64 dividing the passes, 0 = automatic)
// the mean rt_render gives at that split, the variance of the luminance of that mean, the 8 x 8 tile error map and its summary.
struct NoiseOptions {
	float luminance_floor = 0.01f; // untuned starting value
	float threshold = 0.05f;       // untuned starting value
};
struct NoiseEstimate {
	std::vector<float> mean;       // 3*w*h
	std::vector<float> variance;   // w*h
	std::vector<float> lum_mean;   // w*h
	std::vector<float> tile_error; // ceil(w/8) * ceil(h/8)
	rt_noise_summary summary{};
	uint64_t rays_shot = 0;
};
namespace detail {
inline rt_noise_opts noise_opts(const NoiseOptions &n)
{
	rt_noise_opts o;
	check(rt_noise_opts_default(&o));
	o.luminance_floor = n.luminance_floor;
	o.threshold = n.threshold;
	return o;
}
inline rt_render_opts noise_render_opts(const RenderOptions &o, uint32_t sample_split, uint64_t seed, uint64_t sample_begin)
{
	rt_render_opts opts;
	rt_render_opts_default(&opts);
	opts.width = o.width;
	opts.height = o.height;
	opts.samples_per_pixel = o.samples_per_pixel;
	opts.sample_begin = sample_begin;
	opts.seed = seed;
	opts.sample_split = sample_split;
	return opts;
}
} // namespace detail
inline NoiseEstimate render_noise(const RenderOptions &o, const SimpleCamera &camera, const Bvh &bvh, uint32_t sample_split = 0,
                                  const NoiseOptions &n = NoiseOptions(), uint64_t seed = 1, uint64_t sample_begin = 0)
{
	const rt_render_opts opts = detail::noise_render_opts(o, sample_split, seed, sample_begin);
	const rt_noise_opts nopts = detail::noise_opts(n);
	const size_t px = (size_t)o.width * o.height;
	NoiseEstimate r;
	r.mean.resize(3 * px);
	r.variance.resize(px);
	r.lum_mean.resize(px);
	r.tile_error.resize(((size_t)o.width + 7) / 8 * (((size_t)o.height + 7) / 8));
	const rt_noise_buffers b = {r.mean.data(), r.variance.data(), r.lum_mean.data(), r.tile_error.data(), &r.summary};
	check(rt_render_noise(bvh.raw(), &camera.raw(), &opts, &nopts, nullptr, &b, &r.rays_shot));
	return r;
}
// Render windows of `batch` passes until every tile's error is at most the threshold (after at least min_batches windows) or another
// window would exceed max_passes.  The mean is a mean of batch means, not the bytes of one render of all the passes.
struct ConvergedFrame {
	std::vector<float> mean, variance, tile_error;
	rt_noise_result result{};
};
inline ConvergedFrame render_converged(const RenderOptions &o, const SimpleCamera &camera, const Bvh &bvh, uint32_t sample_split, uint64_t batch,
                                       uint32_t min_batches, uint64_t max_passes, const NoiseOptions &n = NoiseOptions(), uint64_t seed = 1)
{
	const rt_render_opts opts = detail::noise_render_opts(o, sample_split, seed, 0);
	const rt_noise_opts nopts = detail::noise_opts(n);
	const size_t px = (size_t)o.width * o.height;
	ConvergedFrame r;
	r.mean.resize(3 * px);
	r.variance.resize(px);
	r.tile_error.resize(((size_t)o.width + 7) / 8 * (((size_t)o.height + 7) / 8));
	check(rt_render_converged(bvh.raw(), &camera.raw(), &opts, &nopts, batch, min_batches, max_passes, r.mean.data(), r.variance.data(),
	                          r.tile_error.data(), &r.result));
	return r;
}

// render_converged that, after min_batches whole-frame windows, renders only the tiles whose error is still above the threshold.
// The mean of a stopped tile is a mean of fewer batches than its neighbour's (tile borders can show at loose thresholds); the
// thresholds are untuned defaults.  passes[p] = the passes rendered for pixel p.
struct AdaptiveFrame {
	std::vector<float> mean, variance, tile_error;
	std::vector<uint32_t> passes;
	rt_adaptive_result result{};
};
inline AdaptiveFrame render_adaptive(const RenderOptions &o, const SimpleCamera &camera, const Bvh &bvh, uint32_t sample_split, uint64_t batch,
                                     uint32_t min_batches, uint64_t max_passes, const NoiseOptions &n = NoiseOptions(), uint64_t seed = 1)
{
	const rt_render_opts opts = detail::noise_render_opts(o, sample_split, seed, 0);
	const rt_noise_opts nopts = detail::noise_opts(n);
	const size_t px = (size_t)o.width * o.height;
	AdaptiveFrame r;
	r.mean.resize(3 * px);
	r.variance.resize(px);
	r.passes.resize(px);
	r.tile_error.resize(((size_t)o.width + 7) / 8 * (((size_t)o.height + 7) / 8));
	check(rt_render_adaptive(bvh.raw(), &camera.raw(), &opts, &nopts, nullptr, batch, min_batches, max_passes, r.mean.data(), r.variance.data(),
	                         r.tile_error.data(), r.passes.data(), &r.result));
	return r;
}
// The pixels of the listed 8 x 8 tiles (distinct indices into the grid of the tile errors) of `frame` (3 * width * height floats)
// receive the bytes render gives them under the same options; every other pixel keeps its value.  Returns the rays shot.
inline uint64_t render_tiles(const RenderOptions &o, const SimpleCamera &camera, const Bvh &bvh, uint32_t sample_split, const std::vector<uint32_t> &tiles,
                             std::vector<float> &frame, uint64_t seed = 1)
{
	const rt_render_opts opts = detail::noise_render_opts(o, sample_split, seed, 0);
	if (frame.size() != 3 * (size_t)o.width * o.height)
		throw std::invalid_argument("render_tiles: frame must hold 3 * width * height floats");
	uint64_t rays = 0;
	check(rt_render_tiles(bvh.raw(), &camera.raw(), &opts, tiles.data(), (uint32_t)tiles.size(), frame.data(), nullptr, &rays));
	return rays;
}
// A whole frame (3 * width * height floats) through a lens camera: a thin lens, an orthographic, fisheye or equirectangular
// projection (semantics: rt_hip.h rt_render_lens).  Not render's bytes even for a pinhole: the camera draws on a stream of its own.
inline std::vector<float> render_lens(const RenderOptions &o, const LensCamera &camera, const Bvh &bvh, uint32_t sample_split = 1, uint64_t seed = 1,
                                      uint64_t *rays_shot = nullptr)
{
	const rt_render_opts opts = detail::noise_render_opts(o, sample_split, seed, 0);
	std::vector<float> frame(3 * (size_t)o.width * o.height);
	check(rt_render_lens(bvh.raw(), &camera.raw(), &opts, frame.data(), nullptr, rays_shot));
	return frame;
}
// The indices, ascending, of the tiles whose error is above `threshold` (strictly; NaN is not): what render_tiles takes next.
inline std::vector<uint32_t> select_tiles(const Bvh &bvh, const std::vector<float> &tile_error, uint32_t width, uint32_t height, float threshold)
{
	std::vector<uint32_t> tiles(tile_error.size());
	uint32_t count = 0;
	check(rt_noise_select_tiles(bvh.raw(), tile_error.data(), width, height, threshold, tiles.data(), &count));
	tiles.resize(count);
	return tiles;
}

// Firefly-robust frames (semantics: rt_hip.h rt_robust_opts): from ONE render at `sample_split` (2..64 dividing the passes, 0 =
// automatic) the rank-trimmed mean of its chunk sums next to the plain mean rt_render gives at that split.  Symmetric trimming
// darkens; the defaults are untuned starting values.
struct RobustOptions {
	rt_robust_mode mode = RT_ROBUST_GINI;
	uint32_t trim = 1;
	float gini_gain = 1.0f;
};
struct RobustFrame {
	std::vector<float> out, mean;         // 3*w*h
	std::vector<float> gini;              // w*h
	std::vector<uint8_t> trimmed, dropped; // w*h
	uint64_t rays_shot = 0;
};
namespace detail {
inline rt_robust_opts robust_opts(const RobustOptions &r)
{
	rt_robust_opts o;
	check(rt_robust_opts_default(&o));
	o.mode = static_cast<int32_t>(r.mode);
	o.trim = r.trim;
	o.gini_gain = r.gini_gain;
	return o;
}
inline rt_robust_buffers robust_frame(RobustFrame &f, size_t px)
{
	f.out.resize(3 * px);
	f.mean.resize(3 * px);
	f.gini.resize(px);
	f.trimmed.resize(px);
	f.dropped.resize(px);
	return rt_robust_buffers{f.out.data(), f.mean.data(), f.gini.data(), f.trimmed.data(), f.dropped.data()};
}
} // namespace detail
inline RobustFrame render_robust(const RenderOptions &o, const SimpleCamera &camera, const Bvh &bvh, uint32_t sample_split = 0,
                                 const RobustOptions &r = RobustOptions(), uint64_t seed = 1, uint64_t sample_begin = 0)
{
	rt_render_opts opts = detail::noise_render_opts(o, sample_split, seed, sample_begin);
	opts.render_method = static_cast<int32_t>(o.render_method);
	const rt_robust_opts ropts = detail::robust_opts(r);
	RobustFrame f;
	const rt_robust_buffers b = detail::robust_frame(f, (size_t)o.width * o.height);
	check(rt_render_robust(bvh.raw(), &camera.raw(), &opts, &ropts, nullptr, &b, &f.rays_shot));
	return f;
}
// The same estimator on the caller's chunk sums, split * width * height * 3 floats laid out [chunk][y][x][3], each the sum of
// chunk_passes passes (rt_robust_combine); `bvh` names the GPU.
inline RobustFrame robust_combine(const Bvh &bvh, const std::vector<float> &chunk_sums, uint32_t split, uint64_t chunk_passes, uint32_t width,
                                  uint32_t height, const RobustOptions &r = RobustOptions())
{
	const rt_robust_opts ropts = detail::robust_opts(r);
	RobustFrame f;
	const rt_robust_buffers b = detail::robust_frame(f, (size_t)width * height);
	check(rt_robust_combine(bvh.raw(), chunk_sums.data(), split, chunk_passes, width, height, nullptr, &ropts, &b));
	return f;
}

// The A-Trous denoiser of rt_hip.h (rt_denoise_opts): the options a caller sets; defaults as rt_denoise_opts_default.
struct DenoiseOptions {
	uint32_t iterations = 5;
	float sigma_luminance = 4.0f, sigma_normal = 128.0f, sigma_depth = 0.1f;
};
inline rt_denoise_opts denoise_opts(const DenoiseOptions &d, uint32_t width, uint32_t height)
{
	rt_denoise_opts o;
	check(rt_denoise_opts_default(&o));
	o.width = width;
	o.height = height;
	o.iterations = d.iterations;
	o.sigma_luminance = d.sigma_luminance;
	o.sigma_normal = d.sigma_normal;
	o.sigma_depth = d.sigma_depth;
	return o;
}
// Filter a width*height*3 radiance frame (what render writes) guided by the albedo, normal and depth of `aov` (render_aov of the
// same passes; nullptr or an empty channel = that guide not used); the variance is estimated from the frame.  Blocking.
inline std::vector<float> denoise(const Bvh &bvh, const std::vector<float> &color, const AovBuffers *aov, uint32_t width,
                                  uint32_t height, const DenoiseOptions &d = DenoiseOptions())
{
	auto ptr = [](const std::vector<float> &v) { return v.empty() ? nullptr : v.data(); };
	rt_denoise_inputs in = {color.data(), nullptr, nullptr, nullptr, nullptr};
	if (aov) {
		in.albedo = ptr(aov->albedo);
		in.normal = ptr(aov->normal);
		in.depth = ptr(aov->depth);
	}
	const rt_denoise_opts o = denoise_opts(d, width, height);
	std::vector<float> out((size_t)width * height * 3);
	check(rt_denoise(bvh.raw(), &in, &o, out.data()));
	return out;
}
// Two half renders, the AOVs of all passes and the filter in one call (rt_render_denoised; o.samples_per_pixel even, >= 2).
struct Denoised {
	std::vector<float> clean, noisy; // w*h*3
	uint64_t rays_shot = 0;
};
inline Denoised render_denoised(const RenderOptions &o, const SimpleCamera &camera, const Bvh &bvh,
                                const DenoiseOptions &d = DenoiseOptions(), uint64_t seed = 1, uint64_t sample_begin = 0)
{
	rt_render_opts opts;
	rt_render_opts_default(&opts);
	opts.width = o.width;
	opts.height = o.height;
	opts.samples_per_pixel = o.samples_per_pixel;
	opts.render_method = static_cast<int32_t>(o.render_method);
	opts.sample_begin = sample_begin;
	opts.seed = seed;
	const rt_denoise_opts dopts = denoise_opts(d, 0, 0); // (the frame size comes from opts)
	Denoised r;
	r.clean.resize((size_t)o.width * o.height * 3);
	r.noisy.resize(r.clean.size());
	check(rt_render_denoised(bvh.raw(), &camera.raw(), &opts, &dopts, r.clean.data(), r.noisy.data(), &r.rays_shot));
	return r;
}

// The channels of render_aov_chain for the frame render_lens makes: every pass starts with that pass's lens ray (semantics:
// rt_hip.h rt_render_lens_aov).  `chain` nullptr: the first hit.  Guides for denoise and upscale of a lens frame.
inline AovChainBuffers render_lens_aov(const RenderOptions &o, const LensCamera &camera, const Bvh &bvh, const AovChainOptions *chain = nullptr,
                                       uint64_t seed = 1, uint64_t sample_begin = 0)
{
	rt_render_opts opts;
	rt_render_opts_default(&opts);
	opts.width = o.width;
	opts.height = o.height;
	opts.samples_per_pixel = o.samples_per_pixel;
	opts.sample_begin = sample_begin;
	opts.seed = seed;
	rt_aov_chain_opts copts;
	rt_aov_chain_opts_default(&copts);
	if (chain) {
		copts.max_chain = chain->max_chain;
		copts.fuzz_limit = chain->fuzz_limit;
	}
	const size_t n = (size_t)o.width * o.height;
	AovChainBuffers a;
	a.albedo.resize(n * 3);
	a.normal.resize(n * 3);
	a.depth.resize(n);
	a.coverage.resize(n);
	a.primitive.resize(n);
	a.material.resize(n);
	a.bounces.resize(n);
	const rt_aov_chain_buffers b = {{a.albedo.data(), a.normal.data(), a.depth.data(), a.coverage.data(), a.primitive.data(), a.material.data()},
	                                a.bounces.data()};
	check(rt_render_lens_aov(bvh.raw(), &camera.raw(), &opts, chain ? &copts : nullptr, &b));
	return a;
}
// render_denoised for a lens camera: two half render_lens frames, the render_lens_aov guides of all passes and the filter in one
// call (rt_render_lens_denoised; o.samples_per_pixel even, >= 2).
inline Denoised render_lens_denoised(const RenderOptions &o, const LensCamera &camera, const Bvh &bvh, const AovChainOptions *chain = nullptr,
                                     const DenoiseOptions &d = DenoiseOptions(), uint32_t sample_split = 1, uint64_t seed = 1,
                                     uint64_t sample_begin = 0)
{
	rt_render_opts opts = detail::noise_render_opts(o, sample_split, seed, sample_begin);
	opts.render_method = static_cast<int32_t>(o.render_method);
	rt_aov_chain_opts copts;
	rt_aov_chain_opts_default(&copts);
	if (chain) {
		copts.max_chain = chain->max_chain;
		copts.fuzz_limit = chain->fuzz_limit;
	}
	const rt_denoise_opts dopts = denoise_opts(d, 0, 0); // (the frame size comes from opts)
	Denoised r;
	r.clean.resize((size_t)o.width * o.height * 3);
	r.noisy.resize(r.clean.size());
	check(rt_render_lens_denoised(bvh.raw(), &camera.raw(), &opts, chain ? &copts : nullptr, &dopts, r.clean.data(), r.noisy.data(), &r.rays_shot));
	return r;
}

// Temporal accumulation with camera reprojection (rt_hip.h rt_temporal_opts): the options a caller sets; defaults as
// rt_temporal_opts_default.
struct TemporalOptions {
	DenoiseOptions denoise;
	float alpha_color = 0.2f, alpha_moments = 0.2f, depth_tolerance = 0.1f, normal_tolerance = 0.9f;
	uint32_t max_history = 32;
};
inline rt_temporal_opts temporal_opts(const TemporalOptions &t, uint32_t width, uint32_t height)
{
	rt_temporal_opts o;
	check(rt_temporal_opts_default(&o));
	o.denoise = denoise_opts(t.denoise, width, height);
	o.alpha_color = t.alpha_color;
	o.alpha_moments = t.alpha_moments;
	o.depth_tolerance = t.depth_tolerance;
	o.normal_tolerance = t.normal_tolerance;
	o.max_history = t.max_history;
	return o;
}
// One camera path through a static scene: each call filters one frame (render + render_aov of the same passes, with depth) and
// accumulates it with the frames before, reprojected through the camera change (rt_denoise_temporal; blocking).  The history
// buffers and the previous camera live on the scene: one TemporalDenoiser per scene at a time.  reset() (and a new frame size)
// starts over, e.g. at a cut.
class TemporalDenoiser {
  public:
	TemporalDenoiser(const Bvh &bvh, uint32_t width, uint32_t height, const TemporalOptions &t = TemporalOptions())
	    : bvh_(bvh), opts_(temporal_opts(t, width, height))
	{
		reset();
	}
	// returns the filtered frame (w*h*3); *motion (unless nullptr) gets w*h*2 floats, the pixel offsets into the previous frame
	std::vector<float> operator()(const std::vector<float> &color, const AovBuffers &aov, const SimpleCamera &camera,
	                              std::vector<float> *motion = nullptr)
	{
		auto ptr = [](const std::vector<float> &v) { return v.empty() ? nullptr : v.data(); };
		const rt_temporal_inputs in = {color.data(), ptr(aov.albedo), ptr(aov.normal), ptr(aov.depth)};
		const size_t n = (size_t)opts_.denoise.width * opts_.denoise.height;
		std::vector<float> out(n * 3);
		if (motion)
			motion->resize(n * 2);
		check(rt_denoise_temporal(bvh_.raw(), &in, &camera.raw(), &opts_, out.data(), motion ? motion->data() : nullptr));
		return out;
	}
	void reset() { check(rt_denoise_temporal_reset(bvh_.raw())); }

  private:
	const Bvh &bvh_;
	rt_temporal_opts opts_;
};

// The display stage (rt_hip.h rt_display_opts): the options a caller sets; defaults as rt_display_opts_default.
struct DisplayOptions {
	rt_exposure_mode exposure_mode = RT_EXPOSURE_AUTO;
	rt_tonemap tonemap = RT_TONEMAP_ACES;
	rt_transfer transfer = RT_TRANSFER_SRGB;
	rt_quantiser quantiser = RT_QUANT_DITHER;
	rt_pixel_format pixel_format = RT_PIXEL_RGBA8;
	float exposure_ev = 0.0f, key_ev = -2.47393119f, meter_low = 0.10f, meter_high = 0.90f, ev_min = -16.0f, ev_max = 16.0f;
	float adaptation = 1.0f, white = 4.0f, gamma = 2.2f;
	uint64_t seed = 0;
};
inline rt_display_opts display_opts(const DisplayOptions &d, uint32_t width, uint32_t height)
{
	rt_display_opts o;
	check(rt_display_opts_default(&o));
	o.width = width;
	o.height = height;
	o.exposure_mode = d.exposure_mode;
	o.tonemap = d.tonemap;
	o.transfer = d.transfer;
	o.quantiser = d.quantiser;
	o.pixel_format = d.pixel_format;
	o.exposure_ev = d.exposure_ev;
	o.key_ev = d.key_ev;
	o.meter_low = d.meter_low;
	o.meter_high = d.meter_high;
	o.ev_min = d.ev_min;
	o.ev_max = d.ev_max;
	o.adaptation = d.adaptation;
	o.white = d.white;
	o.gamma = d.gamma;
	o.seed = d.seed;
	return o;
}
// A sequence of frames to 8-bit display pixels (rt_display; blocking): each call meters, adapts the exposure from the frames
// before, tone-maps and quantises.  The exposure state lives on the scene: one Display per scene at a time.  reset() (and a new
// frame size) starts over, e.g. at a cut.
class Display {
  public:
	Display(const Bvh &bvh, uint32_t width, uint32_t height, const DisplayOptions &d = DisplayOptions())
	    : bvh_(bvh), opts_(display_opts(d, width, height))
	{
		reset();
	}
	// rgb: width*height*3 floats; returns width*height*4 (RGBA8 / BGRA8) or *3 (RGB8) bytes.  *state / *histogram (unless nullptr)
	// receive the state after the call and the 256 luminance counts.
	std::vector<uint8_t> operator()(const std::vector<float> &rgb, rt_display_state *state = nullptr,
	                                std::vector<uint32_t> *histogram = nullptr)
	{
		uint64_t bytes = 0;
		check(rt_display_output_bytes(&opts_, &bytes));
		std::vector<uint8_t> out((size_t)bytes);
		if (histogram)
			histogram->resize(256);
		check(rt_display(bvh_.raw(), rgb.data(), &opts_, out.data(), state, histogram ? histogram->data() : nullptr));
		return out;
	}
	void reset() { check(rt_display_reset(bvh_.raw())); }

  private:
	const Bvh &bvh_;
	rt_display_opts opts_;
};

// AOV-guided upscaling (rt_hip.h rt_upscale_opts): the options a caller sets; defaults as rt_upscale_opts_default.
struct UpscaleOptions {
	float sigma_normal = 32.0f, depth_tolerance = 0.1f;
};
inline rt_upscale_opts upscale_opts(const UpscaleOptions &u, uint32_t src_width, uint32_t src_height, uint32_t dst_width,
                                    uint32_t dst_height)
{
	rt_upscale_opts o;
	check(rt_upscale_opts_default(&o));
	o.src_width = src_width;
	o.src_height = src_height;
	o.dst_width = dst_width;
	o.dst_height = dst_height;
	o.sigma_normal = u.sigma_normal;
	o.depth_tolerance = u.depth_tolerance;
	return o;
}
// A src_width*src_height*3 frame to dst_width*dst_height*3, guided by the albedo, normal and depth of `src` and `dst` (render_aov at
// the two sizes; nullptr, or a channel empty in either, = that guide not used).  *stage (unless nullptr) receives the stage map.
inline std::vector<float> upscale(const Bvh &bvh, const std::vector<float> &color, const AovBuffers *src, const AovBuffers *dst,
                                  uint32_t src_width, uint32_t src_height, uint32_t dst_width, uint32_t dst_height,
                                  const UpscaleOptions &u = UpscaleOptions(), std::vector<uint8_t> *stage = nullptr)
{
	rt_upscale_inputs in = {color.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
	if (src && dst) {
		if (!src->albedo.empty() && !dst->albedo.empty()) {
			in.src_albedo = src->albedo.data();
			in.dst_albedo = dst->albedo.data();
		}
		if (!src->normal.empty() && !dst->normal.empty()) {
			in.src_normal = src->normal.data();
			in.dst_normal = dst->normal.data();
		}
		if (!src->depth.empty() && !dst->depth.empty()) {
			in.src_depth = src->depth.data();
			in.dst_depth = dst->depth.data();
		}
	}
	const rt_upscale_opts o = upscale_opts(u, src_width, src_height, dst_width, dst_height);
	const size_t n = (size_t)dst_width * dst_height;
	std::vector<float> out(n * 3);
	if (stage)
		stage->resize(n);
	check(rt_upscale(bvh.raw(), &in, &o, out.data(), stage ? stage->data() : nullptr));
	return out;
}
// Render at src_width x src_height, filter there, reconstruct o.width x o.height (rt_render_upscaled; o.samples_per_pixel even, >= 2).
struct Upscaled {
	std::vector<float> image;  // o.width*o.height*3
	std::vector<float> source; // src_width*src_height*3: the filtered frame that was upscaled
	uint64_t rays_shot = 0;
};
inline Upscaled render_upscaled(const RenderOptions &o, uint32_t src_width, uint32_t src_height, const SimpleCamera &camera,
                                const Bvh &bvh, const DenoiseOptions &d = DenoiseOptions(), const UpscaleOptions &u = UpscaleOptions(),
                                uint64_t seed = 1, uint64_t sample_begin = 0)
{
	rt_render_opts opts;
	rt_render_opts_default(&opts);
	opts.width = o.width;
	opts.height = o.height;
	opts.samples_per_pixel = o.samples_per_pixel;
	opts.render_method = static_cast<int32_t>(o.render_method);
	opts.sample_begin = sample_begin;
	opts.seed = seed;
	const rt_denoise_opts dopts = denoise_opts(d, 0, 0); // (the frame sizes come from opts and the two arguments)
	const rt_upscale_opts uopts = upscale_opts(u, 0, 0, 0, 0);
	Upscaled r;
	r.image.resize((size_t)o.width * o.height * 3);
	r.source.resize((size_t)src_width * src_height * 3);
	check(rt_render_upscaled(bvh.raw(), &camera.raw(), &opts, src_width, src_height, &dopts, &uopts, r.image.data(), r.source.data(),
	                         &r.rays_shot));
	return r;
}

// The depth-of-field stage (rt_hip.h rt_dof_opts): the options a caller sets; defaults as rt_dof_opts_default.
struct DofOptions {
	float focus_distance = 10.0f, blur_scale = 0.0f;
	uint32_t max_radius = 8;
	bool planar_depth = true;
};
inline rt_dof_opts dof_opts(const DofOptions &d, uint32_t width, uint32_t height)
{
	rt_dof_opts o;
	check(rt_dof_opts_default(&o));
	o.width = width;
	o.height = height;
	o.focus_distance = d.focus_distance;
	o.blur_scale = d.blur_scale;
	o.max_radius = d.max_radius;
	o.planar_depth = d.planar_depth ? 1u : 0u;
	return o;
}
// A scene file's `aperture` and `focus_dis` as a blur (rt_dof_opts_from_camera); `camera` is the one made with that focus_dist.
inline DofOptions dof_options_from_camera(const SimpleCamera &camera, float aperture, float focus_dist, uint32_t width, uint32_t height,
                                          uint32_t max_radius = 8)
{
	rt_dof_opts o;
	check(rt_dof_opts_from_camera(&o, &camera.raw(), aperture, focus_dist, width, height));
	DofOptions d;
	d.focus_distance = o.focus_distance;
	d.blur_scale = o.blur_scale;
	d.max_radius = max_radius;
	d.planar_depth = true;
	return d;
}
// A width*height*3 frame and its width*height depth plane (render_aov's) to the defocused frame; camera nullptr: planar_depth
// must be false.  *coc (unless nullptr) receives the signed circle-of-confusion radii.
inline std::vector<float> dof(const Bvh &bvh, const std::vector<float> &color, const std::vector<float> &depth, const SimpleCamera *camera,
                              uint32_t width, uint32_t height, const DofOptions &d = DofOptions(), std::vector<float> *coc = nullptr)
{
	const rt_dof_opts o = dof_opts(d, width, height);
	const size_t n = (size_t)width * height;
	std::vector<float> out(n * 3);
	if (coc)
		coc->resize(n);
	check(rt_dof(bvh.raw(), color.data(), depth.data(), camera ? &camera->raw() : nullptr, &o, out.data(), coc ? coc->data() : nullptr));
	return out;
}
// Render, take the depth of the same passes and defocus, in one call (rt_render_dof).
inline std::vector<float> render_dof(const RenderOptions &o, const SimpleCamera &camera, const Bvh &bvh, const DofOptions &d,
                                     uint64_t seed = 1, uint64_t sample_begin = 0)
{
	rt_render_opts opts;
	rt_render_opts_default(&opts);
	opts.width = o.width;
	opts.height = o.height;
	opts.samples_per_pixel = o.samples_per_pixel;
	opts.render_method = static_cast<int32_t>(o.render_method);
	opts.sample_begin = sample_begin;
	opts.seed = seed;
	const rt_dof_opts dopts = dof_opts(d, 0, 0); // (the frame size comes from opts)
	std::vector<float> out((size_t)o.width * o.height * 3);
	check(rt_render_dof(bvh.raw(), &camera.raw(), &opts, &dopts, out.data()));
	return out;
}

struct Presentation { // what render_tui keeps: the mean image and the ray total (src/main.rs:160-173)
	SamplerProgress sampler_progress;
	Presentation(uint64_t pixel_num) : sampler_progress(pixel_num, 3) {}
};
inline bool running_mean(Presentation *sp, const SamplerProgressRef &previous, uint64_t i)
{
	sp->sampler_progress.samples_completed += previous.samples_completed;
	sp->sampler_progress.rays_shot += previous.rays_shot;
	const float w = (float)previous.samples_completed / (float)i;
	for (size_t k = 0; k < previous.current_image.size(); ++k) {
		float &pres = sp->sampler_progress.current_image[k];
		pres += (previous.current_image[k] - pres) * w; // *pres += (acc - *pres) / i for batch = 1
	}
	return false;
}

} // namespace rt_hip
