// rt_api_internal.h -- what the host translation units of librt_hip.so share (rt_api.cpp, rt_api_post.cpp, rt_api_query.cpp): the
// scene handle, the error convention, and the plumbing every blocking entry point repeats; rt_output.cpp takes the error
// convention from it.  Not installed, not part of include/.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "../../include/rt_hip.h"
#include "rt_build.h"
#include "rt_layout.h"
#include "rt_types.h"
#include "rt_sky_tiles.h"
#include "rt_sky_cell.h"
#include "rt_aov.h"

// the text behind rt_last_error(): ONE per thread for the whole library (defined in rt_api.cpp)
extern thread_local std::string g_error;

inline int fail(int code, const std::string &msg)
{
	g_error = msg;
	return code;
}
inline int hip_fail(hipError_t e, const char *what)
{
	g_error = std::string(what) + ": " + hipGetErrorString(e);
	return e == hipErrorOutOfMemory ? RT_ERR_OUT_OF_MEMORY : RT_ERR_HIP;
}
#define HIP_TRY(expr)                       \
	do {                                    \
		hipError_t e_ = (expr);             \
		if (e_ != hipSuccess)               \
			return hip_fail(e_, #expr);     \
	} while (0)
// the same for a call that returns an rt status (its message is set already)
#define RT_TRY(expr)            \
	do {                        \
		const int rc_ = (expr); \
		if (rc_ != RT_OK)       \
			return rc_;         \
	} while (0)

// the pruned walk above this many primitives, the exhaustive one up to it (measured: see the crossovers in rt_api.cpp)
constexpr uint32_t kPruneAbove = 100;

// RT_TUNE_WHOLE_PIXEL_SHARE when nobody sets it: -1, the planner's own choice by tiles per resident wave (rt_api.cpp plan_work_items)
constexpr int kWholeShareDefault = -1;

struct rt_scene {
	int device = 0;
	rt::HostScene host;
	rt::DevScene dev{};
	std::vector<void *> allocations;
	hipStream_t stream = nullptr; // used by the blocking entry points
	uint32_t *d_work_counter = nullptr;
	unsigned long long *d_rays = nullptr;
	hipEvent_t ev_start = nullptr, ev_stop = nullptr;
	bool timed = false;
	uint32_t n_launches = 0;
	int n_cus = 0;
	int traversal_mode = -1; // -1 auto, 0 exhaustive (reference order of work), 1 pruned
	int schedule_mode = -1;  // -1 auto, 0 coarse (two super-phases), 1 fine (every step voted)
	int feature_set = 2;     // smallest kernel variant covering the scene: 0 spheres-only, 1 simple, 2 full
	int min_feature_set = 0; // what the scene needs (feature_set may be forced larger for tests)
	// the tree is one inner node over two leaves of one primitive each: launches that would run the spheres-only exhaustive
	// coarse kernels run their FeatPair twins (rt_types.h) -- unless a feature set was asked for by name (RT_TUNE_FEATURE_SET)
	bool pair_tree = false, feature_set_forced = false;
	rt::DevPairScene pair{}; // pair_tree: the scene as the FeatPair kernels take it, in their kernel arguments (rt_types.h)
	bool scene_lds_allowed = true;
	float *d_partial = nullptr; // sample_split > 1: per-chunk means, grown on demand
	size_t partial_floats = 0;
	// rt_sample_image: two batches in flight (device + pinned host buffers, copy stream, events)
	float *d_prog[2] = {nullptr, nullptr};
	float *h_prog[2] = {nullptr, nullptr};
	unsigned long long *d_prog_rays = nullptr; // [2]
	unsigned long long *h_prog_rays = nullptr; // [2], pinned
	size_t d_prog_floats[2] = {0, 0}, h_prog_floats[2] = {0, 0};
	hipStream_t copy_stream = nullptr;
	hipEvent_t ev_batch[2] = {nullptr, nullptr}, ev_copy[2] = {nullptr, nullptr};
	size_t max_lds = 65536;
	rt_launch_info last_launch{};
	uint32_t stack_cap_override = 0; // RT_TUNE_STACK_CAP
	int exchange_mode = 0;           // RT_TUNE_EXCHANGE
	int whole_share = kWholeShareDefault; // RT_TUNE_WHOLE_PIXEL_SHARE
	uint32_t radiance_groups = 0;    // RT_TUNE_RADIANCE_GROUPS (rt_radiance and rt_render_tiles)
	int sky_run = -1;                // RT_TUNE_SKY_RUN: -1 automatic (on where the kernel has it), 0 off, 1 on
	rt::DevSkyCell sky_cell = {};    // the carried sky cell's guard for this scene's sky (rt_sky_cell.h), as the two-sphere kernels are told it
	uint32_t sky_cell_proven = 0;    // sky_cell_guard(...).ok: what RT_TUNE_SKY_CELL != 0 puts in sky_cell.ok
	uint32_t stack_depth_narrow = 2; // HostScene::stack_depth_narrow (members of a multi-device scene have no host scene of their own)
	uint32_t *d_stack_ovf = nullptr; // traversal-stack overflow area (deep trees under the fine schedule), grown on demand
	size_t stack_ovf_words = 0;
	uint8_t *d_rgb8 = nullptr; // rt_render_rgb8: the quantised frame
	size_t d_rgb8_bytes = 0;
	// ---- multi-device scenes (rt_scene_create_multi).  The handle a caller holds is the HEAD: an ordinary scene on
	// devices[0] that additionally owns one member scene per further device (uploaded from the head's host build) and
	// gathers their tile shards into its own frames.  Members render like any single-device scene. ----
	std::vector<rt_scene *> peers;         // head only: the members on devices[1..n-1]
	bool member_call = false;              // set while the head renders its own shard through the single-device path
	float *d_shard = nullptr;              // every member incl. the head: its packed shard (RT_LAYOUT_SHARD)
	size_t shard_floats = 0;
	unsigned long long *d_member_rays = nullptr; // the member's own ray counter (the head's d_rays holds the job's total)
	hipEvent_t ev_shard = nullptr;         // member: its shard is rendered
	hipEvent_t ev_begin = nullptr;         // head: the caller's stream has reached this render
	float *d_gather = nullptr;             // head: the peers' shards, once gathered
	size_t gather_floats = 0;
	unsigned long long *d_gather_rays = nullptr; // head: [n] the members' ray counters
	void *nccl_comms = nullptr;            // head: ncclComm_t[n] when the devices are distinct and RCCL is usable
	int gather_mode = 0;                   // rt_gather_mode, decided when the scene is created (rt_scene_create_multi)
	std::string gather_note;               // why (rt_scene_gather_info)
	hipEvent_t ev_gathered = nullptr;      // head: the last render's gather + scatter have read every member's shard
	bool gathered_once = false;
	uint32_t *d_prim_desc = nullptr;       // AOV passes: BVH slot -> rt_scene_desc index, uploaded with the scene (in `allocations`)
	char *d_denoise = nullptr;             // rt_denoise / rt_render_denoised: device frames + workspace, grown on first use
	size_t d_denoise_bytes = 0;
	char *d_temporal = nullptr;            // rt_denoise_temporal: its two history buffers, for frames of temporal_w x temporal_h
	uint32_t temporal_w = 0, temporal_h = 0;
	int temporal_cur = -1;                 // the history buffer the last call wrote; -1 = no history
	rt_camera temporal_prev{};             // the camera of that call
	char *d_display = nullptr;             // rt_display: state, histogram, workspace, output and input, grown for larger frames
	size_t d_display_bytes = 0;
	uint32_t display_w = 0, display_h = 0; // the frame size of the last successful call
	bool display_has_state = false;        // false: the next rt_display starts from a zero state
	char *d_noise = nullptr;               // rt_render_noise & co.: the batch state (noise_state, rt_api_post.cpp), then what the blocking calls stage
	size_t d_noise_bytes = 0;
	char *d_bloom = nullptr;               // rt_bloom: state, workspace, input and output, grown for larger frames
	size_t d_bloom_bytes = 0;
	char *d_dof = nullptr;                 // rt_dof / rt_render_dof: workspace, output, frame, depth and CoC plane, grown for larger frames
	size_t d_dof_bytes = 0;
};

// sample_split = 0 (automatic), resolved (rt_api.cpp); the noise estimates halve it until it divides the passes (rt_api_post.cpp)
uint32_t auto_sample_split(int n_cus, uint64_t frame_pixels, uint64_t spp, uint32_t n_sharers);
// the work items of a launch in the tiled order: whole-pixel claims first, chunk claims for the tiles left over (rt_api.cpp)
struct WorkItems { uint64_t whole_claims, n_items; };
WorkItems plan_work_items(uint64_t tiles, uint64_t tile_pixels, uint32_t split, bool tiled, int share, uint64_t resident_waves);

// the bytes of the sky's CDF tables and guides: what a launch compares with kSkyLdsLimit before it asks for them in LDS
constexpr size_t kSkyLdsLimit = 96 * 1024;
inline size_t sky_table_bytes(uint32_t res_x, uint32_t res_y, uint32_t guide_k)
{
	if ((res_x | res_y) == 0u)
		return 0;
	return ((size_t)res_y * (res_x + 1u) + res_y + 1u) * 4 + (size_t)(res_y + 1u) * guide_k;
}

// ---- traversal policy: which walk, and for the four-wave kernels which tree and how much stack ----
// the walk every launch on this scene takes (rt_scene_set_traversal / RT_TUNE_TRAVERSAL, else by size); the fine schedule of
// the render kernels additionally implies the pruned walk (plan_render_launch, rt_api.cpp)
inline bool scene_prunes(const rt_scene *s)
{
	return s->traversal_mode == -1 ? s->dev.n_prims > kPruneAbove : s->traversal_mode == 1;
}

// The batch hit queries and both AOV passes keep the whole worst-case stack of their four waves in LDS
// (four_wave_stack_lds_bytes, rt_types.h): the wide tree's only where it is walked and fits the LDS of a CU, the two-child
// tree's (and the two-child walk for every ray: narrow_only) otherwise -- the fallback the coarse render kernels take.  *dev is
// the scene as such a launch sees it.  A scene whose two-child stack does not fit either is refused; no test builds one: a
// two-child tree deeper than 160 levels cannot be made from finite float coordinates with the generators of tests/scenes.py.
// On this hardware the refusal is unreachable whatever the scene: the build caps stack_depth at 96 entries, and
// 4 waves x 96 x 256 B = 98 304 B is below the 160 KB of a CU, so the branch is live only on a device that reports less LDS.
inline int four_wave_traversal(const rt_scene *s, bool *prune, rt::DevScene *dev)
{
	*prune = scene_prunes(s);
	*dev = s->dev;
	const bool walks_wide = *prune && dev->nodes4 != nullptr && dev->narrow_only == 0u;
	if (!walks_wide || rt::four_wave_stack_lds_bytes(*dev) > s->max_lds) {
		if (walks_wide)
			dev->narrow_only = 1u;
		dev->stack_depth = s->stack_depth_narrow;
	}
	if (rt::four_wave_stack_lds_bytes(*dev) > s->max_lds)
		return fail(RT_ERR_UNSUPPORTED, "traversal stacks exceed the LDS of one CU");
	return RT_OK;
}

// The workgroups of a launch of the per-lane path kernels (rt_radiance, rt_render_tiles): what the device holds at once -- `waves`
// workgroups a CU by registers, fewer where their `lds_bytes` of dynamic LDS allow fewer (160 KB a CU) -- never more than the
// `wanted` the work fills (so that a short batch launches no idle workgroup; beyond that lanes refill) and never none;
// RT_TUNE_RADIANCE_GROUPS caps it.
inline uint32_t path_lane_groups(const rt_scene *s, size_t lds_bytes, uint32_t waves, uint64_t wanted)
{
	const uint64_t by_lds = std::max<uint64_t>(1, (160u * 1024u) / std::max<size_t>(1, lds_bytes));
	const uint64_t resident = (uint64_t)std::max(1, s->n_cus) * std::min<uint64_t>(waves, by_lds);
	uint64_t groups = std::min<uint64_t>(wanted, resident);
	if (s->radiance_groups != 0u)
		groups = std::min<uint64_t>(groups, s->radiance_groups);
	return (uint32_t)std::max<uint64_t>(groups, 1);
}

// ---- the geometry of a frame and the camera, as every launch takes them ----

// the 8 x 8 tile grid of a w x h frame (rt_noise_tiles' grid: AOV passes, tile errors, tile lists): tiles across, and how many
struct TileGrid { uint32_t tiles_x; uint64_t count; };
inline TileGrid tile_grid(uint64_t w, uint64_t h)
{
	const uint64_t across = (w + 7) / 8, down = (h + 7) / 8;
	return TileGrid{(uint32_t)across, across * down};
}

// the tiling of a whole-frame render under `o` (tile_width / tile_height 0: 8): what the render kernel hands out as work items, and
// what the readers of its chunk sums find pixels by.  n_work counts the padding of edge tiles.
struct FrameTiling { uint32_t tile_w, tile_h, tiles_x, tiles_y; uint64_t n_work; };
inline FrameTiling frame_tiling(const rt_render_opts *o)
{
	FrameTiling t;
	t.tile_w = o->tile_width ? o->tile_width : 8;
	t.tile_h = o->tile_height ? o->tile_height : 8;
	t.tiles_x = (uint32_t)((o->width + t.tile_w - 1) / t.tile_w);
	t.tiles_y = (uint32_t)((o->height + t.tile_h - 1) / t.tile_h);
	t.n_work = (uint64_t)t.tiles_x * t.tiles_y * t.tile_w * t.tile_h;
	return t;
}

// RT_TUNE_SKY_RUN resolved for a launch of `feature_set` over a shard of n_work pixels (padding included) in the tiled order or not:
// the two-sphere kernels alone have the run (rt_render.hip kSkyRun), the flag needs bit 30 of the wave's pixel base, and only the
// tiled order flags claims.  Automatic equals on.
constexpr uint64_t kPairMaxWork = 1ull << 30; // pixels of a shard, padding included, the two-sphere kernels are launched for (rt_api.cpp)
inline bool sky_run_applies(const rt_scene *s, int feature_set, uint64_t n_work, bool tiled)
{
	return s->sky_run != 0 && feature_set == 3 && tiled && n_work < kPairMaxWork;
}
// the block the per-tile proof reads (rt_sky_tiles.h), for this scene, camera and image size; enabled = 0 unless the run applies
inline rt::DevSkyTiles sky_tiles_block(const rt_scene *s, const rt::DevPairPrimary &primary, const rt::DevCamera &cam, uint32_t width, uint32_t height, bool applies)
{
	rt::DevSkyTiles t{};
	if (applies && s->pair_tree)
		rt::sky_tiles_terms(s->pair, primary, cam, width, height, t);
	return t;
}

inline rt::DevCamera dev_camera(const rt_camera *camera)
{
	rt::DevCamera cam;
	std::memcpy(cam.origin, camera->origin, 12);
	std::memcpy(cam.lower_left, camera->lower_left, 12);
	std::memcpy(cam.horizontal, camera->horizontal, 12);
	std::memcpy(cam.vertical, camera->vertical, 12);
	return cam;
}

template <class T> static int upload(rt_scene *s, const T *src, size_t count, const T **dst)
{
	void *p = nullptr;
	const size_t bytes = (count ? count : 1) * sizeof(T);
	HIP_TRY(hipMalloc(&p, bytes));
	s->allocations.push_back(p);
	if (count)
		HIP_TRY(hipMemcpy(p, src, count * sizeof(T), hipMemcpyHostToDevice));
	*dst = static_cast<const T *>(p);
	return RT_OK;
}

inline bool ranges_overlap(const void *a, uint64_t a_bytes, const void *b, uint64_t b_bytes)
{
	if (!a || !b)
		return false;
	const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
	return x < y + b_bytes && y < x + a_bytes;
}

// ---- the argument checks and buffer plumbing the entry points share ----

// the last check of an entry point that computes (so that a host-only scene still reports bad arguments as such)
inline int need_device(const rt_scene *s)
{
	if (s->device == RT_DEVICE_NONE)
		return fail(RT_ERR_NO_DEVICE, "host-only scene (RT_DEVICE_NONE): this call needs a GPU, there is no CPU fallback");
	return RT_OK;
}

// both sides of a frame >= min_side (2 where u and v divide by W-1 and H-1); `stage` starts the message: "denoise: ", or ""
inline int frame_sides(const char *stage, uint64_t w, uint64_t h, uint64_t min_side)
{
	if (w >= min_side && h >= min_side)
		return RT_OK;
	return fail(RT_ERR_INVALID_ARGUMENT, stage + ("width and height must be >= " + std::to_string(min_side)) +
	                                         (min_side >= 2 ? " (u and v divide by W-1 and H-1)" : ""));
}

// the sides, then *n = w * h, refused above 2^31 pixels (a side above 2^31 too: the product must not wrap).  A stage that reports
// its other options between the two checks calls frame_sides first and this last.
inline int frame_pixels(const char *stage, uint64_t w, uint64_t h, uint64_t min_side, uint64_t *n)
{
	if (const int rc = frame_sides(stage, w, h, min_side); rc != RT_OK)
		return rc;
	if (w > (1ull << 31) || h > (1ull << 31) || w * h > (1ull << 31))
		return fail(RT_ERR_UNSUPPORTED, std::string(stage) + "more than 2^31 pixels");
	*n = w * h;
	return RT_OK;
}

// each of the first n_written buffers against every other of the n_total (those only read may share memory); NULL overlaps nothing
inline int check_disjoint(const char *message, const void *const buf[], const uint64_t bytes[], int n_written, int n_total)
{
	for (int a = 0; a < n_written; ++a)
		for (int b = 0; b < n_total; ++b)
			if (a != b && ranges_overlap(buf[a], bytes[a], buf[b], bytes[b]))
				return fail(RT_ERR_INVALID_ARGUMENT, message);
	return RT_OK;
}

// a scene-owned device buffer of `count` elements, replaced (contents dropped) when `need` is larger; nothing is held after a failure
template <class T> static int grow_device_buffer(T *&p, size_t &count, size_t need)
{
	if (need <= count)
		return RT_OK;
	if (p)
		(void)hipFree(p);
	p = nullptr;
	count = 0;
	HIP_TRY(hipMalloc(reinterpret_cast<void **>(&p), need * sizeof(T)));
	count = need;
	return RT_OK;
}

// a scene-owned byte buffer carved by `L` (rt_layout.h): the one way such a buffer gets its size, and L its base
static int grow_device_buffer(char *&p, size_t &bytes, rt::Layout &L)
{
	if (L.overflowed)
		return fail(RT_ERR_UNSUPPORTED, "internal: a buffer layout of more parts than rt::Layout holds");
	const int rc = grow_device_buffer(p, bytes, (size_t)L.total());
	L.base = p;
	return rc;
}

// ---- what the lens cameras (rt_api_lens.cpp) take from the post-processing stages (rt_api_post.cpp) ----
// the launch parameters of an AOV pass over the frame of `o` (cam: `camera`), and the option ranges of a chain
rt::DevAovParams aov_params(const rt_scene *s, const rt_camera *camera, const rt_render_opts *o, const rt_aov_buffers *d_out, uint32_t mask);
int aov_chain_opts_check(const rt_aov_chain_opts *c);
// a blocking AOV entry point once its arguments are checked: `enqueue` is its _device form on s->stream, handed the staged channels
int render_aov_staged(rt_scene *s, const rt_render_opts *o, const rt_aov_buffers &a, float *bounces, const char *what,
                      const std::function<int(const rt_aov_chain_buffers &)> &enqueue);
// rt_render_denoised's steps that depend on the camera, both on s->stream: a half render into a device frame and ray counter, and
// the albedo / normal / depth guides of all passes
struct DenoisedSource {
	std::function<int(const rt_render_opts *half_opts, float *d_rgb, uint64_t *d_rays)> half;
	std::function<int(const rt_render_opts *opts, const rt_aov_buffers &d_guides)> guides;
};
int render_denoised_opts_check(const char *who, const rt_render_opts *o, const rt_denoise_opts *dopts, uint64_t w, uint64_t h);
// ... once its arguments are checked and the scene has a device
int render_denoised_staged(rt_scene *s, const DenoisedSource &src, const rt_render_opts *o, const rt_denoise_opts *dopts, const char *what,
                           float *out_clean, float *out_noisy, uint64_t *rays_shot);

// The copies and the status of one blocking entry point on s->stream.  Copies are skipped for a NULL (optional) side and once
// anything has failed; finish() always drains the stream.  Which error wins: a non-OK `rc` (set by the caller from the _device
// call, its message kept), else the first HIP error in `e`, else the synchronise error.  Where the device side of a copy is a
// part of a carved buffer, put / get take it as (layout, part): the part's size is the copy's.
struct Staging {
	rt_scene *s;
	int rc = RT_OK;
	hipError_t e = hipSuccess;

	bool ok() const { return rc == RT_OK && e == hipSuccess; }
	void copy(void *dst, const void *src, size_t bytes, hipMemcpyKind kind)
	{
		if (dst && src && ok())
			e = hipMemcpyAsync(dst, src, bytes, kind, s->stream);
	}
	void to_device(void *d, const void *h, size_t bytes) { copy(d, h, bytes, hipMemcpyHostToDevice); }
	void download(void *h, const void *d, size_t bytes) { copy(h, d, bytes, hipMemcpyDeviceToHost); }
	// (always inlined: the library exports no symbol of its host plumbing)
	template <class T> __attribute__((always_inline)) void put(const rt::Layout &L, rt::Layout::Part<T> p, const void *h) { to_device(L.at(p), h, L.size_of(p)); }
	template <class T> __attribute__((always_inline)) void get(void *h, const rt::Layout &L, rt::Layout::Part<T> p) { download(h, L.at(p), L.size_of(p)); }
	int finish(const char *what)
	{
		const hipError_t e_sync = hipStreamSynchronize(s->stream);
		if (ok())
			e = e_sync;
		if (rc == RT_OK && e != hipSuccess)
			rc = hip_fail(e, what);
		return rc;
	}
};
