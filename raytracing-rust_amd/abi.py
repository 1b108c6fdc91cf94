"""ctypes mirror of include/rt_hip.h (the C ABI of librt_hip.so).

Field order and types must match the header exactly; tests/test_abi.py checks the struct
sizes against the values the C compiler reports.
"""
import ctypes as C

RT_ABI_VERSION = 2
RT_GATHER_NONE, RT_GATHER_RCCL, RT_GATHER_PEER, RT_GATHER_PEER_STAGED, RT_GATHER_SAME_DEVICE = 0, 1, 2, 3, 4

RT_OK = 0
RT_ERR_INVALID_ARGUMENT = -1
RT_ERR_NO_DEVICE = -2
RT_ERR_HIP = -3
RT_ERR_OUT_OF_MEMORY = -4
RT_ERR_UNSUPPORTED = -5

# enum AllTextures (textures/mod.rs:18-25)
RT_TEX_CHECKERED, RT_TEX_SOLID, RT_TEX_IMAGE, RT_TEX_LERP, RT_TEX_PERLIN = range(5)
# enum AllMaterials (materials/mod.rs:18-25)
RT_MAT_EMIT, RT_MAT_LAMBERTIAN, RT_MAT_TROWBRIDGE_REITZ, RT_MAT_REFLECT, RT_MAT_REFRACT = range(5)
# enum AllPrimitives (primitives/mod.rs:14-19)
RT_PRIM_SPHERE, RT_PRIM_TRIANGLE, RT_PRIM_MESH_TRIANGLE = range(3)
# enum SplitType (acceleration/split.rs:34-45)
RT_SPLIT_SAH, RT_SPLIT_MIDDLE, RT_SPLIT_EQUAL_COUNTS = range(3)
# enum RenderMethod (samplers/mod.rs:43-47)
RT_METHOD_NAIVE, RT_METHOD_MIS = range(2)
RT_LAYOUT_FRAME, RT_LAYOUT_SHARD = range(2)
RT_TUNE_TRAVERSAL, RT_TUNE_FEATURE_SET, RT_TUNE_SCENE_IN_LDS, RT_TUNE_SCHEDULE, RT_TUNE_WALK, RT_TUNE_STACK_CAP, RT_TUNE_EXCHANGE, RT_TUNE_WHOLE_PIXEL_SHARE = range(8)
RT_TUNE_RADIANCE_GROUPS = 8  # rt_radiance, rt_render_tiles: at most that many workgroups (0: automatic)
RT_TUNE_SKY_CELL = 11  # two-sphere kernels: the sampled sky cell carried to its pdf (-1 automatic = on where proven, 0 off, 1 as -1)
RT_TUNE_SKY_RUN = 10  # two-sphere kernels: tiles that can only see sky run without a walk (-1 automatic = on, 0 off, 1 on); 9 is unassigned

NO_INDEX = 0xFFFFFFFFFFFFFFFF  # usize::MAX
RT_DEVICE_NONE = -1  # rt_scene_create: Bvh::new on the host only (no GPU touched, nothing can be rendered)

f32x3 = C.c_float * 3


class TextureDesc(C.Structure):
    _fields_ = [
        ("type", C.c_int32),
        ("colour_one", f32x3),
        ("colour_two", f32x3),
        ("image_rgb", C.POINTER(C.c_float)),
        ("image_width", C.c_uint32),
        ("image_height", C.c_uint32),
        ("perlin_ran_vecs", C.POINTER(C.c_float)),
        ("perlin_perm", C.POINTER(C.c_uint32)),
    ]


class MaterialDesc(C.Structure):
    _fields_ = [
        ("type", C.c_int32),
        ("texture", C.c_uint32),
        ("param", C.c_float),
        ("ior", f32x3),
        ("metallic", C.c_float),
    ]


class _Sphere(C.Structure):
    _fields_ = [("centre", f32x3), ("radius", C.c_float)]


class _MeshTriangle(C.Structure):
    _fields_ = [("mesh", C.c_uint32), ("point_indices", C.c_uint32 * 3), ("normal_indices", C.c_uint32 * 3)]


class _Triangle(C.Structure):
    _fields_ = [("data", C.c_uint64)]


class _PrimUnion(C.Union):
    _fields_ = [("sphere", _Sphere), ("mesh_triangle", _MeshTriangle), ("triangle", _Triangle)]


class PrimitiveDesc(C.Structure):
    _fields_ = [("type", C.c_int32), ("material", C.c_uint32), ("u", _PrimUnion)]


class TriangleData(C.Structure):
    _fields_ = [("points", C.c_float * 9), ("normals", C.c_float * 9)]


class MeshDesc(C.Structure):
    _fields_ = [
        ("vertices", C.POINTER(C.c_float)),
        ("n_vertices", C.c_uint64),
        ("normals", C.POINTER(C.c_float)),
        ("n_normals", C.c_uint64),
    ]


class SkyDesc(C.Structure):
    _fields_ = [
        ("texture", C.c_uint32),
        ("material", C.c_uint32),
        ("sampler_res_x", C.c_uint32),
        ("sampler_res_y", C.c_uint32),
    ]


class SceneDesc(C.Structure):
    _fields_ = [
        ("abi_version", C.c_uint32),
        ("n_textures", C.c_uint32),
        ("textures", C.POINTER(TextureDesc)),
        ("n_materials", C.c_uint32),
        ("n_meshes", C.c_uint32),
        ("materials", C.POINTER(MaterialDesc)),
        ("meshes", C.POINTER(MeshDesc)),
        ("n_primitives", C.c_uint64),
        ("primitives", C.POINTER(PrimitiveDesc)),
        ("n_triangles", C.c_uint64),
        ("triangles", C.POINTER(TriangleData)),
        ("sky", SkyDesc),
        ("split_type", C.c_int32),
    ]


class Camera(C.Structure):
    _fields_ = [("origin", f32x3), ("lower_left", f32x3), ("horizontal", f32x3), ("vertical", f32x3)]


class RenderOpts(C.Structure):
    _fields_ = [
        ("width", C.c_uint64),
        ("height", C.c_uint64),
        ("samples_per_pixel", C.c_uint64),
        ("sample_begin", C.c_uint64),
        ("seed", C.c_uint64),
        ("render_method", C.c_int32),
        ("max_depth", C.c_uint32),
        ("rr_threshold", C.c_uint32),
        ("shard_index", C.c_uint32),
        ("shard_count", C.c_uint32),
        ("tile_width", C.c_uint32),
        ("tile_height", C.c_uint32),
        ("output_layout", C.c_int32),
        ("sample_split", C.c_uint32),
        ("reserved0", C.c_uint32),
    ]


class HitRecord(C.Structure):
    _fields_ = [
        ("t", C.c_float),
        ("point", f32x3),
        ("error", f32x3),
        ("normal", f32x3),
        ("uv", C.c_float * 2),
        ("has_uv", C.c_int32),
        ("out", C.c_int32),
        ("material", C.c_uint32),
        ("found", C.c_uint32),
        ("index", C.c_uint64),
    ]


class RayDesc(C.Structure):
    _fields_ = [("origin", f32x3), ("direction", f32x3)]


class BvhNode(C.Structure):
    _fields_ = [
        ("min", f32x3),
        ("max", f32x3),
        ("children", C.c_int64 * 2),
        ("primitive_offset", C.c_uint64),
        ("number_primitives", C.c_uint64),
    ]


# sizes the C compiler must agree with (x86-64 SysV); checked by tests/test_abi.py
class SamplerProgressC(C.Structure):  # rt_sampler_progress
    _fields_ = [
        ("samples_completed", C.c_uint64),
        ("rays_shot", C.c_uint64),
        ("current_image", C.POINTER(C.c_float)),
        ("n_floats", C.c_uint64),
    ]


class LaunchInfo(C.Structure):  # rt_launch_info
    _fields_ = [
        ("method", C.c_int32),
        ("pruned", C.c_int32),
        ("fine", C.c_int32),
        ("sky_in_lds", C.c_int32),
        ("scene_in_lds", C.c_int32),
        ("feature_set", C.c_int32),
        ("block_threads", C.c_uint32),
        ("n_blocks", C.c_uint32),
        ("blocks_per_cu", C.c_uint32),
        ("waves_per_simd", C.c_uint32),
        ("lds_bytes", C.c_uint32),
        ("n_cus", C.c_uint32),
        ("sample_split", C.c_uint32),
        ("whole_claims", C.c_uint32),
        ("n_items", C.c_uint64),
        ("sky_run", C.c_uint32),
        ("reserved", C.c_uint32),
        ("kernel", C.c_char * 152),
    ]


class SkyInfo(C.Structure):  # rt_sky_info
    _fields_ = [
        ("res_x", C.c_uint32),
        ("res_y", C.c_uint32),
        ("guide_k", C.c_uint32),
        ("inv_res_ok", C.c_uint32),
        ("inv_res_x", C.c_float),
        ("inv_res_y", C.c_float),
        ("table_bytes", C.c_uint64),
    ]


# Channel tables: one beside each struct of pointers, {channel: the shape of its array} -- "hw" (h, w), "hw3" (h, w, 3), "lhw"
# (layers, h, w), "tiles" (the NOISE_TILE grid: (ceil(h/8), ceil(w/8))) or "summary" (one struct, not an array).  The element type
# is the field's own (see channels()); a nested table stands under the name of the nested struct's field.
class AovBuffers(C.Structure):  # rt_aov_buffers
    _fields_ = [
        ("albedo", C.POINTER(C.c_float)),
        ("normal", C.POINTER(C.c_float)),
        ("depth", C.POINTER(C.c_float)),
        ("coverage", C.POINTER(C.c_float)),
        ("primitive", C.POINTER(C.c_uint32)),
        ("material", C.POINTER(C.c_uint32)),
    ]


AOV_SHAPES = {"albedo": "hw3", "normal": "hw3", "depth": "hw", "coverage": "hw", "primitive": "hw", "material": "hw"}
AOV_CHANNELS = tuple(AOV_SHAPES)


class AovChainOpts(C.Structure):  # rt_aov_chain_opts
    _fields_ = [
        ("max_chain", C.c_uint32),
        ("fuzz_limit", C.c_float),
        ("reserved", C.c_uint32 * 6),
    ]


class AovChainBuffers(C.Structure):  # rt_aov_chain_buffers
    _fields_ = [
        ("aov", AovBuffers),
        ("bounces", C.POINTER(C.c_float)),
    ]


AOV_CHAIN_SHAPES = {"aov": AOV_SHAPES, "bounces": "hw"}
AOV_CHAIN_CHANNELS = AOV_CHANNELS + ("bounces",)
AOV_CHAIN_MAX_CHAIN = 64


# anti-aliased ID mattes (rt_render_matte, rt_matte_extract)
RT_MATTE_SLOTS = 8  # (id, count) slots per pixel, and the most layers
RT_MATTE_ID_PRIMITIVE, RT_MATTE_ID_MATERIAL = range(2)  # rt_matte_id_kind
MATTE_ID_KINDS = {"primitive": RT_MATTE_ID_PRIMITIVE, "material": RT_MATTE_ID_MATERIAL}
MATTE_MAX_IDS = 1 << 20  # largest selection rt_matte_extract takes


class MatteOpts(C.Structure):  # rt_matte_opts
    _fields_ = [
        ("id_kind", C.c_int32),
        ("layers", C.c_uint32),
        ("reserved", C.c_uint32 * 6),
    ]


class MatteBuffers(C.Structure):  # rt_matte_buffers
    _fields_ = [
        ("ids", C.POINTER(C.c_uint32)),
        ("coverage", C.POINTER(C.c_float)),
        ("residual", C.POINTER(C.c_float)),
    ]


MATTE_SHAPES = {"ids": "lhw", "coverage": "lhw", "residual": "hw"}
MATTE_BUFFERS = tuple(MATTE_SHAPES)


# ambient occlusion (rt_render_ao)
AO_MAX_RAYS = 64  # most AO rays per pass


class AoOpts(C.Structure):  # rt_ao_opts
    _fields_ = [
        ("rays_per_pass", C.c_uint32),
        ("radius", C.c_float),
        ("reserved", C.c_uint32 * 6),
    ]


class AoBuffers(C.Structure):  # rt_ao_buffers
    _fields_ = [
        ("visibility", C.POINTER(C.c_float)),
        ("bent_normal", C.POINTER(C.c_float)),
    ]


AO_SHAPES = {"visibility": "hw", "bent_normal": "hw3"}
AO_CHANNELS = tuple(AO_SHAPES)


# radiance queries (rt_radiance)
class RadianceOpts(C.Structure):  # rt_radiance_opts
    _fields_ = [
        ("seed", C.c_uint64),
        ("sample_begin", C.c_uint64),
        ("samples_per_ray", C.c_uint32),
        ("render_method", C.c_int32),
        ("max_depth", C.c_uint32),
        ("rr_threshold", C.c_uint32),
        ("reserved", C.c_uint32 * 2),
    ]


RADIANCE_OPTIONS = tuple(n for n, _ in RadianceOpts._fields_ if n != "reserved")


# noise estimates (rt_render_noise, rt_noise_tiles, rt_render_converged)
NOISE_MAX_SPLIT = 64  # the largest sample_split an estimate is taken from
NOISE_TILE = 8  # tiles of the error map are NOISE_TILE x NOISE_TILE pixels
NOISE_TILES_PER_GRID_PASS = 8192  # tiles the tile kernel's grid covers before it strides (csrc/rt_noise.h kNoiseTileGridBlocks * 4)


class NoiseOpts(C.Structure):  # rt_noise_opts
    _fields_ = [
        ("luminance_floor", C.c_float),
        ("threshold", C.c_float),
        ("reserved", C.c_uint32 * 6),
    ]


class NoiseSummary(C.Structure):  # rt_noise_summary
    _fields_ = [
        ("max_tile_error", C.c_float),
        ("tiles_above", C.c_uint32),
        ("n_tiles", C.c_uint32),
        ("reserved", C.c_uint32),
    ]


class NoiseBuffers(C.Structure):  # rt_noise_buffers
    _fields_ = [
        ("mean", C.POINTER(C.c_float)),
        ("variance", C.POINTER(C.c_float)),
        ("lum_mean", C.POINTER(C.c_float)),
        ("tile_error", C.POINTER(C.c_float)),
        ("summary", C.POINTER(NoiseSummary)),
    ]


class NoiseResult(C.Structure):  # rt_noise_result
    _fields_ = [
        ("passes", C.c_uint64),
        ("rays_shot", C.c_uint64),
        ("batches", C.c_uint32),
        ("converged", C.c_uint32),
        ("summary", NoiseSummary),
    ]


class AdaptiveResult(C.Structure):  # rt_adaptive_result
    _fields_ = [
        ("pixel_passes", C.c_uint64),
        ("rays_shot", C.c_uint64),
        ("batches", C.c_uint32),
        ("converged", C.c_uint32),
        ("summary", NoiseSummary),
    ]


# lens cameras (rt_lens_camera_new, rt_render_lens)
RT_PROJ_PERSPECTIVE, RT_PROJ_ORTHOGRAPHIC, RT_PROJ_FISHEYE, RT_PROJ_EQUIRECT = range(4)  # rt_projection
PROJECTIONS = {"perspective": RT_PROJ_PERSPECTIVE, "orthographic": RT_PROJ_ORTHOGRAPHIC, "fisheye": RT_PROJ_FISHEYE,
               "equirect": RT_PROJ_EQUIRECT}


class LensCamera(C.Structure):  # rt_lens_camera
    _fields_ = [
        ("pinhole", Camera),
        ("right", f32x3),
        ("up", f32x3),
        ("forward", f32x3),
        ("lens_radius", C.c_float),
        ("fisheye_half_angle", C.c_float),
        ("projection", C.c_int32),
        ("reserved0", C.c_uint32),
    ]


# light probes (rt_probe_sh, rt_probe_sh_eval)
class ProbeOpts(C.Structure):  # rt_probe_opts
    _fields_ = [
        ("seed", C.c_uint64),
        ("sample_begin", C.c_uint64),
        ("samples_per_probe", C.c_uint32),
        ("sample_split", C.c_uint32),
        ("render_method", C.c_int32),
        ("max_depth", C.c_uint32),
        ("rr_threshold", C.c_uint32),
        ("convolve", C.c_uint32),
        ("reserved", C.c_uint32 * 2),
    ]


PROBE_OPTIONS = tuple(n for n, _ in ProbeOpts._fields_ if n != "reserved")
PROBE_TERMS = 27  # floats a probe: 9 basis functions x RGB


NOISE_SHAPES = {"mean": "hw3", "variance": "hw", "lum_mean": "hw", "tile_error": "tiles", "summary": "summary"}
NOISE_CHANNELS = tuple(NOISE_SHAPES)


# firefly-robust frames (rt_render_robust, rt_robust_combine, rt_render_denoised_robust)
RT_ROBUST_TRIM, RT_ROBUST_MEDIAN, RT_ROBUST_GINI = range(3)  # rt_robust_mode
ROBUST_MODES = {"trim": RT_ROBUST_TRIM, "median": RT_ROBUST_MEDIAN, "gini": RT_ROBUST_GINI}
ROBUST_MAX_SPLIT = 64  # the most chunks a pixel is ranked over


class RobustOpts(C.Structure):  # rt_robust_opts
    _fields_ = [
        ("mode", C.c_int32),
        ("trim", C.c_uint32),
        ("gini_gain", C.c_float),
        ("reserved", C.c_uint32 * 5),
    ]


class RobustBuffers(C.Structure):  # rt_robust_buffers
    _fields_ = [
        ("out", C.POINTER(C.c_float)),
        ("mean", C.POINTER(C.c_float)),
        ("gini", C.POINTER(C.c_float)),
        ("trimmed", C.POINTER(C.c_uint8)),
        ("dropped", C.POINTER(C.c_uint8)),
    ]


ROBUST_SHAPES = {"out": "hw3", "mean": "hw3", "gini": "hw", "trimmed": "hw", "dropped": "hw"}
ROBUST_CHANNELS = tuple(ROBUST_SHAPES)


class DenoiseOpts(C.Structure):  # rt_denoise_opts
    _fields_ = [
        ("width", C.c_uint32),
        ("height", C.c_uint32),
        ("iterations", C.c_uint32),
        ("sigma_luminance", C.c_float),
        ("sigma_normal", C.c_float),
        ("sigma_depth", C.c_float),
        ("reserved", C.c_uint32 * 6),
    ]


DENOISE_SHAPES = {"color": "hw3", "albedo": "hw3", "normal": "hw3", "depth": "hw", "variance": "hw"}
DENOISE_INPUTS = tuple(DENOISE_SHAPES)


class DenoiseInputs(C.Structure):  # rt_denoise_inputs
    _fields_ = [(name, C.POINTER(C.c_float)) for name in DENOISE_INPUTS]


DENOISE_WORKSPACE_BYTES_PER_PIXEL = 48  # three float4 planes


class TemporalOpts(C.Structure):  # rt_temporal_opts
    _fields_ = [
        ("denoise", DenoiseOpts),
        ("alpha_color", C.c_float),
        ("alpha_moments", C.c_float),
        ("depth_tolerance", C.c_float),
        ("normal_tolerance", C.c_float),
        ("max_history", C.c_uint32),
        ("reserved", C.c_uint32 * 7),
    ]


TEMPORAL_SHAPES = {"color": "hw3", "albedo": "hw3", "normal": "hw3", "depth": "hw"}
TEMPORAL_INPUTS = tuple(TEMPORAL_SHAPES)


class TemporalInputs(C.Structure):  # rt_temporal_inputs
    _fields_ = [(name, C.POINTER(C.c_float)) for name in TEMPORAL_INPUTS]


TEMPORAL_OPTIONS = ("alpha_color", "alpha_moments", "depth_tolerance", "normal_tolerance", "max_history")
TEMPORAL_HISTORY_BYTES_PER_PIXEL = 48  # H0 = (e_1, n), H1 = (n^, z), H2 = (m1, m2, 0, 0): three float4 planes
TEMPORAL_WORKSPACE_BYTES_PER_PIXEL = 32  # the denoiser's two (e, Var) planes
AOV_NO_ID = 0xFFFFFFFF  # primitive / material of a pass that missed

# display stage (rt_display): rt_exposure_mode, rt_tonemap, rt_transfer, rt_quantiser, rt_pixel_format
RT_EXPOSURE_FIXED, RT_EXPOSURE_AUTO = range(2)
RT_TONEMAP_CLAMP, RT_TONEMAP_REINHARD, RT_TONEMAP_ACES, RT_TONEMAP_HABLE = range(4)
RT_TRANSFER_SRGB, RT_TRANSFER_GAMMA, RT_TRANSFER_LINEAR = range(3)
RT_QUANT_ROUND, RT_QUANT_DITHER, RT_QUANT_REFERENCE = range(3)
RT_PIXEL_RGBA8, RT_PIXEL_BGRA8, RT_PIXEL_RGB8 = range(3)
DISPLAY_ENUMS = {  # option -> {name: value}
    "exposure_mode": {"fixed": RT_EXPOSURE_FIXED, "auto": RT_EXPOSURE_AUTO},
    "tonemap": {"clamp": RT_TONEMAP_CLAMP, "reinhard": RT_TONEMAP_REINHARD, "aces": RT_TONEMAP_ACES, "hable": RT_TONEMAP_HABLE},
    "transfer": {"srgb": RT_TRANSFER_SRGB, "gamma": RT_TRANSFER_GAMMA, "linear": RT_TRANSFER_LINEAR},
    "quantiser": {"round": RT_QUANT_ROUND, "dither": RT_QUANT_DITHER, "reference": RT_QUANT_REFERENCE},
    "pixel_format": {"rgba8": RT_PIXEL_RGBA8, "bgra8": RT_PIXEL_BGRA8, "rgb8": RT_PIXEL_RGB8},
}
DISPLAY_HISTOGRAM_BINS = 256


class DisplayOpts(C.Structure):  # rt_display_opts
    _fields_ = [
        ("width", C.c_uint32),
        ("height", C.c_uint32),
        ("exposure_mode", C.c_int32),
        ("tonemap", C.c_int32),
        ("transfer", C.c_int32),
        ("quantiser", C.c_int32),
        ("pixel_format", C.c_int32),
        ("exposure_ev", C.c_float),
        ("key_ev", C.c_float),
        ("meter_low", C.c_float),
        ("meter_high", C.c_float),
        ("ev_min", C.c_float),
        ("ev_max", C.c_float),
        ("adaptation", C.c_float),
        ("white", C.c_float),
        ("gamma", C.c_float),
        ("seed", C.c_uint64),
        ("reserved", C.c_uint32 * 8),
    ]


class DisplayState(C.Structure):  # rt_display_state
    _fields_ = [
        ("ev", C.c_float),
        ("frames", C.c_uint32),
        ("metered", C.c_float),
        ("reserved", C.c_uint32),
    ]


class BloomOpts(C.Structure):  # rt_bloom_opts
    _fields_ = [
        ("width", C.c_uint32),
        ("height", C.c_uint32),
        ("threshold", C.c_float),
        ("knee", C.c_float),
        ("intensity", C.c_float),
        ("scatter", C.c_float),
        ("levels", C.c_uint32),
        ("exposure_ev", C.c_float),
        ("clamp_max", C.c_float),
        ("fuse_tail", C.c_uint32),
        ("reserved", C.c_uint32 * 6),
    ]


BLOOM_OPTIONS = tuple(n for n, _ in BloomOpts._fields_ if n not in ("width", "height", "reserved"))
BLOOM_MAX_LEVELS = 12


class DofOpts(C.Structure):  # rt_dof_opts
    _fields_ = [
        ("width", C.c_uint32),
        ("height", C.c_uint32),
        ("focus_distance", C.c_float),
        ("blur_scale", C.c_float),
        ("max_radius", C.c_uint32),
        ("planar_depth", C.c_uint32),
        ("reserved", C.c_uint32 * 10),
    ]


DOF_OPTIONS = tuple(n for n, _ in DofOpts._fields_ if n not in ("width", "height", "reserved"))
DOF_MAX_RADIUS = 16


class UpscaleOpts(C.Structure):  # rt_upscale_opts
    _fields_ = [
        ("src_width", C.c_uint32),
        ("src_height", C.c_uint32),
        ("dst_width", C.c_uint32),
        ("dst_height", C.c_uint32),
        ("sigma_normal", C.c_float),
        ("depth_tolerance", C.c_float),
        ("reserved", C.c_uint32 * 8),
    ]


UPSCALE_SHAPES = {"color": "hw3", "src_albedo": "hw3", "src_normal": "hw3", "src_depth": "hw",  # color and src_* at the source size,
                  "dst_albedo": "hw3", "dst_normal": "hw3", "dst_depth": "hw"}  # dst_* at the destination size
UPSCALE_INPUTS = tuple(UPSCALE_SHAPES)
UPSCALE_GUIDES = ("albedo", "normal", "depth")
UPSCALE_OPTIONS = ("sigma_normal", "depth_tolerance")


class UpscaleInputs(C.Structure):  # rt_upscale_inputs
    _fields_ = [(name, C.POINTER(C.c_float)) for name in UPSCALE_INPUTS]


# rt_selftest_short_forms (csrc/rt_lean.h: the forms that rest on what gfx950's v_rcp_f32 / v_sqrt_f32 return)
SHORT_FORM_NAMES = ("rcp_refined", "inv_one_pair", "inv_two_pairs", "sqrt_raw", "sqrt_both")
SHORT_SITE_NAMES = ("ray_new_pair", "ray_new_full")


class ShortFormCount(C.Structure):  # rt_short_form_count
    _fields_ = [("tested", C.c_uint64), ("mismatches", C.c_uint64), ("first_mismatch", C.c_uint32), ("reserved", C.c_uint32)]


class ShortFormsResult(C.Structure):  # rt_short_forms_result
    _fields_ = [("form", ShortFormCount * len(SHORT_FORM_NAMES)),
                ("sqrt_raw_exact", C.c_uint64), ("sqrt_raw_high", C.c_uint64), ("sqrt_raw_low", C.c_uint64), ("sqrt_raw_other", C.c_uint64),
                ("site_tested", C.c_uint64), ("site_mismatches", C.c_uint64 * len(SHORT_SITE_NAMES)),
                ("in_use", C.c_uint32), ("reserved", C.c_uint32)]


# rt_selftest_div_forms (csrc/rt_lean.h lean_div_core_gfx950: the quotient with one correction pair, and the sites that guard it)
DIV_FORM_NAMES = ("one_pair", "two_pairs")
DIV_SITE_NAMES = ("fix", "div3_fix", "mis_light_term", "atan2")


class DivFormsSlice(C.Structure):  # rt_div_forms_slice
    _fields_ = [("denominators", C.POINTER(C.c_uint32)), ("n_denominators", C.c_uint64), ("first_denominator", C.c_uint32),
                ("reserved", C.c_uint32), ("exponents", C.POINTER(C.c_int32)), ("n_exponent_pairs", C.c_uint64)]


class DivFormsResult(C.Structure):  # rt_div_forms_result
    _fields_ = [("tested", C.c_uint64), ("mismatches", C.c_uint64 * len(DIV_FORM_NAMES)),
                ("first_numerator", C.c_uint32 * len(DIV_FORM_NAMES)), ("first_denominator", C.c_uint32 * len(DIV_FORM_NAMES)),
                ("site_tested", C.c_uint64), ("site_in_domain", C.c_uint64), ("site_mismatches", C.c_uint64 * len(DIV_SITE_NAMES)),
                ("in_use", C.c_uint32), ("reserved", C.c_uint32)]


# rt_selftest_pair_shadow (csrc/rt_intersect.h sphere_occludes_unlimited): floats per case, names of the counts
PAIR_SHADOW_CASE_FLOATS = 10
PAIR_SHADOW_COUNT_NAMES = ("tested", "mismatches", "asked_mismatches", "asked")
PAIR_SHADOW_WALK_CASE_FLOATS = 16
PAIR_SHADOW_WALK_COUNT_NAMES = ("tested", "mismatches", "asked", "asked_both", "asked_with_occluded")
# rt_selftest_frame_forms (csrc/rt_shade.h coord_from_z_pair, csrc/rt_intersect.h ray_new): names of the counts, and of the bits of "in_use"
FRAME_FORMS_COUNT_NAMES = ("tested", "frame_mismatches", "frame_short", "frame_plain", "ray_mismatches", "ray_short", "ray_plain", "in_use")
FRAME_FORM_NAMES = ("frame_guarded_short", "ray_norm_one_pair")
# rt_selftest_gen_keys (csrc/rt_gen_keys.h): words per case, names of the counts, and of the bits of "in_use"
GEN_KEYS_CASE_WORDS = 4
GEN_KEYS_COUNT_NAMES = ("tested", "state_mismatches", "draw_mismatches", "item_state_mismatches", "item_draw_mismatches", "zero_blocks", "in_use")
GEN_KEYS_FORM_NAMES = ("key_table", "item_product")
# the self-tests that take (n, width) cases and answer named counts: name -> (symbol, element type, width, what the binding calls the
# cases, names of the counts, names of the bits of "in_use" where the counts have one)
SELFTEST_CASE_TABLES = {
    "pair_shadow": ("rt_selftest_pair_shadow", C.c_float, PAIR_SHADOW_CASE_FLOATS, "cases", PAIR_SHADOW_COUNT_NAMES, None),
    "pair_shadow_walk": ("rt_selftest_pair_shadow_walk", C.c_float, PAIR_SHADOW_WALK_CASE_FLOATS, "cases", PAIR_SHADOW_WALK_COUNT_NAMES, None),
    "frame_forms": ("rt_selftest_frame_forms", C.c_float, 3, "vectors", FRAME_FORMS_COUNT_NAMES, FRAME_FORM_NAMES),
    "gen_keys": ("rt_selftest_gen_keys", C.c_uint32, GEN_KEYS_CASE_WORDS, "cases", GEN_KEYS_COUNT_NAMES, GEN_KEYS_FORM_NAMES),
}

DISPLAY_OPTIONS = tuple(n for n, _ in DisplayOpts._fields_ if n not in ("width", "height", "reserved"))

# rt_presentation_update: int (*)(void *data, const rt_sampler_progress *, uint64_t samples_done)
PresentationUpdate = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(SamplerProgressC), C.c_uint64)

EXPECTED_SIZES = {
    "rt_texture_desc": (TextureDesc, 64),
    "rt_material_desc": (MaterialDesc, 28),
    "rt_primitive_desc": (PrimitiveDesc, 40),
    "rt_triangle_data": (TriangleData, 72),
    "rt_mesh_desc": (MeshDesc, 32),
    "rt_sky_desc": (SkyDesc, 16),
    "rt_scene_desc": (SceneDesc, 96),
    "rt_camera": (Camera, 48),
    "rt_render_opts": (RenderOpts, 80),
    "rt_hit_record": (HitRecord, 72),
    "rt_ray_desc": (RayDesc, 24),
    "rt_bvh_node": (BvhNode, 56),
    "rt_sampler_progress": (SamplerProgressC, 32),
    "rt_launch_info": (LaunchInfo, 224),
    "rt_sky_info": (SkyInfo, 32),
    "rt_aov_buffers": (AovBuffers, 48),
    "rt_aov_chain_opts": (AovChainOpts, 32),
    "rt_aov_chain_buffers": (AovChainBuffers, 56),
    "rt_matte_opts": (MatteOpts, 32),
    "rt_matte_buffers": (MatteBuffers, 24),
    "rt_ao_opts": (AoOpts, 32),
    "rt_ao_buffers": (AoBuffers, 16),
    "rt_radiance_opts": (RadianceOpts, 40),
    "rt_noise_opts": (NoiseOpts, 32),
    "rt_noise_summary": (NoiseSummary, 16),
    "rt_noise_buffers": (NoiseBuffers, 40),
    "rt_noise_result": (NoiseResult, 40),
    "rt_adaptive_result": (AdaptiveResult, 40),
    "rt_lens_camera": (LensCamera, 100),
    "rt_probe_opts": (ProbeOpts, 48),
    "rt_robust_opts": (RobustOpts, 32),
    "rt_robust_buffers": (RobustBuffers, 40),
    "rt_denoise_opts": (DenoiseOpts, 48),
    "rt_denoise_inputs": (DenoiseInputs, 40),
    "rt_temporal_opts": (TemporalOpts, 96),
    "rt_temporal_inputs": (TemporalInputs, 32),
    "rt_display_opts": (DisplayOpts, 104),
    "rt_display_state": (DisplayState, 16),
    "rt_bloom_opts": (BloomOpts, 64),
    "rt_dof_opts": (DofOpts, 64),
    "rt_upscale_opts": (UpscaleOpts, 56),
    "rt_upscale_inputs": (UpscaleInputs, 56),
    "rt_short_form_count": (ShortFormCount, 24),
    "rt_short_forms_result": (ShortFormsResult, 184),
    "rt_div_forms_slice": (DivFormsSlice, 40),
    "rt_div_forms_result": (DivFormsResult, 96),
}

# every symbol include/rt_hip.h declares
EXPORTED_SYMBOLS = [
    "rt_last_error",
    "rt_abi_version",
    "rt_device_count",
    "rt_render_opts_default",
    "rt_camera_new",
    "rt_scene_create",
    "rt_scene_create_multi",
    "rt_scene_device_count",
    "rt_scene_destroy",
    "rt_scene_counts",
    "rt_scene_get_nodes",
    "rt_scene_get_primitive_order",
    "rt_scene_get_lights",
    "rt_scene_wide_info",
    "rt_scene_get_wide_nodes",
    "rt_scene_get_leaf_boxes",
    "rt_scene_get_wide_nodes_compact",
    "rt_scene_auto_sample_split",
    "rt_scene_gather_info",
    "rt_rccl_probe",
    "rt_selftest_division",
    "rt_scene_get_leaf_boxes_compact",
    "rt_scene_sky_info",
    "rt_scene_get_sky_tables",
    "rt_scene_set_traversal",
    "rt_scene_set_tuning",
    "rt_render",
    "rt_sample_image",
    "rt_render_device",
    "rt_render_output_floats",
    "rt_shard_pixel_order",
    "rt_plan_work_items",
    "rt_last_kernel_ms",
    "rt_last_launch_info",
    "rt_output_rgb8",
    "rt_output_save",
    "rt_output_rgb8_device",
    "rt_render_rgb8",
    "rt_check_hit",
    "rt_check_hit_index",
    "rt_radiance_opts_default",
    "rt_radiance",
    "rt_radiance_device",
    "rt_selftest_lean",
    "rt_selftest_short_forms",
    "rt_selftest_div_forms",
    "rt_selftest_sky_pdf_forms",
    "rt_selftest_sky_cell",
    "rt_selftest_frame_forms",
    "rt_selftest_gen_keys",
    "rt_philox_round_keys",
    "rt_selftest_pair_shadow",
    "rt_selftest_pair_shadow_walk",
    "rt_selftest_pair_primary",
    "rt_selftest_sky_tiles",
    "rt_selftest_sky",
    "rt_render_aov",
    "rt_render_aov_device",
    "rt_aov_chain_opts_default",
    "rt_render_aov_chain",
    "rt_render_aov_chain_device",
    "rt_matte_opts_default",
    "rt_render_matte",
    "rt_render_matte_device",
    "rt_matte_extract",
    "rt_matte_extract_device",
    "rt_ao_opts_default",
    "rt_render_ao",
    "rt_render_ao_device",
    "rt_denoise_opts_default",
    "rt_denoise_workspace_bytes",
    "rt_denoise",
    "rt_denoise_device",
    "rt_render_denoised",
    "rt_noise_opts_default",
    "rt_render_noise",
    "rt_render_noise_device",
    "rt_noise_tiles",
    "rt_noise_tiles_device",
    "rt_render_converged",
    "rt_render_denoised_split",
    "rt_render_adaptive",
    "rt_render_tiles",
    "rt_render_tiles_device",
    "rt_noise_select_tiles",
    "rt_noise_select_tiles_device",
    "rt_lens_camera_new",
    "rt_render_lens",
    "rt_render_lens_device",
    "rt_render_lens_aov",
    "rt_render_lens_aov_device",
    "rt_render_lens_denoised",
    "rt_probe_opts_default",
    "rt_probe_workspace_bytes",
    "rt_probe_sh",
    "rt_probe_sh_device",
    "rt_probe_sh_eval",
    "rt_probe_sh_eval_device",
    "rt_robust_opts_default",
    "rt_render_robust",
    "rt_render_robust_device",
    "rt_robust_combine",
    "rt_robust_combine_device",
    "rt_render_denoised_robust",
    "rt_temporal_opts_default",
    "rt_temporal_history_bytes",
    "rt_temporal_workspace_bytes",
    "rt_denoise_temporal_device",
    "rt_denoise_temporal",
    "rt_denoise_temporal_reset",
    "rt_display_opts_default",
    "rt_display_workspace_bytes",
    "rt_display_output_bytes",
    "rt_display_device",
    "rt_display",
    "rt_display_reset",
    "rt_bloom_opts_default",
    "rt_bloom_workspace_bytes",
    "rt_bloom_device",
    "rt_bloom",
    "rt_dof_opts_default",
    "rt_dof_opts_from_camera",
    "rt_dof_workspace_bytes",
    "rt_dof_device",
    "rt_dof",
    "rt_render_dof",
    "rt_upscale_opts_default",
    "rt_upscale_device",
    "rt_upscale",
    "rt_render_upscaled",
]


def channels(table, struct):
    """{channel: (the struct that holds its pointer, the element ctype, the shape name)} of a channel table and an instance of
    its struct, a nested table flattened in place"""
    out = {}
    for name, shape in table.items():
        if isinstance(shape, dict):
            out.update(channels(shape, getattr(struct, name)))
        else:
            out[name] = (struct, dict(struct._fields_)[name]._type_, shape)
    return out


def default_aov_chain_opts(max_chain=8, fuzz_limit=0.0):
    """rt_aov_chain_opts_default (include/rt_hip.h)."""
    o = AovChainOpts()
    o.max_chain, o.fuzz_limit = max_chain, fuzz_limit
    return o


def default_matte_opts(id_kind=RT_MATTE_ID_MATERIAL, layers=4):
    """rt_matte_opts_default (include/rt_hip.h)."""
    o = MatteOpts()
    o.id_kind, o.layers = id_kind, layers
    return o


def default_ao_opts(rays_per_pass=4, radius=0.0):
    """rt_ao_opts_default (include/rt_hip.h)."""
    o = AoOpts()
    o.rays_per_pass, o.radius = rays_per_pass, radius
    return o


def default_probe_opts(samples_per_probe=1024, sample_split=64, method=RT_METHOD_MIS, convolve=0, seed=0, sample_begin=0):
    """rt_probe_opts_default (include/rt_hip.h)."""
    o = ProbeOpts()
    o.seed, o.sample_begin = seed, sample_begin
    o.samples_per_probe, o.sample_split = samples_per_probe, sample_split
    o.render_method, o.max_depth, o.rr_threshold, o.convolve = method, 50, 3, convolve
    return o


def default_noise_opts(luminance_floor=0.01, threshold=0.05):
    """rt_noise_opts_default (include/rt_hip.h)."""
    o = NoiseOpts()
    o.luminance_floor, o.threshold = luminance_floor, threshold
    return o


def default_robust_opts(mode=RT_ROBUST_GINI, trim=1, gini_gain=1.0):
    """rt_robust_opts_default (include/rt_hip.h)."""
    o = RobustOpts()
    o.mode, o.trim, o.gini_gain = mode, trim, gini_gain
    return o


def default_denoise_opts(width=0, height=0, iterations=5, sigma_luminance=4.0, sigma_normal=128.0, sigma_depth=0.1):
    """rt_denoise_opts_default (include/rt_hip.h) with the frame size filled in."""
    o = DenoiseOpts()
    o.width, o.height, o.iterations = width, height, iterations
    o.sigma_luminance, o.sigma_normal, o.sigma_depth = sigma_luminance, sigma_normal, sigma_depth
    return o


def default_render_opts(width=1920, height=1080, spp=128, method=RT_METHOD_MIS, seed=1):
    """RenderOptions::default() (samplers/mod.rs:31-41) + MAX_DEPTH/RR consts (integrators/mod.rs:7-8)."""
    o = RenderOpts()
    o.width, o.height = width, height
    o.samples_per_pixel = spp
    o.sample_begin = 0
    o.seed = seed
    o.render_method = method
    o.max_depth = 50
    o.rr_threshold = 3
    o.shard_index, o.shard_count = 0, 1
    o.tile_width = o.tile_height = 0
    o.output_layout = RT_LAYOUT_FRAME
    o.sample_split = 1
    o.reserved0 = 0
    return o
