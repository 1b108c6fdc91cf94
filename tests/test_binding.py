"""The Python binding (hip_backend.py, abi.py) without a GPU: the channel tables against the structs they describe, every options
builder and byte query against the library's own defaults and answers, and every blocking HipScene wrapper from render_aov to
render_upscaled (and radiance) on a host-only scene, where a mis-sized or mis-typed buffer would show as RT_ERR_INVALID_ARGUMENT
ahead of RT_ERR_NO_DEVICE."""
import ctypes as C

import numpy as np
import pytest

import scenes

abi = scenes.abi
F32 = np.float32
W, H = 16, 9  # two 8 x 8 tiles wide, a partial bottom row of tiles

# ---- the tables against the structs ----
TABLES = [  # (table, struct, public tuple)
    ("AOV_SHAPES", abi.AovBuffers, "AOV_CHANNELS"),
    ("AOV_CHAIN_SHAPES", abi.AovChainBuffers, "AOV_CHAIN_CHANNELS"),
    ("MATTE_SHAPES", abi.MatteBuffers, "MATTE_BUFFERS"),
    ("AO_SHAPES", abi.AoBuffers, "AO_CHANNELS"),
    ("NOISE_SHAPES", abi.NoiseBuffers, "NOISE_CHANNELS"),
    ("ROBUST_SHAPES", abi.RobustBuffers, "ROBUST_CHANNELS"),
    ("DENOISE_SHAPES", abi.DenoiseInputs, "DENOISE_INPUTS"),
    ("TEMPORAL_SHAPES", abi.TemporalInputs, "TEMPORAL_INPUTS"),
    ("UPSCALE_SHAPES", abi.UpscaleInputs, "UPSCALE_INPUTS"),
]


def _pointer_fields(struct):
    """{field: pointee ctype} of a struct's pointer fields, nested structs flattened"""
    out = {}
    for name, t in struct._fields_:
        if issubclass(t, C.Structure):
            out.update(_pointer_fields(t))
        else:
            assert issubclass(t, C._Pointer), (struct, name)
            out[name] = t._type_
    return out


@pytest.mark.parametrize("table, struct, public", TABLES, ids=[t[0] for t in TABLES])
def test_table_names_and_element_types_are_the_structs(table, struct, public):
    fields = _pointer_fields(struct)
    channels = abi.channels(getattr(abi, table), struct())
    assert tuple(channels) == tuple(fields) == getattr(abi, public)
    for name, (holder, ctype, shape) in channels.items():
        assert ctype is fields[name] and hasattr(holder, name)
        assert shape in ("hw", "hw3", "lhw", "tiles", "summary"), name
        assert np.dtype(ctype).itemsize == C.sizeof(fields[name]), name
        if name in ("primitive", "material", "ids"):
            assert np.dtype(ctype) == np.uint32
        elif name in ("trimmed", "dropped"):
            assert np.dtype(ctype) == np.uint8
        elif name == "summary":
            assert ctype is abi.NoiseSummary and shape == "summary"
        else:
            assert np.dtype(ctype) == np.float32


def test_the_chain_table_nests_the_aov_table_beside_bounces():
    assert abi.AOV_CHAIN_SHAPES["aov"] is abi.AOV_SHAPES and set(abi.AOV_CHAIN_SHAPES) == {"aov", "bounces"}
    bufs = abi.AovChainBuffers()
    channels = abi.channels(abi.AOV_CHAIN_SHAPES, bufs)
    assert channels["bounces"][0] is bufs and all(isinstance(channels[n][0], abi.AovBuffers) for n in abi.AOV_CHANNELS)
    assert abi.UPSCALE_GUIDES == ("albedo", "normal", "depth")


# ---- the options builders ----
DENOISE_KEYS = ("iterations", "sigma_luminance", "sigma_normal", "sigma_depth")
SIZE2 = {"width": W, "height": H}
BUILDERS = {  # builder -> (struct, the library's stem, frame-size arguments as {field: value}, allowed keys of the struct itself)
    "denoise_opts": (abi.DenoiseOpts, "denoise", SIZE2, DENOISE_KEYS),
    "matte_opts": (abi.MatteOpts, "matte", {}, ("id_kind", "layers")),
    "ao_opts": (abi.AoOpts, "ao", {}, ("rays_per_pass", "radius")),
    "radiance_opts": (abi.RadianceOpts, "radiance", {}, abi.RADIANCE_OPTIONS),
    "noise_opts": (abi.NoiseOpts, "noise", {}, ("luminance_floor", "threshold")),
    "robust_opts": (abi.RobustOpts, "robust", {}, ("mode", "trim", "gini_gain")),
    "temporal_opts": (abi.TemporalOpts, "temporal", SIZE2, abi.TEMPORAL_OPTIONS),
    "display_opts": (abi.DisplayOpts, "display", SIZE2, abi.DISPLAY_OPTIONS),
    "bloom_opts": (abi.BloomOpts, "bloom", SIZE2, abi.BLOOM_OPTIONS),
    "dof_opts": (abi.DofOpts, "dof", SIZE2, abi.DOF_OPTIONS),
    "upscale_opts": (abi.UpscaleOpts, "upscale", {"src_width": W, "src_height": H, "dst_width": 2 * W, "dst_height": 2 * H},
                     ("sigma_normal", "depth_tolerance")),
}


def _library_default(hb, name):
    struct, stem, size, _ = BUILDERS[name]
    o = struct()
    C.memset(C.byref(o), 0xFF, C.sizeof(o))
    assert getattr(hb.lib(), f"rt_{stem}_opts_default")(C.byref(o)) == abi.RT_OK
    for field, v in size.items():
        setattr(o.denoise if name == "temporal_opts" else o, field, v)
    return o


def _other_value(struct, field):
    """a value of the field's type that no default holds"""
    return 0.375 if dict(struct._fields_)[field] is C.c_float else 7


def _check_keys(build, default, holder_of, keys):
    """each key, set alone, changes the bytes of `default()` by that one field of holder_of(struct)"""
    for k in keys:
        want = default()
        holder = holder_of(want)
        v = _other_value(type(holder), k)
        assert getattr(holder, k) != v, k
        setattr(holder, k, v)
        assert bytes(build(**{k: v})) == bytes(want), k


@pytest.mark.parametrize("name", BUILDERS)
def test_options_builder(hb, name):
    struct, _, size, keys = BUILDERS[name]
    build = lambda **kw: getattr(hb, name)(*size.values(), **kw)  # noqa: E731
    default = lambda: _library_default(hb, name)  # noqa: E731
    o = build()
    assert type(o) is struct and bytes(o) == bytes(default())
    _check_keys(build, default, lambda o: o, keys)
    if name == "temporal_opts":
        _check_keys(build, default, lambda o: o.denoise, DENOISE_KEYS)
    with pytest.raises(ValueError, match="no_such_option"):
        build(no_such_option=1)
    with pytest.raises(ValueError):
        build(reserved=0)


def test_dof_opts_from_camera_shares_the_keywords(hb):
    cam = hb.camera_new((0, 0, 0), (0, 0, -1), (0, 1, 0), 0.6, W / H, 0.1, 3.0)

    def default():
        o = abi.DofOpts()
        assert hb.lib().rt_dof_opts_from_camera(C.byref(o), C.byref(cam), C.c_float(0.1), C.c_float(3.0), C.c_uint32(W), C.c_uint32(H)) == abi.RT_OK
        return o

    build = lambda **kw: hb.dof_opts_from_camera(cam, 0.1, 3.0, W, H, **kw)  # noqa: E731
    assert bytes(build()) == bytes(default()) != bytes(hb.dof_opts(W, H))
    _check_keys(build, default, lambda o: o, abi.DOF_OPTIONS)
    with pytest.raises(ValueError, match="no_such_option"):
        build(no_such_option=1)


ENUMS = [("matte_opts", (), "id_kind", abi.MATTE_ID_KINDS), ("robust_opts", (), "mode", abi.ROBUST_MODES)] + \
    [("display_opts", (W, H), k, names) for k, names in abi.DISPLAY_ENUMS.items()]


@pytest.mark.parametrize("builder, size, key, names", ENUMS, ids=[e[2] for e in ENUMS])
def test_enum_options_take_their_names_in_either_case(hb, builder, size, key, names):
    build = getattr(hb, builder)
    for name, value in names.items():
        for spelt in (name, name.upper()):
            assert getattr(build(*size, **{key: spelt}), key) == value
        assert getattr(build(*size, **{key: value}), key) == value
    with pytest.raises(ValueError, match="no_such_name") as e:
        build(*size, **{key: "no_such_name"})
    assert all(name in str(e.value) for name in names)  # the message lists the allowed set


def test_byte_queries_return_what_the_library_returns(hb):
    d, t, p = hb.denoise_opts(W, H), hb.temporal_opts(W, H), hb.display_opts(W, H)
    queries = {"denoise_workspace_bytes": d, "temporal_history_bytes": t, "temporal_workspace_bytes": t, "display_workspace_bytes": p,
               "display_output_bytes": p, "bloom_workspace_bytes": hb.bloom_opts(W, H), "dof_workspace_bytes": hb.dof_opts(W, H)}
    for name, o in queries.items():
        n = C.c_uint64()
        assert getattr(hb.lib(), "rt_" + name)(C.byref(o), C.byref(n)) == abi.RT_OK
        assert getattr(hb, name)(o) == n.value > 0, name
    assert hb.display_output_bytes(hb.display_opts(W, H, pixel_format="rgb8")) == W * H * 3
    bad = hb.denoise_opts(0, H)
    with pytest.raises(hb.RtHipError) as e:
        hb.denoise_workspace_bytes(bad)
    assert e.value.code == abi.RT_ERR_INVALID_ARGUMENT


# ---- every blocking wrapper on a host-only scene ----
def _wrapper_calls(hb, s, cam):
    """{name: call}: each wrapper once with its required arguments only ("name") and once with every optional channel, input
    and flag on ("name+")"""
    rng = np.random.default_rng(5)
    img, rgb, nrm = (rng.random((H, W, 3), dtype=F32) for _ in range(3))
    z, var, lum = (rng.random((H, W), dtype=F32) + F32(0.5) for _ in range(3))
    guides = {"albedo": rgb, "normal": nrm, "depth": z}
    W2, H2 = 2 * W, 2 * H
    big = {"albedo": rng.random((H2, W2, 3), dtype=F32), "normal": rng.random((H2, W2, 3), dtype=F32), "depth": rng.random((H2, W2), dtype=F32)}
    ids, cov = np.zeros((4, H, W), np.uint32), np.full((4, H, W), 0.25, F32)
    sums = rng.random((2, H, W, 3), dtype=F32)
    tile_error = rng.random((2, 2), dtype=F32)
    origins, directions = np.zeros((5, 3), F32), np.tile(np.array([0, 0, -1], F32), (5, 1))

    def opts():
        o = abi.default_render_opts(W, H, 4)
        o.sample_split = 2
        return o

    def frame():
        return np.zeros((H, W, 3), F32)

    dn = dict(iterations=2, sigma_luminance=3.0, sigma_normal=64.0, sigma_depth=0.2)
    return {
        "render_aov": lambda: s.render_aov(cam, opts()),
        "render_aov+": lambda: s.render_aov(cam, opts(), channels=abi.AOV_CHANNELS),
        "render_aov_chain": lambda: s.render_aov_chain(cam, opts()),
        "render_aov_chain+": lambda: s.render_aov_chain(cam, opts(), channels=abi.AOV_CHAIN_CHANNELS, max_chain=3, fuzz_limit=0.25),
        "render_matte": lambda: s.render_matte(cam, opts()),
        "render_matte+": lambda: s.render_matte(cam, opts(), id_kind="primitive", layers=8, residual=True),
        "matte_extract": lambda: s.matte_extract(ids, cov, []),
        "matte_extract+": lambda: s.matte_extract({"ids": ids, "coverage": cov}, None, [3, 1, 3]),
        "render_ao": lambda: s.render_ao(cam, opts()),
        "render_ao+": lambda: s.render_ao(cam, opts(), rays_per_pass=2, radius=1.5, channels=abi.AO_CHANNELS),
        "denoise": lambda: s.denoise(img),
        "denoise+": lambda: s.denoise(img, albedo=rgb, normal=nrm, depth=z, variance=var, **dn),
        "denoise+dict": lambda: s.denoise({"color": img, "variance": var, **guides}, **dn),
        "render_denoised": lambda: s.render_denoised(cam, opts()),
        "render_denoised+": lambda: s.render_denoised(cam, opts(), dopts=hb.denoise_opts(W, H, **dn)),
        "render_noise": lambda: s.render_noise(cam, opts()),
        "render_noise+": lambda: s.render_noise(cam, opts(), albedo=rgb, channels=abi.NOISE_CHANNELS, luminance_floor=0.02, threshold=0.1),
        "noise_tiles": lambda: s.noise_tiles(lum, var),
        "noise_tiles+": lambda: s.noise_tiles(lum, var, luminance_floor=0.02, threshold=0.1),
        "render_converged": lambda: s.render_converged(cam, opts(), 4),
        "render_converged+": lambda: s.render_converged(cam, opts(), 4, min_batches=2, max_passes=12, luminance_floor=0.02, threshold=0.1),
        "render_denoised_split": lambda: s.render_denoised_split(cam, opts()),
        "render_denoised_split+": lambda: s.render_denoised_split(cam, opts(), dopts=hb.denoise_opts(W, H, **dn)),
        "render_tiles": lambda: s.render_tiles(cam, opts(), [0, 3], frame()),
        "render_tiles+": lambda: s.render_tiles(cam, opts(), [0, 3], frame(), chunk_sums=True),
        "render_tiles+none": lambda: s.render_tiles(cam, opts(), [], frame(), chunk_sums=True),
        "render_adaptive": lambda: s.render_adaptive(cam, opts(), 4),
        "render_adaptive+": lambda: s.render_adaptive(cam, opts(), 4, min_batches=2, max_passes=12, albedo=rgb, luminance_floor=0.02, threshold=0.1),
        "noise_select_tiles": lambda: s.noise_select_tiles(tile_error, 0.5),
        "render_robust": lambda: s.render_robust(cam, opts()),
        "render_robust+": lambda: s.render_robust(cam, opts(), albedo=rgb, channels=abi.ROBUST_CHANNELS, mode="trim", trim=1, gini_gain=2.0),
        "robust_combine": lambda: s.robust_combine(sums, 2),
        "robust_combine+": lambda: s.robust_combine(sums, 2, albedo=rgb, channels=abi.ROBUST_CHANNELS, mode="median", trim=1, gini_gain=2.0),
        "render_denoised_robust": lambda: s.render_denoised_robust(cam, opts()),
        "render_denoised_robust+": lambda: s.render_denoised_robust(cam, opts(), dopts=hb.denoise_opts(W, H, **dn), mode="gini", trim=1, gini_gain=2.0),
        "denoise_temporal": lambda: s.denoise_temporal(img, cam, depth=z),
        "denoise_temporal+": lambda: s.denoise_temporal(img, cam, albedo=rgb, normal=nrm, depth=z, motion=True, alpha_color=0.3, alpha_moments=0.3,
                                                        depth_tolerance=0.2, normal_tolerance=0.8, max_history=8, **dn),
        "denoise_temporal+dict": lambda: s.denoise_temporal({"color": img, **guides}, cam, motion=True, **dn),
        "temporal_reset": lambda: s.temporal_reset(),
        "display": lambda: s.display(img),
        "display+": lambda: s.display(img, histogram=True, exposure_mode="auto", tonemap="hable", transfer="gamma", quantiser="dither",
                                      pixel_format="rgb8", exposure_ev=0.5, gamma=2.0, seed=7),
        "display_reset": lambda: s.display_reset(),
        "bloom": lambda: s.bloom(img),
        "bloom+": lambda: s.bloom(img, state=abi.DisplayState(), threshold=0.5, knee=0.25, intensity=0.2, scatter=0.6, levels=2, exposure_ev=0.5,
                                  clamp_max=8.0, fuse_tail=0),
        "dof": lambda: s.dof(img, z),
        "dof+": lambda: s.dof(img, z, camera=cam, coc=True, focus_distance=1.0, blur_scale=2.0, max_radius=4, planar_depth=1),
        "render_dof": lambda: s.render_dof(cam, opts(), hb.dof_opts(W, H)),
        "render_dof+": lambda: s.render_dof(cam, opts(), hb.dof_opts_from_camera(cam, 0.1, 3.0, W, H, max_radius=4)),
        "upscale": lambda: s.upscale(img, dst=(H2, W2)),
        "upscale+": lambda: s.upscale(img, src=guides, dst=big, stage=True, sigma_normal=32.0, depth_tolerance=0.2),
        "render_upscaled": lambda: s.render_upscaled(cam, opts(), W // 2, 5),
        "render_upscaled+": lambda: s.render_upscaled(cam, opts(), W // 2, 5, dopts=hb.denoise_opts(W // 2, 5, **dn),
                                                      uopts=hb.upscale_opts(W // 2, 5, W, H, sigma_normal=32.0, depth_tolerance=0.2)),
        "radiance": lambda: s.radiance(origins, directions),
        "radiance+": lambda: s.radiance(origins, directions, streams=np.arange(5)[::-1], method=abi.RT_METHOD_NAIVE, samples=2, seed=3,
                                        sample_begin=1, max_depth=5, rr_threshold=2),
    }


# what each call gives on a host-only scene: the library checks every argument before it looks for the device, so all but three
# end at RT_ERR_NO_DEVICE.  The two resets need no device; dof without a camera is refused (planar_depth defaults to 1).
WRAPPER_CODES = {"temporal_reset": abi.RT_OK, "display_reset": abi.RT_OK, "dof": abi.RT_ERR_INVALID_ARGUMENT}


def test_every_blocking_wrapper_passes_the_librarys_argument_checks(hb):
    ls = scenes.load_ssml("rtweekend1")
    s = hb.HipScene(ls.scene, device=abi.RT_DEVICE_NONE)
    cam = hb.camera_new(**ls.camera_params)
    got, want = {}, {}
    for name, call in _wrapper_calls(hb, s, cam).items():
        want[name] = WRAPPER_CODES.get(name, abi.RT_ERR_NO_DEVICE)
        try:
            call()
            got[name] = abi.RT_OK
        except hb.RtHipError as e:
            got[name] = e.code
    assert got == want
    assert (abi.RT_OK, abi.RT_ERR_INVALID_ARGUMENT, abi.RT_ERR_NO_DEVICE) == (0, -1, -2)


def test_an_unknown_channel_or_input_is_refused_before_any_library_call(hb):
    ls = scenes.load_ssml("rtweekend1")
    s = hb.HipScene(ls.scene, device=abi.RT_DEVICE_NONE)
    cam = hb.camera_new(**ls.camera_params)
    o, bad = abi.default_render_opts(W, H, 4), {"no_such_name": 32}
    calls = [
        lambda: s.render_aov(cam, o, channels=("depth", "no_such_name")),
        lambda: s.render_aov_chain(cam, o, channels=("bounces", "no_such_name")),
        lambda: s.render_ao(cam, o, channels=("no_such_name",)),
        lambda: s.render_noise(cam, o, channels=("variance", "no_such_name")),
        lambda: s.render_robust(cam, o, channels=("no_such_name",)),
        lambda: s.robust_combine(np.zeros((2, H, W, 3), F32), 2, channels=("no_such_name",)),
        lambda: s.render_aov_device(cam, o, bad),
        lambda: s.render_aov_chain_device(cam, o, bad),
        lambda: s.render_matte_device(cam, o, bad),
        lambda: s.render_ao_device(cam, o, bad),
        lambda: s.denoise_device(bad, 16, 16, hb.denoise_opts(W, H)),
        lambda: s.render_noise_device(cam, o, bad),
        lambda: s.render_robust_device(cam, o, bad),
        lambda: s.robust_combine_device(16, 2, 2, W, H, bad),
        lambda: s.denoise_temporal_device(bad, cam, None, 0, 16, 16, 16, hb.temporal_opts(W, H)),
        lambda: s.upscale_device(bad, 16, hb.upscale_opts(W, H, 2 * W, 2 * H)),
    ]
    for call in calls:
        with pytest.raises(ValueError, match="no_such_name"):
            call()
    for call in (lambda: s.dof(np.zeros((H, W, 3), F32), np.zeros((H, W + 1), F32)), lambda: s.bloom(np.zeros((H, W), F32)),
                 lambda: s.render_noise(cam, o, albedo=np.zeros((H, W), F32)), lambda: s.denoise(np.zeros((H, W, 3), F32), depth=np.zeros((W, H), F32))):
        with pytest.raises(ValueError, match="must be"):
            call()
