"""Specular-chain AOV buffers (rt_render_aov_chain) without a GPU: the CPU checker (tests/aov_chain_checker.py) on answers known
by hand, the ABI surface, the defaults, and every status code the entry points return before they need a device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import aov_chain_checker as KC
import aov_checker as K
import scenes

abi = scenes.abi
ROOT = scenes.ROOT
F32 = np.float32
UP, DOWN = (0.0, 0.0, 1.0), (0.0, 0.0, -1.0)


def _plane(sc, z, normal, material, half=10.0):
    """one big triangle in the plane z = const around the origin (primitive index = order of creation)"""
    sc.triangle([(-half, -half, z), (half, -half, z), (0.0, half, z)], [normal] * 3, material)


def _mirror_and_wall(fuzz=0.0):
    """primitive 0: a mirror in z = 0 tinted (0.9, 0.8, 0.7); primitive 1: a Lambertian wall in z = 5 facing it"""
    sc = scenes.SceneDescription()
    _plane(sc, 0.0, UP, sc.reflect(sc.solid((0.9, 0.8, 0.7)), fuzz))
    _plane(sc, 5.0, DOWN, sc.lambertian(sc.solid((0.2, 0.4, 0.6)), 0.5))
    sc.set_sky(sc.lerp((0.5, 0.7, 1.0), (1.0, 1.0, 1.0)), (0, 0))
    return sc


def _ray(o, d):
    return np.array([o], F32), np.array([d], F32)


def test_offset_ray_restatement_matches_the_oracle(O):
    rng = np.random.default_rng(1)
    p = rng.uniform(-5, 5, (200, 3)).astype(F32)
    n = K.normalised(rng.uniform(-1, 1, (200, 3)).astype(F32))
    n[:20, 0] = 0.0  # components whose offset is +-0
    p[:10, 1] = 0.0
    e = rng.uniform(0, 1e-3, (200, 3)).astype(F32)
    for brdf in (True, False):
        mine = KC.offset_rays(p, n, e, brdf)
        ref = np.stack([O.offset_ray(p[i], n[i], e[i], brdf) for i in range(len(p))])
        assert mine.tobytes() == ref.tobytes()


def test_mirror_facing_a_wall(O):
    sc = _mirror_and_wall()
    cpu = O.Scene(sc)
    c = KC.chain_terms(sc, cpu, *_ray((0.1, 0.2, 3.0), (0.0, 0.0, -1.0)))
    order = cpu.primitive_order()
    assert c["b"][0] == 1 and c["hit"][0]
    assert order[int(c["terminal"]["index"][0])] == 1  # the wall, not the mirror
    assert c["terminal"]["material"][0] == 1
    assert np.allclose(c["normal"][0], DOWN, atol=1e-6)  # the wall's own (interpolated) normal: not un-mirrored
    assert abs(float(c["D"][0]) - 3.0) < 1e-5 and abs(float(c["depth"][0]) - 8.0) < 1e-2
    assert np.allclose(c["wo"][0], UP, atol=1e-6)
    # albedo = the mirror's tint * (the wall's colour * its Lambertian albedo), in f32
    expect = np.array((0.9, 0.8, 0.7), F32) * (np.array((0.2, 0.4, 0.6), F32) * F32(0.5))
    assert c["albedo"][0].tobytes() == expect.tobytes()
    # max_chain = 0: the mirror itself is the terminal, with its own tint and no Lambertian factor
    c0 = KC.chain_terms(sc, cpu, *_ray((0.1, 0.2, 3.0), (0.0, 0.0, -1.0)), max_chain=0)
    assert c0["b"][0] == 0 and order[int(c0["terminal"]["index"][0])] == 0
    assert c0["albedo"][0].tobytes() == np.array((0.9, 0.8, 0.7), F32).tobytes() and abs(float(c0["depth"][0]) - 3.0) < 1e-5


def test_glass_sphere_along_a_diameter_is_traversed_undeviated(O):
    sc = scenes.SceneDescription()
    sc.sphere((0.0, 0.0, 0.0), 1.0, sc.refract(sc.solid((1.0, 0.9, 0.8)), 1.5))
    sc.sphere((-6.0, -4.0, -10.0), 3.0, sc.lambertian(sc.solid((0.3, 0.3, 0.3)), 0.8))  # behind it, on the same line
    sc.set_sky(sc.solid((0.5, 0.5, 0.5)), (0, 0))
    cpu = O.Scene(sc)
    o, d = (3.0, 2.0, 5.0), (-3.0, -2.0, -5.0)
    c = KC.chain_terms(sc, cpu, *_ray(o, d))
    assert c["b"][0] == 2 and c["hit"][0]
    assert cpu.primitive_order()[int(c["terminal"]["index"][0])] == 1
    assert np.allclose(c["wo"][0], K.normalised(np.array([d], F32))[0], atol=2e-3)
    dist = float(np.linalg.norm(o))
    assert abs(float(c["D"][0]) - (dist - 1.0 + 2.0)) < 1e-2  # to the sphere, then across its diameter
    behind = float(np.linalg.norm(np.array((-6.0, -4.0, -10.0)))) - 3.0 - 1.0
    assert abs(float(c["depth"][0]) - (dist + 1.0 + behind)) < 2e-2
    tint = np.array((1.0, 0.9, 0.8), F32)
    assert c["T"][0].tobytes() == (tint * tint).tobytes()  # entered and left


def test_total_internal_reflection_takes_the_reflect_branch(O):
    sc = scenes.SceneDescription()
    sc.sphere((0.0, 0.0, 0.0), 1.0, sc.refract(sc.solid((1.0, 1.0, 1.0)), 1.5))
    sc.set_sky(sc.solid((0.5, 0.5, 0.5)), (0, 0))
    cpu = O.Scene(sc)
    # from inside, meeting the surface at sin(theta) = 0.9: 1.5 * 0.9 > 1
    o, d = np.array((0.9, 0.0, 0.0)), np.array((0.0, 1.0, 0.0))
    p1 = np.array((0.9, np.sqrt(1.0 - 0.81), 0.0))
    r = d - 2.0 * np.dot(d, p1) * p1  # mirrored about the surface normal
    p2 = p1 - 2.0 * np.dot(p1, r) * r  # where that chord meets the sphere again
    c = KC.chain_terms(sc, cpu, *_ray(o, d), max_chain=1)
    assert c["b"][0] == 1 and c["hit"][0] and c["terminal"]["out"][0] == 0  # still inside
    assert np.allclose(c["wo"][0], r, atol=1e-5) and np.allclose(c["terminal"]["point"][0], p2, atol=1e-3)
    # had it refracted it would have left: with a long chain it keeps circling inside instead
    assert KC.chain_terms(sc, cpu, *_ray(o, d), max_chain=6)["b"][0] == 6


def test_two_facing_mirrors_stop_at_max_chain(O):
    sc = scenes.SceneDescription()
    mirror = sc.reflect(sc.solid((0.5, 1.0, 1.0)), 0.0)
    _plane(sc, 0.0, UP, mirror)
    _plane(sc, 2.0, DOWN, mirror)
    sc.set_sky(sc.solid((0.5, 0.5, 0.5)), (0, 0))
    cpu = O.Scene(sc)
    d = np.array((0.01, 0.02, -1.0))
    for max_chain in (1, 5, 64):
        c = KC.chain_terms(sc, cpu, *_ray((0.1, 0.1, 1.0), d), max_chain=max_chain)
        assert c["b"][0] == max_chain and c["hit"][0]
        assert sc.materials[int(c["terminal"]["material"][0])].type == abi.RT_MAT_REFLECT
        assert abs(float(c["depth"][0]) / ((1.0 + 2.0 * max_chain) * np.linalg.norm(d)) - 1.0) < 1e-3
        assert c["T"][0].tobytes() == np.array((F32(0.5) ** max_chain, 1.0, 1.0), F32).tobytes()


def test_a_chain_that_ends_on_the_sky(O):
    sc = _mirror_and_wall()
    cpu = O.Scene(sc)
    c = KC.chain_terms(sc, cpu, *_ray((0.0, 8.0, 3.0), (0.0, 0.5, -1.0)))  # reflected past the wall's tip
    assert c["b"][0] == 1 and not c["hit"][0]
    assert np.array_equal(c["normal"][0], np.zeros(3, F32))
    sky = K.texture_colours(sc, int(sc.materials[int(c["terminal"]["material"][0])].texture), c["wo"], np.zeros((1, 3), F32))
    assert c["albedo"][0].tobytes() == (np.array((0.9, 0.8, 0.7), F32) * sky[0]).tobytes()
    # folded: such passes count toward neither depth nor coverage, but toward bounces
    cam = O.camera_new(origin=(0.0, 0.0, 4.0), lookat=(3.0, 0.0, 0.0), vup=(0.0, 1.0, 0.0), fov=20.0, aspect_ratio=16.0 / 9.0,
                       aperture=0.0, focus_dist=10.0)
    a = KC.aovs(sc, cpu, cam, 16, 9, 1, seed=2)
    sky_end = (a["bounces"] == 1.0) & (a["primitive"] == K.NO_ID)
    assert sky_end.any() and ((a["bounces"] == 1.0) & (a["primitive"] == 1)).any()  # past the wall's edge, and onto the wall
    assert (a["coverage"][sky_end] == 0.0).all() and (a["depth"][sky_end] == 0.0).all() and (a["material"][sky_end] == K.NO_ID).all()
    assert (a["albedo"][sky_end] > 0.0).all()


def test_fuzz_limit_decides_whether_a_fuzzy_mirror_is_followed(O):
    sc = _mirror_and_wall(fuzz=0.3)
    cpu = O.Scene(sc)
    ray = _ray((0.1, 0.2, 3.0), (0.0, 0.0, -1.0))
    order = cpu.primitive_order()
    at0 = KC.chain_terms(sc, cpu, *ray, fuzz_limit=0.0)
    assert at0["b"][0] == 0 and order[int(at0["terminal"]["index"][0])] == 0
    at1 = KC.chain_terms(sc, cpu, *ray, fuzz_limit=1.0)
    assert at1["b"][0] == 1 and order[int(at1["terminal"]["index"][0])] == 1
    sharp = KC.chain_terms(_mirror_and_wall(), O.Scene(_mirror_and_wall()), *ray)
    assert at1["depth"].tobytes() == sharp["depth"].tobytes()  # the fuzz term is left out, not drawn


@pytest.mark.parametrize("name", ["all_materials", "random_everything_2", "random_everything_7"])
def test_max_chain_zero_is_the_first_hit_checker(O, name):
    sc, cam_params = (scenes.all_materials(), scenes.ALL_MATERIALS_CAMERA) if name == "all_materials" else \
        scenes.random_everything(int(name.rsplit("_", 1)[1]))
    cpu, cam = O.Scene(sc), O.camera_new(**cam_params)
    w, h, spp = 32, 18, 3
    first = K.aovs(sc, cpu, cam, w, h, spp, seed=4, sample_begin=2)
    chain = KC.aovs(sc, cpu, cam, w, h, spp, seed=4, sample_begin=2, max_chain=0)
    for ch in abi.AOV_CHANNELS:
        assert chain[ch].dtype == first[ch].dtype and chain[ch].tobytes() == first[ch].tobytes(), ch
    assert (chain["bounces"] == 0.0).all()
    deep = KC.aovs(sc, cpu, cam, w, h, spp, seed=4, sample_begin=2, max_chain=8, fuzz_limit=1.0)
    assert deep["bounces"].max() >= 1.0 and deep["albedo"].tobytes() != first["albedo"].tobytes()  # the scene has delta surfaces


def _buffers(n, channels):
    b, keep = abi.AovChainBuffers(), []
    for name in channels:
        a = np.zeros(n * (3 if name in ("albedo", "normal") else 1), dtype=np.uint32 if name in ("primitive", "material") else F32)
        keep.append(a)
        setattr(b if name == "bounces" else b.aov, name, a.ctypes.data_as(C.POINTER(C.c_uint32 if a.dtype == np.uint32 else C.c_float)))
    return b, keep


def test_symbols_structs_and_defaults(hb):
    lib = hb.lib()
    for sym in ("rt_aov_chain_opts_default", "rt_render_aov_chain", "rt_render_aov_chain_device"):
        assert sym in abi.EXPORTED_SYMBOLS and hasattr(lib, sym)
    assert C.sizeof(abi.AovChainOpts) == abi.EXPECTED_SIZES["rt_aov_chain_opts"][1] == 32
    assert C.sizeof(abi.AovChainBuffers) == abi.EXPECTED_SIZES["rt_aov_chain_buffers"][1] == 56
    assert abi.AOV_CHAIN_CHANNELS == abi.AOV_CHANNELS + ("bounces",)
    o = abi.AovChainOpts()
    C.memset(C.byref(o), 0xFF, C.sizeof(o))
    assert lib.rt_aov_chain_opts_default(C.byref(o)) == abi.RT_OK
    assert o.max_chain == 8 and o.fuzz_limit == 0.0 and list(o.reserved) == [0] * 6
    d = abi.default_aov_chain_opts()
    assert bytes(d) == bytes(o)
    assert lib.rt_aov_chain_opts_default(None) == abi.RT_ERR_INVALID_ARGUMENT


def test_status_codes_without_a_device(hb):
    ls = scenes.load_ssml("rtweekend1")
    s = hb.HipScene(ls.scene, device=abi.RT_DEVICE_NONE)
    cam = hb.camera_new(**ls.camera_params)
    lib = hb.lib()
    w, h = 16, 9

    def call(opts, copts, bufs, device=False, scene=s._h, camera=cam):
        f = lib.rt_render_aov_chain_device if device else lib.rt_render_aov_chain
        ref = lambda x: None if x is None else C.byref(x)  # noqa: E731
        args = (scene, ref(camera), ref(opts), ref(copts), ref(bufs)) + ((C.c_void_p(0),) if device else ())
        return f(*args)

    ok, chain = abi.default_render_opts(w, h, 2), abi.default_aov_chain_opts()
    for device in (False, True):
        full, _keep = _buffers(w * h, abi.AOV_CHAIN_CHANNELS)
        assert call(ok, chain, full, device) == abi.RT_ERR_NO_DEVICE
        only_bounces, _keep2 = _buffers(w * h, ("bounces",))
        assert call(ok, chain, only_bounces, device) == abi.RT_ERR_NO_DEVICE  # `bounces` alone is a channel
        for args in ((None, chain, full), (ok, None, full), (ok, chain, None)):
            assert call(*args, device) == abi.RT_ERR_INVALID_ARGUMENT
        assert call(ok, chain, full, device, scene=None) == abi.RT_ERR_INVALID_ARGUMENT
        assert call(ok, chain, full, device, camera=None) == abi.RT_ERR_INVALID_ARGUMENT
        assert call(ok, chain, abi.AovChainBuffers(), device) == abi.RT_ERR_INVALID_ARGUMENT  # all NULL
        for bad in (dict(max_chain=65), dict(fuzz_limit=-0.5), dict(fuzz_limit=float("nan")), dict(fuzz_limit=float("inf"))):
            assert call(ok, abi.default_aov_chain_opts(**bad), full, device) == abi.RT_ERR_INVALID_ARGUMENT, bad
        for good in (dict(max_chain=0), dict(max_chain=64), dict(fuzz_limit=1.0)):
            assert call(ok, abi.default_aov_chain_opts(**good), full, device) == abi.RT_ERR_NO_DEVICE, good
        o = abi.default_render_opts(w, h, 2)
        o.output_layout = abi.RT_LAYOUT_SHARD
        assert call(o, chain, full, device) == abi.RT_ERR_UNSUPPORTED
        o = abi.default_render_opts(w, h, 2)
        o.shard_count = 2
        assert call(o, chain, full, device) == abi.RT_ERR_UNSUPPORTED
        assert call(abi.default_render_opts(1, h, 2), chain, full, device) == abi.RT_ERR_INVALID_ARGUMENT
        assert call(abi.default_render_opts(w, 1, 2), chain, full, device) == abi.RT_ERR_INVALID_ARGUMENT
        assert call(abi.default_render_opts(w, h, 0), chain, full, device) == abi.RT_ERR_INVALID_ARGUMENT
        assert call(abi.default_render_opts(1 << 16, 1 << 15, 2), chain, full, device) == abi.RT_ERR_UNSUPPORTED  # 2^31 pixels
    with pytest.raises(hb.RtHipError) as e:
        s.render_aov_chain(cam, ok)
    assert e.value.code == abi.RT_ERR_NO_DEVICE
    with pytest.raises(hb.RtHipError) as e:
        s.render_aov_chain(cam, ok, max_chain=65)
    assert e.value.code == abi.RT_ERR_INVALID_ARGUMENT
    with pytest.raises(ValueError):
        s.render_aov_chain(cam, ok, channels=("albedo", "colour"))
    with pytest.raises(ValueError):
        s.render_aov_chain_device(cam, ok, {"colour": 16})


def test_cpp_wrapper_compiles():
    src = ('#include "rt_hip.hpp"\nint main() { rt_hip::AovChainOptions c; c.max_chain = 4; c.fuzz_limit = 0.5f;\n'
           'rt_hip::AovChainBuffers (*f)(const rt_hip::RenderOptions &, const rt_hip::SimpleCamera &, const rt_hip::Bvh &, '
           'const rt_hip::AovChainOptions &, uint64_t, uint64_t) = &rt_hip::render_aov_chain; (void)f; (void)c;\n'
           'rt_hip::AovChainBuffers b; const rt_hip::AovBuffers &as_guides = b; (void)as_guides; return (int)b.bounces.size(); }\n')
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-x", "c++", "-"],
                   input=src.encode(), check=True)
