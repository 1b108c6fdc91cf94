"""The ambient-occlusion pass (rt_render_ao) without a GPU: the CPU checker (tests/ao_checker.py) pinned to the oracle piece by
piece, exact and statistical cases on hand-built scenes, then the C-ABI boundary on a host-only scene: structs, defaults and the
status code of every check."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ao_checker as A
import aov_checker as K
import scenes

abi = scenes.abi
ROOT = scenes.ROOT
F32 = np.float32
SQUARE = dict(vup=(0.0, 0.0, 1.0), aspect_ratio=1.0, aperture=0.0, focus_dist=10.0)


# ---- the restatement against the oracle, piece by piece ----
def test_the_ao_draws_are_the_f32_draws_behind_the_two_jitter_draws(O):
    """every draw of a stream, rt_rng_range_f32 (the jitter) or rt_rng_f32, takes ONE 32-bit word: the jitter is words 0 and 1 as
    aov_checker.jitter forms them, so the rt_rng_f32 draws that follow are words 2 ... as (word >> 8) * 2^-24 -- which is what
    oracle.rng_f32 returns at positions 2 ..."""
    for seed, pixel, sample, k in ((3, 0, 0, 4), (1, 2303, 5, 1), (0xFFFFFFFF12345678, 1 << 30, (1 << 32) + 7, 64)):
        words = O.rng_u32(seed, pixel, sample, 2 + 2 * k)
        as_f32 = (words >> np.uint32(8)).astype(np.float32) * F32(2.0 ** -24)
        assert O.rng_f32(seed, pixel, sample, 2 + 2 * k).tobytes() == as_f32.tobytes()
        assert A.ao_draws(seed, [pixel], sample, k)[0].tobytes() == as_f32[2:].tobytes()
        unit = ((words[:2] >> np.uint32(9)) | np.uint32(0x3F800000)).view(np.float32) - F32(1.0)
        assert K.jitter(seed, [pixel], sample)[0].tobytes() == unit.tobytes()
    assert (A.ao_draws(3, range(16), 1, 8) < 1.0).all() and (A.ao_draws(3, range(16), 1, 8) >= 0.0).all()


def _normals():
    rng = np.random.default_rng(7)
    z = rng.normal(size=(200, 3))
    z /= np.linalg.norm(z, axis=1, keepdims=True)
    axes = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    ties = [(0.6, 0.6, 0.52915026), (-0.6, 0.6, 0.52915026), (0.70710678, 0.70710678, 0.0)]  # |x| == |y|: the second branch
    return np.concatenate([z, np.array(axes + ties)]).astype(np.float32)


def test_the_frame_is_the_oracles(O):
    rng = np.random.default_rng(8)
    for z in _normals():
        for v in rng.uniform(-1, 1, (4, 3)).astype(np.float32):
            mine = A.to_coord(A.coord_from_z(z[None, :]), v[None, :])[0]
            assert mine.tobytes() == O.coord_apply(z, v).tobytes(), (z, v)
    # the frame is orthonormal and right-handed about z to rounding
    x, y, zz = A.coord_from_z(_normals())
    assert np.abs((x * y).sum(axis=1)).max() < 1e-6 and np.abs((x * zz).sum(axis=1)).max() < 1e-6
    assert np.abs(np.linalg.norm(x, axis=1) - 1).max() < 1e-6 and np.abs(np.linalg.norm(y, axis=1) - 1).max() < 1e-6


def test_lambertian_sample_is_the_oracles(O):
    """oracle sample i of ora_sample_directions is lambertian_sample on the stream (seed, 0, i) from its start"""
    n, seed = 64, 11
    draws = np.stack([O.rng_f32(seed, 0, i, 2) for i in range(n)])
    for z in _normals()[::9]:
        ref = O.sample_directions_noscene(0, n, seed=seed, normal=tuple(float(c) for c in z))
        mine = A.lambertian_sample(np.broadcast_to(z, (n, 3)), draws[:, 0], draws[:, 1])
        assert mine.dtype == np.float32 and mine.tobytes() == ref.tobytes(), z
        assert ((mine * z).sum(axis=1) > 0).all()  # in the hemisphere of the normal: cos_theta >= 2^-12


# ---- exact cases on hand-built scenes ----
def _floor(sc, z=0.0, half=500.0):
    """one big triangle in the plane z, normal up"""
    n = (0.0, 0.0, 1.0)
    sc.triangle([(-half, -half, z), (half, -half, z), (0.0, 2 * half, z)], [n, n, n], sc.lambertian(sc.solid((0.5, 0.5, 0.5)), 0.5))


def _sky(sc):
    sc.set_sky(sc.lerp((0.5, 0.7, 1.0), (1.0, 1.0, 1.0)), (0, 0))
    return sc


def test_inside_one_large_sphere(O):
    """every camera ray hits the wall from inside and every AO ray hits it again: visibility exactly 0 without a limit.  An AO ray
    at angle theta to the (inward) normal meets the wall after 2 R cos(theta), and cos(theta) = sqrt(1 - r) >= 2^-12: below
    2 R 2^-12 nothing is near enough, visibility exactly 1"""
    R = 10.0
    sc = scenes.SceneDescription()
    sc.sphere((0, 0, 0), R, sc.lambertian(sc.solid((0.5, 0.5, 0.5)), 0.5))
    cpu, cam = O.Scene(_sky(sc)), O.camera_new(origin=(1.0, 2.0, 0.5), lookat=(0.0, 0.0, 0.0), fov=70.0, **SQUARE)
    w, h, spp, k = 8, 6, 2, 4
    closed = A.ao(cpu, cam, w, h, spp, k, radius=0.0, seed=3)
    assert (closed["hits"] == spp).all() and (closed["rays"] == spp * k).all()
    assert (closed["visibility"] == 0.0).all() and not np.signbit(closed["visibility"]).any()
    assert (closed["bent_normal"] == 0.0).all()
    also_closed = A.ao(cpu, cam, w, h, spp, k, radius=np.inf, seed=3)
    assert also_closed["visibility"].tobytes() == closed["visibility"].tobytes()
    near = 2.0 * R * 2.0 ** -12
    opened = A.ao(cpu, cam, w, h, spp, k, radius=0.5 * near, seed=3)
    assert (opened["visibility"] == 1.0).all() and (opened["unoccluded"] == spp * k).all()
    assert (np.linalg.norm(opened["bent_normal"], axis=1) > 0.2).all()


def test_a_floor_under_an_open_sky(O):
    """visibility exactly 1; the bent normal is the mean of cosine-weighted directions, E[d] = (2/3) normal.  Per ray the component
    along the normal is cos(theta) with E = 2/3, E[cos^2] = 1/2: variance 1/18; a tangential component is sin(theta) cos(phi)
    with mean 0 and variance E[sin^2] E[cos^2 phi] = 1/2 * 1/2 = 1/4.  Over N rays sigma = sqrt(variance / N)."""
    sc = scenes.SceneDescription()
    _floor(sc)
    cpu, cam = O.Scene(_sky(sc)), O.camera_new(origin=(3.0, -4.0, 5.0), lookat=(0.0, 0.0, 0.0), fov=40.0, **SQUARE)
    w, h, spp, k = 8, 8, 4, 8
    r = A.ao(cpu, cam, w, h, spp, k, seed=9)
    assert (r["hits"] == spp).all()
    assert (r["visibility"] == 1.0).all()
    n_rays = int(r["rays"].sum())
    assert n_rays == w * h * spp * k == 2048
    mean = (r["bent_normal"].astype(np.float64) * r["rays"][:, None]).sum(axis=0) / n_rays
    sigma_normal, sigma_tangent = np.sqrt(1.0 / 18.0 / n_rays), np.sqrt(0.25 / n_rays)
    print("bent mean", mean, "sigma", sigma_tangent, sigma_normal)
    assert abs(mean[2] - 2.0 / 3.0) < 4 * sigma_normal
    assert abs(mean[0]) < 4 * sigma_tangent and abs(mean[1]) < 4 * sigma_tangent
    # one pixel's value is the plain f32 mean of its rays
    assert (np.linalg.norm(r["bent_normal"], axis=1) <= 1.0).all()


def test_a_frame_that_is_all_sky(O):
    sc = scenes.SceneDescription()
    sc.sphere((0, 0, 50.0), 1.0, sc.lambertian(sc.solid((0.5, 0.5, 0.5)), 0.5))  # behind the camera
    cpu, cam = O.Scene(_sky(sc)), O.camera_new(origin=(0.0, 0.0, 10.0), lookat=(0.0, 0.0, 0.0), fov=40.0, vup=(0.0, 1.0, 0.0),
                                               aspect_ratio=1.0, aperture=0.0, focus_dist=10.0)
    r = A.ao(cpu, cam, 6, 5, 3, 4, seed=2)
    assert (r["hits"] == 0).all() and (r["rays"] == 0).all()
    assert r["visibility"].tobytes() == np.ones(30, F32).tobytes()
    assert r["bent_normal"].tobytes() == np.zeros((30, 3), F32).tobytes()


def test_a_smaller_radius_never_lowers_the_visibility(O):
    """the same seed gives the same rays; a hit nearer than r is nearer than every larger limit"""
    sc = scenes.random_spheres(500, seed=4)
    cpu = O.Scene(sc)
    cam = O.camera_new(origin=(0.0, 0.0, 25.0), lookat=(0.0, 0.0, 0.0), fov=50.0, vup=(0.0, 1.0, 0.0), aspect_ratio=1.0, aperture=0.0,
                       focus_dist=10.0)
    w, h, spp, k = 12, 12, 2, 4
    by_radius = [A.ao(cpu, cam, w, h, spp, k, radius=r, seed=6) for r in (0.0, np.inf, 8.0, 2.0, 1.0, 0.25)]
    assert by_radius[0]["visibility"].tobytes() == by_radius[1]["visibility"].tobytes()  # no limit = an infinite one
    for wide, narrow in zip(by_radius[1:], by_radius[2:]):
        assert (wide["rays"] == narrow["rays"]).all()
        assert (narrow["unoccluded"] >= wide["unoccluded"]).all()
        assert (narrow["visibility"] >= wide["visibility"]).all()
    total = by_radius[0]["rays"].sum()
    shares = [1.0 - b["unoccluded"].sum() / total for b in by_radius]
    print("occluded shares by radius", shares)
    assert shares[0] > 0.05 and shares[0] > shares[3] > shares[5]  # the limit does something here


# ---- a statistical case: the form factor of a sphere ----
def test_a_floor_point_under_a_sphere_sees_its_form_factor(O):
    """A sphere of radius R centred at height c over a floor point fills, cosine-weighted, (R / c)^2 of the point's hemisphere (the
    configuration factor of a sphere seen from a surface element whose normal points at its centre): visibility = 1 - (R / c)^2.
    A uniform sampler would give the solid-angle share instead, 1 - (1 - sqrt(1 - (R / c)^2)) -- 0.866 against 0.75 here, 17 sigma
    away.  The narrow camera sees the floor within 0.003 of the point, which moves the factor by less than 1e-5."""
    R, c = 1.0, 2.0
    sc = scenes.SceneDescription()
    _floor(sc)
    sc.sphere((0.0, 0.0, c), R, sc.lambertian(sc.solid((0.5, 0.5, 0.5)), 0.5))
    cpu, cam = O.Scene(_sky(sc)), O.camera_new(origin=(5.0, 0.0, 1.0), lookat=(0.0, 0.0, 0.0), fov=0.05, **SQUARE)
    w, h, spp, k = 4, 4, 16, 16
    r = A.ao(cpu, cam, w, h, spp, k, seed=5)
    assert (r["hits"] == spp).all()
    n_rays = int(r["rays"].sum())
    assert n_rays == 4096
    expected = 1.0 - (R / c) ** 2
    sigma = np.sqrt(expected * (1.0 - expected) / n_rays)
    seen = r["unoccluded"].sum() / n_rays
    print("visibility", seen, "expected", expected, "sigma", sigma)
    assert abs(seen - expected) < 4 * sigma
    # the bent normal leans away from nothing: the occluder is centred, the open ring is symmetric
    mean = (r["bent_normal"].astype(np.float64) * r["rays"][:, None]).sum(axis=0) / n_rays
    assert abs(mean[0]) < 4 * np.sqrt(0.25 / n_rays) and abs(mean[1]) < 4 * np.sqrt(0.25 / n_rays)


# ---- the C ABI on a host-only scene ----
def _buffers(n):
    b = abi.AoBuffers()
    keep = [np.zeros(n, F32), np.zeros(3 * n, F32)]
    b.visibility = keep[0].ctypes.data_as(C.POINTER(C.c_float))
    b.bent_normal = keep[1].ctypes.data_as(C.POINTER(C.c_float))
    return b, keep


def test_symbols_structs_and_defaults(hb):
    lib = hb.lib()
    for sym in ("rt_ao_opts_default", "rt_render_ao", "rt_render_ao_device"):
        assert sym in abi.EXPORTED_SYMBOLS and hasattr(lib, sym)
    assert lib.rt_abi_version() == abi.RT_ABI_VERSION == 2
    assert C.sizeof(abi.AoOpts) == abi.EXPECTED_SIZES["rt_ao_opts"][1] == 32
    assert C.sizeof(abi.AoBuffers) == abi.EXPECTED_SIZES["rt_ao_buffers"][1] == 16
    assert tuple(n for n, _ in abi.AoBuffers._fields_) == abi.AO_CHANNELS == ("visibility", "bent_normal")
    assert abi.AO_MAX_RAYS == A.MAX_RAYS == 64
    o = abi.AoOpts()
    C.memset(C.byref(o), 0xFF, C.sizeof(o))
    assert lib.rt_ao_opts_default(C.byref(o)) == abi.RT_OK
    assert o.rays_per_pass == 4 and o.radius == 0.0 and not np.signbit(o.radius) and list(o.reserved) == [0] * 6
    assert bytes(abi.default_ao_opts()) == bytes(o) == bytes(hb.ao_opts())
    assert lib.rt_ao_opts_default(None) == abi.RT_ERR_INVALID_ARGUMENT
    a = hb.ao_opts(rays_per_pass=7, radius=0.5)
    assert (a.rays_per_pass, a.radius) == (7, 0.5)
    with pytest.raises(ValueError):
        hb.ao_opts(falloff=1.0)


def test_render_ao_status_codes_without_a_device(hb):
    ls = scenes.load_ssml("rtweekend1")
    s = hb.HipScene(ls.scene, device=abi.RT_DEVICE_NONE)
    cam = hb.camera_new(**ls.camera_params)
    lib = hb.lib()
    w, h = 16, 9
    n = w * h

    def call(opts, aopts, bufs, device=False, scene=s._h, camera=cam):
        f = lib.rt_render_ao_device if device else lib.rt_render_ao
        ref = lambda x: None if x is None else C.byref(x)  # noqa: E731
        args = (scene, ref(camera), ref(opts), ref(aopts), ref(bufs)) + ((C.c_void_p(0),) if device else ())
        return f(*args)

    ok, ao = abi.default_render_opts(w, h, 2), abi.default_ao_opts()
    for device in (False, True):
        full, keep = _buffers(n)
        for good in (ao, abi.default_ao_opts(1), abi.default_ao_opts(64), abi.default_ao_opts(4, 0.25), abi.default_ao_opts(4, np.inf),
                     abi.default_ao_opts(4, -0.0)):
            assert call(ok, good, full, device) == abi.RT_ERR_NO_DEVICE
        for only in abi.AO_CHANNELS:  # either channel alone
            b = abi.AoBuffers()
            setattr(b, only, getattr(full, only))
            assert call(ok, ao, b, device) == abi.RT_ERR_NO_DEVICE, only
        assert call(ok, ao, abi.AoBuffers(), device) == abi.RT_ERR_INVALID_ARGUMENT  # both NULL
        for args in ((None, ao, full), (ok, None, full), (ok, ao, None)):
            assert call(*args, device) == abi.RT_ERR_INVALID_ARGUMENT
        assert call(ok, ao, full, device, scene=None) == abi.RT_ERR_INVALID_ARGUMENT
        assert call(ok, ao, full, device, camera=None) == abi.RT_ERR_INVALID_ARGUMENT
        for bad in (dict(rays_per_pass=0), dict(rays_per_pass=65), dict(rays_per_pass=0xFFFFFFFF), dict(radius=-1.0),
                    dict(radius=-1e-30), dict(radius=-np.inf), dict(radius=np.nan)):
            assert call(ok, abi.default_ao_opts(**bad), full, device) == abi.RT_ERR_INVALID_ARGUMENT, bad
        for word in range(6):
            a = abi.default_ao_opts()
            a.reserved[word] = 1
            assert call(ok, a, full, device) == abi.RT_ERR_INVALID_ARGUMENT, word
        # samples_per_pixel * K must stay below 2^32
        assert call(abi.default_render_opts(w, h, (1 << 30) - 1), ao, full, device) == abi.RT_ERR_NO_DEVICE
        assert call(abi.default_render_opts(w, h, 1 << 30), ao, full, device) == abi.RT_ERR_INVALID_ARGUMENT
        assert call(abi.default_render_opts(w, h, (1 << 32) - 1), abi.default_ao_opts(1), full, device) == abi.RT_ERR_NO_DEVICE
        assert call(abi.default_render_opts(w, h, 1 << 26), abi.default_ao_opts(64), full, device) == abi.RT_ERR_INVALID_ARGUMENT
        # overlapping outputs: the visibility on the last value of the bent normal, and the other way round
        b, keep = _buffers(n)
        b.visibility = C.cast(C.c_void_p(keep[1].ctypes.data + 4 * (3 * n - 1)), C.POINTER(C.c_float))
        assert call(ok, ao, b, device) == abi.RT_ERR_INVALID_ARGUMENT
        b.visibility = C.cast(C.c_void_p(keep[1].ctypes.data + 4 * 3 * n), C.POINTER(C.c_float))  # ... just behind it
        assert call(ok, ao, b, device) == abi.RT_ERR_NO_DEVICE
        b, keep = _buffers(n)
        b.bent_normal = C.cast(C.c_void_p(keep[0].ctypes.data + 4 * (n - 1)), C.POINTER(C.c_float))
        assert call(ok, ao, b, device) == abi.RT_ERR_INVALID_ARGUMENT
        # the rules of rt_render_aov
        o = abi.default_render_opts(w, h, 2)
        o.output_layout = abi.RT_LAYOUT_SHARD
        assert call(o, ao, full, device) == abi.RT_ERR_UNSUPPORTED
        o = abi.default_render_opts(w, h, 2)
        o.shard_count = 2
        assert call(o, ao, full, device) == abi.RT_ERR_UNSUPPORTED
        assert call(abi.default_render_opts(1, h, 2), ao, full, device) == abi.RT_ERR_INVALID_ARGUMENT
        assert call(abi.default_render_opts(w, 1, 2), ao, full, device) == abi.RT_ERR_INVALID_ARGUMENT
        assert call(abi.default_render_opts(w, h, 0), ao, full, device) == abi.RT_ERR_INVALID_ARGUMENT
        assert call(abi.default_render_opts(1 << 16, 1 << 15, 2), ao, full, device) == abi.RT_ERR_UNSUPPORTED  # 2^31 pixels
    with pytest.raises(hb.RtHipError) as e:
        s.render_ao(cam, ok)
    assert e.value.code == abi.RT_ERR_NO_DEVICE
    with pytest.raises(hb.RtHipError) as e:
        s.render_ao(cam, ok, rays_per_pass=65)
    assert e.value.code == abi.RT_ERR_INVALID_ARGUMENT
    with pytest.raises(hb.RtHipError) as e:
        s.render_ao(cam, ok, radius=-2.0)
    assert e.value.code == abi.RT_ERR_INVALID_ARGUMENT
    with pytest.raises(hb.RtHipError) as e:
        s.render_ao(cam, ok, channels=())
    assert e.value.code == abi.RT_ERR_INVALID_ARGUMENT
    with pytest.raises(ValueError):
        s.render_ao(cam, ok, channels=("visibility", "coverage"))
    with pytest.raises(ValueError):
        s.render_ao_device(cam, ok, {"visibility": 16, "normal": 32})


def test_cpp_wrapper_compiles():
    src = ('#include "rt_hip.hpp"\nint main() { rt_hip::AoOptions a; a.rays_per_pass = 8; a.radius = 0.5f;\n'
           'rt_hip::AoBuffers (*f)(const rt_hip::RenderOptions &, const rt_hip::SimpleCamera &, const rt_hip::Bvh &, '
           'const rt_hip::AoOptions &, uint64_t, uint64_t) = &rt_hip::render_ao; (void)f; (void)a;\n'
           'rt_ao_opts o; rt_ao_buffers b = {nullptr, nullptr}; (void)o; (void)b;\n'
           'rt_hip::AoBuffers r; return (int)(r.visibility.size() + r.bent_normal.size()); }\n')
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-x", "c++", "-"],
                   input=src.encode(), check=True)
