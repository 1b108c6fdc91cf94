"""The two-sphere kernels' shadow walk.  Their scenes have no emissive primitive, so every shadow ray is a sky shadow ray without a
limit and asks of a sphere only whether some t > 0 exists; the kernels answer that from signs, without the square root and the
quotient of Sphere::get_int, and send what the signs cannot settle to the full test (csrc/rt_intersect.h
sphere_occludes_unlimited).  (a) the predicate next to `hit && t > 0` ON the device, over the host check's own edge grid and 2^20
seeded random cases, and trace_any's whole two-sphere arm next to the arm with the full test, on scenes that send lanes into its cold
loop; (b) frames and ray counts, bit for bit against the oracle and against the general spheres-only kernel, on scenes
that stress it.  tests/test_pair_shadow_host.py runs the same predicate on the CPU."""
import numpy as np
import pytest

import host_check
import scenes
from gpu_support import CAMERA_16_9, abi, assert_same_bits

pytestmark = pytest.mark.gpu

W, H, SPP = 64, 48, 16


@pytest.fixture(scope="module")
def edge_grid(tmp_path_factory):
    """(n, 10) f32: centre, radius, origin, direction -- the edge grid of tests/cpp/pair_shadow_check.cpp, written out by that
    program itself (host code only, built here without the sanitizers), so that host and device run the very same operands"""
    return host_check.edge_grid("pair_shadow_check", 10, tmp_path_factory)


def _random_cases(n):
    """seeded: unit directions, radii over twelve decades, origins on (with a shadow ray's offset), inside, near and far from the sphere"""
    rng = np.random.default_rng(20261019)
    radius = (2.0 ** rng.uniform(-20.0, 20.0, n)).astype(np.float32)
    centre = rng.uniform(-4.0, 4.0, (n, 3)).astype(np.float32)
    nrm = rng.normal(size=(n, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    where = rng.integers(0, 8, n)
    dist = np.select([where == 0, where == 1, where == 2, where == 3, where == 4],
                     [1.0, 1.0 + 1e-4 / radius, 1.0 - 1e-4 / radius, rng.uniform(0.0, 1.0, n), 1.0 + rng.uniform(0.0, 1.0, n)],
                     1.0 + 2.0 ** rng.uniform(0.0, 20.0, n))
    origin = centre + (radius * dist)[:, None] * nrm
    return np.concatenate([centre, radius[:, None], origin, d], axis=1).astype(np.float32)


def test_the_sign_predicate_is_the_full_test_on_the_device(hb, edge_grid):
    edges = edge_grid
    res = hb.selftest_pair_shadow(edges)
    print("edge grid:", res)
    assert res["tested"] == len(edges) > 10_000 and res["mismatches"] == 0 and res["asked_mismatches"] == 0, res
    assert res["asked"] > 0, res  # the grid reaches the cold path
    rnd = _random_cases(1 << 20)
    res = hb.selftest_pair_shadow(rnd)
    print("random:", res)
    assert res["tested"] == 1 << 20 and res["mismatches"] == 0 and res["asked_mismatches"] == 0, res
    assert res["asked"] < (1 << 20) // 100, res  # ... which stays cold
    with pytest.raises(hb.RtHipError):
        hb.selftest_pair_shadow(edges, device=99)


# ---- the walk around the predicate: trace_any's two-sphere arm as the render kernels instantiate it.  A pair scene the host accepts
# (radii in [2^-20, 2^32], shadow origins 1e-4 off a surface) practically never sends a lane into the arm's cold loop, so no frame
# reaches it; rt_selftest_pair_shadow_walk runs the arm itself on scenes that do.
# What a sphere is to a ray from the origin along +y (before `skip`): name -> (centre, radius)
_A = float(np.float32(2.0 ** -30.5))  # radius^2 ~ 2^-61: at the sphere's centre c lies in (-2^-60, 0)
WALK_SPHERES = {
    "occludes, by signs": ((0.0, 3.0, 0.0), 1.0),                      # ahead: ddp > 0
    "occludes, inside": ((0.0, -0.25, 0.0), 1.0),                      # centre behind the origin, origin inside: c < 0, tame
    "clear": ((0.0, -3.0, 0.0), 1.0),                                  # behind
    "clear, beside": ((3.0, 3.0, 0.0), 1.0),                           # box hit or not, no root
    "asks, huge radius, occludes": ((0.0, 0.0, -2.0 ** 60), float(np.float32(2.0 ** 60 * (1 + 2.0 ** -20)))),  # inside, ddp = 0
    "asks, huge radius, ahead": ((0.0, 2.0 ** 61, 0.0), 2.0 ** 60),    # ddp > 0 and a root, radius above 2^59
    "asks, huge radius, clear": ((0.0, -2.0 ** 62, 0.0), 2.0 ** 60),   # behind, outside: root fails -> not asked after all
    "asks, origin at the centre": ((0.0, 0.0, 0.0), _A),               # c = -radius^2 in (-2^-60, 0): the full test says occluded
    "asks, c in the band, clear": ((0.0, -_A * float(np.float32(1 - 2.0 ** -12)), 0.0), _A),  # just inside, centre behind... still occluded or not: the arms must agree
}
WALK_DIRECTIONS = [(0.0, 1.0, 0.0), (0.0, 2.0, 0.0), (1e-3, 1.0, -1e-3), (0.0, 1.0, 1e-6), (0.0, -1.0, 0.0), (1.0, 0.0, 0.0)]


def _walk_cases():
    rows = []
    for (c0, r0) in WALK_SPHERES.values():
        for (c1, r1) in WALK_SPHERES.values():
            for d in WALK_DIRECTIONS:
                for skip in (0.0, 1.0, 2.0):
                    rows.append((*c0, r0, *c1, r1, 0.0, 0.0, 0.0, *d, skip, 0.0))
    rows = np.array(rows, dtype=np.float32)
    # the same scenes seen from seeded origins a little off, and moved as a whole
    rng = np.random.default_rng(20261020)
    more = np.repeat(rows, 8, axis=0)
    jitter = (rng.uniform(-1.0, 1.0, (len(more), 3)) * 2.0 ** rng.integers(-40, -1, (len(more), 1))).astype(np.float32)
    more[:, 8:11] += jitter * (rng.integers(0, 2, (len(more), 1)) > 0)
    return np.concatenate([rows, more])


def test_the_shadow_arm_is_the_arm_with_the_full_test(hb):
    cases = _walk_cases()
    res = hb.selftest_pair_shadow_walk(cases)
    print("walk:", res)
    assert res["tested"] == len(cases) and res["mismatches"] == 0, res
    # the cold loop ran: for one sphere, for both, and with the other sphere's answer already in the state word
    assert res["asked"] > 0 and res["asked_both"] > 0 and res["asked_with_occluded"] > 0, res
    assert res["asked"] < res["tested"], res  # ... and lanes the signs settle ran next to them
    for skip, sphere in ((1.0, 0), (2.0, 1)):  # `skip` takes the one sphere that occludes out: then nothing does
        one = np.zeros((1, 16), dtype=np.float32)
        one[0, 4 * sphere:4 * sphere + 4] = (0.0, 3.0, 0.0, 1.0)
        one[0, 4 * (1 - sphere):4 * (1 - sphere) + 4] = (3.0, 3.0, 0.0, 1.0)
        one[0, 11:14] = (0.0, 1.0, 0.0)
        one[0, 14] = skip
        assert hb.selftest_pair_shadow_walk(one)["mismatches"] == 0
    with pytest.raises(hb.RtHipError):
        hb.selftest_pair_shadow_walk(cases, device=99)


def _pair_scene(ground_radius, ball_centre, ball_radius):
    """the shape of rtweekend1: a ground sphere whose top is at z = -0.5 under (0, 1), a second sphere, a lerp sky"""
    sc = scenes.SceneDescription()
    sc.sphere((0.0, 1.0, -0.5 - ground_radius), ground_radius, sc.lambertian(sc.solid((0.5, 0.5, 0.5)), 0.5))
    sc.sphere(ball_centre, ball_radius, sc.lambertian(sc.solid((0.7, 0.3, 0.3)), 0.5))
    sc.set_sky(sc.lerp((0.5, 0.7, 1.0), (1.0, 1.0, 1.0)), (16, 8))
    return sc


def _camera(origin, lookat):
    return dict(origin=origin, lookat=lookat, vup=(0.0, 0.0, 1.0), fov=70.0, aspect_ratio=CAMERA_16_9, aperture=0.0, focus_dist=1.0)


# name -> (scene, camera, whether the host must pick the two-sphere kernels for it)
SCENES = {
    "rtweekend1": (lambda: scenes.load_ssml("rtweekend1").scene, _camera((0.0, 0.0, 0.0), (0.0, 1.0, 0.0)), True),
    # every ray starts inside the ground sphere: c < 0 for it all along the path
    "camera inside the large sphere": (lambda: scenes.load_ssml("rtweekend1").scene, _camera((3.0, -1.0, -40.0), (0.0, 1.0, 0.0)), True),
    # radius above the predicate's 2^59.  Outside what the host hands the two-sphere kernels -- they need a radius whose reciprocal it
    # verified, [2^-20, 2^32], rt_api.cpp -- so these frames run the general kernel and none of the new code: the case only pins that
    # the host keeps declining such a scene.  The cold path such a radius would take is run by the two self-tests above: the
    # predicate's by test_the_sign_predicate..., the arm's loop by test_the_shadow_arm...
    "large radius 2^60": (lambda: _pair_scene(2.0 ** 60, (0.0, 1.0, 0.0), 0.5), _camera((0.0, 0.0, 0.0), (0.0, 1.0, 0.0)), False),
    # a sphere of radius 2^-20 on the ground where the camera looks: bounce and shadow rays start within a few radii of it
    "tiny sphere where rays start": (lambda: _pair_scene(100.0, (0.0, 1.0, -0.5 + 2.0 ** -20), 2.0 ** -20),
                                     _camera((0.0, 0.0, 0.0), (0.0, 1.0, -0.5)), True),
}


@pytest.fixture(scope="module")
def loaded(hb, O):
    out = {}
    for name, (make, cam, _) in SCENES.items():
        sc = make()
        general = hb.HipScene(sc, device=0)
        general.set_tuning(abi.RT_TUNE_FEATURE_SET, 0)
        out[name] = (hb.HipScene(sc, device=0), general, O.Scene(sc))
    return out


@pytest.mark.parametrize("split", [1, 4])
@pytest.mark.parametrize("name", sorted(SCENES))
def test_frames_keep_their_bits(hb, O, loaded, name, split):
    pair, general, cpu = loaded[name]
    _, params, wants_pair = SCENES[name]
    opts = abi.default_render_opts(W, H, SPP, method=abi.RT_METHOD_MIS, seed=23)
    opts.sample_split = split
    cam = hb.camera_new(**params)
    img, rays = pair.render(cam, opts)
    kernel = pair.last_launch_info()["kernel"]
    print(name, "split", split, "->", kernel)
    assert ("rt::FeatPair" in kernel) == wants_pair, (name, kernel)
    img_g, rays_g = general.render(cam, opts)
    assert "rt::Feat<false, false, false, false>" in general.last_launch_info()["kernel"], name
    ref, ref_rays = cpu.render(O.camera_new(**params), opts)
    assert_same_bits(img, img_g, f"{name} split={split}: against the general kernel", nan_equal=True)
    assert_same_bits(img, ref, f"{name} split={split}: against the oracle", nan_equal=True)
    assert rays == rays_g == ref_rays, (name, split, rays, rays_g, ref_rays)
