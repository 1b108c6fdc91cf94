"""The two-sphere kernels' primary walk takes the terms of its box and sphere tests that depend on the camera's origin and the scene
alone (csrc/rt_types.h DevPairPrimary: 28 values) from the host, which forms them once per render.  Frames must keep their bits --
against the oracle and against the general spheres-only kernel, which never sees the block -- for origins that stress those terms;
the host's block must be the device's arithmetic word for word; a camera the block cannot serve must take the kernels' own walk."""
import numpy as np
import pytest

import scenes
from gpu_support import CAMERA_16_9, abi, assert_same_bits

pytestmark = pytest.mark.gpu

W, H, SPP = 64, 48, 8


def _second_scene():
    """the shape of rtweekend1 (a ground sphere, a ball, a lerp sky) with other centres, radii, colours and a sampled sky"""
    sc = scenes.SceneDescription()
    sc.sphere((0.5, 2.0, -50.25), 50.0, sc.lambertian(sc.solid((0.8, 0.3, 0.2)), 0.9))
    sc.sphere((0.25, 1.5, 0.125), 0.375, sc.lambertian(sc.solid((0.1, 0.4, 0.9)), 0.6))
    sc.set_sky(sc.lerp((0.5, 0.7, 1.0), (1.0, 1.0, 1.0)), (16, 8))
    return sc


# name -> (scene, ground (centre, radius), ball (centre, radius))
SCENES = {
    "rtweekend1": (lambda: scenes.load_ssml("rtweekend1").scene, ((0.0, 1.0, -100.5), 100.0), ((0.0, 1.0, 0.0), 0.5)),
    "second": (_second_scene, ((0.5, 2.0, -50.25), 50.0), ((0.25, 1.5, 0.125), 0.375)),
}


def _origins(ground, ball):
    """(what, origin) -- the origins that stress the hoisted operands; every camera looks at the ball (from its centre: along +y)"""
    (gc, gr), (bc, br) = ground, ball
    return [
        ("as shipped", (0.0, 0.0, 0.0)),  # centre - 0 must keep centre's bits, signed zeros included
        ("large and tiny components", (1e3, -3e-5, 7.25)),
        ("inside the large sphere", (gc[0] + 3.0, gc[1] - 2.0, gc[2] + 0.6 * gr)),
        ("on a face of the ball's box", (bc[0] + 0.25 * br, bc[1] - br, bc[2] + 0.5 * br)),  # a slab difference is +-0
        ("at the ball's centre", bc),  # deltap = 0
    ]


def _camera_params(origin, ball):
    bc = ball[0]
    lookat = bc if tuple(origin) != tuple(bc) else (bc[0], bc[1] + 1.0, bc[2])
    return dict(origin=origin, lookat=lookat, vup=(0.0, 0.0, 1.0), fov=70.0, aspect_ratio=CAMERA_16_9, aperture=0.0, focus_dist=1.0)


def _opts(split):
    opts = abi.default_render_opts(W, H, SPP, method=abi.RT_METHOD_MIS, seed=17)
    opts.sample_split = split
    return opts


@pytest.fixture(scope="module")
def loaded(hb, O):
    """per scene: the scene as the pair kernels take it, the same scene forced to the general kernel, the oracle's"""
    out = {}
    for name, (make, ground, ball) in SCENES.items():
        sc = make()
        general = hb.HipScene(sc, device=0)
        general.set_tuning(abi.RT_TUNE_FEATURE_SET, 0)
        out[name] = (hb.HipScene(sc, device=0), general, O.Scene(sc), ground, ball)
    return out


@pytest.mark.parametrize("split", [1, 4])
@pytest.mark.parametrize("name", sorted(SCENES))
def test_frames_keep_their_bits(hb, O, loaded, name, split):
    pair, general, cpu, ground, ball = loaded[name]
    for what, origin in _origins(ground, ball):
        label = f"{name} split={split} origin {what}"
        params = _camera_params(origin, ball)
        cam, opts = hb.camera_new(**params), _opts(split)
        img, rays = pair.render(cam, opts)
        info = pair.last_launch_info()
        assert "rt::FeatPair" in info["kernel"], (label, info)
        assert hb.selftest_pair_primary(pair, origin) == (True, 0), label  # ... and its walk did take the block
        img_g, rays_g = general.render(cam, opts)
        assert "rt::Feat<false, false, false, false>" in general.last_launch_info()["kernel"], label
        ref, ref_rays = cpu.render(O.camera_new(**params), opts)
        assert_same_bits(img, img_g, label + ": pair kernel against the general kernel", nan_equal=True)
        assert_same_bits(img, ref, label + ": pair kernel against the oracle", nan_equal=True)
        assert rays == rays_g == ref_rays, (label, rays, rays_g, ref_rays)


@pytest.mark.parametrize("name", sorted(SCENES))
def test_host_block_is_the_devices_arithmetic(hb, loaded, name):
    pair, _, _, ground, ball = loaded[name]
    rng = np.random.default_rng(20240607)
    origins = [o for _, o in _origins(ground, ball)]
    # seeded random origins over twelve decades of magnitude, both signs; a few with zero components of either sign
    mag = 10.0 ** rng.uniform(-6.0, 6.0, size=(300, 3))
    rnd = (mag * rng.choice([-1.0, 1.0], size=(300, 3))).astype(np.float32)
    rnd[::50, 0] = 0.0
    rnd[25::50, 2] = -0.0
    origins += [tuple(float(x) for x in o) for o in rnd]
    for origin in origins:
        valid, bad = hb.selftest_pair_primary(pair, origin)
        assert valid and bad == 0, (name, origin, valid, bad)


@pytest.mark.parametrize("bad_component", [float("inf"), float("nan")])
def test_a_camera_the_block_cannot_serve_takes_the_kernels_own_walk(hb, loaded, bad_component):
    pair, general, _, ground, ball = loaded["rtweekend1"]
    origin = (0.0, bad_component, 0.0)
    valid, bad = hb.selftest_pair_primary(pair, origin)
    assert not valid and bad == 0  # (the flag is one of the compared words; NaN terms compare equal)
    cam, opts = hb.camera_new(**_camera_params(origin, ball)), _opts(1)
    img, rays = pair.render(cam, opts)
    assert "rt::FeatPair" in pair.last_launch_info()["kernel"]
    img_g, rays_g = general.render(cam, opts)
    assert_same_bits(img, img_g, f"origin y = {bad_component}: pair kernel against the general kernel", nan_equal=True)
    assert rays == rays_g
