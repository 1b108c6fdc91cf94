"""What the lens-camera tests share: the frame, the scenes and cameras, and the checker's pass images, computed once per (scene,
method, projection, aperture) on the CPU oracle and shared read-only.  test_lens.py (CPU) shows on the oracle alone that every
comparison of test_gpu_lens.py tests something.  torch is never imported here."""
import functools

import numpy as np

import lens_checker as LC
import scenes
from gpu_support import ssml_scene

abi = scenes.abi
F32 = np.float32
W, H = 24, 13  # edge tiles in both directions; 312 pixels: more than one 256-lane workgroup
SEED, BEGIN = 7, 5
MAX_SPP = 7  # the passes BEGIN .. BEGIN + 6 cover (spp, S) = (4, 1), (4, 2) and (7, 3)
FOLDS = ((4, 1), (4, 2), (7, 3))
METHODS = (abi.RT_METHOD_NAIVE, abi.RT_METHOD_MIS)
PROJECTIONS = ("perspective", "orthographic", "fisheye", "equirect")
APERTURE = 0.5  # the lens of the thin-lens cases (radius 0.25 scene units)
SCENES = {
    "all_materials": lambda: (scenes.all_materials(), scenes.ALL_MATERIALS_CAMERA),
    "overshadowed": lambda: ssml_scene("overshadowed"),  # emissive primitives: sample_lights' check_hit_index arm
    "rtweekend1": lambda: ssml_scene("rtweekend1"),      # a sampled sky
}
# rtweekend1 from above its small sphere, looking straight up: every ray leaves into the sky (not a panorama's: it looks down too)
SKY_ONLY_PROJECTIONS = ("perspective", "orthographic", "fisheye")
SKY_ONLY_CAMERA = dict(origin=(0.0, 1.0, 2.0), lookat=(0.0, 1.0, 10.0), vup=(0.0, 1.0, 0.0), fov=40.0,
                       aspect_ratio=float(F32(16.0) / F32(9.0)), aperture=0.0, focus_dist=1.0)


@functools.lru_cache(maxsize=None)
def built(name):
    """(scene description, camera parameters, oracle scene), once per scene"""
    import oracle as O
    O.build()
    sc, cam_params = SCENES[name]()
    return sc, dict(cam_params), O.Scene(sc)


def camera(hb, name, projection, aperture=0.0, params=None):
    """the abi.LensCamera of a scene's own camera with another aperture and projection (rt_lens_camera_new runs on the host)"""
    p = dict(built(name)[1] if params is None else params, aperture=aperture)
    return hb.lens_camera_new(**p, projection=projection)


def opts(method, spp, split, w=W, h=H, seed=SEED, begin=BEGIN):
    o = abi.default_render_opts(w, h, spp, method=method, seed=seed)
    o.sample_begin = begin
    o.sample_split = split
    return o


@functools.lru_cache(maxsize=None)
def _passes(name, method, projection, aperture, sky_only):
    import importlib
    hb = importlib.import_module("raytracing-rust_amd.hip_backend")
    cam = camera(hb, name, projection, aperture, SKY_ONLY_CAMERA if sky_only else None)
    got = [LC.pass_image(built(name)[2], cam, W, H, method, SEED, BEGIN + k, return_rays=True) for k in range(MAX_SPP)]
    out = tuple(np.stack([g[i] for g in got]) for i in range(3))
    for a in out:
        a.setflags(write=False)
    return out


def passes(name, method, projection, aperture=0.0, sky_only=False):
    """((MAX_SPP, H, W, 3) f32, (MAX_SPP, H, W) bool): the checker's passes BEGIN .. BEGIN + MAX_SPP - 1 and their inside masks"""
    return _passes(name, method, projection, aperture, sky_only)[:2]


def reference(name, method, projection, spp, split, aperture=0.0, sky_only=False):
    """(frame, chunk sums (S, H, W, 3) or None, inside samples) of the first `spp` passes"""
    img, inside = passes(name, method, projection, aperture, sky_only)
    frame, sums = LC.fold(img[:spp], split)
    return frame, sums, int(inside[:spp].sum())


def rays_shot(name, method, projection, spp, aperture=0.0, sky_only=False):
    """rt_render_lens' rays_shot for the first `spp` passes: the oracle integrator's ray count of every sample, summed"""
    return int(_passes(name, method, projection, aperture, sky_only)[2][:spp].sum())
