"""What the lens-AOV tests share: lens_cases' 24 x 13 frame, its three scenes and one with followed materials (a perfect mirror and a
glass sphere), the cameras, and the checker's channels, computed once per (scene, projection, aperture, chain, frame, stream) on the
CPU oracle and shared read-only.  test_lens_aov.py (CPU) shows on the checker alone that every comparison of test_gpu_lens_aov.py
tests something.  torch is never imported here."""
import functools

import numpy as np

import gpu_support
import lens_aov_checker as LA
import lens_cases as LN
import scenes

abi = scenes.abi
W, H = LN.W, LN.H
SEED, BEGIN, SPP = LN.SEED, LN.BEGIN, 3
MIRRORS = "mirror_and_glass"
SCENES = dict(LN.SCENES)
# (focused 1.5 units ahead: the orthographic view plane, which lies at the focus distance, is in front of the two spheres)
SCENES[MIRRORS] = lambda: (gpu_support.quality_scene(), dict(gpu_support.QUALITY_CAMERA, focus_dist=1.5))
CAMERAS = [(p, 0.0) for p in LN.PROJECTIONS] + [("perspective", LN.APERTURE)]  # the four projections, and the thin lens
CHAINS = (0, 8)
FISHEYE_220 = 220.0  # degrees: the rim looks 20 degrees behind the camera


@functools.lru_cache(maxsize=None)
def built(name):
    """(scene description, camera parameters, oracle scene), once per scene"""
    import oracle as O
    O.build()
    sc, cam_params = SCENES[name]()
    return sc, dict(cam_params), O.Scene(sc)


def followed_materials(name):
    """the Reflect (fuzz 0) and Refract materials of a scene: what a chain with the default fuzz_limit follows"""
    return [m for m in built(name)[0].materials
            if m.type == abi.RT_MAT_REFRACT or (m.type == abi.RT_MAT_REFLECT and np.float32(m.param) <= 0)]


def camera(hb, name, projection, aperture=0.0, **params):
    """the abi.LensCamera of a scene's own camera with another aperture, projection and, by keyword, other parameters"""
    p = dict(built(name)[1], aperture=aperture, **params)
    return hb.lens_camera_new(**p, projection=projection)


def opts(spp=SPP, w=W, h=H, seed=SEED, begin=BEGIN):
    o = abi.default_render_opts(w, h, spp, seed=seed)
    o.sample_begin = begin
    return o


def _hb():
    import importlib
    return importlib.import_module("raytracing-rust_amd.hip_backend")


@functools.lru_cache(maxsize=None)
def _reference(name, projection, aperture, max_chain, w, h, spp, seed, begin, cam_items):
    sc, _, cpu = built(name)
    cam = camera(_hb(), name, projection, aperture, **dict(cam_items))
    flat, inside = LA.aovs(sc, cpu, cam, w, h, spp, seed=seed, sample_begin=begin, max_chain=max_chain, return_inside=True)
    out = LA.framed(flat, w, h)
    for a in (*out.values(), inside):
        a.setflags(write=False)
    return out, inside.reshape(spp, h, w)


def reference(name, projection, aperture=0.0, max_chain=0, w=W, h=H, spp=SPP, seed=SEED, begin=BEGIN, **cam_params):
    """({channel: frame}, inside (spp, h, w) bool) of the checker; cam_params: camera parameters other than the scene's own"""
    return _reference(name, projection, aperture, max_chain, w, h, spp, seed, begin, tuple(sorted(cam_params.items())))
