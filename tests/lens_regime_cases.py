"""The inputs the lens render (rt_render_lens, csrc/rt_lens.hip lens_kernel) treats differently, as ONE table: test_lens_regime_cases.py
(CPU) shows on the oracle and the checker alone that every entry tests something, test_gpu_lens_regimes.py runs the kernel on it.
lens_kernel shares the per-lane integrator with rt_radiance and rt_render_tiles and restates everything around it: the 64-bit
assembly of seed and first sample, a second stream at 2^63 + pixel, the chunk rule with the whole-pixel path, the padding writes of
edge tiles, the fold record behind the stacks, its own copy of max_depth and rr_threshold and a per-lane ray counter.  Seven groups:

  sky/<case>/<scene>/<method>[/fisheye]  every sky of sky_cases.RENDER_CASES on radiance_cases' three scenes under MIS (the 2^24-cell
                                         skies: the floor only), and under NAIVE on the floor, whose reference is the oracle on the
                                         same texture with sampler_res (0, 0).  A panorama from a LEVEL camera (`up` is the sky's
                                         pole), so both polar rows of the table are in frame; the floor also through the fisheye
  arm/<shape>/<method>/s<S>              one scene per arm of sample_lights (radiance_cases.SHAPES), through the thin lens
  uneven/<method>/<spp>_<S>              tiles_cases.UNEVEN: chunk c = passes [floor(c spp / S), floor((c + 1) spp / S)), fisheye
  stream/<method>/s<S>/<seed>/<begin>    seeds and first samples as 64-bit values, through the thin lens (four camera draws)
  depth/<scene>/<method>/d<D>/r<R>       max_depth 1 (the MIS prologue's own exit), 2 and 8, rr_threshold 0 and 3
  ragged/<w>x<h>/<projection>/s<S>       frames smaller than a tile (2 x 2: 60 of the 64 lanes are padding) and one with no padding
  camera/...                             the fisheye past 180 degrees and on frames far from square, a lens wider than the distance
                                         to the ground, a panorama and an orthographic frame whose vup is no axis

An entry is a scene, a camera and render options; its reference is computed once on the oracle through lens_checker (one call of
the oracle's counted fixed-ray integrator per sample) and shared read-only: the frame, the chunk sums in rt_render_lens' tiled
layout, the inside-sample count and the ray count.  Pass images are cached per (scene, camera, options, sample index), so entries
that differ in the fold alone share them.  torch is never imported here."""
import functools

import numpy as np

import lens_cases as LN
import lens_checker as LC
import radiance_cases as RC
import sky_cases as SK
import tiles_cases as TC

abi = TC.abi
F32 = np.float32
NAIVE, MIS = RC.NAIVE, RC.MIS
METHODS = RC.METHODS
SEED, BEGIN = TC.SEED, TC.BEGIN
MASK64, LOW = TC.MASK64, TC.LOW
MATERIALS = TC.MATERIALS
APERTURE = LN.APERTURE


class Entry:
    """scene: what the GPU renders, ref_scene: what the oracle integrates on (the same unless stated); projection: a name of
    abi.PROJECTIONS; aperture and camera: what replaces the scene's own camera parameters; groups: the values of
    RT_TUNE_RADIANCE_GROUPS the entry runs under (0: the automatic grid)"""

    def __init__(self, scene, method, projection, w, h, spp, split, *, aperture=0.0, camera=None, seed=SEED, begin=BEGIN, max_depth=50,
                 rr=3, groups=(0,), ref_scene=None):
        self.scene, self.ref_scene, self.method, self.projection = scene, ref_scene or scene, method, projection
        self.w, self.h, self.spp, self.split = w, h, spp, split
        self.aperture, self.camera = float(aperture), tuple(sorted((camera or {}).items()))
        self.seed, self.begin, self.max_depth, self.rr, self.groups = seed, begin, max_depth, rr, groups

    def n_tiles(self):
        return ((self.w + 7) // 8) * ((self.h + 7) // 8)


def _m(method):
    return "mis" if method == MIS else "naive"


def level(cam_params):
    """the camera parameters with lookat raised to the origin's height: for the z-up cameras of the sky scenes `up` is then (0, 0, 1),
    the pole of the sky's table, and the rows of a panorama are the rows of the table"""
    assert tuple(cam_params["vup"]) == (0.0, 0.0, 1.0)
    o, l = cam_params["origin"], cam_params["lookat"]
    return dict(lookat=(l[0], l[1], o[2]))


ENTRIES = {}

# ---- 1. skies: 16 x 16 x 4 at S = 2 (the 2^24-cell skies 8 x 16 x 2) ----
for _case in SK.RENDER_CASES:
    _shape = (8, 16, 2, 2) if _case in SK.HUGE else (16, 16, 4, 2)
    for _scene in RC.sky_scenes_of(_case):
        ENTRIES[f"sky/{_case}/{_scene}/mis"] = Entry(f"sky/{_case}/{_scene}", MIS, "equirect", *_shape, camera=level(RC.SKY_SCENES[_scene]()[1]))
    _floor = level(RC.SKY_SCENES["floor"]()[1])
    ENTRIES[f"sky/{_case}/floor/naive"] = Entry(f"sky/{_case}/floor", NAIVE, "equirect", *_shape, camera=_floor, ref_scene=f"unsampled/{_case}/floor")
    ENTRIES[f"sky/{_case}/floor/mis/fisheye"] = Entry(f"sky/{_case}/floor", MIS, "fisheye", *_shape, camera=_floor)
    ENTRIES[f"sky/{_case}/floor/naive/fisheye"] = Entry(f"sky/{_case}/floor", NAIVE, "fisheye", *_shape, camera=_floor,
                                                        ref_scene=f"unsampled/{_case}/floor")
SKIES = tuple(k for k in ENTRIES if k.startswith("sky/"))

# ---- 2. the four arms of sample_lights, through the thin lens ----
for _name in RC.SHAPES:
    for _method in METHODS:
        for _split in (1, 2):
            ENTRIES[f"arm/{_name}/{_m(_method)}/s{_split}"] = Entry(f"shape/{_name}", _method, "perspective", 16, 16, 4, _split, aperture=APERTURE)
ARMS = tuple(k for k in ENTRIES if k.startswith("arm/"))

# ---- 3. chunks of unequal length.  Four tiles: without a chunk buffer four items, with one twelve at S = 3, so under
# RT_TUNE_RADIANCE_GROUPS = 1 (four waves) the waves take a second and a third CHUNK item and, 256 pixels on 256 lanes with the
# fisheye's black corners finishing early, lanes refill inside WHOLE-PIXEL items as well ----
UNEVEN = TC.UNEVEN
UNEVEN_ONE_GROUP = TC.UNEVEN_ONE_GROUP
for _method in METHODS:
    for _spp, _split in UNEVEN:
        ENTRIES[f"uneven/{_m(_method)}/{_spp}_{_split}"] = Entry(MATERIALS, _method, "fisheye", 16, 16, _spp, _split,
                                                               groups=(0, 1) if (_spp, _split) == UNEVEN_ONE_GROUP else (0,))
UNEVENS = tuple(k for k in ENTRIES if k.startswith("uneven/"))

# ---- 4. 64-bit seeds and first samples ----
STREAM_SPP = TC.STREAM_SPP
STREAM_BEGINS = TC.STREAM_BEGINS
for _method in METHODS:
    for _split in (1, 2):
        for _seed in RC.SEEDS:
            for _begin in STREAM_BEGINS:
                ENTRIES[f"stream/{_m(_method)}/s{_split}/{_seed:#x}/{_begin:#x}"] = Entry(MATERIALS, _method, "perspective", 16, 8, STREAM_SPP, _split,
                                                                                        aperture=APERTURE, seed=_seed, begin=_begin)
STREAMS = tuple(k for k in ENTRIES if k.startswith("stream/"))

# ---- 5. depth and roulette ----
DEPTH_SCENES = TC.DEPTH_SCENES
DEPTHS, ROULETTES = TC.DEPTHS, TC.ROULETTES
# a panorama of 16 x 8 from all_materials' own camera, six units away, sees its spheres in a handful of samples, and no path of
# them is longer than two vertices: max_depth 2 and 8 would be the same frame.  The panorama stands between the spheres and the box
DEPTH_CAMERAS = {MATERIALS: dict(origin=(0.55, 0.7, 0.9)), "rtweekend1": None}
for _scene in DEPTH_SCENES:
    for _method in METHODS:
        for _d in DEPTHS:
            for _r in ROULETTES:
                ENTRIES[f"depth/{_scene}/{_m(_method)}/d{_d}/r{_r}"] = Entry(_scene, _method, "equirect", 16, 8, 4, 2, camera=DEPTH_CAMERAS[_scene],
                                                                             max_depth=_d, rr=_r)
DEPTH_KEYS = tuple(k for k in ENTRIES if k.startswith("depth/"))

# ---- 6. ragged frames: every size under two projections (2 x 2, the smallest frame the API accepts, where width - 1 = 1 divides
# the jitter: under all four); 16 x 8 has no padding lane at all ----
RAGGED = {(2, 2): ("perspective", "orthographic", "fisheye", "equirect"), (5, 11): ("fisheye", "equirect"),
          (9, 8): ("perspective", "orthographic"), (16, 8): ("fisheye", "perspective")}
for (_w, _h), _projections in RAGGED.items():
    for _p in _projections:
        for _split in (1, 2):
            ENTRIES[f"ragged/{_w}x{_h}/{_p}/s{_split}"] = Entry(MATERIALS, MIS, _p, _w, _h, 4, _split, aperture=APERTURE if _p == "perspective" else 0.0)
RAGGEDS = tuple(k for k in ENTRIES if k.startswith("ragged/"))

# ---- 7. what only this entry has ----
WIDE_FOVS = (220.0, 360.0)
# all_materials' camera stands 1.5 above the ground sphere (primitive 0: centre (0, -1000, 0), radius 1000): a lens of radius 4
# reaches below it, so some origins start INSIDE that sphere.  focus_dist 4: neither 1 nor the scene's 10
BIG_LENS = dict(aperture=8.0, camera=dict(focus_dist=4.0))
GROUND_CENTRE, GROUND_RADIUS = (0.0, -1000.0, 0.0), 1000.0
TILTED_VUP = dict(vup=(0.3, 1.0, 0.2))
for _method in METHODS:
    for _fov in WIDE_FOVS:
        ENTRIES[f"camera/fisheye{_fov:.0f}/{_m(_method)}"] = Entry(MATERIALS, _method, "fisheye", 16, 16, 4, 2, camera=dict(fov=_fov))
    # 24 x 8: b is scaled by 7 / 23, the circle is cut by the frame's top and bottom and the last pixel column (s >= 1) is black;
    # 8 x 24: by 23 / 7, whole pixel rows are black
    ENTRIES[f"camera/fisheye_24x8/{_m(_method)}"] = Entry(MATERIALS, _method, "fisheye", 24, 8, 4, 2)
    ENTRIES[f"camera/fisheye_8x24/{_m(_method)}"] = Entry(MATERIALS, _method, "fisheye", 8, 24, 4, 2)
    ENTRIES[f"camera/big_lens/{_m(_method)}"] = Entry(MATERIALS, _method, "perspective", 16, 16, 4, 2, aperture=BIG_LENS["aperture"],
                                                      camera=BIG_LENS["camera"])
    for _p in ("equirect", "orthographic"):
        ENTRIES[f"camera/tilted_{_p}/{_m(_method)}"] = Entry(MATERIALS, _method, _p, 16, 16, 4, 2, camera=TILTED_VUP)
CAMERAS = tuple(k for k in ENTRIES if k.startswith("camera/"))

GROUPS = {"sky": SKIES, "arm": ARMS, "uneven": UNEVENS, "stream": STREAMS, "depth": DEPTH_KEYS, "ragged": RAGGEDS, "camera": CAMERAS}


# ---- scenes, cameras, passes, references: once each ----
built = TC.built  # (scene description, camera parameters, oracle scene, oracle camera); the 2^24-cell oracle scenes once per process


@functools.lru_cache(maxsize=None)
def _camera(scene, projection, aperture, camera):
    import importlib
    hb = importlib.import_module("raytracing-rust_amd.hip_backend")
    return hb.lens_camera_new(**dict(built(scene)[1], aperture=aperture, **dict(camera)), projection=projection)  # (runs on the host)


def camera(key):
    """the entry's abi.LensCamera: the GPU scene's own camera parameters with the entry's aperture, overrides and projection"""
    e = ENTRIES[key]
    return _camera(e.scene, e.projection, e.aperture, e.camera)


def opts(key):
    e = ENTRIES[key]
    return TC.make_opts(e.method, e.w, e.h, e.spp, e.split, e.seed, e.begin, e.max_depth, e.rr)


@functools.lru_cache(maxsize=None)
def single_pass(ref_scene, cam_scene, method, projection, aperture, camera, w, h, seed, index, max_depth=50, rr=3):
    """((h, w, 3) f32, (h, w) bool inside, (h, w) uint64 rays): the checker's pass at sample index `index` of the camera of
    `cam_scene` over the oracle scene `ref_scene`"""
    out = LC.pass_image(built(ref_scene)[2], _camera(cam_scene, projection, aperture, camera), w, h, method, seed, index, max_depth, rr,
                        return_rays=True)
    for a in out:
        a.setflags(write=False)
    return out


def pass_indices(begin, spp):
    return TC.pass_indices(begin, spp)


def passes(key, indices=None, seed=None, scene=None, method=None):
    """((spp, h, w, 3) f32, (spp, h, w) bool, (spp, h, w) uint64): the entry's passes, or those at other sample indices / another
    seed / on another oracle scene / under the other integrator"""
    e = ENTRIES[key]
    indices = pass_indices(e.begin, e.spp) if indices is None else indices
    got = [single_pass(scene or e.ref_scene, e.scene, e.method if method is None else method, e.projection, e.aperture, e.camera, e.w, e.h,
                       e.seed if seed is None else seed, i, e.max_depth, e.rr) for i in indices]
    return tuple(np.stack([g[i] for g in got]) for i in range(3))


def fold(pass_images, split, bounds=None):
    """what rt_render_lens writes from these passes (tiles_cases.fold: the running mean, or the chunk sums under `bounds`)"""
    return TC.fold(pass_images, split, bounds)


class Reference:
    """frame (h, w, 3) f32; sums (S, h, w, 3) f32 or None; tiled (S, tiles, 8, 8, 3) f32 or None; inside: samples inside the image
    circle; rays: rays_shot; has_nan: the frame holds a NaN -- the one case in which a comparison may treat NaNs as equal"""

    def __init__(self, frame, sums, inside, rays, w, h):
        self.frame, self.sums, self.inside, self.rays = frame, sums, inside, rays
        self.tiled = None if sums is None else LC.tiled(sums, w, h)
        self.has_nan = bool(np.isnan(frame).any())
        for a in (self.frame, self.sums, self.tiled):
            if a is not None:
                a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def reference(key):
    e = ENTRIES[key]
    frame, sums, inside, rays = LC.frame(None, None, opts(key), e.split, passes=passes(key), return_rays=True)
    return Reference(frame, sums, inside, rays, e.w, e.h)


def padding(w, h):
    """(tiles, 8, 8) bool: the padding lanes of the tiled layout"""
    pad = np.ones((1, h, w, 3), F32)
    return LC.tiled(pad, w, h)[0, ..., 0] == 0


def directions(key, index=None):
    """(origins, directions, inside) of the checker for the entry's pass at sample index `index` (default: its first)"""
    e = ENTRIES[key]
    return LC.rays(camera(key), e.w, e.h, e.seed, e.begin if index is None else index)
