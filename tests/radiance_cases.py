"""The inputs the radiance kernels (rt_radiance, csrc/rt_radiance.hip) treat differently, as ONE table: test_radiance_cases.py (CPU)
shows on the oracle alone that every entry tests something, test_gpu_radiance_regimes.py runs the kernels on it.  Four groups:

  tree/<case>          every tree of hard_tree_cases.CASES from the case's own camera: the first 64 pixel-centre rays of a 16 x 9
                       grid and up to 64 surface probes, K = 2
  sky/<case>/<scene>   every sky of sky_cases.RENDER_CASES on three scenes: `floor` and `spheres` (no emissive primitive: under
                       MIS every light sample is a sky sample) and `lit_spheres` (ten emissive spheres and the sky share the
                       choice: light_choices = 11 in sample_lights and in pdf_from_index); 64 pixel centres
                       and 64 probes, K = 2.  The two 2^24-cell skies: the floor only, 32 + 32 rays, K = 1 (the oracle scene of
                       such a sky is built once per process: that build is the cost, not the query)
  shape/<name>         one scene per arm of sample_lights (mis.rs:135-157): (emissive primitives, sky samplable)
  streams              `all_materials`, 257 rays, per-ray 64-bit streams, 64-bit seeds and first samples

An entry is (scene, camera parameters) and a ray count; its references are radiance_checker.prefix_means of the oracle, computed
once per (entry, method, seed, first sample) and shared read-only.  torch is never imported here."""
import functools

import numpy as np

import hard_tree_cases as HT
import radiance_checker as R
import scenes
import sky_cases as SK

abi = scenes.abi
F32 = np.float32
NAIVE, MIS = abi.RT_METHOD_NAIVE, abi.RT_METHOD_MIS
METHODS = (NAIVE, MIS)
SEED = 5
GW, GH = 16, 9        # the grid of pixel centres
PROBE_GRID = (64, 36)  # the probes start on hits of this finer grid of the same camera, spread evenly over them
PROBE_SEED = 11


class Entry:
    """build() -> (SceneDescription, camera parameters) or hard_tree_cases.built's 4-tuple; centres: how many pixel-centre rays
    (first: the first of the grid in row-major order, else spread evenly over the grid); probes: at most how many surface probes;
    k: samples a ray in the oracle comparison"""

    def __init__(self, build, centres, probes, k, first=False):
        self.build, self.centres, self.probes, self.k, self.first = build, centres, probes, k, first


def _floor():
    return SK.RENDER_SCENES["floor"]()


def _spheres():
    return SK.RENDER_SCENES["spheres"]()


def _lit_spheres_under():
    return scenes.random_spheres(30, seed=5, emissive_every=3), scenes.TINY_TREE_CAMERA


# `spheres` is sky_cases' render scene: it has NO emissive primitive either (emissive_every = 0), so `lit_spheres`, the same
# generator and seed with every third sphere a light, is the scene on which the primitives and the sky share the choice
SKY_SCENES = {"floor": _floor, "spheres": _spheres, "lit_spheres": _lit_spheres_under}


def sky_scenes_of(case):
    return ("floor",) if case in SK.HUGE else tuple(SKY_SCENES)


def _with_sky(scene, case):
    def build():
        sc, cam = SKY_SCENES[scene]()
        return SK.with_sky(sc, case), cam
    return build


def unsampled_scene(case, scene):
    """the scene of sky/<case>/<scene> with sampler_res (0, 0): what a NAIVE query of the entry must equal, bit for bit"""
    sc, _ = SKY_SCENES[scene]()
    return SK.unsampled(sc, case)


# sample_lights' four arms: name -> ((emissive primitives present, sky samplable), build)
def _lit_spheres(**kw):
    return lambda: (scenes.random_spheres(30, emissive_every=3, **kw), scenes.TINY_TREE_CAMERA)


SHAPES = {
    "sky_alone": ((False, True), _with_sky("floor", "control")),
    "nothing": ((False, False), lambda: (SK.unsampled(_floor()[0], "control"), SK.FLOOR_CAMERA)),
    "primitives_alone": ((True, False), _lit_spheres(sampler_res=(0, 0))),
    "primitives_and_sky": ((True, True), _lit_spheres()),
}
SHAPE_K = 4

ENTRIES = {}
for _name in HT.CASES:
    ENTRIES[f"tree/{_name}"] = Entry(functools.partial(HT.built, _name), 64, 64, 2, first=True)
for _case in SK.RENDER_CASES:
    for _scene in sky_scenes_of(_case):
        _huge = _case in SK.HUGE
        ENTRIES[f"sky/{_case}/{_scene}"] = Entry(_with_sky(_scene, _case), 32 if _huge else 64, 32 if _huge else 64, 1 if _huge else 2)
for _name, (_, _build) in SHAPES.items():
    ENTRIES[f"shape/{_name}"] = Entry(_build, 64, 64, SHAPE_K)
ENTRIES["streams"] = Entry(lambda: (scenes.all_materials(), scenes.ALL_MATERIALS_CAMERA), GW * GH, 257 - GW * GH, 3)

TREES = tuple(k for k in ENTRIES if k.startswith("tree/"))
SKIES = tuple(k for k in ENTRIES if k.startswith("sky/"))

# ---- streams, seeds and first samples as 64-bit values ----
STREAM_VALUES = (0, 1, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, (1 << 40) + 3, 1 << 63, (1 << 64) - 1)
SEEDS = (5, (1 << 32) + 5, (1 << 63) + 5)
# with K = 3: 2^32 - 1 carries into the high word at the second sample, 2^64 - 2 wraps to 0 at the third
SAMPLE_BEGINS = (0, (1 << 32) - 1, 1 << 32, (1 << 64) - 2)
STREAM_K = 3
LOW = (1 << 32) - 1


@functools.lru_cache(maxsize=None)
def streams():
    """[257] u64, drawn once: every value of STREAM_VALUES on at least 32 rays"""
    n = ENTRIES["streams"].centres + ENTRIES["streams"].probes
    pick = np.random.default_rng(7).permutation(n) % len(STREAM_VALUES)
    out = np.array(STREAM_VALUES, dtype=np.uint64)[pick]
    out.setflags(write=False)
    return out


def low_words(values):
    return np.asarray(values, dtype=np.uint64) & np.uint64(LOW)


# ---- scenes, rays, references: once each ----
@functools.lru_cache(maxsize=None)
def built(key):
    """(scene description, camera parameters, oracle scene, oracle camera), once per entry"""
    import oracle as O
    O.build()
    r = ENTRIES[key].build()
    if len(r) == 4:
        return r
    sc, cam_params = r
    return sc, cam_params, O.Scene(sc), O.camera_new(**cam_params)


@functools.lru_cache(maxsize=None)
def rays(key):
    """(origins, directions, number of pixel-centre rays among them): the entry's pixel centres, then its probes"""
    e = ENTRIES[key]
    _, _, cpu, cam = built(key)
    o, d = R.pixel_centre_rays(cam, GW, GH)
    pick = np.arange(e.centres) if e.first else (np.arange(e.centres) * (GW * GH)) // e.centres
    o, d = o[pick], d[pick]
    po, pd = R.surface_probes(cpu, *R.pixel_centre_rays(cam, *PROBE_GRID), seed=PROBE_SEED)
    m = min(e.probes, len(po))
    spread = (np.arange(m) * len(po)) // max(m, 1)
    o = np.ascontiguousarray(np.concatenate([o, po[spread]]))
    d = np.ascontiguousarray(np.concatenate([d, pd[spread]]))
    o.setflags(write=False)
    d.setflags(write=False)
    return o, d, len(pick)


def repeated(key, n):
    """n rays: the entry's rays over and over"""
    o, d, _ = rays(key)
    idx = np.arange(n) % len(o)
    return o[idx], d[idx]


def compute(key, method, k, seed=SEED, per_ray_streams=None, sample_begin=0, n=None):
    """[rays, k, 3] f64 prefix means, computed now"""
    _, _, cpu, _ = built(key)
    o, d = rays(key)[:2] if n is None else repeated(key, n)
    return R.prefix_means(cpu, o, d, method, k, seed=seed, streams=per_ray_streams, sample_begin=sample_begin)


@functools.lru_cache(maxsize=None)
def reference(key, method, n=None):
    """the entry's reference on stream 0 from sample 0: [rays, k, 3] f64"""
    r = compute(key, method, ENTRIES[key].k, n=n)
    r.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def stream_reference(method, seed, sample_begin, k=STREAM_K):
    """the `streams` entry at (seed, streams()[i], sample_begin + j mod 2^64), j < k: [257, k, 3] f64 prefix means"""
    r = compute("streams", method, k, seed=seed, per_ray_streams=streams(), sample_begin=sample_begin)
    r.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def stream_sample(method, seed, index, low_streams=False):
    """one sample of the `streams` entry at (seed, streams()[i], index): [257, 3] f64, each an f32 widened; low_streams: every
    stream cut to its low 32 bits.  What a kernel that drops a high word would compute is this at the cut seed / index."""
    r = compute("streams", method, 1, seed=seed, per_ray_streams=low_words(streams()) if low_streams else streams(), sample_begin=index)[:, 0]
    r.setflags(write=False)
    return r


def sample_indices(sample_begin, k=STREAM_K):
    """sample_begin + j in 64-bit arithmetic that wraps: rt_radiance's rule (include/rt_hip.h) and the oracle's"""
    return [(sample_begin + j) & ((1 << 64) - 1) for j in range(k)]


def four_wave_lds_bytes(stack_depth):
    """csrc/rt_types.h four_wave_stack_lds_bytes: four waves x depth entries x 64 lanes x 4 B"""
    return 4 * stack_depth * 64 * 4
