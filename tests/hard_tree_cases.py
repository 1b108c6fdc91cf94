"""The trees built to break walks, as ONE table for the four tile kernels (rt_render_aov, rt_render_aov_chain, rt_render_matte,
rt_render_ao): test_hard_trees.py (CPU) shows that every case tests something, test_gpu_hard_trees.py runs the kernels on it.
Each entry is (scene, camera parameters) and a finite AO radius; the frame, the passes and the AO rays are the same everywhere.
The references come from the four checkers over the oracle's check_hit, computed once per (case, stage, options) and shared
read-only.  torch is never imported here."""
import functools

import numpy as np

import ao_checker as A
import aov_chain_checker as KC
import aov_checker as K
import matte_checker as M
import scenes

abi = scenes.abi
W, H, SPP, RAYS, SEED = 40, 27, 2, 2, 5  # 5 x 4 tiles of 8 x 8, ragged on both axes
STAGES = ("aov", "aov_chain", "matte", "ao")
MATTE_KINDS = ("primitive", "material")
MATTE_LAYERS = 4
CHAIN_SPHERES, CHAIN_RATIO, CHAIN_SPECULAR_EVERY = 112, 1.44, 5  # the parity test's chain, every fifth sphere a mirror or glass
SPLITS = {"sah": abi.RT_SPLIT_SAH, "middle": abi.RT_SPLIT_MIDDLE, "equal": abi.RT_SPLIT_EQUAL_COUNTS}


class Case:
    """build() -> (SceneDescription, camera parameters or None for framing_camera); radius: the finite AO limit of the case, chosen
    on the reference so that some rays change from occluded to open (0: the case has no ray to change); specular: the scene has a
    Reflect / Refract material for the chain AOVs to follow; crowded: the geometry allows the 0.05 .. 0.95 occluded share the other
    AO test files ask for; primitives: the size of a tiny tree.  What the geometry of a case provably rules out is named, with the
    reason, and test_hard_trees.py asserts the exact property that holds instead:
      one_id          every camera ray hits the same primitive (no sky, one ID, no second matte layer)
      one_primitive   the scene has one primitive (two distinct IDs cannot exist; the sky is the second layer)
      never_occluded  no AO ray can reach anything: the visibility is exactly 1 on every hit pixel, whatever the radius
      enclosed        every AO ray starts inside a closed surface: without a limit the visibility is exactly 0 everywhere"""

    def __init__(self, build, radius, specular=False, crowded=False, one_id=None, one_primitive=None, never_occluded=None, enclosed=None,
                 primitives=None):
        self.build, self.radius, self.specular, self.crowded = build, radius, specular, crowded
        self.one_id, self.one_primitive, self.never_occluded, self.enclosed = one_id, one_primitive, never_occluded, enclosed
        self.primitives = primitives


def _tiny_spheres(n, split, seed):
    return lambda: (scenes.random_spheres(n, seed=seed, split_type=split, emissive_every=2), None)


def _tiny_triangles(n, split, seed):
    return lambda: (scenes.random_triangle_mesh(n, seed=seed, extent=1.0, edge=1.5, emissive_every=3, split_type=split,
                                                sampler_res=(8, 4)), None)


def framing_camera(root_min, root_max):
    """the tiny trees' camera: the direction of scenes.TINY_TREE_CAMERA, aimed at the centre of the root box from 1.1 of its
    diagonals away (the parity test's 14 units leave two or three primitives a handful of a 40 x 27 frame's pixels)"""
    lo, hi = np.asarray(root_min, np.float64), np.asarray(root_max, np.float64)
    centre = (lo + hi) / 2.0
    towards = np.array([0.0, -14.0, 2.0]) / np.linalg.norm([0.0, -14.0, 2.0])
    origin = centre + towards * 1.1 * np.linalg.norm(hi - lo)
    return dict(scenes.TINY_TREE_CAMERA, origin=tuple(float(x) for x in origin), lookat=tuple(float(x) for x in centre))


# The tiny trees keep the parity test's generators and arguments; the seed is the smallest at which the reference of every split
# type meets every condition of test_hard_trees.py from framing_camera (searched on the CPU, oracle only), the radius the smallest of
# 0.25, 0.5, 1, 2, 4, 8 that opens some occluded ray and leaves another occluded.
TINY_SPHERES = {2: (3, 2.0), 3: (19, 4.0), 5: (94, 0.25)}  # n -> (seed, AO radius)
TINY_TRIANGLES = {2: (6, 0.25), 3: (4, 2.0), 5: (1, 0.25)}
INSIDE = dict(scenes.ORIGIN_CAMERA)
OUTSIDE_DEGENERATE = dict(scenes.ORIGIN_CAMERA, origin=(1.5, 1.0, 1.0), lookat=(0.0, 0.0, -2.5))

# cheap trees first, the chain (the one whose stacks need more than 64 KB of LDS) last
CASES = {"single_sphere": Case(lambda: (scenes.single_sphere(), scenes.ORIGIN_CAMERA), 0.0, one_primitive="one sphere and the sky",
                               never_occluded="nothing can occlude a convex sphere")}
for _n, _splits in ((2, SPLITS), (3, SPLITS), (5, {"sah": abi.RT_SPLIT_SAH})):
    for _what, _split in _splits.items():
        CASES[f"spheres{_n}_{_what}"] = Case(_tiny_spheres(_n, _split, TINY_SPHERES[_n][0]), TINY_SPHERES[_n][1], primitives=_n)
        CASES[f"triangles{_n}_{_what}"] = Case(_tiny_triangles(_n, _split, TINY_TRIANGLES[_n][0]), TINY_TRIANGLES[_n][1], crowded=True,
                                                primitives=_n)
# The parity test's camera.  No AO ray of this scene can be occluded, from any camera: a sphere's hit carries the error EPSILON =
# 3e-4 per axis (sphere.rs:34-105, oracle/ora_geometry.c sphere_get_int), so offset_ray starts every AO ray at least 3e-4 along
# the normal from a clump that is 7e-5 across, and a cosine-weighted ray never turns back through the plane it starts on.
CASES["three_tiny_spheres"] = Case(lambda: (scenes.small_far_scenes()[0][1], scenes.small_far_camera(np.zeros(3, np.float32))), 0.0,
                                   never_occluded="every AO ray starts 3e-4 outside the 7e-5 clump and points away from it")
# The far clump from the other side, still through 0.001 degrees: the camera sits among the ordinary spheres, 62 units from the
# clump, on the line through the clump that is tangent to two of them (the spheres with rt_scene_desc indices 5 and 7; solved on the
# CPU), so the frame shows both silhouettes crossing, the sky behind them, and the rays of the sky pixels cross the clump's
# three-child node.  (The oracle's watertight test rejects the clump's 3e-5 triangles themselves at coordinates near 40: from the
# parity test's side the frame is the floor sphere alone, one ID.)
FAR_CLUMP = np.float32([40.0, 35.0, 30.0])
FAR_CLUMP_CAMERA = dict(scenes.small_far_camera(FAR_CLUMP), origin=(-2.8632063813958055, 0.12906617905773032, 1.0819986185641817))
CASES["far_clump_of_triangles"] = Case(lambda: (scenes.small_far_scenes()[1][1], FAR_CLUMP_CAMERA), 0.5, crowded=True)
CASES["degenerate_geometry"] = Case(lambda: (scenes.degenerate_geometry(), OUTSIDE_DEGENERATE), 1.0, specular=True, crowded=True)
CASES["inside_glass"] = Case(lambda: (scenes.degenerate_geometry(), INSIDE), 0.5, specular=True,
                             one_id="the camera sits inside the glass sphere: its inner surface is every first hit",
                             enclosed="the AO rays start on the inner surface of the glass sphere")
# the parity test's camera turned up and opened to 140 degrees: from its own view the infinite sphere is hit wherever nothing else
# is, and only above does the walk leave sky
NON_FINITE_WIDE = dict(scenes.NON_FINITE_CAMERA, lookat=(0.0, 6.0, 0.0), fov=140.0)
CASES["non_finite_geometry"] = Case(lambda: (scenes.non_finite_geometry(), NON_FINITE_WIDE), 1.0, crowded=True)
CASES["flat_box_lattice"] = Case(lambda: (scenes.flat_box_lattice(np.random.default_rng(21)), scenes.LATTICE_CAMERA), 1.0, crowded=True)
CASES["chain"] = Case(lambda: (scenes.skewed_chain_of_spheres(CHAIN_SPHERES, CHAIN_RATIO, specular_every=CHAIN_SPECULAR_EVERY),
                               scenes.CHAIN_CAMERA), 8.0, specular=True, crowded=True)


@functools.lru_cache(maxsize=None)
def built(name):
    """(scene description, camera parameters, oracle scene, oracle camera), once per case"""
    import oracle as O
    O.build()
    sc, cam_params = CASES[name].build()
    cpu = O.Scene(sc)
    if cam_params is None:
        root = cpu.nodes()[0]
        cam_params = framing_camera(root["min"], root["max"])
    return sc, cam_params, cpu, O.camera_new(**cam_params)


def _frozen(r):
    for v in (r.values() if isinstance(r, dict) else r):
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
        elif isinstance(v, (dict, tuple)):
            _frozen(v)
    return r


@functools.lru_cache(maxsize=None)
def first_hits(name):
    """per pass the oracle's check_hit records of the camera rays, [SPP][W*H]"""
    _, _, cpu, cam = built(name)
    pixels = np.arange(W * H)
    out = tuple(cpu.check_hit(*K.primary_rays(cam, W, H, SEED, pixels, p)) for p in range(SPP))
    return _frozen(out)


@functools.lru_cache(maxsize=None)
def aov(name):
    """the six channels of aov_checker.aovs, flat"""
    sc, _, cpu, cam = built(name)
    return _frozen(K.aovs(sc, cpu, cam, W, H, SPP, seed=SEED))


@functools.lru_cache(maxsize=None)
def aov_chain(name):
    """the seven channels of aov_chain_checker.aovs (max_chain 8, fuzz_limit 0), flat"""
    sc, _, cpu, cam = built(name)
    return _frozen(KC.aovs(sc, cpu, cam, W, H, SPP, seed=SEED))


@functools.lru_cache(maxsize=None)
def matte_pass_ids(name):
    """{kind: [SPP, W*H] u32}: each pass's first-hit IDs from the first-hit checker"""
    sc, _, cpu, cam = built(name)
    passes = [K.aovs(sc, cpu, cam, W, H, 1, seed=SEED, sample_begin=p) for p in range(SPP)]
    return _frozen({kind: np.stack([r[kind] for r in passes]) for kind in MATTE_KINDS})


@functools.lru_cache(maxsize=None)
def matte(name):
    """{kind: (ids [K, n], coverage [K, n], residual [n])}"""
    return _frozen({kind: M.layers_from_pass_ids(matte_pass_ids(name)[kind], MATTE_LAYERS) for kind in MATTE_KINDS})


@functools.lru_cache(maxsize=None)
def ao(name, radius):
    """ao_checker.ao's dict (the two channels flat, and the counts behind them)"""
    _, _, cpu, cam = built(name)
    return _frozen(A.ao(cpu, cam, W, H, SPP, RAYS, radius=radius, seed=SEED))


def framed(r):
    """flat per-pixel arrays ([n] or [n, 3]) as frames"""
    return {k: v.reshape((H, W, 3) if v.ndim == 2 else (H, W)) for k, v in r.items()}


def occluded_share(r):
    return 1.0 - r["unoccluded"].sum() / max(int(r["rays"].sum()), 1)
