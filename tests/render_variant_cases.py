"""The render kernels' variants on the trees built to break walks, as ONE table: test_render_variant_cases.py (CPU) shows that no
entry is vacuous, test_gpu_render_variants.py renders every (case, method, work shape, variant) and compares the frame, the ray
count and what rt_last_launch_info reports with what stands here.

Cases: every entry of hard_tree_cases.CASES under its own camera, `all_materials` as the control that needs the full feature set,
and `chain_along_axis`: the 112-sphere chain seen from its thin end.  That last one is here because of what the numpy walk of the
host tree (wide_walk.py) measured: from scenes.CHAIN_CAMERA, which looks at the chain from the side, no camera ray ever leaves more
than ONE entry pending (a ray crosses the axis once and meets a handful of boxes), so the frame of the `chain` case cannot take a
walk into the overflow area whatever the cap; from (-0.5, 0.5, 0.25) looking along +x the first descent of a camera ray runs down
the whole chain, nearest child first, and leaves 84 of the tree's 85 worst-case entries pending before it reaches its first leaf.

Expected launch: `expected_launch` restates the rules of include/rt_hip.h (RT_TUNE_*) and is never read back from a GPU.
torch is never imported here."""
import collections
import functools
import importlib

import numpy as np

import hard_tree_cases as HT
import scenes
import wide_walk as WW

abi = scenes.abi
W, H, SEED, SPP = HT.W, HT.H, 5, 4
METHODS = (abi.RT_METHOD_NAIVE, abi.RT_METHOD_MIS)
NO_INDEX = np.uint64(abi.NO_INDEX)

# ---- cases: name -> () -> (scene description, camera parameters, oracle scene, oracle camera) ----
CHAIN_AXIS_CAMERA = dict(origin=(-0.5, 0.5, 0.25), lookat=(20.0, 0.0, 0.0), vup=(0.0, 0.0, 1.0), fov=40.0,
                         aspect_ratio=float(np.float32(16.0) / np.float32(9.0)), aperture=0.0, focus_dist=10.0)
EXTRA = {
    "chain_along_axis": lambda: (HT.built("chain")[0], CHAIN_AXIS_CAMERA),
    "all_materials": lambda: (scenes.all_materials(), scenes.ALL_MATERIALS_CAMERA),
}
CASES = list(HT.CASES) + list(EXTRA)

# What the numpy walk measured on the host tree of the chain (test_render_variant_cases.py measures it again and compares): the
# largest number of pending stack entries over the 40 x 27 pixel-centre rays, at a moment when the pruned device walk is still
# the unpruned one (wide_walk.pending_entries "reached").  A forced cap reaches the overflow area only if it lies below it.
CHAIN_CAMERA_MAX_PENDING = 1   # scenes.CHAIN_CAMERA: nothing to overflow (the exemption of the `chain` case, see below)
CHAIN_AXIS_MAX_PENDING = 84    # CHAIN_AXIS_CAMERA; the tree's worst case (rt_scene_wide_info stack_depth) is 85
CHAIN_AXIS_TWO_CHILD_PENDING = 56  # the two-child walk of every seventh of the same rays; stack_depth_narrow is 57
STACK_CAPS = (1, CHAIN_AXIS_MAX_PENDING // 2, CHAIN_AXIS_MAX_PENDING - 1)  # 1, 42, 83
MIDDLE_CAP = STACK_CAPS[1]

# No wide tree: a forced fine schedule stays coarse (the fine kernels walk the wide tree only).  single_sphere: the root is a leaf.
# non_finite_geometry: the build makes no wide tree from non-finite bounds (its NaN centroids also leave the reference tree one
# leaf of eight primitives).  Both are asserted on the host-only scene, whose wide_tree() answers without a GPU.
NO_WIDE_TREE = {"single_sphere": "the root is a leaf", "non_finite_geometry": "non-finite bounds"}
# Not tiny: the packed copy of the scene is above the 12 KB the coarse kernels stage into LDS (the chain: 111 nodes x 64 B +
# 112 primitives x 48 B alone are 12 480 B; the lattice: 1 920 triangles).  No host getter says so: stated here, asserted on the GPU
# through scene_in_lds of every launch.
NOT_STAGED = {"chain": "12 480 B of nodes and primitives alone", "chain_along_axis": "12 480 B of nodes and primitives alone",
              "flat_box_lattice": "1 920 triangles"}
# No case is a pair tree (one node over two single-sphere leaves of Lambertian spheres, feature set 0): the two-sphere trees hold an
# emissive sphere (feature set 1), single_sphere's root is a leaf, three_tiny_spheres has three.  So feature set 3 is never
# expected, and "naming the library's own set turns the pair kernel off" has no case to apply to; the CPU file asserts the premise.

# Frames that provably cannot differ between sample_split 1 and 2, with the property asserted instead (at most one per case):
# name -> (methods, reason).  The splits fold the same samples in another order, so they differ only where a fold rounds.
_DYADIC = "a solid sky of 1.0 over Lambertian surfaces of 0.5 x 0.5: every sample is a short dyadic number, both folds are exact"
SPLIT_EXEMPT = {"three_tiny_spheres": (METHODS, _DYADIC), "far_clump_of_triangles": (METHODS, _DYADIC),
                "inside_glass": ((abi.RT_METHOD_MIS,), "under MIS every sample from inside the glass sphere is +0: the frame is black")}
# ... and the one case whose camera cannot reach the overflow area (see the module docstring): the replacement is chain_along_axis
CAP_EXEMPT = {"chain": "no camera ray of scenes.CHAIN_CAMERA leaves more than one entry pending: chain_along_axis carries the caps"}


@functools.lru_cache(maxsize=None)
def built(name):
    """(scene description, camera parameters, oracle scene, oracle camera), once per case"""
    if name in HT.CASES:
        return HT.built(name)
    import oracle as O
    O.build()
    sc, cam_params = EXTRA[name]()
    cpu = HT.built("chain")[2] if name == "chain_along_axis" else O.Scene(sc)
    return sc, cam_params, cpu, O.camera_new(**cam_params)


def _hb():
    return importlib.import_module("raytracing-rust_amd.hip_backend")


@functools.lru_cache(maxsize=None)
def host_scene(name):
    return _hb().HipScene(built(name)[0], device=abi.RT_DEVICE_NONE)


Facts = collections.namedtuple("Facts", "n_primitives triangles lights wide tiny min_feature_set")


@functools.lru_cache(maxsize=None)
def facts(name):
    """what the header's rules read off a scene, from its description and its host-only build"""
    sc = built(name)[0]
    d = sc.desc()
    _, n_prims, n_lights = host_scene(name).counts()
    triangles = any(d.primitives[i].type != abi.RT_PRIM_SPHERE for i in range(d.n_primitives))
    # RT_TUNE_FEATURE_SET: 0 spheres-only, 1 + triangles and emissive primitives, 2 every material / texture
    every = any(m.type not in (abi.RT_MAT_EMIT, abi.RT_MAT_LAMBERTIAN) for m in sc.materials) or \
        any(t.type not in (abi.RT_TEX_SOLID, abi.RT_TEX_LERP) for t in sc.textures)
    min_fs = 2 if every else 1 if (triangles or n_lights) else 0
    wide = len(host_scene(name).wide_tree()[0]) > 0
    return Facts(int(n_prims), triangles, int(n_lights), wide, name not in NOT_STAGED, min_fs)


# ---- variants: a curated list, every value of every key it names ----
Variant = collections.namedtuple("Variant", "traversal schedule walk scene_in_lds exchange feature_set stack_cap")
AUTOMATIC = Variant(-1, -1, 0, 1, 0, None, 0)
KEYS = {"traversal": abi.RT_TUNE_TRAVERSAL, "schedule": abi.RT_TUNE_SCHEDULE, "walk": abi.RT_TUNE_WALK,
        "scene_in_lds": abi.RT_TUNE_SCENE_IN_LDS, "exchange": abi.RT_TUNE_EXCHANGE, "feature_set": abi.RT_TUNE_FEATURE_SET,
        "stack_cap": abi.RT_TUNE_STACK_CAP}
VALUES = {"traversal": (-1, 0, 1), "schedule": (-1, 0, 1), "walk": (0, 1), "scene_in_lds": (0, 1), "exchange": (0, 1),
          "feature_set": (None, 0, 1, 2), "stack_cap": (0,) + STACK_CAPS}

VARIANTS = [AUTOMATIC]
for _trav in (0, 1):  # the coarse schedule: exhaustive and pruned, the scene staged in LDS and read from memory
    for _lds in (1, 0):
        VARIANTS.append(Variant(_trav, 0, 0, _lds, 0, None, 0))
VARIANTS += [
    Variant(1, 0, 1, 1, 0, None, 0), Variant(1, 0, 1, 0, 0, None, 0),  # coarse pruned, the two-child tree for every ray
    Variant(0, 0, 0, 1, 1, None, 0),  # coarse exhaustive with the exchange: runs under MIS, ignored under NAIVE
    Variant(0, 0, 0, 0, 1, None, 0),
    Variant(1, 0, 0, 1, 1, None, 0),  # coarse pruned: the exchange is ignored
]
for _walk in (0, 1):  # the fine schedule: the wide walk and PH_NARROW for every ray, 256-thread and 512-thread exchange workgroups
    for _x in (0, 1):
        VARIANTS.append(Variant(1, 1, _walk, 1, _x, None, 0))
VARIANTS += [
    Variant(0, 1, 0, 0, 0, None, 0),  # fine implies the pruned walk, and never stages the scene
    Variant(-1, 1, 0, 1, 0, None, 0),
    # forced caps: what lies above them goes to the global overflow area (STACK_CAPS)
    Variant(1, 1, 0, 1, 0, None, STACK_CAPS[0]), Variant(1, 1, 0, 1, 0, None, STACK_CAPS[1]), Variant(1, 1, 0, 1, 0, None, STACK_CAPS[2]),
    Variant(1, 1, 0, 1, 1, None, STACK_CAPS[0]), Variant(1, 1, 0, 1, 1, None, STACK_CAPS[1]),  # ... with the pools behind the stacks
    Variant(1, 1, 1, 1, 0, None, STACK_CAPS[0]), Variant(1, 1, 1, 1, 1, None, STACK_CAPS[1]),  # ... under the two-child walk
    Variant(1, 0, 0, 1, 0, None, STACK_CAPS[0]),  # a coarse launch ignores the cap
]
for _fs in (0, 1, 2):  # every feature set a case admits, by name: automatic, coarse both ways, fine with and without the exchange
    VARIANTS += [Variant(-1, -1, 0, 1, 0, _fs, 0), Variant(0, 0, 0, 0, 0, _fs, 0), Variant(0, 0, 0, 1, 1, _fs, 0),
                 Variant(1, 0, 0, 1, 0, _fs, 0), Variant(1, 1, 0, 1, 0, _fs, 0), Variant(1, 1, 1, 1, 1, _fs, STACK_CAPS[1])]


def variants_for(name):
    """(the variants that run on the case, the feature sets the library refuses for it: below its own).  Variants that name no
    feature set come first: a scene that has had one named cannot go back to the library's choice."""
    low = facts(name).min_feature_set
    run = [v for v in VARIANTS if v.feature_set is None] + [v for v in VARIANTS if v.feature_set is not None and v.feature_set >= low]
    return run, [fs for fs in (0, 1, 2) if fs < low]


Launch = collections.namedtuple("Launch", "fine pruned scene_in_lds feature_set exchange")
PRUNE_ABOVE = 100  # automatic traversal: pruned above 100 primitives
FINE_ABOVE = {True: 4096, False: 32768}  # automatic schedule: fine above so many primitives (with / without triangles), if pruned


def expected_launch(name, v, method):
    """what rt_last_launch_info must report (exchange: the kernel name ends in ", true>")"""
    f = facts(name)
    pruned = f.n_primitives > PRUNE_ABOVE if v.traversal == -1 else v.traversal == 1
    if v.schedule == -1:
        fine = pruned and f.n_primitives > FINE_ABOVE[f.triangles]
    else:
        fine = v.schedule == 1
    fine = fine and f.wide  # NO_WIDE_TREE: a forced fine schedule stays coarse
    pruned = pruned or fine
    staged = (not fine) and f.tiny and v.scene_in_lds == 1
    feature_set = f.min_feature_set if v.feature_set is None else v.feature_set
    exchange = v.exchange == 1 and (fine or (method == abi.RT_METHOD_MIS and not pruned))
    return Launch(int(fine), int(pruned), int(staged), feature_set, bool(exchange))


def describe(name, method, shape, v):
    return (f"{name} m={method} {shape} fs={v.feature_set} trav={v.traversal} sched={v.schedule} walk={v.walk} lds={v.scene_in_lds} "
            f"xchg={v.exchange} cap={v.stack_cap}")


# ---- work shapes and references ----
SHAPES = ("split1", "split2", "shard1of3")


def options(method, shape):
    o = abi.default_render_opts(W, H, SPP, method=method, seed=SEED)
    o.sample_split = 1 if shape == "split1" else 2
    if shape == "shard1of3":
        o.shard_index, o.shard_count, o.output_layout = 1, 3, abi.RT_LAYOUT_SHARD
    return o


@functools.lru_cache(maxsize=None)
def oracle_frame(name, method, split):
    """(frame [H, W, 3] f32, rays_shot) of the CPU oracle, read-only"""
    _, _, cpu, cam = built(name)
    o = options(method, "split1")
    o.sample_split = split
    img, rays = cpu.render(cam, o)
    img.setflags(write=False)
    return img, int(rays)


@functools.lru_cache(maxsize=None)
def shard_pixels(method=abi.RT_METHOD_MIS):
    """pixel indices of shard 1 of 3 in the order RT_LAYOUT_SHARD packs them (padding entries of ragged tiles: NO_INDEX)"""
    order = _hb().shard_pixel_order(options(method, "shard1of3"))
    order.setflags(write=False)
    return order


@functools.lru_cache(maxsize=None)
def oracle_shard_rays(name, method):
    """rays_shot of the oracle's render of shard 1 of 3 alone (0 where MIS traces nothing from the shard's pixels)"""
    _, _, cpu, cam = built(name)
    o = options(method, "shard1of3")
    o.output_layout = abi.RT_LAYOUT_FRAME
    return int(cpu.render(cam, o)[1])


def reference(name, method, shape):
    """the pixels a render of that shape must return: the oracle's frame, or its pixels in the shard's order (padding: zero)"""
    frame, rays = oracle_frame(name, method, 1 if shape == "split1" else 2)
    if shape != "shard1of3":
        return frame, rays
    order = shard_pixels()
    valid = order != NO_INDEX
    out = np.zeros((len(order), 3), np.float32)
    out[valid] = frame.reshape(-1, 3)[order[valid].astype(np.int64)]
    return out, None  # (the shard's ray count: rt_render of the same shard under automatic settings, checked against this frame)


# ---- what the walks of a case's camera rays do, on the host tree ----
@functools.lru_cache(maxsize=None)
def camera_misses(name):
    _, _, cpu, cam = built(name)
    o, d = WW.pixel_centre_rays(cam, W, H)
    hits = cpu.check_hit(np.broadcast_to(o, d.shape).copy(), d)
    return hits["index"] == NO_INDEX


@functools.lru_cache(maxsize=None)
def pending(name):
    return WW.pending_entries(host_scene(name), built(name)[3], W, H, camera_misses(name))


def narrow_stack_depth(name):
    """HostScene::stack_depth_narrow as rt_build.cpp states it: the deepest inner node's level, the root at 1, plus one"""
    nodes = host_scene(name).nodes()
    level = np.zeros(len(nodes), np.int64)
    level[0], deepest = 1, 1
    for i, n in enumerate(nodes):
        if int(n["children"][0]) < 0:
            continue
        deepest = max(deepest, int(level[i]))
        level[int(n["children"][0])] = level[int(n["children"][1])] = level[i] + 1
    return deepest + 1
