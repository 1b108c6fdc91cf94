"""The inputs the tile render (rt_render_tiles, csrc/rt_adaptive.hip tiles_kernel) treats differently, as ONE table:
test_tiles_cases.py (CPU) shows on the oracle alone that every entry tests something, test_gpu_tiles_regimes.py runs the kernel on
it.  tiles_kernel restates the integrator arms, the sky-table view, the roulette and depth tests and the 64-bit stream assembly, and
has a chunk rule of its own, so each of them gets entries here.  Six groups (the seventh, the adaptive loop under a sampled sky, is
an entry of test_adaptive_cases.CASES):

  sky/<case>/<scene>/<method>  every sky of sky_cases.RENDER_CASES on radiance_cases' three scenes under MIS (the 2^24-cell skies:
                               the floor only), and under NAIVE on the floor, whose reference is the oracle on the same texture
                               with sampler_res (0, 0)
  arm/<shape>/<method>/s<S>    one scene per arm of sample_lights (radiance_cases.SHAPES)
  uneven/<method>/<spp>_<S>    splits that do not divide spp: chunk c = passes [floor(c spp / S), floor((c + 1) spp / S))
  stream/...                   seeds and first samples as 64-bit values: the carry into the high word inside a pixel's passes and
                               on a chunk boundary, and the wrap past 2^64 - 1
  depth/...                    max_depth 1 (the MIS prologue's own exit), 2 and 8, rr_threshold 0 and 3
  ragged/<w>x<h>/<list>/s<S>   frames narrower or lower than a tile, down to the smallest the API accepts

An entry is a scene, render options and tile lists; its references are the oracle's frame and ray count (O.Scene.render) and the
chunk sums of the oracle's passes (noise_checker.passes, chunk_sums), computed once per entry and shared read-only.  Every list is
in non-ascending order and, where the frame has more than one tile, a proper subset of them.  torch is never imported here."""
import functools

import numpy as np

import noise_checker as N
import radiance_cases as RC
import scenes
import sky_cases as SK

abi = scenes.abi
F32 = np.float32
NAIVE, MIS = RC.NAIVE, RC.MIS
METHODS = RC.METHODS
SENTINEL = F32(-123.25)
SEED, BEGIN = 7, 5
MASK64 = (1 << 64) - 1
LOW = RC.LOW
MATERIALS = "streams"  # radiance_cases' entry of scenes.all_materials() under ALL_MATERIALS_CAMERA


class Entry:
    """scene: what the GPU renders, ref_scene: what the oracle renders (the same unless stated); lists: the tile lists, each run
    on a frame pre-filled with SENTINEL; sums: with a chunk buffer, without, or both (split 1 has none); groups: the values of
    RT_TUNE_RADIANCE_GROUPS the entry runs under (0: the automatic grid)"""

    def __init__(self, scene, method, w, h, spp, split, lists, *, ref_scene=None, seed=SEED, begin=BEGIN, max_depth=50, rr=3, groups=(0,)):
        self.scene, self.ref_scene, self.method, self.w, self.h, self.spp, self.split = scene, ref_scene or scene, method, w, h, spp, split
        self.lists, self.seed, self.begin, self.max_depth, self.rr, self.groups = tuple(tuple(t) for t in lists), seed, begin, max_depth, rr, groups
        self.sums = (False, True) if split > 1 else (False,)

    def n_tiles(self):
        return ((self.w + 7) // 8) * ((self.h + 7) // 8)


def _m(method):
    return "mis" if method == MIS else "naive"


ENTRIES = {}

# ---- 1. skies: MIS on every scene, [3, 0] of the four tiles of 16 x 16; NAIVE on the floor against the unsampled texture ----
for _case in SK.RENDER_CASES:
    _huge = _case in SK.HUGE
    _shape = (8, 16, 2, 2, [[1]]) if _huge else (16, 16, 4, 2, [[3, 0]])
    for _scene in RC.sky_scenes_of(_case):
        ENTRIES[f"sky/{_case}/{_scene}/mis"] = Entry(f"sky/{_case}/{_scene}", MIS, *_shape)
    ENTRIES[f"sky/{_case}/floor/naive"] = Entry(f"sky/{_case}/floor", NAIVE, *_shape, ref_scene=f"unsampled/{_case}/floor")
SKIES = tuple(k for k in ENTRIES if k.startswith("sky/"))

# ---- 2. the four arms of sample_lights: a list and its complement, whose ray counters add up to the oracle's ----
ARM_LISTS = ([3, 0], [2, 1])
for _name in RC.SHAPES:
    for _method in METHODS:
        for _split in (1, 2):
            ENTRIES[f"arm/{_name}/{_m(_method)}/s{_split}"] = Entry(f"shape/{_name}", _method, 16, 16, 4, _split, ARM_LISTS)
ARMS = tuple(k for k in ENTRIES if k.startswith("arm/"))

# ---- 3. chunks of unequal length ----
UNEVEN = ((7, 3), (7, 4), (7, 5), (5, 5), (3, 2), (7, 7))
# with a chunk buffer an item is one chunk: three tiles at S = 3 are nine items for the four waves of one workgroup, so under
# RT_TUNE_RADIANCE_GROUPS = 1 every wave takes a second item and its lanes refill across items
UNEVEN_ONE_GROUP = (7, 3)
for _method in METHODS:
    for _spp, _split in UNEVEN:
        ENTRIES[f"uneven/{_m(_method)}/{_spp}_{_split}"] = Entry(MATERIALS, _method, 16, 16, _spp, _split, [[3, 2, 0]],
                                                               groups=(0, 1) if (_spp, _split) == UNEVEN_ONE_GROUP else (0,))
UNEVENS = tuple(k for k in ENTRIES if k.startswith("uneven/"))

# ---- 4. 64-bit seeds and first samples ----
STREAM_SPP = 4
# 2^32 - 2: the carry falls inside a pixel's passes, and at split 2 on the chunk boundary; 2^64 - 2: the third pass is sample 0
STREAM_BEGINS = ((1 << 32) - 2, (1 << 32) - 1, 1 << 32, (1 << 64) - 2)
for _method in METHODS:
    for _split in (1, 2):
        for _seed in RC.SEEDS:
            for _begin in STREAM_BEGINS:
                ENTRIES[f"stream/{_m(_method)}/s{_split}/{_seed:#x}/{_begin:#x}"] = Entry(MATERIALS, _method, 16, 8, STREAM_SPP, _split, [[1]],
                                                                                        seed=_seed, begin=_begin)
STREAMS = tuple(k for k in ENTRIES if k.startswith("stream/"))

# ---- 5. depth and roulette ----
DEPTH_SCENES = (MATERIALS, "rtweekend1")
DEPTHS, ROULETTES = (1, 2, 8), (0, 3)
for _scene in DEPTH_SCENES:
    for _method in METHODS:
        for _d in DEPTHS:
            for _r in ROULETTES:
                ENTRIES[f"depth/{_scene}/{_m(_method)}/d{_d}/r{_r}"] = Entry(_scene, _method, 16, 8, 4, 2, [[1]], max_depth=_d, rr=_r)
DEPTH_KEYS = tuple(k for k in ENTRIES if k.startswith("depth/"))

# ---- 6. ragged frames: every non-empty proper sublist of at most two tiles.  2 x 2, the smallest frame rt_render accepts, has ONE
# tile and so no proper sublist: its list is that tile, 60 of whose 64 lanes are padding ----
RAGGED = {(2, 2): ([0],), (5, 11): ([0], [1]), (9, 8): ([0], [1])}
for (_w, _h), _lists in RAGGED.items():
    for _list in _lists:
        for _split in (1, 2):
            ENTRIES[f"ragged/{_w}x{_h}/{'_'.join(map(str, _list))}/s{_split}"] = Entry(MATERIALS, MIS, _w, _h, 4, _split, [_list])
RAGGEDS = tuple(k for k in ENTRIES if k.startswith("ragged/"))


# ---- scenes, options, references: once each ----
@functools.lru_cache(maxsize=None)
def built(scene):
    """(scene description, camera parameters, oracle scene, oracle camera): radiance_cases' scenes (the oracle scene of a
    2^24-cell sky is built once per process), `unsampled/<case>/<scene>` the same texture with sampler_res (0, 0), else a scene of
    test_gpu_ao.SCENES"""
    if scene.startswith("unsampled/"):
        import oracle as O
        O.build()
        _, case, base = scene.split("/")
        sc, cam_params = RC.unsampled_scene(case, base), RC.SKY_SCENES[base]()[1]
        return sc, cam_params, O.Scene(sc), O.camera_new(**cam_params)
    if scene in RC.ENTRIES:
        return RC.built(scene)
    from test_gpu_ao import _built
    return _built(scene)


def make_opts(method, w, h, spp, split, seed=SEED, begin=BEGIN, max_depth=50, rr=3):
    o = abi.default_render_opts(w, h, spp, method=method, seed=seed)
    o.sample_begin, o.sample_split, o.max_depth, o.rr_threshold = begin, split, max_depth, rr
    return o


def opts(key):
    e = ENTRIES[key]
    return make_opts(e.method, e.w, e.h, e.spp, e.split, e.seed, e.begin, e.max_depth, e.rr)


def render(scene, o):
    """the oracle's frame and rays_shot, computed now"""
    _, _, cpu, cam = built(scene)
    return cpu.render(cam, o, n_threads=1)


@functools.lru_cache(maxsize=None)
def reference(key):
    """(frame (H, W, 3) f32, rays_shot) of the oracle under the entry's options"""
    img, rays = render(ENTRIES[key].ref_scene, opts(key))
    img.setflags(write=False)
    return img, rays


def has_nan(key):
    """the entry's oracle frame holds a NaN: the one case in which a comparison may treat NaNs as equal"""
    return bool(np.isnan(reference(key)[0]).any())


@functools.lru_cache(maxsize=None)
def single_pass(scene, method, w, h, seed, index, max_depth=50, rr=3):
    """(H, W, 3) f32: the pass at sample index `index` -- a render of one pass is that pass"""
    img, _ = render(scene, make_opts(method, w, h, 1, 1, seed, index, max_depth, rr))
    img.setflags(write=False)
    return img


def pass_indices(begin, spp):
    """begin + k in 64-bit arithmetic that wraps (include/rt_hip.h rt_render_opts.sample_begin)"""
    return [(begin + k) & MASK64 for k in range(spp)]


def passes(key, indices=None, seed=None):
    """(spp, H, W, 3) f32: the entry's passes, or those at the given sample indices / seed"""
    e = ENTRIES[key]
    indices = pass_indices(e.begin, e.spp) if indices is None else indices
    return np.stack([single_pass(e.ref_scene, e.method, e.w, e.h, e.seed if seed is None else seed, i, e.max_depth, e.rr) for i in indices])


def fold(pass_images, split, bounds=None):
    """what rt_render writes from these passes: split 1 the running mean `mean += (pass - mean) / i`, else the chunk sums added in
    chunk order from +0 and divided by spp once"""
    if split == 1:
        mean = np.zeros(pass_images.shape[1:], F32)
        with np.errstate(all="ignore"):
            for i, p in enumerate(pass_images):
                mean = mean + (p - mean) / F32(i + 1)
        return mean
    with np.errstate(all="ignore"):
        return N.combine(N.chunk_sums(pass_images, split, bounds), len(pass_images))


@functools.lru_cache(maxsize=None)
def sums_reference(key):
    """(S, H, W, 3) f32: the chunk sums of the entry's passes under noise_checker.chunk_bounds"""
    e = ENTRIES[key]
    assert e.split > 1
    with np.errstate(all="ignore"):
        s = N.chunk_sums(passes(key), e.split)
    s.setflags(write=False)
    return s


def padded_sums(key, tiles):
    """(S, len(tiles), 8, 8, 3) f32: sums_reference in rt_render_tiles' layout, +0 in the padding lanes of edge tiles"""
    e = ENTRIES[key]
    tx, ty = (e.w + 7) // 8, (e.h + 7) // 8
    padded = np.zeros((e.split, 8 * ty, 8 * tx, 3), F32)
    padded[:, :e.h, :e.w] = sums_reference(key)
    return np.stack([padded[:, 8 * (t // tx):8 * (t // tx) + 8, 8 * (t % tx):8 * (t % tx) + 8] for t in tiles], axis=1)


def mask(tiles, w, h):
    """(h, w) bool: the pixels of the listed tiles"""
    tx = (w + 7) // 8
    m = np.zeros((h, w), bool)
    for t in tiles:
        y, x = 8 * (int(t) // tx), 8 * (int(t) % tx)
        m[y:y + 8, x:x + 8] = True
    return m


def listed(key):
    """(h, w) bool: the pixels of the entry's first list"""
    e = ENTRIES[key]
    return mask(e.lists[0], e.w, e.h)


def ceil_bounds(spp, split):
    """the alternative rule the header does NOT state: ceil(spp / S) passes a chunk, a short (or empty) last chunk"""
    n = -(-spp // split)
    return [min(c * n, spp) for c in range(split)] + [spp]
