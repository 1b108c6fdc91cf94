"""The ambient-occlusion pass (rt_render_ao) on the GPU against the CPU checker (tests/ao_checker.py): every comparison of both
channels is bit-exact (NaN == NaN).  A scene's checker result is computed once per set of options and shared."""
import functools

import numpy as np
import pytest

import ao_checker as A
import aov_checker as K
import scenes
from gpu_support import GuardedBuffers, assert_render_unaffected, assert_same_bits, capture, ssml_scene

pytestmark = pytest.mark.gpu
abi = scenes.abi
W, H, SPP, RAYS, SEED = 64, 36, 2, 2, 3  # 36 rows: an edge row of half tiles
F32 = np.float32
CHANNELS = abi.AO_CHANNELS


SCENES = {
    "emit_scene": lambda: (K.emit_scene(), K.EMIT_CAMERA),
    "all_materials": lambda: (scenes.all_materials(), scenes.ALL_MATERIALS_CAMERA),
    "spheres500": lambda: (scenes.random_spheres(500), scenes.ALL_MATERIALS_CAMERA),
    "pyramid": lambda: ssml_scene("pyramid"),
    "rtweekend1": lambda: ssml_scene("rtweekend1"),
    "overshadowed": lambda: ssml_scene("overshadowed"),
    # triangles wide enough to be seen and to shadow each other (the default edge of 0.05 is hit by 0.2 % of the camera rays)
    "mesh2000_wide": lambda: (scenes.random_triangle_mesh(2000, edge=2.0), scenes.MESH_CAMERA),
    "mesh20000": lambda: (scenes.random_triangle_mesh(20000, edge=1.0), scenes.MESH_CAMERA),
}
SIX = ["emit_scene", "all_materials", "spheres500", "pyramid", "rtweekend1", "overshadowed"]


@functools.lru_cache(maxsize=None)
def _built(name):
    """(scene description, camera parameters, oracle scene, oracle camera), once per scene"""
    import oracle as O
    O.build()
    sc, cam_params = SCENES[name]()
    return sc, cam_params, O.Scene(sc), O.camera_new(**cam_params)


@functools.lru_cache(maxsize=None)
def _checked(name, w, h, spp, rays, radius, seed, sample_begin):
    _, _, cpu, cam = _built(name)
    r = A.ao(cpu, cam, w, h, spp, rays, radius=radius, seed=seed, sample_begin=sample_begin)
    for v in r.values():
        v.setflags(write=False)
    return r


def _frames(r, w, h):
    return {"visibility": r["visibility"].reshape(h, w), "bent_normal": r["bent_normal"].reshape(h, w, 3)}


def _gpu(hb, name, **kw):
    sc, cam_params, _, _ = _built(name)
    return hb.HipScene(sc, **(kw or dict(device=0))), hb.camera_new(**cam_params)


def _opts(w=W, h=H, spp=SPP, seed=SEED, sample_begin=0):
    o = abi.default_render_opts(w, h, spp, seed=seed)
    o.sample_begin = sample_begin
    return o


def assert_ao_equal(gpu, ref, what):
    assert set(gpu) == set(ref), (what, sorted(gpu), sorted(ref))
    for name in ref:
        assert_same_bits(gpu[name], ref[name], f"{what} {name}", nan_equal=True)


def _shares(r):
    n = int(r["rays"].sum())
    return r["hits"].sum() / (len(r["hits"]) * r["open"].shape[1]), 1.0 - r["unoccluded"].sum() / max(n, 1)


# ---- the six reference scenes ----
@pytest.mark.parametrize("name", SIX)
def test_reference_scenes_match_the_checker(hb, name):
    gpu, cam = _gpu(hb, name)
    for radius in (0.0, 1.0):
        r = _checked(name, W, H, SPP, RAYS, radius, SEED, 0)
        hit_share, occluded_share = _shares(r)
        print(f"{name} radius {radius}: hit share {hit_share:.3f} occluded share of the AO rays {occluded_share:.3f}")
        if radius == 0.0:  # a frame that is all open or all closed would test nothing
            assert 0.05 <= occluded_share <= 0.95, (name, hit_share, occluded_share)
        ref = _frames(r, W, H)
        for mode in (0, 1, -1):  # forced exhaustive / pruned, automatic: the same bytes
            gpu.set_traversal(mode)
            assert_ao_equal(gpu.render_ao(cam, _opts(), rays_per_pass=RAYS, radius=radius), ref, f"{name} radius={radius} traversal={mode}")


# ---- triangle meshes ----
@pytest.mark.parametrize("name", ["mesh2000_wide", "mesh20000"])
def test_triangle_meshes_under_both_traversals(hb, name):
    gpu, cam = _gpu(hb, name)
    r = _checked(name, W, H, SPP, RAYS, 0.0, SEED, 0)
    hit_share, occluded_share = _shares(r)
    print(f"{name}: hit share {hit_share:.3f} occluded share of the AO rays {occluded_share:.3f}")
    assert 0.05 <= occluded_share <= 0.95 and hit_share > 0.5
    ref = _frames(r, W, H)
    for mode in (0, 1, -1):
        gpu.set_traversal(mode)
        assert_ao_equal(gpu.render_ao(cam, _opts(), rays_per_pass=RAYS), ref, f"{name} traversal={mode}")
    limited = _frames(_checked(name, W, H, SPP, RAYS, 0.25, SEED, 0), W, H)
    for mode in (0, 1):
        gpu.set_traversal(mode)
        assert_ao_equal(gpu.render_ao(cam, _opts(), rays_per_pass=RAYS, radius=0.25), limited, f"{name} radius=0.25 traversal={mode}")


def test_the_wide_walk_and_the_two_child_walk_give_the_same_bytes(hb):
    """the pruned traversal walks the four-wide tree with its big leaves where the scene has one; RT_TUNE_WALK = 1 sends every ray
    through the two-child tree instead"""
    name = "mesh20000"
    gpu, cam = _gpu(hb, name)
    nodes, _root, depth, _boxes = gpu.wide_tree()
    n_prims = int(gpu.counts()[0])
    print(f"{name}: {n_prims} primitives, automatic traversal = {'pruned' if n_prims > 100 else 'exhaustive'}; "
          f"wide tree of {len(nodes)} nodes, depth {depth}: the pruned walk is the {'wide' if len(nodes) else 'two-child'} one")
    assert len(nodes) > 0, "the scene has no wide tree: the case tests nothing"
    ref = _frames(_checked(name, W, H, SPP, RAYS, 0.0, SEED, 0), W, H)
    limited = _frames(_checked(name, W, H, SPP, RAYS, 0.25, SEED, 0), W, H)
    gpu.set_traversal(1)
    for walk in (0, 1):
        gpu.set_tuning(abi.RT_TUNE_WALK, walk)
        assert_ao_equal(gpu.render_ao(cam, _opts(), rays_per_pass=RAYS), ref, f"walk={walk}")
        assert_ao_equal(gpu.render_ao(cam, _opts(), rays_per_pass=RAYS, radius=0.25), limited, f"walk={walk} radius=0.25")


# ---- options and shapes ----
@pytest.mark.parametrize("rays,size", [(1, (W, H)), (3, (W, H)), (4, (W, H)), (64, (16, 9))])
def test_rays_per_pass(hb, rays, size):
    w, h = size
    gpu, cam = _gpu(hb, "all_materials")
    ref = _frames(_checked("all_materials", w, h, SPP, rays, 0.0, SEED, 0), w, h)
    assert_ao_equal(gpu.render_ao(cam, _opts(w, h), rays_per_pass=rays), ref, f"K={rays}")


@pytest.mark.parametrize("radius", [0.0, 0.25, 1.0, np.inf])
def test_radius(hb, radius):
    gpu, cam = _gpu(hb, "spheres500")
    r = _checked("spheres500", W, H, SPP, 4, radius, 8, 0)
    assert_ao_equal(gpu.render_ao(cam, _opts(seed=8), radius=radius), _frames(r, W, H), f"radius={radius}")
    if radius == np.inf:  # an infinite limit is no limit
        assert r["visibility"].tobytes() == _checked("spheres500", W, H, SPP, 4, 0.0, 8, 0)["visibility"].tobytes()


def test_a_window_that_starts_at_pass_five(hb):
    gpu, cam = _gpu(hb, "all_materials")
    ref = _frames(_checked("all_materials", W, H, 3, 4, 0.0, SEED, 5), W, H)
    assert_ao_equal(gpu.render_ao(cam, _opts(spp=3, sample_begin=5)), ref, "sample_begin=5")
    first = gpu.render_ao(cam, _opts(spp=3))
    assert first["visibility"].tobytes() != ref["visibility"].tobytes()  # other passes, other rays


@pytest.mark.parametrize("size", [(2, 2), (9, 7), (65, 37)])
def test_ragged_and_tiny_frames(hb, size):
    w, h = size
    gpu, cam = _gpu(hb, "all_materials")
    ref = _frames(_checked("all_materials", w, h, 3, 4, 0.5, 12, 4), w, h)
    assert_ao_equal(gpu.render_ao(cam, _opts(w, h, 3, seed=12, sample_begin=4), radius=0.5), ref, f"{w}x{h}")


def device_ao(torch, w, h, off=0):
    """device buffers `off` floats past an aligned base, with guard values before and after every channel"""
    return GuardedBuffers(torch, {"visibility": ((h, w), np.float32), "bent_normal": ((h, w, 3), np.float32)}, off=off)


def test_each_channel_alone_off_alignment_with_guards(hb):
    import torch
    gpu, cam = _gpu(hb, "all_materials")
    w, h = 65, 37
    ref = _frames(_checked("all_materials", w, h, 3, 4, 0.5, 12, 4), w, h)
    opts = _opts(w, h, 3, seed=12, sample_begin=4)
    for name in CHANNELS:  # the host entry: only what was asked for comes back
        got = gpu.render_ao(cam, opts, radius=0.5, channels=(name,))
        assert set(got) == {name}
        assert_same_bits(got[name], ref[name], f"host entry, {name} alone", nan_equal=True)
    for off in (0, 1, 3):  # 0, 4 and 12 bytes off a 16-byte boundary
        run = device_ao(torch, w, h, off)
        torch.cuda.synchronize()
        gpu.render_ao_device(cam, opts, run.ptrs(), radius=0.5)
        torch.cuda.synchronize()
        assert_ao_equal(run.read_all(), ref, f"device entry off={off}")
        for name, other in (CHANNELS, CHANNELS[::-1]):
            run.refill()
            torch.cuda.synchronize()
            gpu.render_ao_device(cam, opts, run.ptrs((name,)), radius=0.5)
            torch.cuda.synchronize()
            assert_same_bits(run.read(name), ref[name], f"device entry off={off}, {name} alone", nan_equal=True)
            assert run.untouched(other), f"{other} was written though not asked for"


# ---- entry points and side effects ----
def test_host_entry_device_entry_streams_and_a_multi_device_head(hb):
    import torch
    name = "spheres500"
    ref = _frames(_checked(name, W, H, SPP, 4, 1.0, 8, 0), W, H)
    opts = _opts(seed=8)
    dev = torch.device("cuda", 0)
    for what, kw in (("device=0", dict(device=0)), ("devices=[0, 0]", dict(devices=[0, 0]))):
        gpu, cam = _gpu(hb, name, **kw)
        assert_ao_equal(gpu.render_ao(cam, opts, radius=1.0), ref, f"{what} host entry")
        created = torch.cuda.Stream(device=dev)
        for stream in (0, created.cuda_stream):
            run = device_ao(torch, W, H)
            torch.cuda.synchronize()
            gpu.render_ao_device(cam, opts, run.ptrs(), radius=1.0, stream=stream)
            torch.cuda.synchronize()
            assert_ao_equal(run.read_all(), ref, f"{what} device entry, stream {'null' if stream == 0 else 'created'}")


def test_three_streams_in_flight(hb):
    import torch
    name = "all_materials"
    gpu, cam = _gpu(hb, name)
    ref = _frames(_checked(name, W, H, SPP, 4, 0.0, SEED, 0), W, H)
    dev = torch.device("cuda", 0)
    streams = [torch.cuda.Stream(device=dev) for _ in range(3)]
    runs = [device_ao(torch, W, H) for _ in streams]
    torch.cuda.synchronize()
    for _ in range(2):
        for s, run in zip(streams, runs):  # in flight together
            gpu.render_ao_device(cam, _opts(), run.ptrs(), stream=s.cuda_stream)
    torch.cuda.synchronize()
    for i, run in enumerate(runs):
        assert_ao_equal(run.read_all(), ref, f"stream {i}")


def test_graph_captured_from_the_first_call_replays_the_checkers_bytes(hb):
    """no warm-up: the first AO call of a fresh scene is the captured one"""
    import torch
    name = "all_materials"
    gpu, cam = _gpu(hb, name)
    ref = _frames(_checked(name, W, H, SPP, 4, 0.0, SEED, 0), W, H)
    dev = torch.device("cuda", 0)
    run = device_ao(torch, W, H)
    g = capture(torch, lambda stream: gpu.render_ao_device(cam, _opts(), run.ptrs(), stream=stream))
    assert all(run.untouched(name) for name in CHANNELS)  # capture ran nothing
    for _ in range(2):
        run.refill()
        torch.cuda.synchronize(dev)
        g.replay()
        torch.cuda.synchronize(dev)
        assert_ao_equal(run.read_all(), ref, "graph replay")


def test_no_side_effects_on_render(hb):
    gpu, cam = _gpu(hb, "overshadowed")
    assert_render_unaffected(gpu, cam, lambda opts, img: gpu.render_ao(cam, opts))


# ---- properties ----
def test_a_smaller_radius_never_lowers_the_visibility_on_the_gpu(hb):
    gpu, cam = _gpu(hb, "spheres500")
    frames = [gpu.render_ao(cam, _opts(seed=8), radius=r, channels=("visibility",))["visibility"] for r in (np.inf, 4.0, 1.0, 0.25, 0.0625)]
    for wide, narrow in zip(frames, frames[1:]):
        assert (narrow >= wide).all()
    assert frames[-1].mean() > frames[0].mean()  # and raises it somewhere


def test_the_rays_of_a_pass_are_the_same_for_every_k(hb):
    """one pass, K = 1 .. 4: ray k is the same ray whatever K, so the unoccluded count at K is the checker's count over the first
    K of its four rays"""
    name = "spheres500"
    gpu, cam = _gpu(hb, name)
    four = _checked(name, W, H, 1, 4, 0.0, 8, 0)
    hit = four["hits"] == 1
    assert hit.sum() > 100
    for k in (1, 2, 3, 4):
        got = gpu.render_ao(cam, _opts(spp=1, seed=8), rays_per_pass=k)
        assert_ao_equal(got, _frames(_checked(name, W, H, 1, k, 0.0, 8, 0), W, H), f"K={k}")
        open_first_k = four["open"][:, 0, :k].sum(axis=1)
        expected = np.where(hit, open_first_k.astype(np.float32) / F32(k), F32(1.0)).astype(np.float32)
        assert_same_bits(got["visibility"].reshape(-1), expected, f"K={k}: the first {k} of four rays", nan_equal=True)


# ---- full size ----
def test_tiles_of_a_1080p_frame(hb):
    name = "all_materials"
    sc, _, cpu, cam_c = _built(name)
    gpu, cam = _gpu(hb, name)
    w, h, spp, rays = 1920, 1080, 1, 2
    opts = _opts(w, h, spp, seed=1)
    got = gpu.render_ao(cam, opts, rays_per_pass=rays)
    material = gpu.render_aov(cam, opts, channels=("material",))["material"]
    tiles = [(0, 0), (w // 8 - 1, h // 8 - 1)]
    for mat_type in (abi.RT_MAT_REFLECT, abi.RT_MAT_REFRACT):  # four tiles each on the mirror ball and on the glass ball
        index = [i for i, m in enumerate(sc.materials) if m.type == mat_type]
        seen = np.argwhere(np.isin(material, index))
        assert len(seen) > 1000, mat_type
        for y, x in seen[:: len(seen) // 4][:4]:
            tiles.append((int(x) // 8, int(y) // 8))
    rng = np.random.default_rng(0)
    while len(set(tiles)) < 12:
        tiles.append((int(rng.integers(0, w // 8)), int(rng.integers(0, h // 8))))
    pixels = K.tile_pixels(w, h, sorted(set(tiles)))
    ref = A.ao(cpu, cam_c, w, h, spp, rays, seed=1, pixels=pixels)
    assert 0.05 <= _shares(ref)[1] <= 0.95
    assert_same_bits(got["visibility"].reshape(-1)[pixels], ref["visibility"], "1080p tiles visibility", nan_equal=True)
    assert_same_bits(got["bent_normal"].reshape(-1, 3)[pixels], ref["bent_normal"], "1080p tiles bent_normal", nan_equal=True)
    assert np.isfinite(got["visibility"]).all() and got["visibility"].min() >= 0.0 and got["visibility"].max() <= 1.0
