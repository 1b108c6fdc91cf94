"""First-hit AOV buffers (rt_render_aov) on the GPU against the CPU checker (tests/aov_checker.py): every comparison is
bit-exact (NaN == NaN)."""
import itertools

import numpy as np
import pytest

import aov_checker as K
import scenes
from gpu_support import GuardedBuffers, assert_render_unaffected, assert_same_bits, ssml_scene

pytestmark = pytest.mark.gpu
abi = scenes.abi
W, H, SPP = 64, 36, 16


def _lambertian_sky():
    """every texture type on the primitives, and a sky whose material is a Lambertian over a point-dependent texture"""
    sc = scenes.all_materials()
    sc.set_sky(sc.checkered((0.8, 0.7, 0.3), (0.2, 0.4, 0.9)), (0, 0), material=sc.lambertian(sc.lerp((0.9, 0.9, 0.9), (0.2, 0.3, 0.5)), 0.6))
    return sc, scenes.ALL_MATERIALS_CAMERA


SCENES = {
    "rtweekend1": lambda: ssml_scene("rtweekend1"),
    "overshadowed": lambda: ssml_scene("overshadowed"),
    "pyramid": lambda: ssml_scene("pyramid"),
    "all_materials": lambda: (scenes.all_materials(), scenes.ALL_MATERIALS_CAMERA),
    "structured_meshes": lambda: (scenes.structured_meshes(), scenes.STRUCTURED_CAMERA),
    "mesh50k": lambda: (scenes.random_triangle_mesh(50_000), scenes.MESH_CAMERA),
    "lambertian_sky": _lambertian_sky,
}
SCENES.update({f"random_everything_{seed}": (lambda seed=seed: scenes.random_everything(seed)) for seed in range(12)})


def assert_aovs_equal(gpu, ref, what):
    for name in ref:
        assert_same_bits(gpu[name], ref[name], f"{what} {name}", nan_equal=True)


def _reference(sc, cpu, cam, w, h, spp, seed, sample_begin, pixels=None):
    r = K.aovs(sc, cpu, cam, w, h, spp, seed=seed, sample_begin=sample_begin, pixels=pixels)
    if pixels is None:
        r = {k: v.reshape((h, w, 3) if v.ndim == 2 else (h, w)) for k, v in r.items()}
    return r


@pytest.mark.parametrize("name", list(SCENES))
def test_aovs_match_the_checker(hb, O, name):
    sc, cam_params = SCENES[name]()
    gpu, cpu = hb.HipScene(sc, device=0), O.Scene(sc)
    cam_g, cam_c = hb.camera_new(**cam_params), O.camera_new(**cam_params)
    for sample_begin in (0, 5):
        opts = abi.default_render_opts(W, H, SPP, seed=3)
        opts.sample_begin = sample_begin
        ref = _reference(sc, cpu, cam_c, W, H, SPP, 3, sample_begin)
        got = gpu.render_aov(cam_g, opts)
        assert_aovs_equal(got, ref, f"{name} sample_begin={sample_begin} auto traversal")
        for mode in (0, 1):  # forced exhaustive / pruned: the same bytes
            gpu.set_traversal(mode)
            assert_aovs_equal(gpu.render_aov(cam_g, opts), ref, f"{name} sample_begin={sample_begin} traversal={mode}")
        gpu.set_traversal(-1)
    # the buffers say something: some passes hit, and (but for scenes seen whole) some miss
    assert ref["coverage"].max() > 0.0


def test_every_channel_subset_gives_the_same_bytes(hb):
    sc, cam_params = _lambertian_sky()
    gpu = hb.HipScene(sc, device=0)
    cam = hb.camera_new(**cam_params)
    opts = abi.default_render_opts(W, H, 4, seed=9)
    full = gpu.render_aov(cam, opts)
    for k in range(1, len(abi.AOV_CHANNELS)):
        for subset in itertools.combinations(abi.AOV_CHANNELS, k):
            got = gpu.render_aov(cam, opts, channels=subset)
            assert set(got) == set(subset)
            for name in subset:
                assert_same_bits(got[name], full[name], f"subset {subset} {name}", nan_equal=True)


def test_device_entry_point_on_a_side_stream(hb):
    import torch
    sc, cam_params = SCENES["all_materials"]()
    gpu = hb.HipScene(sc, device=0)
    cam = hb.camera_new(**cam_params)
    opts = abi.default_render_opts(W, H, SPP, seed=4)
    opts.sample_begin = 3
    ref = gpu.render_aov(cam, opts)
    dev = torch.device("cuda", 0)
    run = GuardedBuffers(torch, {name: (ref[name].shape, ref[name].dtype.type) for name in abi.AOV_CHANNELS})
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        gpu.render_aov_device(cam, opts, run.ptrs(), stream=side.cuda_stream)
    side.synchronize()
    for name in abi.AOV_CHANNELS:
        assert_same_bits(run.read(name), ref[name], f"device entry point {name}", nan_equal=True)


def test_no_side_effects_on_render(hb):
    sc, cam_params = SCENES["overshadowed"]()
    gpu = hb.HipScene(sc, device=0)
    cam = hb.camera_new(**cam_params)
    assert_render_unaffected(gpu, cam, lambda opts, img: gpu.render_aov(cam, opts))


def test_multi_device_head_scene(hb):
    sc, cam_params = SCENES["random_everything_3"]()
    single, multi = hb.HipScene(sc, device=0), hb.HipScene(sc, devices=[0, 0])
    cam = hb.camera_new(**cam_params)
    opts = abi.default_render_opts(W, H, SPP, seed=6)
    assert_aovs_equal(multi.render_aov(cam, opts), single.render_aov(cam, opts), "devices=[0, 0]")


def test_albedo_equals_the_render_of_an_all_emit_scene(hb):
    """the product path itself: one naive pass of an all-Emit(1.0) scene renders the texture colour of each primary ray"""
    sc = K.emit_scene()
    gpu = hb.HipScene(sc, device=0)
    cam = hb.camera_new(**K.EMIT_CAMERA)
    for sample_begin in (0, 11):
        opts = abi.default_render_opts(W, H, 1, method=abi.RT_METHOD_NAIVE, seed=8)
        opts.sample_begin = sample_begin
        opts.sample_split = 1
        img, _ = gpu.render(cam, opts)
        assert_same_bits(gpu.render_aov(cam, opts, channels=("albedo",))["albedo"], img, f"sample_begin={sample_begin}", nan_equal=True)


def test_full_frame_rtweekend1(hb, O):
    sc, cam_params = SCENES["rtweekend1"]()
    gpu, cpu = hb.HipScene(sc, device=0), O.Scene(sc)
    w, h, spp = 1920, 1080, 4
    opts = abi.default_render_opts(w, h, spp, seed=1)
    got = gpu.render_aov(hb.camera_new(**cam_params), opts)
    tiles_x, tiles_y = w // 8, h // 8
    rng = np.random.default_rng(0)
    tiles = {(0, 0), (tiles_x - 1, tiles_y - 1), (0, tiles_y - 1), (tiles_x - 1, 0)}
    while len(tiles) < 72:
        tiles.add((int(rng.integers(0, tiles_x)), int(rng.integers(0, tiles_y))))
    pixels = K.tile_pixels(w, h, sorted(tiles))
    ref = _reference(sc, cpu, O.camera_new(**cam_params), w, h, spp, 1, 0, pixels=pixels)
    flat = {k: v.reshape(w * h, -1) if v.ndim == 3 else v.reshape(w * h) for k, v in got.items()}
    for name in ref:
        assert_same_bits(flat[name][pixels], ref[name], f"1080p tiles {name}", nan_equal=True)
    for name in ("albedo", "normal", "depth", "coverage"):
        assert np.isfinite(got[name]).all(), name
    assert ((got["coverage"] >= 0) & (got["coverage"] <= 1)).all()
    n_prims, n_mats = gpu.counts()[1], len(sc.materials)
    assert ((got["primitive"] < n_prims) | (got["primitive"] == abi.AOV_NO_ID)).all()
    assert ((got["material"] < n_mats) | (got["material"] == abi.AOV_NO_ID)).all()
    assert ((got["primitive"] == abi.AOV_NO_ID) == (got["material"] == abi.AOV_NO_ID)).all()
