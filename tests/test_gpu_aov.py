"""First-hit AOV buffers (rt_render_aov) on the GPU against the CPU checker (tests/aov_checker.py): every comparison is
bit-exact (NaN == NaN)."""
import itertools

import numpy as np
import pytest

import aov_checker as K
import scenes

pytestmark = pytest.mark.gpu
abi = scenes.abi
W, H, SPP = 64, 36, 16


def _lambertian_sky():
    """every texture type on the primitives, and a sky whose material is a Lambertian over a point-dependent texture"""
    sc = scenes.all_materials()
    sc.set_sky(sc.checkered((0.8, 0.7, 0.3), (0.2, 0.4, 0.9)), (0, 0), material=sc.lambertian(sc.lerp((0.9, 0.9, 0.9), (0.2, 0.3, 0.5)), 0.6))
    return sc, scenes.ALL_MATERIALS_CAMERA


def _ssml(name):
    ls = scenes.load_ssml(name)
    return ls.scene, ls.camera_params


SCENES = {
    "rtweekend1": lambda: _ssml("rtweekend1"),
    "overshadowed": lambda: _ssml("overshadowed"),
    "pyramid": lambda: _ssml("pyramid"),
    "all_materials": lambda: (scenes.all_materials(), scenes.ALL_MATERIALS_CAMERA),
    "structured_meshes": lambda: (scenes.structured_meshes(), scenes.STRUCTURED_CAMERA),
    "mesh50k": lambda: (scenes.random_triangle_mesh(50_000), scenes.MESH_CAMERA),
    "lambertian_sky": _lambertian_sky,
}
SCENES.update({f"random_everything_{seed}": (lambda seed=seed: scenes.random_everything(seed)) for seed in range(12)})


def assert_same(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    if a.dtype == np.float32:  # bits, but any NaN equals any NaN
        same = (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))
    else:
        same = a == b
    if not same.all():
        bad = np.argwhere(~same)
        pytest.fail(f"{what}: {len(bad)} elements differ, first at {bad[0].tolist()}: gpu {a[tuple(bad[0])]!r} checker {b[tuple(bad[0])]!r}")


def assert_aovs_equal(gpu, ref, what):
    for name in ref:
        assert_same(gpu[name], ref[name], f"{what} {name}")


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
                assert_same(got[name], full[name], f"subset {subset} {name}")


def test_device_entry_point_on_a_side_stream(hb):
    import torch
    sc, cam_params = SCENES["all_materials"]()
    gpu = hb.HipScene(sc, device=0)
    cam = hb.camera_new(**cam_params)
    opts = abi.default_render_opts(W, H, SPP, seed=4)
    opts.sample_begin = 3
    ref = gpu.render_aov(cam, opts)
    dev = torch.device("cuda", 0)
    t = {name: torch.full(ref[name].shape, 7, dtype=torch.int32 if ref[name].dtype == np.uint32 else torch.float32, device=dev)
         for name in abi.AOV_CHANNELS}
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        gpu.render_aov_device(cam, opts, {name: t[name].data_ptr() for name in abi.AOV_CHANNELS}, stream=side.cuda_stream)
    side.synchronize()
    for name in abi.AOV_CHANNELS:
        got = t[name].cpu().numpy()
        if ref[name].dtype == np.uint32:
            got = got.view(np.uint32)
        assert_same(got, ref[name], f"device entry point {name}")


def test_no_side_effects_on_render(hb):
    sc, cam_params = SCENES["overshadowed"]()
    gpu = hb.HipScene(sc, device=0)
    cam = hb.camera_new(**cam_params)
    opts = abi.default_render_opts(96, 54, 8, method=abi.RT_METHOD_MIS, seed=2)
    img_a, rays_a = gpu.render(cam, opts)
    n_a = gpu.last_kernel_ms()[1]
    info_a = gpu.last_launch_info()
    gpu.render_aov(cam, opts)
    assert gpu.last_kernel_ms()[1] == n_a and gpu.last_launch_info() == info_a  # still describe the render
    img_b, rays_b = gpu.render(cam, opts)
    assert np.array_equal(img_a, img_b) and rays_a == rays_b
    assert gpu.last_kernel_ms()[1] == n_a and gpu.last_launch_info() == info_a


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
        assert_same(gpu.render_aov(cam, opts, channels=("albedo",))["albedo"], img, f"sample_begin={sample_begin}")


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
        assert_same(flat[name][pixels], ref[name], f"1080p tiles {name}")
    for name in ("albedo", "normal", "depth", "coverage"):
        assert np.isfinite(got[name]).all(), name
    assert ((got["coverage"] >= 0) & (got["coverage"] <= 1)).all()
    n_prims, n_mats = gpu.counts()[1], len(sc.materials)
    assert ((got["primitive"] < n_prims) | (got["primitive"] == abi.AOV_NO_ID)).all()
    assert ((got["material"] < n_mats) | (got["material"] == abi.AOV_NO_ID)).all()
    assert ((got["primitive"] == abi.AOV_NO_ID) == (got["material"] == abi.AOV_NO_ID)).all()
